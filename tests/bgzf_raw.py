"""Shared by tests/test_gpu_bgzf.py and tests/soak_bgzf.py: one raw sk_bgzf_device_async + finish on a sentinel-filled
image buffer, and a walk over the members of an image."""
import ctypes as C
import struct

import numpy as np

from sickle_amd import capi

SENTINEL = 0xAB
BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def torch_mod():
    import torch
    return torch


def to_device(data):
    return torch_mod().from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def upload(text, shift=0, room=0):
    """text (bytes) on the device at an address `shift` bytes past a 16-byte boundary, `room` spare bytes behind it."""
    torch = torch_mod()
    buf = torch.zeros(len(text) + room + shift + 16, dtype=torch.uint8, device="cuda")
    if len(text):
        buf[shift:shift + len(text)] = to_device(text)
    return buf, buf.data_ptr() + shift


def word(value):
    torch = torch_mod()
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def raw(ctx, text, eof, shift=0, bound=None, dev_len=None, valid=None, capacity=None):
    """One async + finish on raw pointers, `out` pre-filled with SENTINEL.  bound: what in->bytes says (default: the
    length); dev_len / valid: the values of the device words, None = no such word.  -> (rc, counts, out tensor)."""
    torch = torch_mod()
    L = capi.lib()
    nbytes = len(text) if bound is None else bound
    keep, ptr = upload(text, shift, room=nbytes - len(text))
    flags = capi.SK_BGZF_EOF if eof else 0
    cap = L.sk_bgzf_bound(nbytes, flags) if capacity is None else capacity
    out = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws_bytes = L.sk_bgzf_workspace_bytes(nbytes)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    wl, wv = None if dev_len is None else word(dev_len), None if valid is None else word(valid)
    inp = capi.BgzfInput(ptr, nbytes, None if wl is None else wl.data_ptr(), None if wv is None else wv.data_ptr())
    rc = L.sk_bgzf_device_async(ctx._h, C.byref(inp), out.data_ptr(), cap, flags, ws.data_ptr(), ws_bytes, None)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    c = capi.BgzfCounts()
    rc = L.sk_bgzf_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
    del keep
    return rc, c.as_dict(), out


def image_of(out, counts):
    n = counts["bytes_out"]
    assert bool((out[n:] == SENTINEL).all()), "bytes of out past bytes_out were written"
    return out[:n].cpu().numpy().tobytes()


def walk(image):
    """Steps over the members by their BSIZE fields -> their count; must land exactly on the end."""
    at = members = 0
    while at < len(image):
        assert image[at:at + 16] == EOF[:16], at
        at += struct.unpack_from("<H", image, at + 16)[0] + 1
        members += 1
    assert at == len(image)
    return members
