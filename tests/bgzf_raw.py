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


HOSTILE_LEAD, HOSTILE_TAIL = 256, 4096


def hostile_image():
    """a complete valid gzip member of the word HOSTILE: what lies around an image whose reader must not look there"""
    import zlib
    body = zlib.compressobj(6, zlib.DEFLATED, -15)
    data = body.compress(b"HOSTILE") + body.flush()
    return bytes.fromhex("1f8b08000000000000ff") + data + struct.pack("<II", zlib.crc32(b"HOSTILE"), 7)


def surrounded(data, shift, room, surround):
    """data on the device `shift` bytes past a 16-byte boundary with HOSTILE_LEAD bytes in front of it and HOSTILE_TAIL
    behind it (and behind `room`), all a repetition of `surround`, which also fills `room` -> (tensor, address)"""
    lead = HOSTILE_LEAD + shift
    total = lead + len(data) + room + HOSTILE_TAIL
    fill = (surround * (total // len(surround) + 1))[:total]
    buf = to_device(fill[:lead] + data + fill[lead + len(data):])
    assert buf.data_ptr() % 16 == 0 and HOSTILE_LEAD % 16 == 0
    return buf, buf.data_ptr() + lead


def upload(text, shift=0, room=0, surround=None):
    """text (bytes) on the device at an address `shift` bytes past a 16-byte boundary, `room` spare bytes behind it.
    surround: None = zeros around the text, else bytes that are repeated around it (surrounded)."""
    torch = torch_mod()
    if surround is not None:
        return surrounded(text, shift, room, surround)
    buf = torch.zeros(len(text) + room + shift + 16, dtype=torch.uint8, device="cuda")
    if len(text):
        buf[shift:shift + len(text)] = to_device(text)
    return buf, buf.data_ptr() + shift


def word(value):
    torch = torch_mod()
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def raw(ctx, text, eof, shift=0, bound=None, dev_len=None, valid=None, capacity=None, ws=None, surround=None):
    """One async + finish on raw pointers, `out` pre-filled with SENTINEL.  bound: what in->bytes says (default: the
    length); dev_len / valid: the values of the device words, None = no such word.  ws: the workspace tensor, used as it
    is (the byte count handed to the library stays the formula's).  -> (rc, counts, out tensor)."""
    torch = torch_mod()
    L = capi.lib()
    nbytes = len(text) if bound is None else bound
    keep, ptr = upload(text, shift, room=nbytes - len(text), surround=surround)
    flags = capi.SK_BGZF_EOF if eof else 0
    cap = L.sk_bgzf_bound(nbytes, flags) if capacity is None else capacity
    out = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws_bytes = L.sk_bgzf_workspace_bytes(nbytes)
    if ws is None:
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
