"""Shared by tests/test_gpu_fastq.py and tests/soak_fastq.py: one raw sk_trim_fastq_device_async + finish on sentinel-filled
outputs, and the comparison of such a call with the numpy model of tests/fastq_model.py."""
import ctypes as C

import numpy as np

import fastq_model as fm
from sickle_amd import capi

SENTINEL = 0xAB


def torch_mod():
    import torch
    return torch


HOSTILE_TEXT = b"\n@x\nACGT\n+\nIIII\n"  # records that an over-read would find around a text


def upload(text, shift=0, surround=None):
    """text (bytes) on the device at an address that is `shift` bytes past a 16-byte boundary.  surround: None = zeros
    around the text, else bytes repeated in the 256 bytes before and the 4096 bytes behind it (bgzf_raw.surrounded)."""
    torch = torch_mod()
    if surround is not None:
        import bgzf_raw
        return bgzf_raw.surrounded(text, shift, 0, surround)
    buf = torch.zeros(len(text) + shift + 16, dtype=torch.uint8, device="cuda")
    if len(text):
        buf[shift:shift + len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    return buf, buf.data_ptr() + shift


def raw(ctx, params, texts, mode, caps=None, rec_caps=None, shift=0, max_read_len=0, index=True, ws=None, stream=None,
        finish=True, room=0, surround=None):
    """One async + finish on raw pointers, every output pre-filled with SENTINEL.  caps / rec_caps: per output (None =
    what the model says plus a little); room: sentinel bytes / entries behind every output's capacity; surround: what
    lies around the texts (upload).  -> (rc, counts, [bytes or None], [index arrays or None])."""
    torch = torch_mod()
    bufs = [upload(t, shift, surround) for t in texts]
    T = sum(len(t) for t in texts)
    ws_bytes = capi.lib().sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    caps = caps or [T + 64] * 3
    rec_caps = rec_caps or [T // 4 + 4] * 3
    outs, keep = [], []
    for o in range(3):
        if caps[o] is None:
            outs.append(capi.FastqOutput())
            keep.append(None)
            continue
        t = torch.full((max(caps[o], 16) + room,), SENTINEL, dtype=torch.uint8, device="cuda")
        ix = torch.full((max(rec_caps[o], 1) + room,), -7, dtype=torch.int64, device="cuda") if index else None
        outs.append(capi.FastqOutput(t.data_ptr(), caps[o], ix.data_ptr() if index else None, rec_caps[o]))
        keep.append((t, ix))
    inp = capi.FastqInput((C.c_void_p * 2)(*([b[1] for b in bufs] + [None] * (2 - len(bufs)))),
                          (C.c_uint64 * 2)(*([len(t) for t in texts] + [0] * (2 - len(texts)))), max_read_len)
    arr = (capi.FastqOutput * 3)(*outs)
    L = capi.lib()
    rc = L.sk_trim_fastq_device_async(ctx._h, C.byref(params), C.byref(inp), capi.TRIM_MODES[mode], arr, ws.data_ptr(),
                                      ws_bytes, stream)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    if not finish:
        return ws, keep, bufs
    c = capi.FastqCounts()
    rc = L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), stream, C.byref(c))
    return rc, c.as_dict(), keep


def texts_of(keep, counts):
    return [None if k is None else k[0][:counts["bytes"][o]].cpu().numpy().tobytes() for o, k in enumerate(keep)]


def untouched(keep):
    for k in keep:
        if k is not None:
            assert bool((k[0] == SENTINEL).all()), "an output was written after an error"
            if k[1] is not None:
                assert bool((k[1] == -7).all())


def check(ctx, ptuple, texts, mode, **kw):
    """The device against the model: verdict, range error or every output text, index and count."""
    want = fm.expected(ptuple, texts, mode)
    rc, counts, keep = raw(ctx, capi.make_params(*ptuple), texts, mode, **kw)
    assert counts["records_in"] == want["records_in"] and counts["tail_lines"] == want["tail_lines"]
    assert counts["dropped_unpaired"] == want["dropped_unpaired"]
    if want["verdict"] is not None:
        assert rc == capi.SK_EFORMAT
        assert (counts["format_error"], counts["format_input"], counts["format_record"]) == want["verdict"]
        untouched(keep)
        return rc, counts, None
    if want["range"] is not None:
        assert rc == capi.SK_ERANGE
        assert counts["range"] == tuple(want["range"])
        untouched(keep)
        return rc, counts, None
    assert rc == capi.SK_OK, capi.lib().sk_last_error(ctx._h)
    got = texts_of(keep, counts)
    for o in range(3):
        if o not in fm.USED[mode]:
            continue
        assert got[o] == want["texts"][o], "output %d" % o
        assert counts["records"][o] == len(want["index"][o]) and counts["bytes"][o] == len(want["texts"][o])
        if keep[o][1] is not None:
            assert np.array_equal(keep[o][1][:counts["records"][o]].cpu().numpy(), want["index"][o])
    return rc, counts, got
