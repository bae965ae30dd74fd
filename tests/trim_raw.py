"""Shared by tests/test_gpu_trim.py and tests/soak_trim.py: numpy <-> device, and the canary-filled output buffers of a raw
sk_trim_device_async call."""
import numpy as np

from sickle_amd import capi


def torch_mod():
    import torch
    return torch


def dev(a):
    torch = torch_mod()
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def host(t):
    return None if t is None else t.cpu().numpy()


class Raw:
    """Device buffers for the three outputs of a raw sk_trim_device_async call, filled with a canary."""
    CANARY = 0xA5
    WORD = -0x5a5a5a5a

    def __init__(self, recs, nbytes, seq=True, index=True):
        torch = torch_mod()
        self.t = []
        self.outs = []
        for o in range(3):
            q = torch.full((nbytes[o] + 16,), self.CANARY, dtype=torch.uint8, device="cuda")
            s = torch.full((nbytes[o] + 16,), self.CANARY, dtype=torch.uint8, device="cuda") if seq else None
            off = torch.full((recs[o] + 2,), self.WORD, dtype=torch.int64, device="cuda")
            idx = torch.full((recs[o] + 1,), self.WORD, dtype=torch.int64, device="cuda") if index else None
            self.t.append((q, s, off, idx))
            self.outs.append(capi.TrimOutput(q.data_ptr(), None if s is None else s.data_ptr(), off.data_ptr(),
                                             None if idx is None else idx.data_ptr(), nbytes[o], recs[o]))

    def untouched(self, o):
        q, s, off, idx = self.t[o]
        ok = bool((q == self.CANARY).all()) and bool((off == self.WORD).all())
        ok = ok and (idx is None or bool((idx == self.WORD).all()))
        return ok and (s is None or bool((s == self.CANARY).all()))

    def canaries_intact(self, o, records, nbytes):
        """The canary behind the last byte and the last record of output o, which holds `records` and `nbytes`."""
        q, s, off, idx = self.t[o]
        ok = bool((q[nbytes:] == self.CANARY).all()) and bool((off[records + 1:] == self.WORD).all())
        ok = ok and (idx is None or bool((idx[records:] == self.WORD).all()))
        return ok and (s is None or bool((s[nbytes:] == self.CANARY).all()))


def raw_call(ctx, qual_t, seq_t, off_t, cuts_t, n, outs, mode, ws=None, stream=None):
    torch = torch_mod()
    nb = capi.lib().sk_trim_workspace_bytes(n)
    if ws is None:
        ws = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    return ctx.trim_device(cuts_t.data_ptr(), n, outs, ws.data_ptr(), nb, mode=mode, stream=stream,
                           qual_ptr=qual_t.data_ptr(), seq_ptr=None if seq_t is None else seq_t.data_ptr(),
                           offsets_ptr=off_t.data_ptr())
