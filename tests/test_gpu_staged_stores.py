"""The staged uniform kernels' cut stores (write-through, through a buffer descriptor of each tile's rows) on the
device-resident path -- the only one on which the caller chooses `out`: `out` on a 16-byte boundary and 8 bytes past
one, nothing written outside it, visible to the next kernel on the stream.  Every result is compared with the oracle."""
import functools

import numpy as np
import pytest

import oracle_bind as ob
from sickle_amd import capi, synth

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A  # no cut is this value (cuts lie in [-2, read length])
PAD = 64               # int32 words of sentinel on each side of `out` (256 bytes: a 16-byte boundary)
ROUND = 12 * 256 * 64  # reads one round of the staged grid takes: 12 waves x 256 CUs x 64 reads
COUNTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 2 * ROUND + 37)
STRIDES = (72, 104, 152, 160)  # STAGE 5, 7, 10, 10


def read_len(stride):
    # as test_register_staged_tiles picks them: a length whose rows have this stride
    return 70 if stride == 72 else stride - int(np.random.default_rng(stride).integers(0, 8))


@functools.lru_cache(maxsize=None)
def case(stride, n, salt=0):
    """(params, packed quals, oracle cuts) of one batch; computed once, shared by the tests, never written to"""
    L = read_len(stride)
    rng = np.random.default_rng(31 * stride + n + 1000003 * salt)
    qt = ("sanger", "illumina", "solexa")[(stride // 8 + n + salt) % 3]
    lo, hi = {"sanger": (33, 74), "solexa": (59, 105), "illumina": (64, 105)}[qt]
    mid = int(rng.integers(lo + 14, hi - 6))
    qual = np.clip(mid + rng.integers(-16, 17, size=(n, L), dtype=np.int16), lo, hi).astype(np.uint8)
    drop = rng.integers(0, L + 1, size=n)
    qual[np.arange(L)[None, :] >= drop[:, None]] = lo + 1
    qs = synth.pack_fixed(qual, stride)
    # a threshold a little under the reads' middle quality and a length threshold of a quarter to half a read: reads are
    # cut where their quality drops, the ones that drop early are discarded
    base = 33 if qt == "sanger" else 64
    q, l, x = min(41, max(1, mid - base - 8)), int(rng.integers(L // 4, L // 2)), int(rng.integers(0, 2))
    want, err = ob.oracle_trim_batch(ob.make_params(qt, q, l, x, 0), qs, None, stride=stride, read_len=L, n_reads=n, threads=4)
    assert err is None
    if n >= 63:  # the batch is a real mix (a statement about the test's data: `want` is the oracle's)
        kept = want[:, 1] >= 0
        assert kept.any() and (~kept).any() and np.unique(want[kept, 1]).size >= 4, (stride, n, qt, q, l, x)
    want.setflags(write=False)
    return (qt, q, l, x), qs, want


def framed_out(torch, dev, n, shift_bytes):
    """`out` for n cuts as a view into a larger int32 tensor of sentinels: `shift_bytes` past a 16-byte boundary"""
    big = torch.full((PAD + 2 * n + PAD + 4,), SENTINEL, dtype=torch.int32, device=dev)
    start = PAD + shift_bytes // 4
    ptr = big.data_ptr() + 4 * start
    assert big.data_ptr() % 16 == 0 and ptr % 16 == shift_bytes
    return big, start, ptr


def check_frame(big, start, n, want, what):
    host = big.cpu().numpy()
    assert (host[:start] == SENTINEL).all(), (what, "words before out[0] were written", np.nonzero(host[:start] != SENTINEL)[0][:8])
    tail = host[start + 2 * n:]
    assert tail.size >= PAD and (tail == SENTINEL).all(), (what, "words after out[n-1] were written", np.nonzero(tail != SENTINEL)[0][:8])
    got = host[start:start + 2 * n].reshape(n, 2)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (what, bad[:6], got[bad[:6]], want[bad[:6]])


@pytest.mark.parametrize("shift_bytes", (0, 8))
@pytest.mark.parametrize("stride", STRIDES)
def test_cuts_and_frame_on_any_out_alignment(sk_ctx, stride, shift_bytes):
    """Every read count around the tile boundaries, odd and even, and one of several tiles per wave ending in a ragged
    tile with an odd row count: the oracle's cuts, and not a word written outside out[0 .. n-1]."""
    import torch
    dev = torch.device("cuda", 0)
    L = read_len(stride)
    b = capi.Batch(0, None, None, stride, L, None, 10)
    assert capi.lib().sk_kernel_for(b) == 4, stride  # the register-staged kernel
    s = torch.cuda.Stream(dev)
    for n in COUNTS:
        (qt, q, l, x), qs, want = case(stride, n)
        qd = torch.from_numpy(qs).to(dev)
        big, start, ptr = framed_out(torch, dev, n, shift_bytes)
        torch.cuda.synchronize(dev)
        sk_ctx.scan_device_async(capi.make_params(qt, q, l, x, 0), qd.data_ptr(), ptr, n, stride=stride, read_len=L, stream=s.cuda_stream)
        sk_ctx.scan_device_finish(s.cuda_stream)
        check_frame(big, start, n, want, (stride, L, n, shift_bytes))


@pytest.mark.parametrize("shift_bytes", (8, 0))
def test_range_errors_last_full_tile_and_ragged_tail(sk_ctx, shift_bytes):
    """A bad char in the last full tile of a long batch and one in its ragged tail: the reference's (read, position, char)."""
    import torch
    dev = torch.device("cuda", 0)
    n, stride, L = 2 * ROUND + 37, 152, 150
    qs = np.full((n, stride), 75, dtype=np.uint8)
    po = ob.make_params("sanger", 20, 20, 0, 0)
    s = torch.cuda.Stream(dev)
    big, start, ptr = framed_out(torch, dev, n, shift_bytes)
    qd = torch.from_numpy(qs.reshape(-1)).to(dev)
    # both planted: the one in the last full tile comes first; then the tail's alone
    for plant in (((n - 3, 5, 20), (n - 70, 149, 31)), ((n - 3, 5, 20),)):
        qd.view(n, stride)[:, :L] = 75
        host = qs.copy()
        for read, pos, ch in plant:
            qd.view(n, stride)[read, pos] = ch
            host[read, pos] = ch
        _, want_err = ob.oracle_trim_batch(po, host.reshape(-1), None, stride=stride, read_len=L, n_reads=n)
        assert want_err == min(plant), want_err
        torch.cuda.synchronize(dev)
        sk_ctx.scan_device_async(capi.make_params("sanger", 20, 20, 0, 0), qd.data_ptr(), ptr, n, stride=stride, read_len=L, stream=s.cuda_stream)
        with pytest.raises(capi.RangeError) as ei:
            sk_ctx.scan_device_finish(s.cuda_stream)
        assert (ei.value.read, ei.value.pos, ei.value.ch) == want_err
    host = big.cpu().numpy()
    assert (host[:start] == SENTINEL).all() and (host[start + 2 * n:] == SENTINEL).all()


@pytest.mark.parametrize("shift_bytes", (0, 8))
def test_next_kernel_on_the_stream_sees_the_cuts(sk_ctx, shift_bytes):
    """Two scans queued back to back into one `out` over different inputs, then a torch reduction on the same stream
    with no host wait in between: it must see the second scan's cuts (write-through stores are visible to the next
    kernel like any others)."""
    import torch
    dev = torch.device("cuda", 0)
    stride, n = 152, 2 * ROUND + 37
    L = read_len(stride)
    p1, qs1, want1 = case(stride, n)
    p2, qs2, want2 = case(stride, n, salt=1)
    assert (want1 != want2).any() and int(want1.astype(np.int64).sum()) != int(want2.astype(np.int64).sum())
    q1, q2 = torch.from_numpy(qs1).to(dev), torch.from_numpy(qs2).to(dev)
    big, start, ptr = framed_out(torch, dev, n, shift_bytes)
    s = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    sk_ctx.scan_device_async(capi.make_params(*p1, 0), q1.data_ptr(), ptr, n, stride=stride, read_len=L, stream=s.cuda_stream)
    sk_ctx.scan_device_async(capi.make_params(*p2, 0), q2.data_ptr(), ptr, n, stride=stride, read_len=L, stream=s.cuda_stream)
    with torch.cuda.stream(s):
        view = big[start:start + 2 * n]
        total = view.sum(dtype=torch.int64)
        kept = (view.view(n, 2)[:, 1] >= 0).sum()
    sk_ctx.scan_device_finish(s.cuda_stream)
    assert int(total.item()) == int(want2.astype(np.int64).sum())
    assert int(kept.item()) == int((want2[:, 1] >= 0).sum())
    check_frame(big, start, n, want2, ("back to back", shift_bytes))
