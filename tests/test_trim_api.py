"""CPU: the device-side trim of include/sickle_amd.h (sk_trim_*): the symbols, the workspace bound, the argument checks
that need no device, and the numpy model the GPU tests compare against, pinned to the reference runs."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import cli_util as cu
import trim_model as tm
from sickle_amd import capi


def test_trim_symbols_exported():
    L = capi.lib()
    for name in ("sk_trim_workspace_bytes", "sk_trim_device_async", "sk_trim_device_finish"):
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.sk_abi_version() == 2
    assert capi.SK_ESPACE == -5


def test_workspace_bytes_monotone_and_bounded():
    ws = capi.lib().sk_trim_workspace_bytes
    ns = [0, 1, 2, 3, 1000, 2047, 2048, 2049, 4096, 65535, 1 << 20, 10_000_000, 10_000_001, 1 << 32]
    sizes = [ws(n) for n in ns]
    assert sizes == sorted(sizes)
    for n, b in zip(ns, sizes):
        # the header's bound: 128 + 64 * ceil(n / 2048) + 8 n, below 8.04 bytes per read + 192 bytes
        assert b == 128 + 64 * ((n + 2047) // 2048) + 8 * n
        assert b <= 8.04 * n + 192
    for n in range(0, 5000, 7):
        assert ws(n) <= ws(n + 1)


def _batch(n=4, tiles=None):
    return capi.Batch(0x1000, None, 0x2000, 0, 0, None, n, tiles, 1 if tiles else 0)


def _call(ctx=None, batch=None, mode=capi.SK_TRIM_SE, outs=None, ws=0x10000, ws_bytes=1 << 20, cuts=0x3000):
    arr = (capi.TrimOutput * 3)(*(outs or []))
    b = batch if batch is not None else _batch()
    return capi.lib().sk_trim_device_async(ctx, C.byref(b), cuts, mode, arr, ws, ws_bytes, None)


def test_trim_argument_checks_without_device():
    """Every one of these returns SK_EINVAL before anything touches a device (the pointers are never dereferenced)."""
    L = capi.lib()
    assert _call() == capi.SK_EINVAL  # NULL ctx
    assert _call(batch=_batch(tiles=0x4000)) == capi.SK_EINVAL  # segmented
    assert _call(batch=_batch(3), mode=capi.SK_TRIM_PE_SPLIT) == capi.SK_EINVAL  # odd n_reads in a PE mode
    assert _call(batch=_batch(3), mode=capi.SK_TRIM_PE_INTERLEAVED) == capi.SK_EINVAL
    assert _call(outs=[capi.TrimOutput(0x5001, None, 0x6000, None, 64, 4)]) == capi.SK_EINVAL  # unaligned out.qual
    assert _call(mode=7) == capi.SK_EINVAL
    c = capi.TrimCounts()
    assert L.sk_trim_device_finish(None, 0x10000, None, C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_device_finish(None, None, None, None) == capi.SK_EINVAL


def test_model_pair_rule():
    cuts = np.array([[0, 5], [0, 4], [0, 3], [-1, -1], [-1, -1], [1, 2], [-1, -1], [-1, -1]], dtype=np.int32)
    assert tm.dests(cuts, "se").tolist() == [0, 0, 0, -1, -1, 0, -1, -1]
    assert tm.dests(cuts, "pe_split").tolist() == [0, 1, 2, -1, -1, 2, -1, -1]
    assert tm.dests(cuts, "pe_interleaved").tolist() == [0, 0, 2, -1, -1, 2, -1, -1]
    qual = np.arange(64, dtype=np.uint8)
    res = tm.expected(qual, None, np.arange(8) * 8, cuts, "pe_split")
    assert res[0]["qual"].tolist() == list(range(0, 5)) and res[1]["qual"].tolist() == list(range(8, 12))
    assert res[2]["qual"].tolist() == [16, 17, 18, 41] and res[2]["read_index"].tolist() == [2, 5]
    assert res[2]["offsets"].tolist() == [0, 3, 4]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_model")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


@pytest.mark.parametrize("name,rec", tm.golden_params())
def test_model_reproduces_reference_runs(workdir, name, rec):
    """The numpy model of the trim, on the oracle's cuts, rebuilds every recorded output file of the reference: what the
    GPU test holds the device to is the reference's behaviour."""
    mode, recs, files = tm.run_batch(rec["argv"], workdir)
    qual, seq, offsets = tm.pack(recs)
    cuts = tm.oracle_cuts(tm.run_params(rec["argv"]), qual, seq, offsets)
    res = tm.expected(qual, seq, offsets[:-1].astype(np.int64), cuts, mode)
    for fname, want in rec["outputs"].items():
        text = tm.fastq_text(recs, res[files[fname]])
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname
