"""GPU: the FASTQ trim with its scan and per-read steps stopping at the records the framing found (the default) against the
same call walking the bound (SK_FQ_COUNTED=0, read by the library on every call): return code, counts, errors and every
byte of every output buffer -- sentinels behind the outputs included -- must be identical."""
import ctypes as C
import os

import numpy as np
import pytest

import cli_util as cu
import fastq_util as fu
import soak_fastq
import trim_model as tm
from sickle_amd import capi
from fastq_raw import SENTINEL, raw, torch_mod, upload
from test_fastq_api import golden_texts
from test_gpu_fastq import BAD, RANGE_BAD, many_good
from test_gpu_fastq_order import budget, raw as raw_ordered

pytestmark = pytest.mark.gpu


def snapshot(rc, counts, keep, *more):
    outs = [None if k is None else (k[0].cpu().numpy().tobytes(), None if k[1] is None else k[1].cpu().numpy().tobytes())
            for k in keep]
    return (rc, counts, outs) + tuple(more)


def both(call):
    """call() -> snapshot, once walking the bound and once with the count; -> the common snapshot"""
    assert "SK_FQ_COUNTED" not in os.environ
    os.environ["SK_FQ_COUNTED"] = "0"
    try:
        bound = call()
    finally:
        del os.environ["SK_FQ_COUNTED"]
    counted = call()
    assert counted[0] == bound[0], ("return code", counted[0], bound[0])
    assert counted[1] == bound[1], ("counts", counted[1], bound[1])
    for o, (a, b) in enumerate(zip(counted[2], bound[2])):
        assert a == b, "output %d differs between SK_FQ_COUNTED=0 and the default" % o
    assert counted[3:] == bound[3:]
    return counted


def plain(ctx, ptuple, texts, mode, **kw):
    return both(lambda: snapshot(*raw(ctx, capi.make_params(*ptuple), texts, mode, **kw)))


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_counted_gpu")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


GOLDEN = [(name, rec) for name, rec in tm.golden_runs() if name not in tm.UNREPLAYABLE]


@pytest.mark.parametrize("name,rec", GOLDEN, ids=[n for n, _ in GOLDEN])
def test_golden_runs(sk_ctx, workdir, name, rec):
    """every -a 1 run the FASTQ tests replay from the input files: interleaved and split, with and without -n"""
    mode, texts, _ = golden_texts(rec["argv"], workdir)
    got = plain(sk_ctx, tm.run_params(rec["argv"]), texts, mode)
    assert got[0] == capi.SK_OK and sum(got[1]["records"]) > 0


def test_golden_se(sk_ctx, workdir):
    runs = [(n, r) for n, r in tm.golden_runs() if n.startswith("se_equiv_selfpair")]
    assert runs
    for name, rec in runs:
        argv = rec["argv"]
        text = open(tm._plain(argv[argv.index("-f") + 1], workdir), "rb").read()
        got = plain(sk_ctx, tm.run_params(argv), [text], "se")
        assert got[0] == capi.SK_OK and got[1]["records"][0] > 0


def test_golden_run_in_thread_order(sk_ctx, workdir):
    """the recorded -a 3 run through the ordered call: outputs, counts, order counts and the table of first units"""
    rec = cu.e2e()["thread_order"]["pe_fr_illumina_n_a3"]
    argv = rec["argv"]
    assert argv[argv.index("-a") + 1] == "3"
    mode, texts, _ = golden_texts(argv, workdir)
    params = capi.make_params(*tm.run_params(argv))
    got = both(lambda: snapshot(*raw_ordered(sk_ctx, params, texts, mode, 3, budget(argv, workdir))))
    assert got[0] == capi.SK_OK and got[1]["order"]["batches"] == rec.get("batches", 0) and sum(got[1]["records"]) > 0


def test_drawn_texts(sk_ctx):
    """100 texts of tests/soak_fastq.py's generator: every mode and encoding, placed newlines, malformed records, chars out
    of range, degenerate texts, capacities that are too small"""
    rng = np.random.default_rng(2033)
    seen = set()
    for it in range(100):
        c = soak_fastq.draw(rng)
        T = sum(len(t) for t in c["texts"])
        caps = [T + 64] * 3 if it % 10 else [max(T // 3, 1)] * 3
        got = plain(sk_ctx, tuple(c["params"]), c["texts"], c["mode"], caps=caps, shift=c["shift"], index=c["index"],
                    max_read_len=0 if it % 3 else 1 << 20)
        seen.add(got[0])
    assert {capi.SK_OK, capi.SK_EFORMAT, capi.SK_ERANGE} <= seen, seen


def test_errors_and_degenerate_texts(sk_ctx):
    pt = ("sanger", 20, 20, False, False)
    good = many_good(3000)
    got = plain(sk_ctx, pt, [b"".join(good[:2100] + [BAD[capi.SK_FQ_LENGTHS]] + good[2100:])], "se")
    assert got[0] == capi.SK_EFORMAT and got[1]["format_record"] == 2100
    got = plain(sk_ctx, pt, [b"".join(good[:2100] + [RANGE_BAD] + good[2100:])], "se")
    assert got[0] == capi.SK_ERANGE and got[1]["range"][0] == 2100
    got = plain(sk_ctx, pt, [b"".join(good[:2999] + [RANGE_BAD])], "se")  # ... in the last record: the read below the count
    assert got[0] == capi.SK_ERANGE and got[1]["range"][0] == 2999
    for text in (b"", b"\n"):
        for mode in ("se", "pe_interleaved"):
            got = plain(sk_ctx, pt, [text], mode)
            assert got[0] == capi.SK_OK and got[1]["records"] == [0, 0, 0]


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4096])
def test_record_counts_around_a_block(sk_ctx, n):
    """records that fill the blocks of 2 048 reads exactly, one more, one fewer: the last block with a record and the first
    without one.  Tiny records, so that the bound is not far above the count, and long ones, where it is 40 times it."""
    tiny = b"".join(b"@%c\n%s\n+\n%s\n" % (97 + k % 26, b"A" * (1 + k % 3), bytes([40 + (k * 7) % 30]) * (1 + k % 3)) for k in range(n))
    for text, pt in ((tiny, ("sanger", 20, 0, False, False)), (b"".join(many_good(n, seed=n)), ("sanger", 20, 20, False, True))):
        for mode in ("se", "pe_interleaved"):
            got = plain(sk_ctx, pt, [text], mode)
            assert got[0] == capi.SK_OK and got[1]["records_in"][0] == n
    halves = [b"".join(many_good(n // 2, seed=1)), b"".join(many_good(n // 2, seed=2))]
    assert plain(sk_ctx, ("sanger", 25, 20, False, False), halves, "pe_split")[0] == capi.SK_OK


def test_chained_call_with_a_short_length_word(sk_ctx):
    """sk_trim_fastq_chained_device_async: the text's length is a device word well below the bound, the buffer behind it
    0x01; read order and the -a 3 order"""
    torch = torch_mod()
    L = capi.lib()
    pt = ("sanger", 20, 20, False, True)
    params = capi.make_params(*pt)
    text = b"".join(many_good(2500, seed=9))
    bound = 3 * len(text) + 5
    buf = torch.full((bound + 16,), 1, dtype=torch.uint8, device="cuda")
    buf[:len(text)] = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    word = torch.tensor([len(text)], dtype=torch.int64, device="cuda")

    def call(order):
        extra = 0 if order is None else order.batch_capacity
        ws_bytes = L.sk_trim_fastq_workspace_bytes(bound, 1) if order is None else L.sk_trim_fastq_ordered_workspace_bytes(bound, 1, extra)
        ws = torch.zeros(ws_bytes, dtype=torch.uint8, device="cuda")
        keep = [(torch.full((bound + 64,), SENTINEL, dtype=torch.uint8, device="cuda"),
                 torch.full((bound // 4 + 4,), -7, dtype=torch.int64, device="cuda")) for _ in range(3)]
        outs = [capi.FastqOutput(t.data_ptr(), bound + 64, ix.data_ptr(), bound // 4 + 4) for t, ix in keep]
        sk_ctx.trim_fastq_chained_device_async(params, [buf.data_ptr()], [bound], outs, ws.data_ptr(), ws_bytes,
                                               bytes_dev_ptrs=[word.data_ptr()], mode="pe_interleaved", order=order)
        c, oc = capi.FastqCounts(), capi.FastqOrderCounts()
        if order is None:
            rc = L.sk_trim_fastq_device_finish(sk_ctx._h, ws.data_ptr(), None, C.byref(c))
        else:
            rc = L.sk_trim_fastq_ordered_device_finish(sk_ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(oc))
        return snapshot(rc, dict(c.as_dict(), order=oc.as_dict()), keep)

    batch_len = fu.reference_batch_len(len(text), paired=True)
    for order in (None, capi.FastqOrder(3, 0, batch_len, bound // batch_len + 16, 0)):
        got = both(lambda: call(order))
        assert got[0] == capi.SK_OK and got[1]["records_in"][0] == 2500 and got[1]["records"][0] > 0
