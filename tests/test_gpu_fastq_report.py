"""GPU: sk_trim_fastq_report_device_async against tests/fastq_report_model.py.  Every comparison is == with the model;
every device array has guard words behind its bins, which must stay untouched."""
import ctypes as C
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:  # the child process of test_uncounted_in_a_child_process runs this file as a script
    sys.path.insert(0, ROOT)

import cli_util as cu
import fastq_model as fm
import fastq_order_model as fo
import fastq_report_model as rm
import fastq_util as fu
import soak_fastq
import trim_model as tm
from sickle_amd import capi
from fastq_raw import torch_mod, upload
from test_fastq_report_model import GOLDEN_SUMMARY_RUNS, P5, PAIRS, TABLE, fastq, golden_case

pytestmark = pytest.mark.gpu

# the quality kernel's chunk, from the source
CHUNK = eval(re.search(r"#define FQP_CHUNK_BYTES \(([^)]*)\)", open(os.path.join(ROOT, "sickle_amd", "csrc", "sk_fastq_report.h")).read())
             .group(1).replace("u", ""))
PATTERN = 0x0101010101010101
GUARD = 4
ARRAYS = rm.LEN_ARRAYS + rm.POS_ARRAYS
KEEP_ALL = ("sanger", 20, 1, False, False)


class Dev:
    """A sk_fastq_report and the histograms in one device tensor pre-filled with PATTERN, GUARD words behind each."""

    def __init__(self, len_bins, pos_bins, arrays=ARRAYS, hists=True):
        torch = torch_mod()
        self.len_bins, self.pos_bins, self.arrays = len_bins, pos_bins, tuple(arrays) if hists else ()
        self.at, n = {}, capi.REPORT_WORDS + GUARD
        for name in ARRAYS:
            if name in self.arrays:
                self.at[name] = n
                n += (len_bins if name in rm.LEN_ARRAYS else pos_bins) + GUARD
        self.t = torch.full((n,), PATTERN, dtype=torch.int64, device="cuda")
        self.ptr = self.t.data_ptr()
        self.hists = None
        if hists:
            p = {name: self.ptr + 8 * self.at[name] if name in self.at else None for name in ARRAYS}
            self.hists = capi.FastqReportHists(p["len_in"], p["len_out"], len_bins, p["qsum_in"], p["qcnt_in"], p["qsum_out"],
                                               p["qcnt_out"], pos_bins)

    def bins(self, name):
        return self.len_bins if name in rm.LEN_ARRAYS else self.pos_bins

    def read(self):
        """-> the report as the model words it (only the arrays given); the guards must hold the pattern"""
        w = self.t.cpu().numpy().view(np.uint64)
        rep = capi.FastqReport.from_buffer_copy(w[:capi.REPORT_WORDS].tobytes()).as_dict()
        assert (w[capi.REPORT_WORDS:capi.REPORT_WORDS + GUARD] == PATTERN).all(), "the words behind the report were written"
        for name, at in self.at.items():
            n = self.bins(name)
            rep[name] = w[at:at + n].copy()
            assert (w[at + n:at + n + GUARD] == PATTERN).all(), "the words behind %s were written" % name
        return rep


def restrict(want, dev):
    """the model's report with only the arrays the device was given"""
    return {k: v for k, v in want.items() if k not in ARRAYS or k in dev.arrays}


def run(ctx, ptuple, texts, mode, dev, form="plain", reset=True, outs="full", order=None, bound_extra=0, valid=1, length=None):
    """One text call and the report behind it, on the null stream.  form: "plain" (sk_trim_fastq_device_async), "piece" (the
    piece call, more == 0), "chained" (the lengths from device words: length, or the text's; bound_extra bytes of bound
    beyond the text), "ordered" (order = (threads, batch_len)).  outs: "full", "count" (every output NULL) or a list of three
    capacities.  -> the finish's return code"""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*ptuple)
    bufs = [upload(t + b"\x01" * bound_extra) for t in texts]
    bounds = [len(t) + bound_extra for t in texts]
    T = sum(bounds)
    cap = capi.fastq_output_bound(T, mode)
    caps = [cap] * 3 if outs == "full" else [None] * 3 if outs == "count" else outs
    keep = [None if c is None else torch.empty(max(c, 16), dtype=torch.uint8, device="cuda") for c in caps]
    arr = [capi.FastqOutput() if k is None else capi.FastqOutput(k.data_ptr(), c, None, 0) for k, c in zip(keep, caps)]
    ptrs = [b[1] for b in bufs]
    fo_ = None
    if form == "ordered":
        fo_ = capi.FastqOrder(order[0], 0, order[1], T // order[1] + 16, 0)
        ws_bytes = L.sk_trim_fastq_ordered_workspace_bytes(T, params.trunc_n, fo_.batch_capacity)
    else:
        ws_bytes = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    ws = torch.full((ws_bytes,), 0x5a, dtype=torch.uint8, device="cuda")
    words = None
    if form == "plain":
        ctx.trim_fastq_device_async(params, ptrs, bounds, arr, ws.data_ptr(), ws_bytes, mode=mode)
    elif form == "ordered":
        ctx.trim_fastq_ordered_device_async(params, ptrs, bounds, fo_, arr, ws.data_ptr(), ws_bytes, mode=mode)
    else:
        kw = {}
        if form == "chained":
            lens = [len(t) for t in texts] if length is None else length
            words = torch.tensor([[n, valid] for n in lens], dtype=torch.int64, device="cuda")
            kw = dict(bytes_dev_ptrs=[words.data_ptr() + 16 * i for i in range(len(texts))],
                      valid_dev_ptrs=[words.data_ptr() + 16 * i + 8 for i in range(len(texts))])
        ctx.trim_fastq_piece_device_async(params, ptrs, bounds, arr, ws.data_ptr(), ws_bytes, mode=mode, piece=form == "piece", **kw)
    kind = {"plain": "plain", "chained": "plain", "piece": "piece", "ordered": "ordered"}[form]
    ctx.trim_fastq_report_device_async(ws.data_ptr(), T, params.trunc_n, dev.ptr, kind=kind,
                                       batch_capacity=fo_.batch_capacity if fo_ else 0, hists=dev.hists, reset=reset)
    c = capi.FastqCounts()
    if form == "piece":
        return ctx._piece_finish(ws.data_ptr(), None)[0]
    if form == "ordered":
        return L.sk_trim_fastq_ordered_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(capi.FastqOrderCounts()))
    return L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))


def check(ctx, ptuple, texts, mode, len_bins=40, pos_bins=40, arrays=ARRAYS, hists=True, want=None, rc=capi.SK_OK, **kw):
    dev = Dev(len_bins, pos_bins, arrays, hists)
    got_rc = run(ctx, ptuple, texts, mode, dev, **kw)
    assert got_rc == rc, (got_rc, capi.lib().sk_last_error(ctx._h))
    if want is None:
        want = rm.report(ptuple, texts, mode, len_bins, pos_bins)
    got = dev.read()
    assert rm.equal(got, restrict(want, dev)) == []
    return got


def reads_text(rng, lens, kind="mixed", names=None):
    """records with the given lengths: qualities all high ("keep"), all low ("drop") or drawn"""
    recs = []
    for i, n in enumerate(lens):
        n = int(n)
        if kind == "keep":
            q = b"I" * n
        elif kind == "drop":
            q = b"#" * n
        else:
            q = np.clip(int(rng.integers(36, 70)) + rng.integers(-14, 9, n), 33, 73).astype(np.uint8).tobytes()
        recs.append((bytes(rng.choice(list(b"ACGTn"), n, p=[.24, .24, .24, .24, .04]).astype(np.uint8)), q))
    return fastq(recs, names=names)


# ---- the hand truth table -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qualtype", ["phred", "sanger", "solexa", "illumina"])
@pytest.mark.parametrize("mode", ["se", "pe_split", "pe_interleaved", "pe_combo_all"])
def test_hand_truth_table(sk_ctx, mode, qualtype):
    """the four pair classes (and SE's kept / discarded) in every mode and quality type, names of 2 to 34 bytes"""
    offset, lowest = {"phred": (0, 4), "sanger": (33, 33), "solexa": (64, 58), "illumina": (64, 64)}[qualtype]
    shift = bytes.maketrans(b"I#", bytes([offset + 40, lowest + 2]))  # quality 40, and two above the type's lowest byte
    reads = [(s, q.translate(shift)) for s, q in PAIRS]
    for name_len in (1, 2, 15, 16, 33):
        names = [b"x" * name_len] * len(reads)
        texts = [fastq(reads[0::2], names[0::2]), fastq(reads[1::2], names[1::2])] if mode == "pe_split" else [fastq(reads, names)]
        pt = (qualtype, 20, 5, False, False)
        got = check(sk_ctx, pt, texts, mode, 16, 16)
        assert (got["reads"], got["kept"], got["discarded"]) == (8, 4, 4) and got["bases_out"] == 2 * 10 + 2 * 10
        assert got["pairs"] == ([0, 0, 0, 0] if mode == "se" else [1, 1, 1, 1])


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
def test_hand_table_of_the_model_test(sk_ctx, case):
    """-x, -n, the 1-base read, the odd interleaved record and the unterminated last line, as the CPU test words them"""
    _, params, mode, texts, _, _ = case
    check(sk_ctx, params, texts, mode, 13, 12)


# ---- shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 3 * 2048 + 1])
@pytest.mark.parametrize("kind", ["keep", "drop"])
def test_read_counts_around_a_block(sk_ctx, n, kind):
    rng = np.random.default_rng(n)
    text = reads_text(rng, rng.integers(1, 40, n), kind)
    got = check(sk_ctx, KEEP_ALL, [text], "se")
    assert got["reads"] == n and got["kept"] == (n if kind == "keep" else 0)
    if n > 1:
        m = n & ~1
        got = check(sk_ctx, KEEP_ALL, [text], "pe_interleaved")
        assert got["reads"] == m and got["pairs"] == ([0, 0, 0, m // 2] if kind == "keep" else [m // 2, 0, 0, 0])


@pytest.mark.parametrize("length", [1, 15, 16, 17, 31, 32, 33])
def test_granule_edges(sk_ctx, length):
    rng = np.random.default_rng(length)
    text = reads_text(rng, [length] * 301)
    for bins in (length, length + 1):
        check(sk_ctx, ("sanger", 20, 1, False, False), [text], "se", bins, bins)


def test_one_base_reads_only(sk_ctx):
    """thousands of reads in one step of the quality kernel"""
    rng = np.random.default_rng(1)
    text = reads_text(rng, [1] * 9001)
    got = check(sk_ctx, KEEP_ALL, [text], "se", 4, 4)
    assert got["reads"] == 9001 and 0 < got["kept"] < 9001


def test_read_longer_than_a_chunk(sk_ctx):
    rng = np.random.default_rng(2)
    lens = [20] * 40
    lens[17] = CHUNK + 1000
    text = reads_text(rng, lens)
    for pos_bins in (1, 64, capi.SK_FQ_REPORT_MAX_POS_BINS):
        got = check(sk_ctx, KEEP_ALL, [text], "pe_interleaved", 64, pos_bins)
    assert got["max_len_in"] == CHUNK + 1000


def test_read_across_a_chunk_boundary(sk_ctx):
    """five on one side of the boundary and three on the other"""
    reads, at = [], 0
    while at + 150 < CHUNK - 40:
        reads.append((b"A" * 150, b"I" * 150))
        at += 150
    before = CHUNK - at  # bytes of the next read below the boundary
    assert 20 < before < 150
    # 200 bases have a window of 20, which reaches quality 20 with ten bases of 40 in it: the 5' cut is the run's first base,
    # ten below the boundary, the 3' cut its end, twenty above
    q = b"#" * (before - 10) + b"I" * 30 + b"#" * (200 - before - 20)
    reads += [(b"C" * 200, q), (b"G" * 150, b"I" * 150)]
    text = fastq(reads)
    buf, recs = fm.reads([text], "se")
    cuts, _ = fm.oracle_cuts(KEEP_ALL, buf, recs)
    five, three = (int(x) for x in cuts[len(reads) - 2])
    assert 0 < five < before < three < 200
    check(sk_ctx, KEEP_ALL, [text], "se", 256, 256)
    check(sk_ctx, KEEP_ALL, [text], "se", 256, 7)


@pytest.fixture(scope="module")
def mixed():
    """one text of 500 pairs of drawn lengths up to 90 and its reports' parameters"""
    rng = np.random.default_rng(3)
    lens = rng.integers(1, 91, 1000)
    lens[3] = 90
    return reads_text(rng, lens), ("sanger", 20, 10, False, False)


@pytest.mark.parametrize("bins", [1, 2, 90, 91, "limits"])
def test_bin_limits(sk_ctx, mixed, bins):
    text, pt = mixed
    lb, pb = (capi.SK_FQ_REPORT_MAX_LEN_BINS, capi.SK_FQ_REPORT_MAX_POS_BINS) if bins == "limits" else (bins, bins)
    got = check(sk_ctx, pt, [text], "pe_interleaved", lb, pb)
    assert got["max_len_in"] == 90 and int(got["len_in"].sum()) == 1000 and int(got["qcnt_in"].sum()) == got["bases_in"]


@pytest.mark.parametrize("missing", list(ARRAYS) + ["positions", "hists"])
def test_null_arrays(sk_ctx, mixed, missing):
    """any single array NULL; all four position arrays NULL (no quality kernel runs); hists NULL"""
    text, pt = mixed
    if missing == "hists":
        check(sk_ctx, pt, [text], "pe_interleaved", hists=False)
    elif missing == "positions":
        check(sk_ctx, pt, [text], "pe_interleaved", 33, 0, arrays=rm.LEN_ARRAYS)
    else:
        check(sk_ctx, pt, [text], "pe_interleaved", 33, 47, arrays=[a for a in ARRAYS if a != missing])


@pytest.mark.parametrize("flags", [(True, False), (False, True), (True, True)])
def test_no5_and_trunc_n(sk_ctx, mixed, flags):
    text, _ = mixed
    for mode in ("se", "pe_interleaved"):
        check(sk_ctx, ("sanger", 25, 10) + flags, [text], mode, 91, 91)


def test_counting_call_and_short_capacity(sk_ctx, mixed):
    """every output NULL, and a capacity one byte short (SK_ESPACE): both report in full"""
    text, pt = mixed
    check(sk_ctx, pt, [text], "pe_interleaved", outs="count")
    need = [len(t) if t is not None else None for t in fm.expected(pt, [text], "pe_interleaved")["texts"]]
    assert need[0] > 1 and need[2] > 1
    check(sk_ctx, pt, [text], "pe_interleaved", outs=[need[0] - 1, None, need[2]], rc=capi.SK_ESPACE)
    check(sk_ctx, pt, [text], "pe_interleaved", outs=[need[0], None, need[2] - 1], rc=capi.SK_ESPACE, form="piece")


@pytest.mark.parametrize("where", ["front", "middle", "end"])
@pytest.mark.parametrize("what", ["format", "range"])
def test_failed_calls_touch_nothing(sk_ctx, where, what):
    """calls_failed is one more; every other word and every array keeps the pattern it was pre-filled with"""
    rng = np.random.default_rng(4)
    good = [reads_text(rng, [int(n)]) for n in rng.integers(20, 80, 5000)]
    # (a quality char below the range at the end of a read that is longer than -l 20: the scan reads it to its end)
    bad = b"@bad\nACGT\n+\nIII\n" if what == "format" else b"@bad\n" + b"ACGT" * 6 + b"\n+\n" + b"I" * 23 + b" \n"
    at = {"front": 0, "middle": 2500, "end": 5000}[where]
    text = b"".join(good[:at] + [bad] + good[at:])
    for form in ("plain", "piece"):
        dev = Dev(32, 32)
        rc = run(sk_ctx, ("sanger", 20, 20, False, False), [text], "se", dev, form=form, reset=False)
        assert rc == (capi.SK_EFORMAT if what == "format" else capi.SK_ERANGE)
        got = dev.read()
        assert got.pop("calls_failed") == PATTERN + 1
        assert got.pop("pairs") == [PATTERN] * 4
        for k, v in got.items():
            assert np.all(np.asarray(v, np.uint64) == PATTERN), k


def test_accumulation(sk_ctx, mixed):
    """two texts into one report without RESET are the sum of their models; RESET over a dirty report is one model"""
    text, pt = mixed
    rng = np.random.default_rng(5)
    other = reads_text(rng, rng.integers(1, 200, 700))
    dev = Dev(64, 64)
    a, b = rm.report(pt, [text], "pe_interleaved", 64, 64), rm.report(pt, [other], "se", 64, 64)
    assert run(sk_ctx, pt, [text], "pe_interleaved", dev, reset=True) == capi.SK_OK  # over the pattern
    assert rm.equal(dev.read(), a) == []
    assert run(sk_ctx, pt, [other], "se", dev, reset=False) == capi.SK_OK
    assert rm.equal(dev.read(), rm.add(a, b)) == []
    bad = b"@bad\nACGT\n+\nIII\n"
    assert run(sk_ctx, pt, [bad], "se", dev, reset=False) == capi.SK_EFORMAT
    assert rm.equal(dev.read(), rm.add(rm.add(a, b), rm.failed(64, 64))) == []
    assert run(sk_ctx, pt, [other], "se", dev, reset=True) == capi.SK_OK
    assert rm.equal(dev.read(), b) == []
    assert run(sk_ctx, pt, [bad], "se", dev, reset=True) == capi.SK_EFORMAT
    assert rm.equal(dev.read(), rm.failed(64, 64)) == []


def test_chained_call(sk_ctx, mixed):
    """the length a device word: at a record's end, one byte behind it, 0; and valid_dev = 0"""
    text, pt = mixed
    ends = [m.end() for m in re.finditer(rb"\n(?=@r)", text)]
    cut = ends[len(ends) // 2 | 1]  # an even number of records in front of it
    for n in (cut, cut + 1, 0):
        want = rm.report(pt, [text[:n]], "pe_interleaved", 40, 40)
        check(sk_ctx, pt, [text], "pe_interleaved", form="chained", length=[n], bound_extra=77, want=want)
    empty = rm.zero(40, 40)
    empty["calls"] = 1
    check(sk_ctx, pt, [text], "pe_interleaved", form="chained", valid=0, want=empty)


def test_uncounted_in_a_child_process(sk_ctx):
    """SK_FQ_COUNTED=0 (the per-read steps walk the bound) in a fresh process"""
    env = dict(os.environ, SK_FQ_COUNTED="0")
    pr = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode == 0 and "child ok" in pr.stdout, pr.stdout[-2000:] + pr.stderr[-2000:]


def _child():
    assert os.environ.get("SK_FQ_COUNTED") == "0"
    import torch
    torch.cuda.is_available()
    ctx = capi.Context(device=0, slots=2)
    rng = np.random.default_rng(6)
    for n in (1, 2048, 2049, 5000):
        text = reads_text(rng, rng.integers(1, 60, n))
        for mode in ("se", "pe_interleaved"):
            if n > 1 or mode == "se":
                check(ctx, ("sanger", 20, 10, False, True), [text], mode, 50, 50)
    check(ctx, P5, [fastq(PAIRS[0::2]), fastq(PAIRS[1::2])], "pe_split", 16, 16)
    ctx.close()
    print("child ok")


# ---- the drivers ----------------------------------------------------------------------------------------------------
def drain(st):
    pieces = list(st)
    return [b"".join(p[o] for p in pieces if p[o] is not None) for o in range(3)]


@pytest.fixture(scope="module")
def pairs300():
    rng = np.random.default_rng(7)
    return [reads_text(rng, rng.integers(20, 120, 300)), reads_text(rng, rng.integers(20, 120, 300))], ("sanger", 22, 15, False, False)


@pytest.mark.parametrize("piece_bytes", [256, 1000, 8192])
def test_stream_driver(sk_ctx, pairs300, piece_bytes):
    """a few hundred pairs in pieces, split and interleaved: the whole-text report"""
    texts, pt = pairs300
    params = capi.make_params(*pt)
    for mode, tt in (("pe_split", texts), ("pe_interleaved", texts[:1]), ("pe_combo_all", texts[:1])):
        want = rm.report(pt, tt, mode, 128, 128)
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=piece_bytes, room=max(2048, piece_bytes),
                                      report=dict(len_bins=128, pos_bins=128))
        assert st.report is None
        out = drain(st)
        want["calls"] = st.pieces
        assert st.pieces > 1 and rm.equal(st.report, want) == []
        plain = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=piece_bytes, room=max(2048, piece_bytes))
        assert drain(plain) == out and plain.report is None and plain.counts == st.counts


@pytest.fixture(scope="module")
def same_lines():
    """two inputs whose lines have the same lengths, so that the reference's reader cuts them into the same batches"""
    lens = np.random.default_rng(8).integers(20, 120, 300)
    return [reads_text(np.random.default_rng(9 + i), lens) for i in range(2)], ("sanger", 22, 15, False, False)


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_ordered_call(sk_ctx, same_lines, threads):
    """the -a T order: the reads inside the batches, whatever their order"""
    texts, pt = same_lines
    for mode, tt in (("pe_split", texts), ("pe_interleaved", texts[:1]), ("se", texts[:1])):
        batch_len = 1500
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        n_reads = units * (1 if mode == "se" else 2)
        assert n_reads > 100
        want = rm.report(pt, tt, mode, 128, 128, n_reads=n_reads)
        check(sk_ctx, pt, tt, mode, 128, 128, form="ordered", order=(threads, batch_len), want=want)


@pytest.mark.parametrize("piece_bytes", [4096, 20000])
def test_ordered_stream_driver(sk_ctx, same_lines, piece_bytes):
    texts, pt = same_lines
    params = capi.make_params(*pt)
    batch_len = 1500
    for mode, tt in (("pe_split", texts), ("pe_interleaved", texts[:1])):
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        want = rm.report(pt, tt, mode, 128, 0, n_reads=2 * units)
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=piece_bytes, room=8192,
                                      order=(3, batch_len), report=dict(len_bins=128))
        drain(st)
        want["calls"] = st.report["calls"]
        assert st.report["calls"] >= st.pieces > 1 and rm.equal(st.report, want) == []


def to_device(data):
    torch = torch_mod()
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def golden_tmp(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("report_golden_gpu")
    cu.prepare_inputs(tmp)
    cu.prepare_long_inputs(tmp)
    return tmp


@pytest.mark.parametrize("name", GOLDEN_SUMMARY_RUNS)
def test_golden_summaries(sk_ctx, golden_tmp, name):
    """trim_gz, trim_gz_stream and trim_gzip_stream on the recorded runs' inputs: summary_text of the device's report is in
    the reference's recorded stdout.  The run whose reader ends at its first batch goes through the ordered calls at the
    reader's budget, as the reference read it."""
    ptuple, texts, mode, n_reads, stdout = golden_case(golden_tmp, name)
    params = capi.make_params(*ptuple)
    want = rm.report(ptuple, texts, mode, 64, 64, n_reads=n_reads)
    kw = {}
    if n_reads is not None:
        rec = cu.e2e()["runs"][name]
        first = rec["argv"][rec["argv"].index("-c") + 1].format(inputs=cu.INPUTS, tmp=str(golden_tmp))
        kw = dict(order=(1, fu.reference_batch_len(os.path.getsize(first), paired=True)))
    rep_opts = dict(len_bins=64, pos_bins=64)
    plain = [gzip.compress(t, 6) for t in texts]
    bgzf = [sk_ctx.bgzf(to_device(t)).cpu().numpy().tobytes() for t in texts]
    two = lambda xs, f=lambda x: x: (f(xs[0]), f(xs[1]) if len(xs) > 1 else None)
    reports = []
    for images in (plain, bgzf):
        out, counts, rep = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode, report=rep_opts, **kw)
        reports.append(rep)
        out2, counts2 = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode, **kw)
        assert counts2 == counts and all((a is None and b is None) or bool((a == b).all()) for a, b in zip(out, out2))
    out, counts, rep = sk_ctx.trim_gz(params, *two(plain, to_device), mode=mode, report=rep_opts,
                                      text_capacity=[len(t) + 10 for t in texts], **kw)
    reports.append(rep)
    piece = max(1 << 20, 4 * kw["order"][1]) if kw else 1 << 20
    longest = max(len(line) for t in texts for line in t.split(b"\n"))
    st = sk_ctx.trim_gz_stream(params, *two(bgzf), mode=mode, piece_bytes=piece, room=4 * longest + 65536, report=rep_opts, **kw)
    list(st)
    reports.append(dict(st.report, calls=1))
    st = sk_ctx.trim_gzip_stream(params, *two(plain), mode=mode, piece_bytes=piece, room=4 * longest + 65536, report=rep_opts, **kw)
    list(st)
    reports.append(dict(st.report, calls=1))
    for rep in reports:
        assert rm.equal(rep, want) == []
        text = capi.summary_text(rep, mode)
        assert text == rm.summary_text(want, mode) and text in stdout


def test_report_false_is_the_parent(sk_ctx, mixed):
    """report=False returns what the calls returned before, and report=True changes no output"""
    text, pt = mixed
    params = capi.make_params(*pt)
    for mode in ("se", "pe_interleaved", "pe_combo_all"):
        a = sk_ctx.trim_fastq(params, to_device(text), mode=mode)
        b = sk_ctx.trim_fastq(params, to_device(text), mode=mode, report=True)
        assert len(a) == 2 and len(b) == 3 and a[1] == b[1]
        assert all((x is None and y is None) or bool((x == y).all()) for x, y in zip(a[0], b[0]))
        assert rm.equal(b[2], rm.report(pt, [text], mode)) == []
        g = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode)
        h = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode, report=dict(pos_bins=91))
        assert len(g) == 2 and len(h) == 3 and g[1] == h[1]
        assert all((x is None and y is None) or bool((x == y).all()) for x, y in zip(g[0], h[0]))
        assert rm.equal(h[2], rm.report(pt, [text], mode, 0, 91)) == []
    o = sk_ctx.trim_fastq(params, to_device(text), mode="pe_interleaved", order=(3, 1500), report=dict(len_bins=91))
    units = fo.batch_tables([fo.lines_of(text)], "pe_interleaved", 1500)["units"]
    assert rm.equal(o[2], rm.report(pt, [text], "pe_interleaved", 91, 0, n_reads=2 * units)) == []


@pytest.mark.parametrize("part", range(10))
def test_drawn_texts(sk_ctx, part):
    """100 texts of tests/soak_fastq.py's generator, ten a case, in plain and piece form: every mode and encoding, malformed
    records, chars out of range, degenerate texts"""
    rng = np.random.default_rng(4100 + part)
    for it in range(10):
        c = soak_fastq.draw(rng)
        pt = tuple(c["params"])
        lb, pb = int(rng.integers(1, 400)), int(rng.integers(1, 400))
        want = rm.report(pt, c["texts"], c["mode"], lb, pb)
        rc_want = capi.SK_OK if want["calls"] else None
        for form in ("plain", "piece"):
            dev = Dev(lb, pb)
            rc = run(sk_ctx, pt, c["texts"], c["mode"], dev, form=form)
            assert (rc == capi.SK_OK) == (rc_want == capi.SK_OK), (rc, c["notes"])
            assert rm.equal(dev.read(), want) == [], (form, c["notes"])


if __name__ == "__main__" and "--child" in sys.argv:
    _child()
