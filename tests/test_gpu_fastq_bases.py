"""GPU: sk_trim_fastq_bases_device_async against tests/fastq_bases_model.py.  Every comparison is == with the model; the
struct and every array have guard words behind them, which must stay untouched."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import fastq_bases_model as bm
import fastq_model as fm
import fastq_order_model as fo
import fastq_report_model as rm
import soak_fastq
from sickle_amd import capi
from fastq_raw import torch_mod, upload
from test_fastq_bases_model import GOLDEN, consistent

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
CHUNK = bm.CHUNK_BYTES  # the kernel's chunk of packed positions
PATTERN = 0x0101010101010101
GUARD = 4
W = capi.BASES_WORDS
G = capi.SK_FQ_BASES_GC_BINS
KEEP_ALL = ("sanger", 20, 1, False, False)
PT = ("sanger", 22, 15, False, False)
ARRAYS = ("pos_in", "pos_out", "gc_in", "gc_out")


class Dev:
    """A sk_fastq_bases and the four arrays in one device tensor pre-filled with PATTERN, GUARD words behind each.
    given: the arrays the call is handed (the others are NULL and must keep the pattern); hists=False: hists == NULL."""

    def __init__(self, pos_bins=0, given=ARRAYS, hists=True):
        torch = torch_mod()
        self.P = pos_bins
        self.given = tuple(a for a in given if pos_bins or not a.startswith("pos")) if hists else ()
        sizes = [W, 6 * pos_bins, 6 * pos_bins, G, G]
        self.at = [0]
        for s in sizes:
            self.at.append(self.at[-1] + s + GUARD)
        self.sizes = sizes
        self.t = torch.full((self.at[-1],), PATTERN, dtype=torch.int64, device="cuda")
        self.ptr = self.t.data_ptr()
        ptr = lambda name: self.ptr + 8 * self.at[1 + ARRAYS.index(name)] if name in self.given else None
        self.hists = capi.FastqBasesHists(ptr("pos_in"), ptr("pos_out"), pos_bins, ptr("gc_in"), ptr("gc_out")) if hists else None

    def words(self):
        w = self.t.cpu().numpy().view(np.uint64)
        for a, s in zip(self.at, self.sizes):
            assert (w[a + s:a + s + GUARD] == PATTERN).all(), "the words behind the struct or an array were written"
        return w

    def read(self):
        """-> the bases as the model words them: the arrays that were given; one that was not must hold the pattern"""
        w = self.words()
        b = capi.FastqBases.from_buffer_copy(w[:W].tobytes()).as_dict()
        for i, name in enumerate(ARRAYS):
            a, s = self.at[1 + i], self.sizes[1 + i]
            if name in self.given:
                b[name] = w[a:a + s].reshape(6, self.P).copy() if name.startswith("pos") else w[a:a + s].copy()
            else:
                assert (w[a:a + s] == PATTERN).all(), "an array that was not given was written"
        self.reserved = [int(x) for x in w[W - 2:W]]
        return b


def run(ctx, ptuple, texts, mode, dev, form="plain", reset=True, outs="full", order=None, bound_extra=0, valid=1, length=None,
        bases_mode=None, shifts=(0, 0), cap_short=0):
    """One text call and the bases behind it, on the null stream.  form: "plain", "piece" (the piece call, more == 0),
    "chained" (the lengths from device words) or "ordered" (order = (threads, batch_len)).  outs: "full" or "count" (every
    output NULL).  bases_mode: the mode the bases are told (the call's, if None).  shifts: each text's offset from a
    16-byte boundary.  cap_short: bytes the output capacities fall short.  -> the finish's return code"""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*ptuple)
    bufs = [upload(t + b"\x01" * bound_extra, s) for t, s in zip(texts, shifts)]
    bounds = [len(t) + bound_extra for t in texts]
    T = sum(bounds)
    cap = capi.fastq_output_bound(T, mode)
    keep = [None if outs == "count" else torch.empty(max(cap, 16), dtype=torch.uint8, device="cuda") for _ in range(3)]
    arr = [capi.FastqOutput() if k is None else capi.FastqOutput(k.data_ptr(), cap - cap_short, None, 0) for k in keep]
    ptrs = [b[1] for b in bufs]
    fo_ = None
    if form == "ordered":
        fo_ = capi.FastqOrder(order[0], 0, order[1], T // order[1] + 16, 0)
        ws_bytes = L.sk_trim_fastq_ordered_workspace_bytes(T, params.trunc_n, fo_.batch_capacity)
    else:
        ws_bytes = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    ws = torch.full((ws_bytes,), 0x5a, dtype=torch.uint8, device="cuda")
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
    ctx.trim_fastq_bases_device_async(ws.data_ptr(), T, params.trunc_n, dev.ptr, ptrs, bounds, mode=bases_mode or mode, kind=kind,
                                      batch_capacity=fo_.batch_capacity if fo_ else 0, hists=dev.hists, reset=reset)
    c = capi.FastqCounts()
    if form == "piece":
        return ctx._piece_finish(ws.data_ptr(), None)[0]
    if form == "ordered":
        return L.sk_trim_fastq_ordered_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(capi.FastqOrderCounts()))
    return L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))


def narrowed(want, dev):
    """the model's result with the arrays the device was given"""
    return {k: v for k, v in want.items() if k not in ARRAYS or k in dev.given}


def check(ctx, ptuple, texts, mode, pos_bins=64, want=None, rc=capi.SK_OK, given=ARRAYS, hists=True, **kw):
    dev = Dev(pos_bins, given, hists)
    got_rc = run(ctx, ptuple, texts, mode, dev, **kw)
    assert got_rc == rc, (got_rc, capi.lib().sk_last_error(ctx._h))
    if want is None:
        want = bm.bases(ptuple, texts, mode, pos_bins, gc=True)
    got = dev.read()
    assert bm.equal(got, narrowed(want, dev)) == [], ({k: got[k] for k in bm.SCALARS + bm.LISTS}, {k: want[k] for k in bm.SCALARS + bm.LISTS})
    assert dev.reserved == [0, 0], "the reserved words are not zero"
    return got


def rec(name, seq, qual):
    return name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def text_of(reads, start=0):
    return b"".join(rec(b"@r%d" % (start + i), s, q) for i, (s, q) in enumerate(reads))


def texts_of(reads, mode):
    """reads: [(seq, qual)], an even number -> the call's texts"""
    if mode == "pe_split":
        return [text_of(reads[0::2]), text_of(reads[1::2])]
    return [text_of(reads)]


def drawn_reads(seed, n, lens=(20, 120), alphabet=b"ACGTACGTACGTNacgtnR."):
    """n reads with drawn lengths, bases and qualities (sanger; lows at either end so that both cuts move)"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, np.uint8)
    out = []
    for _ in range(n):
        m = int(rng.integers(lens[0], lens[1] + 1)) if isinstance(lens, tuple) else lens
        q = np.clip(int(rng.integers(36, 70)) + rng.integers(-14, 9, m), 33, 73).astype(np.uint8)
        out.append((letters[rng.integers(0, len(letters), m)].tobytes(), q.tobytes()))
    return out


# ---- the truth table --------------------------------------------------------------------------------------------------------
def table(hi, lo):
    """the hand table's reads (tests/test_fastq_bases_model.py) with quality bytes that every quality type takes"""
    H, L = bytes([hi]), bytes([lo])
    whole, end, start, low = H * 12, H * 10 + L * 2, L * 2 + H * 10, L * 12
    seqs = [(b"ACGTNacgtnRU", end), (b"A.\x80\xff\rUYRacgt", start), (b"NNNNNNNNNNNN", end), (b"NNNNNNNNNNNN", low),
            (b"ACGTACGTACGN", end), (b"NCGTACGTACGT", start), (b"AAAAAAAAAAAA", whole), (b"GATGATGATGAT", whole),
            (b"GCATGCATGCAT", whole), (b"GCAGCAGCAGCA", whole), (b"GCGCGCGCGCGC", whole), (b"GAAAAAAAAAAA", whole),
            (b"GCNNNNNNNNNA", whole), (b"gcgcgcaNNNNN", whole), (b"AAAAAAAAAAGC", end), (b"ACGTACnGTACG", end),
            (b"ACGnACGTACGT", end), (b"ACGTACNGTACG", end), (b"A", H), (b"n", H), (b"ACGT", low[:4]), (b"T", L)]
    return seqs


@pytest.mark.parametrize("mode", ["se", "pe_split", "pe_interleaved", "pe_combo_all"])
@pytest.mark.parametrize("qualtype", ["phred", "sanger", "solexa", "illumina"])
def test_truth_table(sk_ctx, mode, qualtype):
    reads = table(40, 5) if qualtype == "phred" else table(104, 66)  # a high and a low byte inside the type's range
    for trunc_n in (False, True):
        pt = (qualtype, 20, 5, False, trunc_n)
        want = bm.bases(pt, texts_of(reads, mode), mode, 16, gc=True)
        assert (want["calls"], want["reads"]) == (1, len(reads))
        got = check(sk_ctx, pt, texts_of(reads, mode), mode, pos_bins=16, want=want)
        # counted by hand from the table: the two all-N reads and the lone n have no byte of class 0-3
        assert got["bases_in"] == [66, 37, 42, 23, 46, 9] and got["reads_n_in"] == 11 and got["gc_none_in"] == 3


# ---- alignment and counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s0", [0, 1, 7, 15])
@pytest.mark.parametrize("s1", [0, 1, 7, 15])
def test_split_alignments(sk_ctx, s0, s1):
    """both texts of a split call at byte offsets 0, 1, 7, 15 from an aligned buffer, independently"""
    check(sk_ctx, PT, texts_of(drawn_reads(1, 300), "pe_split"), "pe_split", shifts=(s0, s1))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
def test_read_counts(sk_ctx, n):
    reads = drawn_reads(2, n, lens=(1, 40))
    got = check(sk_ctx, PT, [text_of(reads)], "se", pos_bins=33)
    assert got["reads"] == n
    if n > 1:
        got = check(sk_ctx, PT, [text_of(reads)], "pe_interleaved", pos_bins=33)
        assert got["reads"] == n & ~1


@pytest.mark.parametrize("length", [1, 15, 16, 17, 31, 32, 33, 150])
def test_read_lengths(sk_ctx, length):
    """reads of one length, so that the reads' starts fall at every place in the granules"""
    for shift in (0, 7):
        reads = drawn_reads(3 + length, 700, lens=length)
        check(sk_ctx, ("sanger", 22, 1, False, False), [text_of(reads)], "se", pos_bins=32, shifts=(shift, 0))
    check(sk_ctx, PT, texts_of(reads, "pe_split"), "pe_split", pos_bins=151)


def test_one_base_reads(sk_ctx):
    rng = np.random.default_rng(4)
    reads = [(bytes([int(b)]), bytes([int(rng.integers(33, 74))])) for b in rng.choice(list(b"ACGTNacgtn."), 9001)]
    assert check(sk_ctx, KEEP_ALL, [text_of(reads)], "se", pos_bins=2)["reads"] == 9001
    assert check(sk_ctx, ("sanger", 30, 1, False, False), [text_of(reads)], "pe_interleaved", pos_bins=1)["reads"] == 9000


# ---- chunk and bin edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_bins", [1, 64, 1024])
def test_read_longer_than_a_chunk(sk_ctx, pos_bins):
    """a read of chunk + 1 000 bases among 20-base ones: its owner walks beyond its chunk, the next workgroup starts inside it"""
    short = drawn_reads(5, 100, lens=20)
    long_ = drawn_reads(6, 1, lens=CHUNK + 1000)
    reads = short[:50] + long_ + short[50:]
    for pt in (("sanger", 22, 15, False, False), ("sanger", 22, 15, False, True)):
        got = check(sk_ctx, pt, [text_of(reads)], "se", pos_bins=pos_bins)
        assert got["reads"] == 101 and sum(got["bases_in"]) == 2000 + CHUNK + 1000


def across_the_boundary(n_at):
    """150-base reads up to 100 positions below the chunk boundary, then a 200-base read with five = 40 and three = 160
    under ("sanger", 20, 15, ..) whose only N is at n_at; -> reads"""
    fill = drawn_reads(7, (CHUNK - 100) // 150, lens=150, alphabet=b"ACGT")
    have = 150 * len(fill)
    fill.append((b"A" * (CHUNK - 100 - have), b"I" * (CHUNK - 100 - have)))
    seq = bytearray(b"ACGT" * 50)
    seq[n_at] = ord("N")
    qual = b"#" * 40 + b"I" * 120 + b"#" * 40
    return fill + [(bytes(seq), qual)] + drawn_reads(8, 30, lens=150, alphabet=b"ACGT")


@pytest.mark.parametrize("n_at", [0, 39, 70, 99, 100, 130, 160, 199])
def test_read_across_the_chunk_boundary(sk_ctx, n_at):
    """five below the boundary and three above it; the N on either side of the boundary, inside and outside the output, and
    as the read's first and last byte"""
    reads = across_the_boundary(n_at)
    pt = ("sanger", 20, 15, False, False)
    want = bm.bases(pt, [text_of(reads)], "se", 151, gc=True)
    assert want["reads_n_in"] == 1 and want["reads_n_out"] == (1 if 40 <= n_at < 160 else 0)
    check(sk_ctx, pt, [text_of(reads)], "se", pos_bins=151, want=want)


def test_seq_line_across_a_framing_chunk(sk_ctx):
    """a seq line of 70 000 bytes, across a 64 KiB framing chunk"""
    reads = drawn_reads(9, 3, lens=30) + drawn_reads(10, 1, lens=70000) + drawn_reads(11, 4, lens=30)
    for mode in ("se", "pe_split", "pe_interleaved"):
        check(sk_ctx, PT, texts_of(reads, mode), mode, pos_bins=1024)


# ---- limits and NULLs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_bins", [1, 2, 150, 151, capi.SK_FQ_BASES_MAX_POS_BINS])
def test_pos_bins(sk_ctx, pos_bins):
    reads = drawn_reads(12, 400, lens=150) + drawn_reads(13, 5, lens=1500)
    check(sk_ctx, PT, [text_of(reads)], "se", pos_bins=pos_bins)


@pytest.mark.parametrize("missing", ARRAYS + ("all", "hists"))
def test_null_arrays(sk_ctx, missing):
    reads = drawn_reads(14, 500)
    given = () if missing in ("all", "hists") else tuple(a for a in ARRAYS if a != missing)
    check(sk_ctx, PT, [text_of(reads)], "pe_interleaved", pos_bins=64, given=given, hists=missing != "hists")


# ---- options ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no5,trunc_n", [(False, True), (True, False), (True, True)])
def test_options(sk_ctx, no5, trunc_n):
    reads = drawn_reads(15, 800)
    for mode in ("se", "pe_combo_all"):
        check(sk_ctx, ("sanger", 22, 15, no5, trunc_n), [text_of(reads)], mode, pos_bins=121)


# ---- calls that must touch nothing ------------------------------------------------------------------------------------------
def only_calls_failed(dev):
    w = dev.words()
    assert w[1] == PATTERN + 1
    assert (np.delete(w, 1) == PATTERN).all(), "a call that does not add wrote something"


def test_counting_call_and_short_capacities(sk_ctx):
    """with every output NULL (a counting call), or a byte short (the finish says SK_ESPACE), the bases are there in full"""
    reads = drawn_reads(16, 1300)
    for mode in ("pe_split", "pe_combo_all"):
        check(sk_ctx, KEEP_ALL, texts_of(reads, mode), mode, outs="count")
    # the capacity one byte less than the output the model writes
    text = text_of(drawn_reads(17, 300))
    need = len(fm.expected(PT, [text], "se")["texts"][0])
    check(sk_ctx, PT, [text], "se", rc=capi.SK_ESPACE, cap_short=capi.fastq_output_bound(len(text), "se") - need + 1)
    check(sk_ctx, PT, [text], "se", cap_short=capi.fastq_output_bound(len(text), "se") - need)


@pytest.mark.parametrize("what", ["format", "range"])
@pytest.mark.parametrize("form", ["plain", "piece"])
def test_failed_calls_touch_nothing(sk_ctx, what, form):
    reads = drawn_reads(18, 3000, alphabet=b"ACGT")
    bad = rec(b"@bad", b"ACGT", b"III") if what == "format" else rec(b"@low", b"A" * 41, b"I" * 20 + b" " + b"I" * 20)
    text = text_of(reads[:1400]) + bad + rec(b"@mate", b"C" * 30, b"I" * 30) + text_of(reads[1400:], 1400)
    dev = Dev(64)
    rc = run(sk_ctx, ("sanger", 20, 20, False, False), [text], "pe_interleaved", dev, form=form, reset=False)
    assert rc == (capi.SK_EFORMAT if what == "format" else capi.SK_ERANGE)
    only_calls_failed(dev)


def test_mode_that_disagrees(sk_ctx):
    reads = drawn_reads(19, 80)
    text = [text_of(reads)]
    for call_mode, bases_mode in (("pe_interleaved", "se"), ("se", "pe_interleaved"), ("pe_combo_all", "se")):
        dev = Dev(64)
        assert run(sk_ctx, KEEP_ALL, text, call_mode, dev, reset=False, bases_mode=bases_mode) == capi.SK_OK
        only_calls_failed(dev)
    # SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED: either name fits either call
    want = bm.bases(KEEP_ALL, text, "pe_interleaved", 64, gc=True)
    check(sk_ctx, KEEP_ALL, text, "pe_combo_all", bases_mode="pe_interleaved", want=want)
    check(sk_ctx, KEEP_ALL, text, "pe_interleaved", bases_mode="pe_combo_all", want=want)


def test_accumulation(sk_ctx):
    """two texts with a failed one between them; RESET over a dirty struct"""
    t1 = [text_of(drawn_reads(20, 2500))]
    t2 = texts_of(drawn_reads(21, 900), "pe_split")
    bad = [rec(b"@bad", b"ACGT", b"III")]
    a, b = bm.bases(PT, t1, "pe_interleaved", 64, gc=True), bm.bases(PT, t2, "pe_split", 64, gc=True)
    f = bm.failed(64, True)
    dev = Dev(64)
    assert run(sk_ctx, PT, t1, "pe_interleaved", dev, reset=True) == capi.SK_OK  # over the pattern
    assert bm.equal(dev.read(), a) == []
    assert run(sk_ctx, PT, bad, "se", dev, reset=False) == capi.SK_EFORMAT
    assert bm.equal(dev.read(), bm.add(a, f)) == []
    assert run(sk_ctx, PT, t2, "pe_split", dev, reset=False) == capi.SK_OK
    assert bm.equal(dev.read(), bm.add(bm.add(a, f), b)) == []
    assert run(sk_ctx, PT, t2, "pe_split", dev, reset=True) == capi.SK_OK
    assert bm.equal(dev.read(), b) == [] and dev.reserved == [0, 0]
    assert run(sk_ctx, PT, bad, "se", dev, reset=True) == capi.SK_EFORMAT
    assert bm.equal(dev.read(), f) == []


# ---- the other kinds ----------------------------------------------------------------------------------------------------------
def test_chained_call(sk_ctx):
    """the length a device word, at a record's end; and valid_dev = 0"""
    text = text_of(drawn_reads(22, 800))
    ends = [m.end() for m in re.finditer(rb"\n(?=@r)", text)]
    cut = ends[len(ends) // 2 | 1]  # an even number of records in front of it
    want = bm.bases(PT, [text[:cut]], "pe_interleaved", 64, gc=True)
    assert 0 < want["reads"] < 800
    check(sk_ctx, PT, [text], "pe_interleaved", form="chained", length=[cut], bound_extra=77, want=want)
    check(sk_ctx, PT, [text], "pe_interleaved", form="chained", valid=0, want=dict(bm.zero(64, True), calls=1))


def drain(st):
    pieces = list(st)
    return [b"".join(p[o] for p in pieces if p[o] is not None) for o in range(3)]


def as_stream(want, got):
    """the whole-text model with the calls of the stream: the pieces that added"""
    return dict(want, calls=got["calls"])


OPTS = dict(pos_bins=130, gc=True)


@pytest.mark.parametrize("piece_bytes", [256, 1000, 8192])
def test_stream_driver(sk_ctx, piece_bytes):
    """300 pairs in pieces, split, interleaved and -M: one result for the file, and bases=False is the parent"""
    params = capi.make_params(*PT)
    reads = drawn_reads(23, 600)
    for mode in ("pe_split", "pe_interleaved", "pe_combo_all"):
        tt = texts_of(reads, mode)
        args = dict(mode=mode, piece_bytes=piece_bytes, room=max(2048, piece_bytes))
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, bases=OPTS, **args)
        assert st.bases is None
        out = drain(st)
        assert st.pieces > 1 and st.bases["calls"] == st.pieces and st.bases["calls_failed"] == 0
        assert bm.equal(st.bases, as_stream(bm.bases(PT, tt, mode, 130, gc=True), st.bases)) == []
        plain = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, **args)
        assert drain(plain) == out and plain.bases is None and plain.counts == st.counts


@pytest.fixture(scope="module")
def same_lines():
    """two inputs whose lines have the same lengths, so that the reference's reader cuts them into the same batches"""
    rng = np.random.default_rng(8)
    letters = np.frombuffer(b"ACGTNacgtn", np.uint8)
    t = [[], []]
    for k, m in enumerate(rng.integers(20, 120, 300)):
        for i in range(2):
            q = np.clip(50 + rng.integers(-14, 9, int(m)), 33, 73).astype(np.uint8).tobytes()
            t[i].append(rec(b"@r%03d/%d" % (k, i + 1), letters[rng.integers(0, 10, int(m))].tobytes(), q))
    return [b"".join(t[0]), b"".join(t[1]), b"".join(a + b for a, b in zip(*t))]


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_ordered_call(sk_ctx, same_lines, threads):
    """the -a T order: the reads inside the batches; the order plays no part"""
    for mode, tt in (("pe_split", same_lines[:2]), ("pe_interleaved", same_lines[2:]), ("se", same_lines[2:])):
        batch_len = 1500
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        n_reads = units * (1 if mode == "se" else 2)
        assert n_reads > 100
        check(sk_ctx, PT, tt, mode, form="ordered", order=(threads, batch_len), want=bm.bases(PT, tt, mode, 64, gc=True, n_reads=n_reads))


def test_ordered_stream_driver(sk_ctx, same_lines):
    params = capi.make_params(*PT)
    batch_len = 1500
    for mode, tt in (("pe_split", same_lines[:2]), ("pe_interleaved", same_lines[2:])):
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        want = bm.bases(PT, tt, mode, 130, gc=True, n_reads=2 * units)
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=4096, room=8192,
                                      order=(3, batch_len), bases=OPTS)
        drain(st)
        assert st.bases["calls"] >= st.pieces > 1 and bm.equal(st.bases, as_stream(want, st.bases)) == []


def to_device(data):
    torch = torch_mod()
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _golden(name):
    return open(os.path.join(INPUTS, name), "rb").read()


@pytest.mark.parametrize("case", ["test.fastq", "test.f.fastq", "test.r.fastq", "split"])
def test_gz_drivers_on_the_golden_inputs(sk_ctx, case):
    """trim_gz (two-pass from gzip and BGZF, one-pass), trim_gz_stream and trim_gzip_stream: the numbers of the issue's table"""
    mode = "pe_split" if case == "split" else "pe_interleaved" if case == "test.fastq" else "se"
    texts = [_golden("test.f.fastq"), _golden("test.r.fastq")] if case == "split" else [_golden(case)]
    numbers = GOLDEN["test.fastq" if case == "split" else case]
    pt = ("illumina", 20, 20, False, False)
    params = capi.make_params(*pt)
    want = bm.bases(pt, texts, mode, 151, gc=True)
    opts = dict(pos_bins=151, gc=True)
    plain = [gzip.compress(t, 6) for t in texts]
    bgzf = [sk_ctx.bgzf(to_device(t)).cpu().numpy().tobytes() for t in texts]
    two = lambda xs, f=lambda x: x: (f(xs[0]), f(xs[1]) if len(xs) > 1 else None)
    results = []
    for images in (plain, bgzf):
        out, counts = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode, bases=opts)
        results.append(counts.pop("bases"))
        out2, counts2 = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode)
        assert counts2 == counts and all((a is None and b is None) or bool((a == b).all()) for a, b in zip(out, out2))
    out, counts = sk_ctx.trim_gz(params, *two(plain, to_device), mode=mode, bases=opts, text_capacity=[len(t) + 10 for t in texts])
    results.append(counts["bases"])
    longest = max(len(line) for t in texts for line in t.split(b"\n"))
    for st in (sk_ctx.trim_gz_stream(params, *two(bgzf), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, bases=opts),
               sk_ctx.trim_gzip_stream(params, *two(plain), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, bases=opts)):
        list(st)
        assert st.bases["calls"] >= 1 and st.bases["calls_failed"] == 0
        results.append(dict(st.bases, calls=1))
    for b in results:
        assert bm.equal(b, want) == []
        assert (b["reads"], b["bases_in"], b["reads_n_in"], b["pos_in"][:5, 0].tolist(), int(b["gc_in"][50])) == numbers


def test_bases_false_is_the_parent_and_report_agrees(sk_ctx):
    """bases=False returns what the calls returned before, bases= changes no output and no count, and with report= as well
    the device's own two results satisfy the equalities of the two rules"""
    text = text_of(drawn_reads(24, 1400))
    params = capi.make_params(*PT)
    same = lambda xs, ys: all((x is None and y is None) or bool((x == y).all()) for x, y in zip(xs, ys))
    for mode in ("se", "pe_interleaved", "pe_combo_all"):
        want = bm.bases(PT, [text], mode, 130, gc=True)
        a = sk_ctx.trim_fastq(params, to_device(text), mode=mode)
        b = sk_ctx.trim_fastq(params, to_device(text), mode=mode, bases=OPTS, report=dict(pos_bins=130))
        assert len(a) == 2 and len(b) == 3 and "bases" not in a[1]
        got = b[1].pop("bases")
        assert bm.equal(got, want) == [] and a[1] == b[1] and same(a[0], b[0])
        consistent(got, b[2])
        g = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode)
        h = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode, bases=True, audit=True)
        assert len(g) == len(h) == 2 and bm.equal(h[1].pop("bases"), bm.bases(PT, [text], mode)) == []
        h[1].pop("audit")
        assert g[1] == h[1] and same(g[0], h[0])
    torch = torch_mod()
    e = sk_ctx.trim_fastq(params, torch.empty(0, dtype=torch.uint8, device="cuda"), mode="pe_interleaved", bases=OPTS)
    assert bm.equal(e[1]["bases"], bm.bases(PT, [b""], "pe_interleaved", 130, gc=True)) == [] and e[1]["bases"]["calls"] == 1
    o = sk_ctx.trim_fastq(params, to_device(text), mode="pe_interleaved", order=(3, 1500), bases=OPTS)
    units = fo.batch_tables([fo.lines_of(text)], "pe_interleaved", 1500)["units"]
    assert bm.equal(o[1]["bases"], bm.bases(PT, [text], "pe_interleaved", 130, gc=True, n_reads=2 * units)) == []
    st = sk_ctx.trim_fastq_stream(params, text, mode="pe_interleaved", piece_bytes=20000, room=4096, bases=OPTS,
                                  report=dict(pos_bins=130))
    list(st)
    consistent(st.bases, st.report)
    assert rm.equal({k: st.report[k] for k in ("reads", "kept")}, {k: st.bases[k] for k in ("reads", "kept")}) == []


@pytest.mark.parametrize("part", range(10))
def test_drawn_texts(sk_ctx, part):
    """100 texts of tests/soak_fastq.py's generator, ten a case, in plain and piece form: every mode and encoding, malformed
    records, chars out of range, degenerate texts"""
    rng = np.random.default_rng(5300 + part)
    for it in range(10):
        c = soak_fastq.draw(rng)
        pt = tuple(c["params"])
        bins = int(rng.choice([1, 7, 64, 300]))
        want = bm.bases(pt, c["texts"], c["mode"], bins, gc=True)
        for form in ("plain", "piece"):
            dev = Dev(bins)
            rc = run(sk_ctx, pt, c["texts"], c["mode"], dev, form=form)
            assert (rc == capi.SK_OK) == bool(want["calls"]), (rc, c["notes"])
            assert bm.equal(dev.read(), want) == [], (form, c["notes"])
