"""GPU: sk_trim_fastq_audit_device_async against tests/fastq_audit_model.py.  Every comparison is == with the model; the
struct and the histogram have guard words behind them, which must stay untouched."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import fastq_audit_model as am
import fastq_model as fm
import fastq_order_model as fo
import soak_fastq
from sickle_amd import capi
from fastq_raw import torch_mod, upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
CHUNK = am.CHUNK_BYTES  # the quality kernel's chunk
PATTERN = 0x0101010101010101
GUARD = 4
W = capi.AUDIT_WORDS
KEEP_ALL = ("sanger", 20, 1, False, False)
PT = ("sanger", 22, 15, False, False)
NAME_WORDS = am.NAME_WORDS


class Dev:
    """A sk_fastq_audit and the histogram in one device tensor pre-filled with PATTERN, GUARD words behind each."""

    def __init__(self, hist=True):
        torch = torch_mod()
        self.t = torch.full((W + GUARD + 256 + GUARD,), PATTERN, dtype=torch.int64, device="cuda")
        self.ptr = self.t.data_ptr()
        self.hist_ptr = self.ptr + 8 * (W + GUARD) if hist else None

    def words(self):
        w = self.t.cpu().numpy().view(np.uint64)
        assert (w[W:W + GUARD] == PATTERN).all(), "the words behind the struct were written"
        assert (w[W + GUARD + 256:] == PATTERN).all(), "the words behind the histogram were written"
        return w

    def read(self):
        """-> the audit as the model words it; without a histogram the array must hold the pattern"""
        w = self.words()
        a = capi.FastqAudit.from_buffer_copy(w[:W].tobytes()).as_dict()
        a["qual_hist"] = w[W + GUARD:W + GUARD + 256].copy()
        if self.hist_ptr is None:
            assert (a["qual_hist"] == PATTERN).all(), "a histogram that was not given was written"
        a["reserved"] = [int(x) for x in w[9:W]]
        return a


def run(ctx, ptuple, texts, mode, dev, form="plain", reset=True, outs="full", order=None, bound_extra=0, valid=1, length=None,
        names=True, audit_mode=None, shifts=(0, 0)):
    """One text call and the audit behind it, on the null stream.  form: "plain", "piece" (the piece call, more == 0),
    "chained" (the lengths from device words) or "ordered" (order = (threads, batch_len)).  outs: "full" or "count" (every
    output NULL).  names=False: in == NULL.  audit_mode: the mode the audit is told (the call's, if None).  shifts: each
    text's offset from a 16-byte boundary.  -> the finish's return code"""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*ptuple)
    bufs = [upload(t + b"\x01" * bound_extra, s) for t, s in zip(texts, shifts)]
    bounds = [len(t) + bound_extra for t in texts]
    T = sum(bounds)
    cap = capi.fastq_output_bound(T, mode)
    keep = [None if outs == "count" else torch.empty(max(cap, 16), dtype=torch.uint8, device="cuda") for _ in range(3)]
    arr = [capi.FastqOutput() if k is None else capi.FastqOutput(k.data_ptr(), cap, None, 0) for k in keep]
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
    ctx.trim_fastq_audit_device_async(ws.data_ptr(), T, params.trunc_n, dev.ptr, text_ptrs=ptrs if names else None,
                                      text_bounds=bounds, mode=audit_mode or mode, kind=kind,
                                      batch_capacity=fo_.batch_capacity if fo_ else 0, qual_hist_ptr=dev.hist_ptr, reset=reset)
    c = capi.FastqCounts()
    if form == "piece":
        return ctx._piece_finish(ws.data_ptr(), None)[0]
    if form == "ordered":
        return L.sk_trim_fastq_ordered_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(capi.FastqOrderCounts()))
    return L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))


def check(ctx, ptuple, texts, mode, want=None, rc=capi.SK_OK, hist=True, **kw):
    dev = Dev(hist)
    got_rc = run(ctx, ptuple, texts, mode, dev, **kw)
    assert got_rc == rc, (got_rc, capi.lib().sk_last_error(ctx._h))
    if want is None:
        want = am.audit(ptuple, texts, mode, names=kw.get("names", True))
    got = dev.read()
    assert am.equal(got, want, hist=hist) == [], ({k: got[k] for k in am.SCALARS}, {k: want[k] for k in am.SCALARS})
    assert got["reserved"] == [am.NONE, 0, 0, 0, 0, 0, 0], "the kernels' own words are not at rest"
    return got


def rec(name, qual=b"IIIII", seq=None):
    return name + b"\n" + (seq or b"A" * len(qual)) + b"\n+\n" + qual + b"\n"


def texts_of(pairs, mode, qual=b"IIIII"):
    """pairs: [(name 1, name 2)] -> the call's texts"""
    if mode == "pe_split":
        return [b"".join(rec(a, qual) for a, _ in pairs), b"".join(rec(b, qual) for _, b in pairs)]
    return [b"".join(rec(a, qual) + rec(b, qual) for a, b in pairs)]


def table(lens=range(2, 41)):
    """the truth table at every name length: the mate equal, off by the key's last byte, a byte longer, the tags, swapped,
    swapped on unequal keys, /3, /1/1, a tag on one side; bare and with a comment behind each kind of end"""
    out = []
    for n in lens:
        base = b"@" + b"k" * (n - 1)
        off = base[:-1] + b"j"
        rows = [(base, base), (base, off), (base, base + b"k"), (base + b"/1", base + b"/2"), (base + b"/2", base + b"/1"),
                (base + b"/2", off + b"/1"), (base + b"/3", base + b"/3"), (base + b"/1/1", base + b"/1/2"), (base, base + b"/1")]
        for a, b in rows:
            out.append((a, b))
            for e in (b" ", b"\t", b"\r"):
                out.append((a + e + b"1:N:0:ACGT", b + e + b"2:N"))
    out += [(b"@/1", b"@/2"), (b"@/2", b"@/1"), (b"@ a", b"@ b"), (b"@M:1:FC:1:1101:1:1 1:N:0:ACGT", b"@M:1:FC:1:1101:1:1 2:N:0:ACGT")]
    return out


# ---- names --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["se", "pe_split", "pe_interleaved", "pe_combo_all"])
def test_truth_table(sk_ctx, mode):
    """names of 2 to 40 bytes in the three pair modes; SK_TRIM_SE leaves the name words alone and fills the quality words"""
    pairs = table()
    texts = texts_of(pairs, "pe_interleaved" if mode == "se" else mode)
    got = check(sk_ctx, KEEP_ALL, texts, mode)
    if mode == "se":
        assert got["pairs"] == 0 and got["qual_bytes"] == 10 * len(pairs)
        dev = Dev()
        assert run(sk_ctx, KEEP_ALL, texts, mode, dev, reset=False) == capi.SK_OK  # over the pattern: untouched is untouched
        a = dev.read()
        assert [a[k] for k in NAME_WORDS] == [PATTERN] * 4 and a["reserved"] == [PATTERN] * 7
        assert (a["calls"], a["qual_bytes"], a["qual_min"]) == (PATTERN + 1, PATTERN + 10 * len(pairs), 73)
    else:
        # by hand: of the nine rows, rows 1, 2, 5 and 8 ("k.." against "k../1" is equal) ...
        per_len = 4 * 3  # (base, off), (base, longer), (swapped tags on unequal keys): three mismatches, each four times
        assert got["pairs"] == len(pairs) and got["name_mismatch"] == 39 * per_len and got["first_mismatch"] == 4
        assert got["tags_swapped"] == 39 * 4 + 1


@pytest.mark.parametrize("s0", [0, 1, 7, 15])
@pytest.mark.parametrize("s1", [0, 1, 7, 15])
def test_split_alignments(sk_ctx, s0, s1):
    """both texts of a split call at byte offsets 0, 1, 7, 15 from an aligned buffer, independently"""
    check(sk_ctx, KEEP_ALL, texts_of(table(range(2, 41, 3)), "pe_split"), "pe_split", shifts=(s0, s1))


def counted_pairs(n, how, at=0):
    return [(b"@r%d/1" % k, b"@r%d%s/2" % (k, b"x" if how == "all" or (how == "one" and k == at) else b"")) for k in range(n)]


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 3073])
def test_pair_counts_around_a_block(sk_ctx, n):
    for how, at in [("none", 0), ("all", 0)] + [("one", x) for x in sorted({0, n // 2, n - 1})]:
        for mode in ("pe_interleaved", "pe_split"):
            got = check(sk_ctx, KEEP_ALL, texts_of(counted_pairs(n, how, at), mode), mode)
            assert got["pairs"] == n
            assert got["name_mismatch"] == {"none": 0, "all": n, "one": 1}[how]
            assert got["first_mismatch"] == {"none": am.NONE, "all": 0, "one": at}[how]


@pytest.mark.parametrize("differ", [True, False])
def test_long_name_lines(sk_ctx, differ):
    """a name line of 70 000 bytes, across a 64 KiB framing chunk: its only differing byte is its last key byte, or none"""
    a = b"@" + b"n" * 69999
    b = a[:-1] + (b"m" if differ else b"n")
    for mode in ("pe_split", "pe_interleaved"):
        for x, y in ((a, b), (a + b" 1:N", b + b"\t2:N"), (a + b"/1", b + b"/2")):
            got = check(sk_ctx, KEEP_ALL, texts_of([(b"@p/1", b"@p/2"), (x, y), (b"@q", b"@q")], mode), mode)
            assert (got["pairs"], got["name_mismatch"]) == (3, 1 if differ else 0)
            assert got["first_mismatch"] == (1 if differ else am.NONE)


# ---- quality ------------------------------------------------------------------------------------------------------------
def planted(n_reads, length, spots):
    """n_reads reads of `length` bases of quality 'F'; spots: {packed position: byte}"""
    q = np.full(n_reads * length, ord("F"), np.uint8)
    for at, v in spots.items():
        q[at] = v
    return b"".join(rec(b"@r%d" % i, q[i * length:(i + 1) * length].tobytes()) for i in range(n_reads))


def test_extremes_at_the_edges(sk_ctx):
    """the minimum and the maximum at the first and the last packed byte, at either side of a read boundary and of the
    kernel's chunk boundary"""
    n, length = 1400, 200
    total = n * length
    assert total > CHUNK + length and CHUNK % length not in (0, length - 1)
    for lo_at, hi_at in ((0, total - 1), (total - 1, 0), (700 * length - 1, 700 * length), (700 * length, 700 * length - 1),
                         (CHUNK - 1, CHUNK), (CHUNK, CHUNK - 1)):
        got = check(sk_ctx, KEEP_ALL, [planted(n, length, {lo_at: 33, hi_at: 126})], "se")
        assert (got["qual_bytes"], got["qual_min"], got["qual_max"]) == (total, 33, 126)
        assert got["qual_hist"][33] == 1 and got["qual_hist"][126] == 1 and got["qual_hist"][70] == total - 2


def test_high_bytes_in_short_reads(sk_ctx):
    """bytes >= 0x80 in reads shorter than -l: no range error, and they count as unsigned"""
    text = rec(b"@a", b"I" * 30) + rec(b"@b", b"\x80\xff\x90", b"ACG") + rec(b"@c", b"5" * 30) + rec(b"@d", b"\xfe", b"A")
    for mode in ("se", "pe_interleaved"):
        got = check(sk_ctx, ("sanger", 20, 20, False, False), [text], mode)
        assert (got["calls"], got["qual_bytes"], got["qual_min"], got["qual_max"]) == (1, 64, 53, 255)
        assert got["qual_hist"][0x80] == got["qual_hist"][0xff] == got["qual_hist"][0xfe] == 1


def test_one_base_reads(sk_ctx):
    rng = np.random.default_rng(1)
    text = b"".join(rec(b"@r%d" % i, bytes([int(rng.integers(33, 74))])) for i in range(9001))
    assert check(sk_ctx, KEEP_ALL, [text], "se")["qual_bytes"] == 9001
    assert check(sk_ctx, KEEP_ALL, [text], "pe_interleaved")["qual_bytes"] == 9000


def test_one_value_and_all_printable(sk_ctx):
    """the histogram's worst case, every byte one value, and all 94 printable values"""
    one = b"".join(rec(b"@r%d" % i, b"I" * 151) for i in range(2000))
    got = check(sk_ctx, KEEP_ALL, [one], "se")
    assert got["qual_hist"][73] == 2000 * 151 == got["qual_bytes"] and (got["qual_min"], got["qual_max"]) == (73, 73)
    rng = np.random.default_rng(2)
    every = b"".join(rec(b"@r%d" % i, rng.integers(33, 127, 97).astype(np.uint8).tobytes()) for i in range(1500))
    got = check(sk_ctx, ("sanger", 0, 1, False, False), [every], "se")
    assert (got["qual_min"], got["qual_max"]) == (33, 126) and np.count_nonzero(got["qual_hist"]) == 94


def test_null_histogram_and_null_input(sk_ctx):
    texts = texts_of(counted_pairs(700, "one", 350), "pe_split")
    check(sk_ctx, KEEP_ALL, texts, "pe_split", hist=False)
    got = check(sk_ctx, KEEP_ALL, texts, "pe_split", names=False)
    assert (got["pairs"], got["first_mismatch"], got["qual_bytes"]) == (0, am.NONE, 1400 * 5)
    dev = Dev()
    assert run(sk_ctx, KEEP_ALL, texts, "pe_split", dev, reset=False, names=False) == capi.SK_OK
    assert [dev.read()[k] for k in NAME_WORDS] == [PATTERN] * 4  # in == NULL: the four name words stay as they are


# ---- validity -----------------------------------------------------------------------------------------------------------
def only_calls_failed(dev):
    w = dev.words()
    assert w[1] == PATTERN + 1
    assert (np.delete(w, 1) == PATTERN).all(), "a call that does not add wrote something"


@pytest.mark.parametrize("what", ["format", "range"])
@pytest.mark.parametrize("form", ["plain", "piece"])
def test_failed_calls_touch_nothing(sk_ctx, what, form):
    pairs = counted_pairs(1500, "all")
    bad = rec(b"@bad", b"III", b"ACGT") if what == "format" else rec(b"@low", b"I" * 20 + b" " + b"I" * 20)
    text = texts_of(pairs[:700], "pe_interleaved")[0] + bad + rec(b"@mate", b"I" * 30) + texts_of(pairs[700:], "pe_interleaved")[0]
    dev = Dev()
    rc = run(sk_ctx, ("sanger", 20, 20, False, False), [text], "pe_interleaved", dev, form=form, reset=False)
    assert rc == (capi.SK_EFORMAT if what == "format" else capi.SK_ERANGE)
    only_calls_failed(dev)


def test_mode_that_disagrees(sk_ctx):
    texts = texts_of(counted_pairs(40, "all"), "pe_interleaved")
    for call_mode, audit_mode, names in (("pe_interleaved", "se", True), ("pe_interleaved", "pe_split", False),
                                         ("se", "pe_interleaved", True), ("pe_combo_all", "se", True)):
        dev = Dev()
        assert run(sk_ctx, KEEP_ALL, texts, call_mode, dev, reset=False, audit_mode=audit_mode, names=names) == capi.SK_OK
        only_calls_failed(dev)
    # SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED: either name fits either call
    want = am.audit(KEEP_ALL, texts, "pe_interleaved")
    check(sk_ctx, KEEP_ALL, texts, "pe_combo_all", audit_mode="pe_interleaved", want=want)
    check(sk_ctx, KEEP_ALL, texts, "pe_interleaved", audit_mode="pe_combo_all", want=want)


def test_accumulation(sk_ctx):
    """two texts with a failed one between them: first_mismatch numbers pairs over the ADDING calls; RESET over a dirty struct"""
    t1 = texts_of(counted_pairs(2500, "none"), "pe_interleaved")
    t2 = texts_of(counted_pairs(900, "one", 611), "pe_split")
    bad = [rec(b"@bad", b"III", b"ACGT")]
    a, b = am.audit(PT, t1, "pe_interleaved"), am.audit(PT, t2, "pe_split")
    dev = Dev()
    assert run(sk_ctx, PT, t1, "pe_interleaved", dev, reset=True) == capi.SK_OK  # over the pattern
    assert am.equal(dev.read(), a) == []
    assert run(sk_ctx, PT, bad, "se", dev, reset=False) == capi.SK_EFORMAT
    assert am.equal(dev.read(), am.add(a, am.failed())) == []
    assert run(sk_ctx, PT, t2, "pe_split", dev, reset=False) == capi.SK_OK
    got = dev.read()
    assert am.equal(got, am.add(am.add(a, am.failed()), b)) == [] and got["first_mismatch"] == 2500 + 611
    assert run(sk_ctx, PT, t2, "pe_split", dev, reset=True) == capi.SK_OK
    assert am.equal(dev.read(), b) == [] and dev.read()["first_mismatch"] == 611
    assert run(sk_ctx, PT, bad, "se", dev, reset=True) == capi.SK_EFORMAT
    assert am.equal(dev.read(), am.failed()) == []


def test_counting_call(sk_ctx):
    """with every output NULL (SK_ESPACE does not matter) the audit is there in full"""
    for mode in ("pe_split", "pe_combo_all"):
        check(sk_ctx, PT, texts_of(counted_pairs(1300, "one", 1299), mode), mode, outs="count")


# ---- the other kinds ------------------------------------------------------------------------------------------------------
def drawn_pairs(seed, n, mismatch_at=None, lens=(20, 120), same_length=False):
    """n pairs with drawn lengths and qualities, named r<k>/1 and r<k>/2 -> (text 1, text 2, interleaved).  The mismatching
    mate 2 is r<k>x/2, or with same_length q<k>/2, which leaves every byte of the texts but that one where it was."""
    rng = np.random.default_rng(seed)
    t = [[], []]
    for k in range(n):
        for i in range(2):
            m = int(rng.integers(*lens))
            q = np.clip(int(rng.integers(36, 70)) + rng.integers(-14, 9, m), 33, 73).astype(np.uint8).tobytes()
            off = k == mismatch_at and i
            name = b"@%s%d%s/%d" % (b"q" if off and same_length else b"r", k, b"x" if off and not same_length else b"", i + 1)
            t[i].append(rec(name, q, bytes(rng.choice(list(b"ACGT"), m).astype(np.uint8))))
    return b"".join(t[0]), b"".join(t[1]), b"".join(a + b for a, b in zip(*t))


def test_chained_call(sk_ctx):
    """the length a device word, at a record's end; and valid_dev = 0"""
    _, _, text = drawn_pairs(3, 400, mismatch_at=77)
    ends = [m.end() for m in re.finditer(rb"\n(?=@r)", text)]
    cut = ends[len(ends) // 2 | 1]  # an even number of records in front of it
    want = am.audit(PT, [text[:cut]], "pe_interleaved")
    assert want["first_mismatch"] == 77 and 0 < want["pairs"] < 400
    check(sk_ctx, PT, [text], "pe_interleaved", form="chained", length=[cut], bound_extra=77, want=want)
    empty = am.zero()
    empty["calls"] = 1
    check(sk_ctx, PT, [text], "pe_interleaved", form="chained", valid=0, want=empty)


def drain(st):
    pieces = list(st)
    return [b"".join(p[o] for p in pieces if p[o] is not None) for o in range(3)]


def as_stream(want, st_audit):
    """the whole-text model with the calls of the stream: the pieces that added"""
    return dict(want, calls=st_audit["calls"])


def drain_with_starts(st, mode):
    """-> (the outputs, the number in the file of the first pair of every piece that took pairs), the starts from the
    driver's counts as they stand behind each piece: the records the pieces before it took"""
    pieces, starts, before = [], [], 0
    for p in st:
        pieces.append(p)
        rec = st.counts["records_in"]
        if mode == "pe_split":
            assert rec[0] == rec[1]
            after = rec[0]
        else:
            assert rec[0] % 2 == 0, "a piece took half a pair"
            after = rec[0] // 2
        if after > before:
            starts.append(before)
        before = after
    return [b"".join(p[o] for p in pieces if p[o] is not None) for o in range(3)], starts


@pytest.mark.parametrize("piece_bytes", [256, 1000, 8192])
def test_stream_driver(sk_ctx, piece_bytes):
    """300 pairs in pieces, split, interleaved and -M, one mismatch planted in the first pair of a piece, so that a piece
    boundary separates it from its predecessor: first_mismatch is the pair's number in the file.  The planted name has the
    length of the one it replaces, so the pieces fall where they fell in the run without it, which gives the boundaries;
    the planted run's own counts must then show the pair at the start of its piece."""
    params = capi.make_params(*PT)
    two = lambda tt: (tt[0], tt[1] if len(tt) > 1 else None)
    pick = lambda t, mode: [t[0], t[1]] if mode == "pe_split" else [t[2]]
    clean = drawn_pairs(7, 300)
    for mode in ("pe_split", "pe_interleaved", "pe_combo_all"):
        args = dict(mode=mode, piece_bytes=piece_bytes, room=max(2048, piece_bytes))
        st = sk_ctx.trim_fastq_stream(params, *two(pick(clean, mode)), audit=True, **args)
        _, starts = drain_with_starts(st, mode)
        assert am.equal(st.audit, as_stream(am.audit(PT, pick(clean, mode), mode), st.audit)) == []
        assert st.audit["name_mismatch"] == 0 and st.audit["first_mismatch"] == am.NONE
        behind = [s for s in starts if s > 0]  # the pieces with a pair in front of them
        assert len(behind) >= 2
        for at in (behind[len(behind) // 2], behind[-1]):
            tt = pick(drawn_pairs(7, 300, mismatch_at=at, same_length=True), mode)
            want = am.audit(PT, tt, mode)
            assert (want["pairs"], want["name_mismatch"], want["first_mismatch"]) == (300, 1, at)
            st = sk_ctx.trim_fastq_stream(params, *two(tt), audit=True, **args)
            assert st.audit is None
            out, got_starts = drain_with_starts(st, mode)
            assert at in got_starts, "the planted pair is not the first of its piece"
            assert st.pieces > 1 and st.audit["calls"] == st.pieces and st.audit["calls_failed"] == 0
            assert am.equal(st.audit, as_stream(want, st.audit)) == []
            assert st.audit["first_mismatch"] == at
        plain = sk_ctx.trim_fastq_stream(params, *two(tt), **args)
        assert drain(plain) == out and plain.audit is None and plain.counts == st.counts


@pytest.fixture(scope="module")
def same_lines():
    """two inputs whose lines have the same lengths, so that the reference's reader cuts them into the same batches"""
    rng = np.random.default_rng(8)
    lens = rng.integers(20, 120, 300)
    t = [[], []]
    for k, m in enumerate(lens):
        for i in range(2):
            q = np.clip(50 + rng.integers(-14, 9, int(m)), 33, 73).astype(np.uint8).tobytes()
            t[i].append(rec(b"@r%03d%s/%d" % (k, b"x" if (k == 33 and i) else b"y", i + 1), q))
    return [b"".join(t[0]), b"".join(t[1]), b"".join(a + b for a, b in zip(*t))]


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_ordered_call(sk_ctx, same_lines, threads):
    """the -a T order: the reads inside the batches, numbered in read order"""
    for mode, tt in (("pe_split", same_lines[:2]), ("pe_interleaved", same_lines[2:]), ("se", same_lines[2:])):
        batch_len = 1500
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        n_reads = units * (1 if mode == "se" else 2)
        assert n_reads > 100
        want = am.audit(PT, tt, mode, n_reads=n_reads)
        got = check(sk_ctx, PT, tt, mode, form="ordered", order=(threads, batch_len), want=want)
        assert got["first_mismatch"] == (am.NONE if mode == "se" else 33)


@pytest.mark.parametrize("piece_bytes", [4096, 20000])
def test_ordered_stream_driver(sk_ctx, same_lines, piece_bytes):
    params = capi.make_params(*PT)
    batch_len = 1500
    for mode, tt in (("pe_split", same_lines[:2]), ("pe_interleaved", same_lines[2:])):
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        want = am.audit(PT, tt, mode, n_reads=2 * units)
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=piece_bytes, room=8192,
                                      order=(3, batch_len), audit=True)
        drain(st)
        assert st.audit["calls"] >= st.pieces > 1 and am.equal(st.audit, as_stream(want, st.audit)) == []
        assert st.audit["first_mismatch"] == 33


def to_device(data):
    torch = torch_mod()
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _golden(name):
    return open(os.path.join(INPUTS, name), "rb").read()


def _drop(text, first=False, last=False):
    """the text without its first and / or its last record"""
    f = fm.frame(text)
    a = int(f["e3"][0]) + 1 if first else 0
    b = int(f["s0"][-1]) if last else len(text)
    return text[a:b]


# the issue's table: (file, drop its first record, drop its last), mode ->
# (pairs, mismatches, swapped, first_mismatch, bytes, min, max), None: the model's
GOLDEN = {
    "split": ((("test.f.fastq", 0, 0), ("test.r.fastq", 0, 0)), "pe_split", (1250, 0, 0, am.NONE, None, None, None)),
    "swapped": ((("test.r.fastq", 0, 0), ("test.f.fastq", 0, 0)), "pe_split", (1250, 0, 1250, am.NONE, None, None, None)),
    "shifted": ((("test.f.fastq", 0, 1), ("test.r.fastq", 1, 0)), "pe_split", (1249, 1249, None, 0, None, None, None)),
    "interleaved": ((("test.fastq", 0, 0),), "pe_interleaved", (1250, 0, 0, am.NONE, 375000, 66, 105)),
    "combo_all": ((("test.fastq", 0, 0),), "pe_combo_all", (1250, 0, 0, am.NONE, 375000, 66, 105)),
    "lost_read": ((("test.fastq", 1, 1),), "pe_interleaved", (1249, 1249, None, None, None, None, None)),
    "problem1": ((("problem1.fastq", 0, 0),), "pe_interleaved", (2, 0, None, None, None, None, None)),  # its fifth record in no count
}


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_gz_drivers_on_the_golden_inputs(sk_ctx, case):
    """trim_gz (two-pass from gzip and BGZF, one-pass), trim_gz_stream and trim_gzip_stream: the numbers of DESIGN 4.18's table"""
    files, mode, numbers = GOLDEN[case]
    texts = [_drop(_golden(f), bool(first), bool(last)) for f, first, last in files]
    pt = ("illumina", 20, 20, False, False)
    params = capi.make_params(*pt)
    want = am.audit(pt, texts, mode)
    keys = ("pairs", "name_mismatch", "tags_swapped", "first_mismatch", "qual_bytes", "qual_min", "qual_max")
    assert all(n is None or want[k] == n for k, n in zip(keys, numbers))
    plain = [gzip.compress(t, 6) for t in texts]
    bgzf = [sk_ctx.bgzf(to_device(t)).cpu().numpy().tobytes() for t in texts]
    two = lambda xs, f=lambda x: x: (f(xs[0]), f(xs[1]) if len(xs) > 1 else None)
    audits = []
    for images in (plain, bgzf):
        out, counts = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode, audit=True)
        audits.append(counts.pop("audit"))
        out2, counts2 = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode)
        assert counts2 == counts and all((a is None and b is None) or bool((a == b).all()) for a, b in zip(out, out2))
    out, counts = sk_ctx.trim_gz(params, *two(plain, to_device), mode=mode, audit=True, text_capacity=[len(t) + 10 for t in texts])
    audits.append(counts["audit"])
    longest = max(len(line) for t in texts for line in t.split(b"\n"))
    for st in (sk_ctx.trim_gz_stream(params, *two(bgzf), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, audit=True),
               sk_ctx.trim_gzip_stream(params, *two(plain), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, audit=True)):
        list(st)
        assert st.audit["calls"] >= 1 and st.audit["calls_failed"] == 0
        audits.append(dict(st.audit, calls=1))
    for a in audits:
        assert am.equal(a, want) == []
    assert capi.qualtypes_consistent(audits[0]) == ["sanger", "solexa", "illumina"]


def test_audit_false_is_the_parent(sk_ctx):
    """audit=False returns what the calls returned before, and audit=True changes no output and no count"""
    _, _, text = drawn_pairs(11, 700, mismatch_at=5)
    params = capi.make_params(*PT)
    same = lambda xs, ys: all((x is None and y is None) or bool((x == y).all()) for x, y in zip(xs, ys))
    for mode in ("se", "pe_interleaved", "pe_combo_all"):
        want = am.audit(PT, [text], mode)
        a = sk_ctx.trim_fastq(params, to_device(text), mode=mode)
        b = sk_ctx.trim_fastq(params, to_device(text), mode=mode, audit=True)
        assert len(a) == len(b) == 2 and "audit" not in a[1] and am.equal(b[1].pop("audit"), want) == []
        assert a[1] == b[1] and same(a[0], b[0])
        g = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode)
        h = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode, audit=True, report=True)
        assert len(g) == 2 and len(h) == 3 and am.equal(h[1].pop("audit"), want) == []
        assert g[1] == h[1] and same(g[0], h[0])
    torch = torch_mod()
    e = sk_ctx.trim_fastq(params, torch.empty(0, dtype=torch.uint8, device="cuda"), mode="pe_interleaved", audit=True)
    assert am.equal(e[1]["audit"], am.audit(PT, [b""], "pe_interleaved")) == [] and e[1]["audit"]["qual_min"] == am.NONE
    o = sk_ctx.trim_fastq(params, to_device(text), mode="pe_interleaved", order=(3, 1500), audit=True)
    units = fo.batch_tables([fo.lines_of(text)], "pe_interleaved", 1500)["units"]
    assert am.equal(o[1]["audit"], am.audit(PT, [text], "pe_interleaved", n_reads=2 * units)) == []


@pytest.mark.parametrize("part", range(10))
def test_drawn_texts(sk_ctx, part):
    """100 texts of tests/soak_fastq.py's generator, ten a case, in plain and piece form: every mode and encoding, malformed
    records, chars out of range, degenerate texts"""
    rng = np.random.default_rng(5200 + part)
    for it in range(10):
        c = soak_fastq.draw(rng)
        pt = tuple(c["params"])
        want = am.audit(pt, c["texts"], c["mode"])
        for form in ("plain", "piece"):
            dev = Dev()
            rc = run(sk_ctx, pt, c["texts"], c["mode"], dev, form=form)
            assert (rc == capi.SK_OK) == bool(want["calls"]), (rc, c["notes"])
            assert am.equal(dev.read(), want) == [], (form, c["notes"])
