"""GPU: sk_trim_fastq_adapters_device_async against tests/fastq_adapters_model.py.  Every comparison is == with the model;
the struct and every array have guard words behind them, the clip words in front of them too, which must stay untouched."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

import fastq_adapters_model as am
import fastq_model as fm
import fastq_order_model as fo
import soak_fastq
from sickle_amd import capi
from fastq_raw import torch_mod, upload
from test_fastq_adapters_model import EXACT, GAT, HAND, HAND_CLIP, HAND_PAIRS, LINES, READS, SOAK_SEQS, TRUSEQ, finds

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
PATTERN = 0x0101010101010101
CLIP_PATTERN = 0x01010101
GUARD = 4
W = capi.ADAPTERS_WORDS
V = capi.SK_FQ_ADAPTERS_OVERLAP_BINS
KEEP_ALL = ("sanger", 20, 1, False, False)
PT = ("sanger", 22, 15, False, False)
P5 = ("sanger", 20, 5, False, False)
ARRAYS = ("pos", "overlap", "clip")
SET3 = am.make_set(SOAK_SEQS, 5, 100)


class Dev:
    """A sk_fastq_adapters, pos and overlap in one device tensor pre-filled with PATTERN, GUARD words behind each; the clip
    words in a tensor of their own, GUARD words in front of and behind clip_alloc entries of which the call is told
    clip_capacity.  given: the arrays the call is handed (the others are NULL and must keep the pattern); out=False:
    out == NULL."""

    def __init__(self, pos_bins=0, given=ARRAYS, out=True, clip_capacity=4096, clip_alloc=None):
        torch = torch_mod()
        self.P = pos_bins
        self.given = tuple(a for a in given if pos_bins or a != "pos") if out else ()
        sizes = [W, 8 * pos_bins, 8 * V]
        self.at = [0]
        for s in sizes:
            self.at.append(self.at[-1] + s + GUARD)
        self.sizes = sizes
        self.t = torch.full((self.at[-1],), PATTERN, dtype=torch.int64, device="cuda")
        self.ptr = self.t.data_ptr()
        self.cap = clip_capacity
        self.alloc = max(clip_alloc or clip_capacity, clip_capacity)
        self.c = torch.full((self.alloc + 2 * GUARD,), CLIP_PATTERN, dtype=torch.int32, device="cuda")
        ptr = lambda name: self.ptr + 8 * self.at[1 + ARRAYS.index(name)] if name in self.given else None
        clip = self.c.data_ptr() + 4 * GUARD if "clip" in self.given else None
        self.out = capi.FastqAdaptersOut(ptr("pos"), pos_bins, ptr("overlap"), clip, clip_capacity if clip else 0) if out else None

    def words(self):
        w = self.t.cpu().numpy().view(np.uint64)
        for a, s in zip(self.at, self.sizes):
            assert (w[a + s:a + s + GUARD] == PATTERN).all(), "the words behind the struct or an array were written"
        return w

    def clip_words(self):
        c = self.c.cpu().numpy().view(np.uint32)
        assert (c[:GUARD] == CLIP_PATTERN).all() and (c[GUARD + self.alloc:] == CLIP_PATTERN).all(), "the clip guards were written"
        assert (c[GUARD + self.cap:] == CLIP_PATTERN).all(), "a clip word at or beyond clip_capacity was written"
        return c[GUARD:GUARD + self.alloc]

    def read(self):
        """-> the result as the model words it, with the arrays that were given; one that was not must hold the pattern;
        clip: the words as they are"""
        w = self.words()
        r = capi.FastqAdapters.from_buffer_copy(w[:W].tobytes()).as_dict()
        for i, name in enumerate(ARRAYS[:2]):
            a, s = self.at[1 + i], self.sizes[1 + i]
            if name in self.given:
                r[name] = w[a:a + s].reshape(8, -1).copy()
            else:
                assert (w[a:a + s] == PATTERN).all(), "an array that was not given was written"
        self.reserved = int(w[W - 1])
        c = self.clip_words()
        if "clip" not in self.given:
            assert (c == CLIP_PATTERN).all(), "clip was not given and was written"
        self.clip = c
        return r


def run(ctx, ptuple, texts, mode, st, dev, form="plain", reset=True, outs="full", order=None, bound_extra=0, valid=1,
        length=None, adapters_mode=None, shifts=(0, 0), cap_short=0):
    """One text call and the adapter search behind it, on the null stream.  form: "plain", "piece" (the piece call, more ==
    0), "chained" (the lengths from device words) or "ordered" (order = (threads, batch_len)).  outs: "full" or "count"
    (every output NULL).  adapters_mode: the mode the search is told (the call's, if None).  shifts: each text's offset
    from a 16-byte boundary.  cap_short: bytes the output capacities fall short.  -> the finish's return code"""
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
    ctx.trim_fastq_adapters_device_async(ws.data_ptr(), T, params.trunc_n, dev.ptr, ptrs, bounds, capi.adapter_set(**st),
                                         mode=adapters_mode or mode, kind=kind, batch_capacity=fo_.batch_capacity if fo_ else 0,
                                         out=dev.out, reset=reset)
    c = capi.FastqCounts()
    if form == "piece":
        return ctx._piece_finish(ws.data_ptr(), None)[0]
    if form == "ordered":
        return L.sk_trim_fastq_ordered_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(capi.FastqOrderCounts()))
    return L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))


def narrowed(want, dev):
    """the model's result with the arrays the device was given"""
    return {k: v for k, v in want.items() if k not in ARRAYS or k in dev.given}


def clip_is(dev, want):
    """the clip words against the model's: the reads below clip_capacity, and nothing else"""
    if "clip" not in dev.given:
        return
    words = am.clip_words(want) if want["calls"] else []
    n = min(len(words), dev.cap)
    assert dev.clip[:n].tolist() == words[:n], "the clip words differ"
    assert (dev.clip[n:] == CLIP_PATTERN).all(), "a clip word at or beyond the call's reads was written"


def check(ctx, ptuple, texts, mode, st, pos_bins=64, want=None, rc=capi.SK_OK, given=ARRAYS, out=True, clip_capacity=4096,
          clip_alloc=None, **kw):
    dev = Dev(pos_bins, given, out, clip_capacity, clip_alloc)
    got_rc = run(ctx, ptuple, texts, mode, st, dev, **kw)
    assert got_rc == rc, (got_rc, capi.lib().sk_last_error(ctx._h))
    if want is None:
        want = am.adapters(ptuple, texts, mode, st, pos_bins, overlap=True)
    got = dev.read()
    show = lambda r: {k: r[k] for k in am.SCALARS + ("hits",)}
    assert am.equal(got, narrowed(want, dev)) == [], (show(got), show(want))
    assert dev.reserved == 0, "the reserved word is not zero"
    clip_is(dev, want)
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


def drawn_reads(seed, n, lens=(20, 120), alphabet=b"ACGTACGTACGTNacgtnR.", seqs=SOAK_SEQS, rate=0.5):
    """n reads with drawn lengths, bases and qualities (sanger; lows at either end so that both cuts move), an adapter of
    `seqs` planted into about `rate` of them at a drawn start, with a drawn mismatch now and then"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, np.uint8)
    out = []
    for _ in range(n):
        m = int(rng.integers(lens[0], lens[1] + 1)) if isinstance(lens, tuple) else lens
        q = np.clip(int(rng.integers(36, 70)) + rng.integers(-14, 9, m), 33, 73).astype(np.uint8)
        s = bytearray(letters[rng.integers(0, len(letters), m)].tobytes())
        if rng.random() < rate:
            ad = bytearray(seqs[int(rng.integers(0, len(seqs)))])
            if rng.random() < 0.4:
                ad[int(rng.integers(0, len(ad)))] = int(rng.choice(list(b"ACGTNn")))
            p = int(rng.integers(0, m))
            s[p:p + len(ad)] = ad[:m - p]
        out.append((bytes(s[:m]), q.tobytes()))
    return out


# ---- the truth table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["se", "pe_split", "pe_interleaved", "pe_combo_all"])
def test_truth_table(sk_ctx, mode):
    """the hand table's call (tests/test_fastq_adapters_model.py): the numbers written out there"""
    got = check(sk_ctx, P5, texts_of(READS, mode), mode, GAT, pos_bins=7)
    want = dict(HAND, **(HAND_PAIRS if mode != "se" else dict(pairs_both=0, pairs_one=0, pairs_same_clip=0)))
    assert {k: got[k] for k in want} == want
    dev = Dev(7)
    assert run(sk_ctx, P5, texts_of(READS, mode), mode, GAT, dev) == capi.SK_OK
    dev.read()
    assert dev.clip[:8].tolist() == [am.CLIP_NONE if h is None else h[0] << 24 | h[1] for h in HAND_CLIP]


@pytest.mark.parametrize("mode", ["se", "pe_split", "pe_interleaved", "pe_combo_all"])
def test_truth_table_lines(sk_ctx, mode):
    """every line of the hand table as a call of its own (its mate: the same line), the hit by hand"""
    for name, seqs, mo, pm, line, hit in LINES:
        st = am.make_set(seqs, mo, pm)
        reads = [(line, b"I" * len(line))] * 2
        dev = Dev(16)
        assert run(sk_ctx, KEEP_ALL, texts_of(reads, mode), mode, st, dev) == capi.SK_OK, name
        got = dev.read()
        want_word = am.CLIP_NONE if hit is None else hit[0] << 24 | hit[1]
        assert dev.clip[:2].tolist() == [want_word] * 2 and (dev.clip[2:] == CLIP_PATTERN).all(), name
        assert (got["reads"], got["reads_hit"], got["mismatches"]) == (2, 0 if hit is None else 2, 0 if hit is None else 2 * hit[3]), name
        if hit is not None:
            assert got["overlap"][hit[0]][hit[2]] == 2 and got["hits"][hit[0]] == 2 and got["bases_behind"] == 2 * (len(line) - hit[1]), name
            assert got["pairs_same_clip"] == (0 if mode == "se" else 1), name


# ---- alignment and counts ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s0", [0, 1, 7, 15])
@pytest.mark.parametrize("s1", [0, 1, 7, 15])
def test_split_alignments(sk_ctx, s0, s1):
    """both texts of a split call at byte offsets 0, 1, 7, 15 from an aligned buffer, independently"""
    check(sk_ctx, PT, texts_of(drawn_reads(1, 300), "pe_split"), "pe_split", SET3, shifts=(s0, s1))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049])
def test_read_counts(sk_ctx, n):
    reads = drawn_reads(2, n, lens=(1, 40))
    got = check(sk_ctx, PT, [text_of(reads)], "se", SET3, pos_bins=33)
    assert got["reads"] == n
    if n > 1:
        got = check(sk_ctx, PT, [text_of(reads)], "pe_interleaved", SET3, pos_bins=33)
        assert got["reads"] == n & ~1


@pytest.mark.parametrize("length", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129])
def test_read_lengths(sk_ctx, length):
    """reads of one length around the tile of 64 starts, the adapters planted at drawn starts"""
    for mo in (1, 3, 13):
        reads = drawn_reads(3 + length, 400, lens=length, rate=0.8)
        got = check(sk_ctx, ("sanger", 22, 1, False, False), [text_of(reads)], "se", am.make_set(SOAK_SEQS, mo, 100), pos_bins=130,
                    shifts=(mo, 0))
        assert length < mo or got["reads_hit"] > 0
    check(sk_ctx, PT, texts_of(reads, "pe_split"), "pe_split", SET3, pos_bins=130)


def test_long_read_with_the_hit_in_its_last_bases(sk_ctx):
    """one 20 000-base read whose only hit is the adapter's first min_overlap bases at its very end"""
    mo = 9
    seq = b"AC" * 10000
    seq = seq[:20000 - mo] + TRUSEQ[:mo]
    reads = [(b"ACACACAC", b"IIIIIIII"), (seq, b"I" * 20000), (b"ACACACAC", b"IIIIIIII")]
    st = am.make_set([TRUSEQ], mo, 0)
    got = check(sk_ctx, KEEP_ALL, [text_of(reads)], "se", st, pos_bins=2048)
    assert got["reads_hit"] == 1 and got["bases_behind"] == mo and got["pos"][0][2047] == 1 and got["overlap"][0][mo] == 1
    assert got["hits_full"] == 0


def test_hit_across_a_framing_chunk(sk_ctx):
    """a seq line across the 64 KiB framing chunk boundary of the text, with the hit straddling the boundary"""
    head = text_of([(b"ACACACAC", b"IIIIIIII")] * 3)
    name = b"@long\n"
    at = 65536 - len(head) - len(name)  # the line's byte at the boundary
    n = at + 5000
    seq = bytearray(b"AC" * (n // 2 + 1))[:n]
    seq[at - 6:at - 6 + len(TRUSEQ)] = TRUSEQ
    text = head + name + bytes(seq) + b"\n+\n" + b"I" * n + b"\n" + text_of([(b"ACACACAC", b"IIIIIIII")] * 2, 3)
    assert text[65536 - 6:65536 - 6 + 13] == TRUSEQ
    got = check(sk_ctx, KEEP_ALL, [text], "se", EXACT, pos_bins=2048)
    assert got["reads_hit"] == 1 and got["bases_behind"] == n - (at - 6)
    check(sk_ctx, KEEP_ALL, [text, text], "pe_split", EXACT, pos_bins=2048)


def test_one_base_reads(sk_ctx):
    rng = np.random.default_rng(4)
    reads = [(bytes([int(b)]), bytes([int(rng.integers(33, 74))])) for b in rng.choice(list(b"ACGTNacgtn."), 9001)]
    st = am.make_set([b"G"], 1, 0)
    got = check(sk_ctx, KEEP_ALL, [text_of(reads)], "se", st, pos_bins=2, clip_capacity=9001)
    assert got["reads"] == 9001 and got["reads_hit"] == sum(s in (b"G", b"g") for s, _ in reads) == got["hits_at_0"]
    assert check(sk_ctx, ("sanger", 30, 1, False, False), [text_of(reads)], "pe_interleaved", st, pos_bins=1, clip_capacity=9000)["reads"] == 9000


def test_eight_adapters_of_64_bases_and_one_of_1(sk_ctx):
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seqs = [letters[rng.integers(0, 4, 64)].tobytes() for _ in range(8)]
    reads = drawn_reads(6, 300, lens=(1, 200), seqs=seqs, rate=0.7)
    for mo, pm in ((64, 100), (20, 100), (1, 0), (7, 500)):
        got = check(sk_ctx, PT, [text_of(reads)], "pe_interleaved", am.make_set(seqs, mo, pm), pos_bins=200)
        assert got["reads_hit"] > 0
    assert sum(h > 0 for h in check(sk_ctx, PT, [text_of(reads)], "se", am.make_set(seqs, 20, 100))["hits"]) == 8
    check(sk_ctx, PT, [text_of(reads)], "se", am.make_set([b"T"], 1, 0), pos_bins=200)
    check(sk_ctx, PT, [text_of(reads)], "se", am.make_set([b"t"], 1, 500), pos_bins=200)


# ---- limits and NULLs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pos_bins", [1, 2, 150, 151, capi.SK_FQ_ADAPTERS_MAX_POS_BINS])
def test_pos_bins(sk_ctx, pos_bins):
    reads = drawn_reads(12, 400, lens=150) + drawn_reads(13, 5, lens=2500)
    check(sk_ctx, PT, [text_of(reads)], "se", SET3, pos_bins=pos_bins)


@pytest.mark.parametrize("missing", ARRAYS + ("all", "out"))
def test_null_arrays(sk_ctx, missing):
    reads = drawn_reads(14, 500)
    given = () if missing in ("all", "out") else tuple(a for a in ARRAYS if a != missing)
    check(sk_ctx, PT, [text_of(reads)], "pe_interleaved", SET3, pos_bins=64, given=given, out=missing != "out")


@pytest.mark.parametrize("capacity", [1, 499, 500, 501, 4096])
def test_clip_capacity(sk_ctx, capacity):
    """below, at and above the call's 500 reads: the words behind the capacity, and behind the reads, keep the pattern"""
    reads = drawn_reads(15, 500)
    got = check(sk_ctx, PT, [text_of(reads)], "se", SET3, clip_capacity=capacity, clip_alloc=4096)
    assert got["reads"] == 500


# ---- options ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no5,trunc_n", [(False, True), (True, False), (True, True)])
def test_options(sk_ctx, no5, trunc_n):
    """-x and -n move the cuts, not the hits: the bytes are the text's"""
    reads = drawn_reads(16, 800)
    for mode in ("se", "pe_combo_all"):
        got = check(sk_ctx, ("sanger", 22, 15, no5, trunc_n), [text_of(reads)], mode, SET3, pos_bins=121)
        base = am.adapters(PT, [text_of(reads)], mode, SET3)
        assert got["reads_hit"] == base["reads_hit"] and got["bases_behind"] == base["bases_behind"]


# ---- calls that must touch nothing ------------------------------------------------------------------------------------------
def only_calls_failed(dev):
    w = dev.words()
    assert w[1] == PATTERN + 1
    assert (np.delete(w, 1) == PATTERN).all(), "a call that does not add wrote something"
    assert (dev.clip_words() == CLIP_PATTERN).all(), "a call that does not add wrote clip words"


def test_counting_call_and_short_capacities(sk_ctx):
    """with every output NULL (a counting call), or a byte short (the finish says SK_ESPACE), the search is there in full"""
    reads = drawn_reads(17, 1300)
    for mode in ("pe_split", "pe_combo_all"):
        check(sk_ctx, KEEP_ALL, texts_of(reads, mode), mode, SET3, outs="count")
    text = text_of(drawn_reads(18, 300))
    need = len(fm.expected(PT, [text], "se")["texts"][0])
    check(sk_ctx, PT, [text], "se", SET3, rc=capi.SK_ESPACE, cap_short=capi.fastq_output_bound(len(text), "se") - need + 1)


@pytest.mark.parametrize("what", ["format", "range"])
@pytest.mark.parametrize("form", ["plain", "piece"])
def test_failed_calls_touch_nothing(sk_ctx, what, form):
    reads = drawn_reads(19, 3000, alphabet=b"ACGT")
    bad = rec(b"@bad", b"ACGT", b"III") if what == "format" else rec(b"@low", b"A" * 41, b"I" * 20 + b" " + b"I" * 20)
    text = text_of(reads[:1400]) + bad + rec(b"@mate", b"C" * 30, b"I" * 30) + text_of(reads[1400:], 1400)
    dev = Dev(64)
    rc = run(sk_ctx, ("sanger", 20, 20, False, False), [text], "pe_interleaved", SET3, dev, form=form, reset=False)
    assert rc == (capi.SK_EFORMAT if what == "format" else capi.SK_ERANGE)
    only_calls_failed(dev)


def test_mode_that_disagrees(sk_ctx):
    reads = drawn_reads(20, 80)
    text = [text_of(reads)]
    for call_mode, told in (("pe_interleaved", "se"), ("se", "pe_interleaved"), ("pe_combo_all", "se")):
        dev = Dev(64)
        assert run(sk_ctx, KEEP_ALL, text, call_mode, SET3, dev, reset=False, adapters_mode=told) == capi.SK_OK
        only_calls_failed(dev)
    # SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED: either name fits either call
    want = am.adapters(KEEP_ALL, text, "pe_interleaved", SET3, 64, True)
    check(sk_ctx, KEEP_ALL, text, "pe_combo_all", SET3, adapters_mode="pe_interleaved", want=want)
    check(sk_ctx, KEEP_ALL, text, "pe_interleaved", SET3, adapters_mode="pe_combo_all", want=want)


def test_accumulation(sk_ctx):
    """two texts with a failed one between them; RESET over a dirty struct; clip is the last adding call's alone"""
    t1 = [text_of(drawn_reads(21, 2500))]
    t2 = texts_of(drawn_reads(22, 900), "pe_split")
    bad = [rec(b"@bad", b"ACGT", b"III")]
    a, b = am.adapters(PT, t1, "pe_interleaved", SET3, 64, True), am.adapters(PT, t2, "pe_split", SET3, 64, True)
    f = am.failed(64, True)
    dev = Dev(64)
    assert run(sk_ctx, PT, t1, "pe_interleaved", SET3, dev, reset=True) == capi.SK_OK  # over the pattern
    assert am.equal(dev.read(), a) == []
    clip_is(dev, a)
    assert run(sk_ctx, PT, bad, "se", SET3, dev, reset=False) == capi.SK_EFORMAT
    assert am.equal(dev.read(), am.add(a, f)) == []
    clip_is(dev, a)
    assert run(sk_ctx, PT, t2, "pe_split", SET3, dev, reset=False) == capi.SK_OK
    assert am.equal(dev.read(), am.add(am.add(a, f), b)) == []
    assert dev.clip[:900].tolist() == am.clip_words(b) and dev.clip[900:2500].tolist() == am.clip_words(a)[900:]
    assert run(sk_ctx, PT, t2, "pe_split", SET3, dev, reset=True) == capi.SK_OK
    assert am.equal(dev.read(), b) == [] and dev.reserved == 0
    assert run(sk_ctx, PT, bad, "se", SET3, dev, reset=True) == capi.SK_EFORMAT
    assert am.equal(dev.read(), f) == []


# ---- the other kinds ----------------------------------------------------------------------------------------------------------
def test_chained_call(sk_ctx):
    """the length a device word, at a record's end; and valid_dev = 0"""
    text = text_of(drawn_reads(23, 800))
    ends = [m.end() for m in re.finditer(rb"\n(?=@r)", text)]
    cut = ends[len(ends) // 2 | 1]  # an even number of records in front of it
    want = am.adapters(PT, [text[:cut]], "pe_interleaved", SET3, 64, True)
    assert 0 < want["reads"] < 800
    check(sk_ctx, PT, [text], "pe_interleaved", SET3, form="chained", length=[cut], bound_extra=77, want=want)
    check(sk_ctx, PT, [text], "pe_interleaved", SET3, form="chained", valid=0, want=dict(am.zero(64, True), calls=1))


def drain(st):
    pieces = list(st)
    return [b"".join(p[o] for p in pieces if p[o] is not None) for o in range(3)]


def as_stream(want, got):
    """the whole-text model with the calls of the stream: the pieces that added"""
    return dict(want, calls=got["calls"])


OPTS = dict(seqs=SOAK_SEQS, min_overlap=5, max_mismatch_permille=100, pos_bins=130, overlap=True)


@pytest.mark.parametrize("piece_bytes", [256, 1000, 8192])
def test_stream_driver(sk_ctx, piece_bytes):
    """300 pairs in pieces, split, interleaved and -M: one result for the file, and adapters=False is the parent"""
    params = capi.make_params(*PT)
    reads = drawn_reads(24, 600)
    for mode in ("pe_split", "pe_interleaved", "pe_combo_all"):
        tt = texts_of(reads, mode)
        args = dict(mode=mode, piece_bytes=piece_bytes, room=max(2048, piece_bytes))
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, adapters=OPTS, **args)
        assert st.adapters is None
        out = drain(st)
        assert st.pieces > 1 and st.adapters["calls"] == st.pieces and st.adapters["calls_failed"] == 0
        assert am.equal(st.adapters, as_stream(am.adapters(PT, tt, mode, SET3, 130, True), st.adapters)) == []
        plain = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, **args)
        assert drain(plain) == out and plain.adapters is None and plain.counts == st.counts
    with pytest.raises(ValueError):
        sk_ctx.trim_fastq_stream(params, tt[0], mode="se", adapters=dict(OPTS, clip=True))


@pytest.fixture(scope="module")
def same_lines():
    """two inputs whose lines have the same lengths, so that the reference's reader cuts them into the same batches"""
    rng = np.random.default_rng(8)
    letters = np.frombuffer(b"ACGTNacgtn", np.uint8)
    t = [[], []]
    for k, m in enumerate(rng.integers(20, 120, 300)):
        for i in range(2):
            q = np.clip(50 + rng.integers(-14, 9, int(m)), 33, 73).astype(np.uint8).tobytes()
            s = bytearray(letters[rng.integers(0, 10, int(m))].tobytes())
            if rng.random() < 0.5:
                p = int(rng.integers(0, int(m)))
                s[p:p + 13] = TRUSEQ[:int(m) - p]
            t[i].append(rec(b"@r%03d/%d" % (k, i + 1), bytes(s), q))
    return [b"".join(t[0]), b"".join(t[1]), b"".join(a + b for a, b in zip(*t))]


def test_ordered_call_at_3_64(sk_ctx):
    """the -a 3 order at a byte budget of 64: records that short that a batch holds a pair, drawn bases of 2 .. 7 a read
    against two short adapters; a pair that uses a whole budget up ends the run, and the records behind it are no reads"""
    rng = np.random.default_rng(64)
    letters = np.frombuffer(b"ACGT", np.uint8)
    records = []
    for k in range(600):
        if k % 2 == 0:
            m = int(rng.integers(2, 8))
        records.append((b"@r%03d" % (k // 2), letters[rng.integers(0, 4, m)].tobytes(), (b"#" if rng.integers(3) == 0 else b"I") * m))
    records[400] = records[401] = (b"@" + b"s" * 33, b"A" * 34, b"#" * 34)
    text = lambda recs: b"".join(rec(n, s, q) for n, s, q in recs)
    st = am.make_set([b"GT", b"ACG"], 2, 0)
    for mode, tt in (("se", [text(records)]), ("pe_interleaved", [text(records)]), ("pe_split", [text(records[0::2]), text(records[1::2])])):
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, 64)["units"]
        n_reads = units * (1 if mode == "se" else 2)
        assert 300 < n_reads <= 400
        want = am.adapters(P5, tt, mode, st, 8, True, n_reads=n_reads)
        assert want["reads"] == n_reads and want["hits"][0] > 20 and want["hits"][1] > 20
        check(sk_ctx, P5, tt, mode, st, pos_bins=8, form="ordered", order=(3, 64), want=want)


@pytest.mark.parametrize("order", [(1, 1500), (16, 1500)])
def test_ordered_call(sk_ctx, same_lines, order):
    """the -a T order: the reads inside the batches, numbered in read order; the order plays no part"""
    threads, batch_len = order
    for mode, tt in (("pe_split", same_lines[:2]), ("pe_interleaved", same_lines[2:]), ("se", same_lines[2:])):
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        n_reads = units * (1 if mode == "se" else 2)
        assert n_reads > 100
        check(sk_ctx, PT, tt, mode, SET3, form="ordered", order=(threads, batch_len),
              want=am.adapters(PT, tt, mode, SET3, 64, True, n_reads=n_reads))


def test_ordered_stream_driver(sk_ctx, same_lines):
    params = capi.make_params(*PT)
    batch_len = 1500
    for mode, tt in (("pe_split", same_lines[:2]), ("pe_interleaved", same_lines[2:])):
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, batch_len)["units"]
        want = am.adapters(PT, tt, mode, SET3, 130, True, n_reads=2 * units)
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=4096, room=8192,
                                      order=(3, batch_len), adapters=OPTS)
        drain(st)
        assert st.adapters["calls"] >= st.pieces > 1 and am.equal(st.adapters, as_stream(want, st.adapters)) == []


def to_device(data):
    torch = torch_mod()
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _golden(name):
    return open(os.path.join(INPUTS, name), "rb").read()


@pytest.mark.parametrize("case", ["test.fastq", "test.f.fastq", "test.r.fastq", "split"])
def test_gz_drivers_on_the_golden_inputs(sk_ctx, case):
    """trim_gz (two-pass from gzip and BGZF, one-pass), trim_gz_stream and trim_gzip_stream: the reads bytes.find sees"""
    mode = "pe_split" if case == "split" else "pe_interleaved" if case == "test.fastq" else "se"
    texts = [_golden("test.f.fastq"), _golden("test.r.fastq")] if case == "split" else [_golden(case)]
    found = [finds(t) for t in texts]
    n = sum(f >= 0 for fs in found for f in fs)
    pt = ("illumina", 20, 20, False, False)
    params = capi.make_params(*pt)
    want = am.adapters(pt, texts, mode, EXACT, 151, True)
    opts = dict(seqs=[TRUSEQ], min_overlap=13, max_mismatch_permille=0, pos_bins=151, overlap=True)
    plain = [gzip.compress(t, 6) for t in texts]
    bgzf = [sk_ctx.bgzf(to_device(t)).cpu().numpy().tobytes() for t in texts]
    two = lambda xs, f=lambda x: x: (f(xs[0]), f(xs[1]) if len(xs) > 1 else None)
    results = []
    for images in (plain, bgzf):
        out, counts = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode, adapters=opts)
        results.append(counts.pop("adapters"))
        out2, counts2 = sk_ctx.trim_gz(params, *two(images, to_device), mode=mode)
        assert counts2 == counts and all((a is None and b is None) or bool((a == b).all()) for a, b in zip(out, out2))
    out, counts = sk_ctx.trim_gz(params, *two(plain, to_device), mode=mode, adapters=opts, text_capacity=[len(t) + 10 for t in texts])
    results.append(counts["adapters"])
    longest = max(len(line) for t in texts for line in t.split(b"\n"))
    for st in (sk_ctx.trim_gz_stream(params, *two(bgzf), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, adapters=opts),
               sk_ctx.trim_gzip_stream(params, *two(plain), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, adapters=opts)):
        list(st)
        assert st.adapters["calls"] >= 1 and st.adapters["calls_failed"] == 0
        results.append(dict(st.adapters, calls=1))
    for r in results:
        assert am.equal(r, want) == []
        assert r["reads_hit"] == n == r["hits_full"] and int(r["pos"][0].sum()) == n and r["mismatches"] == 0
    # trim_fastq's clip: every read's start is the find's (the reads of a split call alternate between the texts)
    res = sk_ctx.trim_fastq(params, *two(texts, to_device), mode=mode, adapters=dict(opts, clip=True))
    got = res[1]["adapters"]
    per_read = [f for pair in zip(*found) for f in pair] if case == "split" else found[0]
    assert got["clip"].cpu().tolist() == per_read and got["adapter"].cpu().tolist() == [0 if f >= 0 else -1 for f in per_read]
    assert am.equal({k: v for k, v in got.items() if k not in ("clip", "adapter")}, want) == []


def test_adapters_false_is_the_parent_and_report_agrees(sk_ctx):
    """adapters=False returns what the calls returned before, adapters= changes no output and no count, and with report=
    as well reads and kept are the device's own report's"""
    text = text_of(drawn_reads(25, 1400))
    params = capi.make_params(*PT)
    same = lambda xs, ys: all((x is None and y is None) or bool((x == y).all()) for x, y in zip(xs, ys))
    for mode in ("se", "pe_interleaved", "pe_combo_all"):
        want = am.adapters(PT, [text], mode, SET3, 130, True)
        a = sk_ctx.trim_fastq(params, to_device(text), mode=mode)
        b = sk_ctx.trim_fastq(params, to_device(text), mode=mode, adapters=dict(OPTS, clip=True), report=True)
        assert len(a) == 2 and len(b) == 3 and "adapters" not in a[1]
        got = b[1].pop("adapters")
        clip, adapter = got.pop("clip").cpu().tolist(), got.pop("adapter").cpu().tolist()
        assert am.equal(got, want) == [] and a[1] == b[1] and same(a[0], b[0])
        assert clip == [-1 if h is None else h[1] for h in want["clip"]] and adapter == [-1 if h is None else h[0] for h in want["clip"]]
        assert (got["calls"], got["calls_failed"], got["reads"], got["kept"]) == tuple(b[2][k] for k in ("calls", "calls_failed", "reads", "kept"))
        g = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode)
        h = sk_ctx.trim_fastq_gz(params, to_device(text), mode=mode, adapters=dict(seqs=SOAK_SEQS, min_overlap=5), audit=True)
        assert len(g) == len(h) == 2 and am.equal(h[1].pop("adapters"), am.adapters(PT, [text], mode, SET3)) == []
        h[1].pop("audit")
        assert g[1] == h[1] and same(g[0], h[0])
    torch = torch_mod()
    e = sk_ctx.trim_fastq(params, torch.empty(0, dtype=torch.uint8, device="cuda"), mode="pe_interleaved", adapters=dict(OPTS, clip=True))
    assert am.equal({k: v for k, v in e[1]["adapters"].items() if k not in ("clip", "adapter")}, dict(am.zero(130, True), calls=1)) == []
    assert e[1]["adapters"]["clip"].numel() == 0
    o = sk_ctx.trim_fastq(params, to_device(text), mode="pe_interleaved", order=(3, 1500), adapters=OPTS)
    units = fo.batch_tables([fo.lines_of(text)], "pe_interleaved", 1500)["units"]
    assert am.equal(o[1]["adapters"], am.adapters(PT, [text], "pe_interleaved", SET3, 130, True, n_reads=2 * units)) == []
    st = sk_ctx.trim_fastq_stream(params, text, mode="pe_interleaved", piece_bytes=20000, room=4096, adapters=OPTS, report=True)
    list(st)
    assert {k: st.report[k] for k in ("reads", "kept")} == {k: st.adapters[k] for k in ("reads", "kept")}


@pytest.mark.parametrize("part", range(10))
def test_drawn_texts(sk_ctx, part):
    """100 texts of tests/soak_fastq.py's generator with adapters planted, ten a case, in plain and piece form: every mode
    and encoding, malformed records, chars out of range, degenerate texts"""
    rng = np.random.default_rng(5700 + part)
    for it in range(10):
        c = soak_fastq.draw(rng)
        texts = [am.plant(rng, t, SOAK_SEQS) for t in c["texts"]]
        pt = tuple(c["params"])
        bins = int(rng.choice([1, 7, 64, 300]))
        st = am.make_set(SOAK_SEQS, int(rng.integers(1, 14)), int(rng.choice([0, 100, 200])))
        want = am.adapters(pt, texts, c["mode"], st, bins, True)
        for form in ("plain", "piece"):
            dev = Dev(bins, clip_capacity=max(want["reads"], 1) + 3)
            rc = run(sk_ctx, pt, texts, c["mode"], st, dev, form=form)
            assert (rc == capi.SK_OK) == bool(want["calls"]), (rc, c["notes"])
            assert am.equal(dev.read(), want) == [], (form, c["notes"])
            clip_is(dev, want)
