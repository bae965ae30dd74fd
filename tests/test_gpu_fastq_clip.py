"""GPU: sk_trim_fastq_clipped_device_async against tests/fastq_clip_model.py.  Every comparison is == with the model.  The
stats struct has guard words behind it, every output a sentinel band behind its capacity, and the workspace lies on
tests/guarded.py's arena, sized to the byte, so that the clip section's last byte has a guard band right behind it."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import combo_all_model as cm
import fastq_adapters_model as am
import fastq_bases_model as bm
import fastq_clip_model as clm
import fastq_model as fm
import fastq_order_model as fo
import fastq_report_model as rm
import guarded
import gunzip_model as gm
from sickle_amd import capi
from fastq_raw import SENTINEL, torch_mod, upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
PATTERN = 0x0101010101010101
GUARD = 4
ROOM = 64
W = capi.CLIP_WORDS
MODES = ("se", "pe_split", "pe_interleaved", "pe_combo_all")
QUALTYPES = ("phred", "sanger", "solexa", "illumina")
TRUSEQ = clm.TRUSEQ
PT = ("sanger", 22, 15, False, False)
KEEP_ALL = ("sanger", 20, 1, False, False)
SEQS3 = [TRUSEQ, b"CTGTCTCTTATACACATCT", b"TGGAATTCTCGGGTGCCAAGG"]
SET3 = clm.make_set(SEQS3, 5, 100)
EXACT = clm.make_set([TRUSEQ], 13, 0)


class Stats:
    """a sk_fastq_clip_stats in device memory, pre-filled with PATTERN, GUARD words behind it"""

    def __init__(self):
        torch = torch_mod()
        self.t = torch.full((W + GUARD,), PATTERN, dtype=torch.int64, device="cuda")
        self.ptr = self.t.data_ptr()

    def words(self):
        w = self.t.cpu().numpy().view(np.uint64)
        assert (w[W:] == PATTERN).all(), "the words behind the stats were written"
        return w[:W]

    def read(self):
        w = self.words()
        assert w[14] == 0 and w[15] == 0, "the reserved words are not zero"
        return capi.FastqClipStats.from_buffer_copy(w.tobytes()).as_dict()


def ws_need(T, trunc_n, form, fo_):
    L = capi.lib()
    if form == "ordered":
        base = L.sk_trim_fastq_ordered_workspace_bytes(T, trunc_n, fo_.batch_capacity)
    else:
        base = L.sk_trim_fastq_workspace_bytes(T, trunc_n)
    return base, base + L.sk_trim_fastq_clip_extra_bytes(T)


def run(ctx, ptuple, texts, mode, st, form="plain", stats=None, reset=True, outs="full", order=None, bound_extra=0, valid=1,
        length=None, shifts=(0, 0), cap_short=0, rec_short=0, clip=True, lead=16, poison="pattern"):
    """One text call on the null stream, clipped (clip=True) or not.  form: "plain", "piece" (more == 0), "chained" (the
    lengths from device words) or "ordered" (order = (threads, batch_len)).  outs: "full" or "count".  -> dict(rc, counts,
    texts, index, words: this call's clip words for the reads the stats name)"""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*ptuple)
    bufs = [upload(t + b"\x01" * bound_extra, s) for t, s in zip(texts, shifts)]
    bounds = [len(t) + bound_extra for t in texts]
    T = sum(bounds)
    cap = capi.fastq_output_bound(T, mode)
    rcap = T // 8 + 2
    keep, arr = [], []
    for o in range(3):
        if outs == "count":
            keep.append(None)
            arr.append(capi.FastqOutput())
            continue
        t = torch.full((max(cap, 16) + ROOM,), SENTINEL, dtype=torch.uint8, device="cuda")
        ix = torch.full((rcap + ROOM,), -7, dtype=torch.int64, device="cuda")
        keep.append((t, ix))
        arr.append(capi.FastqOutput(t.data_ptr(), cap - cap_short, ix.data_ptr(), rcap - rec_short))
    ptrs = [b[1] for b in bufs]
    fo_ = capi.FastqOrder(order[0], 0, order[1], T // order[1] + 16, 0) if form == "ordered" else None
    base, need = ws_need(T, params.trunc_n, form, fo_)
    ws_bytes = need if clip else base
    ar = guarded.arena(ws_bytes, lead, poison, seed=len(texts[0]))
    kw = {}
    if form in ("chained", "piece"):
        lens = [len(t) for t in texts] if length is None else length
        words = torch.tensor([[n, valid] for n in lens], dtype=torch.int64, device="cuda")
        kw = dict(bytes_dev_ptrs=[words.data_ptr() + 16 * i for i in range(len(texts))],
                  valid_dev_ptrs=[words.data_ptr() + 16 * i + 8 for i in range(len(texts))])
    words_ptr = None
    if clip:
        words_ptr = ctx.trim_fastq_clipped_device_async(params, ptrs, bounds, capi.adapter_set(**st), arr, ar.ws.data_ptr(), ws_bytes,
                                                        mode=mode, piece=form == "piece", order=fo_,
                                                        stats_ptr=stats.ptr if stats else None, reset=reset, **kw)
        assert words_ptr == ar.ws.data_ptr() + base + 128, "the clip words lie behind the stats block at the kind's size"
    elif form == "plain":
        ctx.trim_fastq_device_async(params, ptrs, bounds, arr, ar.ws.data_ptr(), ws_bytes, mode=mode)
    elif form == "ordered":
        ctx.trim_fastq_ordered_device_async(params, ptrs, bounds, fo_, arr, ar.ws.data_ptr(), ws_bytes, mode=mode)
    else:
        ctx.trim_fastq_piece_device_async(params, ptrs, bounds, arr, ar.ws.data_ptr(), ws_bytes, mode=mode, piece=form == "piece", **kw)
    c = capi.FastqCounts()
    if form == "piece":
        rc, c, counts = ctx._piece_finish(ar.ws.data_ptr(), None)
    elif form == "ordered":
        oc = capi.FastqOrderCounts()
        rc = L.sk_trim_fastq_ordered_device_finish(ctx._h, ar.ws.data_ptr(), None, C.byref(c), C.byref(oc))
        counts = dict(c.as_dict(), order=oc.as_dict())
    else:
        rc = L.sk_trim_fastq_device_finish(ctx._h, ar.ws.data_ptr(), None, C.byref(c))
        counts = c.as_dict()
    ar.check()
    res = dict(rc=rc, counts=counts, texts=[None] * 3, index=[None] * 3, keep=keep, ws=ar, base=base)
    for o, k in enumerate(keep):
        if k is None:
            continue
        t, ix = k
        assert bool((t[cap - cap_short:] == SENTINEL).all()) and bool((ix[rcap - rec_short:] == -7).all()), "an output's band was written"
        if rc == capi.SK_OK and o in capi.TRIM_OUTPUTS[mode]:
            res["texts"][o] = t[:counts["bytes"][o]].cpu().numpy().tobytes()
            res["index"][o] = ix[:counts["records"][o]].cpu().tolist()
    if clip:
        at = base + 128
        res["all_words"] = ar.ws[at:].cpu().numpy().view(np.uint32)
    return res


def untouched(res):
    for k in res["keep"]:
        if k is not None:
            assert bool((k[0] == SENTINEL).all()) and bool((k[1] == -7).all()), "an output was written after an error"


def check(ctx, ptuple, texts, mode, st, want=None, rc=None, stats=None, **kw):
    """the clipped call against the model: the return code, the outputs, the indices, the stats and the clip words"""
    own = stats is None
    stats = stats or Stats()
    if want is None:
        want = clm.expected(ptuple, texts, mode, st)
    got = run(ctx, ptuple, texts, mode, st, stats=stats, **kw)
    want_rc = capi.SK_EFORMAT if want["verdict"] is not None else capi.SK_ERANGE if want["range"] is not None else capi.SK_OK
    assert got["rc"] == (want_rc if rc is None else rc), (got["rc"], capi.lib().sk_last_error(ctx._h))
    if own:
        assert stats.read() == want["clip"], (stats.read(), want["clip"])
    if want_rc != capi.SK_OK:
        untouched(got)
        return got
    if got["rc"] == capi.SK_OK and kw.get("outs") != "count":
        for o in capi.TRIM_OUTPUTS[mode]:
            assert got["texts"][o] == want["texts"][o], "output %d differs" % o
            assert got["index"][o] == [int(x) for x in want["index"][o]], "index %d differs" % o
    n = len(want["words"])
    assert got["all_words"][:n].tolist() == want["words"], "the clip words differ"
    return got


def rec(name, seq, qual):
    return name + b"\n" + seq + b"\n+\n" + qual + b"\n"


def text_of(reads, start=0):
    return b"".join(rec(b"@r%d" % (start + i), s, q) for i, (s, q) in enumerate(reads))


def texts_of(reads, mode):
    if mode == "pe_split":
        return [text_of(reads[0::2]), text_of(reads[1::2])]
    return [text_of(reads)]


def drawn_reads(seed, n, lens=(20, 120), alphabet=b"ACGTACGTACGTNacgtnR.", seqs=SEQS3, rate=0.5, min_start=0):
    """n reads with drawn lengths, bases and qualities (sanger; lows at either end so that both cuts move), an adapter of
    `seqs` planted into about `rate` of them at a drawn start, with a drawn mismatch now and then"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(alphabet, np.uint8)
    out = []
    for _ in range(n):
        m = int(rng.integers(lens[0], lens[1] + 1)) if isinstance(lens, tuple) else lens
        q = np.clip(int(rng.integers(36, 70)) + rng.integers(-14, 9, m), 33, 73).astype(np.uint8)
        s = bytearray(letters[rng.integers(0, len(letters), m)].tobytes())
        if rng.random() < rate and m > min_start:
            ad = bytearray(seqs[int(rng.integers(0, len(seqs)))])
            if rng.random() < 0.4:
                ad[int(rng.integers(0, len(ad)))] = int(rng.choice(list(b"ACGTNn")))
            p = int(rng.integers(min_start, m))
            s[p:p + len(ad)] = ad[:m - p]
        out.append((bytes(s[:m]), q.tobytes()))
    return out


# ---- the truth table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qualtype", QUALTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_truth_table(sk_ctx, mode, qualtype):
    """the hand table (tests/fastq_clip_model.py): the texts, the indices, the stats and the words written out there"""
    texts, want_texts, want_index = clm.truth(qualtype, mode)
    stats = Stats()
    got = run(sk_ctx, clm.truth_params(qualtype), texts, mode, clm.TRUTH_SET, stats=stats)
    assert got["rc"] == capi.SK_OK and got["texts"] == want_texts and got["index"] == want_index
    assert stats.read() == clm.TRUTH_STATS and got["all_words"][:8].tolist() == clm.TRUTH_WORDS
    check(sk_ctx, clm.truth_params(qualtype), texts, mode, clm.TRUTH_SET)


@pytest.mark.parametrize("qualtype", QUALTYPES)
def test_truth_range_and_n(sk_ctx, qualtype):
    """a quality byte out of range in front of p is SK_ERANGE, behind it SK_OK; an N behind p does not count for -n"""
    p = clm.truth_params(qualtype)
    text, want, bad = clm.truth_range(qualtype, front=False)
    got = check(sk_ctx, p, [text], "se", clm.TRUTH_SET)
    assert got["rc"] == capi.SK_OK and got["texts"][0] == want
    assert run(sk_ctx, p, [text], "se", clm.TRUTH_SET, clip=False)["rc"] == capi.SK_ERANGE  # unclipped, it is an error
    text, want, bad = clm.truth_range(qualtype, front=True)
    stats = Stats()
    got = run(sk_ctx, p, [text], "se", clm.TRUTH_SET, stats=stats, reset=False)
    assert got["rc"] == capi.SK_ERANGE
    untouched(got)
    w = stats.words()
    assert w[1] == PATTERN + 1 and (np.delete(w, 1) == PATTERN).all(), "a failed call moves calls_failed alone"
    text, want = clm.truth_n(qualtype)
    got = check(sk_ctx, clm.truth_params(qualtype, True), [text], "se", clm.TRUTH_SET)
    assert got["texts"][0] == want


# ---- shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 12, 13, 63, 64, 65, 127, 128, 129])
def test_read_lengths_with_the_adapter_at_every_start(sk_ctx, length):
    """reads of one length on the tile edges of 64 starts, the adapter planted at every start, and one read without"""
    rng = np.random.default_rng(length)
    reads = []
    for p in range(length + 1):
        s = bytearray(rng.choice(np.frombuffer(b"CT", np.uint8), length).tobytes())
        s[p:p + 13] = TRUSEQ[:length - p]
        reads.append((bytes(s), b"I" * length))
    for mo in (1, 5, 13):
        st = clm.make_set([TRUSEQ], mo, 0)
        got = check(sk_ctx, KEEP_ALL, [text_of(reads)], "se", st)
        want = [p if length - p >= mo else clm.CLIP_NONE for p in range(length + 1)]
        assert got["all_words"][:length + 1].tolist() == want
    if len(reads) % 2 == 0:
        check(sk_ctx, KEEP_ALL, texts_of(reads, "pe_split"), "pe_split", EXACT)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2047, 2048, 2049])
@pytest.mark.parametrize("which", ["none", "all", "first", "last"])
def test_read_counts(sk_ctx, n, which):
    """a wave's 64 reads, the pack's block of 2 048: none, all, the first and the last read clipped"""
    rng = np.random.default_rng(n)
    reads = []
    for r in range(n):
        m = int(rng.integers(20, 41))
        s = bytearray(rng.choice(np.frombuffer(b"CT", np.uint8), m).tobytes())
        if which == "all" or (which == "first" and r == 0) or (which == "last" and r == n - 1):
            p = int(rng.integers(1, m - 13))
            s[p:p + 13] = TRUSEQ
        reads.append((bytes(s), bytes(rng.integers(40, 74, m).astype(np.uint8))))
    stats = Stats()
    got = check(sk_ctx, PT, [text_of(reads)], "se", EXACT, stats=stats)
    assert stats.read()["reads_clipped"] == {"none": 0, "all": n, "first": 1, "last": 1}[which] and stats.read()["reads"] == n
    if n > 1:
        check(sk_ctx, PT, [text_of(reads)], "pe_interleaved", EXACT)


@pytest.mark.parametrize("mode", MODES)
def test_every_read_emptied(sk_ctx, mode):
    """every read starts with the adapter: nothing is kept, -M writes N records alone, and no check refuses the text"""
    reads = [(TRUSEQ + b"ACGT" * (r % 5), b"I" * (13 + 4 * (r % 5))) for r in range(300)]
    stats = Stats()
    got = check(sk_ctx, ("sanger", 20, 0, False, False), texts_of(reads, mode), mode, EXACT, stats=stats)
    s = stats.read()
    assert got["rc"] == capi.SK_OK and s["reads_emptied"] == s["reads"] == 300
    assert got["counts"]["records"][0] == (300 if mode == "pe_combo_all" else 0)


def test_long_read_with_the_hit_in_its_last_bases(sk_ctx):
    """one 20 000-base read whose only hit is the adapter's first min_overlap bases at its very end"""
    mo = 9
    seq = (b"AC" * 10000)[:20000 - mo] + TRUSEQ[:mo]
    reads = [(b"ACACACAC", b"IIIIIIII"), (seq, b"I" * 20000), (b"ACACACAC", b"IIIIIIII")]
    stats = Stats()
    got = check(sk_ctx, KEEP_ALL, [text_of(reads)], "se", clm.make_set([TRUSEQ], mo, 0), stats=stats)
    assert got["all_words"][:3].tolist() == [clm.CLIP_NONE, 20000 - mo, clm.CLIP_NONE] and stats.read()["bases_clipped"] == mo


def test_hit_across_a_framing_chunk(sk_ctx):
    """a seq line across the 64 KiB framing chunk boundary of the text, with the hit straddling the boundary"""
    head = text_of([(b"ACACACAC", b"IIIIIIII")] * 3)
    name = b"@long\n"
    at = 65536 - len(head) - len(name)
    n = at + 5000
    seq = bytearray(b"AC" * (n // 2 + 1))[:n]
    seq[at - 6:at - 6 + len(TRUSEQ)] = TRUSEQ
    text = head + name + bytes(seq) + b"\n+\n" + b"I" * n + b"\n" + text_of([(b"ACACACAC", b"IIIIIIII")] * 2, 3)
    assert text[65536 - 6:65536 - 6 + 13] == TRUSEQ
    got = check(sk_ctx, KEEP_ALL, [text], "se", EXACT)
    assert got["all_words"][3] == at - 6
    check(sk_ctx, KEEP_ALL, [text, text], "pe_split", EXACT)


@pytest.mark.parametrize("s0", [0, 1, 7, 15])
@pytest.mark.parametrize("s1", [0, 1, 7, 15])
def test_split_alignments(sk_ctx, s0, s1):
    """both texts of a split call at byte offsets 0, 1, 7, 15 from an aligned buffer, independently"""
    check(sk_ctx, PT, texts_of(drawn_reads(1, 300), "pe_split"), "pe_split", SET3, shifts=(s0, s1))


def test_eight_adapters_of_64_bases_and_one_of_1(sk_ctx):
    rng = np.random.default_rng(5)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seqs = [letters[rng.integers(0, 4, 64)].tobytes() for _ in range(8)]
    reads = drawn_reads(6, 300, lens=(1, 200), seqs=seqs, rate=0.7)
    for mo, pm in ((64, 100), (20, 100), (7, 500)):
        check(sk_ctx, PT, [text_of(reads)], "pe_interleaved", clm.make_set(seqs, mo, pm))
    stats = Stats()
    check(sk_ctx, PT, [text_of(reads)], "se", clm.make_set(seqs, 20, 100), stats=stats)
    assert sum(h > 0 for h in stats.read()["hits"]) == 8
    check(sk_ctx, PT, [text_of(reads)], "se", clm.make_set([b"T"], 1, 0))
    check(sk_ctx, PT, [text_of(reads)], "se", clm.make_set([b"t"], 1, 500))
    for n in range(2, 8):
        check(sk_ctx, PT, [text_of(reads)], "se", clm.make_set(seqs[:n], 20, 100))


@pytest.mark.parametrize("trunc_n", [False, True])
@pytest.mark.parametrize("lead", guarded.LEADS)
def test_workspace_guards(sk_ctx, lead, trunc_n):
    """the workspace at every lead of the arena and under every poison, with and without the packed seq"""
    pt, tt = ("sanger", 22, 15, False, trunc_n), [text_of(drawn_reads(7, 700))]
    want = clm.expected(pt, tt, "pe_interleaved", SET3)
    for poison in guarded.POISONS:
        check(sk_ctx, pt, tt, "pe_interleaved", SET3, want=want, lead=lead, poison=poison)


# ---- calls that must write nothing -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "piece", "chained"])
def test_format_errors_write_nothing(sk_ctx, form):
    """a planted format error: nothing is written, only calls_failed moves, and the outputs keep their pattern"""
    reads = drawn_reads(19, 3000, alphabet=b"ACGT")
    for bad in (rec(b"@bad", b"ACGT", b"III"), rec(b"@bad", b"", b""), rec(b"Xbad", b"ACGT", b"IIII")):
        text = text_of(reads[:1400]) + bad + rec(b"@mate", b"C" * 30, b"I" * 30) + text_of(reads[1400:], 1400)
        stats = Stats()
        got = run(sk_ctx, ("sanger", 20, 20, False, False), [text], "pe_interleaved", SET3, form=form, stats=stats, reset=False)
        assert got["rc"] == capi.SK_EFORMAT
        untouched(got)
        w = stats.words()
        assert w[1] == PATTERN + 1 and (np.delete(w, 1) == PATTERN).all(), "a call that does not add wrote something"
    stats = Stats()
    got = run(sk_ctx, PT, texts_of(reads[:10], "se") + texts_of(reads[:8], "se"), "pe_split", SET3, stats=stats)  # SK_FQ_PAIR_COUNT
    assert got["rc"] == capi.SK_EFORMAT and stats.read() == clm.failed()


def test_counting_call_and_short_capacities(sk_ctx):
    """with every output NULL (a counting call), or one short (the finish says SK_ESPACE), the clip is there in full"""
    reads = drawn_reads(17, 1300)
    for mode in ("pe_split", "pe_combo_all"):
        want = clm.expected(KEEP_ALL, texts_of(reads, mode), mode, SET3)
        got = check(sk_ctx, KEEP_ALL, texts_of(reads, mode), mode, SET3, want=want, outs="count")
        used = capi.TRIM_OUTPUTS[mode]
        assert [got["counts"]["bytes"][o] for o in used] == [len(want["texts"][o]) for o in used]
    text = text_of(drawn_reads(18, 300))
    want = clm.expected(PT, [text], "se", SET3)
    need, recs = len(want["texts"][0]), len(want["index"][0])
    bound = capi.fastq_output_bound(len(text), "se")
    for short in (dict(cap_short=bound - need + 1), dict(rec_short=len(text) // 8 + 2 - recs + 1)):
        got = check(sk_ctx, PT, [text], "se", SET3, want=want, rc=capi.SK_ESPACE, **short)
        assert got["counts"]["bytes"][0] == need and got["counts"]["records"][0] == recs
        assert bool((got["keep"][0][0] == SENTINEL).all()), "an output that does not fit is not written"
    check(sk_ctx, PT, [text], "se", SET3, want=want, cap_short=bound - need)  # exactly what it needs


def test_accumulation_and_reset(sk_ctx):
    """two texts with a failed one between them; RESET over a dirty struct; stats_dev NULL"""
    t1 = [text_of(drawn_reads(21, 2500))]
    t2 = texts_of(drawn_reads(22, 900), "pe_split")
    bad = [rec(b"@bad", b"ACGT", b"III")]
    a, b = clm.expected(PT, t1, "pe_interleaved", SET3)["clip"], clm.expected(PT, t2, "pe_split", SET3)["clip"]
    stats = Stats()
    assert run(sk_ctx, PT, t1, "pe_interleaved", SET3, stats=stats, reset=True)["rc"] == capi.SK_OK  # over the pattern
    assert stats.read() == a
    assert run(sk_ctx, PT, bad, "se", SET3, stats=stats, reset=False)["rc"] == capi.SK_EFORMAT
    assert stats.read() == clm.add(a, clm.failed())
    assert run(sk_ctx, PT, t2, "pe_split", SET3, stats=stats, reset=False)["rc"] == capi.SK_OK
    assert stats.read() == clm.add(clm.add(a, clm.failed()), b)
    assert run(sk_ctx, PT, t2, "pe_split", SET3, stats=stats, reset=True)["rc"] == capi.SK_OK
    assert stats.read() == b
    assert run(sk_ctx, PT, bad, "se", SET3, stats=stats, reset=True)["rc"] == capi.SK_EFORMAT
    assert stats.read() == clm.failed()
    want = clm.expected(PT, t2, "pe_split", SET3)
    got = run(sk_ctx, PT, t2, "pe_split", SET3, stats=None)
    assert got["texts"] == want["texts"]


# ---- the other kinds ----------------------------------------------------------------------------------------------------------
def test_chained_call_with_device_lengths(sk_ctx):
    """the length a device word, at a record's end, in front of bytes that hold further records; and valid_dev = 0"""
    import re
    text = text_of(drawn_reads(23, 800))
    ends = [m.end() for m in re.finditer(rb"\n(?=@r)", text)]
    cut = ends[len(ends) // 2 | 1]
    want = clm.expected(PT, [text[:cut]], "pe_interleaved", SET3)
    assert 0 < want["clip"]["reads"] < 800
    check(sk_ctx, PT, [text], "pe_interleaved", SET3, form="chained", length=[cut], bound_extra=77, want=want)
    empty = clm.expected(PT, [b""], "pe_interleaved", SET3)
    check(sk_ctx, PT, [text], "pe_interleaved", SET3, form="chained", valid=0, want=empty)


def test_raw_piece(sk_ctx):
    """the piece call with more == 0 is the whole text"""
    for mode in MODES:
        tt = texts_of(drawn_reads(24, 600), mode)
        check(sk_ctx, PT, tt, mode, SET3, form="piece")


def test_counted_off_in_a_child_process():
    """SK_FQ_COUNTED=0: every per-read step walks the bound; the clipped call gives the same bytes"""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import torch; torch.cuda.is_available()\n"
            "import test_gpu_fastq_clip as t\n"
            "from sickle_amd import capi\n"
            "ctx = capi.Context(device=0, slots=2)\n"
            "for mode in t.MODES:\n"
            "    t.check(ctx, t.PT, t.texts_of(t.drawn_reads(31, 2500), mode), mode, t.SET3)\n"
            "t.check(ctx, t.PT, [b''], 'se', t.SET3)\n"
            "ctx.close(); print('child ok')\n") % (ROOT, os.path.join(ROOT, "tests"))
    pr = subprocess.run([sys.executable, "-c", code], capture_output=True, env=dict(os.environ, SK_FQ_COUNTED="0"), timeout=300)
    assert pr.returncode == 0 and b"child ok" in pr.stdout, pr.stderr.decode()[-3000:]


def drain(st):
    pieces = list(st)
    return [b"".join(p[o] for p in pieces if p[o] is not None) for o in range(3)]


OPTS = dict(seqs=SEQS3, min_overlap=5, max_mismatch_permille=100)


@pytest.mark.parametrize("piece_bytes", [256, 1000, 8192])
def test_stream_driver_against_the_whole_text_call(sk_ctx, piece_bytes):
    """300 pairs in pieces, every mode: the outputs are the whole-text call's, the stats the model's"""
    params = capi.make_params(*PT)
    reads = drawn_reads(24, 600)
    for mode in MODES:
        tt = texts_of(reads, mode)
        want = clm.expected(PT, tt, mode, SET3)
        args = dict(mode=mode, piece_bytes=piece_bytes, room=max(2048, piece_bytes))
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, clip_adapters=OPTS, **args)
        assert st.clip is None
        out = drain(st)
        assert st.pieces > 1 and st.clip == dict(want["clip"], calls=st.pieces)
        assert [out[o] for o in capi.TRIM_OUTPUTS[mode]] == [want["texts"][o] for o in capi.TRIM_OUTPUTS[mode]]
        whole = check(sk_ctx, PT, tt, mode, SET3, want=want)
        assert [out[o] for o in capi.TRIM_OUTPUTS[mode]] == [whole["texts"][o] for o in capi.TRIM_OUTPUTS[mode]]
    with pytest.raises(ValueError):
        sk_ctx.trim_fastq_stream(params, tt[0], mode="se", clip_adapters=dict(OPTS, clip=True))


@pytest.mark.parametrize("mode", ["se", "pe_split"])
def test_gzip_stream_in_pieces_of_8192(sk_ctx, monkeypatch, mode):
    """trim_gzip_stream at the small end: gzip of small blocks read in stretches of 256 bytes, text pieces of 8 192 bytes.
    (trim_gz_stream takes no piece below a BGZF member's 65 536 bytes of text: test_gz_drivers_on_the_golden_inputs.)"""
    monkeypatch.setenv("SK_GZIP_CHUNK", "256")
    tt = texts_of(drawn_reads(28, 600), mode)
    want = clm.expected(PT, tt, mode, SET3)
    images = [gm.small_blocks(t, 6) for t in tt]
    st = sk_ctx.trim_gzip_stream(capi.make_params(*PT), images[0], images[1] if len(images) > 1 else None, mode=mode, piece_bytes=8192,
                                 room=16384, gz=False, clip_adapters=OPTS)
    out = drain(st)
    used = capi.TRIM_OUTPUTS[mode]
    assert st.pieces > 4 and [out[o] for o in used] == [want["texts"][o] for o in used]
    assert st.clip == dict(want["clip"], calls=st.clip["calls"]) and st.clip["calls_failed"] == 0


def ordered_want(ptuple, tt, mode, st, threads, batch_len):
    """the ordered clipped call: the clip model's records of the reads inside the batches, in the -a T order"""
    framing = clm.FRAMING[mode]
    tabs = fo.batch_tables([fo.lines_of(t) for t in tt], framing, batch_len)
    order = fo.read_order(tabs["first_unit"], threads, framing)
    want = clm.expected(ptuple, tt, mode, st, n_reads=len(order))
    recs = cm.records_of(want["buf"], want["recs"], want["cuts"], ptuple[0])
    kept = want["cuts"][:, 1] >= 0
    if mode == "pe_combo_all":
        dest = np.zeros(len(kept), np.int8)
    else:
        dest = fm.dests(want["cuts"], framing)
    texts, index = [None] * 3, [None] * 3
    for o in capi.TRIM_OUTPUTS[mode]:
        sel = [r for r in order if dest[r] == o]
        texts[o], index[o] = b"".join(recs[r] for r in sel), sel
    return dict(want, texts=texts, index=index)


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
    """the -a 3 order at a byte budget of 64: records that short that a batch holds a pair, reads of 2 .. 7 bases against two
    short adapters"""
    rng = np.random.default_rng(64)
    letters = np.frombuffer(b"ACGT", np.uint8)
    records = []
    for k in range(400):
        if k % 2 == 0:
            m = int(rng.integers(2, 8))
        records.append((b"@r%03d" % (k // 2), letters[rng.integers(0, 4, m)].tobytes(), (b"#" if rng.integers(3) == 0 else b"I") * m))
    text = lambda recs: b"".join(rec(n, s, q) for n, s, q in recs)
    st = clm.make_set([b"GT", b"ACG"], 2, 0)
    P1 = ("sanger", 20, 1, False, False)
    for mode, tt in (("se", [text(records)]), ("pe_interleaved", [text(records)]), ("pe_combo_all", [text(records)]),
                     ("pe_split", [text(records[0::2]), text(records[1::2])])):
        want = ordered_want(P1, tt, mode, st, 3, 64)
        assert want["clip"]["reads"] > 300 and want["clip"]["hits"][0] > 20 and want["clip"]["hits"][1] > 20
        check(sk_ctx, P1, tt, mode, st, form="ordered", order=(3, 64), want=want)
        # and in pieces of 256 bytes, four batches or so a piece
        s = sk_ctx.trim_fastq_stream(capi.make_params(*P1), tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=256,
                                     room=2048, order=(3, 64), clip_adapters=dict(seqs=[b"GT", b"ACG"], min_overlap=2, max_mismatch_permille=0))
        out = drain(s)
        used = capi.TRIM_OUTPUTS[mode]
        assert s.pieces > 8 and [out[o] for o in used] == [want["texts"][o] for o in used]
        assert s.clip == dict(want["clip"], calls=s.clip["calls"]) and s.clip["calls"] >= s.pieces


def test_ordered_whole_and_in_pieces(sk_ctx, same_lines):
    params = capi.make_params(*PT)
    batch_len = 1500
    for mode, tt in (("pe_split", same_lines[:2]), ("pe_interleaved", same_lines[2:]), ("pe_combo_all", same_lines[2:])):
        want = ordered_want(PT, tt, mode, EXACT, 3, batch_len)
        check(sk_ctx, PT, tt, mode, EXACT, form="ordered", order=(3, batch_len), want=want)
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode, piece_bytes=4096, room=8192,
                                      order=(3, batch_len), clip_adapters=dict(seqs=[TRUSEQ], min_overlap=13, max_mismatch_permille=0))
        out = drain(st)
        used = capi.TRIM_OUTPUTS[mode]
        assert st.pieces > 1 and [out[o] for o in used] == [want["texts"][o] for o in used]
        assert st.clip == dict(want["clip"], calls=st.clip["calls"]) and st.clip["calls"] >= st.pieces
        a = sk_ctx.trim_fastq(params, *[to_device(t) for t in tt], mode=mode, order=(3, batch_len),
                              clip_adapters=dict(seqs=[TRUSEQ], min_overlap=13, max_mismatch_permille=0))
        assert [a[0][o].cpu().numpy().tobytes() for o in used] == [want["texts"][o] for o in used] and a[1]["clip"] == want["clip"]


def to_device(data):
    torch = torch_mod()
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _golden(name):
    return open(os.path.join(INPUTS, name), "rb").read()


@pytest.mark.parametrize("case", ["test.fastq", "test.f.fastq", "split"])
def test_gz_drivers_on_the_golden_inputs(sk_ctx, case):
    """trim_gz (two-pass from gzip and BGZF, one-pass), trim_fastq_gz, trim_gz_stream and trim_gzip_stream: the texts and
    the stats of the model"""
    mode = "pe_split" if case == "split" else "pe_interleaved" if case == "test.fastq" else "se"
    texts = [_golden("test.f.fastq"), _golden("test.r.fastq")] if case == "split" else [_golden(case)]
    pt = ("illumina", 20, 20, False, False)
    params = capi.make_params(*pt)
    want = clm.expected(pt, texts, mode, EXACT)
    assert want["clip"]["reads_clipped"] > 0
    opts = dict(seqs=[TRUSEQ], min_overlap=13, max_mismatch_permille=0)
    used = capi.TRIM_OUTPUTS[mode]
    plain = [gzip.compress(t, 6) for t in texts]
    bgzf = [sk_ctx.bgzf(to_device(t)).cpu().numpy().tobytes() for t in texts]
    two = lambda xs, f=lambda x: x: (f(xs[0]), f(xs[1]) if len(xs) > 1 else None)
    unzip = lambda im: gzip.decompress(im.cpu().numpy().tobytes())

    def same(out, counts):
        assert counts["clip"] == want["clip"]
        assert [unzip(out[o]) for o in used] == [want["texts"][o] for o in used]
    for images in (plain, bgzf):
        same(*sk_ctx.trim_gz(params, *two(images, to_device), mode=mode, clip_adapters=opts))
    same(*sk_ctx.trim_gz(params, *two(plain, to_device), mode=mode, clip_adapters=opts, text_capacity=[len(t) + 10 for t in texts]))
    same(*sk_ctx.trim_fastq_gz(params, *two(texts, to_device), mode=mode, clip_adapters=opts))
    longest = max(len(line) for t in texts for line in t.split(b"\n"))
    for st in (sk_ctx.trim_gz_stream(params, *two(bgzf), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, clip_adapters=opts),
               sk_ctx.trim_gzip_stream(params, *two(plain), mode=mode, piece_bytes=1 << 17, room=4 * longest + 65536, clip_adapters=opts)):
        out = drain(st)
        assert st.clip == dict(want["clip"], calls=st.clip["calls"]) and st.clip["calls_failed"] == 0
        assert [gzip.decompress(out[o]) for o in used] == [want["texts"][o] for o in used]
    # trim_fastq's clip words: every read's start is the model's
    res = sk_ctx.trim_fastq(params, *two(texts, to_device), mode=mode, clip_adapters=dict(opts, clip=True))
    got = res[1]["clip"]
    assert got.pop("clip").cpu().tolist() == [-1 if w == clm.CLIP_NONE else w & 0xFFFFFF for w in want["words"]]
    assert got.pop("adapter").cpu().tolist() == [-1 if w == clm.CLIP_NONE else w >> 24 for w in want["words"]]
    assert got == want["clip"] and [res[0][o].cpu().numpy().tobytes() for o in used] == [want["texts"][o] for o in used]


def test_clip_adapters_none_is_the_parent(sk_ctx):
    """clip_adapters=None returns what the calls returned before, byte for byte, and the unclipped raw call is untouched by
    the clip's presence in the library: it equals fastq_model"""
    text = text_of(drawn_reads(25, 1400))
    params = capi.make_params(*PT)
    same = lambda xs, ys: all((x is None and y is None) or bool((x == y).all()) for x, y in zip(xs, ys))
    for mode in ("se", "pe_interleaved", "pe_combo_all"):
        a = sk_ctx.trim_fastq(params, to_device(text), mode=mode)
        b = sk_ctx.trim_fastq(params, to_device(text), mode=mode, clip_adapters=None)
        assert a[1] == b[1] and same(a[0], b[0]) and "clip" not in a[1]
        if mode != "pe_combo_all":
            assert a[0][0].cpu().numpy().tobytes() == fm.expected(PT, [text], mode)["texts"][0]
        got = run(sk_ctx, PT, [text], mode, SET3, clip=False)
        assert got["texts"][0] == a[0][0].cpu().numpy().tobytes()
        c = sk_ctx.trim_fastq(params, to_device(text), mode=mode, clip_adapters=OPTS, record_index=True)
        want = clm.expected(PT, [text], mode, SET3)
        assert c[0][0][0].cpu().numpy().tobytes() == want["texts"][0] and c[1]["clip"] == want["clip"]
        assert c[0][0][1].cpu().tolist() == [int(x) for x in want["index"][0]]
    torch = torch_mod()
    e = sk_ctx.trim_fastq(params, torch.empty(0, dtype=torch.uint8, device="cuda"), mode="pe_interleaved", clip_adapters=dict(OPTS, clip=True))
    assert e[1]["clip"].pop("clip").numel() == 0 and e[1]["clip"].pop("adapter").numel() == 0
    assert e[1]["clip"] == dict(clm.zero(), calls=1)


def side_models(want, mode, st, pos_bins):
    """the bases' and the adapters' models fed what the scan saw behind the clip: the clipped seq lines and the cuts"""
    _, seq, offsets = want["batch"]
    data, off = np.asarray(seq, np.uint8).tobytes(), [int(x) for x in offsets]
    lines = [data[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return bm.of_batch(seq, offsets, want["cuts"], pos_bins, gc=True), am.of_reads(lines, want["cuts"], mode != "se", st)


@pytest.mark.parametrize("mode", MODES)
def test_side_calls_on_the_truth_table(sk_ctx, mode):
    """the report, the bases and the adapters behind the clipped call on the hand table: each equals its model fed the
    clipped lengths, and the bases that come in are the table's, written out"""
    pt = clm.truth_params("sanger")
    texts, want_texts, _ = clm.truth("sanger", mode)
    want = clm.expected(pt, texts, mode, clm.TRUTH_SET)
    res, counts, report = sk_ctx.trim_fastq(capi.make_params(*pt), *[to_device(t) for t in texts], mode=mode, clip_adapters=clm.TRUTH_SET,
                                            report=dict(len_bins=32, pos_bins=32), bases=dict(pos_bins=32, gc=True),
                                            adapters=dict(clm.TRUTH_SET))
    used = capi.TRIM_OUTPUTS[mode]
    assert [res[o].cpu().numpy().tobytes() for o in used] == [want_texts[o] for o in used] and counts["clip"] == clm.TRUTH_STATS
    bases, side = side_models(want, mode, clm.TRUTH_SET, 32)
    assert bm.equal(counts["bases"], bases) == []
    assert am.equal(counts["adapters"], side) == []
    assert rm.equal(report, clm.report(want, mode, 32, 32)) == []
    # 0 + 16 + 10 + 0 + 16 + 12 + 4 + 0 bases are left of the eight reads, all of them upper-case A, C, G or T
    assert sum(counts["bases"]["bases_in"]) == sum(counts["bases"]["bases_in"][:4]) == 58 == report["bases_in"]
    assert counts["bases"]["gc_none_in"] == 3  # the three emptied reads have no A, C, G or T


def test_side_calls_behind_a_clipped_call(sk_ctx):
    """the device's own report behind a clipped call is the report's model fed the clipped lengths, and bases_in +
    bases_clipped is the unclipped report's bases_in; the bases count and the adapters search the clipped reads"""
    text = text_of(drawn_reads(26, 1500))
    params = capi.make_params(*PT)
    for mode in ("se", "pe_interleaved", "pe_combo_all"):
        want = clm.expected(PT, [text], mode, SET3)
        res, counts, report = sk_ctx.trim_fastq(params, to_device(text), mode=mode, clip_adapters=OPTS,
                                                report=dict(len_bins=128, pos_bins=128), bases=dict(pos_bins=128, gc=True),
                                                adapters=dict(OPTS))
        assert rm.equal(report, clm.report(want, mode, 128, 128)) == []
        plain = sk_ctx.trim_fastq(params, to_device(text), mode=mode, report=True)[2]
        assert report["bases_in"] + counts["clip"]["bases_clipped"] == plain["bases_in"] == rm.report(PT, [text], mode)["bases_in"]
        # the bases and the adapters behind the clip: their models over the clipped seq lines and the clipped call's cuts
        bases, side = side_models(want, mode, SET3, 128)
        assert bm.equal(counts["bases"], bases) == []
        assert sum(counts["bases"]["bases_in"]) == report["bases_in"]
        assert am.equal(counts["adapters"], side) == []


@pytest.mark.parametrize("mode", MODES)
def test_device_to_device_identity(sk_ctx, mode):
    """the clipped call on a text equals the unclipped call on its truncated text"""
    tt = texts_of(drawn_reads(27, 2000, min_start=1, alphabet=b"ACGTACGTNacgtn"), mode)
    cut = clm.truncated(tt, mode, SET3)
    assert cut is not None
    a = run(sk_ctx, PT, tt, mode, SET3)
    b = run(sk_ctx, PT, cut, mode, SET3, clip=False)
    assert a["rc"] == b["rc"] == capi.SK_OK and a["texts"] == b["texts"] and a["index"] == b["index"]
    assert a["counts"]["records"] == b["counts"]["records"] and a["counts"]["bytes"] == b["counts"]["bytes"]


@pytest.mark.parametrize("part", range(10))
def test_drawn_texts(sk_ctx, part):
    """the 100 drawn texts of tests/fastq_clip_model.py, ten a case, in plain and piece form"""
    st = clm.make_set(**clm.DRAWN_SET)
    for seed in range(10 * part, 10 * part + 10):
        ptuple, texts, mode = clm.drawn(seed)
        want = clm.expected(ptuple, texts, mode, st)
        for form in ("plain", "piece"):
            check(sk_ctx, ptuple, texts, mode, st, want=want, form=form)
