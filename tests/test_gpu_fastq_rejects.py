"""GPU: sk_trim_fastq_rejects_device_async against tests/fastq_rejects_model.py.  Every comparison is == with the model.  The
text buffer and the index carry a pattern that must survive behind `bytes` and behind `records`, and the call's workspace
lies on tests/guarded.py's arena: a base that is 16-byte aligned and no more, pattern bands around it, and the fills of
tests/test_gpu_workspace.py (zeros, random bytes, 0xFF, a larger call's leftovers)."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import fastq_model as fm
import fastq_order_model as fo
import fastq_piece_model as pm
import fastq_rejects_model as jm
import guarded as gd
from fastq_raw import torch_mod, upload
from sickle_amd import capi
from test_fastq_rejects_model import K, PAIRS, TABLE, X, text_of, texts_for, want_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
ROOM = 64                       # pattern bytes behind the text's capacity, pattern entries behind the index's
INDEX_PATTERN = 0x0706050403020100
P5 = ("sanger", 20, 5, False, False)
ALL_LOST = ("sanger", 20, 1 << 20, False, False)  # -l above every read length: every read is rejected
LEGS = [(16, "zeros"), (48, "pattern"), (240, "ones"), (16, "leftover"), (48, "ones"), (240, "pattern")]


def byte_pattern(n):
    torch = torch_mod()
    i = torch.arange(n, dtype=torch.int64, device="cuda")
    return ((i * 37 + 11) & 0xFF).to(torch.uint8)


class Out:
    """the rejects' text buffer and index, patterned; cap and rec_cap are what the call is told, ROOM lies behind each"""

    def __init__(self, cap, rec_cap, index=True):
        torch = torch_mod()
        self.cap, self.rec_cap = cap, rec_cap
        self.text = byte_pattern(cap + ROOM)
        self.index = torch.full((rec_cap + ROOM,), INDEX_PATTERN, dtype=torch.int64, device="cuda") if index else None
        self.struct = capi.FastqOutput(self.text.data_ptr(), cap, self.index.data_ptr() if index else None, rec_cap)

    def read(self, n_bytes, n_records):
        """-> (text, index) of what was written; everything behind must be the pattern"""
        assert bool((self.text[n_bytes:] == byte_pattern(self.cap + ROOM)[n_bytes:]).all()), "the text buffer was written behind `bytes`"
        idx = None
        if self.index is not None:
            assert bool((self.index[n_records:] == INDEX_PATTERN).all()), "the index was written behind `records`"
            idx = self.index[:n_records].cpu().numpy()
        return self.text[:n_bytes].cpu().numpy().tobytes(), idx


def run(ctx, ptuple, texts, mode, pairs=False, form="plain", out=None, shifts=(0, 0), leg=(16, "zeros"), seed=0, arena=None,
        call_mode=None, order=None, bound_extra=0, behind=b"\x01", length=None, more=False, text_outs=False):
    """One text call and the rejects behind it, on the null stream.  form: "plain", "piece" (the piece call), "chained" (the
    lengths from device words) or "ordered" (order = (threads, batch_len)).  out: an Out, or None for a counting call.
    text_outs: the text call writes its outputs too (else it only counts).  call_mode: the mode the rejects are told.
    -> dict(text_rc, rc, counts, words, arena)"""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*ptuple)
    pad = (behind * (bound_extra // len(behind) + 1))[:bound_extra]
    bufs = [upload(t + pad, s) for t, s in zip(texts, shifts)]
    bounds = [len(t) + bound_extra for t in texts]
    T = sum(bounds)
    cap = capi.fastq_output_bound(T, mode)
    keep = [torch.empty(max(cap, 16), dtype=torch.uint8, device="cuda") if text_outs else None for _ in range(3)]
    arr = [capi.FastqOutput() if k is None else capi.FastqOutput(k.data_ptr(), cap, None, 0) for k in keep]
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
            words = torch.tensor([[n, 1] for n in lens], dtype=torch.int64, device="cuda")
            kw = dict(bytes_dev_ptrs=[words.data_ptr() + 16 * i for i in range(len(texts))],
                      valid_dev_ptrs=[words.data_ptr() + 16 * i + 8 for i in range(len(texts))])
        ctx.trim_fastq_piece_device_async(params, ptrs, bounds, arr, ws.data_ptr(), ws_bytes, mode=mode, piece=form == "piece",
                                          more=more, **kw)
    need = L.sk_trim_fastq_rejects_workspace_bytes(T)
    if arena is None:
        arena = gd.arena(need, leg[0], leg[1], seed)
    assert arena.nbytes >= need
    kind = {"plain": "plain", "chained": "plain", "piece": "piece", "ordered": "ordered"}[form]
    ctx.trim_fastq_rejects_device_async(ws.data_ptr(), T, params.trunc_n, ptrs, bounds, out.struct if out else None,
                                        arena.ws.data_ptr(), arena.nbytes, mode=call_mode or mode, kind=kind,
                                        batch_capacity=fo_.batch_capacity if fo_ else 0, pairs=pairs)
    c = capi.FastqCounts()
    if form == "piece":
        text_rc = ctx._piece_finish(ws.data_ptr(), None)[0]
    elif form == "ordered":
        text_rc = L.sk_trim_fastq_ordered_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(capi.FastqOrderCounts()))
    else:
        text_rc = L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
    jc = capi.FastqRejectsCounts()
    rc = L.sk_trim_fastq_rejects_device_finish(ctx._h, arena.ws.data_ptr(), None, C.byref(jc))
    arena.check()
    b, w = ctx.trim_fastq_rejects_output_words(arena.ws.data_ptr())
    word = lambda p: int(arena.ws[p - arena.ws.data_ptr():p - arena.ws.data_ptr() + 8].cpu().numpy().view(np.uint64)[0])
    return {"text_rc": text_rc, "rc": rc, "counts": jc.as_dict(), "words": (word(b), word(w)), "arena": arena}


def check(ctx, ptuple, texts, mode, pairs=False, want=None, index=True, leg=(16, "zeros"), **kw):
    """the device against the model, with buffers of exactly what the model says"""
    if want is None:
        want = jm.rejects(ptuple, texts, mode, pairs)
    arena = None
    if leg[1] == "leftover":  # a larger call's leftovers: the same texts twice over, then this call in its workspace
        big = run(ctx, ptuple, [t + t for t in texts], mode, pairs, out=Out(2 * want["bytes"] + 64, 2 * want["records"] + 8),
                  leg=(leg[0], "pattern"), seed=1)
        arena = big["arena"]
    out = Out(want["bytes"], want["records"], index)
    got = run(ctx, ptuple, texts, mode, pairs, out=out, leg=leg, arena=arena, **kw)
    assert got["rc"] == capi.SK_OK, capi.lib().sk_last_error(ctx._h)
    flags = capi.SK_FQ_REJECTS_PAIRS if pairs else 0
    assert got["counts"] == {"records": want["records"], "bytes": want["bytes"], "reads": want["reads"], "valid": want["valid"],
                             "flags": flags}
    text, idx = out.read(want["bytes"], want["records"])
    assert text == want["text"]
    if index:
        assert np.array_equal(idx, want["index"])
    assert got["words"] == ((want["bytes"], 1) if want["valid"] else (0, 0))
    return got


def untouched(out):
    text, idx = out.read(0, 0)
    assert text == b"" and (idx is None or len(idx) == 0)


# ---- the truth table --------------------------------------------------------------------------------------------------------
QUALS = {"phred": (b"(", b"\x05"), "sanger": (b"I", b"#"), "solexa": (b"h", b";"), "illumina": (b"h", b"B")}


def retyped(records, qualtype):
    """the table's records with the quality bytes of another type: 'I' -> its quality 40, '#' -> a quality below 20"""
    hi, lo = QUALS[qualtype]
    return [(n, s, p, q.replace(b"I", hi).replace(b"#", lo)) for n, s, p, q in records]


@pytest.mark.parametrize("mode", jm.MODES)
@pytest.mark.parametrize("qualtype", ["phred", "sanger", "solexa", "illumina"])
def test_truth_table(sk_ctx, mode, qualtype):
    """the hand table: the chosen records are listed by hand, the text is their own four lines"""
    for n, (name, params, records, reads, lost, lost_pairs) in enumerate(TABLE):
        if params[0] == "phred":
            if qualtype != "phred":
                continue  # the '\r' cases: a '\r' is a quality byte of phred alone
        else:
            records, params = retyped(records, qualtype), (qualtype,) + params[1:]
        for pairs in ((False,) if mode == "se" else (False, True)):
            chosen = lost_pairs if pairs else lost
            want = {"text": want_of(records, chosen), "index": np.array(chosen, np.int64), "records": len(chosen),
                    "bytes": len(want_of(records, chosen)), "reads": reads, "valid": 1}
            check(sk_ctx, params, texts_for(records, mode), mode, pairs, want=want, leg=LEGS[(n + pairs) % len(LEGS)], seed=n)


def test_unterminated_last_line_and_odd_record(sk_ctx):
    records = [K(b"a"), X(b"b")]
    check(sk_ctx, P5, [text_of(records, last_newline=False)], "se",
          want=dict(jm.rejects(P5, [text_of(records)], "se"), text=want_of(records, [1])))
    pair = [X(b"a/1"), X(b"a/2")]
    for pairs in (False, True):
        got = check(sk_ctx, P5, texts_for(pair, "pe_split", last_newline=False), "pe_split", pairs)
        assert got["counts"]["bytes"] == len(text_of(pair))  # two bytes more than the two texts hold
    odd = [K(b"a/1"), X(b"a/2"), X(b"odd")]
    for mode in ("pe_interleaved", "pe_combo_all"):
        assert check(sk_ctx, P5, [text_of(odd)], mode)["counts"]["reads"] == 2
        assert check(sk_ctx, P5, [text_of(odd)], mode, pairs=True)["counts"]["records"] == 2


# ---- the shapes ---------------------------------------------------------------------------------------------------------------
def uniform(n, pattern, length=30):
    """n reads of `length` bases: pattern "none", "all", "first" or "last" rejected"""
    lost = lambda k: pattern == "all" or (pattern == "first" and k == 0) or (pattern == "last" and k == n - 1)
    return [(b"@r%d" % k, b"A" * length, b"+", (b"#" if lost(k) else b"I") * length) for k in range(n)]


@pytest.mark.parametrize("n", [1, 2, 2047, 2048, 2049, 4097])
@pytest.mark.parametrize("pattern", ["none", "all", "first", "last"])
def test_read_counts(sk_ctx, n, pattern):
    """around a block of 2 048 reads; the interleaved call drops an odd last record, whose rejection then shows nowhere"""
    records = uniform(n, pattern)
    leg = LEGS[(n + len(pattern)) % len(LEGS)]
    got = check(sk_ctx, P5, [text_of(records)], "se", leg=leg, seed=n)
    assert got["counts"]["records"] == {"none": 0, "all": n}.get(pattern, 1)
    check(sk_ctx, P5, [text_of(records)], "pe_interleaved", pairs=True, leg=leg, seed=n + 1)
    if n % 2 == 0:
        check(sk_ctx, P5, texts_for(records, "pe_split"), "pe_split", pairs=pattern == "last", leg=leg, seed=n + 2)


def test_granule_boundaries_at_every_offset(sk_ctx):
    """record lengths that put the records' starts, and so the output's granule boundaries inside them, at every offset"""
    records = [(b"@" + b"n" * (1 + k % 16), b"ACGTACG", b"+", b"#######") for k in range(67)]
    want = jm.rejects(P5, [text_of(records)], "se")
    starts = np.cumsum([0] + [len(text_of([r])) for r in records])[:-1]
    assert want["records"] == 67 and set(int(s) % 16 for s in starts) == set(range(16))
    check(sk_ctx, P5, [text_of(records)], "se", want=want, leg=(48, "ones"))
    for length in range(1, 34):
        check(sk_ctx, P5, [text_of(uniform(70, "all", length))], "se", leg=LEGS[length % 3], seed=length)


@pytest.mark.parametrize("s0", [0, 1, 7, 15])
@pytest.mark.parametrize("s1", [0, 1, 7, 15])
def test_split_alignments(sk_ctx, s0, s1):
    """either text at any offset from a 16-byte boundary: every load is an aligned one, funnel-shifted"""
    records = [(b"@p%d/%d" % (k // 2, 1 + k % 2), b"ACGTTGCA" * (2 + k % 5), b"+", (b"#" if k % 3 else b"I") * (8 * (2 + k % 5)))
               for k in range(300)]
    for pairs in (False, True):
        check(sk_ctx, P5, texts_for(records, "pe_split"), "pe_split", pairs, shifts=(s0, s1), leg=LEGS[(s0 + s1) % len(LEGS)], seed=s0)
    check(sk_ctx, P5, [text_of(records)], "pe_interleaved", shifts=(s1, 0))


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_output_of_one_gather_chunk(sk_ctx, delta):
    """exactly jm.GCHUNK output bytes, one more, one fewer"""
    records = [(b"@%04d" % k, b"A" * 27, b"+", b"#" * 27) for k in range(jm.GCHUNK // 64)]  # 5 + 27 + 1 + 27 and four '\n'
    records[-1] = (b"@" + b"x" * (4 + delta),) + records[-1][1:]
    want = jm.rejects(P5, [text_of(records)], "se")
    assert want["bytes"] == jm.GCHUNK + delta
    check(sk_ctx, P5, [text_of(records)], "se", want=want, leg=LEGS[1 + delta], seed=delta + 1)


def test_record_longer_than_a_gather_chunk(sk_ctx):
    """a 70 000-byte name line and a 20 000-base read among short records, kept and rejected"""
    records = [K(b"a"), X(b"b"), (b"@" + b"N" * 69_999, b"ACGT", b"+", b"####"), K(b"c"),
               (b"@long", b"ACGT" * 5000, b"+" + b"p" * 500, b"#" * 20_000), X(b"d"), (b"@kept", b"ACGT" * 5000, b"+", b"I" * 20_000),
               X(b"e")]
    assert jm.rejects(P5, [text_of(records)], "se")["index"].tolist() == [1, 2, 4, 5, 7]
    check(sk_ctx, P5, [text_of(records)], "se", leg=(240, "pattern"), seed=3)
    check(sk_ctx, P5, texts_for(records, "pe_split"), "pe_split", pairs=True, shifts=(3, 9), leg=(16, "ones"))


def test_more_records_in_a_chunk_than_the_window_holds(sk_ctx):
    """9 001 one-base reads, every one rejected: 910 records overlap a chunk, the window stages jm.WIN"""
    records = [(b"@a", b"A", b"+", b"I")] * 9001
    want = jm.rejects(P5, [text_of(records)], "se")
    assert want["records"] == 9001 and want["bytes"] == 9 * 9001 and jm.GCHUNK // 9 > jm.WIN
    check(sk_ctx, P5, [text_of(records)], "se", want=want, leg=(48, "zeros"))
    check(sk_ctx, P5, [text_of(records)], "pe_combo_all", pairs=True, leg=(16, "leftover"))


def test_unterminated_rejected_last_line_in_the_chained_form(sk_ctx):
    """the lengths are device words, the bounds 64 bytes longer, and records lie behind the text's end: the '\\n' the last
    line gains is synthesized, nothing behind the text is copied"""
    records = [K(b"a"), X(b"b"), K(b"c"), X(b"last")]
    text = text_of(records, last_newline=False)
    want = dict(jm.rejects(P5, [text], "se"))
    assert want["text"] == want_of(records, [1, 3]) and want["text"].endswith(b"####\n")
    for behind in (b"\n@g\nACGT\n+\n####\n", b"#", b"\xff"):
        check(sk_ctx, P5, [text], "se", want=want, form="chained", bound_extra=64, behind=behind, leg=(240, "ones"))
    pair = [X(b"a/1"), X(b"a/2")]
    tt = texts_for(pair, "pe_split", last_newline=False)
    check(sk_ctx, P5, tt, "pe_split", want=jm.rejects(P5, tt, "pe_split"), form="chained", bound_extra=64,
          behind=b"\n@g\nACGT\n+\n####\n", shifts=(5, 11))


# ---- capacities and counting ------------------------------------------------------------------------------------------------
def test_capacities_one_short(sk_ctx):
    records = uniform(300, "all") + uniform(300, "none")
    text = [text_of(records)]
    want = jm.rejects(P5, text, "se")
    assert want["records"] == 300
    for cap, rec_cap, index in ((want["bytes"] - 1, 300, True), (want["bytes"], 299, True), (want["bytes"] - 1, 0, False)):
        out = Out(cap, rec_cap, index)
        got = run(sk_ctx, P5, text, "se", out=out, leg=(48, "pattern"), seed=cap)
        assert got["rc"] == capi.SK_ESPACE and b"rejects" in capi.lib().sk_last_error(sk_ctx._h)
        assert got["counts"] == {"records": 300, "bytes": want["bytes"], "reads": 600, "valid": 1, "flags": 0}
        assert got["words"] == (0, 0)
        untouched(out)
    # record_capacity plays no part without an index
    out = Out(want["bytes"], 0, False)
    got = run(sk_ctx, P5, text, "se", out=out)
    assert got["rc"] == capi.SK_OK and out.read(want["bytes"], 0)[0] == want["text"] and got["words"] == (want["bytes"], 1)


def test_counting_call_behind_a_counting_text_call(sk_ctx):
    records = uniform(2500, "all")[:1200] + uniform(1300, "none")
    for mode, pairs in (("se", False), ("pe_interleaved", True), ("pe_combo_all", False)):
        want = jm.rejects(P5, [text_of(records)], mode, pairs)
        got = run(sk_ctx, P5, [text_of(records)], mode, pairs, out=None, leg=(240, "pattern"), seed=7)
        assert (got["text_rc"], got["rc"]) == (capi.SK_OK, capi.SK_OK) and got["words"] == (0, 0)
        assert got["counts"] == {"records": want["records"], "bytes": want["bytes"], "reads": 2500, "valid": 1,
                                 "flags": int(pairs)}
    # and behind a text call that wrote its outputs: the same rejects
    check(sk_ctx, P5, [text_of(records)], "pe_interleaved", pairs=True, text_outs=True)


# ---- calls that must touch nothing ------------------------------------------------------------------------------------------
VOID = {"records": 0, "bytes": 0, "reads": 0, "valid": 0, "flags": 0}


def void(got, out):
    assert got["rc"] == capi.SK_OK and got["counts"] == VOID and got["words"] == (0, 0)
    untouched(out)


@pytest.mark.parametrize("what", ["format", "range"])
@pytest.mark.parametrize("form", ["plain", "piece"])
def test_failed_calls_touch_nothing(sk_ctx, what, form):
    records = uniform(3000, "all")
    bad = (b"@bad", b"ACGT", b"+", b"###") if what == "format" else (b"@low", b"A" * 41, b"+", b"#" * 20 + b" " + b"#" * 20)
    records[1400:1400] = [bad, X(b"mate")]
    out = Out(1 << 20, 4096)
    got = run(sk_ctx, P5, [text_of(records)], "pe_interleaved", out=out, form=form, leg=(48, "ones"))
    assert got["text_rc"] == (capi.SK_EFORMAT if what == "format" else capi.SK_ERANGE)
    void(got, out)


def test_mode_that_disagrees(sk_ctx):
    text = [text_of(uniform(80, "all"))]
    for call_mode, told in (("pe_interleaved", "se"), ("se", "pe_interleaved"), ("pe_combo_all", "se")):
        out = Out(1 << 16, 128)
        void(run(sk_ctx, P5, text, call_mode, out=out, call_mode=told), out)
    # SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED: either name fits either call
    want = jm.rejects(P5, text, "pe_interleaved", True)
    check(sk_ctx, P5, text, "pe_combo_all", pairs=True, call_mode="pe_interleaved", want=want)
    check(sk_ctx, P5, text, "pe_interleaved", pairs=True, call_mode="pe_combo_all", want=want)


def test_void_piece_behind_a_failed_one(sk_ctx):
    """a piece enqueued behind one with a range error, before that one's finish, takes no record: its rejects are void"""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*P5)
    bad = text_of([X(b"a"), (b"@low", b"A" * 41, b"+", b"#" * 20 + b" " + b"#" * 20), X(b"b")])
    good = text_of(uniform(500, "all"))
    calls = []
    for text in (bad, good):
        buf, ptr = upload(text)
        ws_bytes = L.sk_trim_fastq_workspace_bytes(len(text), 0)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        sk_ctx.trim_fastq_piece_device_async(params, [ptr], [len(text)], [capi.FastqOutput()] * 3, ws.data_ptr(), ws_bytes, mode="se")
        arena = gd.arena(L.sk_trim_fastq_rejects_workspace_bytes(len(text)), 48, "pattern", 9)
        out = Out(len(text) + 2, 600)
        sk_ctx.trim_fastq_rejects_device_async(ws.data_ptr(), len(text), 0, [ptr], [len(text)], out.struct, arena.ws.data_ptr(),
                                               arena.nbytes, mode="se", kind="piece")
        calls.append((buf, ws, arena, out))
    rcs = [sk_ctx._piece_finish(c[1].data_ptr(), None) for c in calls]
    assert rcs[0][0] == capi.SK_ERANGE and rcs[1][0] == capi.SK_ERANGE and rcs[1][2]["piece"]["inherited_range"] == 1
    for _, _, arena, out in calls:
        jc = capi.FastqRejectsCounts()
        assert L.sk_trim_fastq_rejects_device_finish(sk_ctx._h, arena.ws.data_ptr(), None, C.byref(jc)) == capi.SK_OK
        assert jc.as_dict() == VOID
        arena.check()
        untouched(out)
    # the finishes cleared the stream's word: the same text behind them is trimmed, and rejected
    check(sk_ctx, P5, [good], "se", form="piece")


def test_long_line_refusal(sk_ctx):
    """SK_ELONGLINE of the ordered call: nothing was written there, nothing is written here"""
    records = uniform(40, "all", 8)
    records[20] = (b"@" + b"n" * 40,) + records[20][1:]
    out = Out(1 << 14, 64)
    got = run(sk_ctx, P5, [text_of(records)], "se", out=out, form="ordered", order=(1, 20))
    assert got["text_rc"] == capi.SK_ELONGLINE
    void(got, out)


# ---- the other kinds ----------------------------------------------------------------------------------------------------------
P1 = ("sanger", 20, 1, False, False)


def short_lines(n, batch_len):
    """Records that the reference's reader takes at this byte budget: a batch needs a whole pair, eight lines, before the
    lines' lengths use the budget up, so at 20 bytes the names are "@a" and the reads 2 or 3 bases.  The mates of a pair
    are equally long, so that two split inputs are cut into the same batches.  A third is rejected."""
    rng = np.random.default_rng(batch_len)
    out = []
    for k in range(n):
        if k % 2 == 0:
            m = int(rng.integers(2, 4)) if batch_len == 20 else int(rng.integers(2, 8))
        name = b"@a" if batch_len == 20 else b"@r%03d" % (k // 2)
        out.append((name, (b"ACGT" * 4)[:m], b"+", (b"#" if rng.integers(3) == 0 else b"I") * m))
    # a pair whose name and seq lines use a whole budget up: the batch that meets it holds no unit, which ends the
    # reader's run; the 198 records behind it are in no batch
    w = batch_len // 2 + 2
    out[400] = out[401] = (b"@" + b"s" * (w - 1), b"A" * w, b"+", b"#" * w)
    return out


@pytest.mark.parametrize("order", [(1, 20), (3, 64)])
def test_ordered_call(sk_ctx, order):
    """the -a T order: the rejects stay in read order, and the records behind the last batch are no reads"""
    records = short_lines(600, order[1])
    for mode in ("se", "pe_interleaved", "pe_split"):
        tt = texts_for(records, mode)
        units = fo.batch_tables([fo.lines_of(t) for t in tt], mode, order[1])["units"]
        n_reads = units * (1 if mode == "se" else 2)
        assert 300 < n_reads <= 400
        for pairs in ((False,) if mode == "se" else (False, True)):
            want = jm.rejects(P1, tt, mode, pairs, n_reads=n_reads)
            assert want["records"] > 20 and np.all(np.diff(want["index"]) > 0)
            check(sk_ctx, P1, tt, mode, pairs, want=want, form="ordered", order=order, leg=(240, "zeros"))


def test_raw_piece_call_with_more(sk_ctx):
    """more != 0: the piece takes whole records (pairs) only; the carry is the next piece's, and is not rejected twice"""
    records = uniform(401, "all", 12)
    text = text_of(records)
    cut = len(text) - 20  # inside the last record
    for mode in ("se", "pe_interleaved"):
        p = pm.piece(P5, [text[:cut]], mode, True)
        n_reads = p["records_in"][0]
        assert n_reads == 400
        first = jm.rejects(P5, [text[:cut]], mode, n_reads=n_reads)
        check(sk_ctx, P5, [text[:cut]], mode, want=first, form="piece", more=True)
        rest = jm.rejects(P5, [text[p["consumed"][0]:]], "se")
        check(sk_ctx, P5, [text[p["consumed"][0]:]], "se", want=rest, form="piece")
        assert first["text"] + rest["text"] == jm.rejects(P5, [text], "se")["text"]


def mixed(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(20, 120))
        q = np.clip(int(rng.integers(36, 70)) + rng.integers(-14, 9, m), 33, 73).astype(np.uint8).tobytes()
        out.append((b"@r%d/%d" % (k // 2, 1 + k % 2), (b"ACGT" * 30)[:m], b"+", q))
    return out


PT = ("sanger", 22, 40, False, False)


@pytest.mark.parametrize("piece_bytes", [256, 1000, 8192])
@pytest.mark.parametrize("gz", [False, True])
def test_text_stream_driver(sk_ctx, piece_bytes, gz):
    """trim_fastq_stream: the fourth entries concatenated are the whole text's rejects; with gz=True one valid .gz file"""
    params = capi.make_params(*PT)
    records = mixed(600, 31)
    for mode, pairs in (("se", False), ("pe_split", True), ("pe_interleaved", True), ("pe_combo_all", False)):
        tt = texts_for(records, mode)
        want = jm.rejects(PT, tt, mode, pairs)
        assert 50 < want["records"] < 600
        args = dict(mode=mode, piece_bytes=piece_bytes, room=max(2048, piece_bytes), gz=gz)
        st = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, rejects="pairs" if pairs else True, **args)
        assert st.rejects is None
        pieces = list(st)
        assert st.pieces > 1 and all(len(p) == 4 for p in pieces)
        rej = b"".join(p[3] for p in pieces)
        if gz:
            assert all(p[3].endswith(capi.BGZF_EOF_MEMBER) == (p is pieces[-1]) for p in pieces)
            rej = gzip.decompress(rej)
        assert rej == want["text"] and st.rejects == {"records": want["records"], "bytes": want["bytes"]}
        plain = sk_ctx.trim_fastq_stream(params, tt[0], tt[1] if len(tt) > 1 else None, **args)
        ppieces = list(plain)
        assert all(len(p) == 3 for p in ppieces) and [p[:3] for p in pieces] == ppieces
        assert plain.rejects is None and plain.counts == st.counts and plain.device_bytes < st.device_bytes


def test_device_bytes_is_a_function_of_the_sizes(sk_ctx):
    params = capi.make_params(*PT)
    a = sk_ctx.trim_fastq_stream(params, text_of(mixed(10, 1)), piece_bytes=4096, room=2048, rejects=True)
    b = sk_ctx.trim_fastq_stream(params, text_of(mixed(900, 2)), piece_bytes=4096, room=2048, rejects=True)
    assert a.device_bytes == b.device_bytes
    with pytest.raises(ValueError):
        sk_ctx.trim_fastq_stream(params, b"", piece_bytes=4096, rejects="pairs")


def to_device(data):
    torch = torch_mod()
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def test_ordered_stream_driver(sk_ctx):
    """order= reorders the outputs, not the rejects"""
    params = capi.make_params(*PT)
    records = mixed(600, 33)
    tt = texts_for(records, "pe_interleaved")
    units = fo.batch_tables([fo.lines_of(t) for t in tt], "pe_interleaved", 1500)["units"]
    want = jm.rejects(PT, tt, "pe_interleaved", True, n_reads=2 * units)
    st = sk_ctx.trim_fastq_stream(params, tt[0], mode="pe_interleaved", piece_bytes=4096, room=8192, order=(3, 1500), rejects="pairs")
    assert b"".join(p[3] for p in st) == want["text"] and st.rejects["records"] == want["records"]


@pytest.mark.parametrize("gz", [False, True])
def test_image_stream_drivers(sk_ctx, gz):
    """trim_gz_stream and trim_gzip_stream at the smallest pieces they take (a BGZF member's text, 65 536 bytes; the gzip
    reader's stretches): several pieces each"""
    params = capi.make_params(*PT)
    records = mixed(6000, 35)
    for mode, pairs in (("pe_split", True), ("pe_interleaved", False)):
        tt = texts_for(records, mode)
        want = jm.rejects(PT, tt, mode, pairs)
        bgzf = [sk_ctx.bgzf(to_device(t)).cpu().numpy().tobytes() for t in tt]
        plain = [gzip.compress(t, 6) for t in tt]
        two = lambda xs: (xs[0], xs[1] if len(xs) > 1 else None)
        rej = "pairs" if pairs else True
        for st in (sk_ctx.trim_gz_stream(params, *two(bgzf), mode=mode, piece_bytes=65536, room=65536, gz=gz, rejects=rej),
                   sk_ctx.trim_gzip_stream(params, *two(plain), mode=mode, piece_bytes=1 << 17, room=65536, gz=gz, rejects=rej)):
            pieces = list(st)
            got = b"".join(p[3] for p in pieces)
            assert st.pieces > 1 and (gzip.decompress(got) if gz else got) == want["text"]
            assert st.rejects == {"records": want["records"], "bytes": want["bytes"]}


# ---- trim_fastq -----------------------------------------------------------------------------------------------------------------
def _golden(name):
    return open(os.path.join(INPUTS, name), "rb").read()


@pytest.mark.parametrize("case", ["test.fastq", "test.f.fastq", "split"])
def test_trim_fastq_on_the_golden_inputs(sk_ctx, case):
    """rejects=True and "pairs" against the model and against the device's own report of the same call"""
    mode = "pe_split" if case == "split" else "pe_interleaved" if case == "test.fastq" else "se"
    texts = [_golden("test.f.fastq"), _golden("test.r.fastq")] if case == "split" else [_golden(case)]
    seen = 0
    for pt in (("illumina", 20, 20, False, False), ("illumina", 30, 50, True, False)):
        params = capi.make_params(*pt)
        dev = [to_device(t) for t in texts]
        for rej in ((True,) if mode == "se" else (True, "pairs")):
            want = jm.rejects(pt, texts, mode, rej == "pairs")
            outs, counts, report = sk_ctx.trim_fastq(params, dev[0], dev[1] if len(dev) > 1 else None, mode=mode, rejects=rej,
                                                     report=True, record_index=True)
            r = counts["rejects"]
            got = {"text": r["text"].cpu().numpy().tobytes(), "index": r["index"].cpu().numpy(), "records": r["records"],
                   "bytes": r["bytes"], "reads": r["reads"]}
            assert jm.equal(got, {k: v for k, v in want.items() if k != "valid"}) == []
            assert report["reads"] == r["reads"]
            seen += r["records"]
            if rej is True:
                assert r["records"] == report["discarded"]
            else:
                assert r["records"] == 2 * (report["pairs"][0] + report["pairs"][1] + report["pairs"][2])
        plain = sk_ctx.trim_fastq(params, dev[0], dev[1] if len(dev) > 1 else None, mode=mode, rejects=True)
        assert plain[1]["rejects"]["index"] is None and plain[1]["rejects"]["records"] == jm.rejects(pt, texts, mode)["records"]
    assert seen > 0  # (at -q 20 -l 20 test.f.fastq alone loses no read)


def test_rejects_false_returns_what_it_returned(sk_ctx):
    text = text_of(mixed(1400, 37))
    params = capi.make_params(*PT)
    same = lambda xs, ys: all((x is None and y is None) or bool((x == y).all()) for x, y in zip(xs, ys))
    for mode in ("se", "pe_interleaved", "pe_combo_all"):
        a = sk_ctx.trim_fastq(params, to_device(text), mode=mode)
        b = sk_ctx.trim_fastq(params, to_device(text), mode=mode, rejects=True)
        assert len(a) == len(b) == 2 and "rejects" not in a[1]
        b[1].pop("rejects")
        assert a[1] == b[1] and same(a[0], b[0])
    o = sk_ctx.trim_fastq(params, to_device(text), mode="pe_interleaved", order=(3, 1500), rejects="pairs", record_index=True)
    units = fo.batch_tables([fo.lines_of(text)], "pe_interleaved", 1500)["units"]
    want = jm.rejects(PT, [text], "pe_interleaved", True, n_reads=2 * units)
    r = o[1]["rejects"]
    assert r["text"].cpu().numpy().tobytes() == want["text"] and np.array_equal(r["index"].cpu().numpy(), want["index"])
    torch = torch_mod()
    e = sk_ctx.trim_fastq(params, torch.empty(0, dtype=torch.uint8, device="cuda"), mode="pe_interleaved", rejects="pairs")
    assert e[1]["rejects"]["records"] == 0 and e[1]["rejects"]["text"].numel() == 0
    with pytest.raises(ValueError):
        sk_ctx.trim_fastq(params, to_device(text), rejects="both")


def test_pairs_trimmed_again_give_the_same_cuts(sk_ctx):
    """the "pairs" rejects are a valid interleaved text: trimmed again, no pair of it is whole, its singles are the first
    run's singles byte for byte (the same cuts), and its rejects are the first run's"""
    text = text_of(mixed(2000, 39))
    params = capi.make_params(*PT)
    outs, counts = sk_ctx.trim_fastq(params, to_device(text), mode="pe_interleaved", rejects="pairs")
    first = sk_ctx.trim_fastq(params, to_device(text), mode="pe_interleaved", rejects=True)[1]["rejects"]
    rej = counts["rejects"]["text"]
    assert rej.numel() > 0 and counts["rejects"]["records"] % 2 == 0
    outs2, counts2 = sk_ctx.trim_fastq(params, rej.clone(), mode="pe_interleaved", rejects="pairs")
    assert counts2["records"][0] == 0 and counts2["records_in"][0] == counts["rejects"]["records"]
    assert outs2[2].numel() == outs[2].numel() > 0 and bool((outs2[2] == outs[2]).all())
    assert counts2["rejects"]["bytes"] == rej.numel() and bool((counts2["rejects"]["text"] == rej).all())
    again = sk_ctx.trim_fastq(params, rej.clone(), mode="pe_interleaved", rejects=True)[1]["rejects"]
    assert again["records"] == first["records"] > 0 and again["bytes"] == first["bytes"]
    assert bool((again["text"] == first["text"]).all())


# ---- the drawn texts ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn_cases():
    return jm.drawn()


@pytest.mark.parametrize("part", range(10))
def test_drawn_texts(sk_ctx, drawn_cases, part):
    """the hundred texts of tests/test_fastq_rejects_model.py, ten a case, in plain and piece form: every mode and encoding,
    malformed records, chars out of range, degenerate texts"""
    for n, c in enumerate(drawn_cases[10 * part:10 * part + 10]):
        pt = tuple(c["params"])
        want = jm.rejects(pt, c["texts"], c["mode"], c["pairs"])
        for form in ("plain", "piece"):
            leg = LEGS[(n + (form == "piece")) % 3]
            if want["valid"]:
                check(sk_ctx, pt, c["texts"], c["mode"], c["pairs"], want=want, form=form, shifts=(c["shift"], 0), leg=leg, seed=n)
            else:
                out = Out(sum(len(t) for t in c["texts"]) + 2, 16)
                got = run(sk_ctx, pt, c["texts"], c["mode"], c["pairs"], out=out, form=form, shifts=(c["shift"], 0), leg=leg, seed=n)
                assert got["text_rc"] in (capi.SK_EFORMAT, capi.SK_ERANGE), c["notes"]
                assert got["rc"] == capi.SK_OK and got["counts"] == dict(VOID, flags=int(c["pairs"])) and got["words"] == (0, 0)
                untouched(out)
