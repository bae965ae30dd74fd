"""GPU: every device call that keeps its scratch in a caller's workspace, held to the three promises of
include/sickle_amd.h about it: a base that is 16-byte aligned and nothing more, a size by the formula alone, and contents
on entry that do not matter while nothing outside [workspace, workspace + bytes) is written.  Each case of
tests/workspace_cases.py runs through the family's existing helper on tests/guarded.py's arena at every lead (16, 48, 240)
and every poison (zeros, seeded random bytes with the seed of the test id, 0xFF, and the leftovers of a larger call of the
family), is compared with the family's model by its existing comparison, and must give the same bytes, counts and
published device words on every leg.  The control, the first and the last case of a family run once more between hostile
surroundings (records around a text, complete members around an image) at shifts 0, 1 and 15.

Where a cause is read from if a leg faults or differs: which kernel writes what before anything reads it.
  FASTQ text calls (sk_launch_fastq_front, sk_fastq.hip): sk_fq_frame_count_kernel writes every chunk entry;
    sk_fq_frame_scan_kernel (one workgroup) turns them into bases and writes the header's lines, records, FMT, MODE, NREAL
    and the piece words; sk_fq_frame_lines_kernel writes desc for every line (every record with a line has a slot:
    sk_fq_slots); sk_fq_check_kernel reads desc below the record count only; the pack's count kernel writes every block
    entry, its scan the bases, its place kernel offsets and the packed bytes; the emission does the same with emit.
    Ordered calls add the chain kernel (the table of first units); ordered pieces the extension block.
  sk_launch_trim (sk_trim.hip): the count kernel writes every block-table entry, the scan kernel the header.
  sk_launch_bgzf (sk_bgzf.hip): the block kernel writes its table entry, tokens and slot per block, the scan kernel the
    header and the members' offsets; the search's cand section is written per block before it is read.
  sk_launch_bgzf_inflate (sk_inflate.hip): the tile kernel writes every tile count, the scan the header; candidates,
    successors and ranks are written for every candidate before the pointer doubling reads them.
  sk_launch_gunzip (sk_gunzip.hip): the header kernel writes the header, the search kernels every stretch entry."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgunzip_model as bm
import bgzf_raw
import cli_util as cu
import combo_all_model as cm
import fastq_model as fm
import fastq_order_model as om
import fastq_piece_model as pm
import fastq_raw as fr
import foreign_images as fi
import guarded
import gunzip_model as gm
import gunzip_piece_model as gpm
import test_gpu_bgunzip as tbu
import test_gpu_fastq_chain as tch
import test_gpu_fastq_order as tor
import test_gpu_fastq_order_piece as top
import test_gpu_fastq_piece as tpi
import test_gpu_gunzip as tgu
import test_gpu_gunzip_piece as tgp
import trim_model as tm
import trim_raw
import workspace_cases as wc
from sickle_amd import capi
from test_gz_inflater import SIM

pytestmark = pytest.mark.gpu
TEXTS = wc.fastq_texts()
BIG_TEXT = wc.many_good(2000, seed=3)  # larger than every text of the table: its call's leftovers are the fourth poison
MEMO = {}                              # models of the big calls and the plain-Python ordered models: once a session


def seeded(names):
    """one parameter per case, the poison's seed in its id"""
    return [pytest.param(n, k, id="%s-seed%d" % (n, k)) for k, n in enumerate(names)]


def hostile_of(names):
    """the control, the first and the last case of a family"""
    names = list(names)
    return {names[0], names[-1]} | {n for n in names if n.startswith("control")}


def memo(key, make):
    if key not in MEMO:
        MEMO[key] = make()
    return MEMO[key]


def words_of(ws, addrs):
    """the 8-byte device words at the addresses `addrs` inside the workspace tensor ws"""
    base = ws.data_ptr()
    return [int(ws[a - base:a - base + 8].cpu().numpy().view(np.uint64)[0]) for a in addrs]


def sweep(nbytes, run, big, seed, hostile=None):
    """run(ws, shift=None, surround=None) -> a summary of one call (already compared with its model).  It runs at every
    lead and poison, then on what big = (bytes, run of a larger call of the family) left in the arena; behind each call
    the bands are checked, and every leg's summary must equal the first.  hostile: the bytes to put around the input for
    three more legs (lead 16, random bytes) at shifts 0, 1 and 15."""
    first = None
    for lead in guarded.LEADS:
        for poison in guarded.POISONS:
            a = guarded.arena(nbytes, lead, poison, seed=seed)
            got = run(a.ws)
            a.check()
            first = got if first is None else first
            assert got == first, "the result depends on the workspace's base or contents (lead %d, %s)" % (lead, poison)
        if big is not None:
            a = guarded.arena(max(big[0], nbytes), lead, "pattern", seed=seed)
            big[1](a.ws[:big[0]])
            got = run(a.ws[:nbytes])
            a.check()
            assert got == first, "the result depends on what an earlier call left (lead %d)" % lead
    if hostile is not None:
        for shift in (0, 1, 15):
            a = guarded.arena(nbytes, 16, "pattern", seed=seed)
            got = run(a.ws, shift=shift, surround=hostile)
            a.check()
            assert got == first, "the result depends on what lies around the input (shift %d)" % shift
    return first


def bytes_of(keep):
    return [None if k is None else (k[0].cpu().numpy().tobytes(), None if k[1] is None else k[1].cpu().numpy().tobytes())
            for k in keep]


# ---- 0 the tool itself -----------------------------------------------------------------------------------------------------
def test_arena_self_test():
    for lead in guarded.LEADS:
        a = guarded.arena(1000, lead, "ones")
        assert a.ws.data_ptr() % 16 == 0 and a.ws.data_ptr() % 32 != 0 and a.ws.numel() == 1000
        assert bool((a.ws == 0xFF).all())
        a.check()
        a.ws.fill_(3)  # the workspace itself is the call's
        a.check()
        a.buf[a.front - 5] ^= 1
        with pytest.raises(guarded.GuardError, match=r"offsets -5 \.\. -5"):
            a.check()
        a.buf[a.front - 5] ^= 1
        a.check()
        a.buf[a.front + 1000 + 17] ^= 0x80
        a.buf[a.front + 1000 + 4000] ^= 0x80
        with pytest.raises(guarded.GuardError, match=r"offsets 17 \.\. 4000"):
            a.check()
    assert bool((guarded.arena(64, 16, "pattern", 5).ws == guarded.arena(64, 48, "pattern", 5).ws).all())


# ---- 1 FASTQ text calls ----------------------------------------------------------------------------------------------------
FQ_NAMES = sorted(TEXTS)
FQ_HOSTILE = hostile_of(FQ_NAMES)
ALL_MODES = wc.FASTQ_MODES + (cm.MODE,)


def fastq_bytes(T, trunc_n):
    return capi.lib().sk_trim_fastq_workspace_bytes(T, trunc_n)


def fastq_want(pt, texts, mode):
    """the model of the mode: fastq_model's, or combo_all_model's for pe_combo_all (one interleaved text)"""
    return cm.expected(pt, texts[0]) if mode == cm.MODE else fm.expected(pt, texts, mode)


def fastq_compare(ctx, want, rc, counts, keep, mode):
    """tests/test_gpu_fastq_chain.py's compare; pe_combo_all, whose model is combo_all_model's, writes output 0 alone:
    the same comparison for that output, as tests/test_gpu_fastq_combo.py's check makes it"""
    if mode != cm.MODE:
        return tch.compare(ctx, want, rc, counts, keep, mode)
    assert counts["records_in"] == want["records_in"] and counts["tail_lines"] == want["tail_lines"]
    assert counts["dropped_unpaired"] == want["dropped_unpaired"]
    fr.untouched(keep[1:])
    if want["verdict"] is not None:
        assert rc == capi.SK_EFORMAT
        assert (counts["format_error"], counts["format_input"], counts["format_record"]) == want["verdict"]
        return fr.untouched(keep[:1])
    assert want["range"] is None and rc == capi.SK_OK, capi.lib().sk_last_error(ctx._h)
    t, ix = keep[0]
    n, size = len(want["index"][0]), len(want["texts"][0])
    assert counts["records"] == [n, 0, 0] and counts["bytes"] == [size, 0, 0]
    assert t[:size].cpu().numpy().tobytes() == want["texts"][0] and bool((t[size:] == fr.SENTINEL).all())
    assert np.array_equal(ix[:n].cpu().numpy(), want["index"][0]) and bool((ix[n:] == -7).all())


def output_words(ws):
    return words_of(ws, [w for o in range(3) for w in capi.Context.trim_fastq_output_words(ws.data_ptr(), o)])


def plain_run(ctx, pt, texts, mode, want, default_shift=0):
    T = sum(map(len, texts))
    caps = [cm.bound(T, T // 7 + 1) + 16, 64, 64] if mode == cm.MODE else None
    rec_caps = [T // 4 + 4, 8, 8] if mode == cm.MODE else None

    def run(ws, shift=None, surround=None):
        rc, counts, keep = fr.raw(ctx, capi.make_params(*pt), texts, mode, caps=caps, rec_caps=rec_caps, ws=ws, room=64,
                                  shift=default_shift if shift is None else shift, surround=surround)
        fastq_compare(ctx, want, rc, counts, keep, mode)
        return rc, counts, bytes_of(keep), output_words(ws)
    return run


def mode_texts(text, mode):
    return [text] if mode == cm.MODE else wc.texts_of_mode(text, mode)


@pytest.mark.parametrize("name,seed", seeded(FQ_NAMES))
def test_fastq_plain(sk_ctx, name, seed):
    text = TEXTS[name][0]
    for mode in ALL_MODES:
        texts, bigs = mode_texts(text, mode), mode_texts(BIG_TEXT, mode)
        for trunc_n in (0, 1):
            pt = wc.fq_params(trunc_n)
            want = fastq_want(pt, texts, mode)
            if mode == "se":
                assert want["verdict"] == TEXTS[name][1]
            big_want = memo(("plain", mode, trunc_n), lambda: fastq_want(pt, bigs, mode))
            big = (fastq_bytes(sum(map(len, bigs)), trunc_n), plain_run(sk_ctx, pt, bigs, mode, big_want))
            sweep(fastq_bytes(sum(map(len, texts)), trunc_n), plain_run(sk_ctx, pt, texts, mode, want, len(name) % 16), big,
                  seed, hostile=fr.HOSTILE_TEXT if name in FQ_HOSTILE else None)


GAP = 37  # in->bytes of the chained call is this much beyond the device length


def chained_run(ctx, pt, texts, mode, want):
    """the lengths are device words and in->bytes a bound GAP bytes beyond them; surround also fills the gap"""
    T = sum(len(t) + GAP for t in texts)

    def run(ws, shift=None, surround=None):
        shift = 5 if shift is None else shift
        if surround is None:
            bufs = [tch.place(t + bytes(GAP), shift) for t in texts]
        else:
            bufs = [bgzf_raw.surrounded(t, shift, GAP, surround) for t in texts]
        ptrs, bounds, ns = [b[1] for b in bufs], [len(t) + GAP for t in texts], [len(t) for t in texts]
        if mode != cm.MODE:
            rc, counts, out, _ = tch.chained(ctx, pt, ptrs, bounds, mode, ns=ns, valids=[1] * len(texts), ws=ws)
        else:  # the helper's outputs hold the text and 64 bytes; this mode's output 0 can be longer than its text
            torch = fr.torch_mod()
            cap = capi.fastq_output_bound(T, mode)
            t = torch.full((cap + 64,), fr.SENTINEL, dtype=torch.uint8, device="cuda")
            ix = torch.full((T // 4 + 4 + 64,), -7, dtype=torch.int64, device="cuda")
            n, v = tch.word(ns[0]), tch.word(1)
            ctx.trim_fastq_chained_device_async(capi.make_params(*pt), ptrs, bounds,
                                                [capi.FastqOutput(t.data_ptr(), cap, ix.data_ptr(), T // 4 + 4)], ws.data_ptr(),
                                                ws.numel(), bytes_dev_ptrs=[n.data_ptr()], valid_dev_ptrs=[v.data_ptr()], mode=mode)
            c = capi.FastqCounts()
            rc = capi.lib().sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
            counts, out = c.as_dict(), [(t, ix)]
            assert bool((t[cap:] == fr.SENTINEL).all()) and bool((ix[T // 4 + 4:] == -7).all())
            fastq_compare(ctx, want, rc, counts, out, mode)
            return rc, counts, bytes_of(out), output_words(ws)
        tch.compare(ctx, want, rc, counts, out, mode)
        return rc, counts, bytes_of(out), output_words(ws)
    return T, run


@pytest.mark.parametrize("name,seed", seeded(FQ_NAMES))
def test_fastq_chained(sk_ctx, name, seed):
    text = TEXTS[name][0]
    for mode in ALL_MODES:
        texts, bigs = mode_texts(text, mode), mode_texts(BIG_TEXT, mode)
        for trunc_n in (0, 1):
            pt = wc.fq_params(trunc_n)
            T, run = chained_run(sk_ctx, pt, texts, mode, fastq_want(pt, texts, mode))
            big_want = memo(("plain", mode, trunc_n), lambda: fastq_want(pt, bigs, mode))
            big_T, big_run = chained_run(sk_ctx, pt, bigs, mode, big_want)
            sweep(fastq_bytes(T, trunc_n), run, (fastq_bytes(big_T, trunc_n), big_run), seed,
                  hostile=fr.HOSTILE_TEXT if name in FQ_HOSTILE else None)


@pytest.fixture
def cached_models(monkeypatch):
    """the ordered models are plain Python: one evaluation per case, not one per leg"""
    real_expected, real_sequence = om.expected, top.model_sequence

    def expected(ptuple, texts, *rest):
        return memo(("e", ptuple, tuple(texts)) + tuple(rest), lambda: real_expected(ptuple, texts, *rest))

    def sequence(ptuple, texts, mode, threads, batch_len, capacity, steps, limit=0, short=None):
        key = ("s", ptuple, tuple(texts), mode, threads, batch_len, capacity, tuple((tuple(n), m) for n, m in steps), limit)
        return memo(key, lambda: real_sequence(ptuple, texts, mode, threads, batch_len, capacity, steps, limit, short))

    monkeypatch.setattr(om, "expected", expected)
    monkeypatch.setattr(top, "model_sequence", sequence)
    yield
    for key in [k for k in MEMO if k[0] in "es" and k[2] and k[2][0] is not ORDER_BIG]:
        del MEMO[key]  # keep the big text's models alone


ORDER_BIG = wc.many_good(1000, seed=4)  # the ordered doors' larger call (their models are plain Python)


@pytest.mark.parametrize("name,seed", seeded(FQ_NAMES))
def test_fastq_ordered(sk_ctx, cached_models, name, seed):
    """The three texts with more records than a valid text holds (bad7_600, newlines_4096, newlines_65541) are the ones
    that showed the ordered calls stopping at the last of (b + 1) / 8 + 1 descriptor slots: units 526 for the model's 600,
    513 for 1024, 8193 for 16385.  sk_fq_slots is b / 4 + 1 since: a slot for every line of any text."""
    text = TEXTS[name][0]
    L = capi.lib()
    for mode in ("se", "pe_split"):
        texts, bigs = wc.texts_of_mode(text, mode), wc.texts_of_mode(ORDER_BIG, mode)
        T, big_T = sum(map(len, texts)), sum(map(len, bigs))
        for trunc_n in (0, 1):
            pt = wc.fq_params(trunc_n)
            for threads, batch_len in wc.ORDERED:
                batches = om.expected(pt, texts, mode, threads, batch_len, 0)["order"]["batches"]
                for capacity in (max(batches, 1), T // batch_len + 16):  # exact and ample

                    def run(ws, shift=None, surround=None):
                        rc, counts, got = tor.check(sk_ctx, pt, texts, mode, threads, batch_len, capacity=capacity, ws=ws,
                                                    shift=len(name) % 16 if shift is None else shift, surround=surround)
                        table = capi.Context.trim_fastq_ordered_batches(ws.data_ptr())
                        nb = min(counts["order"]["batches"], capacity)
                        return rc, counts, got, words_of(ws, [table + 8 * k for k in range(nb + 1)])

                    def big_run(ws):
                        tor.check(sk_ctx, pt, bigs, mode, threads, batch_len, capacity=big_T // batch_len + 16, ws=ws)
                    big = (L.sk_trim_fastq_ordered_workspace_bytes(big_T, trunc_n, big_T // batch_len + 16), big_run)
                    sweep(L.sk_trim_fastq_ordered_workspace_bytes(T, trunc_n, capacity), run, big, seed,
                          hostile=fr.HOSTILE_TEXT if name in FQ_HOSTILE and capacity != max(batches, 1) else None)


def cut_in_a_record(text):
    """a window end in the middle of a record (or of the text, where it has none)"""
    at = len(text) // 2
    return at + 1 if text[at - 1:at] == b"\n" and at + 1 < len(text) else at


@pytest.mark.parametrize("name,seed", seeded(FQ_NAMES))
def test_fastq_piece(sk_ctx, name, seed):
    text = TEXTS[name][0]
    for mode in ("se", "pe_split"):
        n_in = 2 if mode == "pe_split" else 1
        for trunc_n in (0, 1):
            pt = wc.fq_params(trunc_n)
            cut = cut_in_a_record(text)
            first = pm.piece(pt, [text[:cut]] * n_in, mode, True)
            s = first["consumed"][:n_in]
            plans = [(len(text), [0] * n_in, False, pm.piece(pt, [text] * n_in, mode, False)),  # one piece, more = 0
                     (cut, [0] * n_in, True, first),
                     (len(text), s, False, pm.piece(pt, [text[a:] for a in s], mode, False))]
            big_bytes = fastq_bytes(n_in * len(BIG_TEXT), trunc_n)

            def big_run(ws):
                bufs = [tch.place(BIG_TEXT, 3) for _ in range(n_in)]
                tpi.Call(sk_ctx, pt, [b[1] for b in bufs], [len(BIG_TEXT)] * n_in, mode,
                         ns=[tch.word(len(BIG_TEXT)) for _ in range(n_in)], ws=ws).finish()
            for n, starts, more, want in plans:

                def run(ws, shift=None, surround=None):
                    if surround is None:
                        bufs = [tch.place(text, 3 if shift is None else shift) for _ in range(n_in)]
                    else:
                        bufs = [bgzf_raw.surrounded(text, shift, 0, surround) for _ in range(n_in)]
                    call = tpi.Call(sk_ctx, pt, [b[1] for b in bufs], [len(text)] * n_in, mode,
                                    ns=[tch.word(n) for _ in range(n_in)], starts=[tch.word(a) for a in starts], more=more, ws=ws)
                    rc, counts = tpi.check_piece(call, want, s=tuple(starts) + (0,) * (2 - n_in))
                    return rc, counts, bytes_of(call.keep), [call.published(i) for i in range(n_in)]
                sweep(fastq_bytes(n_in * len(text), trunc_n), run, (big_bytes, big_run), seed,
                      hostile=fr.HOSTILE_TEXT if name in FQ_HOSTILE else None)


@pytest.mark.parametrize("name,seed", seeded(FQ_NAMES))
def test_fastq_ordered_piece(sk_ctx, cached_models, name, seed):
    """records_in of a one-piece call on the same three texts was the slot count (526, 513, 8193) before sk_fq_slots grew"""
    text = TEXTS[name][0]
    L = capi.lib()
    cut = cut_in_a_record(text)
    for mode in ("se", "pe_split"):
        texts, bigs = wc.texts_of_mode(text, mode), wc.texts_of_mode(ORDER_BIG, mode)
        n_in = len(texts)
        for trunc_n in (0, 1):
            pt = wc.fq_params(trunc_n)
            for threads, batch_len in wc.ORDERED:
                capacity, big_capacity = n_in * len(text) // batch_len + 16, n_in * len(ORDER_BIG) // batch_len + 16
                big_bytes = L.sk_trim_fastq_ordered_piece_workspace_bytes(n_in * len(ORDER_BIG), trunc_n, big_capacity)
                for steps in ([([len(text)] * n_in, False)], [([cut] * n_in, True), ([len(text)] * n_in, False)]):
                    sizes = [L.sk_trim_fastq_ordered_piece_workspace_bytes(sum(ns), trunc_n, capacity) for ns, _ in steps]

                    def run(arenas, views, shift=3, surround=None):
                        seen = []
                        top.run_sequence(sk_ctx, pt, texts, mode, threads, batch_len, capacity, steps, ws=views, seen=seen,
                                         shift=shift, surround=surround)
                        for a in arenas:
                            a.check()
                        return seen
                    first = None
                    for lead in guarded.LEADS:
                        for poison in guarded.POISONS:
                            arenas = [guarded.arena(b, lead, poison, seed=seed) for b in sizes]
                            got = run(arenas, [a.ws for a in arenas])
                            first = got if first is None else first
                            assert got == first, "an ordered piece depends on its workspace (lead %d, %s)" % (lead, poison)
                        arenas = [guarded.arena(max(b, big_bytes), lead, "pattern", seed=seed) for b in sizes]
                        for a in arenas:  # the leftovers of a larger piece
                            top.run_sequence(sk_ctx, pt, bigs, mode, threads, batch_len, big_capacity,
                                             [([len(ORDER_BIG)] * n_in, False)], ws=[a.ws[:big_bytes]])
                        assert run(arenas, [a.ws[:b] for a, b in zip(arenas, sizes)]) == first, "leftovers (lead %d)" % lead
                    if name in FQ_HOSTILE:
                        for shift in (0, 1, 15):
                            arenas = [guarded.arena(b, 16, "pattern", seed=seed) for b in sizes]
                            assert run(arenas, [a.ws for a in arenas], shift, fr.HOSTILE_TEXT) == first, "hostile, shift %d" % shift


# ---- 2 sk_trim_device_async ------------------------------------------------------------------------------------------------
def trim_run(ctx, n, kept, layout, mode):
    """a batch of arrays that the offsets (or the stride) address: there is no text whose surroundings could be hostile"""
    nb = capi.lib().sk_trim_workspace_bytes(n)
    qual, seq, off, starts, cuts = wc.trim_case(n, kept, layout, mode)
    want = tm.expected(qual, seq, starts, cuts, mode)
    need = tm.counts_of(want)
    dq, ds, doff = trim_raw.dev(qual), trim_raw.dev(seq), trim_raw.dev(off)
    dc = trim_raw.dev(cuts if n else np.zeros((1, 2), np.int32))
    batch = dict(stride=37, read_len=37) if layout == "fixed" else dict(offsets_ptr=doff.data_ptr())

    def run(ws, alive=(dq, ds, doff, dc)):  # the batch's tensors live as long as the run
        r = trim_raw.Raw(need["records"], need["bytes"])
        counts = ctx.trim_device(dc.data_ptr(), n, r.outs, ws.data_ptr(), nb, mode=mode, qual_ptr=dq.data_ptr(),
                                 seq_ptr=ds.data_ptr(), **batch)
        assert {k: counts[k] for k in ("records", "bytes")} == need, (mode, kept, layout)
        for o in range(3):
            R, B = need["records"][o], need["bytes"][o]
            assert r.canaries_intact(o, R if want[o] is not None else -1, B), (mode, kept, layout, o)
            if want[o] is None:
                continue
            q, s, o_, idx = r.t[o]
            assert np.array_equal(trim_raw.host(q[:B]), want[o]["qual"])
            assert np.array_equal(trim_raw.host(s[:B]), want[o]["seq"])
            assert np.array_equal(trim_raw.host(o_[:R + 1]), want[o]["offsets"])
            assert np.array_equal(trim_raw.host(idx[:R]), want[o]["read_index"])
        return counts
    return nb, run


@pytest.mark.parametrize("n,seed", seeded(wc.TRIM_N))
def test_trim(sk_ctx, n, seed):
    for mode in tm.MODES:
        if mode != "se" and n % 2:
            continue
        big = trim_run(sk_ctx, 6000, "all", "ragged", mode)
        for kept in wc.TRIM_KEPT:
            for layout in wc.TRIM_LAYOUTS:
                nb, run = trim_run(sk_ctx, n, kept, layout, mode)
                sweep(nb, run, big, seed)


# ---- 3 sk_bgzf_device_async ------------------------------------------------------------------------------------------------
BGZF_CASES = [(n, kind) for n in wc.BGZF_LENGTHS for kind in wc.BGZF_KINDS]
BGZF_IDS = ["%d-%s" % c for c in BGZF_CASES]
BGZF_HOSTILE = hostile_of(BGZF_IDS)
BGZF_BIG = wc.bgzf_text("fastq", 5 * 65280 + 7)


@pytest.fixture(scope="module")
def sim_image(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "cpu_shim"), "all"], check=True)
    d = tmp_path_factory.mktemp("workspace_bgzf")

    def image(kind, n):
        if n == 0:
            return b""
        src = str(d / ("%s_%d.txt" % (kind, n)))
        open(src, "wb").write(wc.bgzf_text(kind, n))
        return subprocess.run([SIM, src], capture_output=True, check=True).stdout
    return image


def bgzf_check(text, want, eof, rc, c, out):
    n = len(text)
    assert rc == capi.SK_OK
    got = bgzf_raw.image_of(out, c)
    assert got == want + (bgzf_raw.EOF if eof else b"")
    assert (c["bytes_in"], c["blocks"]) == (n, wc.bgzf_blocks(n))
    assert bgzf_raw.walk(got) == wc.bgzf_blocks(n) + eof and (gzip.decompress(got) if got else b"") == text
    return rc, c, got


@pytest.mark.parametrize("case,seed", seeded(BGZF_IDS))
def test_bgzf(sk_ctx, sim_image, case, seed):
    n, kind = BGZF_CASES[BGZF_IDS.index(case)]
    text = wc.bgzf_text(kind, n)
    want = sim_image(kind, n)
    nb = capi.lib().sk_bgzf_workspace_bytes(n)
    big = (capi.lib().sk_bgzf_workspace_bytes(len(BGZF_BIG)), lambda ws: bgzf_raw.raw(sk_ctx, BGZF_BIG, True, ws=ws))
    for eof in (False, True):

        def run(ws, shift=None, surround=None):
            return bgzf_check(text, want, eof, *bgzf_raw.raw(sk_ctx, text, eof, ws=ws, shift=shift or 0, surround=surround))
        sweep(max(nb, 16), run, big, seed, hostile=fr.HOSTILE_TEXT if case in BGZF_HOSTILE else None)


@pytest.fixture(scope="module")
def search_image(tmp_path_factory):
    import bgzf_search_texts as st
    st.build()
    d = tmp_path_factory.mktemp("workspace_bgzf_search")
    return lambda kind, n: st.host_image(wc.bgzf_text(kind, n), d, "%s_%d" % (kind, n), "eof") if n else bgzf_raw.EOF


@pytest.mark.parametrize("case,seed", seeded(BGZF_IDS))
def test_bgzf_search(sk_ctx, search_image, case, seed):
    """SK_BGZF_SEARCH: the cand section is the last one and sits against the guard"""
    import test_gpu_bgzf_search as tbs
    n, kind = BGZF_CASES[BGZF_IDS.index(case)]
    text = wc.bgzf_text(kind, n)
    want = search_image(kind, n)[:-len(bgzf_raw.EOF)]
    sizes = capi.lib().sk_bgzf_workspace_bytes_flags
    big = (sizes(len(BGZF_BIG), tbs.SEARCH), lambda ws: tbs.raw(sk_ctx, BGZF_BIG, ws=ws))
    for eof in (False, True):
        flags = capi.SK_BGZF_SEARCH | (capi.SK_BGZF_EOF if eof else 0)
        nb = sizes(n, flags)
        assert nb > capi.lib().sk_bgzf_workspace_bytes(n) or n == 0

        def run(ws, shift=None, surround=None):
            return bgzf_check(text, want, eof, *tbs.raw(sk_ctx, text, flags=flags, ws=ws, shift=shift or 0, surround=surround))
        sweep(max(nb, 16), run, big, seed, hostile=fr.HOSTILE_TEXT if case in BGZF_HOSTILE else None)


# ---- 4 sk_bgzf_inflate_device_async ----------------------------------------------------------------------------------------
def bgunzip_images():
    g = {"valid_" + k: v[0] for k, v in bm.images().items()}
    g.update({"bad_" + k: v for k, v in bm.bad_images().items()})
    g.update({"empty_x%d" % k: wc.empty_members(k) for k in wc.EMPTY_MEMBERS})
    g["control_fastq"] = bm.bgzip(wc.many_good(600))
    return {k: (v[0] if isinstance(v, tuple) else v) for k, v in g.items()}


BGUNZIP = bgunzip_images()
BGUNZIP_HOSTILE = hostile_of(sorted(BGUNZIP))
BGUNZIP_BIG = bm.bgzip(BIG_TEXT)
HOSTILE_BGZF = bm.bgzip(b"HOSTILE")  # a complete BGZF member: a candidate for the reader's framing


def bgunzip_case(ctx, name, image, want, text, seed, hostile):
    """want: error, members, bytes_out (and error_member, error_offset); a capacity of exactly the text and one byte short"""
    L = capi.lib()
    nb = L.sk_bgzf_inflate_workspace_bytes(len(image))
    big = (L.sk_bgzf_inflate_workspace_bytes(len(BGUNZIP_BIG)),
           lambda ws: tbu.inflate(ctx, BGUNZIP_BIG, capacity=len(BIG_TEXT), ws=ws))
    caps = [want["bytes_out"]] + ([want["bytes_out"] - 1] if want["bytes_out"] and not want["error"] else [])
    for cap in caps:

        def run(ws, shift=None, surround=None):
            rc, c, out = tbu.inflate(ctx, image, shift=len(name) % 16 if shift is None else shift, capacity=cap, ws=ws,
                                     surround=surround)
            assert (c["error"], c["members"], c["bytes_out"]) == (want["error"], want["members"], want["bytes_out"]), (name, c)
            if want["error"]:
                assert rc == capi.SK_EDATA and (c["error_member"], c["error_offset"]) == (want["error_member"], want["error_offset"])
            elif cap < want["bytes_out"]:
                assert rc == capi.SK_ESPACE and bool((out == bgzf_raw.SENTINEL).all())
            else:
                assert rc == capi.SK_OK and tbu.text_of(out, c) == text
            words = words_of(ws, capi.Context.bgzf_inflate_output_words(ws.data_ptr()))
            return rc, c, (out.cpu().numpy().tobytes() if rc == capi.SK_OK else None), words
        sweep(nb, run, big, seed, hostile=HOSTILE_BGZF if hostile else None)


@pytest.mark.parametrize("name,seed", seeded(sorted(BGUNZIP)))
def test_bgzf_inflate(sk_ctx, name, seed):
    image = BGUNZIP[name]
    want = bm.bgunzip(image)
    bgunzip_case(sk_ctx, name, image, want, None if want["error"] else gzip.decompress(image), seed, name in BGUNZIP_HOSTILE)


@pytest.mark.parametrize("case,seed", seeded(BGZF_IDS))
def test_bgzf_inflate_of_the_device_writers_images(sk_ctx, case, seed):
    n, kind = BGZF_CASES[BGZF_IDS.index(case)]
    text = wc.bgzf_text(kind, n)
    for eof in (False, True):
        if n == 0 and not eof:
            continue  # the image of no text without the EOF member is no image
        image = sk_ctx.bgzf(bgzf_raw.to_device(text) if n else bgzf_raw.to_device(b"x")[:0], eof=eof).cpu().numpy().tobytes()
        want = dict(error=0, members=wc.bgzf_blocks(n) + eof, bytes_out=n)
        bgunzip_case(sk_ctx, case, image, want, text, seed, False)


# ---- 5 sk_gzip_inflate_device_async ----------------------------------------------------------------------------------------
def gunzip_images():
    g = {"valid_" + k: (v[0], 0) for k, v in gm.images().items()}
    g.update({"bad_" + k: v for k, v in gm.bad_images().items()})
    g.update({"foreign_" + k: (v[0], 0) for k, v in fi.valid("gzip").items()})
    g.update({k: (v[0], 0) for k, v in wc.gzip_images().items()})
    g["control_fastq"] = (gzip.compress(wc.many_good(600), 6), 0)
    return g


GUNZIP = gunzip_images()
GUNZIP_HOSTILE = hostile_of(sorted(GUNZIP))
GUNZIP_BIG_TEXT = wc.many_good(5000, seed=5)  # 1.5 MB: two bytes of symbols a text byte, more than the 1 MiB of zeros
GUNZIP_BIG = gzip.compress(GUNZIP_BIG_TEXT, 1)
KEYS = ("error", "error_member", "error_offset", "members", "bytes_out")


def gunzip_big(ctx, monkeypatch):
    """(bytes, run) of the larger call; sized and run at the default chunk"""
    tgp.set_chunk(monkeypatch, 0)
    nb = capi.lib().sk_gzip_inflate_workspace_bytes(len(GUNZIP_BIG), len(GUNZIP_BIG_TEXT))
    return nb, lambda ws: tgu.inflate(ctx, GUNZIP_BIG, capacity=len(GUNZIP_BIG_TEXT), chunk=0, monkeypatch=monkeypatch, ws=ws)


@pytest.mark.parametrize("name,seed", seeded(sorted(GUNZIP)))
def test_gzip_inflate(sk_ctx, monkeypatch, name, seed):
    image, chunk0 = GUNZIP[name]
    want = gm.gunzip(image)
    L = capi.lib()
    chunks = sorted({0, chunk0, 256, 1024}) if len(image) < 100_000 else [0]
    caps = [want["bytes_out"], None] + ([want["bytes_out"] - 1] if want["bytes_out"] and not want["error"] else [])
    big = gunzip_big(sk_ctx, monkeypatch)
    for chunk in chunks:
        for cap in caps:  # None: count only
            count_only = cap is None

            def size():
                tgp.set_chunk(monkeypatch, chunk)  # the formula reads SK_GZIP_CHUNK: set it before the arena is sized
                return L.sk_gzip_inflate_workspace_bytes(len(image), 0 if count_only else cap)

            def run(ws, shift=None, surround=None):
                assert ws.numel() == size()
                rc, c, out = tgu.inflate(sk_ctx, image, shift=len(name) % 16 if shift is None else shift,
                                         capacity=0 if count_only else cap, count_only=count_only, chunk=chunk,
                                         monkeypatch=monkeypatch, ws=ws, surround=surround)
                # a counting call sees headers and Huffman-level damage: no CRC, no ISIZE, and no distance that reaches
                # before its member (bad_far@*), which only the resolve stage meets: it counts such an image as a good one
                unseen = count_only and (want["error"] in (capi.SK_GZ_CRC, capi.SK_GZ_LENGTH) or name.startswith("bad_far"))
                if unseen:
                    # ... or finds damage it does see in a later member (bad_crc_then_header)
                    assert (rc == capi.SK_OK and c["error"] == 0) or \
                        (rc == capi.SK_EDATA and c["error_member"] > want["error_member"]), (name, c)
                    assert c["bytes_out"] >= want["bytes_out"] and c["members"] >= want["members"], (name, c)
                elif want["error"]:
                    assert rc == capi.SK_EDATA and tuple(c[k] for k in KEYS[:3]) == tuple(want[k] for k in KEYS[:3]), (name, c)
                else:
                    assert tuple(c[k] for k in KEYS) == tuple(want[k] for k in KEYS), (name, chunk, c)
                    if count_only:
                        assert rc == capi.SK_OK
                    elif cap < want["bytes_out"]:
                        assert rc == capi.SK_ESPACE and bool((out == bgzf_raw.SENTINEL).all())
                    else:
                        assert rc == capi.SK_OK and tgu.text_of(out, c) == gzip.decompress(image)
                words = words_of(ws, capi.Context.gzip_inflate_output_words(ws.data_ptr()))
                return rc, c, (out.cpu().numpy().tobytes() if rc == capi.SK_OK else None), words
            hostile = name in GUNZIP_HOSTILE or (chunk == 0 and cap == want["bytes_out"])
            sweep(size(), run, big if chunk == 0 else None, seed, hostile=bgzf_raw.hostile_image() if hostile else None)


def test_gzip_inflate_rebased_bit_reader(sk_ctx, monkeypatch):
    """past16m_a of tests/gunzip_model.py, as tests/test_gpu_gunzip.py::test_long_images runs it: one wavefront reads more
    than 16 MiB of image and re-bases its bit reader on the way.  The case names its size; the leftover leg is left out,
    since a larger call would be one of more than 17 MiB of image."""
    image, text, chunk = gm.long_images()["past16m_a"]
    tgp.set_chunk(monkeypatch, chunk)
    nb = capi.lib().sk_gzip_inflate_workspace_bytes(len(image), len(text))
    digest = hash(text)

    def run(ws, shift=None, surround=None):
        rc, c, out = tgu.inflate(sk_ctx, image, shift=9, capacity=len(text), chunk=chunk, monkeypatch=monkeypatch, ws=ws)
        assert rc == capi.SK_OK and (c["error"], c["members"], c["bytes_out"]) == (0, 1, len(text)), c
        got = tgu.text_of(out, c)
        assert got == text
        return rc, c, digest, words_of(ws, capi.Context.gzip_inflate_output_words(ws.data_ptr()))
    sweep(nb, run, None, 16)


PIECE_NAMES = sorted(wc.gzip_images()) + ["control_fastq", "valid_level6", "valid_two"]


@pytest.mark.parametrize("window", [600, 4096])
@pytest.mark.parametrize("name,seed", seeded(PIECE_NAMES))
def test_gzip_inflate_pieces(sk_ctx, monkeypatch, name, seed, window):
    """every piece with a capacity of exactly what the model says it writes"""
    image = GUNZIP[name][0]
    tgp.set_chunk(monkeypatch, 0)
    want, whole = gpm.stream(image, window, 70000)
    want = want[:40]  # the first pieces of the long images: each is a call of its own
    L = capi.lib()
    sizes = [L.sk_gzip_inflate_piece_workspace_bytes(info["window"], len(t)) for w, t, info in want]
    big_bytes = L.sk_gzip_inflate_piece_workspace_bytes(len(GUNZIP_BIG), len(GUNZIP_BIG_TEXT))

    def run(arenas, views, shift=len(name) % 16, surround=None):
        p = tgp.Pieces(sk_ctx, image, len(want) + 1, shift=shift, surround=surround)
        for i, (w, t, info) in enumerate(want):
            p.add(info["window"], len(t), i, i + 1, ws=views[i])
        got = p.finish()
        for a in arenas:
            a.check()
        for i, (g, (w, t, info)) in enumerate(zip(got, want)):
            assert {f: g["state"][f] for f in tgp.FIELDS} == {f: w[f] for f in tgp.FIELDS}, (name, i, g["counts"])
            assert g["rc"] == capi.SK_OK and g["text"] == t, (name, i, g["counts"])
        return got
    first = None
    for lead in guarded.LEADS:
        for poison in guarded.POISONS:
            arenas = [guarded.arena(b, lead, poison, seed=seed) for b in sizes]
            got = run(arenas, [a.ws for a in arenas])
            first = got if first is None else first
            assert got == first, "a piece depends on its workspace (lead %d, %s)" % (lead, poison)
    # the leftovers of a larger piece (one arena for all: the pieces of a stream may share a workspace once finished)
    a = guarded.arena(max(sizes + [big_bytes]), 48, "pattern", seed=seed)
    p = tgp.Pieces(sk_ctx, GUNZIP_BIG, 2)
    p.add(len(GUNZIP_BIG), len(GUNZIP_BIG_TEXT), 0, 1, ws=a.ws[:big_bytes])
    assert p.finish()[0]["rc"] == capi.SK_OK
    for i, (w, t, info) in enumerate(want):  # one at a time on the same leftovers, each refilled by the piece before
        q = tgp.Pieces(sk_ctx, image, len(want) + 1, shift=len(name) % 16, start=first[i - 1]["raw"] if i else None)
        q.add(info["window"], len(t), 0, 1, ws=a.ws[:sizes[i]])
        g = q.finish()[0]
        a.check()
        assert (g["rc"], g["text"], g["raw"]) == (first[i]["rc"], first[i]["text"], first[i]["raw"]), (name, i)
    if name in hostile_of(PIECE_NAMES):
        for shift in (0, 1, 15):
            arenas = [guarded.arena(b, 16, "pattern", seed=seed) for b in sizes]
            assert run(arenas, [a.ws for a in arenas], shift, bgzf_raw.hostile_image()) == first, "hostile, shift %d" % shift
