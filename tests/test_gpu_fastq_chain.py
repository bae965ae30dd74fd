"""GPU: the FASTQ trim with its texts' lengths taken from device words (sk_trim_fastq_chained_device_async), the words the
two gzip readers publish (sk_bgzf_inflate_output_words, sk_gzip_inflate_output_words) and the chain reader -> trim -> BGZF
writer with every finish behind the last enqueue (raw, and Context.trim_gz(text_capacity=...)).  The trim is held to
tests/fastq_model.py and tests/fastq_order_model.py on the exact text text[:n]; the chain to the two-pass Context.trim_gz."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

import bgunzip_model as bm
import cli_util as cu
import fastq_model as fm
import fastq_order_model as om
import fastq_util as fu
import trim_model as tm
from bgzf_raw import EOF, to_device
from fastq_raw import SENTINEL, raw, texts_of, torch_mod, untouched
from sickle_amd import capi
from test_fastq_api import golden_texts

pytestmark = pytest.mark.gpu
PT = ("sanger", 20, 20, False, False)
GUARD = 64
CHUNK = 65536
BASES = np.frombuffer(b"ACGT" * 30 + b"Nn", np.uint8)


# ---- helpers ---------------------------------------------------------------------------------------------------------
def good_records(seed, total=200_000):
    """Seeded good records of mixed lengths (reads of 20 .. 300 bases, names and '+' lines of several sizes, quality
    levels that keep, cut and drop reads at -q 20), about `total` bytes."""
    rng = np.random.default_rng(seed)
    recs, size = [], 0
    while size < total:
        L = int(rng.integers(20, 301))
        level = int(rng.choice([35, 50, 60, 70]))
        qual = np.clip(level + rng.integers(-6, 7, L), 33, 126).astype(np.uint8).tobytes()
        name = b"@r%d" % len(recs) + b"x" * int(rng.integers(0, 30))
        plus = b"+" + (name[1:] if rng.random() < 0.2 else b"")
        recs.append(name + b"\n" + rng.choice(BASES, L).tobytes() + b"\n" + plus + b"\n" + qual + b"\n")
        size += len(recs[-1])
    return recs


def place(data, shift):
    """data (bytes) on the device `shift` bytes past a 16-byte boundary -> (tensor that keeps it alive, address)"""
    torch = torch_mod()
    buf = torch.zeros(len(data) + shift + 16, dtype=torch.uint8, device="cuda")
    if len(data):
        buf[shift:shift + len(data)] = to_device(data)
    return buf, buf.data_ptr() + shift


def word(value):
    torch = torch_mod()
    return torch.tensor([value], dtype=torch.int64, device="cuda")


def chained(ctx, ptuple, ptrs, bounds, mode, ns=(), valids=(), order=None, no_lengths=False, index=True, ws=None):
    """One sk_trim_fastq_chained_device_async + finish on raw pointers, every output pre-filled with SENTINEL and GUARD
    more bytes / entries behind its capacity.  ptrs / bounds: the texts' addresses and in->bytes; ns / valids: the values of
    the device words (None = no such word).  ws: the workspace tensor, used as it is (the byte count handed to the library
    stays the formula's).  -> (rc, counts (with "order" in ordered calls), keep, batch table or None)"""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*ptuple)
    T = sum(bounds)
    if order is None:
        ws_bytes = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    else:
        ws_bytes = L.sk_trim_fastq_ordered_workspace_bytes(T, params.trunc_n, order.batch_capacity)
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    cap, rcap = T + 64, T // 4 + 4
    outs, keep = [], []
    for o in range(3):
        t = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        ix = torch.full((rcap + GUARD,), -7, dtype=torch.int64, device="cuda") if index else None
        outs.append(capi.FastqOutput(t.data_ptr(), cap, ix.data_ptr() if index else None, rcap))
        keep.append((t, ix))
    pad = lambda xs: list(xs) + [None] * (2 - len(xs))
    wn = [None if n is None else word(n) for n in pad(ns)]
    wv = [None if v is None else word(v) for v in pad(valids)]
    ptr_of = lambda w: None if w is None else w.data_ptr()
    inp = capi.FastqInput((C.c_void_p * 2)(*pad(ptrs)), (C.c_uint64 * 2)(*(list(bounds) + [0] * (2 - len(bounds)))), 0)
    lengths = capi.FastqLengths((C.c_void_p * 2)(*[ptr_of(w) for w in wn]), (C.c_void_p * 2)(*[ptr_of(w) for w in wv]))
    rc = L.sk_trim_fastq_chained_device_async(ctx._h, C.byref(params), C.byref(inp), None if no_lengths else C.byref(lengths),
                                              capi.TRIM_MODES[mode], None if order is None else C.byref(order),
                                              (capi.FastqOutput * 3)(*outs), ws.data_ptr(), ws_bytes, None)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    c = capi.FastqCounts()
    if order is None:
        rc = L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
        counts, table = c.as_dict(), None
    else:
        oc = capi.FastqOrderCounts()
        rc = L.sk_trim_fastq_ordered_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(oc))
        counts = dict(c.as_dict(), order=oc.as_dict())
        nb = min(counts["order"]["batches"], order.batch_capacity)
        at = capi.Context.trim_fastq_ordered_batches(ws.data_ptr()) - ws.data_ptr()
        table = ws[at:at + 8 * (nb + 1)].cpu().numpy().view(np.uint64).astype(np.int64).tolist()
    for t, ix in keep:
        assert bool((t[cap:] == SENTINEL).all()) and (ix is None or bool((ix[rcap:] == -7).all())), "a guard was written"
    return rc, counts, keep, table


def compare(ctx, want, rc, counts, keep, mode):
    """tests/fastq_raw.py's check, on a call that has been made: verdict, range error or every text, index and count."""
    assert counts["records_in"] == want["records_in"] and counts["tail_lines"] == want["tail_lines"]
    assert counts["dropped_unpaired"] == want["dropped_unpaired"]
    if want["verdict"] is not None:
        assert rc == capi.SK_EFORMAT
        assert (counts["format_error"], counts["format_input"], counts["format_record"]) == want["verdict"]
        untouched(keep)
        return
    if want["range"] is not None:
        assert rc == capi.SK_ERANGE and counts["range"] == tuple(want["range"])
        untouched(keep)
        return
    assert rc == capi.SK_OK, capi.lib().sk_last_error(ctx._h)
    got = texts_of(keep, counts)
    for o in range(3):
        if o not in fm.USED[mode]:
            assert bool((keep[o][0] == SENTINEL).all())
            continue
        assert got[o] == want["texts"][o], "output %d" % o
        assert counts["records"][o] == len(want["index"][o]) and counts["bytes"][o] == len(want["texts"][o])
        assert bool((keep[o][0][counts["bytes"][o]:] == SENTINEL).all())
        if keep[o][1] is not None:
            assert np.array_equal(keep[o][1][:counts["records"][o]].cpu().numpy(), want["index"][o])
            assert bool((keep[o][1][counts["records"][o]:] == -7).all())


# ---- 1 a device length is the exact text -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact():
    """the text of test 1 and a cache of the model's results on its prefixes, shared by the test's cases"""
    recs = good_records(41)
    return {"recs": recs, "text": b"".join(recs), "want": {}}


def lengths_under_test(recs, text, sh):
    B = len(text)
    starts = np.concatenate(([0], np.cumsum([len(r) for r in recs])))
    k = int(np.searchsorted(starts, 70_000))  # a record in the second 64 KiB chunk
    r = int(starts[k])
    ns = {0, 1, 7, 8, r - 1, r, r + 1, B - 1, B}
    p = r
    for line in recs[k].split(b"\n")[:4]:
        p += len(line)  # the line's '\n'
        ns |= {p - 1, p, p + 1, p + 2}  # the text ends before the byte before it, before it, behind it, a byte later
        p += 1
    ns |= {v - sh for v in (65535, 65536, 65537, 131072)}
    assert any(text[n - 1] != 10 and text[n] == 10 for n in ns if 0 < n < B)
    assert all(0 <= n <= B for n in ns) and B > 3 * CHUNK
    return sorted(ns)


@pytest.mark.parametrize("shift", [0, 9])
@pytest.mark.parametrize("mode", ["se", "pe_interleaved"])
def test_device_length_is_the_exact_text(sk_ctx, exact, mode, shift):
    """The buffer holds the whole text (an over-read shows as extra records), then newlines behind n (an over-read shows
    as extra lines): the call with *bytes_dev = n gives what the model gives on text[:n]."""
    recs, text = exact["recs"], exact["text"]
    B = len(text)
    whole = place(text, shift)
    for n in lengths_under_test(recs, text, shift):
        if (mode, n) not in exact["want"]:
            exact["want"][mode, n] = fm.expected(PT, [text[:n]], mode)
        want = exact["want"][mode, n]
        for keep_buf, ptr in (whole, place(text[:n] + b"\n" * (B - n), shift)):
            rc, counts, keep, _ = chained(sk_ctx, PT, [ptr], [B], mode, ns=[n])
            compare(sk_ctx, want, rc, counts, keep, mode)


# ---- 2 the words' edge values, the argument checks -------------------------------------------------------------------
def test_word_edge_values(sk_ctx, exact):
    text = exact["text"][:70_001]  # ends inside a record: an unterminated last line
    B = len(text)
    buf, ptr = place(text, 5)
    for mode in ("se", "pe_interleaved"):
        want = fm.expected(PT, [text], mode)
        for n in (B, B + 1, 1 << 62):  # a larger word is taken as the bound
            rc, counts, keep, _ = chained(sk_ctx, PT, [ptr], [B], mode, ns=[n])
            compare(sk_ctx, want, rc, counts, keep, mode)
        for valid in (1, 7):
            rc, counts, keep, _ = chained(sk_ctx, PT, [ptr], [B], mode, ns=[B], valids=[valid])
            compare(sk_ctx, want, rc, counts, keep, mode)
        # *valid_dev == 0: the existing call with bytes = 0
        rc0, counts0, keep0 = raw(sk_ctx, capi.make_params(*PT), [b""], mode)
        for ns in ([B], [None], [1 << 62]):
            rc, counts, keep, _ = chained(sk_ctx, PT, [ptr], [B], mode, ns=ns, valids=[0])
            assert (rc, counts) == (rc0, counts0) and rc == capi.SK_OK and counts["records_in"] == [0, 0]
            untouched(keep)
        # no lengths at all, and a struct of four NULLs: sk_trim_fastq_device_async on the same text
        rc0, counts0, keep0 = raw(sk_ctx, capi.make_params(*PT), [text], mode, shift=5)
        for kw in (dict(no_lengths=True), dict(ns=[None], valids=[None])):
            rc, counts, keep, _ = chained(sk_ctx, PT, [ptr], [B], mode, **kw)
            assert (rc, counts) == (rc0, counts0)
            assert texts_of(keep, counts) == texts_of(keep0, counts0)
            for o in fm.USED[mode]:
                R = counts["records"][o]
                assert np.array_equal(keep[o][1][:R].cpu().numpy(), keep0[o][1][:R].cpu().numpy())


def test_bad_words_enqueue_nothing(sk_ctx, exact):
    torch = torch_mod()
    L = capi.lib()
    text = exact["text"][:5000]
    buf, ptr = place(text, 0)
    params = capi.make_params(*PT)
    ws_bytes = L.sk_trim_fastq_workspace_bytes(2 * len(text), 0)
    ws = torch.full((ws_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    w = torch.zeros(4, dtype=torch.int64, device="cuda")
    out = torch.full((len(text) + 64,), SENTINEL, dtype=torch.uint8, device="cuda")

    def call(mode, lengths, two=False):
        inp = capi.FastqInput((C.c_void_p * 2)(ptr, ptr if two else None), (C.c_uint64 * 2)(len(text), len(text) if two else 0), 0)
        ln = capi.FastqLengths((C.c_void_p * 2)(*lengths[0]), (C.c_void_p * 2)(*lengths[1]))
        outs = (capi.FastqOutput * 3)(capi.FastqOutput(out.data_ptr(), len(text) + 64, None, 0))
        return L.sk_trim_fastq_chained_device_async(sk_ctx._h, C.byref(params), C.byref(inp), C.byref(ln), capi.TRIM_MODES[mode],
                                                    None, outs, ws.data_ptr(), ws_bytes, None)

    a = w.data_ptr()
    assert call("se", ((a + 4, None), (None, None))) == capi.SK_EINVAL
    assert call("se", ((a, None), (a + 9, None))) == capi.SK_EINVAL
    assert call("pe_split", ((a, a + 8), (a + 16, a + 28)), two=True) == capi.SK_EINVAL
    assert call("se", ((a, a + 8), (None, None))) == capi.SK_EINVAL  # a word for text[1] outside SK_TRIM_PE_SPLIT
    assert call("pe_interleaved", ((a, None), (None, a + 8))) == capi.SK_EINVAL
    torch.cuda.synchronize()
    assert bool((ws == SENTINEL).all()) and bool((out == SENTINEL).all()), "a refused call enqueued something"
    assert call("pe_split", ((a, a + 8), (a + 16, a + 24)), two=True) == capi.SK_OK  # all words 0: two empty texts
    c = capi.FastqCounts()
    assert L.sk_trim_fastq_device_finish(sk_ctx._h, ws.data_ptr(), None, C.byref(c)) == capi.SK_OK
    assert list(c.records_in) == [0, 0]


# ---- 3 two texts, two words -------------------------------------------------------------------------------------------
def test_pe_split_two_words(sk_ctx):
    ra, rb = good_records(42, 150_000), good_records(43, 150_000)
    ta, tb = b"".join(ra), b"".join(rb)
    end = lambda recs, k: sum(len(r) for r in recs[:k])
    ba, bb = place(ta, 3), place(tb, 12)
    seen = set()
    for ka, kb, extra in ((400, 400, 0), (400, 399, 0), (380, 400, 0), (400, 400, 17), (300, 300, -1)):
        na, nb = end(ra, ka), end(rb, kb) + extra
        assert na != nb
        want = fm.expected(PT, [ta[:na], tb[:nb]], "pe_split")
        rc, counts, keep, _ = chained(sk_ctx, PT, [ba[1], bb[1]], [len(ta), len(tb)], "pe_split", ns=[na, nb])
        compare(sk_ctx, want, rc, counts, keep, "pe_split")
        seen.add(want["verdict"])
    # a pair count that differs: SK_FQ_PAIR_COUNT at the first record without a mate, in either input
    assert (fm.SK_FQ_PAIR_COUNT, 0, 399) in seen and (fm.SK_FQ_PAIR_COUNT, 1, 380) in seen and None in seen
    # interleaved with an odd record count: the last record is dropped after its check
    want = fm.expected(PT, [ta[:end(ra, 401)]], "pe_interleaved")
    assert want["dropped_unpaired"] == 1 and want["verdict"] is None
    rc, counts, keep, _ = chained(sk_ctx, PT, [ba[1]], [len(ta)], "pe_interleaved", ns=[end(ra, 401)])
    compare(sk_ctx, want, rc, counts, keep, "pe_interleaved")


# ---- 4 the -a T order --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["se", "pe_interleaved"])
def test_ordered_with_a_device_length(sk_ctx, exact, mode):
    """T = 3, batches of about 3 000 bytes: n on the kernel's chunk boundary, on a record boundary and in mid-record,
    against tests/fastq_order_model.py on text[:n]."""
    recs, text = exact["recs"], exact["text"][:150_000]
    B, sh, threads, batch_len = len(text), 9, 3, 3000
    starts = np.concatenate(([0], np.cumsum([len(r) for r in recs])))
    r = int(starts[int(np.searchsorted(starts, 100_000))])
    buf, ptr = place(text, sh)
    for n in (CHUNK - sh, r, r + 40, B):
        want = om.expected(PT, [text[:n]], mode, threads, batch_len)
        assert want["long_line"] is None
        order = capi.FastqOrder(threads, 0, batch_len, B // batch_len + 16, 0)
        rc, counts, keep, table = chained(sk_ctx, PT, [ptr], [B], mode, ns=[n], order=order)
        oc = counts["order"]
        assert {k: oc[k] for k in want["order"]} == want["order"] and table == want["tables"]["first_unit"]
        assert oc["error_batch"] == want["error_batch"]
        compare(sk_ctx, dict(want, dropped_unpaired=0), rc, counts, keep, mode)


# ---- 5 the readers' words ------------------------------------------------------------------------------------------------
def reader(ctx, kind, image, capacity, count_only=False):
    """One reader call + finish -> (rc, counts, value of *bytes_dev, value of *written_dev, out[:capacity])"""
    torch = torch_mod()
    L = capi.lib()
    buf, ptr = place(image, 0)
    if kind == "bgzf":
        ws_bytes = L.sk_bgzf_inflate_workspace_bytes(len(image))
        run, fin, words, c = L.sk_bgzf_inflate_device_async, L.sk_bgzf_inflate_device_finish, \
            capi.Context.bgzf_inflate_output_words, capi.BgzfInflateCounts()
    else:
        ws_bytes = L.sk_gzip_inflate_workspace_bytes(len(image), 0 if count_only else capacity)
        run, fin, words, c = L.sk_gzip_inflate_device_async, L.sk_gzip_inflate_device_finish, \
            capi.Context.gzip_inflate_output_words, capi.GzipInflateCounts()
    ws = torch.full((ws_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((capacity + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = run(ctx._h, ptr, len(image), None if count_only else out.data_ptr(), 0 if count_only else capacity, ws.data_ptr(),
             ws_bytes, None)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    rc = fin(ctx._h, ws.data_ptr(), None, C.byref(c))
    b, w = words(ws.data_ptr())
    hdr = ws[:256].cpu().numpy().view(np.uint64)
    assert bool((out[capacity:] == SENTINEL).all())
    return rc, c.as_dict(), int(hdr[(b - ws.data_ptr()) // 8]), int(hdr[(w - ws.data_ptr()) // 8]), out[:capacity]


def flip_crc(kind, image):
    """the image with one byte of its first member's CRC-32 flipped"""
    at = (struct.unpack_from("<H", image, 16)[0] + 1 if kind == "bgzf" else len(image)) - 8
    return image[:at] + bytes([image[at] ^ 0x40]) + image[at + 1:]


def image_of(kind, text, level=6):
    return bm.bgzip(text, level=level) if kind == "bgzf" else gzip.compress(text, level)


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
def test_reader_words(sk_ctx, exact, kind):
    text = exact["text"][:150_000]
    image = image_of(kind, text)
    need = len(text)
    for cap in (need, need + 70_000):
        rc, c, nbytes, written, out = reader(sk_ctx, kind, image, cap)
        assert (rc, c["bytes_out"], nbytes, written) == (capi.SK_OK, need, need, 1)
        assert out[:need].cpu().numpy().tobytes() == text
    rc, c, nbytes, written, out = reader(sk_ctx, kind, image, need, count_only=True)
    assert (rc, c["bytes_out"], nbytes, written) == (capi.SK_OK, need, need, 0)
    rc, c, nbytes, written, out = reader(sk_ctx, kind, image, need - 1)
    assert (rc, c["bytes_out"], nbytes, written) == (capi.SK_ESPACE, need, need, 0)
    assert bool((out == SENTINEL).all())
    rc, c, nbytes, written, out = reader(sk_ctx, kind, flip_crc(kind, image), need)
    assert (rc, c["error"], written) == (capi.SK_EDATA, capi.SK_GZ_CRC, 0) and nbytes == c["bytes_out"]
    rc, c, nbytes, written, out = reader(sk_ctx, kind, image[:len(image) // 2], need)  # a framing-level failure
    assert rc == capi.SK_EDATA and written == 0


# ---- 6 the whole chain, raw ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_chain")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


RUNS = [pytest.param(name, rec, id=name) for name, rec in tm.golden_runs() if name not in tm.UNREPLAYABLE]


@pytest.fixture(scope="module")
def two_pass(sk_ctx, workdir):
    """(name, kind) -> what the two-pass Context.trim_gz gives on that golden run's inputs: computed once, shared"""
    cache = {}

    def get(name, rec, kind):
        if (name, kind) not in cache:
            mode, texts, files = golden_texts(rec["argv"], workdir)
            images = [image_of(kind, t, level=1 + k) for k, t in enumerate(texts)]
            params = capi.make_params(*tm.run_params(rec["argv"]))
            zz = [to_device(z) for z in images]
            got, counts = sk_ctx.trim_gz(params, zz[0], zz[1] if len(zz) > 1 else None, mode=mode)
            cache[name, kind] = dict(mode=mode, texts=texts, images=images, params=params, counts=counts,
                                     out=[None if g is None else g.cpu().numpy().tobytes() for g in got])
        return cache[name, kind]
    return get


def chain_raw(ctx, params, images, kinds, caps, mode):
    """reader(s) -> chained trim -> BGZF writers, every call on raw pointers into sentinel-filled buffers, every finish
    behind the last enqueue.  -> dict(readers: [(rc, counts)], writers: [(rc, counts) or None], trim: (rc, counts),
    images: [bytes or None])"""
    torch = torch_mod()
    L = capi.lib()
    full = lambda n: torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    hold, readers, ptrs, nb, va = [], [], [], [], []
    for image, kind, cap in zip(images, kinds, caps):
        buf, ptr = place(image, 0)
        text = full(cap + GUARD)
        if kind == "bgzf":
            ws = full(L.sk_bgzf_inflate_workspace_bytes(len(image)))
            rc = L.sk_bgzf_inflate_device_async(ctx._h, ptr, len(image), text.data_ptr(), cap, ws.data_ptr(), ws.numel(), None)
            b, w = capi.Context.bgzf_inflate_output_words(ws.data_ptr())
            readers.append((L.sk_bgzf_inflate_device_finish, ws, capi.BgzfInflateCounts()))
        else:
            ws = full(L.sk_gzip_inflate_workspace_bytes(len(image), cap))
            rc = L.sk_gzip_inflate_device_async(ctx._h, ptr, len(image), text.data_ptr(), cap, ws.data_ptr(), ws.numel(), None)
            b, w = capi.Context.gzip_inflate_output_words(ws.data_ptr())
            readers.append((L.sk_gzip_inflate_device_finish, ws, capi.GzipInflateCounts()))
        assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
        hold += [buf, text]
        ptrs.append(text.data_ptr())
        nb.append(b)
        va.append(w)
    T = sum(caps)
    ws_bytes = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    ws = full(ws_bytes)
    ocap = T + 2
    bound = L.sk_bgzf_bound(ocap, capi.SK_BGZF_EOF)
    zws_bytes = L.sk_bgzf_workspace_bytes(ocap)
    outs, trimmed = [capi.FastqOutput() for _ in range(3)], [None] * 3
    for o in fm.USED[mode]:
        trimmed[o] = full(ocap + GUARD)
        outs[o] = capi.FastqOutput(trimmed[o].data_ptr(), ocap, None, 0)
    pad = lambda xs: list(xs) + [None] * (2 - len(xs))
    inp = capi.FastqInput((C.c_void_p * 2)(*pad(ptrs)), (C.c_uint64 * 2)(*(list(caps) + [0] * (2 - len(caps)))), 0)
    lengths = capi.FastqLengths((C.c_void_p * 2)(*pad(nb)), (C.c_void_p * 2)(*pad(va)))
    rc = L.sk_trim_fastq_chained_device_async(ctx._h, C.byref(params), C.byref(inp), C.byref(lengths), capi.TRIM_MODES[mode],
                                              None, (capi.FastqOutput * 3)(*outs), ws.data_ptr(), ws_bytes, None)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    writers = [None] * 3
    for o in fm.USED[mode]:
        img, zws = full(bound + GUARD), full(zws_bytes)
        b, w = capi.Context.trim_fastq_output_words(ws.data_ptr(), o)
        zin = capi.BgzfInput(trimmed[o].data_ptr(), ocap, b, w)
        rc = L.sk_bgzf_device_async(ctx._h, C.byref(zin), img.data_ptr(), bound, capi.SK_BGZF_EOF, zws.data_ptr(), zws_bytes, None)
        assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
        writers[o] = (img, zws)
    # everything is enqueued: only now does anything wait
    res = {"readers": [], "writers": [None] * 3, "images": [None] * 3}
    for fin, rws, c in readers:
        rc = fin(ctx._h, rws.data_ptr(), None, C.byref(c))
        res["readers"].append((rc, c.as_dict()))
    for o in fm.USED[mode]:
        img, zws = writers[o]
        c = capi.BgzfCounts()
        rc = L.sk_bgzf_device_finish(ctx._h, zws.data_ptr(), None, C.byref(c))
        res["writers"][o] = (rc, c.as_dict())
        assert bool((img[c.bytes_out:] == SENTINEL).all())
        res["images"][o] = img[:c.bytes_out].cpu().numpy().tobytes()
    c = capi.FastqCounts()
    rc = L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
    res["trim"] = (rc, c.as_dict())
    for t, cap in zip(hold[1::2], caps):
        assert bool((t[cap:] == SENTINEL).all()), "a reader wrote beyond its capacity"
    for o in fm.USED[mode]:
        assert bool((trimmed[o][ocap:] == SENTINEL).all())
    return res


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
@pytest.mark.parametrize("name,rec", RUNS)
def test_whole_chain_raw(sk_ctx, two_pass, name, rec, kind):
    want = two_pass(name, rec, kind)
    caps = [len(t) + 70_000 for t in want["texts"]]
    res = chain_raw(sk_ctx, want["params"], want["images"], [kind] * len(caps), caps, want["mode"])
    for (rc, c), t in zip(res["readers"], want["texts"]):
        assert rc == capi.SK_OK and c["bytes_out"] == len(t)
    assert res["trim"] == (capi.SK_OK, want["counts"])
    for o in range(3):
        assert res["images"][o] == want["out"][o], "image %d" % o
        if want["out"][o] is not None:
            assert res["writers"][o][0] == capi.SK_OK and res["writers"][o][1]["bytes_in"] == want["counts"]["bytes"][o]


# ---- 7 an upstream failure goes through the chain --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
def test_upstream_failure_through_the_chain(sk_ctx, two_pass, kind):
    name, rec = next((n, r) for n, r in tm.golden_runs() if n.startswith("pe_inter_illumina"))
    want = two_pass(name, rec, kind)
    mode, text, image = want["mode"], want["texts"][0], want["images"][0]
    bad = flip_crc(kind, image)
    res = chain_raw(sk_ctx, want["params"], [bad], [kind], [len(text)], mode)
    assert res["readers"][0][0] == capi.SK_EDATA and res["readers"][0][1]["error"] == capi.SK_GZ_CRC
    rc, counts = res["trim"]
    assert rc == capi.SK_OK and counts["records_in"] == [0, 0] and counts["records"] == [0, 0, 0]
    for o in range(3):
        assert res["images"][o] == (EOF if o in fm.USED[mode] else None)
    # a capacity one byte short: the same, by SK_ESPACE
    res = chain_raw(sk_ctx, want["params"], [image], [kind], [len(text) - 1], mode)
    assert res["readers"][0][0] == capi.SK_ESPACE and res["readers"][0][1]["bytes_out"] == len(text)
    assert res["trim"][0] == capi.SK_OK and res["trim"][1]["records_in"] == [0, 0]
    assert all(res["images"][o] == EOF for o in fm.USED[mode])
    # Context.trim_gz
    with pytest.raises(capi.GzDataError) as e:
        sk_ctx.trim_gz(want["params"], to_device(bad), mode=mode, text_capacity=len(text), kind=kind)
    assert e.value.reason == capi.SK_GZ_CRC
    z = to_device(image)
    with pytest.raises(capi.TrimError) as e:
        sk_ctx.trim_gz(want["params"], z, mode=mode, text_capacity=len(text) // 2, kind=kind)
    assert e.value.rc == capi.SK_ESPACE and e.value.counts["bytes_out"] == len(text)
    got, counts = sk_ctx.trim_gz(want["params"], z, mode=mode, text_capacity=e.value.counts["bytes_out"], kind=kind)
    assert counts == want["counts"]
    assert [None if g is None else g.cpu().numpy().tobytes() for g in got] == want["out"]
    assert e.value.readers == [e.value.counts]
    # the same with order: the reader's errors pass the retry for a batch table that was too small, and the second call
    # with the need gives what the two-pass ordered call gives
    order = (3, 5000)
    with pytest.raises(capi.GzDataError):
        sk_ctx.trim_gz(want["params"], to_device(bad), mode=mode, text_capacity=len(text), kind=kind, order=order)
    with pytest.raises(capi.TrimError) as e:
        sk_ctx.trim_gz(want["params"], z, mode=mode, text_capacity=len(text) - 1, kind=kind, order=order)
    assert e.value.rc == capi.SK_ESPACE and e.value.counts["bytes_out"] == len(text) and "order" not in e.value.counts
    got, counts = sk_ctx.trim_gz(want["params"], z, mode=mode, text_capacity=e.value.counts["bytes_out"], kind=kind, order=order)
    ref, ref_counts = sk_ctx.trim_gz(want["params"], z, mode=mode, order=order)
    assert counts == ref_counts and counts["order"]["batches"] > 1
    assert all((g is None and r is None) or torch_mod().equal(g, r) for g, r in zip(got, ref))


def test_two_short_capacities_are_learnt_in_one_call(sk_ctx, two_pass):
    """Two images, both capacities short: the error is the first image's, and `readers` holds both needs."""
    name, rec = next((n, r) for n, r in tm.golden_runs() if n == "pe_fr_illumina")
    want = two_pass(name, rec, "bgzf")
    zz = [to_device(z) for z in want["images"]]
    sizes = [len(t) for t in want["texts"]]
    with pytest.raises(capi.TrimError) as e:
        sk_ctx.trim_gz(want["params"], zz[0], zz[1], mode=want["mode"], text_capacity=[sizes[0] - 1, 100])
    assert e.value.rc == capi.SK_ESPACE and e.value.counts["bytes_out"] == sizes[0]
    assert [c["bytes_out"] for c in e.value.readers] == sizes
    got, counts = sk_ctx.trim_gz(want["params"], zz[0], zz[1], mode=want["mode"],
                                 text_capacity=[c["bytes_out"] for c in e.value.readers])
    assert counts == want["counts"]
    assert [None if g is None else g.cpu().numpy().tobytes() for g in got] == want["out"]


# ---- 8 trim_gz: one pass equals two -----------------------------------------------------------------------------------------
def one_pass(ctx, want, **kw):
    zz = [to_device(z) for z in want["images"]]
    got, counts = ctx.trim_gz(want["params"], zz[0], zz[1] if len(zz) > 1 else None, mode=want["mode"], **kw)
    return [None if g is None else g.cpu().numpy().tobytes() for g in got], counts


@pytest.mark.parametrize("name,rec", RUNS)
def test_trim_gz_one_pass_equals_two_pass(sk_ctx, two_pass, name, rec):
    """at the exact capacity, and with slack (one value for both images)"""
    want = two_pass(name, rec, "bgzf")
    sizes = [len(t) for t in want["texts"]]
    for cap in (sizes, max(sizes) + 12_345):
        got, counts = one_pass(sk_ctx, want, text_capacity=cap if isinstance(cap, int) or len(cap) > 1 else cap[0])
        assert counts == want["counts"] and got == want["out"]


def test_trim_gz_one_pass_variants(sk_ctx, two_pass, workdir):
    runs = dict(tm.golden_runs())
    # kind=None on plain gzip (and on BGZF), kind named
    for name in ("pe_fr_illumina_n", "pe_inter_illumina"):
        for kind in ("gzip", "bgzf"):
            want = two_pass(name, runs[name], kind)
            assert capi.Context._gz_kind(to_device(want["images"][0])) == kind
            sizes = [len(t) + 1000 for t in want["texts"]]
            for k in (None, kind, "gzip"):  # the gzip reader reads BGZF too
                got, counts = one_pass(sk_ctx, want, text_capacity=sizes, kind=k)
                assert counts == want["counts"] and got == want["out"], (name, kind, k)
    # search=True and order pass through: against the two-pass call with the same arguments
    name = "pe_fr_illumina"
    want = two_pass(name, runs[name], "bgzf")
    zz = [to_device(z) for z in want["images"]]
    sizes = [len(t) + 5000 for t in want["texts"]]
    first = runs[name]["argv"][runs[name]["argv"].index("-f") + 1]
    budget = fu.reference_batch_len(os.path.getsize(first.format(inputs=cu.INPUTS, tmp=str(workdir))), paired=True)
    for kw in (dict(search=True), dict(order=(3, budget)), dict(order=(2, 5000))):
        ref, ref_counts = sk_ctx.trim_gz(want["params"], zz[0], zz[1], mode=want["mode"], **kw)
        got, counts = one_pass(sk_ctx, want, text_capacity=sizes, **kw)
        assert counts == ref_counts
        assert got == [None if g is None else g.cpu().numpy().tobytes() for g in ref]
        if "order" in kw:
            assert counts["order"]["batches"] > 1


# ---- 9 a seeded slice of the soak's texts -----------------------------------------------------------------------------------
def draw_length(rng, text, shift):
    """a length for a drawn text: the bound, nothing, anywhere, next to a newline, next to a framing-chunk boundary"""
    B = len(text)
    how = rng.random()
    if how < 0.15 or B == 0:
        return B
    if how < 0.2:
        return 0
    if how < 0.55:
        return int(rng.integers(0, B + 1))
    if how < 0.8:
        nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)
        if len(nl):
            return int(np.clip(int(rng.choice(nl)) + int(rng.integers(-1, 3)), 0, B))
    chunks = (B + shift) // CHUNK
    if chunks:
        return int(np.clip(int(rng.integers(1, chunks + 1)) * CHUNK - shift + int(rng.integers(-1, 2)), 0, B))
    return int(rng.integers(0, B + 1))


def test_seeded_slice_of_the_soak(sk_ctx):
    """200 (text, n, shift, mode) cases from tests/soak_fastq.py's generator (placed newlines, lines over chunks, endings,
    malformed records, qualities out of range, every mode and encoding), each text cut at a drawn n by a device word."""
    import soak_fastq
    rng, rng_n = np.random.default_rng(2031), np.random.default_rng(2032)
    outcomes = {}
    for it in range(200):
        c = soak_fastq.draw(rng)
        ns = [draw_length(rng_n, t, c["shift"]) for t in c["texts"]]
        want = fm.expected(tuple(c["params"]), [t[:n] for t, n in zip(c["texts"], ns)], c["mode"])
        bufs = [place(t, c["shift"]) for t in c["texts"]]
        rc, counts, keep, _ = chained(sk_ctx, tuple(c["params"]), [b[1] for b in bufs], [len(t) for t in c["texts"]],
                                      c["mode"], ns=ns, index=c["index"])
        try:
            compare(sk_ctx, want, rc, counts, keep, c["mode"])
        except AssertionError as e:
            raise AssertionError("iteration %d: mode %s, shift %d, params %r, bounds %r, n %r: %s" % (
                it, c["mode"], c["shift"], c["params"], [len(t) for t in c["texts"]], ns, e)) from None
        outcomes[rc] = outcomes.get(rc, 0) + 1
    print("outcomes of the slice:", outcomes)
    assert outcomes.get(capi.SK_OK, 0) >= 50 and outcomes.get(capi.SK_EFORMAT, 0) >= 20
