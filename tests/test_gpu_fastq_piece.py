"""GPU: the FASTQ trim in pieces: the window start and the piece rule of sk_trim_fastq_piece_device_async, the words a
piece publishes, its finish (every verdict from its own workspace), the carry kernel (sk_fastq_carry_device_async), many
pieces enqueued on one stream before any finish, and the drivers Context.trim_fastq_stream / trim_gz_stream.  The device is
held to tests/fastq_model.py on the exact window and to tests/fastq_piece_model.py for the piece rule."""
import ctypes as C
import gzip

import numpy as np
import pytest

import cli_util as cu
import fastq_model as fm
import fastq_piece_model as pm
import soak_fastq
import trim_model as tm
from bgzf_raw import EOF, to_device
from fastq_raw import SENTINEL, torch_mod, untouched
from sickle_amd import capi
from test_fastq_api import golden_texts
from test_gpu_fastq_chain import chained, compare, good_records, place, word

pytestmark = pytest.mark.gpu
PT = ("sanger", 20, 20, False, False)
GUARD = 64
BAD = b"@bad\nACGT\n+\nIII\n"
LOW = b"@low\n" + b"ACGT" * 10 + b"\n+\nII\x1f" + b"I" * 37 + b"\n"  # a quality byte below sanger's range


# ---- helpers ---------------------------------------------------------------------------------------------------------
class Call:
    """One sk_trim_fastq_piece_device_async on raw pointers, every output pre-filled with SENTINEL and GUARD more bytes /
    entries behind its capacity; finish() -> (rc, counts with "piece")."""

    def __init__(self, ctx, ptuple, ptrs, bounds, mode, ns=(), valids=(), starts=(), more=False, piece=True, index=True,
                 ws=None):
        torch = torch_mod()
        L = capi.lib()
        self.ctx, self.mode = ctx, mode
        params = capi.make_params(*ptuple)
        T = sum(bounds)
        self.ws_bytes = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device="cuda") if ws is None else ws
        self.cap, self.rcap = T + 64, T // 4 + 4
        outs, self.keep = [], []
        for o in range(3):
            t = torch.full((self.cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
            ix = torch.full((self.rcap + GUARD,), -7, dtype=torch.int64, device="cuda") if index else None
            outs.append(capi.FastqOutput(t.data_ptr(), self.cap, ix.data_ptr() if index else None, self.rcap))
            self.keep.append((t, ix))
        pad = lambda xs: list(xs) + [None] * (2 - len(xs))
        as_ptr = lambda v: v if v is None or isinstance(v, int) else v.data_ptr()
        self.words = [v for v in list(ns) + list(valids) + list(starts) if v is not None and not isinstance(v, int)]
        inp = capi.FastqInput((C.c_void_p * 2)(*pad(ptrs)), (C.c_uint64 * 2)(*(list(bounds) + [0] * (2 - len(bounds)))), 0)
        ln = capi.FastqLengths((C.c_void_p * 2)(*[as_ptr(v) for v in pad(ns)]), (C.c_void_p * 2)(*[as_ptr(v) for v in pad(valids)]))
        pc = capi.FastqPiece((C.c_void_p * 2)(*[as_ptr(v) for v in pad(starts)]), 1 if more else 0, 0)
        rc = L.sk_trim_fastq_piece_device_async(ctx._h, C.byref(params), C.byref(inp), C.byref(ln), C.byref(pc) if piece else None,
                                                capi.TRIM_MODES[mode], (capi.FastqOutput * 3)(*outs), self.ws.data_ptr(),
                                                self.ws_bytes, None)
        assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
        self.piece = piece

    def finish(self):
        L = capi.lib()
        c, pc = capi.FastqCounts(), capi.FastqPieceCounts()
        if self.piece:
            rc = L.sk_trim_fastq_piece_device_finish(self.ctx._h, self.ws.data_ptr(), None, C.byref(c), C.byref(pc))
        else:
            rc = L.sk_trim_fastq_device_finish(self.ctx._h, self.ws.data_ptr(), None, C.byref(c))
        for t, ix in self.keep:
            assert bool((t[self.cap:] == SENTINEL).all()) and (ix is None or bool((ix[self.rcap:] == -7).all())), "a guard was written"
        return rc, dict(c.as_dict(), piece=pc.as_dict())

    def texts(self, counts):
        return [self.keep[o][0][:counts["bytes"][o]].cpu().numpy().tobytes() for o in range(3)]

    def index(self, counts, o):
        return self.keep[o][1][:counts["records"][o]].cpu().numpy().tolist()

    def published(self, i):
        """the words of sk_trim_fastq_piece_words, read back: (consumed, end, ok)"""
        base = self.ws.data_ptr()
        at = [(p - base) // 8 for p in capi.Context.trim_fastq_piece_words(base, i)]
        hdr = self.ws[:256].cpu().numpy().view(np.uint64)
        return tuple(int(hdr[a]) for a in at)


def check_piece(call, want, s=(0, 0)):
    """a finished piece call against pm.piece's dict `want` on its window(s), which start at s[i] of text[i]"""
    rc, counts = call.finish()
    res = want["res"]
    assert counts["records_in"] == want["records_in"] and counts["tail_lines"] == want["tail_lines"]
    assert counts["dropped_unpaired"] == want["dropped_unpaired"]
    n_in = 2 if call.mode == "pe_split" else 1
    for i in range(n_in):
        assert counts["piece"]["consumed"][i] == s[i] + want["consumed"][i], "consumed of input %d" % i
        assert counts["piece"]["carried_bytes"][i] == want["carried"][i]
        assert call.published(i)[0] == s[i] + want["consumed"][i]
        assert call.published(i)[1] == s[i] + want["consumed"][i] + want["carried"][i]
    assert counts["piece"]["inherited_range"] == 0
    compare(call.ctx, dict(res, records_in=want["records_in"], tail_lines=want["tail_lines"],
                           dropped_unpaired=want["dropped_unpaired"]), rc, counts, call.keep, call.mode)
    assert counts["piece"]["ok"] == call.published(0)[2] == int(rc == capi.SK_OK)
    return rc, counts


@pytest.fixture(scope="module")
def base():
    """the text most tests share (about 200 KB: it crosses the 64 KiB framing chunk three times), and the model's result
    on it, computed once"""
    recs = good_records(77)
    text = b"".join(recs)
    return {"recs": recs, "text": text, "want": fm.expected(PT, [text], "se"), "cache": {}}


# ---- 1 piece == NULL and an empty piece are the chained call -----------------------------------------------------------
def test_null_piece_and_empty_piece_are_the_chained_call(sk_ctx, base):
    b0 = sum(len(r) for r in base["recs"][:400])
    text = base["text"][:b0 + 50]
    n = b0 + 3  # an unterminated last line: the first bytes of a name
    keep, ptr = place(text, 5)
    rc0, counts0, keep0, _ = chained(sk_ctx, PT, [ptr], [len(text)], "se", ns=[n], valids=[1])
    assert rc0 == capi.SK_OK
    for piece in (False, True):
        call = Call(sk_ctx, PT, [ptr], [len(text)], "se", ns=[word(n)], valids=[word(1)], piece=piece)
        rc, counts = call.finish()
        assert rc == rc0 and {k: counts[k] for k in counts0} == counts0
        for o in range(3):
            assert bool((call.keep[o][0] == keep0[o][0]).all()) and bool((call.keep[o][1] == keep0[o][1]).all())
        if piece:
            assert counts["piece"] == {"consumed": [n, 0], "carried_bytes": [0, 0], "ok": 1, "inherited_range": 0}


# ---- 2 the window start ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 9])
@pytest.mark.parametrize("fill", ["fastq", "newline"])
def test_window_start(sk_ctx, base, shift, fill):
    """The text lies s bytes into the buffer; what lies before s and behind n (the head of another FASTQ text, or
    newlines) bears on nothing: the result is the model's on text[s:n], read numbers included."""
    text, want = base["text"], base["want"]
    other = b"".join(good_records(78, 140_000)) if fill == "fastq" else b"\n" * 140_000
    for s in (0, 1, 15, 16, 17, 65535, 65536, 65537, 131081):
        data = other[:s] + text + other[:100]
        n = s + len(text)
        keep, ptr = place(data, shift)
        call = Call(sk_ctx, PT, [ptr], [len(data)], "se", ns=[word(n)], starts=[word(s)])
        rc, counts = call.finish()
        compare(sk_ctx, want, rc, counts, call.keep, "se")
        assert counts["piece"]["consumed"][0] == n and counts["piece"]["ok"] == 1
    # a start word above n: an empty text
    keep, ptr = place(text, shift)
    call = Call(sk_ctx, PT, [ptr], [len(text)], "se", ns=[word(1000)], starts=[word(1001)])
    rc, counts = call.finish()
    assert rc == capi.SK_OK and counts["records_in"] == [0, 0] and counts["records"] == [0, 0, 0]
    assert counts["piece"]["consumed"][0] == 1000 and call.published(0)[:2] == (1000, 1000)
    untouched(call.keep)


# ---- 3 more = 1 --------------------------------------------------------------------------------------------------------
def cut_points(base):
    text, recs = base["text"], base["recs"]
    k = len(recs) // 2
    b0 = sum(len(r) for r in recs[:k])
    ns = {b0, 0, 1, 7}
    at = b0
    for line in recs[k].split(b"\n")[:4]:
        at += len(line) + 1  # one past this line's '\n'
        ns |= {at - 2, at - 1, at, at + 1}
    for c in (65536, 131072):
        ns |= {c - 1, c, c + 1}
    return sorted(ns)


def test_more_takes_whole_records(sk_ctx, base):
    text = base["text"]
    keep, ptr = place(text, 3)
    for n in cut_points(base):
        want = pm.piece(PT, [text[:n]], "se", True)
        check_piece(Call(sk_ctx, PT, [ptr], [len(text)], "se", ns=[word(n)], more=True), want)
    # a window start as well: the carry of the cut above becomes the front of this window
    n0, n1 = cut_points(base)[6], 150_000
    s = pm.piece(PT, [text[:n0]], "se", True)["consumed"][0]
    want = pm.piece(PT, [text[s:n1]], "se", True)
    check_piece(Call(sk_ctx, PT, [ptr], [len(text)], "se", ns=[word(n1)], starts=[word(s)], more=True), want, s=(s, 0))


def test_more_degenerate_and_paired(sk_ctx, base):
    recs = base["recs"]
    # no '\n' at all: nothing is taken, nothing is an error
    flat = b"A" * 70_001
    keep, ptr = place(flat, 1)
    rc, counts = check_piece(Call(sk_ctx, PT, [ptr], [len(flat)], "se", starts=[word(5)], more=True),
                             pm.piece(PT, [flat[5:]], "se", True), s=(5, 0))
    assert rc == capi.SK_OK and counts["records_in"] == [0, 0] and counts["piece"]["consumed"][0] == 5
    # interleaved, an odd count: the odd record is carried whole (4 tail lines), more lines behind it too
    odd = b"".join(recs[:301]) + b"@tail\nAC"
    keep, ptr = place(odd, 7)
    rc, counts = check_piece(Call(sk_ctx, PT, [ptr], [len(odd)], "pe_interleaved", more=True),
                             pm.piece(PT, [odd], "pe_interleaved", True))
    assert counts["records_in"][0] == 300 and counts["tail_lines"][0] == 5 and counts["dropped_unpaired"] == 0
    # split, more records in either input: the extra ones are carried, no SK_FQ_PAIR_COUNT
    a, b = b"".join(recs[:350]), b"".join(recs[350:550])
    for t0, t1 in ((a, b), (b, a)):
        k0, p0 = place(t0, 2)
        k1, p1 = place(t1, 11)
        rc, counts = check_piece(Call(sk_ctx, PT, [p0, p1], [len(t0), len(t1)], "pe_split", more=True),
                                 pm.piece(PT, [t0, t1], "pe_split", True))
        assert rc == capi.SK_OK and counts["records_in"] == [200, 200] and max(counts["tail_lines"]) == 600


# ---- 4 errors in the carry ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec,rc_want", [(BAD, capi.SK_EFORMAT), (LOW, capi.SK_ERANGE)])
def test_errors_in_the_carry_wait_for_their_piece(sk_ctx, base, rec, rc_want):
    recs = base["recs"]
    # interleaved: 20 good records and the bad one, whole, as the carried odd record; then the same with its last byte cut
    for text, mode in ((b"".join(recs[:20]) + rec + recs[20], "pe_interleaved"), (b"".join(recs[:20]) + rec[:-1], "se")):
        n1 = len(b"".join(recs[:20]) + rec) if mode == "pe_interleaved" else len(text)
        keep, ptr = place(text, 4)
        first = Call(sk_ctx, PT, [ptr], [len(text)], mode, ns=[word(n1)], more=True)
        rc, counts = check_piece(first, pm.piece(PT, [text[:n1]], mode, True))
        assert rc == capi.SK_OK and counts["records_in"][0] == 20 and counts["piece"]["ok"] == 1
        # the next piece starts at the word the first one published
        consumed_dev = capi.Context.trim_fastq_piece_words(first.ws.data_ptr(), 0)[0]
        full = text if mode == "pe_interleaved" else text + b"\n"
        keep2, ptr2 = place(full, 4)
        second = Call(sk_ctx, PT, [ptr2], [len(full)], mode, starts=[consumed_dev], more=False)
        s = counts["piece"]["consumed"][0]
        rc2, counts2 = check_piece(second, pm.piece(PT, [full[s:]], mode, False), s=(s, 0))
        assert rc2 == rc_want


# ---- 5 the carry kernel alone ------------------------------------------------------------------------------------------
def fake_header(consumed, end, ok, input=0):
    """a previous piece's header with the three words a carry reads"""
    torch = torch_mod()
    h = np.zeros(32, np.int64)
    base = 0x1000
    at = [(p - base) // 8 for p in capi.Context.trim_fastq_piece_words(base, input)]
    h[at[0]], h[at[1]], h[at[2]] = consumed, end, ok
    return torch.from_numpy(h).cuda()


def carry_words(values=None):
    torch = torch_mod()
    return torch.tensor(values or [-1, -1, -1, -1], dtype=torch.int64, device="cuda")


def test_carry_copies_exactly_the_carry(sk_ctx):
    torch = torch_mod()
    rng = np.random.default_rng(5)
    room, chunk = 4112, 321
    src_host = rng.integers(1, 255, 16384, dtype=np.uint8)
    src = torch.from_numpy(src_host).cuda()
    src = src[(-src.data_ptr()) % 16:]  # 16-byte aligned
    src_host = src.cpu().numpy()
    dst_all = torch.empty(room + 64 + 32, dtype=torch.uint8, device="cuda")
    dst_all = dst_all[(-dst_all.data_ptr()) % 16:]
    for c in (0, 1, 15, 16, 17, 255, 4097):
        for so in range(16):
            for target in (0, 1, 8, 15):  # (address of next_text + room - c) mod 16
                d = (target - (room - c)) % 16
                consumed = 32 + so
                end = consumed + c
                hdr, words = fake_header(consumed, end, 1), carry_words()
                dst_all.fill_(SENTINEL)
                nxt = dst_all[d:]
                sk_ctx.fastq_carry_device_async(hdr.data_ptr(), 0, src.data_ptr(), 8192, nxt.data_ptr(), room, words.data_ptr(),
                                                chunk_bytes=chunk)
                got = dst_all.cpu().numpy()
                want = np.full(len(got), SENTINEL, np.uint8)
                want[d + room - c:d + room] = src_host[consumed:end]
                assert np.array_equal(got, want), (c, so, target)
                assert words.cpu().tolist() == list(pm.carry(c, 1, room, chunk)), (c, so, target)


def test_carry_status(sk_ctx):
    torch = torch_mod()
    room = 64
    src = to_device(bytes(range(1, 201)))
    dst = torch.full((room + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    run = lambda hdr, words, **kw: sk_ctx.fastq_carry_device_async(None if hdr is None else hdr.data_ptr(), 0, src.data_ptr(), 200,
                                                                   dst.data_ptr(), room, words.data_ptr(), chunk_bytes=10, **kw)
    cases = [
        (fake_header(10, 10 + room + 1, 1), {}, pm.carry(room + 1, 1, room, 10)),                       # c = room + 1
        (fake_header(10, 20, 1), {"chunk_valid_dev_ptr": 0}, pm.carry(10, 1, room, 10, chunk_valid=0)),  # valid = 0
        (fake_header(10, 20, 0), {}, pm.carry(10, 0, room, 10)),                                        # ok = 0
        (fake_header(10, 20, 1), {"prev_words_ptr": [0, 0, 0, 3]}, pm.carry(10, 1, room, 10, prev_status=3)),
        (fake_header(10, 20, 1), {"other_prev_words_ptr": [0, 0, 0, 2]}, pm.carry(10, 1, room, 10, other_status=2)),
    ]
    assert [w[3] for _, _, w in cases] == [2, 3, 1, 3, 2]
    zero = word(0)
    for hdr, kw, want in cases:
        held = {k: (zero if v == 0 else carry_words(v)) for k, v in kw.items()}
        words = carry_words()
        run(hdr, words, **{k: v.data_ptr() for k, v in held.items()})
        assert tuple(words.cpu().tolist()) == want and want[:3] == (room, room, 0)
        assert bool((dst == SENTINEL).all()), "a failed carry copied something"
    # the first piece: no previous workspace, nothing carried; a chunk length from a device word
    words, seven, one = carry_words(), word(7), word(1)
    sk_ctx.fastq_carry_device_async(None, 0, None, 0, dst.data_ptr(), room, words.data_ptr(), chunk_bytes=10,
                                    chunk_bytes_dev_ptr=seven.data_ptr(), chunk_valid_dev_ptr=one.data_ptr())
    assert words.cpu().tolist() == [room, room + 7, 1, 0] and bool((dst == SENTINEL).all())
    # overlapping buffers are refused and nothing runs
    big = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    words = carry_words()
    for nxt_off, prev_off in ((0, 0), (0, 63), (100, 0)):
        with pytest.raises(capi.SickleError):
            sk_ctx.fastq_carry_device_async(fake_header(0, 10, 1).data_ptr(), 0, big.data_ptr() + prev_off, 200,
                                            big.data_ptr() + nxt_off, room, words.data_ptr(), chunk_bytes=10)
    assert words.cpu().tolist() == [-1] * 4 and bool((big == SENTINEL).all())


# ---- 6 many pieces, one wait -------------------------------------------------------------------------------------------
def enqueue_pieces(ctx, ptuple, texts, mode, size, room, carries=True, writer=False):
    """Every chunk uploaded, then every carry and piece (each with its own workspace, and for output 0 a BGZF writer when
    asked) enqueued on the stream; nothing waits.  -> the Calls, the carry words and the writers."""
    torch = torch_mod()
    n_in = len(texts)
    n_pieces = max(1, max(-(-len(t) // size) for t in texts))
    bufs = []
    for k in range(n_pieces):
        row = []
        for t in texts:
            chunk = t[k * size:(k + 1) * size]
            b = torch.zeros(room + size + 16 + 15, dtype=torch.uint8, device="cuda")
            off = (k * 5 + 3) % 16  # pieces at several alignments (room is a multiple of 16)
            if chunk:
                b[off + room:off + room + len(chunk)] = to_device(chunk)
            row.append((b, b.data_ptr() + off, len(chunk)))
        bufs.append(row)
    words = torch.full((n_pieces, n_in, 4), -1, dtype=torch.int64, device="cuda")
    wptr = lambda k, i: words.data_ptr() + 32 * (k * n_in + i)
    calls, writers = [], []
    for k in range(n_pieces):
        for i in range(n_in):
            prev = calls[-1] if k else None
            ctx.fastq_carry_device_async(prev.ws.data_ptr() if k else None, i, bufs[k - 1][i][1] if k else None,
                                         room + bufs[k - 1][i][2] if k else 0, bufs[k][i][1], room, wptr(k, i),
                                         chunk_bytes=bufs[k][i][2], prev_words_ptr=wptr(k - 1, i) if k else None,
                                         other_prev_words_ptr=wptr(k - 1, 1 - i) if k and n_in == 2 else None)
        call = Call(ctx, ptuple, [bufs[k][i][1] for i in range(n_in)], [room + bufs[k][i][2] for i in range(n_in)], mode,
                    ns=[wptr(k, i) + 8 for i in range(n_in)], valids=[wptr(k, i) + 16 for i in range(n_in)],
                    starts=[wptr(k, i) for i in range(n_in)], more=k + 1 < n_pieces)
        calls.append(call)
        if writer:
            L = capi.lib()
            cap = L.sk_bgzf_bound(call.cap, capi.SK_BGZF_EOF)
            zws_bytes = L.sk_bgzf_workspace_bytes(call.cap)
            img = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
            zws = torch.empty(zws_bytes, dtype=torch.uint8, device="cuda")
            b, w = capi.Context.trim_fastq_output_words(call.ws.data_ptr(), 0)
            ctx.bgzf_device_async(call.keep[0][0].data_ptr(), call.cap, img.data_ptr(), cap, zws.data_ptr(), zws_bytes,
                                  eof=k + 1 == n_pieces, bytes_dev_ptr=b, valid_dev_ptr=w)
            writers.append((img, zws))
    return calls, words, writers, bufs


def many(ctx, ptuple, texts, mode, size, room, writer=False):
    """enqueue_pieces, then every finish; the concatenation against the model on the whole text"""
    want = fm.expected(ptuple, texts, mode)
    assert want["verdict"] is None and want["range"] is None
    calls, words, writers, bufs = enqueue_pieces(ctx, ptuple, texts, mode, size, room, writer=writer)
    got, index, records_in, reads, idle = [b""] * 3, [[], [], []], [0, 0], 0, 0
    for k, call in enumerate(calls):
        rc, counts = call.finish()
        assert rc == capi.SK_OK, (k, capi.lib().sk_last_error(ctx._h))
        assert counts["piece"]["ok"] == 1 and counts["piece"]["inherited_range"] == 0
        texts_k = call.texts(counts)
        for o in fm.USED[mode]:
            got[o] += texts_k[o]
            index[o] += [r + reads for r in call.index(counts, o)]
            assert bool((call.keep[o][0][counts["bytes"][o]:] == SENTINEL).all())
        for o in set(range(3)) - set(fm.USED[mode]):
            assert bool((call.keep[o][0] == SENTINEL).all())
        records_in = [a + b for a, b in zip(records_in, counts["records_in"])]
        reads += counts["records_in"][0] * (2 if mode == "pe_split" else 1)
        idle += counts["records_in"][0] == 0
        last = counts
    assert words[:, :, 3].cpu().abs().sum().item() == 0  # every carry's status
    for o in fm.USED[mode]:
        assert got[o] == want["texts"][o], "output %d" % o
        assert index[o] == [int(x) for x in want["index"][o]]
    assert records_in == want["records_in"] and last["tail_lines"] == want["tail_lines"]
    assert last["dropped_unpaired"] == want["dropped_unpaired"]
    if writer:
        image = b""
        for k, (img, zws) in enumerate(writers):
            n = ctx.bgzf_device_finish(zws.data_ptr())["bytes_out"]
            assert bool((img[n:] == SENTINEL).all())
            image += img[:n].cpu().numpy().tobytes()
        assert gzip.decompress(image) == want["texts"][0] and image.count(EOF) == 1 and image.endswith(EOF)
    return len(calls), idle


@pytest.mark.parametrize("size", [997, 4096, 65536, 70001])
@pytest.mark.parametrize("mode", ["se", "pe_interleaved", "pe_split"])
def test_many_pieces_one_wait(sk_ctx, base, mode, size):
    recs = base["recs"]
    if mode == "pe_split":
        half = len(recs) // 2
        texts = [b"".join(recs[:half]), b"".join(recs[half:2 * half])[:-1]]  # the second one's last line is unterminated
    else:
        texts = [base["text"][:-1] if mode == "se" else b"".join(recs[:len(recs) | 1])]  # interleaved: an odd count
    n, _ = many(sk_ctx, PT, texts, mode, size, room=2048 if mode != "pe_split" else 32768, writer=(mode == "se" and size == 65536))
    assert n == -(-max(len(t) for t in texts) // size)


def test_many_pieces_longer_mate_and_trunc_n(sk_ctx):
    """split inputs whose mate 2 has the longer names and reads (its carry grows piece by piece), once with -n"""
    rng = np.random.default_rng(9)
    m1, m2 = [], []
    for k in range(400):
        for out, L, pad in ((m1, 60, 0), (m2, 110, 25)):
            seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), L).tobytes()
            qual = np.clip(55 + rng.integers(-25, 10, L), 33, 126).astype(np.uint8).tobytes()
            out.append(b"@p%d" % k + b"y" * pad + b"\n" + seq + b"\n+\n" + qual + b"\n")
    for pt in (PT, ("sanger", 20, 20, False, True)):
        many(sk_ctx, pt, [b"".join(m1), b"".join(m2)], "pe_split", 4096, room=65536)


def test_many_pieces_long_records(sk_ctx):
    """three records of 10 000 bases at a piece size of 4 096: pieces that take nothing, a carry that grows"""
    rng = np.random.default_rng(10)
    recs = []
    for k in range(3):
        qual = np.clip(60 + rng.integers(-30, 10, 10_000), 33, 126).astype(np.uint8).tobytes()
        recs.append(b"@long%d\n" % k + rng.choice(np.frombuffer(b"ACGT", np.uint8), 10_000).tobytes() + b"\n+\n" + qual + b"\n")
    n, idle = many(sk_ctx, PT, [b"".join(recs)], "se", 4096, room=32768)
    assert n == 15 and idle >= 10


# ---- 7 failure across pieces in flight ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rec,rc_want", [(BAD, capi.SK_EFORMAT), (LOW, capi.SK_ERANGE)])
def test_failure_across_pieces_in_flight(sk_ctx, base, rec, rc_want):
    recs = list(base["recs"][:100])
    size = -(-len(b"".join(recs)) // 5)
    at = 0
    for k, r in enumerate(recs):  # the first record that lies wholly inside chunk 2
        if at >= 2 * size + 400:
            break
        at += len(r)
    recs[k] = rec
    text = b"".join(recs)
    calls, words, _, bufs = enqueue_pieces(sk_ctx, PT, [text], "se", size, room=1024)
    assert len(calls) == 5
    model = [pm.piece(PT, [text[:size]], "se", True)]
    c0 = model[0]["consumed"][0]
    model.append(pm.piece(PT, [text[c0:2 * size]], "se", True))
    c1 = c0 + model[1]["consumed"][0]
    model.append(pm.piece(PT, [text[c1:3 * size]], "se", True))
    assert model[2]["res"]["verdict" if rc_want == capi.SK_EFORMAT else "range"] is not None
    # a further piece behind them, on a text of its own, WITHOUT a carry
    keep, ptr = place(base["text"][:5000], 0)
    lone = Call(sk_ctx, PT, [ptr], [5000], "se", more=True)
    for k in (0, 1):  # what came before the failure is intact, and its finish does not see the later error
        rc, counts = check_piece(calls[k], model[k], s=(1024 - (0 if k == 0 else model[k - 1]["carried"][0]), 0))
        assert rc == capi.SK_OK
    rc, counts = check_piece(calls[2], model[2], s=(1024 - model[1]["carried"][0], 0))
    assert rc == rc_want and counts["piece"]["inherited_range"] == 0 and counts["piece"]["ok"] == 0
    failed = counts
    assert words[:, 0, 3].cpu().tolist() == [0, 0, 0, 1, 1]
    for k in (3, 4):  # behind the failure: an empty text, nothing taken, nothing written
        rc, counts = calls[k].finish()
        assert counts["records_in"] == [0, 0] and counts["records"] == [0, 0, 0]
        untouched(calls[k].keep)
        assert rc != capi.SK_ESPACE
        if rc_want == capi.SK_EFORMAT:
            assert rc == capi.SK_OK and counts["piece"]["inherited_range"] == 0
        else:  # the word was still set when they began: the earlier error, marked as inherited
            assert rc == capi.SK_ERANGE and counts["piece"]["inherited_range"] == 1 and counts["range"] == failed["range"]
    rc, counts = lone.finish()
    if rc_want == capi.SK_EFORMAT:
        check = pm.piece(PT, [base["text"][:5000]], "se", True)
        assert rc == capi.SK_OK and counts["records_in"] == check["records_in"] and counts["piece"]["inherited_range"] == 0
    else:
        assert rc == capi.SK_ERANGE and counts["piece"]["inherited_range"] == 1 and counts["range"] == failed["range"]
        assert counts["records_in"] == [0, 0] and counts["piece"]["ok"] == 0
        untouched(lone.keep)
    # the finishes cleared the stream's word: the next call is clean
    again = Call(sk_ctx, PT, [ptr], [5000], "se", more=True)
    rc, counts = again.finish()
    assert rc == capi.SK_OK and counts["piece"]["inherited_range"] == 0 and counts["piece"]["ok"] == 1


# ---- 8 the drivers -----------------------------------------------------------------------------------------------------
def run_stream(stream):
    parts = list(stream)
    return [None if parts[0][o] is None else b"".join(p[o] for p in parts) for o in range(3)], stream


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_piece")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


@pytest.mark.parametrize("name,rec", [pytest.param(n, r, id=n) for n, r in tm.golden_runs()])
def test_stream_drivers_on_golden_runs(sk_ctx, workdir, name, rec):
    """trim_fastq_stream against trim_fastq, trim_gz_stream (BGZF in, BGZF out) against the same texts"""
    mode, texts, _ = golden_texts(rec["argv"], workdir)
    params = capi.make_params(*tm.run_params(rec["argv"]))
    dev = [to_device(t) for t in texts]
    want, counts = sk_ctx.trim_fastq(params, dev[0], dev[1] if len(dev) > 1 else None, mode=mode)
    want = [None if w is None else w.cpu().numpy().tobytes() for w in want]
    longest = max(len(line) for t in texts for line in t.split(b"\n"))
    room = 4 * longest + 65536
    got, st = run_stream(sk_ctx.trim_fastq_stream(params, texts[0], texts[1] if len(texts) > 1 else None, mode=mode,
                                                  piece_bytes=100_000, room=room))
    assert got == want
    for key in ("records_in", "records", "bytes", "tail_lines", "dropped_unpaired"):
        assert st.counts[key] == counts[key], key
    assert st.pieces >= max(len(t) for t in texts) // 100_000
    images = [sk_ctx.bgzf(d).cpu().numpy().tobytes() for d in dev]
    got, st = run_stream(sk_ctx.trim_gz_stream(params, images[0], images[1] if len(images) > 1 else None, mode=mode,
                                               piece_bytes=131072, room=room))
    for o in fm.USED[mode]:
        assert gzip.decompress(got[o]) == want[o], "output %d" % o
        assert got[o].endswith(EOF) and got[o].count(EOF) == 1


@pytest.mark.parametrize("group", range(4))
def test_stream_on_drawn_texts(sk_ctx, group):
    """100 texts of tests/soak_fastq.py's generator (25 per case), each at a drawn piece size from 64 to 100 000 (raised to a
    fortieth of the text, so that a case stays at 40 pieces): trim_fastq's outputs and counts, or its error.  An error
    the whole call orders differently (it lets a format error beat any range error; the stream raises what its first
    failing piece meets) is held to the piece model."""
    rng = np.random.default_rng(1000 + group)
    for it in range(25):
        c = soak_fastq.draw(rng)
        texts, mode, pt = c["texts"], c["mode"], tuple(c["params"])
        size = max(int(np.exp(rng.uniform(np.log(64), np.log(100_000)))), max(len(t) for t in texts) // 40, 1)
        longest = max(len(r) for t in texts for r in t.split(b"\n")) if texts else 0
        room = 8 * longest + 4096 + 2 * size  # (split inputs drawn on their own: the steered carry stays below two pieces)
        params = capi.make_params(*pt)
        want = fm.expected(pt, texts, mode)
        stream = sk_ctx.trim_fastq_stream(params, [t[a:a + 7919] for t in texts[:1] for a in range(0, len(t), 7919)],
                                          texts[1] if len(texts) > 1 else None, mode=mode, piece_bytes=size, room=room)
        tag = (group, it, mode, size)
        if want["verdict"] is None and want["range"] is None:
            got, st = run_stream(stream)
            for o in fm.USED[mode]:
                assert got[o] == want["texts"][o], tag
            assert st.counts["records_in"] == want["records_in"] and st.counts["tail_lines"] == want["tail_lines"], tag
            assert st.counts["dropped_unpaired"] == want["dropped_unpaired"], tag
            continue
        with pytest.raises((capi.FormatError, capi.RangeError)) as e:
            run_stream(stream)
        if want["verdict"] is None:
            assert isinstance(e.value, capi.RangeError) and (e.value.read, e.value.pos, e.value.ch) == tuple(want["range"]), tag
        elif isinstance(e.value, capi.FormatError):
            assert (e.value.reason, e.value.input, e.value.record) == want["verdict"], tag
        else:  # a range error in a piece before the malformed record's: it lies in a read below that record
            why, i, k = want["verdict"]
            assert e.value.read < (2 * k + i if mode == "pe_split" else k), tag


def test_stream_gz_and_allocation(sk_ctx, base):
    params = capi.make_params(*PT)
    text = base["text"]
    want = base["want"]["texts"][0]
    got, st = run_stream(sk_ctx.trim_fastq_stream(params, text, piece_bytes=50_000, room=4096, gz=True))
    assert gzip.decompress(got[0]) == want and got[0].count(EOF) == 1 and got[0].endswith(EOF) and st.pieces == 5
    # the device memory is a function of piece_bytes and room alone
    one = sk_ctx.trim_fastq_stream(params, text, piece_bytes=50_000, room=4096)
    eight = sk_ctx.trim_fastq_stream(params, [text] * 8, piece_bytes=50_000, room=4096)
    assert one.device_bytes == eight.device_bytes > 0
    got8, st8 = run_stream(eight)
    assert got8[0] == want * 8 and st8.counts["records_in"][0] == 8 * base["want"]["records_in"][0]
    assert eight.device_bytes == one.device_bytes
    # plain gzip cannot be cut
    with pytest.raises(ValueError, match="trim_gz"):
        sk_ctx.trim_gz_stream(params, gzip.compress(text[:5000]))


def test_stream_room_too_small(sk_ctx):
    long = b"@long\n" + b"ACGT" * 2500 + b"\n+\n" + b"I" * 10_000 + b"\n"
    text = b"@a\nACGT\n+\nIIII\n" * 50 + long + b"@a\nACGT\n+\nIIII\n" * 50
    params = capi.make_params(*PT)
    with pytest.raises(capi.TrimError, match="room") as e:
        run_stream(sk_ctx.trim_fastq_stream(params, text, piece_bytes=1024, room=4096))
    assert e.value.rc == capi.SK_ESPACE
    got, _ = run_stream(sk_ctx.trim_fastq_stream(params, text, piece_bytes=1024, room=32768))
    assert got[0] == fm.expected(PT, [text], "se")["texts"][0]


def test_stream_steers_split_inputs(sk_ctx):
    """mate 2's records are twice mate 1's: with equal chunks mate 1's carry would grow by half a piece per piece and
    pass room = piece_bytes; the driver sizes each input's chunk by what it carried"""
    rng = np.random.default_rng(12)
    m1, m2 = [], []
    for k in range(1500):
        for out, L in ((m1, 50), (m2, 104)):
            seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), L).tobytes()
            qual = np.clip(60 + rng.integers(-30, 10, L), 33, 126).astype(np.uint8).tobytes()
            out.append(b"@q%d\n" % k + seq + b"\n+\n" + qual + b"\n")
    texts = [b"".join(m1), b"".join(m2)]
    want = fm.expected(PT, texts, "pe_split")
    got, st = run_stream(sk_ctx.trim_fastq_stream(capi.make_params(*PT), texts[0], texts[1], mode="pe_split", piece_bytes=8192))
    assert st.pieces >= 30 and st.room == 8192
    for o in range(3):
        assert got[o] == want["texts"][o]
