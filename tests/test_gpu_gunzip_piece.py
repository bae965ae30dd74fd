"""GPU: plain gzip read on the device in pieces (sk_gzip_inflate_piece_device_async / finish, Context.gunzip_stream)
against tests/gunzip_piece_model.py: every piece's state and text over images of many small blocks at windows of 600 bytes
to 1 MiB, every kind of member at windows that hold a piece and that stall, a window end swept over a member boundary,
the capacity cut, every damaged image, a sliding image buffer, and the driver.  The pieces of a stream are all enqueued
before the first is finished: each has its own workspace, text buffer and state.  And the legal streams zlib never writes
(tests/foreign_images.py): one-symbol blocks, runs of empty blocks and set padding bits in pieces, where nearly every
state carries a bit offset inside a byte."""
import ctypes as C
import functools
import gzip

import pytest

import foreign_images as fi
import gunzip_model as gm
import gunzip_piece_model as pm
from bgzf_raw import SENTINEL, to_device, torch_mod, upload
from sickle_amd import capi

pytestmark = pytest.mark.gpu
GUARD = 64
STATE = capi.SK_GZIP_PIECE_STATE_BYTES
FIELDS = pm.FIELDS + ("done", "status")


@functools.lru_cache(maxsize=None)
def model(kind, name, window, grow=0):
    image = getattr(gm, kind)()[name][0]
    return pm.stream(image, window, grow)


def set_chunk(monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("SK_GZIP_CHUNK", str(chunk))
    else:
        monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)


class Pieces:
    """Pieces on raw pointers, enqueued by add() and read by finish(): piece i goes from states[i] to states[i + 1] unless
    told otherwise, into a text buffer of capacity + GUARD bytes of SENTINEL whose guard finish() checks."""

    def __init__(self, ctx, image, slots, shift=0, start=None, surround=None):
        torch = torch_mod()
        self.ctx, self.L, self.image = ctx, capi.lib(), image
        self.keep, self.ptr = upload(image, shift, surround=surround)
        self.states = torch.zeros((slots + 1, STATE), dtype=torch.uint8, device="cuda")
        if start is not None:
            self.states[0] = to_device(start)
        self.calls = []

    def add(self, window, capacity, src, dst, last=1, lo=0, hi=None, ws=None):
        """image[lo:hi] is handed in, with image_offset = lo.  ws: the workspace tensor, used as it is (the byte count
        handed to the library stays the formula's)"""
        torch = torch_mod()
        hi = len(self.image) if hi is None else hi
        ws_bytes = self.L.sk_gzip_inflate_piece_workspace_bytes(window, capacity)
        if ws is None:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        out = torch.full((capacity + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
        piece = capi.GzipPiece(lo, window, last, 0)
        rc = self.L.sk_gzip_inflate_piece_device_async(self.ctx._h, self.ptr + lo if hi > lo else None, hi - lo, C.byref(piece),
                                                       self.states[src].data_ptr(), self.states[dst].data_ptr(), out.data_ptr(),
                                                       capacity, ws.data_ptr(), ws_bytes, None)
        assert rc == capi.SK_OK, self.L.sk_last_error(self.ctx._h)
        self.calls.append((ws, out, capacity, dst))

    def finish(self):
        """-> per piece dict(rc, counts, state (dict of the words), raw (the state's bytes), text)"""
        got = []
        for ws, out, capacity, dst in self.calls:
            c, pc = capi.GzipInflateCounts(), capi.GzipPieceCounts()
            rc = self.L.sk_gzip_inflate_piece_device_finish(self.ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(pc))
            counts = dict(c.as_dict(), **pc.as_dict())
            assert bool((out[capacity:] == SENTINEL).all()), "bytes of out at or beyond the capacity were written"
            written = rc == capi.SK_OK
            raw = self.states[dst].cpu().numpy().tobytes()
            state = capi.GzipPieceState.from_buffer_copy(raw).as_dict()
            assert (counts["pos_bit"], counts["in_member"], counts["done"]) == (state["pos_bit"], state["in_member"], state["done"])
            got.append(dict(rc=rc, counts=counts, state=state, raw=raw,
                            text=out[:counts["bytes_out"]].cpu().numpy().tobytes() if written else b""))
            if rc == capi.SK_ESPACE or counts["inherited"] or state["status"] == 3:  # after SK_EDATA of its own, out is undefined
                assert bool((out == SENTINEL).all()), "a piece that is void or whose text did not fit wrote text"
        self.calls = []
        return got

    def raw_state(self, i):
        return self.states[i].cpu().numpy().tobytes()


def check_against_model(got, want, text, tag):
    assert len(got) >= len(want)
    for i, (g, (w, t, info)) in enumerate(zip(got, want)):
        assert {k: g["state"][k] for k in FIELDS} == {k: w[k] for k in FIELDS}, (tag, i, g["counts"])
        assert g["raw"][128:] == w["history"], (tag, i)
        assert g["rc"] == capi.SK_OK and g["text"] == t and g["counts"]["bytes_out"] == len(t), (tag, i, g["counts"])
        assert (g["counts"]["window_limited"], g["counts"]["inherited"]) == (0, 0), (tag, i)
    assert b"".join(g["text"] for g in got) == text and got[len(want) - 1]["state"]["done"] == 1, tag
    for g in got[len(want):]:  # behind the end: empty successful pieces
        assert g["rc"] == capi.SK_OK and g["counts"]["bytes_out"] == 0 and g["state"]["done"] == 1, tag


# ---- 1 many small blocks: windows from 600 bytes to one piece -------------------------------------------------------
@pytest.mark.parametrize("window", [600, 1024, 4096, 1 << 20])
@pytest.mark.parametrize("name", list(gm.stretch_images()))
def test_stretch_images(sk_ctx, monkeypatch, name, window):
    """far_c256 and run_c256 at 600 are the history cases: matches reach the far end of a window that some 36 pieces of
    under 1 KB each assembled"""
    image, text, chunk = gm.stretch_images()[name]
    set_chunk(monkeypatch, chunk)
    want, whole = model("stretch_images", name, window)
    assert whole == text and (window < (1 << 20) or len(want) == 1)
    p = Pieces(sk_ctx, image, len(want) + 1, shift=len(name) % 16)
    for i in range(len(want) + 1):
        p.add(window, max(len(t) for _, t, _ in want), i, i + 1)
    check_against_model(p.finish(), want, text, (name, window))


# ---- 2 every kind of member; a window that stalls -------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 256])
@pytest.mark.parametrize("window", [70000, 20000])
def test_every_kind_of_member(sk_ctx, monkeypatch, window, chunk):
    """stored0 is one stored block of 60 005 bytes: at 20 000 the piece is window-limited, state_in is what it was, and
    the repeat at 70 000 goes on"""
    set_chunk(monkeypatch, chunk)
    stalls = []
    for k, (name, (image, text)) in enumerate(gm.images().items()):
        want, whole = model("images", name, window, 70000)
        assert whole == text
        p = Pieces(sk_ctx, image, 2 * len(want) + 2, shift=k % 16)
        spare = len(want) + 1  # states that take what a stalled piece publishes
        for i, (w, t, info) in enumerate(want):
            if info["stalled"]:
                p.add(window, len(text), i, spare + i)
            p.add(info["window"], len(text), i, i + 1)
        got = p.finish()
        real = []
        for i, (w, t, info) in enumerate(want):
            if info["stalled"]:
                g = got.pop(0)
                stalls.append(name)
                assert g["rc"] == capi.SK_EDATA and g["counts"]["window_limited"] == 1 and g["state"]["status"] == 1, (name, g["counts"])
                assert p.raw_state(i) == (real[-1]["raw"] if real else bytes(STATE)), name  # state_in is byte-identical
            real.append(got.pop(0))
        check_against_model(real, want, text, (name, window, chunk))
    assert ("stored0" in stalls) == (window == 20000) and (window == 20000 or not stalls)


# ---- 3 a window end swept over a member boundary --------------------------------------------------------------------
def test_window_end_swept_over_a_member_boundary(sk_ctx, monkeypatch):
    set_chunk(monkeypatch, 256)
    first = gm.small_blocks(gm.fastq_text(3000, 71))
    second, text2 = gm.images()["all_fields"]
    image = first + second
    blocks = gm.walk(image)[1]
    final = max(b[0] for b in blocks if b[3] == 0)  # the first member's final block
    body = gm.parse_header(second, 0)[1]
    lo, hi = len(first) - 8 - 3, len(first) + body + 3
    assert final < 8 * lo
    p = Pieces(sk_ctx, image, 2 * (hi - lo + 1))
    ends = list(range(lo, hi + 1))
    for j, w in enumerate(ends):
        p.add(w, 8192, 2 * j, 2 * j + 1)
    seen = set()
    for w, g in zip(ends, p.finish()):
        want, t, info = pm.piece(image, pm.zero_state(), w, 1)
        assert g["rc"] == capi.SK_OK and {k: g["state"][k] for k in FIELDS} == {k: want[k] for k in FIELDS}, (w, g["counts"])
        assert g["text"] == t and g["raw"][128:] == want["history"], w
        seen.add((want["pos_bit"], want["in_member"]))
    assert seen == {(final, 1), (8 * len(first), 0), (8 * (len(first) + body), 1)}  # before the final block, the member start, behind the header


# ---- 4 the capacity -------------------------------------------------------------------------------------------------
def test_capacity_cut(sk_ctx, monkeypatch):
    """No stretch of fq200k_c256 holds more than 4 096 bytes of text (tests/test_gunzip_piece_host.py::test_capacity_cut
    asserts it on the host run of the same stages)"""
    image, text, chunk = gm.stretch_images()["fq200k_c256"]
    set_chunk(monkeypatch, chunk)
    points = pm.resume_points(image)
    state, texts, pos, rounds = None, [], -1, 0
    while True:
        p = Pieces(sk_ctx, image, 32, start=state)
        for i in range(32):
            p.add(8192, 4096, i, i + 1)
        got = p.finish()
        for g in got:
            assert g["rc"] == capi.SK_OK and g["counts"]["bytes_out"] <= 4096, g["counts"]
            if g["counts"]["bytes_out"] or not g["state"]["done"]:
                assert g["state"]["pos_bit"] > pos and (g["state"]["pos_bit"], g["state"]["in_member"]) in points, g["counts"]
                pos = g["state"]["pos_bit"]
            texts.append(g["text"])
        state, rounds = got[-1]["raw"], rounds + 1
        if got[-1]["state"]["done"]:
            break
        assert rounds < 40
    assert b"".join(texts) == text
    assert sum(1 for t in texts if t) > len(image) // 8192 + 1  # the capacity cut them, not the window
    p = Pieces(sk_ctx, image, 3)
    p.add(8192, 64, 0, 1)
    short = p.finish()[0]
    need = short["counts"]["bytes_out"]
    assert short["rc"] == capi.SK_ESPACE and short["state"]["status"] == 2 and 64 < need <= 4096, short["counts"]
    assert p.raw_state(0) == bytes(STATE)
    p.add(8192, need, 0, 2)
    again = p.finish()[0]
    assert again["rc"] == capi.SK_OK and again["counts"]["bytes_out"] == need and again["text"] == text[:need]


# ---- 5 damaged images -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gm.bad_images()))
def test_damaged_images(sk_ctx, monkeypatch, name):
    """The stream's reason, member and offset are gm.gunzip's.  So is `members` where the whole-image walk stops at the
    failure; behind a distance, length or CRC error it goes on and counts the members behind it, and the pieces behind the
    one that failed are void: the stream's count is then the model's, that of the pieces up to the failing one."""
    image, chunk = gm.bad_images()[name]
    set_chunk(monkeypatch, chunk)
    want, whole = model("bad_images", name, 2048)
    ref = gm.gunzip(image)
    assert whole is None
    p = Pieces(sk_ctx, image, len(want) + 2, shift=len(name) % 16)
    for i in range(len(want) + 2):
        p.add(2048, 65536, i, i + 1)
    got = p.finish()
    for g, (w, t, info) in zip(got[:len(want) - 1], want):
        assert g["rc"] == capi.SK_OK and g["text"] == t and {k: g["state"][k] for k in FIELDS} == {k: w[k] for k in FIELDS}, name
    bad, w = got[len(want) - 1], want[-1][0]
    assert bad["rc"] == capi.SK_EDATA and bad["counts"]["inherited"] == 0 and bad["counts"]["window_limited"] == want[-1][2]["window_limited"]
    verdict = {k: bad["state"][k] for k in ("error", "error_member", "error_offset", "members")}
    assert (bad["counts"]["error"], bad["counts"]["error_member"], bad["counts"]["error_offset"]) == tuple(verdict.values())[:3]
    assert {k: verdict[k] for k in ("error", "error_member", "error_offset")} == {k: ref[k] for k in ("error", "error_member", "error_offset")}, name
    assert verdict["members"] == w["members"] and ref["error_member"] <= verdict["members"] <= ref["members"], name
    stops = ref["error"] in (gm.HEADER, gm.TRUNCATED) or (ref["error"] == gm.DEFLATE and not name.startswith("far@"))
    assert not stops or verdict["members"] == ref["members"], name
    for g in got[len(want):]:  # void
        assert g["rc"] == capi.SK_EDATA and g["counts"]["inherited"] == 1 and g["counts"]["bytes_out"] == 0 and g["text"] == b""
        assert {k: g["state"][k] for k in verdict} == verdict and g["raw"] == bad["raw"], name


# ---- 5b what zlib never writes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [600, 4096])
@pytest.mark.parametrize("name", list(fi.TINY) + ["empty_runs", "empty_runs_fixed", "empty_runs_pigz", "pad_bits", "foreign_members"])
def test_foreign_images_in_pieces(sk_ctx, monkeypatch, name, window):
    """Every piece's state and text against the model, all pieces enqueued before the first finish.  foreign_members holds
    blocks wider than the window: such a piece is window-limited, leaves its state_in as it was and is repeated at 70 000."""
    set_chunk(monkeypatch, 256)
    image, text = fi.valid("gzip")[name]
    want, whole = fi.piece_stream("valid", name, window)
    assert whole == text
    p = Pieces(sk_ctx, image, 2 * len(want) + 2, shift=len(name) % 16)
    spare = len(want) + 1  # states that take what a stalled piece publishes
    capacity = max(len(t) for _, t, _ in want)
    for i, (w, t, info) in enumerate(want):
        if info["stalled"]:
            p.add(window, capacity, i, spare + i)
        p.add(info["window"], capacity, i, i + 1)
    got, real = p.finish(), []
    for i, (w, t, info) in enumerate(want):
        if info["stalled"]:
            g = got.pop(0)
            assert g["rc"] == capi.SK_EDATA and g["counts"]["window_limited"] == 1 and g["state"]["status"] == 1, (name, i, g["counts"])
        real.append(got.pop(0))
    check_against_model(real, want, text, (name, window))
    assert name != "foreign_members" or sum(info["stalled"] for _, _, info in want) >= 5


@pytest.mark.parametrize("name", ["tiny_blocks_match", "tiny_blocks_batch"])
def test_foreign_capacity_cut(sk_ctx, monkeypatch, name):
    """The whole image in the window and 4 096 bytes of text a piece: every block boundary is a resume point, and each
    piece ends at one, within the capacity (tests/test_gunzip_piece_host.py::test_foreign_capacity_cut: no stretch of
    these images at chunk 256 holds more)"""
    image, text = fi.valid("gzip")[name]
    set_chunk(monkeypatch, 256)
    points = pm.resume_points(image)
    p = Pieces(sk_ctx, image, 8)
    for i in range(8):
        p.add(len(image), 4096, i, i + 1)
    got, pos = p.finish(), -1
    for g in got:
        assert g["rc"] == capi.SK_OK and g["counts"]["bytes_out"] <= 4096, g["counts"]
        if g["counts"]["bytes_out"] or not g["state"]["done"]:
            assert g["state"]["pos_bit"] > pos and (g["state"]["pos_bit"], g["state"]["in_member"]) in points, g["counts"]
            pos = g["state"]["pos_bit"]
    assert b"".join(g["text"] for g in got) == text and got[-1]["state"]["done"] == 1
    assert sum(1 for g in got if g["text"]) >= -(-len(text) // 4096)


@pytest.mark.parametrize("name", ["one_dist_unassigned@1", "stored_nlen@last"])
def test_foreign_bad_images_in_pieces(sk_ctx, monkeypatch, name):
    """The failing piece's verdict is the whole-image model's, and the pieces behind it are void"""
    image, chunk = fi.bad_images("gzip")[name]
    set_chunk(monkeypatch, chunk)
    want, whole = fi.piece_stream("bad", name, 4096, 0)
    ref = fi.bad_expected("gzip")[name]
    assert whole is None
    p = Pieces(sk_ctx, image, len(want) + 2, shift=len(name) % 16)
    for i in range(len(want) + 2):
        p.add(4096, 65536, i, i + 1)
    got = p.finish()
    for g, (w, t, info) in zip(got[:len(want) - 1], want):
        assert g["rc"] == capi.SK_OK and g["text"] == t and {k: g["state"][k] for k in FIELDS} == {k: w[k] for k in FIELDS}, name
    bad = got[len(want) - 1]
    # a block that fails in a window that does not reach the image's end might be one the window cuts: window_limited
    assert bad["rc"] == capi.SK_EDATA and bad["counts"]["inherited"] == 0, bad["counts"]
    assert bad["counts"]["window_limited"] == want[-1][2]["window_limited"] == int(name.endswith("@1")), bad["counts"]
    verdict = {k: bad["state"][k] for k in ("error", "error_member", "error_offset")}
    assert verdict == {k: ref[k] for k in verdict} and verdict["error"] == gm.DEFLATE, (name, verdict)
    for g in got[len(want):]:  # void
        assert g["rc"] == capi.SK_EDATA and g["counts"]["inherited"] == 1 and g["counts"]["bytes_out"] == 0 and g["text"] == b""
        assert g["raw"] == bad["raw"], name


# ---- 6 a sliding image buffer ---------------------------------------------------------------------------------------
def test_image_offset(sk_ctx, monkeypatch):
    image, text, chunk = gm.stretch_images()["two_members_c1024"]
    set_chunk(monkeypatch, chunk)
    window = 4096
    want, whole = model("stretch_images", "two_members_c1024", window)
    p = Pieces(sk_ctx, image, len(want) + 3)
    at = 0
    for i, (w, t, info) in enumerate(want):  # the buffer begins up to 5 bytes before the position and holds the window and 7 more
        lo, hi = max(0, at - i % 6), min(len(image), at + window + 7)
        p.add(window, len(text), i, i + 1, last=int(hi == len(image)), lo=lo, hi=hi)
        at = w["pos_bit"] >> 3
    check_against_model(p.finish(), want, text, "sliding")
    n = len(want) + 1
    p.add(window, 4096, 0, n, lo=1)  # position 0 lies before the buffer
    p.add(window, 4096, 1, n + 1, last=0, hi=(want[0][0]["pos_bit"] >> 3) - 1)  # and behind it
    for g in p.finish():
        assert g["rc"] == capi.SK_EINVAL and g["state"]["status"] == 3 and g["counts"]["bytes_out"] == 0, g["counts"]


# ---- 7 the driver ---------------------------------------------------------------------------------------------------
def test_gunzip_stream(sk_ctx, monkeypatch):
    set_chunk(monkeypatch, 0)
    fq = gm.fastq_text(3 << 20, 81)
    bgzf = sk_ctx.bgzf(to_device(gm.texts()["fq"] * 3), eof=True).cpu().numpy().tobytes()
    cases = [(gzip.compress(fq, 6), fq, 200000, None), (gm.images()["two"][0], gm.images()["two"][1], 70000, None),
             (bgzf, gm.texts()["fq"] * 3, 50000, None), (b"", b"", 4096, None), (gzip.compress(fq, 1), fq, 1 << 20, 600000)]
    for image, text, window, cap in cases:
        parts = [t.cpu().numpy().tobytes() for t in sk_ctx.gunzip_stream(to_device(image or b"x")[:len(image)], window, cap)]
        assert b"".join(parts) == text and (len(parts) > 1 or len(text) < 100000), (len(image), window)
        assert cap is None or max(len(t) for t in parts) <= cap
    image, text = gm.images()["stored0"]
    with pytest.raises(capi.GzDataError) as e:
        list(sk_ctx.gunzip_stream(to_device(image), 20000))
    assert e.value.counts["window_limited"] == 1 and "window_bytes=20000" in str(e.value)
    with pytest.raises(capi.TrimError) as e:
        list(sk_ctx.gunzip_stream(to_device(gzip.compress(fq, 6)), 1 << 20, 1000))
    assert e.value.rc == capi.SK_ESPACE and "piece_bytes" in str(e.value)
    bad = gm.bad_images()["crc@1"][0]
    with pytest.raises(capi.GzDataError) as e:
        list(sk_ctx.gunzip_stream(to_device(bad), 2048))
    assert (e.value.reason, e.value.member) == (gm.CRC, 1) and e.value.counts["window_limited"] == 0
