"""CPU: tests/gunzip_piece_model.py, the rules of the piece call in Python, against gunzip_model.gunzip: streamed at
windows of 600, 1 024, 4 096 and 70 000 bytes it reproduces the text of every valid image and the verdict on every damaged
one, and every state's member_crc is zlib's crc32 of the open member's text.  The same for the legal streams zlib never writes (tests/foreign_images.py), the
one-symbol blocks also at the smallest window in which every block fits."""
import zlib

import pytest

import foreign_images as fi
import gunzip_model as gm
import gunzip_piece_model as pm

WINDOWS = (600, 1024, 4096, 70000)


def valid():
    out = {name: v[:2] for name, v in gm.images().items()}
    out.update({name: v[:2] for name, v in gm.stretch_images().items()})
    return out


def member_starts(image):
    """text offset of every member's first byte"""
    starts, at, rest = [], 0, image
    while rest:
        d = zlib.decompressobj(31)
        at += len(d.decompress(rest))
        starts.append(at)
        rest = d.unused_data
    return [0] + starts


@pytest.mark.parametrize("window", WINDOWS)
def test_valid_images(window):
    for name, (image, text) in valid().items():
        pieces, whole = pm.stream(image, window, grow=70000)
        assert whole == text == gm.gunzip(image)["text"], (name, window)
        last = pieces[-1][0]
        assert last["done"] == 1 and last["in_member"] == 0 and last["text_bytes"] == len(text), (name, window)
        assert last["members"] == gm.gunzip(image)["members"] and last["pos_bit"] == 8 * len(image), (name, window)
        starts, at = member_starts(image), 0
        for st, t, info in pieces:
            at += len(t)
            assert st["text_bytes"] == at and st["history"] == (bytes(32768) + text[:at])[-32768:], (name, window)
            if st["in_member"]:
                first = starts[st["members"]]
                assert st["member_text"] == at - first and st["member_crc"] == zlib.crc32(text[first:at]), (name, window)
            else:
                assert st["member_text"] == 0 and st["member_crc"] == 0, (name, window)


@pytest.mark.parametrize("window", WINDOWS)
def test_damaged_images(window):
    for name, (image, chunk) in gm.bad_images().items():
        pieces, whole = pm.stream(image, window)
        want = gm.gunzip(image)
        got = pm.verdict(pieces)
        assert whole is None and pieces[-1][0]["status"] == 1, (name, window)
        assert {k: got[k] for k in ("error", "error_member", "error_offset")} == \
            {k: want[k] for k in ("error", "error_member", "error_offset")}, (name, window, got, want)
        assert want["error_member"] <= got["members"] <= want["members"], (name, window)
        # a void piece hands the failure on
        st, t, info = pm.piece(image, pieces[-1][0], window, 1)
        assert st == pieces[-1][0] and t == b"" and info["inherited"] == 1


FOREIGN_WINDOWS = (600, 4096, 70000)


def smallest_window(image):
    """The smallest window at which no piece of the image stalls: the widest block, a header in front of it or a trailer
    behind it included (searched from a little below the widest block, and the window one byte smaller stalls)"""
    w = max(fi.block_spans(image)) - 2
    while any(info["window_limited"] for _, _, info in pm.stream(image, w)[0]):
        w += 1
    assert any(info["window_limited"] for _, _, info in pm.stream(image, w - 1)[0])
    return w


def foreign_cases():
    """(name, image, text, window): every image at the three windows, the one-symbol blocks at their smallest too"""
    images = fi.valid("gzip")
    out = [(name, image, text, w) for w in FOREIGN_WINDOWS for name, (image, text) in images.items()]
    return out + [(name, images[name][0], images[name][1], smallest_window(images[name][0])) for name in fi.TINY]


def test_foreign_images():
    """Blocks wider than the window stall and are repeated at 70 000 (no block here is wider than that)"""
    for name, image, text, window in foreign_cases():
        pieces, whole = fi.piece_stream("valid", name, window)
        want = fi.expected("gzip")[name]
        assert whole == text == want["text"], (name, window)
        last = pieces[-1][0]
        assert last["done"] == 1 and last["in_member"] == 0 and last["text_bytes"] == len(text), (name, window)
        assert last["members"] == want["members"] and last["pos_bit"] == 8 * len(image), (name, window)
        at = 0
        for st, t, info in pieces:
            at += len(t)
            assert st["text_bytes"] == at and st["history"] == (bytes(32768) + text[:at])[-32768:], (name, window)
    assert [c[3] for c in foreign_cases()[-3:]] < [100, 100, 400]


def test_foreign_bad_images():
    for name, (image, chunk) in fi.bad_images("gzip").items():
        want = fi.bad_expected("gzip")[name]
        for window in FOREIGN_WINDOWS:
            pieces, whole = fi.piece_stream("bad", name, window)
            got = pm.verdict(pieces)
            assert whole is None and pieces[-1][0]["status"] == 1, (name, window)
            assert {k: got[k] for k in ("error", "error_member", "error_offset")} == \
                {k: want[k] for k in ("error", "error_member", "error_offset")}, (name, window, got, want)


def test_resume_points_hold_every_state():
    image, text, _ = gm.stretch_images()["two_members_c1024"]
    points = pm.resume_points(image)
    blocks = gm.walk(image)[1]
    assert {(b[0], 1) for b in blocks} <= points and (0, 0) in points and (8 * len(image), 0) in points
    assert sum(1 for p in points if p[1] == 0) == 3
    for st, t, info in pm.stream(image, 1024)[0]:
        assert (st["pos_bit"], st["in_member"]) in points
