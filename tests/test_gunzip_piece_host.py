"""The piece stages of the device's plain-gzip reader without a device: tests/gunzip_piece/piece_host (the stages of
sickle_amd/csrc/sk_gunzip_block.h in the order of sk_gunzip_piece.hip's launches, lane after lane, built with the address
and undefined-behaviour sanitizers) streams images from the zero state and is held against tests/gunzip_piece_model.py:
every piece's state, the texts, the verdict on damaged images, window-limited pieces and their repeat, the capacity cut.
The same once more with the build whose bit reader re-bases every 64 bytes, and the legal streams zlib never writes
(tests/foreign_images.py).  CPU only."""
import os
import struct
import subprocess

import pytest

import cli_util as cu
import foreign_images as fi
import gunzip_model as gm
import gunzip_piece_model as pm

HOST = os.path.join(cu.ROOT, "tests", "gunzip_piece", "piece_host")
COLUMNS = ("status", "error", "error_member", "error_offset", "pos_bit", "in_member", "member_text", "member_crc", "members",
           "text_bytes", "done", "window_limited", "inherited", "bytes_out", "written", "stretches_used", "max_stretch_text")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "gunzip_piece"), "all"], check=True)
    return HOST


def run_host(tool, items, d, tag="batch"):
    """items: list of (image, chunk, window, capacity, grow) -> per image the list of its pieces (dict of COLUMNS + text)"""
    batch, res, txt = (str(d / (tag + e)) for e in (".bin", ".res", ".txt"))
    with open(batch, "wb") as f:
        for image, chunk, window, capacity, grow in items:
            f.write(struct.pack("<IIQQQ", chunk, len(image), window, capacity, grow) + image)
    pr = subprocess.run([tool, batch, res, txt], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    texts, at, out = open(txt, "rb").read(), 0, []
    lines = open(res).read().split("\n")
    i = 0
    while lines[i]:
        count = int(lines[i].split()[1])
        pieces = []
        for line in lines[i + 1:i + 1 + count]:
            p = dict(zip(COLUMNS, (int(x) for x in line.split())))
            p["text"] = texts[at:at + p["bytes_out"]] if p["written"] else b""
            at += len(p["text"])
            pieces.append(p)
        out.append(pieces)
        i += 1 + count
    assert len(out) == len(items) and at == len(texts)
    return out


def check_stream(name, got, image, text, window, grow=0, model=None):
    """got: the harness's pieces; every piece against the model's, in order"""
    want, whole = model if model is not None else pm.stream(image, window, grow)
    got = [g for g in got if not (g["window_limited"] and grow)]  # the repeat is the model's piece
    assert len(got) == len(want), (name, window, len(got), len(want))
    for i, (g, (w, t, info)) in enumerate(zip(got, want)):
        assert g["status"] == w["status"], (name, window, i, g)
        if w["status"]:
            assert tuple(g[k] for k in ("error", "error_member", "error_offset", "members", "window_limited")) == \
                tuple(w[k] for k in ("error", "error_member", "error_offset", "members")) + (info["window_limited"],), (name, window, i, g)
            continue
        assert {k: g[k] for k in pm.FIELDS + ("done",)} == {k: w[k] for k in pm.FIELDS + ("done",)}, (name, window, i)
        assert g["text"] == t and g["written"] == 1, (name, window, i)
    if whole is not None:
        assert b"".join(g["text"] for g in got) == whole == text, (name, window)
    return got


def test_blocks_fit_the_smallest_window():
    """what the windows of the tests below and of tests/test_gpu_gunzip_piece.py rest on"""
    for name, v in list(gm.stretch_images().items()) + list(gm.bad_images().items()):
        lengths = []
        blocks = gm.walk(v[0], lengths)[1]
        bits = [b[0] for b in blocks]
        assert max((b - a for a, b in zip(bits, bits[1:])), default=0) <= 254 * 8 + 18 * 8, name  # + a trailer and a header


@pytest.mark.parametrize("build", ["", "_rebase"])
def test_stretch_images_in_pieces(tool, tmp_path, build):
    s = gm.stretch_images()
    windows = (600, 1024, 4096, 1 << 20) if not build else (1024,)
    items = [(name, v, w) for name, v in s.items() for w in windows]
    got = run_host(tool + build, [(v[0], v[2], w, len(v[1]), 0) for name, v, w in items], tmp_path)
    for (name, (image, text, chunk), w), g in zip(items, got):
        check_stream(name, g, image, text, w)
        assert g[-1]["done"] == 1 and (w < (1 << 20) or len(g) == 1), (name, w)


@pytest.mark.parametrize("chunk", [256, 32768])
def test_images_in_pieces(tool, tmp_path, chunk):
    """windows of 20 000 stall on stored0's one block of 60 005 bytes: window-limited, and the repeat at 70 000 goes on"""
    images = gm.images()
    items = [(name, v, w) for name, v in images.items() for w in (70000, 20000)]
    got = run_host(tool, [(v[0], chunk, w, len(v[1]), 70000 if w == 20000 else 0) for name, v, w in items], tmp_path)
    stalled = set()
    for (name, (image, text), w), g in zip(items, got):
        check_stream(name, g, image, text, w, 70000 if w == 20000 else 0)
        if any(p["window_limited"] for p in g):
            stalled.add((name, w))
    assert ("stored0", 20000) in stalled and not any(w == 70000 for _, w in stalled)


def test_damaged_images_in_pieces(tool, tmp_path):
    bad = gm.bad_images()
    got = run_host(tool, [(image, chunk, 2048, 200000, 0) for image, chunk in bad.values()], tmp_path)
    for (name, (image, chunk)), g in zip(bad.items(), got):
        check_stream(name, g, image, None, 2048)
        want = gm.gunzip(image)
        last = g[-1]
        assert last["status"] == 1 and last["written"] == 0, name
        assert {k: last[k] for k in ("error", "error_member", "error_offset")} == \
            {k: want[k] for k in ("error", "error_member", "error_offset")}, (name, last)
        # the whole-image walk goes on behind a distance, length or CRC error and counts the members behind it; the pieces
        # behind the one that failed are void, so the stream's count ends with that piece
        stops = want["error"] in (gm.HEADER, gm.TRUNCATED) or (want["error"] == gm.DEFLATE and not name.startswith("far@"))
        assert last["members"] == want["members"] if stops else want["error_member"] <= last["members"] <= want["members"], (name, last)


@pytest.mark.parametrize("build", ["", "_rebase"])
def test_foreign_images_in_pieces(tool, tmp_path, build):
    """Every published state against the model at windows of 600, 4 096 and 70 000 (a block wider than the window stalls and
    is repeated at 70 000); the one-symbol blocks also at the smallest window in which each of their blocks fits, where
    nearly every piece is one block and resumes inside a byte"""
    from test_gunzip_piece_model import foreign_cases
    cases = [c for c in foreign_cases() if not build or c[3] in (600,) or c[3] < 600]
    got = run_host(tool + build, [(image, 256, w, len(text), 70000) for name, image, text, w in cases], tmp_path)
    for (name, image, text, w), g in zip(cases, got):
        g = check_stream(name, g, image, text, w, 70000, fi.piece_stream("valid", name, w))
        assert g[-1]["done"] == 1, (name, w)
        if name in fi.TINY and w < 600:
            assert sum(1 for p in g if p["pos_bit"] & 7) > len(g) // 2 and len(g) > 100, (name, w, len(g))


def test_foreign_bad_images_in_pieces(tool, tmp_path):
    bad = fi.bad_images("gzip")
    items = [(name, image, w) for w in (600, 4096, 70000) for name, (image, chunk) in bad.items()]
    got = run_host(tool, [(image, 256, w, 200000, 70000) for name, image, w in items], tmp_path)
    for (name, image, w), g in zip(items, got):
        g = check_stream(name, g, image, None, w, 70000, fi.piece_stream("bad", name, w))
        want, last = fi.bad_expected("gzip")[name], g[-1]
        assert last["status"] == 1 and last["written"] == 0, name
        assert {k: last[k] for k in ("error", "error_member", "error_offset")} == \
            {k: want[k] for k in ("error", "error_member", "error_offset")}, (name, w, last)


def test_reencoded_fastq_in_pieces(tool, tmp_path):
    """The chain test's images through windows of 66 666 bytes (a third of its pieces of 200 000), the text alone"""
    text, bgzf, plain = fi.reencoded_fastq()
    for g in run_host(tool, [(plain, 1024, 66666, len(text), 0), (bgzf, 1024, 66666, len(text), 0)], tmp_path):
        assert all(p["status"] == 0 for p in g) and g[-1]["done"] == 1 and len(g) > 8
        assert b"".join(p["text"] for p in g) == text


def test_foreign_capacity_cut(tool, tmp_path):
    """One-token blocks, the whole image in the window, 4 096 bytes of text a piece: each piece ends at a block boundary
    within the capacity and the next goes on from there"""
    for name in ("tiny_blocks_match", "tiny_blocks_batch"):
        image, text = fi.valid("gzip")[name]
        points = pm.resume_points(image)
        g = run_host(tool, [(image, 256, len(image), 4096, 0)], tmp_path)[0]
        assert all(p["status"] == 0 and (p["pos_bit"], p["in_member"]) in points and p["bytes_out"] <= 4096 for p in g), name
        assert max(p["max_stretch_text"] for p in g) <= 4096 and all(b["pos_bit"] > a["pos_bit"] for a, b in zip(g, g[1:])), name
        assert b"".join(p["text"] for p in g) == text and g[-1]["done"] == 1 and len(g) >= -(-len(text) // 4096), name


def test_capacity_cut(tool, tmp_path):
    """fq200k_c256 through windows of 8 192 bytes into 4 096 bytes of text a piece: every piece ends at a resume point,
    within the capacity, and goes on; 64 bytes are less than the first stretch needs: status 2 with the need, and the repeat
    at the need goes on"""
    image, text, chunk = gm.stretch_images()["fq200k_c256"]
    points = pm.resume_points(image)
    for capacity in (4096, 64):
        g = run_host(tool, [(image, chunk, 8192, capacity, 0)], tmp_path)[0]
        short = [p for p in g if p["status"] == 2]
        assert bool(short) == (capacity == 64)
        assert all(p["bytes_out"] > 64 and p["written"] == 0 for p in short)
        ok = [p for p in g if p["status"] != 2]
        assert all(p["status"] == 0 and (p["pos_bit"], p["in_member"]) in points for p in ok)
        assert b"".join(p["text"] for p in ok) == text and ok[-1]["done"] == 1
        if capacity == 4096:
            assert max(p["max_stretch_text"] for p in g) <= 4096  # no stretch alone is beyond the capacity
            assert all(p["bytes_out"] <= capacity for p in ok)
            assert all(b["pos_bit"] > a["pos_bit"] for a, b in zip(ok, ok[1:]))
            assert len(ok) > len(text) // 8192  # the capacity cut them, not the window
