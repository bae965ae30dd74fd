"""The device's plain-gzip reader without a device: the stages of sickle_amd/csrc/sk_gunzip_block.h (search, count, chain,
decode, windows, resolve, CRC) run on the host lane after lane (tests/gunzip_device/gunzip_host, built with the address and
undefined-behaviour sanitizers) against tests/gunzip_model.py: every image the GPU tests use, at chunk sizes that cut them
into one, a few and hundreds of stretches, every damaged image, and seeded corruptions.  The same once more with a second
build of the harness whose bit reader re-bases every 64 bytes (gunzip_host_rebase), the images beyond 16 MiB, beyond the
guess's text cap and with 6 000 members (gunzip_model.long_images), and the CRC-32 shift table against Python integers.
And the legal streams zlib never writes (tests/foreign_images.py) through both builds.  CPU only."""
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import cli_util as cu
import foreign_images as fi
import gunzip_model as gm

HOST = os.path.join(cu.ROOT, "tests", "gunzip_device", "gunzip_host")
KEYS = ("error", "error_member", "error_offset")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "gunzip_device"), "all"], check=True)
    return HOST


@pytest.fixture(scope="module")
def rebase_tool(tool):
    return tool + "_rebase"


def run_host(tool, items, d, tag="batch"):
    """items: list of (image, chunk) -> list of dict(error, error_member, error_offset, members, bytes_out, text,
    stretches, stretches_used)"""
    batch, res, txt = (str(d / (tag + e)) for e in (".bin", ".res", ".txt"))
    with open(batch, "wb") as f:
        for image, chunk in items:
            f.write(struct.pack("<II", chunk, len(image)) + image)
    pr = subprocess.run([tool, batch, res, txt], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    texts, at, out = open(txt, "rb").read(), 0, []
    for line in open(res):
        e, m, off, members, need, S, U = (int(x) for x in line.split())
        text = None
        if e == 0:
            text, at = texts[at:at + need], at + need
        out.append(dict(error=e, error_member=m, error_offset=off, members=members, bytes_out=need, text=text, stretches=S,
                        stretches_used=U))
    assert len(out) == len(items) and at == len(texts)
    return out


def test_valid_images_at_every_chunk_size(tool, tmp_path):
    images = dict(gm.images())
    images["empty"] = (b"", b"")
    items = [(name, image, text, chunk) for chunk in (256, 4096, 32768) for name, (image, text) in images.items()]
    got = run_host(tool, [(i[1], i[3]) for i in items], tmp_path)
    for (name, image, text, chunk), g in zip(items, got):
        want = gm.gunzip(image)
        assert {k: g[k] for k in want} == want, (name, chunk)
        assert g["text"] == text and g["stretches"] == -(-len(image) // chunk), (name, chunk)


def test_stretch_images(tool, tmp_path):
    """Text and counts are the model's, and the chain goes through at least half the chunks in which a non-final dynamic
    block begins: a reader that decodes everything from stretch 0 does not pass."""
    s = gm.stretch_images()
    got = run_host(tool, [(v[0], v[2]) for v in s.values()], tmp_path)
    for (name, (image, text, chunk)), g in zip(s.items(), got):
        want = gm.gunzip(image)
        assert {k: g[k] for k in want} == want and g["text"] == text, name
        dyn = gm.dynamic_chunks(image, chunk)
        assert g["stretches_used"] >= 1 + len(dyn) / 2, (name, g["stretches_used"], len(dyn))
        assert g["stretches_used"] <= g["stretches"] == -(-len(image) // chunk), name
    counts = {name: g["stretches_used"] for name, g in zip(s, got)}
    assert [g["stretches"] for name, g in zip(s, got) if name in ("s63_c1024", "s64_c1024", "s65_c1024")] == [63, 64, 65]
    assert counts["fq48k_c4096"] > 4 and 60 < counts["fq48k_c256"] and counts["fq200k_c256"] > 250


def test_damaged_images(tool, tmp_path):
    bad = gm.bad_images()
    got = run_host(tool, list(bad.values()), tmp_path)
    for (name, (image, chunk)), g in zip(bad.items(), got):
        want = gm.gunzip(image)
        assert want["error"] != 0 and tuple(g[k] for k in KEYS) == tuple(want[k] for k in KEYS), (name, g)


def corruptions(count, seed):
    """Seeded single-bit flips, single-byte changes and truncations of short multi-member images -> [(what, image)]"""
    rng = np.random.default_rng(seed)
    pool = [gm.small_blocks(gm.fastq_text(2500, 40 + k), 1 + k) for k in range(6)]
    pool += [gm.member(gm.images()[k][1][:2500], lv, st) for k, lv, st in
             (("fixed", 6, 4), ("stored0", 0, 0), ("huffman_only", 6, 2))]
    out = []
    for i in range(count):
        picks = [pool[int(k)] for k in rng.integers(0, len(pool), 3)]
        image = bytearray(b"".join(picks))
        kind, at = int(rng.integers(0, 8)), int(rng.integers(0, len(image)))
        if kind < 4:
            image[at] ^= 1 << int(rng.integers(0, 8))
        elif kind < 7:
            image[at] = int(rng.integers(0, 256))
        else:
            del image[at:]
        out.append(((i, kind, at), bytes(image)))
    return out


def test_seeded_corruptions(tool, tmp_path):
    """The model's verdict, to the byte, or a clean decode where the change hit bytes nothing looks at.  No sanitizer report
    (run_host asserts an empty stderr)."""
    cases = corruptions(1500, 2031)
    got = run_host(tool, [(c[1], 256) for c in cases], tmp_path)
    clean = 0
    for (what, image), g in zip(cases, got):
        want = gm.gunzip(image)
        assert tuple(g[k] for k in KEYS) == tuple(want[k] for k in KEYS), (what, g, want)
        if want["error"] == 0:
            assert g["text"] == want["text"], what
            clean += 1
    assert 0 < clean < len(cases) // 3


# ---- the bit reader re-based every 64 bytes: at every block, every batch of tokens, every alignment of the fixtures ----
def test_rebase_valid_images(rebase_tool, tmp_path):
    images = dict(gm.images())
    images["empty"] = (b"", b"")
    items = [(name, image, text, chunk) for chunk in (256, 4096) for name, (image, text) in images.items()]
    got = run_host(rebase_tool, [(i[1], i[3]) for i in items], tmp_path)
    for (name, image, text, chunk), g in zip(items, got):
        want = gm.gunzip(image)
        assert {k: g[k] for k in want} == want, (name, chunk)
        assert g["text"] == text and g["stretches"] == -(-len(image) // chunk), (name, chunk)


def test_rebase_stretch_images(rebase_tool, tool, tmp_path):
    s = gm.stretch_images()
    got = run_host(rebase_tool, [(v[0], v[2]) for v in s.values()], tmp_path)
    plain = run_host(tool, [(v[0], v[2]) for v in s.values()], tmp_path, "plain")
    for (name, (image, text, chunk)), g, p in zip(s.items(), got, plain):
        want = gm.gunzip(image)
        assert {k: g[k] for k in want} == want and g["text"] == text, name
        assert (g["stretches"], g["stretches_used"]) == (p["stretches"], p["stretches_used"]), name


def test_rebase_damaged_images_and_corruptions(rebase_tool, tmp_path):
    bad = gm.bad_images()
    got = run_host(rebase_tool, list(bad.values()), tmp_path)
    for (name, (image, chunk)), g in zip(bad.items(), got):
        want = gm.gunzip(image)
        assert want["error"] != 0 and tuple(g[k] for k in KEYS) == tuple(want[k] for k in KEYS), (name, g)
    cases = corruptions(300, 2032)
    got = run_host(rebase_tool, [(c[1], 256) for c in cases], tmp_path, "seeded")
    for (what, image), g in zip(cases, got):
        want = gm.gunzip(image)
        assert tuple(g[k] for k in KEYS) == tuple(want[k] for k in KEYS), (what, g, want)
        if want["error"] == 0:
            assert g["text"] == want["text"], what


# ---- legal streams zlib never writes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("build", ["", "_rebase"])
def test_foreign_images(tool, tmp_path, build):
    """Every key of the model at chunks of 256, 1 024 and 32 768 (for `nested`, whose stored text is full of block starts,
    the text alone).  At 256 the chain joins at guessed starts inside the one-symbol blocks and between the empty ones: more
    than half the stretches are used.  (empty_runs_fixed alone is 20 000 fixed blocks and has no start to guess: the search
    takes non-final dynamic blocks only.)"""
    images = fi.valid("gzip")
    items = [(name, image, text, chunk) for chunk in (256, 1024, 32768) for name, (image, text) in images.items()]
    got = run_host(tool + build, [(i[1], i[3]) for i in items], tmp_path)
    for (name, image, text, chunk), g in zip(items, got):
        want = fi.expected("gzip")[name]
        assert g["text"] == text, (name, chunk)
        if name not in fi.NESTED:
            assert {k: g[k] for k in want} == want and g["stretches"] == -(-len(image) // chunk), (name, chunk)
        if chunk == 256 and name in fi.TINY + ("empty_runs", "empty_runs_pigz"):
            assert g["stretches_used"] > g["stretches"] / 2, (name, g["stretches_used"], g["stretches"])


def test_reencoded_fastq(tool, tmp_path):
    """The chain test's plain member and its BGZF image, on the host first, at the chunk that test reads them with"""
    text, bgzf, plain = fi.reencoded_fastq()
    for g in run_host(tool, [(plain, 1024), (bgzf, 1024)], tmp_path):
        assert g["error"] == 0 and g["text"] == text and g["stretches_used"] > g["stretches"] / 4, (g["stretches"], g["stretches_used"])


@pytest.mark.parametrize("build", ["", "_rebase"])
def test_foreign_bad_images(tool, tmp_path, build):
    bad = fi.bad_images("gzip")
    got = run_host(tool + build, list(bad.values()), tmp_path)
    for (name, (image, chunk)), g in zip(bad.items(), got):
        want = fi.bad_expected("gzip")[name]
        assert want["error"] == gm.DEFLATE and tuple(g[k] for k in KEYS) == tuple(want[k] for k in KEYS), (name, g)


# ---- the long images, with the threshold where the library has it ------------------------------------------------------
def host_chunk(chunk):
    return chunk or 32768  # what the library takes for an image of up to 128 MiB


@pytest.fixture(scope="module")
def long_runs(tool, tmp_path_factory):
    """name -> the host run of every long image, valid and damaged (tests/test_gpu_gunzip.py holds the device to them)"""
    d = tmp_path_factory.mktemp("gunzip_long")
    items = {name: (v[0], host_chunk(v[2])) for name, v in gm.long_images().items()}
    items.update({name: (v[0], host_chunk(v[1])) for name, v in gm.long_bad_images().items()})
    got = {}
    for name, item in items.items():  # one at a time: the harness reads a batch's texts back as one file
        got[name] = run_host(tool, [item], d, name)[0]
    return got


def test_long_images(long_runs):
    """One stretch that reads 16 MiB and more re-bases its bit reader: in small dynamic blocks at eight alignments, in a
    stored and in a fixed block.  A guessed block of more than 4 MiB of text is dropped, one of 2 MiB is not.  6 000
    members, runs of empty ones among them."""
    for name, (image, text, chunk) in gm.long_images().items():
        g, want = long_runs[name], gm.long_want(name)
        assert {k: g[k] for k in want if k != "text"} == {k: want[k] for k in want if k != "text"}, name
        assert g["text"] == text, name
        assert g["stretches"] == -(-len(image) // host_chunk(chunk)), name
        if chunk == 1 << 25:
            assert g["stretches"] == g["stretches_used"] == 1, name
    assert gm.gunzip(gm.long_images()["empty_members"][0]) == gm.long_want("empty_members")
    assert long_runs["past16m_d_default"]["stretches_used"] > 1 and long_runs["empty_members_c256"]["stretches_used"] > 50
    assert long_runs["past16m_stored"]["stretches_used"] == long_runs["past16m_fixed"]["stretches_used"] == 1
    assert long_runs["long_run_m7"]["stretches_used"] > 1
    # m8: the two blocks that begin inside the run hold 4 226 814 bytes of text each, more than the cap and the 64 copies
    # of a batch beyond it, so their guesses are dropped; the FASTQ ends lie in the first and the last block, and the last
    # is final: nothing is left to join, and the text is right all the same
    assert long_runs["long_run_m8"]["stretches_used"] == 1


def test_long_damaged_images(long_runs):
    for name, (image, chunk, want) in gm.long_bad_images().items():
        g = long_runs[name]
        assert want["error"] != 0 and tuple(g[k] for k in KEYS) == tuple(want[k] for k in KEYS), (name, g)


# ---- the CRC-32 shifts -------------------------------------------------------------------------------------------------
def shift_numbers():
    rng = np.random.default_rng(34)
    ks = [0, 1, (1 << 34) - 1]
    for j in range(34):
        ks += [1 << j, (1 << j) - 1, (1 << j) + 1]
    return ks + [int(k) for k in rng.integers(0, 1 << 34, 200)]


def test_crc_shifts_against_python_integers(tool, tmp_path):
    """skg_crc_tables and skg_shift_of for every power x^(8 * 2^j), j = 0..33, and drawn 34-bit shifts; and a CRC-32
    assembled as skg_crc_piece and skg_check_member do it, from two spans, against zlib"""
    rng = np.random.default_rng(35)
    for n in (0, 1, 7, 4096, 1 << 20):  # the model's algebra first, against zlib alone
        a, b = (rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in (rng.integers(0, 5000), n))
        assert gm.crc_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b)
    assert gm.crc_shift(0) == 0x80000000 and gm.crc_shift(1) == 0x00800000
    ks = shift_numbers()
    numbers, res = tmp_path / "k.txt", tmp_path / "shift.txt"
    numbers.write_text("".join("%d\n" % k for k in ks))
    pr = subprocess.run([tool, "--shift", str(numbers), str(res)], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    got = [int(x) for x in res.read_text().split()]
    assert len(got) == len(ks)
    for k, g in zip(ks, got):
        assert g == gm.crc_shift(k), (k, hex(g))
    for n, cut in ((1 << 20, 1 << 19), (100001, 50000), (70000, 0), (70000, 70000), (1, 0)):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        buf = tmp_path / "buffer.bin"
        buf.write_bytes(data)
        pr = subprocess.run([tool, "--crc", str(buf), str(cut), str(res)], capture_output=True)
        assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
        assert int(res.read_text()) == zlib.crc32(data), (n, cut)
