"""The device's BGZF reader without a device: the functions of sickle_amd/csrc/sk_inflate_block.h run on the host lane
after lane (tests/bgunzip_device/inflate_host, built with the address and undefined-behaviour sanitizers) against
tests/bgunzip_model.py: every image the GPU tests use, the constructed bad ones reason by reason, and a few thousand seeded
bit flips, byte changes and truncations; and the legal streams zlib never writes (tests/foreign_images.py), constructed,
drawn and bad.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bgunzip_model as bm
import cli_util as cu
import foreign_images as fi

HOST = os.path.join(cu.ROOT, "tests", "bgunzip_device", "inflate_host")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "bgunzip_device"), "all"], check=True)
    return HOST


def run_host(tool, images, d, tag="batch"):
    """images (list of bytes) -> list of dict(error, error_member, error_offset, members, bytes_out, text)"""
    batch, res, txt = (str(d / (tag + e)) for e in (".bin", ".res", ".txt"))
    with open(batch, "wb") as f:
        for image in images:
            f.write(struct.pack("<I", len(image)) + image)
    pr = subprocess.run([tool, batch, res, txt], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    texts, at, out = open(txt, "rb").read(), 0, []
    for line in open(res):
        e, m, off, members, need = (int(x) for x in line.split())
        text = None
        if e == 0:
            text, at = texts[at:at + need], at + need
        out.append(dict(error=e, error_member=m, error_offset=off, members=members, bytes_out=need, text=text))
    assert len(out) == len(images) and at == len(texts)
    return out


def test_valid_images_reproduce_the_text(tool, tmp_path):
    images = bm.images()
    images["empty"] = (b"", b"")
    for count in (1, 63, 64, 65):
        images["small%d" % count] = bm.small_members(count)
    got = run_host(tool, [v[0] for v in images.values()], tmp_path)
    for (name, (image, text)), g in zip(images.items(), got):
        assert g == bm.bgunzip(image), name
        assert g["error"] == 0 and g["text"] == text, name


def test_constructed_bad_images(tool, tmp_path):
    bad = bm.bad_images()
    got = run_host(tool, list(bad.values()), tmp_path)
    for (name, image), g in zip(bad.items(), got):
        assert g == bm.bgunzip(image), name
        assert g["error"] != 0


def test_foreign_valid_and_drawn_images(tool, tmp_path):
    """What zlib never writes: no or one distance code, end-of-block alone, 15-bit codes, repeats across HLIT, 284 + 31,
    set padding bits, thousands of one-symbol and of empty blocks; 40 drawn members in one image"""
    images = fi.valid("bgzf")
    got = run_host(tool, [v[0] for v in images.values()], tmp_path)
    for (name, (image, text)), g in zip(images.items(), got):
        assert g == fi.expected("bgzf")[name], name
        assert g["error"] == 0 and g["text"] == text, name


def test_foreign_drawn_around_the_wave_and_the_reencoded_fastq(tool, tmp_path):
    """The images of tests/test_gpu_bgunzip.py::test_foreign_drawn and of the chain test, on the host first"""
    images = {count: fi.drawn_members("bgzf", seeds)[:2] for count, seeds in fi.WAVE_SEEDS.items()}
    text, bgzf, plain = fi.reencoded_fastq()
    images["fastq"] = (bgzf, text)
    got = run_host(tool, [v[0] for v in images.values()], tmp_path)
    for (name, (image, text)), g in zip(images.items(), got):
        assert (g["error"], g["bytes_out"]) == (0, len(text)) and g["text"] == text, name
        assert g["members"] == (name if name != "fastq" else -(-len(text) // 30000) + 1), name


def test_foreign_bad_images(tool, tmp_path):
    """Reason, member and offset exactly; the two of fi.PRECEDENCE are SK_GZ_LENGTH: under ISIZE 0 the literal in front of
    the failing match is the first token to fail"""
    bad = fi.bad_images("bgzf")
    got = run_host(tool, list(bad.values()), tmp_path)
    reasons = {name: reason for name, (m, reason) in fi.foreign_bad("bgzf").items()}
    for (name, image), g in zip(bad.items(), got):
        assert g == fi.bad_expected("bgzf")[name], name
        assert g["error"] == reasons[name.rsplit("@", 1)[0]], name
    assert {reasons[n] for n in fi.PRECEDENCE} == {bm.LENGTH}


def corruptions(count, seed):
    """Seeded single-bit flips, single-byte changes and truncations of short valid images -> [(what, image)]"""
    rng = np.random.default_rng(seed)
    src = bm.images()
    pool = [src[k][0] for k in ("fixed", "level6", "multi_block", "huffman_only", "extra_first", "chain", "period3", "rle")]
    pool = [m[:0] + bm.member(bm.bgunzip(m)["text"][:3000], lv) for m, lv in zip(pool, (6, 6, 6, 6, 6, 9, 9, 6))]
    pool += [src["extra_first"][0], src["multi_block"][0][:0] + bm.member(src["fq_head"][1], 6, flush_every=300),
             src["chain_fixed"][0], bm.member(src["fq_head"][1], 0), bm.member(src["fq_head"][1], 1, zlib_fixed())]
    out = []
    for i in range(count):
        picks = [pool[int(k)] for k in rng.integers(0, len(pool), 3)]
        image = bytearray(picks[0] + picks[1] + bm.EOF + picks[2])
        kind = int(rng.integers(0, 8))
        at = int(rng.integers(0, len(image)))
        if kind < 4:
            image[at] ^= 1 << int(rng.integers(0, 8))
        elif kind < 7:
            image[at] = int(rng.integers(0, 256))
        else:
            del image[at:]
        out.append(((i, kind, at), bytes(image)))
    return out


def zlib_fixed():
    import zlib
    return zlib.Z_FIXED


def test_seeded_corruptions(tool, tmp_path):
    """An error at the model's member, or a clean decode where the change hit bytes nothing looks at (MTIME, XFL, OS,
    foreign subfields) or left the image as it was.  No sanitizer report (run_host asserts an empty stderr)."""
    cases = corruptions(4000, 2029)
    got = run_host(tool, [c[1] for c in cases], tmp_path)
    clean = same_reason = 0
    for (what, image), g in zip(cases, got):
        want = bm.bgunzip(image)
        if want["error"] == 0:
            assert g == want, what
            clean += 1
        else:
            assert g["error"] != 0 and g["error_member"] == want["error_member"], (what, g["error"], want["error"])
            same_reason += g["error"] == want["error"]
    assert 0 < clean < len(cases) // 4
    assert same_reason > 0.9 * (len(cases) - clean)
