"""The device's plain-gzip reader without a device: the stages of sickle_amd/csrc/sk_gunzip_block.h (search, count, chain,
decode, windows, resolve, CRC) run on the host lane after lane (tests/gunzip_device/gunzip_host, built with the address and
undefined-behaviour sanitizers) against tests/gunzip_model.py: every image the GPU tests use, at chunk sizes that cut them
into one, a few and hundreds of stretches, every damaged image, and seeded corruptions.  CPU only."""
import os
import struct
import subprocess

import numpy as np
import pytest

import cli_util as cu
import gunzip_model as gm

HOST = os.path.join(cu.ROOT, "tests", "gunzip_device", "gunzip_host")
KEYS = ("error", "error_member", "error_offset")


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "gunzip_device"), "all"], check=True)
    return HOST


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
