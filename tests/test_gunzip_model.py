"""tests/gunzip_model.py against zlib and against itself: the valid images decode to their texts, the block walker sees
what the fixtures are meant to hold, and every damaged image has the reason it was built for.  CPU only."""
import gzip
import zlib

import numpy as np
import pytest

import gunzip_model as gm
import soak_gunzip


def test_valid_images_are_what_zlib_reads():
    for name, (image, text) in gm.images().items():
        assert gzip.decompress(image) == text, name
        g = gm.gunzip(image)
        assert (g["error"], g["text"], g["bytes_out"]) == (0, text, len(text)), name
    assert gm.gunzip(b"") == dict(error=0, error_member=0, error_offset=0, members=0, bytes_out=0, text=b"")
    assert gm.gunzip(gm.images()["two"][0])["members"] == 2


def test_the_walker_sees_every_kind_of_block():
    kinds = lambda name: {k for _, k, _, _ in gm.walk(gm.images()[name][0])[1]}
    assert kinds("stored0") == {0} and kinds("fixed") == {1} and kinds("level6") == {2}
    assert kinds("mixed") == {0, 2} or kinds("mixed") == {0, 1, 2}
    assert len(gm.walk(gm.images()["multi_block"][0])[1]) > 50


def test_small_blocks_are_mostly_dynamic():
    """memLevel 1 is the generator's setting because its blocks are dynamic: a few hundred per 48 KiB of text"""
    image, text, _ = gm.stretch_images()["fq48k_c1024"]
    blocks = gm.walk(image)[1]
    dynamic = [b for b in blocks if b[1] == 2 and not b[2]]
    assert len(blocks) > 100 and len(dynamic) > 0.9 * len(blocks)
    assert len(gm.dynamic_chunks(image, 1024)) >= len(image) // 1024 - 2


def test_stretch_images_decode():
    for name, (image, text, chunk) in gm.stretch_images().items():
        assert gzip.decompress(image) == text, name
    s = gm.stretch_images()
    assert gm.gunzip(s["members300_c1024"][0])["members"] == 300
    image = s["member_on_boundary_c1024"][0]
    assert gm.walk(image)[1][-1][3] == 1 and image.index(b"\x1f\x8b\x08", 10) % 1024 == 0


REASONS = {"magic": gm.HEADER, "cm": gm.HEADER, "reserved_flag": gm.HEADER, "trailing_byte": gm.HEADER, "cut_header": gm.TRUNCATED,
           "cut_body": gm.DEFLATE, "cut_trailer": gm.TRUNCATED, "dynamic_header": gm.DEFLATE, "far": gm.DEFLATE,
           "isize": gm.LENGTH, "text_bit": gm.CRC, "crc": gm.CRC}


def test_every_damage_has_its_reason():
    bad = gm.bad_images()
    for name, (image, chunk) in bad.items():
        g = gm.gunzip(image)
        assert g["error"] != 0 and g["text"] is None, name
        if "@" in name:
            what, where = name.split("@")
            assert g["error"] == REASONS[what], (name, g)
            assert g["error_member"] == (3 if what == "trailing_byte" else int(where)), (name, g)
            if int(where) == 1:
                assert g["error_offset"] >= 1024, name  # the damaged member starts in a later stretch
        if not name.startswith("reserved_flag"):  # Python's gzip does not look at the reserved bits
            with pytest.raises(Exception):
                gzip.decompress(image)
                pytest.fail("gzip reads " + name)
    assert gm.gunzip(bad["crc_then_header"][0])["error"] == gm.CRC  # the lower member wins


def test_crc_algebra_against_zlib():
    rng = np.random.default_rng(36)
    for n in (0, 1, 2, 255, 65537, 1 << 20):
        a, b = (rng.integers(0, 256, int(k), dtype=np.uint8).tobytes() for k in (rng.integers(0, 70000), n))
        assert gm.crc_combine(zlib.crc32(a), zlib.crc32(b), len(b)) == zlib.crc32(a + b), n
    assert gm.crc_shift(0) == 0x80000000 and gm.crc_shift(1) == 0x00800000 and gm.crc_shift(4) == gm.POLY


def test_spliced_and_repeated_members():
    t = gm.texts()
    image = gm.spliced_member([(t["rnd"], 0, 0, 8), (t["fq"], 6, 0, 1), (t["acgt"], 6, zlib.Z_FIXED, 8), (t["fq"], 9, 0, 1)])
    assert {k for _, k, _, _ in gm.walk(image)[1]} == {0, 1, 2}
    assert gm.gunzip(image)["text"] == t["rnd"] + t["fq"] + t["acgt"] + t["fq"]
    # the member of 4 GiB and more of tests/test_gpu_gunzip.py, with three segments: the structure, the CRC-32 and the
    # blocks, which a guess must be able to decode within its cap for the device to use more than one stretch
    image, seg, tail = gm.repeated_member(3)
    assert gzip.decompress(image) == seg * 3 + tail
    lengths = []
    blocks = gm.walk(image, lengths)[1]
    assert max(lengths) < 4 << 20 and sum(1 for b in blocks if b[1] == 2 and not b[2]) >= 6


def test_long_images_are_what_they_are_for():
    long = gm.long_images()
    image = long["past16m_a"][0]
    blocks = gm.walk(image)[1]
    beyond = {b[1] for b in blocks if b[0] > 8 << 24}
    assert beyond == {0, 1, 2} and sum(1 for b in blocks if b[1] == 2 and b[0] > 8 << 24) > 100
    assert [b[1] for b in blocks if b[0] < 8 * ((1 << 24) - 80000)] == [0] * 256
    assert gm.gunzip(image) == gm.long_want("past16m_a")  # what stands in for the walk of the long valid images is the walk's
    assert gm.long_blocks(long["long_run_m8"][0]) and not gm.long_blocks(long["long_run_m7"][0])
    empty = gm.member(b"")
    image, text, _ = long["empty_members"]
    assert image.startswith(empty) and image.endswith(empty) and gm.gunzip(image) == gm.long_want("empty_members")
    for run in (1, 2, 63, 64, 65):
        assert image.count(empty * run) > 0
    bad = gm.long_bad_images()
    assert bad["past16m_a_bit"][2]["error"] in (gm.DEFLATE, gm.CRC) and bad["past16m_a_crc"][2]["error"] == gm.CRC
    assert bad["past16m_a_cut"][2]["error"] == gm.DEFLATE and bad["past16m_a_cut"][2]["error_offset"] > 1 << 24


def test_soak_gunzip_dry():
    stats = {}
    assert soak_gunzip.run(*soak_gunzip.SLICE, dry=True, verbose=False, stats=stats) == soak_gunzip.SLICE[0]
    soak_gunzip.check_slice(stats, soak_gunzip.SLICE[0])
    assert {k: stats[k] for k in soak_gunzip.SLICE_STATS} == soak_gunzip.SLICE_STATS  # what the device run of the slice is held to
