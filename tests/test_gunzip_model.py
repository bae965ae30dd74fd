"""tests/gunzip_model.py against zlib and against itself: the valid images decode to their texts, the block walker sees
what the fixtures are meant to hold, and every damaged image has the reason it was built for.  CPU only."""
import gzip

import pytest

import gunzip_model as gm


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
