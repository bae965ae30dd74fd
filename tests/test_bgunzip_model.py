"""tests/bgunzip_model.py, the Python statement of the rules of sk_bgzf_inflate_device_async, against gzip.decompress on
valid images and against hand-built bad ones.  CPU only."""
import gzip
import zlib

import pytest

import bgunzip_model as bm
import soak_bgunzip


@pytest.fixture(scope="module")
def images():
    return bm.images()


def test_valid_images_equal_gzip(images):
    for name, (image, text) in images.items():
        assert gzip.decompress(image) == text, name
        r = bm.bgunzip(image)
        assert (r["error"], r["text"], r["bytes_out"]) == (bm.OK, text, len(text)), name
    assert bm.bgunzip(b"") == dict(error=0, error_member=0, error_offset=0, members=0, bytes_out=0, text=b"")
    assert bm.bgunzip(bm.EOF)["members"] == 1 and len(bm.EOF) == 28
    assert bm.bgunzip(images["empties"][0])["members"] == 6


def test_member_kinds(images):
    """member() yields what the tests rely on: stored, fixed and dynamic blocks, several blocks, subfields ahead of BC."""
    first = lambda image: (image[12 + int.from_bytes(image[10:12], "little")] >> 1) & 3
    assert first(images["stored0"][0]) == 0 and first(images["stored_random"][0]) == 0
    assert first(images["fixed"][0]) == 1 and first(bm.EOF) == 1
    for name in ("level1", "level6", "level9", "huffman_only", "rle", "chain"):
        assert first(images[name][0]) == 2, name
    assert first(images["far"][0]) == 0 and len(images["far"][0]) < 34000  # stored, then copies from 32 768 back
    assert images["extra_first"][0][12:14] == b"XY" and len(images["full"][1]) == 65536
    assert len(images["multi_block"][0]) > len(images["level6"][0])
    image, text = bm.small_members(65)
    assert bm.bgunzip(image)["members"] == 65 and gzip.decompress(image) == text


def test_every_constructed_reason():
    good = bm.member(b"ahead\n")
    for name, (m, want) in bm.bad_members().items():
        r = bm.bgunzip(good + m)
        assert (r["error"], r["error_member"], r["error_offset"], r["text"]) == (want, 1, len(good), None), name
        if want in (bm.DEFLATE, bm.LENGTH, bm.CRC):
            assert r["members"] == 2, name
            with pytest.raises((zlib.error, EOFError, gzip.BadGzipFile)):
                gzip.decompress(good + m)
        else:
            assert r["members"] == 1, name
    reasons = {want for _, want in bm.bad_members().values()}
    assert reasons == {bm.HEADER, bm.DEFLATE, bm.LENGTH, bm.CRC}


def test_framing_damage_and_precedence():
    bad = bm.bad_images()
    r = bm.bgunzip(bad["two_bad"])
    assert (r["error"], r["error_member"]) == (bm.CRC, 1)
    r = bm.bgunzip(bad["bad_then_garbage"])
    assert (r["error"], r["error_member"], r["members"]) == (bm.LENGTH, 1, 2)  # the lower member wins over the framing
    assert (bm.bgunzip(bad["plain_gzip"])["error"], bm.bgunzip(bad["plain_gzip"])["error_member"]) == (bm.HEADER, 0)
    for name, want, member in (("garbage_after", bm.HEADER, 3), ("short_garbage_after", bm.HEADER, 2),
                               ("cut_one_short", bm.TRUNCATED, 2), ("cut_in_header", bm.TRUNCATED, 1),
                               ("cut_magic", bm.TRUNCATED, 1), ("cut_in_extra", bm.TRUNCATED, 1)):
        r = bm.bgunzip(bad[name])
        assert (r["error"], r["error_member"], r["members"]) == (want, member, member), name
    for name, image in bad.items():
        r = bm.bgunzip(image)
        assert r["error"] != bm.OK and r["text"] is None, name
        if "@" in name:
            want = bm.bad_members()[name.split("@")[0]][1]
            at = {"0": 0, "1": 1, "last": 2}[name.split("@")[1]]
            assert (r["error"], r["error_member"]) == (want, at), name


def test_soak_bgunzip_dry():
    stats = {}
    assert soak_bgunzip.run(*soak_bgunzip.SLICE, dry=True, verbose=False, stats=stats) == soak_bgunzip.SLICE[0]
    soak_bgunzip.check_slice(stats, soak_bgunzip.SLICE[0])
    assert {k: stats[k] for k in soak_bgunzip.SLICE_STATS} == soak_bgunzip.SLICE_STATS  # what the device run of the slice is held to
