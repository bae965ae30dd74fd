"""CPU: tests/deflate_writer.py and tests/foreign_images.py against zlib and the Python models.  Every constructed and every
drawn stream is accepted by zlib.decompressobj(-15), ends there and gives the text its tokens spell (the builders assert it;
here once more from outside), gzip.decompress, bgunzip_model.bgunzip and gunzip_model.walk (its own Python inflate and Code
class) agree, the drawn seeds hit every feature, and every constructed bad member takes the verdict stated for it."""
import gzip
import zlib

import pytest

import bgunzip_model as bm
import deflate_writer as dw
import foreign_images as fi
import gunzip_model as gm


def raw_inflate(raw):
    d = zlib.decompressobj(-15)
    text = d.decompress(raw)
    assert d.eof and not d.unused_data
    return text


def test_bit_writer_and_codes():
    w = dw.Bits()
    w.put(1, 1)
    w.put(2, 2)
    w.code(0b110, 3)  # first bit first: 1, 1, 0 follow the three header bits
    assert (w.acc, w.n) == (0b011101, 6)
    w.align(0xff)
    assert bytes(w.out) == bytes([0b11011101])
    assert dw.codes([2, 1, 3, 3]) == [(0b10, 2), (0, 1), (0b110, 3), (0b111, 3)]  # RFC 1951 3.2.2
    assert dw.codes([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]
    assert sorted(dw.ladder(list(range(16)), 16)) == list(range(1, 15)) + [15, 15]
    assert [dw.length_symbol(n) for n in (3, 10, 11, 12, 257, 258)] == [0, 7, 8, 8, 27, 28]
    assert [dw.distance_symbol(d) for d in (1, 4, 5, 6, 7, 24576, 24577, 32768)] == [0, 3, 4, 4, 5, 28, 29, 29]


def test_constructed_streams_are_zlibs_text():
    names = set(fi.streams())
    assert names == set(fi.BUILDERS) and {"no_dist", "one_dist_0", "one_dist_3", "eob_only", "deep_lit15", "deep_dist15", "cl_depth7",
                                         "cross_repeat_zero", "cross_repeat_16", "hlit29_hdist29", "len284_31", "all_symbols", "pad_bits",
                                         "empty_runs_fixed", "empty_runs_pigz"} | set(fi.TINY) <= names
    for name, (raw, text) in fi.streams().items():
        assert raw_inflate(raw) == text and text, name
    # what the names promise, read back off the streams by gunzip_model's walk
    for name, (image, text) in fi.foreign_images("gzip").items():
        lengths = []
        res, blocks = gm.walk(image, lengths)
        assert res["error"] == 0 and res["text"] == text == gzip.decompress(image), name
        if name == "tiny_blocks_sym":
            assert set(lengths) == {1} and len(blocks) == 2400 and {b[1] for b in blocks} == {0, 1, 2}
        if name == "tiny_blocks_batch":
            assert len(blocks) >= 192
        if name == "empty_runs":
            assert lengths[:20000] == [0] * 20000 and len(blocks) > 28000
        if name == "empty_runs_fixed":
            assert lengths[:20000] == [0] * 20000 and all(b[1] == 1 for b in blocks)
        if name == "empty_runs_pigz":
            assert sum(1 for b, n in zip(blocks, lengths) if b[1] == 0 and n == 0) > 5000 and len(blocks) > 8000


def test_both_framings_agree_with_the_models():
    for framing in ("bgzf", "gzip"):
        images = fi.foreign_images(framing)
        assert ("nested_level6" in images) == (framing == "gzip")
        for name, (image, text) in images.items():
            assert gzip.decompress(image) == text, (framing, name)
            got = fi.expected(framing)[name]
            assert got["error"] == 0 and got["text"] == text and got["bytes_out"] == len(text), (framing, name)
    assert bm.bgunzip(fi.foreign_images("bgzf")["foreign_members"][0])["members"] > len(fi.BUILDERS)
    assert gm.gunzip(fi.foreign_images("gzip")["foreign_members"][0])["members"] == len(fi.BUILDERS) + len(fi.GZIP_ONLY)


def test_drawn_streams_and_their_features():
    total = dict.fromkeys(dw.FEATURES, 0)
    for seed in fi.DRAWN_SEEDS:  # none skipped, none redrawn: drawn() raises where zlib does not give the text back
        raw, text, f = dw.drawn(seed)
        assert raw_inflate(raw) == text and 200 <= len(text) <= 40000, seed
        assert dw.drawn(seed)[0] == raw
        for k in f:
            total[k] += f[k]
        res = gm.walk(dw.gzip_member(raw, text))[0]
        assert res["error"] == 0 and res["text"] == text, seed
        assert bm.bgunzip(dw.bgzf_member(raw, text))["text"] == text, seed
    print("drawn features over %d seeds:" % len(fi.DRAWN_SEEDS), total)
    assert all(total[k] >= 1 for k in dw.FEATURES), total


def test_bad_streams_take_their_verdict():
    want = {"one_dist_unassigned", "match_no_dist", "hlit_30", "hlit_31", "hdist_30", "hdist_31", "cl_all_zero",
            "repeat_16_across_past_end", "dist_over", "dist_incomplete_2bit", "lit_single_not_eob", "stored_nlen"}
    assert want <= set(fi.bad_streams())
    for name, (raw, before) in fi.bad_streams().items():
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(raw)
        assert bm.text_before_failure(raw) == before, name
    bad = fi.foreign_bad("bgzf")
    assert set(fi.PRECEDENCE) <= set(bad)
    for name, (member, reason) in bad.items():
        got = bm.bgunzip(member + bm.EOF)
        assert (got["error"], got["error_member"], got["error_offset"]) == (reason, 0, 0), name
        assert reason == (bm.LENGTH if name in fi.PRECEDENCE else bm.DEFLATE), name
    for name, (member, reason) in fi.foreign_bad("gzip").items():
        got = gm.gunzip(member)
        assert (got["error"], got["error_member"]) == (reason, 0), name
    for framing in ("bgzf", "gzip"):
        for name, image in fi.bad_images(framing).items():
            got = bm.bgunzip(image) if framing == "bgzf" else gm.gunzip(image[0])
            where = {"0": 0, "1": 1, "last": 2}[name.rsplit("@", 1)[1]]
            assert got["error"] in (bm.DEFLATE, bm.LENGTH) and got["error_member"] == where, (framing, name)


def test_precedence_of_length_over_a_later_deflate_fault():
    """include/sickle_amd.h: text beyond ISIZE is SK_GZ_LENGTH at the token that would cross it, and the first check to fail
    is the member's reason.  A literal, then a match whose distance has no code: under ISIZE 0 the literal crosses first;
    under ISIZE 1 the match is the first to fail, and its distance is looked at before its length is."""
    for name in ("one_dist_unassigned_first", "match_no_dist_first"):
        raw = fi.bad_streams()[name][0]
        assert [bm.decode(raw, 0, isize)[0] for isize in (0, 1, 2, 4, 65536)] == [bm.LENGTH] + [bm.DEFLATE] * 4, name
