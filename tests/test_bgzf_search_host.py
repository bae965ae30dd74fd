"""The searching BGZF encoder (SK_BGZF_SEARCH) without a device: the phases of sickle_amd/csrc/sk_bgzf_search.h and of
the two headers it builds on run on the host lane after lane (tests/bgzf_search/search_host), in both lane orders, against
zlib; the tokens it dumps against the limits of deflate and of the design; the image sizes against the encoder without
the search and against zlib; the same program under the address and undefined-behaviour sanitizers; and the pure sizing
function of the C ABI.  CPU only."""
import struct
import zlib

import pytest

import bgzf_search_texts as st
from bgzf_search_texts import BLOCK


@pytest.fixture(scope="module")
def texts():
    st.build()
    t = dict(st.edge_texts())
    t.update(st.fastq_texts())
    t["synth"] = st.synth_text(3)
    return t


@pytest.fixture(scope="module")
def results(texts, tmp_path_factory):
    """name -> (image, tokens) of the host program, the image being the same for both lane orders"""
    d = tmp_path_factory.mktemp("bgzf_search")
    res = {}
    for name, data in texts.items():
        image = st.host_image(data, d, name)
        assert st.host_image(data, d, name, "rev") == image, name + ": the image depends on the order of the lanes"
        path = str(d / (name + ".txt"))
        tokens = st.run(st.HOST, "tokens", path)
        assert st.run(st.HOST, "tokens", path, "rev") == tokens, name
        res[name] = (image, [tuple(int(x) for x in line.split()) for line in tokens.splitlines()], path)
    return res


def members(image):
    """-> [(text, stored)] of the image's members, each checked against its CRC-32, ISIZE and BSIZE"""
    out, at = [], 0
    while at < len(image):
        assert image[at:at + 4] == b"\x1f\x8b\x08\x04" and image[at + 12:at + 16] == b"BC\x02\x00", at
        m = struct.unpack_from("<H", image, at + 16)[0] + 1
        body = image[at + 18:at + m - 8]
        text = zlib.decompress(body, -15)
        crc, isize = struct.unpack_from("<II", image, at + m - 8)
        assert (zlib.crc32(text), len(text)) == (crc, isize), at
        out.append((text, body[0] & 7 == 1))
        at += m
    assert at == len(image)
    return out


def test_every_member_inflates_to_its_block(texts, results):
    for name, data in texts.items():
        got = members(results[name][0])
        assert [t for t, _ in got] == [data[a:a + BLOCK] for a in range(0, len(data), BLOCK)], name
    assert all(stored for _, stored in members(results["random"][0]))
    assert not any(stored for _, stored in members(results["test.fastq"][0]))
    assert results["empty"][0] == b""


def test_tokens_stay_within_deflate_and_within_their_lines(texts, results):
    for name, data in texts.items():
        last_line = {}  # block -> where its line 2047 starts: the encoder takes everything from there as one line
        for block, pos, length, dist, line_end in results[name][1]:
            where = (name, block, pos, length, dist)
            if block not in last_line:
                ends = [i for i, c in enumerate(data[block * BLOCK:(block + 1) * BLOCK]) if c == 10]
                last_line[block] = ends[2046] + 1 if len(ends) > 2046 else BLOCK
            assert 1 <= dist <= 32768 and dist <= pos, where
            assert 3 <= length <= 258, where
            assert pos + length <= line_end, where
            at = block * BLOCK + pos
            assert data[at:at + length] == bytes(data[at - dist + k % dist] for k in range(length)), where
            # a line ends with its newline: only a match's last byte may be one
            assert pos >= last_line[block] or b"\n" not in data[at:at + length - 1], where
    assert not results["one_byte"][1]
    # nothing reaches back over a block start: the second block is one byte, a literal
    assert all(block == 0 for block, *_ in results["second_block_one_byte"][1])


def test_the_window_ends_at_32768(results):
    """Two equal 40-byte strings 32 768 bytes apart are found (the second is one token); 32 769 apart they are not."""
    near = {(pos, length, dist) for _, pos, length, dist, _ in results["apart_32768"][1]}
    assert (32768, 40, 32768) in near
    far = [(pos, length, dist) for _, pos, length, dist, _ in results["apart_32769"][1]]
    assert far and all(dist <= 32768 for _, _, dist in far)
    assert not any(32769 <= pos < 32769 + 40 and dist > 1 for pos, _, dist in far)


def test_a_repeat_longer_than_258(results):
    tokens = [(pos, length, dist) for _, pos, length, dist, _ in results["long_repeat"][1]]
    # the second and third copy of the 700-byte line: with its newline, 258 + 258 + 185 each, 701 bytes back
    assert [t for t in tokens if t[2] == 701] == [(701, 258, 701), (959, 258, 701), (1217, 185, 701),
                                                  (1402, 258, 701), (1660, 258, 701), (1918, 185, 701)]
    assert any(length == 258 for _, _, length, _, _ in results["one_repeated_byte"][1])


def zlib_blocks(data, level):
    total = 0
    for a in range(0, len(data), BLOCK):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(c.compress(data[a:a + BLOCK]) + c.flush()) + 26  # framed as a member
    return total


def test_sizes(texts, results, tmp_path):
    """The two size conditions; all four sizes are printed (DESIGN 4.8.1 records them)."""
    ratio = {}
    for name in ("test.fastq", "synth"):
        data = texts[name]
        plain = st.host_image(data, tmp_path, name, tool=st.PLAIN)
        assert b"".join(t for t, _ in members(plain)) == data
        search = results[name][0]
        sizes = (len(plain), len(search), zlib_blocks(data, 1), zlib_blocks(data, 6))
        print("%s: text %d  no flag %d (%.2f %%)  SEARCH %d (%.2f %%)  zlib 1 %d (%.2f %%)  zlib 6 %d (%.2f %%)" %
              ((name, len(data)) + sum(((s, 100.0 * s / len(data)) for s in sizes), ())))
        ratio[name] = len(search) / len(plain)
    assert ratio["test.fastq"] <= 0.96
    assert ratio["synth"] <= 1.005


def test_under_the_sanitizers(texts, results):
    """The same program built with -fsanitize=address,undefined, as a stand-alone executable, on every text, in both modes:
    it ends clean and writes the same bytes."""
    for name in texts:
        image, _, path = results[name]
        assert st.run(st.HOST_SAN, "image", path) == image, name
        st.run(st.HOST_SAN, "tokens", path, "rev")


def test_workspace_bytes_flags_needs_no_device():
    from sickle_amd import capi
    L = capi.lib()
    assert capi.SK_BGZF_SEARCH == 2
    for n in [0, 1, 2, 100] + [k * BLOCK + d for k in (1, 2, 3, 1279, 1280, 1281, 70000) for d in (-1, 0, 1)] + [1 << 32, 1 << 40]:
        nb = (n + BLOCK - 1) // BLOCK
        old = L.sk_bgzf_workspace_bytes(n)
        assert L.sk_bgzf_workspace_bytes_flags(n, 0) == L.sk_bgzf_workspace_bytes_flags(n, capi.SK_BGZF_EOF) == old
        for flags in (capi.SK_BGZF_SEARCH, capi.SK_BGZF_SEARCH | capi.SK_BGZF_EOF):
            need = L.sk_bgzf_workspace_bytes_flags(n, flags)
            assert need == old + 261152 * min(nb, 1280) and need % 16 == 0  # the formula of include/sickle_amd.h
