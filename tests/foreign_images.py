"""Legal deflate streams zlib never writes, as test images for all four gzip readers: streams() are the constructed raw
streams (each held against zlib where it is built), foreign_images(framing) frames them as BGZF members or plain gzip
members, drawn_members() frames tests/deflate_writer.py's drawn streams, bad_streams() / foreign_bad() are the constructed
bad members.  Everything comes from seeds; nothing here is zlib's output except the texts of `nested`."""
import functools
import gzip
import os

import numpy as np

import bgunzip_model as bm
import deflate_writer as dw
import gunzip_model as gm
from deflate_writer import Stream, balanced, ladder

BASES = b"ACGTN"
PRE = b"foreign "


def fq(n, seed=1951):
    return gm.fastq_text(n, seed)


def _no_dist():
    text = fq(3000)
    s = Stream()
    s.dynamic(1, balanced(dw.symbols_of(text)[0], 257), [0], list(text))
    return s.finish()


def _one_dist(sym):
    """one distance code of one bit, as symbol `sym`; length 258 from distance 1 or 4: the copies overlap themselves"""
    d = dw.DIST_BASE[sym]
    tokens = list(b"ACGT") + [(258, d)] * 20 + list(b"\n+xyz") + [(258, d)] * 3 + [(5, d), 10]
    s = Stream()
    lit = dw.symbols_of(tokens)[0]
    s.dynamic(1, balanced(lit, max(lit) + 1), [0] * sym + [1], tokens)
    return s.finish()


def _eob_only():
    s = Stream()
    s.dynamic(0, [0] * 256 + [1], [0], [])
    s.fixed(1, list(fq(500)))
    return s.finish()


def _deep_lit15():
    """two blocks of the ladder 1, 2, ..., 14, 15, 15 over fifteen literals and end-of-block, which sits on 15 bits"""
    rng = np.random.default_rng(15)
    alphabet = list(b"ACGTN@+\n0123456")
    s = Stream()
    for k, order in enumerate((alphabet, alphabet[::-1])):
        tokens = [int(x) for x in rng.choice(order, 700)] + order + order[::-1]
        lens = ladder(order[:14] + ([256, order[14]] if k else [order[14], 256]), 257)
        assert lens[256] == 15 and all(lens[c] for c in order)
        s.dynamic(k, lens, [0], tokens)
    return s.finish()


def _deep_dist15():
    """the ladder over distance symbols 0..15 (every one used at both ends of its extra bits) and, behind 25 000 bytes,
    over symbols 14..29"""
    s = Stream()
    s.fixed(0, list(fq(300, 16)))
    for k, order in enumerate(([5, 0, 9, 3, 12, 1, 15, 7, 2, 10, 4, 13, 6, 11, 8, 14], [20, 29, 14, 25, 17, 22, 28, 15, 19, 26, 16, 23, 18, 27, 24, 21])):
        if k:
            s.stored(0, fq(33000, 17))
        tokens = []
        for i, d in enumerate(order):
            for x in (0, (1 << dw.DIST_EXTRA[d]) - 1):
                tokens += [(3 + (i + x) % 9, dw.DIST_BASE[d] + x), BASES[i % 5]]
        lit = dw.symbols_of(tokens)[0]
        s.dynamic(k, balanced(lit, max(lit) + 1), ladder(order, max(order) + 1), tokens)
    return s.finish()


def _cl_depth7():
    """a code-length code 1, 2, ..., 6, 7, 7 over the eight symbols the lengths use"""
    rng = np.random.default_rng(7)
    lens = ladder(list(b"ACGTN") + [256], 257, top=5)
    items = dw.rle(lens + [0])
    assert {it[0] if isinstance(it, tuple) else it for it in items} == {0, 1, 2, 3, 4, 5, 17, 18}
    s = Stream()
    s.dynamic(1, lens, [0], [int(x) for x in rng.choice(list(BASES), 900)], ladder([18, 17, 1, 2, 3, 0, 4, 5], 19, top=7), items)
    return s.finish()


def _cross_repeat_zero():
    """HLIT = 29; the zeros of the last literal/length entries and of the first distance entries are one 18"""
    tokens = list(fq(400, 18)) + [(10, 100), (20, 200), (3, 9)] + list(b"\n")
    lit, dist = dw.symbols_of(tokens)
    lens = balanced(lit, 286) + balanced(dist, 16)
    items = dw.rle(lens)
    cross = [it for it, at in zip(items, dw.spelled(items)[1]) if isinstance(it, tuple) and at < 286 < at + it[1]]
    assert cross == [(18, 286 - 1 - max(lit) + min(dist))]
    s = Stream()
    s.dynamic(1, lens[:286], lens[286:], tokens, cl_items=items)
    return s.finish()


def _cross_repeat_16():
    """sixteen literal/length codes and sixteen distance codes of four bits: the run of fours goes from symbol 256 to the
    last distance entry, spelt 4, 16 x 6, 16 x 6, ...: the second 16 covers 263, 264 and the first four distance entries"""
    lits = list(b"ACGTN\n@")
    tokens = lits * 40
    for i in range(16):
        tokens += [(3 + i % 8, dw.DIST_BASE[i] + (i & 1 if dw.DIST_EXTRA[i] else 0)), lits[i % 7]]
    lit, dist = dw.symbols_of(tokens)
    assert sorted(lit) == sorted(lits) + list(range(256, 265)) and sorted(dist) == list(range(16))
    lens = balanced(lit, 265) + balanced(dist, 16)
    items = dw.rle(lens)
    assert items[-5:] == [4, (16, 6), (16, 6), (16, 6), (16, 6)] and dw.crossings(items, 265) == 1
    s = Stream()
    s.dynamic(1, lens[:265], lens[265:], tokens, cl_items=items)
    return s.finish()


def _hlit29_hdist29():
    tokens = list(fq(25000, 19)) + [(258, 24577 + 100), 10, (258, 25000), 10]
    lit, dist = dw.symbols_of(tokens)
    assert 285 in lit and 29 in dist
    s = Stream()
    s.dynamic(1, balanced(range(286), 286), balanced(range(30), 30), tokens)
    return s.finish()


def _len284_31():
    s = Stream()
    s.fixed(0, list(b"abc") + [(258, 3, 284), 10])
    tokens = list(b"xy") + [(258, 1, 284), (258, 258), (258, 2, 284), 10]
    s.plain_dynamic(1, tokens)
    return s.finish()


def sweep():
    """every length symbol and every distance symbol at the lowest and the highest value of its extra bits"""
    tokens = []
    for sym in range(29):
        for x in sorted({0, (1 << dw.LEN_EXTRA[sym]) - 1}):
            tokens.append((dw.LEN_BASE[sym] + x, 1 + 37 * sym + x, 257 + sym))
    for sym in range(30):
        for x in sorted({0, (1 << dw.DIST_EXTRA[sym]) - 1}):
            tokens.append((3 + sym % 5, dw.DIST_BASE[sym] + x))
    return tokens


def _all_symbols():
    s = Stream()
    s.fixed(0, list(fq(33000, 20)) + sweep())
    s.plain_dynamic(1, sweep())
    return s.finish()


def _pad_bits():
    """stored blocks behind blocks that end at each of the 8 bit phases, every padding bit set; an empty stored block in
    the middle and a final one"""
    s, phases = Stream(), set()
    for j in range(8):
        s.fixed(0, list(b"phase %d " % j) + [200] * j)  # 200 has a code of 9 bits
        phases.add(s.w.n)
        s.stored(0, b"<stored %d>" % j, 0xff)
    assert phases == set(range(8))
    s.stored(0, b"", 0xff)
    s.plain_dynamic(0, list(b"dyn"))
    s.stored(0, b"behind a dynamic block\n", 0xff)
    s.fixed(0, [10])
    s.stored(1, b"", 0xff)
    return s.finish(0xff)


def _block(s, kind, final, tokens):
    if kind == 0:
        s.stored(final, s.spell(tokens), 0xaa)
    elif kind == 1:
        s.fixed(final, tokens)
    else:
        s.plain_dynamic(final, tokens)


def _tiny_blocks_sym():
    """one literal a block, the kinds alternating"""
    text = fq(2400, 21)
    s = Stream()
    for i, c in enumerate(text):
        _block(s, i % 3, i + 1 == len(text), [c])
    return s.finish()


def _tiny_blocks_match():
    """one token a block, several hundred of them matches: every copy reads what blocks before it wrote"""
    rng = np.random.default_rng(22)
    text = fq(9000, 22)
    tokens = dw.tokenize(rng, text, 0.97)
    assert sum(isinstance(t, tuple) for t in tokens) > 300
    s = Stream()
    for i, t in enumerate(tokens):
        _block(s, (i + i // 7) % 3, i + 1 == len(tokens), [t])
    return s.finish()


def _tiny_blocks_batch():
    """blocks of exactly 63, 64 and 65 tokens (the readers' batch is 64) among blocks of 0 to 9, more than 192 in all"""
    rng = np.random.default_rng(23)
    tokens = dw.tokenize(rng, fq(12000, 23), 0.5)
    sizes = [63, 1, 64, 2, 65, 0, 3, 64, 64, 1, 65, 63, 5, 128, 9, 1, 1, 127, 129, 4, 2]
    s, i, k = Stream(), 0, 0
    while i < len(tokens):
        n = sizes[k % len(sizes)] if k < 60 else 1 + k % 9
        _block(s, 1 + k % 2 if n > 9 else k % 3, i + n >= len(tokens), tokens[i:i + n])
        i, k = i + n, k + 1
    assert k >= 192
    return s.finish()


def _empty_runs_fixed():
    s = Stream()
    for _ in range(20000):
        s.fixed(0, [])
    s.fixed(1, list(fq(2000, 24)))
    return s.finish()


def _empty_runs_pigz(s=None):
    """3 000 small blocks with 0 to 4 empty stored blocks between each"""
    rng = np.random.default_rng(25)
    tokens = dw.tokenize(rng, fq(9000, 25), 0.3)
    assert len(tokens) >= 3000
    s = s or Stream()
    for k in range(3000):
        a, b = k * len(tokens) // 3000, (k + 1) * len(tokens) // 3000
        _block(s, int(rng.choice([0, 1, 1, 1, 1, 2])), 0, tokens[a:b])
        for _ in range(int(rng.integers(0, 5))):
            s.stored(0, b"", int(rng.integers(0, 256)))
    s.fixed(1, [])
    return s.finish()


def _empty_runs():
    """both in one stream, more than a BGZF member holds: 20 000 empty fixed blocks in front of the 3 000 small blocks"""
    s = Stream()
    for _ in range(20000):
        s.fixed(0, [])
    return _empty_runs_pigz(s)


BUILDERS = {
    "no_dist": _no_dist, "one_dist_0": lambda: _one_dist(0), "one_dist_3": lambda: _one_dist(3), "eob_only": _eob_only,
    "deep_lit15": _deep_lit15, "deep_dist15": _deep_dist15, "cl_depth7": _cl_depth7, "cross_repeat_zero": _cross_repeat_zero,
    "cross_repeat_16": _cross_repeat_16, "hlit29_hdist29": _hlit29_hdist29, "len284_31": _len284_31, "all_symbols": _all_symbols,
    "pad_bits": _pad_bits, "tiny_blocks_sym": _tiny_blocks_sym, "tiny_blocks_match": _tiny_blocks_match,
    "tiny_blocks_batch": _tiny_blocks_batch, "empty_runs_fixed": _empty_runs_fixed, "empty_runs_pigz": _empty_runs_pigz,
}
TINY = ("tiny_blocks_sym", "tiny_blocks_match", "tiny_blocks_batch")
EMPTY_RUNS = ("empty_runs_fixed", "empty_runs_pigz")
GZIP_ONLY = ("empty_runs", "nested_small_blocks", "nested_tiny_x4", "nested_level6")
NESTED = ("nested_small_blocks", "nested_tiny_x4", "nested_level6")


@functools.lru_cache(maxsize=None)
def streams():
    """name -> (raw deflate stream, text), each accepted by zlib with this text (Stream.finish)"""
    return {name: build() for name, build in BUILDERS.items()}


@functools.lru_cache(maxsize=None)
def foreign_images(framing):
    """framing "bgzf" or "gzip" -> name -> (image, text): each stream as one member, `nested` (plain gzip only) and
    `foreign_members`, all of them as members of one image (BGZF: with EOF members between some)."""
    assert framing in ("bgzf", "gzip")
    wrap = dw.bgzf_member if framing == "bgzf" else dw.gzip_member
    out = {name: (wrap(raw, text), text) for name, (raw, text) in streams().items()}
    if framing == "gzip":
        both = _empty_runs()
        out["empty_runs"] = (wrap(*both), both[1])
        small = gm.small_blocks(fq(60000, 26))
        tiny4 = streams()["tiny_blocks_sym"][0] * 4
        out["nested_small_blocks"] = (gm.member(small, 0), small)
        out["nested_tiny_x4"] = (gm.member(tiny4, 0), tiny4)
        both = out["nested_small_blocks"][0] + out["tiny_blocks_batch"][0] + out["nested_tiny_x4"][0]
        out["nested_level6"] = (gm.member(both, 6), both)
    parts = list(out.values())
    image = b"".join(m + (bm.EOF if framing == "bgzf" and k % 3 == 1 else b"") for k, (m, _) in enumerate(parts))
    out["foreign_members"] = (image, b"".join(t for _, t in parts))
    for name, (image, text) in out.items():
        assert gzip.decompress(image) == text, name
    return out


@functools.lru_cache(maxsize=None)
def expected(framing):
    """name -> what the model says of foreign_images(framing)[name] and of "drawn", computed once"""
    images = dict(foreign_images(framing))
    images["drawn"] = drawn_members(framing, DRAWN_SEEDS)[:2]
    return {name: (bm.bgunzip if framing == "bgzf" else gm.gunzip)(image) for name, (image, text) in images.items()}


@functools.lru_cache(maxsize=None)
def valid(framing):
    """foreign_images(framing) and "drawn", one member a seed of DRAWN_SEEDS"""
    images = dict(foreign_images(framing))
    images["drawn"] = drawn_members(framing, DRAWN_SEEDS)[:2]
    return images


@functools.lru_cache(maxsize=None)
def drawn_members(framing, seeds):
    """-> (image of one member a seed, text, features summed)"""
    wrap = dw.bgzf_member if framing == "bgzf" else dw.gzip_member
    images, texts, total = [], [], dict.fromkeys(dw.FEATURES, 0)
    for seed in seeds:
        raw, text, f = dw.drawn(seed)
        images.append(wrap(raw, text))
        texts.append(text)
        for k in f:
            total[k] += f[k]
    return b"".join(images), b"".join(texts), total


DRAWN_SEEDS = tuple(range(40))
WAVE_SEEDS = {64: tuple(range(6400, 6464)), 65: tuple(range(6500, 6565))}  # drawn members around the wave


# ---- bad streams -------------------------------------------------------------------------------------------------------
def _started(pre=True):
    s = Stream()
    if pre:
        s.fixed(0, list(PRE))
    return s


def _header_fields(hlit, hdist):
    s = _started()
    for v, n in ((1, 1), (2, 2), (hlit, 5), (hdist, 5), (15, 4)):
        s.w.put(v, n)
    return s


def _dyn(lit_lens, dist_lens, symbols=(), pre=True, **kw):
    """a final dynamic block whose symbols are given as ("lit", s), ("dist", s) or ("bits", value, width)"""
    s = _started(pre)
    lit, dist = s.dynamic_header(1, lit_lens, dist_lens, **kw)
    for x in symbols:
        if x[0] == "bits":
            s.w.put(x[1], x[2])
        else:
            s.w.code(*(lit if x[0] == "lit" else dist)[x[1]])
    return s


@functools.lru_cache(maxsize=None)
def bad_streams():
    """name -> (raw stream, text bytes in front of the token or block that fails): every one raises in zlib"""
    n = len(PRE)
    a_len_eob = balanced({97, 256, 257}, 258)
    out = {
        # 'a', length 3, then the bit pattern '1' of a distance code whose one code is '0'
        "one_dist_unassigned": (_dyn(a_len_eob, [1], (("lit", 97), ("lit", 257), ("bits", 1, 1), ("lit", 256))), n + 1),
        "match_no_dist": (_dyn(a_len_eob, [0], (("lit", 97), ("lit", 257), ("bits", 0, 8))), n + 1),
        "hlit_30": (_header_fields(30, 0), n), "hlit_31": (_header_fields(31, 0), n),
        "hdist_30": (_header_fields(0, 30), n), "hdist_31": (_header_fields(0, 31), n),
        "dist_over": (_dyn(balanced({97, 256}, 257), [1, 1, 1]), n),
        "dist_incomplete_2bit": (_dyn(balanced({97, 256}, 257), [2, 2]), n),
        "lit_single_not_eob": (_dyn(balanced({97}, 257), [0]), n),
    }
    s = _started()  # HCLEN = 4 and the four lengths zero
    for v, w in ((1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (0, 12)):
        s.w.put(v, w)
    out["cl_all_zero"] = (s, n)
    s = _started()  # 255 zeros, a one for symbol 255, then a 16 over 256, the one distance entry and one entry more
    dw.put_dynamic_header(s.w, 1, 0, 0, balanced({1, 16, 18}, 19), 18, [(18, 138), (18, 117), 1, (16, 3)])
    out["repeat_16_across_past_end"] = (s, n)
    s = _started()
    assert s.w.n == 2  # so the stored header is followed by three padding bits
    s.w.put(1, 3)
    s.w.align(0xff)
    s.w.raw(b"\x03\x00\xfc\xfe" + b"abc")
    out["stored_nlen"] = (s, n)
    # the same two distance failures with one literal in front and nothing else: under ISIZE 0 the literal crosses first
    out["one_dist_unassigned_first"] = (_dyn(a_len_eob, [1], (("lit", 97), ("lit", 257), ("bits", 1, 1), ("lit", 256)), pre=False), 1)
    out["match_no_dist_first"] = (_dyn(a_len_eob, [0], (("lit", 97), ("lit", 257), ("bits", 0, 8)), pre=False), 1)
    done = {}
    for name, (s, before) in out.items():
        s.w.put(0, 32)
        s.w.put(0, 32)
        s.w.align()
        done[name] = (dw.refused(bytes(s.w.out) + bytes(40)), before)
    return done


PRECEDENCE = ("one_dist_unassigned_isize0", "match_no_dist_isize0")


@functools.lru_cache(maxsize=None)
def foreign_bad(framing):
    """framing "bgzf" -> name -> (member, reason): the ISIZE holds the text up to the failure (and the match that fails), so
    SK_GZ_DEFLATE is the reason; the two of PRECEDENCE state ISIZE 0 with one literal in front of the failing match, and the
    literal is the token that crosses it: SK_GZ_LENGTH (include/sickle_amd.h: the first check to fail is the reason).
    framing "gzip" -> name -> (member, reason): the stream fails, whatever the trailer says."""
    out = {}
    for name, (raw, before) in bad_streams().items():
        if framing == "gzip":
            out[name] = (dw.gzip_member(raw, b"", isize=before), gm.DEFLATE)
        else:
            out[name] = (dw.bgzf_member(raw, b"", isize=before + 3), bm.DEFLATE)
            if name.endswith("_first"):
                out[name[:-6] + "_isize0"] = (dw.bgzf_member(raw, b"", isize=0), bm.LENGTH)
    return out


@functools.lru_cache(maxsize=None)
def bad_images(framing):
    """name -> image (BGZF) or (image, chunk) (plain gzip): each bad member at index 0, in the middle and last"""
    out = {}
    if framing == "bgzf":
        t = bm.texts()
        a, c = bm.member(t["fq"][:4000]), foreign_images("bgzf")["one_dist_3"][0]
        for name, (m, _) in foreign_bad("bgzf").items():
            out[name + "@0"] = m + a + c + bm.EOF
            out[name + "@1"] = a + m + c + bm.EOF
            out[name + "@last"] = a + c + m
    else:
        a, c = gm.small_blocks(fq(30000, 27)), foreign_images("gzip")["tiny_blocks_batch"][0]
        for name, (m, _) in foreign_bad("gzip").items():
            out[name + "@0"] = (m + a + c, 1024)
            out[name + "@1"] = (a + m + c, 1024)
            out[name + "@last"] = (a + c + m, 1024)
    return out


@functools.lru_cache(maxsize=None)
def bad_expected(framing):
    """name -> the model's verdict on bad_images(framing)[name]"""
    if framing == "bgzf":
        return {name: bm.bgunzip(image) for name, image in bad_images("bgzf").items()}
    return {name: gm.gunzip(image) for name, (image, chunk) in bad_images("gzip").items()}


def block_spans(image):
    """the bytes from each block's first byte to the first byte behind it (a member's last block: behind its trailer)"""
    res, blocks = gm.walk(image)
    starts = [b[0] for b in blocks] + [8 * len(image)]
    return [(b + 7) // 8 - a // 8 for a, b in zip(starts, starts[1:])]


@functools.lru_cache(maxsize=None)
def piece_stream(kind, name, window, grow=70000):
    """tests/gunzip_piece_model.py's stream() over valid("gzip")[name] (kind "valid") or bad_images("gzip")[name] ("bad"),
    computed once for the model's test, the host run's and the device's"""
    import gunzip_piece_model as pm
    image = valid("gzip")[name][0] if kind == "valid" else bad_images("gzip")[name][0]
    return pm.stream(image, window, grow)


@functools.lru_cache(maxsize=None)
def reencoded_fastq():
    """tests/golden/inputs/test.fastq through the drawn tokenizer and block cutter -> (text, BGZF image of members of
    30 000 bytes of text, one plain gzip member)"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs", "test.fastq"), "rb").read()
    members = [dw.bgzf_member(*dw.drawn(1000 + a, text[a:a + 30000])[:2]) for a in range(0, len(text), 30000)]
    raw, spelt, _ = dw.drawn(2000, text, one_bgzf_member=False)
    assert spelt == text
    return text, b"".join(members) + bm.EOF, dw.gzip_member(raw, text)
