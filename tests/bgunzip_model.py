"""The rules of sk_bgzf_inflate_device_async (include/sickle_amd.h) stated in Python, with zlib as the decoder: frame by
walking, zlib.decompressobj(-15) per member, the reason codes.  And the test images: member() builds any BGZF member zlib
can write, images() the valid ones the CPU harness and the GPU tests share, bad_images() the constructed bad ones.  Where
zlib refuses a stream, text_before_failure() (gunzip_model's inflate) tells whether ISIZE was crossed before the fault."""
import gzip
import struct
import zlib

import numpy as np

OK, HEADER, TRUNCATED, DEFLATE, LENGTH, CRC = range(6)
MAX_ISIZE = 65536
MIN_MEMBER = 26
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def frame(image, body, text, extra=b"", crc=None, isize=None):
    """A member around a raw deflate stream; extra: subfields ahead of BC."""
    x = extra + b"BC\x02\x00"
    size = 12 + len(x) + 2 + len(body) + 8
    assert size <= 65536
    return (image + b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", len(x) + 2) + x + struct.pack("<H", size - 1) + body +
            struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize))


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0, extra=b""):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    body = b""
    if flush_every:
        for a in range(0, len(text), flush_every):
            body += c.compress(text[a:a + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    else:
        body = c.compress(text)
    return frame(b"", body + c.flush(), text, extra)


def bgzip(text, block=65280, **kw):
    """text -> a BGZF image of members of `block` bytes, closed with the EOF member."""
    return b"".join(member(text[a:a + block], **kw) for a in range(0, len(text), block)) + EOF


def parse(image, pos):
    """-> (OK, size, body offset, body length, crc, isize) or (reason,)"""
    rem = len(image) - pos
    if image[pos:pos + 4] != b"\x1f\x8b\x08\x04"[:min(4, rem)]:
        return (HEADER,)
    if rem < MIN_MEMBER:
        return (TRUNCATED,)
    end = 12 + struct.unpack_from("<H", image, pos + 10)[0]
    if end > rem:
        return (TRUNCATED,)
    at, bsize = 12, None
    while at < end:
        if at + 4 > end:
            return (HEADER,)
        slen = struct.unpack_from("<H", image, pos + at + 2)[0]
        if at + 4 + slen > end:
            return (HEADER,)
        if bsize is None and image[pos + at:pos + at + 2] == b"BC" and slen == 2:
            bsize = struct.unpack_from("<H", image, pos + at + 4)[0]
        at += 4 + slen
    if bsize is None or bsize + 1 < end + 8:
        return (HEADER,)
    if bsize + 1 > rem:
        return (TRUNCATED,)
    crc, isize = struct.unpack_from("<II", image, pos + bsize + 1 - 8)
    return OK, bsize + 1, end, bsize + 1 - end - 8, crc, isize


def decode(body, crc, isize):
    """-> (reason, text)"""
    if isize > MAX_ISIZE:
        return LENGTH, b""
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(body, isize + 1)
    except zlib.error:
        # zlib was let one byte beyond ISIZE and, with that byte out, reads on to the next token's codes; if the fault lies
        # there, the byte beyond ISIZE came first, and the first check to fail is the member's reason
        return (LENGTH if text_before_failure(body) > isize else DEFLATE), b""
    if len(text) > isize:
        return LENGTH, b""
    if not d.eof:
        # zlib stops when the text is full; what follows may still be an end-of-block code, empty blocks, or more text
        try:
            more = d.decompress(d.unconsumed_tail, 1)
        except zlib.error:
            return DEFLATE, b""
        if more:
            return LENGTH, b""
        if not d.eof:
            return DEFLATE, b""
    if len(text) < isize:
        return LENGTH, b""
    if zlib.crc32(text) != crc:
        return CRC, b""
    return OK, text


def text_before_failure(body):
    """The text bytes in front of the token or block header a raw stream fails at (zlib tells that it fails, not where):
    gunzip_model's block-by-block inflate, which appends the text token by token and raises at the fault."""
    import gunzip_model as gm

    class Far(list):  # block() sets far[0] just before it appends the copy of a distance beyond the text
        at = None

        def __setitem__(self, i, v):
            if self.at is None:
                self.at = len(out)

    out, r, far = bytearray(), gm.Reader(body, 0), Far([False])
    try:
        final = 0
        while not final and far.at is None:
            final = gm.block(r, out, 0, far)[1]
    except gm.Bad:
        pass
    return len(out) if far.at is None else far.at


def bgunzip(image):
    """-> dict(error, error_member, error_offset, members, bytes_out, text); text is None after an error"""
    pos, table, err = 0, [], None
    while pos < len(image):
        p = parse(image, pos)
        if p[0] != OK:
            err = (p[0], len(table), pos)
            break
        table.append((pos,) + p[1:])
        pos += p[1]
    need = sum(m[5] for m in table if m[5] <= MAX_ISIZE)
    texts = []
    for k, (off, size, boff, blen, crc, isize) in enumerate(table):
        why, text = decode(image[off + boff:off + boff + blen], crc, isize)
        if why != OK:
            err = (why, k, off)
            break
        texts.append(text)
    e = err or (OK, 0, 0)
    return dict(error=e[0], error_member=e[1], error_offset=e[2], members=len(table), bytes_out=need,
                text=None if err else b"".join(texts))


# ---- the images ----------------------------------------------------------------------------------------------------
def chain_text(n_matches=70):
    """A text whose every match copies the match before it: 24 fresh bytes, then each round repeats the last 12 bytes
    (a match that reads what the match before wrote) and adds one fresh byte, so a batch of 64 tokens resolves one match
    per round."""
    rng = np.random.default_rng(11)
    out = bytearray(rng.integers(0, 256, 24, dtype=np.uint8).tobytes())
    for _ in range(n_matches):
        out += out[-12:]
        out.append(int(rng.integers(0, 256)))
    return bytes(out)


def texts():
    rng = np.random.default_rng(7)
    rnd = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
    acgt = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 30000).tobytes()
    fq = b"".join(b"@read%d\n%s\n+\n%s\n" % (i, rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), 100).tobytes(),
                                          rng.integers(35, 74, 100, dtype=np.uint8).tobytes()) for i in range(250))
    half = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    return dict(rnd=rnd, acgt=acgt, fq=fq, half=half)


def images():
    """name -> (image, text): every kind of member zlib writes, singly and (as "all") in one image."""
    t = texts()
    rnd, acgt, fq, half = t["rnd"], t["acgt"], t["fq"], t["half"]
    m = {
        "stored0": (member(fq, 0), fq),
        "stored_random": (member(rnd, 6), rnd),
        "fixed": (member(fq[:20000], 6, zlib.Z_FIXED), fq[:20000]),
        "level1": (member(fq, 1), fq),
        "level6": (member(fq, 6), fq),
        "level9": (member(fq + acgt[:10000], 9), fq + acgt[:10000]),
        "huffman_only": (member(acgt, 6, zlib.Z_HUFFMAN_ONLY), acgt),
        "rle": (member(b"".join(bytes([65 + i % 7]) * (1 + i % 40) for i in range(2000)), 6, zlib.Z_RLE),
                b"".join(bytes([65 + i % 7]) * (1 + i % 40) for i in range(2000))),
        "multi_block": (member(fq, 6, flush_every=1000), fq),
        "extra_first": (member(fq[:5000], 6, extra=b"XY\x03\x00abc" + b"BC\x01\x00z"), fq[:5000]),
        "one_byte": (member(b"x"), b"x"),
        "full": (member(b"A" * 65536), b"A" * 65536),
        "full_text": (member((fq * 2)[:65536], 9), (fq * 2)[:65536]),
        "far": (far_member(half), half + half),
        "chain": (member(chain_text(), 9), chain_text()),
        "chain_fixed": (member(chain_text(), 9, zlib.Z_FIXED), chain_text()),
        "eof_only": (EOF, b""),
        "fq_head": (member(fq[:3000]), fq[:3000]),
    }
    assert len(m["stored_random"][0]) == 65280 + 5 + 26 + 5  # two stored blocks
    for d in list(range(1, 65)) + [255, 256, 257, 258, 259]:
        text = (rng_period(d) * (3000 // d + 2))[:3000 + d]
        m["period%d" % d] = (member(text, 9), text)
    m["empties"] = (EOF + member(b"abc") + EOF + member(fq[:3000], 1) + EOF + EOF, b"abc" + fq[:3000])
    m["all"] = (b"".join(v[0] for v in m.values()), b"".join(v[1] for v in m.values()))
    return m


def far_member(half):
    """32 768 bytes stored, then the same again as copies from exactly 32 768 back (zlib's own matches stop at 32 506):
    126 of length 258 and two of length 130, in one fixed block."""
    assert len(half) == 32768
    rev = lambda code, n: (int(format(code, "0%db" % n)[::-1], 2), n)
    far = [rev(29, 5), (32768 - 24577, 13)]
    fields = [(1, 1), (1, 2)] + ([rev(0xc5, 8)] + far) * 126 + ([rev(0xc0, 8), (130 - 115, 4)] + far) * 2 + [(0, 7)]
    return frame(b"", b"\x00\x00\x80\xff\x7f" + half + bits(*fields), half + half)


def rng_period(d):
    return np.random.default_rng(100 + d).integers(0, 256, d, dtype=np.uint8).tobytes()


def small_members(count, seed=3):
    """count members of 1 to 40 bytes of text -> (image, text)"""
    rng = np.random.default_rng(seed)
    parts = [rng.integers(65, 91, int(rng.integers(1, 41)), dtype=np.uint8).tobytes() for _ in range(count)]
    return b"".join(member(p, int(rng.integers(0, 10))) for p in parts), b"".join(parts)


def bits(*fields):
    """(value, width) fields, LSB first -> bytes"""
    v = n = 0
    for val, width in fields:
        v |= val << n
        n += width
    return v.to_bytes((n + 7) // 8, "little")


def bad_members():
    """name -> (member, reason): one bad member each, built by hand"""
    good = b"hello, hello, hello, hello\n"
    ok = member(good)
    body = ok[18:-8]
    huff = lambda code, n: (int(format(code, "0%db" % n)[::-1], 2), n)  # a Huffman code goes out first bit first
    # a dynamic header: HLIT, HDIST, HCLEN = 19, then the code-length code's lengths in transmission order
    dyn = lambda cl, rest, hlit=0, hdist=0: bits((1, 1), (2, 2), (hlit, 5), (hdist, 5), (15, 4), *[(c, 3) for c in cl], *rest)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl_of = lambda d: [d.get(s, 0) for s in order]
    b = {
        "block_type_3": (frame(b"", bits((1, 1), (3, 2)) + b"\0", b""), DEFLATE),
        "stored_nlen": (frame(b"", b"\x01\x03\x00\xfc\xfe" + b"abc", b"abc"), DEFLATE),
        "stored_beyond_body": (frame(b"", b"\x01\x05\x00\xfa\xff" + b"abc", b"abcde"), DEFLATE),
        "no_bits": (frame(b"", b"", b""), DEFLATE),
        "cut_stream": (frame(b"", body[:-3], good), DEFLATE),
        # fixed block: literal 'a' (0x30 + 0x61 = 8 bits), then length symbol 286 (1100 0110) / distance symbol 30
        "length_286": (frame(b"", bits((1, 1), (1, 2), huff(0x30 + 97, 8), huff(0xc0 + 6, 8), (0, 16)), b"a"), DEFLATE),
        "distance_30": (frame(b"", bits((1, 1), (1, 2), huff(0x30 + 97, 8), huff(1, 7), huff(30, 5), (0, 16)), b"aaaa"), DEFLATE),
        "distance_too_far": (frame(b"", bits((1, 1), (1, 2), huff(0x30 + 97, 8), huff(1, 7), huff(1, 5), huff(0, 7)), b"aaaa"), DEFLATE),
        # code-length code over-subscribed (three codes of one bit) and incomplete (one code of one bit)
        "cl_over": (frame(b"", dyn(cl_of({0: 1, 1: 1, 2: 1}), [(0, 32)]), b""), DEFLATE),
        "cl_incomplete": (frame(b"", dyn(cl_of({0: 1}), [(0, 32)]), b""), DEFLATE),
        # code-length code {0: 1 bit '0', 16: 2 bits '10', 18: 2 bits '11'}: a repeat of the length before as first symbol
        "repeat_first": (frame(b"", dyn(cl_of({0: 1, 18: 2, 16: 2}), [huff(2, 2), (0, 2), (0, 32)]), b""), DEFLATE),
        # 18 with 138 zeros twice = 276 > 257 + 1
        "repeat_past_end": (frame(b"", dyn(cl_of({0: 1, 18: 2, 16: 2}), [huff(3, 2), (127, 7), huff(3, 2), (127, 7), (0, 32)]), b""), DEFLATE),
        # all 258 lengths zero: no end-of-block code
        "no_end_of_block": (frame(b"", dyn(cl_of({0: 1, 18: 2, 16: 2}), [huff(3, 2), (127, 7), huff(3, 2), (109, 7), (0, 32)]), b""), DEFLATE),
        "isize_short": (frame(b"", body, good, isize=len(good) - 1, crc=zlib.crc32(good[:-1])), LENGTH),
        "isize_long": (frame(b"", body, good, isize=len(good) + 1), LENGTH),
        "isize_huge": (frame(b"", body, good, isize=65537), LENGTH),
        "crc": (frame(b"", body, good, crc=zlib.crc32(good) ^ 1), CRC),
        "flipped_text": (frame(b"", b"\x01\x03\x00\xfc\xff" + b"abd", b"abc"), CRC),
        "flg_8": (ok[:3] + b"\x0c" + ok[4:], HEADER),
        "not_deflate": (ok[:2] + b"\x07" + ok[3:], HEADER),
        "no_bc": (ok[:12] + b"BD" + ok[14:], HEADER),
        "subfield_overrun": (ok[:14] + b"\x03" + ok[15:], HEADER),
        "bsize_small": (ok[:16] + struct.pack("<H", 24) + ok[18:], HEADER),
    }
    # lit/len code over-subscribed: lengths of one bit for symbols 0, 1, 2 through the code-length code {1: 1 bit, 18: 1 bit}
    over = dyn(cl_of({1: 1, 18: 1}), [(0, 1), (0, 1), (0, 1), (1, 1), (127, 7), (1, 1), (106, 7), (0, 32)])
    b["lit_over"] = (frame(b"", over, b""), DEFLATE)
    # lit/len code incomplete: symbols 0 and 256 get lengths 2 and 2 (Kraft 1/2), the distance code one length of 1 (allowed)
    cl = cl_of({1: 2, 2: 2, 18: 1})  # 18: '0'; 1: '10'; 2: '11'
    inc = dyn(cl, [huff(3, 2), (0, 1), (127, 7), (0, 1), (106, 7), huff(3, 2), huff(2, 2), (0, 32)])
    b["lit_incomplete"] = (frame(b"", inc, b""), DEFLATE)
    return b


def bad_images():
    """name -> image: each bad member at index 0, in the middle and last; two bad members; framing damage.  The expected
    verdict is the model's (asserted reason by reason in tests/test_bgunzip_model.py)."""
    t = texts()
    a, c = member(t["fq"][:4000]), member(t["acgt"][:3000], 9)
    out = {}
    for name, (m, _) in bad_members().items():
        out[name + "@0"] = m + a + c + EOF
        out[name + "@1"] = a + m + c + EOF
        out[name + "@last"] = a + c + m
    bm = bad_members()
    out["two_bad"] = a + bm["crc"][0] + c + bm["block_type_3"][0] + EOF
    out["bad_then_garbage"] = a + bm["isize_long"][0] + b"garbage"
    out["plain_gzip"] = gzip.compress(t["fq"], 6)
    out["garbage_after"] = a + c + EOF + b"\0" * 40
    out["short_garbage_after"] = a + EOF + b"xyz"
    out["cut_one_short"] = (a + c + EOF)[:-1]
    out["cut_in_header"] = a + c[:10]
    out["cut_magic"] = a + c[:2]
    out["cut_in_extra"] = a + member(b"abc", extra=b"XY\x28\x00" + b"q" * 40)[:30]
    return out
