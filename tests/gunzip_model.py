"""The rules of sk_gzip_inflate_device_async (include/sickle_amd.h) stated in Python: the gzip header, a small inflate that
walks the stream block by block (so it knows every block's first bit, which zlib does not tell), the reason codes and
their order.  zlib is the decoder every valid text is held against (gunzip() asserts it).  And the test images: small_blocks()
draws gzip whose blocks hold a few hundred symbols, images() the valid ones the CPU harness and the GPU tests share,
bad_images() the damaged ones, long_images() and long_bad_images() those beyond 16 MiB of image, beyond the guess's text
cap and with thousands of members.  crc_shift() and crc_combine() are the CRC-32 algebra of the device's member check on
Python integers."""
import functools
import gzip
import struct
import zlib

import numpy as np

OK, HEADER, TRUNCATED, DEFLATE, LENGTH, CRC = range(6)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


class Bad(Exception):
    pass


def parse_header(image, pos):
    """-> (OK, offset of the deflate stream) or (reason,)"""
    rem = len(image) - pos
    if image[pos:pos + 3] != b"\x1f\x8b\x08"[:min(3, rem)]:
        return (HEADER,)
    if rem < 10:
        return (TRUNCATED,)
    flg = image[pos + 3]
    if flg & 0xe0:
        return (HEADER,)
    at = 10
    if flg & 4:
        if at + 2 > rem:
            return (TRUNCATED,)
        at += 2 + struct.unpack_from("<H", image, pos + at)[0]
        if at > rem:
            return (TRUNCATED,)
    for bit in (8, 16):
        if flg & bit:
            z = image.find(b"\0", pos + at)
            if z < 0:
                return (TRUNCATED,)
            at = z - pos + 1
    if flg & 2:
        at += 2
    if at > rem:
        return (TRUNCATED,)
    return OK, pos + at


class Code:
    """A canonical Huffman code, accepted and refused as zlib does; decode() goes bit by bit over count[] as the device's
    slow path does."""

    def __init__(self, lens, is_cl=False):
        self.count = [0] * 16
        for l in lens:
            self.count[l] += 1
        self.count[0] = 0
        left, mx = 1, 0
        for l in range(1, 16):
            left = (left << 1) - self.count[l]
            if left < 0:
                raise Bad("over-subscribed")
            if self.count[l]:
                mx = l
        if mx and left > 0 and (is_cl or mx != 1):
            raise Bad("incomplete")
        self.sorted = [s for l in range(1, 16) for s, x in enumerate(lens) if x == l]

    def decode(self, r):
        v = r.peek(15)
        code = first = index = 0
        for l in range(1, 16):
            code |= (v >> (l - 1)) & 1
            c = self.count[l]
            if code - c < first:
                r.skip(l)
                return self.sorted[index + code - first]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise Bad("no symbol")


class Reader:
    def __init__(self, data, bit):
        self.data, self.bit, self.end = data, bit, 8 * len(data)

    def peek(self, k):
        at = self.bit >> 3
        return (int.from_bytes(self.data[at:at + 8], "little") >> (self.bit & 7)) & ((1 << k) - 1)

    def skip(self, k):
        self.bit += k
        if self.bit > self.end:
            raise Bad("bits beyond the image")

    def take(self, k):
        v = self.peek(k)
        self.skip(k)
        return v


@functools.lru_cache(maxsize=None)
def _fixed():
    return Code([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), Code([5] * 32)


def block(r, out, floor, far):
    """One block from r.bit on; text appended to out (a bytearray).  A distance that reaches before out[floor] appends
    zeros and sets far[0].  -> (type, final)"""
    final = r.take(1)
    kind = r.take(2)
    if kind == 0:
        r.skip(-r.bit % 8)
        v = r.take(32)
        n = v & 0xffff
        if n != (~v >> 16) & 0xffff:
            raise Bad("stored lengths")
        at = r.bit >> 3
        if at + n > len(r.data):
            raise Bad("stored beyond the image")
        out += r.data[at:at + n]
        r.bit += 8 * n
        return kind, final
    if kind == 3:
        raise Bad("block type 3")
    if kind == 1:
        lit, dist = _fixed()
    else:
        nlen, ndist, ncl = 257 + r.take(5), 1 + r.take(5), 4 + r.take(4)
        if nlen > 286 or ndist > 30:
            raise Bad("too many codes")
        cl = [0] * 19
        for i in range(ncl):
            cl[CL_ORDER[i]] = r.take(3)
        clc = Code(cl, True)
        lens = []
        while len(lens) < nlen + ndist:
            s = clc.decode(r)
            if s < 16:
                lens.append(s)
                continue
            if s == 16:
                if not lens:
                    raise Bad("repeat of nothing")
                rep, v = 3 + r.take(2), lens[-1]
            elif s == 17:
                rep, v = 3 + r.take(3), 0
            else:
                rep, v = 11 + r.take(7), 0
            if len(lens) + rep > nlen + ndist:
                raise Bad("repeat past the end")
            lens += [v] * rep
        if lens[256] == 0:
            raise Bad("no end-of-block code")
        lit, dist = Code(lens[:nlen]), Code(lens[nlen:])
    while True:
        s = lit.decode(r)
        if s < 256:
            out.append(s)
            continue
        if s == 256:
            return kind, final
        s -= 257
        if s >= 29:
            raise Bad("length symbol")
        n = LEN_BASE[s] + r.take(LEN_EXTRA[s])
        d = dist.decode(r)
        if d >= 30:
            raise Bad("distance symbol")
        d = DIST_BASE[d] + r.take(DIST_EXTRA[d])
        if d > len(out) - floor:
            far[0] = True
            out += bytes(n)
        elif d >= n:
            out += out[len(out) - d:len(out) - d + n]
        else:  # the copy overlaps itself: its d bytes repeat
            out += (bytes(out[len(out) - d:]) * (n // d + 1))[:n]


def walk(image, lengths=None):
    """The whole image -> (result dict, blocks): blocks is the list of (first bit, type, final, member) of every block that
    decoded; a list given as `lengths` gets the text bytes of each of them.  The failures: a header or truncation error or
    a block that does not decode stops the walk; a distance before the member's first byte, a length unlike ISIZE and a
    CRC-32 unlike the trailer's are noted and the walk goes on.  The lowest (member, reason number) wins, for two of one
    member and reason the lower offset."""
    n, pos, member = len(image), 0, 0
    out, blocks, errors = bytearray(), [], []
    while pos < n:
        h = parse_header(image, pos)
        if h[0] != OK:
            errors.append((member, h[0], pos))
            break
        r, floor, far_seen, stop = Reader(image, 8 * h[1]), len(out), False, False
        while True:
            b, far, before = r.bit, [False], len(out)
            try:
                kind, final = block(r, out, floor, far)
            except Bad:
                errors.append((member, DEFLATE, b >> 3))
                stop = True
                break
            finally:
                if far[0] and not far_seen:
                    far_seen = True
                    errors.append((member, DEFLATE, b >> 3))
            blocks.append((b, kind, final, member))
            if lengths is not None:
                lengths.append(len(out) - before)
            if final:
                break
        if stop:
            break
        at = (r.bit + 7) >> 3
        if n - at < 8:
            errors.append((member, TRUNCATED, pos))
            break
        crc, isize = struct.unpack_from("<II", image, at)
        text = bytes(out[floor:])
        if len(text) & 0xffffffff != isize:
            errors.append((member, LENGTH, pos))
        elif zlib.crc32(text) != crc:
            errors.append((member, CRC, pos))
        member += 1
        pos = at + 8
    e = min(errors) if errors else None
    res = dict(error=e[1] if e else 0, error_member=e[0] if e else 0, error_offset=e[2] if e else 0, members=member,
               bytes_out=len(out), text=None if e else bytes(out))
    return res, blocks


def gunzip(image):
    """-> dict(error, error_member, error_offset, members, bytes_out, text); text is None after an error.  A valid image's
    text is zlib's."""
    res = walk(image)[0]
    if res["error"] == 0:
        assert res["text"] == (gzip.decompress(image) if image else b"")
    return res


def dynamic_chunks(image, chunk):
    """The chunks 1.. of `chunk` bytes in which a non-final dynamic block begins"""
    return sorted({b // (8 * chunk) for b, kind, final, _ in walk(image)[1] if kind == 2 and not final and b // (8 * chunk) > 0})


# ---- the images ----------------------------------------------------------------------------------------------------
def fastq_text(n_bytes, seed=5):
    rng = np.random.default_rng(seed)
    acgt, out, i = np.frombuffer(b"ACGTN", dtype=np.uint8), [], 0
    size = 0
    while size < n_bytes:
        rec = b"@read%d/%d\n%s\n+\n%s\n" % (i, seed, rng.choice(acgt, 100, p=[.3, .2, .2, .29, .01]).tobytes(),
                                       rng.integers(35, 74, 100, dtype=np.uint8).tobytes())
        out.append(rec)
        size += len(rec)
        i += 1
    return b"".join(out)[:n_bytes]


def small_blocks(text, level=6, mem_level=1):
    """gzip with small blocks: memLevel 1 ends a block every 128 symbols or so, and most of them are dynamic"""
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem_level)
    return c.compress(text) + c.flush()


def header(flags=0, extra=b"", name=b"", comment=b"", hcrc=False):
    h = bytearray(b"\x1f\x8b\x08\0\0\0\0\0\0\xff")
    if extra:
        h[3] |= 4
        h += struct.pack("<H", len(extra)) + extra
    if name:
        h[3] |= 8
        h += name + b"\0"
    if comment:
        h[3] |= 16
        h += comment + b"\0"
    if hcrc:
        h[3] |= 2
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xffff)
    h[3] |= flags
    return bytes(h)


def member(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flush_every=0, head=None, crc=None, isize=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    body = b""
    if flush_every:
        for a in range(0, len(text), flush_every):
            body += c.compress(text[a:a + flush_every]) + c.flush(zlib.Z_FULL_FLUSH)
    else:
        body = c.compress(text)
    body += c.flush()
    return (header() if head is None else head) + body + struct.pack(
        "<II", zlib.crc32(text) if crc is None else crc, len(text) & 0xffffffff if isize is None else isize)


@functools.lru_cache(maxsize=None)
def texts():
    rng = np.random.default_rng(7)
    fq = fastq_text(60000)
    period = rng.integers(0, 256, 32500, dtype=np.uint8).tobytes()
    return dict(fq=fq, rnd=rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(),
                acgt=rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 30000).tobytes(),
                far=fastq_text(3000, 9) + period * 8,  # matches that reach the far end of the unknown window
                run=fastq_text(5000, 10) + b"A" * 150000 + fastq_text(5000, 11))  # a self-overlapping copy across stretch starts


@functools.lru_cache(maxsize=None)
def images():
    """name -> (image, text): every kind of member, headers of every shape"""
    t = texts()
    fq, rnd, acgt = t["fq"], t["rnd"], t["acgt"]
    m = {
        "stored0": (member(fq, 0), fq),
        "stored_random": (member(rnd, 6), rnd),
        "fixed": (member(fq[:20000], 6, zlib.Z_FIXED), fq[:20000]),
        "level1": (member(fq, 1), fq),
        "level6": (member(fq, 6), fq),
        "level9": (member(fq + acgt[:10000], 9), fq + acgt[:10000]),
        "huffman_only": (member(acgt, 6, zlib.Z_HUFFMAN_ONLY), acgt),
        "multi_block": (member(fq, 6, flush_every=1000), fq),
        "mixed": (member(fq[:9000] + rnd[:9000] + fq[:9000], 6, mem_level=2), fq[:9000] + rnd[:9000] + fq[:9000]),
        "empty_text": (member(b""), b""),
        "one_byte": (member(b"x"), b"x"),
        "py_gzip": (gzip.compress(fq, 6), fq),
        "fextra": (member(fq[:5000], head=header(extra=b"XY\x03\x00abc")), fq[:5000]),
        "fname": (member(fq[:5000], head=header(name=b"reads.fastq")), fq[:5000]),
        "fcomment": (member(fq[:5000], head=header(comment=b"a comment")), fq[:5000]),
        "fhcrc": (member(fq[:5000], head=header(hcrc=True)), fq[:5000]),
        "all_fields": (member(fq[:5000], head=header(extra=b"AB\x01\x00z", name=b"n", comment=b"c", hcrc=True)), fq[:5000]),
        "bgzf_like": (member(fq[:3000], head=header(extra=b"BC\x02\x00\xff\xff")), fq[:3000]),
    }
    m["two"] = (m["level6"][0] + m["fname"][0], fq + fq[:5000])
    return m


@functools.lru_cache(maxsize=None)
def stretch_images():
    """name -> (image, text, chunk): images of many small dynamic blocks, to be read with SK_GZIP_CHUNK = chunk"""
    t = texts()
    out = {}
    for kib, chunk in ((48, 4096), (48, 1024), (48, 256), (200, 4096), (200, 1024), (200, 256)):
        text = fastq_text(kib * 1024, seed=kib)
        out["fq%dk_c%d" % (kib, chunk)] = (small_blocks(text), text, chunk)
    for want in (63, 64, 65):  # around the wave: the text's length is searched until the image has this many chunks
        lo, hi = 40000, 400000
        while True:
            mid = (lo + hi) // 2
            image = small_blocks(fastq_text(mid, seed=63))
            got = -(-len(image) // 1024)
            if got == want:
                break
            lo, hi = (mid, hi) if got < want else (lo, mid)
        out["s%d_c1024" % want] = (image, fastq_text(mid, seed=63), 1024)
    out["far_c256"] = (small_blocks(t["far"], 9), t["far"], 256)
    out["run_c256"] = (small_blocks(t["run"]), t["run"], 256)
    # a stretch whose whole text is shorter than 32 KiB between two others: every stretch of a 256-byte chunk is
    short = fastq_text(90000, 12)
    out["short_c256"] = (small_blocks(short, 9), short, 256)
    # members: an end inside a stretch, many members, an end exactly on a chunk boundary
    a, b = small_blocks(fastq_text(20000, 13)), small_blocks(fastq_text(30000, 14))
    out["two_members_c1024"] = (a + b, fastq_text(20000, 13) + fastq_text(30000, 14), 1024)
    pad = header(name=b"x" * ((-len(a) - 2) % 1024 + 1))  # the second member's header then begins on a chunk boundary
    first = member(fastq_text(20000, 13), mem_level=1, head=pad)
    assert len(first) % 1024 == 0
    out["member_on_boundary_c1024"] = (first + b, fastq_text(20000, 13) + fastq_text(30000, 14), 1024)
    for count in (65, 300):
        parts = [fastq_text(150 + 7 * (i % 40), 100 + i) for i in range(count)]
        out["members%d_c1024" % count] = (b"".join(small_blocks(p, 1 + i % 9) for i, p in enumerate(parts)), b"".join(parts), 1024)
    return out


def bits(*fields):
    v = n = 0
    for val, width in fields:
        v |= val << n
        n += width
    return v.to_bytes((n + 7) // 8, "little")


def far_member():
    """a fixed block: literal 'a', then a match of length 3 from distance 2: one byte before the member's first"""
    huff = lambda code, n: (int(format(code, "0%db" % n)[::-1], 2), n)
    body = bits((1, 1), (1, 2), huff(0x30 + 97, 8), huff(1, 7), huff(1, 5), huff(0, 7))
    return header() + body + struct.pack("<II", zlib.crc32(b"aaaa"), 4)


def damage(good, where):
    """The damaged versions of a valid image whose member `where` (0 = the first) takes the damage -> name -> image.
    good: list of members; the damage goes to good[where]."""
    pre, m, post = b"".join(good[:where]), good[where], b"".join(good[where + 1:])
    body_at = parse_header(m, 0)[1]
    w = lambda x: pre + x + post
    flip = lambda at, bit=0: m[:at] + bytes([m[at] ^ (1 << bit)]) + m[at + 1:]
    out = {
        "magic": w(b"\x1f\x8c" + m[2:]),
        "cm": w(m[:2] + b"\x07" + m[3:]),
        "reserved_flag": w(m[:3] + bytes([m[3] | 0x20]) + m[4:]),
        "trailing_byte": pre + m + post + b"\x01",
        "cut_header": pre + m[:6],
        "cut_body": pre + m[:body_at + (len(m) - body_at) // 2],
        "cut_trailer": pre + m[:-3],
        "dynamic_header": w(flip(body_at + 1, 1)),
        "far": w(far_member()),
        "isize": w(m[:-4] + struct.pack("<I", (struct.unpack("<I", m[-4:])[0] + 1) & 0xffffffff)),
        "text_bit": w(flip(body_at + (len(m) - body_at) * 2 // 3, 3)),
        "crc": w(m[:-8] + bytes([m[-8] ^ 1]) + m[-7:]),
    }
    return out


@functools.lru_cache(maxsize=None)
def bad_images():
    """name -> (image, chunk): each damage at member 0 and at a member that starts in a later stretch"""
    t = texts()
    a, b, c = small_blocks(fastq_text(30000, 21)), small_blocks(fastq_text(30000, 22), 9), small_blocks(t["acgt"][:9000])
    out = {}
    for where in (0, 1):
        for name, image in damage([a, b, c], where).items():
            out["%s@%d" % (name, where)] = (image, 1024)
    out["garbage"] = (bytes(range(256)) * 8, 256)
    out["crc_then_header"] = (a[:-8] + bytes([a[-8] ^ 1]) + a[-7:] + b"\x1f\x8b\x07" + b[3:], 1024)
    return out


@functools.lru_cache(maxsize=None)
def big_images():
    """name -> (image, text, chunk): a few hundred stretches, and one member whose CRC-32 is combined over many pieces"""
    mib = fastq_text(1 << 20, 31)
    five = fastq_text(5 << 20, 32)
    small = small_blocks(mib)
    return {"fq1m_c4096": (small, mib, 4096), "fq1m_c1024": (small, mib, 1024), "fq1m_c256": (small, mib, 256),
            "fq5m_gzip1": (gzip.compress(five, 1), five, 0)}


# ---- CRC-32 algebra: polynomials over GF(2) modulo the CRC-32 polynomial, reflected (bit 31 is x^0) --------------------
POLY = 0xedb88320


def _mul(a, b):
    """a * b modulo the polynomial"""
    p = 0
    for i in range(31, -1, -1):  # a's coefficient of x^(31 - i)
        if (a >> i) & 1:
            p ^= b
        b = (b >> 1) ^ POLY if b & 1 else b >> 1  # b * x
    return p


def crc_shift(k):
    """x^(8 k) modulo the polynomial (1 is 0x80000000): what appending k bytes multiplies a CRC register by"""
    r, p = 0x80000000, 0x00800000
    while k:
        if k & 1:
            r = _mul(r, p)
        p = _mul(p, p)
        k >>= 1
    return r


def crc_combine(crc_a, crc_b, len_b):
    """zlib.crc32(a + b) from zlib.crc32(a), zlib.crc32(b) and len(b)"""
    return _mul(crc_shift(len_b), crc_a) ^ crc_b


# ---- the long images -----------------------------------------------------------------------------------------------
def spliced_member(parts, head=None):
    """One member of parts (text, level, strategy, mem_level): each its own raw deflate stream, all but the last ended by a
    full flush (an empty stored block, behind which the next starts on a byte and with an empty window)"""
    body = []
    for i, (t, level, strategy, mem_level) in enumerate(parts):
        c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
        body.append(c.compress(t) + (c.flush(zlib.Z_FULL_FLUSH) if i + 1 < len(parts) else c.flush()))
    text = b"".join(p[0] for p in parts)
    image = (header() if head is None else head) + b"".join(body) + struct.pack("<II", zlib.crc32(text), len(text) & 0xffffffff)
    assert gzip.decompress(image) == text
    return image


PAST16M_D = dict(zip("abcdefgh", (0, 1, 2, 3, 5, 8, 11, 15)))  # the stored run's length is (1 << 24) - 70000 + d
LONG_RUN = 13 << 20


@functools.lru_cache(maxsize=None)
def long_images():
    """name -> (image, text, chunk); chunk 0 is the default.  The texts are zlib's (asserted here)."""
    rng = np.random.default_rng(16)
    rnd = rng.integers(0, 256, 17 << 20, dtype=np.uint8).tobytes()
    out = {}
    tail = [(fastq_text(300000, 41), 6, 0, 1), (fastq_text(50000, 42), 6, zlib.Z_FIXED, 8), (rnd[-200000:], 0, 0, 8),
            (fastq_text(300000, 43), 9, 0, 1)]
    for letter, d in PAST16M_D.items():  # the bit reader's base moves inside the small dynamic blocks, at 8 alignments
        parts = [(rnd[d:d + (1 << 24) - 70000 + d], 0, 0, 8)] + tail
        out["past16m_" + letter] = (spliced_member(parts), b"".join(p[0] for p in parts), 1 << 25)
    out["past16m_d_default"] = out["past16m_d"][:2] + (0,)
    out["past16m_stored"] = (member(rnd, 0), rnd, 0)
    fq = fastq_text(26 << 20, 44)
    out["past16m_fixed"] = (member(fq, 6, zlib.Z_FIXED), fq, 0)
    assert len(out["past16m_fixed"][0]) > 17 << 20
    for mem_level in (8, 7):  # blocks of 16 383 and of 8 191 copies of 258 bytes: beyond the guess's text cap, and within
        text = fastq_text(5000, 45) + b"A" * LONG_RUN + fastq_text(5000, 46)
        image = member(text, 9, mem_level=mem_level)
        over = long_blocks(image)
        assert bool(over) == (mem_level == 8), (mem_level, over)
        out["long_run_m%d" % mem_level] = (image, text, 256)
    parts, texts, i = [member(b"")], [b""], 0
    while len(parts) < 5900:  # runs of 1, 2, 63, 64 and 65 empty members between members of one byte and of 200
        run = (1, 2, 63, 64, 65)[i % 5]
        t = bytes([65 + i % 26]) if i % 2 else fastq_text(200, 300 + i)
        parts += [member(b"")] * run + [member(t, mem_level=1)]
        texts.append(t)
        i += 1
    parts += [member(b"")] * (6000 - len(parts))
    image, text = b"".join(parts), b"".join(texts)
    assert gzip.decompress(image) == text
    out["empty_members_c256"] = (image, text, 256)
    out["empty_members"] = (image, text, 0)
    for name, (image, text, chunk) in out.items():
        assert name.startswith("past16m") == (len(image) > 1 << 24), name
    return out


def long_blocks(image):
    """The (first bit, text bytes) of the non-final dynamic blocks that hold more than 4 MiB of text"""
    lengths = []
    blocks = walk(image, lengths)[1]
    return [(b[0], n) for b, n in zip(blocks, lengths) if b[1] == 2 and not b[2] and n > 4 << 20]


LONG_MEMBERS = {"empty_members": 6000, "empty_members_c256": 6000}


def long_want(name):
    """What gunzip() says of long_images()[name], without the walk: its text is zlib's and its members are counted"""
    image, text, _ = long_images()[name]
    return dict(error=0, error_member=0, error_offset=0, members=LONG_MEMBERS.get(name, 1), bytes_out=len(text), text=text)


@functools.lru_cache(maxsize=None)
def long_bad_images():
    """name -> (image, chunk, gunzip(image)): past16m_a with a bit flipped in a dynamic block beyond byte 2^24, with a
    damaged CRC-32 and cut short"""
    image = long_images()["past16m_a"][0]
    at = next(b[0] for b in walk(image)[1] if b[0] > 8 * ((1 << 24) + 4096) and b[1] == 2) // 8 + 40
    assert 1 << 24 < at < len(image) - 400000  # in the level 6 part
    out = {"past16m_a_bit": image[:at] + bytes([image[at] ^ 4]) + image[at + 1:],
           "past16m_a_crc": image[:-8] + bytes([image[-8] ^ 1]) + image[-7:],
           "past16m_a_cut": image[:-100000]}
    out = {name: (bad, 1 << 25, gunzip(bad)) for name, bad in out.items()}
    assert [v[2]["error"] for v in out.values()] == [out["past16m_a_bit"][2]["error"], CRC, DEFLATE]
    assert out["past16m_a_bit"][2]["error"] in (DEFLATE, CRC) and out["past16m_a_bit"][2]["error_offset"] in (0, at - 40)
    return out


SEGMENT = 4 << 20


@functools.lru_cache(maxsize=None)
def repeated_member(repeats, tail_bytes=70000):
    """-> (image, segment text, tail text): one member whose text is the segment text `repeats` times, then the tail, built
    without compressing more than one segment: a raw deflate stream ended by a full flush leaves the compressor as it
    began, so the same text gives the same bytes again (asserted), and the image repeats them.  The segment is a random
    period of 32 500 bytes behind a little FASTQ: copies of 258 bytes from 32 500 back, about 2 MiB of text a block.  The
    trailer's CRC-32 is crc_combine's; ISIZE is the length modulo 2^32."""
    rng = np.random.default_rng(77)
    period = rng.integers(0, 256, 32500, dtype=np.uint8).tobytes()
    seg_text = (fastq_text(300, 47) + period * (SEGMENT // 32500 + 1))[:SEGMENT]
    tail_text = fastq_text(tail_bytes, 48)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    seg = c.compress(seg_text) + c.flush(zlib.Z_FULL_FLUSH)
    again = c.compress(seg_text) + c.flush(zlib.Z_FULL_FLUSH)
    assert seg == again
    tail = c.compress(tail_text) + c.flush()
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    assert tail == c.compress(tail_text) + c.flush()
    crc, shift, seg_crc = 0, crc_shift(SEGMENT), zlib.crc32(seg_text)
    for _ in range(repeats):
        crc = _mul(shift, crc) ^ seg_crc
    crc = crc_combine(crc, zlib.crc32(tail_text), tail_bytes)
    image = header() + seg * repeats + tail + struct.pack("<II", crc, (repeats * SEGMENT + tail_bytes) & 0xffffffff)
    return image, seg_text, tail_text
