"""A deflate writer for tests (RFC 1951, nothing of zlib's): every block structure a legal stream may have and zlib never
writes.  Bits is the bit writer, Stream takes blocks (stored, fixed, dynamic) whose tokens are literal bytes or (length,
distance[, length symbol]) and keeps the text they spell; finish() holds the stream against zlib.decompressobj(-15), so a
miscounted hand-made case fails where it is built.  balanced(), ladder() and drawn_lengths() give complete code-length
assignments, rle() the straightforward spelling of a code-length sequence, tokenize() and cut() a drawn token stream and
its split into drawn blocks, drawn(seed) the whole pipeline with a counter of the features it hit."""
import bisect
import struct
import zlib

import numpy as np

import gunzip_model as gm

CL_ORDER, LEN_BASE, LEN_EXTRA, DIST_BASE, DIST_EXTRA = gm.CL_ORDER, gm.LEN_BASE, gm.LEN_EXTRA, gm.DIST_BASE, gm.DIST_EXTRA
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30
EOB = 256


class Bits:
    """Fields go out LSB first, Huffman codes first bit first."""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, width):
        assert 0 <= value < 1 << width
        self.acc |= value << self.n
        self.n += width
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        self.put(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self, fill=0):
        """to the next byte; the padding bits are `fill`'s low ones"""
        if self.n:
            self.put(fill & ((1 << (8 - self.n)) - 1), 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bits(self):
        return 8 * len(self.out) + self.n


def codes(lens):
    """canonical codes of a list of lengths -> [(code, length)], length 0 for a symbol without one"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        out.append((nxt[l], l))
        nxt[l] += 1 if l else 0
    return out


def kraft(lens):
    """sum of 2^-l in units of 2^-15"""
    return sum(1 << (15 - l) for l in lens if l)


# ---- complete length assignments -------------------------------------------------------------------------------------
def balanced(used, n):
    """n lengths; the symbols of `used` share a complete code of two adjacent lengths (one symbol: one bit)"""
    used = sorted(set(used))
    k, lens = len(used), [0] * n
    if k == 1:
        lens[used[0]] = 1
        return lens
    d = (k - 1).bit_length()
    for i, s in enumerate(used):
        lens[s] = d - 1 if i < (1 << d) - k else d
    assert kraft(lens) == 1 << 15
    return lens


def ladder(used, n, top=15):
    """n lengths; used[0] gets 1 bit, used[1] 2, ..., the last two `top` bits: 1, 2, ..., 14, 15, 15 for top = 15"""
    assert len(used) == top + 1
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = min(i + 1, top)
    assert kraft(lens) == 1 << 15
    return lens


def drawn_lengths(rng, used, n, cap=15, weights=None):
    """n lengths; a complete code over `used` drawn by splitting Kraft budget at drawn leaves, no code beyond `cap` bits.
    weights: symbol -> frequency; then the frequent symbols get the short codes (ties and a tenth of them at random)."""
    used = list(dict.fromkeys(used))
    lens = [0] * n
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    assert len(used) <= 1 << cap
    leaves = [1, 1]
    while len(leaves) < len(used):
        open_ = [i for i, d in enumerate(leaves) if d < cap]
        i = open_[int(rng.integers(0, len(open_)))] if rng.random() < 0.7 else max(open_, key=lambda j: leaves[j])
        leaves[i] += 1
        leaves.append(leaves[i])
    leaves.sort()
    order = list(used)
    rng.shuffle(order)
    if weights is not None:
        order.sort(key=lambda s: -weights.get(s, 0) * (rng.random() if rng.random() < 0.1 else 1.0))
    for s, d in zip(order, leaves):
        lens[s] = d
    assert kraft(lens) == 1 << 15
    return lens


# ---- the code-length sequence ------------------------------------------------------------------------------------------
def rle(lens, rng=None):
    """lens (literal/length and distance lengths in one list) -> items: a length 0..15, or (16, n), (17, n), (18, n) with
    n the number of entries the repeat covers.  Without rng the longest repeat is taken wherever one fits; with rng a
    repeat is used or not, and its count drawn."""
    items, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        take = rng is None or rng.random() < 0.75
        if v == 0 and run >= 3 and take:
            n = min(run, 138)
            if rng is not None:
                n = int(rng.integers(3, n + 1))
            items.append((18 if n >= 11 else 17, n))
            i += n
        elif v and i and lens[i - 1] == v and run >= 3 and take:
            n = min(run, 6)
            if rng is not None:
                n = int(rng.integers(3, n + 1))
            items.append((16, n))
            i += n
        else:
            items.append(v)
            i += 1
    return items


def spelled(items):
    """the lengths a list of items spells, and for each item its first entry"""
    lens, starts = [], []
    for it in items:
        starts.append(len(lens))
        if isinstance(it, tuple):
            lens += [lens[-1] if it[0] == 16 else 0] * it[1]
        else:
            lens.append(it)
    return lens, starts


def crossings(items, nlit):
    """how many repeats begin among the literal/length entries and end among the distance entries"""
    lens, starts = spelled(items)
    return sum(1 for it, at in zip(items, starts) if isinstance(it, tuple) and at < nlit < at + it[1])


_LENGTH_SYMBOL = [None] * 3 + [28 if n == 258 else max(s for s in range(28) if LEN_BASE[s] <= n) for n in range(3, 259)]


def length_symbol(n):
    """the symbol (less 257) a length is usually written with: 258 has its own, 285"""
    return _LENGTH_SYMBOL[n]


def distance_symbol(d):
    return bisect.bisect_right(DIST_BASE, d) - 1


def symbols_of(tokens):
    """-> (literal/length symbols used incl. 256, distance symbols used), each a dict symbol -> count"""
    lit, dist = {EOB: 1}, {}
    for t in tokens:
        if isinstance(t, tuple):
            s = 257 + (t[2] - 257 if len(t) > 2 else length_symbol(t[0]))
            lit[s] = lit.get(s, 0) + 1
            d = distance_symbol(t[1])
            dist[d] = dist.get(d, 0) + 1
        else:
            lit[t] = lit.get(t, 0) + 1
    return lit, dist


def put_dynamic_header(w, final, hlit, hdist, cl_lens, sent, items):
    """The fields as given, unchecked (the bad streams use it): BFINAL, BTYPE 2, HLIT, HDIST, HCLEN = sent - 4, `sent`
    code-length code lengths, then the items through that code"""
    w.put(int(bool(final)), 1)
    w.put(2, 2)
    w.put(hlit, 5)
    w.put(hdist, 5)
    w.put(sent - 4, 4)
    for i in range(sent):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cl = codes(cl_lens)
    for it in items:
        s = it[0] if isinstance(it, tuple) else it
        assert cl[s][1], ("no code for code-length symbol", s)
        w.code(*cl[s])
        if s == 16:
            assert 3 <= it[1] <= 6
            w.put(it[1] - 3, 2)
        elif s == 17:
            assert 3 <= it[1] <= 10
            w.put(it[1] - 3, 3)
        elif s == 18:
            assert 11 <= it[1] <= 138
            w.put(it[1] - 11, 7)


class Stream:
    """A raw deflate stream block by block, with the text its tokens spell."""

    def __init__(self):
        self.w, self.text, self.closed, self.kinds, self.ends = Bits(), bytearray(), False, [], []

    def _open(self, final, kind):
        assert not self.closed
        self.closed = bool(final)
        self.kinds.append((kind, int(bool(final))))
        self.w.put(int(bool(final)), 1)
        self.w.put(kind, 2)

    def spell(self, tokens):
        """the bytes the tokens add to the text (the text is not changed)"""
        t = bytearray(self.text[-32768:])
        base = len(t)
        for k in tokens:
            if isinstance(k, tuple):
                n, d = k[0], k[1]
                assert 3 <= n <= 258 and 1 <= d <= min(32768, len(t)), k
                for _ in range(n):
                    t.append(t[-d])
            else:
                t.append(k)
        return bytes(t[base:])

    def stored(self, final, data, fill=0):
        assert len(data) <= 65535
        self._open(final, 0)
        self.w.align(fill)
        self.w.raw(struct.pack("<HH", len(data), len(data) ^ 0xffff) + bytes(data))
        self.text += data
        self.ends.append(self.w.bits())

    def _tokens(self, lit, dist, tokens):
        w = self.w
        self.text += self.spell(tokens)
        for t in tokens:
            if isinstance(t, tuple):
                s = t[2] - 257 if len(t) > 2 else length_symbol(t[0])
                assert 0 <= t[0] - LEN_BASE[s] < 1 << LEN_EXTRA[s] and lit[257 + s][1], t
                w.code(*lit[257 + s])
                w.put(t[0] - LEN_BASE[s], LEN_EXTRA[s])
                d = distance_symbol(t[1])
                assert dist[d][1], t
                w.code(*dist[d])
                w.put(t[1] - DIST_BASE[d], DIST_EXTRA[d])
            else:
                assert lit[t][1], t
                w.code(*lit[t])
        w.code(*lit[EOB])
        self.ends.append(w.bits())

    def fixed(self, final, tokens):
        self._open(final, 1)
        self._tokens(codes(FIXED_LIT), codes(FIXED_DIST), tokens)

    def dynamic_header(self, final, lit_lens, dist_lens, cl_lens=None, cl_items=None, hclen=None):
        """BFINAL, BTYPE, the three counts, the code-length code and the lengths through it -> (literal/length codes,
        distance codes).  cl_items: the sequence symbol by symbol (see rle()); cl_lens: the code-length code's 19
        lengths, else a balanced code over the symbols the items use (and one more where they use one alone); hclen: how
        many of them are sent, else up to the last one used."""
        assert 257 <= len(lit_lens) <= 286 and 1 <= len(dist_lens) <= 30
        items = rle(list(lit_lens) + list(dist_lens)) if cl_items is None else cl_items
        assert spelled(items)[0] == list(lit_lens) + list(dist_lens)
        if cl_lens is None:
            used = {it[0] if isinstance(it, tuple) else it for it in items}
            if len(used) == 1:
                used.add(0 if 0 not in used else 1)
            cl_lens = balanced(used, 19)
        sent = max(4, 1 + max(i for i in range(19) if cl_lens[CL_ORDER[i]])) if hclen is None else hclen
        assert all(cl_lens[CL_ORDER[i]] == 0 for i in range(sent, 19)) and max(cl_lens) <= 7
        self.closed = bool(final)
        self.kinds.append((2, int(bool(final))))
        put_dynamic_header(self.w, final, len(lit_lens) - 257, len(dist_lens) - 1, cl_lens, sent, items)
        return codes(lit_lens), codes(dist_lens)

    def dynamic(self, final, lit_lens, dist_lens, tokens, cl_lens=None, cl_items=None, hclen=None):
        lit, dist = self.dynamic_header(final, lit_lens, dist_lens, cl_lens, cl_items, hclen)
        self._tokens(lit, dist, tokens)

    def plain_dynamic(self, final, tokens):
        """a dynamic block of balanced codes over what the tokens use"""
        lit, dist = symbols_of(tokens)
        self.dynamic(final, balanced(lit, max(lit) + 1 if max(lit) > 256 else 257), balanced(dist, max(dist) + 1) if dist else [0], tokens)

    def finish(self, fill=0):
        """-> (raw stream, text); zlib accepts the stream, ends on it and gives the text"""
        assert self.closed
        self.w.align(fill)
        return checked(bytes(self.w.out), bytes(self.text))


def checked(raw, text):
    d = zlib.decompressobj(-15)
    got = d.decompress(raw)
    assert d.eof and not d.unused_data and got == text, (d.eof, len(d.unused_data), len(got), len(text))
    return raw, text


def refused(raw):
    """a bad stream: zlib raises on it (not merely wants more input)"""
    d = zlib.decompressobj(-15)
    try:
        d.decompress(raw)
    except zlib.error:
        return raw
    raise AssertionError("zlib takes the stream")


def gzip_member(raw, text, head=None, crc=None, isize=None):
    return (gm.header() if head is None else head) + raw + struct.pack(
        "<II", zlib.crc32(text) if crc is None else crc, len(text) & 0xffffffff if isize is None else isize)


def bgzf_member(raw, text, crc=None, isize=None):
    import bgunzip_model as bm
    return bm.frame(b"", raw, text, crc=crc, isize=isize)


# ---- a drawn token stream and its blocks -------------------------------------------------------------------------------
def tokenize(rng, text, p_match=0.6):
    """At each position a literal or a match is drawn; the match among earlier occurrences of the next three bytes (the
    first one, far back, and the latest few), at most 32 768 back, its length drawn up to what matches (258 at most) and
    beyond the distance where the text allows."""
    seen, tokens, i, n = {}, [], 0, len(text)

    def note(a, b):
        for j in range(a, min(b, n - 2)):
            e = seen.setdefault(text[j:j + 3], [])
            if len(e) >= 5:
                del e[1]
            e.append(j)

    while i < n:
        cands = [j for j in seen.get(text[i:i + 3], ()) if i - j <= 32768] if i + 3 <= n else []
        if cands and rng.random() < p_match:
            j = cands[int(rng.integers(0, len(cands)))]
            m = 3
            while m < 258 and i + m < n and text[j + m] == text[i + m]:
                m += 1
            if m > 3 and rng.random() < 0.3:
                m = int(rng.integers(3, m + 1))
            tokens.append((m, i - j))
            note(i, i + m)
            i += m
        else:
            tokens.append(text[i])
            note(i, i + 1)
            i += 1
    return tokens


def cut(rng, tokens, sizes=(0, 0, 1, 2, 5, 20, 63, 64, 65, 200, 900)):
    """-> [(kind, tokens)]: the token stream split at drawn points into blocks of drawn kinds (0 stored, 1 fixed, 2 dynamic)"""
    out, i = [], 0
    while True:
        n = int(rng.integers(0, 1 + sizes[int(rng.integers(0, len(sizes)))]))
        out.append((int(rng.integers(0, 3)), tokens[i:i + n]))
        i += n
        if i >= len(tokens) and rng.random() < 0.5:
            return out


def drawn_text(rng):
    """200 to 40 000 bytes: FASTQ-like, bytes of a small alphabet, runs, a far repeat; uniform bytes stay under 6 000"""
    want, parts, size = int(rng.integers(200, 40001)), [], 0
    far = gm.fastq_text(int(rng.integers(50, 400)), int(rng.integers(0, 1 << 30)))
    while size < want:
        k = int(rng.integers(0, 6))
        n = int(rng.integers(20, 6000))
        if k == 0:
            p = gm.fastq_text(n, int(rng.integers(0, 1 << 30)))
        elif k == 1:
            p = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n).tobytes()
        elif k == 2:
            p = bytes([int(rng.integers(0, 256))]) * int(rng.integers(1, 700))
        elif k == 3:
            p = rng.integers(0, 256, min(n, 1500), dtype=np.uint8).tobytes()
        elif k == 4:
            p = far
        else:
            unit = rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes()
            p = (unit * (n // len(unit) + 1))[:n // 4 + 1]
        parts.append(p)
        size += len(p)
    return (b"".join(parts) + far)[:want]


FEATURES = ("stored_final", "stored_inner", "fixed_final", "fixed_inner", "dynamic_final", "dynamic_inner", "code_15_bits",
            "crossing_repeat", "no_distance_code", "one_distance_code", "empty_block", "distance_below_length", "distance_16385")


def drawn(seed, text=None, one_bgzf_member=True):
    """-> (raw stream, text, features): the whole pipeline from one seed.  features: name -> count over FEATURES.  text: the
    text to encode instead of a drawn one; one_bgzf_member: hold the result to what one BGZF member takes."""
    rng = np.random.default_rng([seed, 1951])
    f = dict.fromkeys(FEATURES, 0)
    text = drawn_text(rng) if text is None else text
    tokens = tokenize(rng, text, float(rng.choice([0.2, 0.6, 0.95])))
    blocks = cut(rng, tokens)
    s = Stream()
    for k, (kind, toks) in enumerate(blocks):
        final = k + 1 == len(blocks)
        f["empty_block"] += not toks
        for t in toks:
            if isinstance(t, tuple):
                f["distance_below_length"] += t[1] < t[0]
                f["distance_16385"] += t[1] >= 16385
        if kind == 0 and len(s.spell(toks)) > 65535:
            kind = 1  # more than a stored block holds
        f[("stored", "fixed", "dynamic")[kind] + ("_final" if final else "_inner")] += 1
        if kind == 0:
            s.stored(final, s.spell(toks), int(rng.integers(0, 256)))
        elif kind == 1:
            s.fixed(final, toks)
        else:
            lit, dist = symbols_of(toks)
            nlit = int(rng.integers(max(max(lit) + 1, 257), 287))
            extra = [int(x) for x in rng.integers(0, nlit, int(rng.integers(0, 12)))]
            lit_lens = drawn_lengths(rng, list(lit) + extra, nlit, 15, lit)
            force = rng.random() < 1 / 6
            if force and not dist:
                dist_lens = [0]
            elif force and len(dist) == 1:
                dist_lens = [0] * max(dist) + [1]
            else:
                ndist = int(rng.integers(max(dist, default=0) + 1, 31))
                extra = [int(x) for x in rng.integers(0, ndist, int(rng.integers(1, 6)))]
                dist_lens = drawn_lengths(rng, list(dist) + extra, ndist, 15, dist)
            items = rle(lit_lens + dist_lens, rng)
            syms = {it[0] if isinstance(it, tuple) else it for it in items}
            cl_extra = [int(x) for x in rng.integers(0, 19, int(rng.integers(1, 5)))]
            cl_lens = drawn_lengths(rng, list(syms) + cl_extra, 19, 7)
            f["no_distance_code"] += not any(dist_lens)
            f["one_distance_code"] += sum(1 for l in dist_lens if l) == 1
            f["crossing_repeat"] += crossings(items, nlit) > 0
            used = [lit_lens[x] for x in lit] + [dist_lens[x] for x in dist]
            f["code_15_bits"] += 15 in used
            s.dynamic(final, lit_lens, dist_lens, toks, cl_lens, items)
    raw, text = s.finish(int(rng.integers(0, 256)))
    assert not one_bgzf_member or (len(raw) <= 65000 and len(text) <= 65536)
    return raw, text, f
