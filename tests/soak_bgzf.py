#!/usr/bin/env python3
"""TEST INFRASTRUCTURE.  Soak of the BGZF writer over one text generator.  A text is a row of block-sized stretches
(65 280 bytes), each of a drawn kind: FASTQ-like text with a drawn share of its bytes replaced by random ones (dense
between 90 % and 100 %, where the encoder's verdict turns from deflated to stored); lines of one repeated byte; exactly
2 047, 2 048, 2 049 or 5 000 lines in the block; lines sized so that the line four up starts 32 767, 32 768 or 32 769
bytes back; alphabets of 2 .. 20 symbols with Fibonacci or geometric frequencies, permuted (deep literal trees) or as
runs (deep code-length trees); four lines repeated (one match distance); binary bytes.  The text's length is k * 65 280 + d, d in -2 .. 5.
  run_host: no device.  text -> tests/cpu_shim/gpu_deflate_sim -> every member inflated with zlib, CRC-32 and ISIZE
            against zlib, the dynamic header of every deflated member parsed (no literal/length or distance code longer
            than 15 bits, no code-length code longer than 7, all three codes complete); tests/bgzf_device/bgzf_host image
            equal to the sim's; bgzf_host crclen on drawn lengths against zlib.crc32.
  run:      sk_bgzf_device_async with a drawn shift, EOF flag, bound, device-side length and validity word, against the
            sim's image of the same text.  The capacity is sk_bgzf_bound, the image's exact size, or (1 in 10) one byte less.
usage: soak_bgzf.py host [iterations] [seed] | soak_bgzf.py [--dry] [iterations] [seed] | soak_bgzf.py --replay DIR"""
import heapq
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

SIM = os.path.join(ROOT, "tests", "cpu_shim", "gpu_deflate_sim")
HOST = os.path.join(ROOT, "tests", "bgzf_device", "bgzf_host")
BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
KINDS = ("fastq_noise", "repeat_lines", "n_lines", "back_32k", "skew", "binary", "one_distance")


def build_tools():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpu_shim"), "all"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "bgzf_device"), "all"], check=True)


# ---- the text generator ------------------------------------------------------------------------------------------
def fastq_like(rng, size, L=150):
    n = size // (2 * L + 20) + 2
    recs = []
    for k in range(n):
        q = bytes(rng.integers(35, 75, L, dtype=np.uint8))
        s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L))
        recs.append(b"@M0:%d:FC:1:%d:%d 1:N:0\n%s\n+\n%s\n" % (k % 7, 1100 + k, 13 * k % 2500, s, q))
    return b"".join(recs)[:size]


def fit(data, size):
    return (data * (size // max(len(data), 1) + 1))[:size]


def one_distance_text(rng, size):
    """Four lines of one length without runs, repeated: every match copies the line four up, so all match distances are
    one value and the distance code has one used symbol (next to the one the encoder adds to keep the code complete)."""
    L = int(rng.integers(40, 400))
    four = b"".join(bytes(np.resize(rng.permutation(np.arange(48, 123).astype(np.uint8)), L - 1)) + b"\n" for _ in range(4))
    return fit(four, size)


def stretch(rng, size):
    """-> (bytes of exactly `size`, a note on what was drawn)."""
    kind = str(rng.choice(KINDS, p=[0.38, 0.08, 0.14, 0.12, 0.16, 0.07, 0.05]))
    if kind == "fastq_noise":
        share = float(rng.uniform(0.9, 1.0)) if rng.random() < 0.6 else float(rng.uniform(0, 1))
        a = np.frombuffer(fastq_like(rng, size), np.uint8).copy()
        hit = rng.random(size) < share
        a[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
        return a.tobytes(), (kind, round(share, 4))
    if kind == "repeat_lines":
        lines = []
        while sum(map(len, lines)) < size:
            lines.append(bytes([int(rng.integers(33, 127))]) * int(rng.integers(1, 700)) + b"\n")
        return b"".join(lines)[:size], (kind,)
    if kind == "n_lines":
        n = int(rng.choice([2047, 2048, 2049, 5000]))
        base = size // n
        lens = np.full(n, base)
        lens[:size - base * n] += 1  # n lines filling the stretch exactly, each ending in '\n'
        src = fastq_like(rng, size)
        out, at = [], 0
        for L in lens.tolist():
            out.append(src[at:at + L - 1].replace(b"\n", b"N") + b"\n")
            at += L
        return b"".join(out)[:size], (kind, n)
    if kind == "back_32k":
        back = int(rng.choice([32767, 32768, 32769]))
        lens = [back // 4] * 3 + [back - 3 * (back // 4)]
        one = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), back))
        lines, k = [], 0
        while sum(map(len, lines)) < size:
            body = bytearray(one[:lens[k % 4] - 1])
            for at in rng.integers(0, len(body), 20):  # the line four up is nearly this line
                body[int(at)] = 78
            lines.append(bytes(body) + b"\n")
            k += 1
        return b"".join(lines)[:size], (kind, back)
    if kind == "skew":
        m = int(rng.integers(2, 21))
        law = str(rng.choice(["fibonacci", "geometric"]))
        w = [1, 1]
        while len(w) < m:
            w.append(w[-1] + w[-2] if law == "fibonacci" else w[-1] * 2)
        w = np.array(w[:m], np.float64)
        syms = rng.permutation(np.arange(33, 127))[:m].astype(np.uint8)
        if rng.random() < 0.5:
            return rng.choice(syms, size, p=w / w.sum()).tobytes(), (kind, m, law, "permuted")
        # as runs: symbol i in runs whose lengths follow the weights, so the code LENGTHS of the block repeat in runs
        counts = np.maximum(1, (w / w.sum() * min(size, int(rng.choice([300, 3000, size])))).astype(np.int64))
        return fit(b"".join(bytes([int(s)]) * int(c) for s, c in zip(syms, counts)), size), (kind, m, law, "runs")
    if kind == "one_distance":
        return one_distance_text(rng, size), (kind,)
    low = int(rng.choice([2, 16, 256]))
    return rng.integers(0, low, size, dtype=np.uint8).tobytes(), (kind, low)


def text_of(rng):
    """-> (text, notes): 1 .. 5 block-sized stretches, the whole k * 65 280 + d bytes long, d in -2 .. 5."""
    k = int(rng.integers(1, 6))
    d = int(rng.integers(-2, 6))
    sizes = [BLOCK] * k
    if d <= 0:
        sizes[-1] += d
    else:
        sizes.append(d)
    parts = [stretch(rng, s) for s in sizes]
    return b"".join(p[0] for p in parts), [p[1] for p in parts] + [("d", d)]


# ---- what the decoder cannot see: the three Huffman codes of a dynamic header ----------------------------------------
def kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


def dynamic_header(body):
    """The code lengths of a deflate stream that starts with a dynamic block -> (literal/length, distance, code-length
    code lengths), or None for a stored / fixed block."""
    bits = int.from_bytes(body[:400], "little")
    pos = 0

    def take(n):
        nonlocal pos
        v = (bits >> pos) & ((1 << n) - 1)
        pos += n
        return v

    assert take(1) == 1, "the member's first block is not its last"
    btype = take(2)
    if btype != 2:
        return None
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = take(3)
    # canonical code of the code-length alphabet, read bit by bit (codes are sent most significant bit first)
    code, table = 0, {}
    for length in range(1, 8):
        for s in range(19):
            if cl[s] == length:
                table[(length, code)] = s
                code += 1
        code <<= 1
    lens = []
    while len(lens) < hlit + hdist:
        c, n = 0, 0
        while (n, c) not in table:
            c, n = (c << 1) | take(1), n + 1
            assert n <= 7, "no code-length code matches"
        s = table[(n, c)]
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + take(2))
        else:
            lens += [0] * ((3 + take(3)) if s == 17 else (11 + take(7)))
    assert len(lens) == hlit + hdist, "a run of code lengths crosses the end of the table"
    return lens[:hlit], lens[hlit:], cl


def code_length_symbols(ll, dl):
    """Frequencies of the 19 code-length symbols for these lengths, run-length coded as RFC 1951 3.2.7 allows and
    skd_phase_codes_and_header does it (zeros: 18 for 11 .. 138, then 17 for 3 .. 10; others: the value, then 16 for 3 .. 6)."""
    lens, freq, i = list(ll) + list(dl), [0] * 19, 0
    while i < len(lens):
        run = 1
        while i + run < len(lens) and lens[i + run] == lens[i]:
            run += 1
        v, left = lens[i], run
        if v == 0:
            while left >= 11:
                freq[18] += 1
                left -= min(left, 138)
            if left >= 3:
                freq[17] += 1
                left = 0
        else:
            freq[v] += 1
            left -= 1
            while left >= 3:
                freq[16] += 1
                left -= min(left, 6)
        freq[v] += left
        i += run
    return freq


def unlimited_depth(freq):
    """Depth of a Huffman tree over the used symbols with no length limit (the smallest possible over tie-breaks)."""
    heap = [(f, 0) for f in freq if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1] if heap else 0


def one_far_distance(dl):
    """The distance code has two symbols: number 0 (distance 1, or the one the encoder adds) and one of a distance > 2."""
    used = [i for i, x in enumerate(dl) if x]
    return len(used) == 2 and used[0] == 0 and used[1] >= 2


def check_header(body, depth):
    """Asserts the limits and the completeness of the three codes of a deflated member; depth: deepest seen, updated (and
    under "code-length, unlimited" the depth the code-length tree would have had without the 7-bit limit).  The Kraft sum
    of exactly 1 pins THIS encoder's convention: it always writes complete codes (a second distance symbol is added when
    fewer than two are used); RFC 1951 would also allow a single one-bit distance code."""
    h = dynamic_header(body)
    assert h is not None, "a deflated member without a dynamic block"
    for name, lens, limit in zip(("literal/length", "distance", "code-length"), h, (15, 15, 7)):
        assert max(lens) <= limit, "%s code of %d bits" % (name, max(lens))
        assert kraft(lens) == 1.0, "%s code is not complete: Kraft sum %r, lengths %r" % (name, kraft(lens), lens)
        depth[name] = max(depth.get(name, 0), max(lens))
    assert h[0][256] > 0, "no end-of-block code"
    depth["code-length, unlimited"] = max(depth.get("code-length, unlimited", 0),
                                          unlimited_depth(code_length_symbols(h[0], h[1])))
    if one_far_distance(h[1]):
        depth["members with one far match distance code"] = depth.get("members with one far match distance code", 0) + 1


def members(image, text, depth=None):
    """Walks the image member by member against the text -> [(stored, member bytes, text bytes)]."""
    out, at, t = [], 0, 0
    while at < len(image):
        assert image[at:at + 16] == EOF[:16], "member header at %d" % at
        m = struct.unpack_from("<H", image, at + 16)[0] + 1
        body = image[at + 18:at + m - 8]
        crc, isize = struct.unpack_from("<II", image, at + m - 8)
        piece = zlib.decompress(body, -15)
        want = text[t:t + BLOCK]
        assert piece == want, "member %d does not inflate to its block" % len(out)
        assert (crc, isize) == (zlib.crc32(want), len(want)), "CRC-32 / ISIZE of member %d" % len(out)
        stored = body[0] & 7 == 1  # BFINAL = 1, BTYPE = 00
        if stored:
            assert len(body) == len(want) + 5
        else:
            assert len(body) < len(want) + 5, "a deflated member of text + 5 bytes or more"
            if depth is not None:
                check_header(body, depth)
        out.append((stored, m, len(want)))
        at += m
        t += len(want)
    assert at == len(image) and t == len(text)
    return out


def sim_image(text, d, name="text"):
    src = os.path.join(d, name)
    open(src, "wb").write(text)
    pr = subprocess.run([SIM, src], capture_output=True)
    assert pr.returncode == 0, pr.stderr
    return (b"" if not text else pr.stdout), src


def fail(what, it, seed, notes, text, e):
    d = tempfile.mkdtemp(prefix="soak_bgzf_", dir=os.environ.get("SOAK_DUMP_DIR") or None)
    open(os.path.join(d, "text"), "wb").write(text)
    if isinstance(notes, dict):  # a call of the device run: soak_bgzf.py --replay DIR runs it alone
        json.dump(notes, open(os.path.join(d, "case.json"), "w"))
    return AssertionError("%s: iteration %d, seed %d, %r: %s; the text is in %s" % (what, it, seed, notes, e, d))


def run_host(iters=200, seed=1, verbose=True, stats=None):
    """-> number of comparisons.  stats (dict) gets stored / deflated member counts, the smallest margin of a deflated
    member (member body / text) and the deepest codes seen."""
    build_tools()
    rng = np.random.default_rng(seed)
    stats = {} if stats is None else stats
    stats.update(stored=0, deflated=0, closest=0.0, depth={})
    checked, t0 = 0, time.time()
    with tempfile.TemporaryDirectory() as d:
        for it in range(iters):
            text, notes = text_of(rng)
            try:
                image, src = sim_image(text, d)
                for stored, m, n in members(image, text, stats["depth"]):
                    stats["stored" if stored else "deflated"] += 1
                    if not stored:
                        stats["closest"] = max(stats["closest"], (m - 26) / n)
                eof = bool(it % 2)
                pr = subprocess.run([HOST, "image", src] + (["eof"] if eof else []), capture_output=True)
                assert pr.returncode == 0 and pr.stdout == image + (EOF if eof else b""), "bgzf_host image differs from the sim's"
                lens = sorted(set(int(x) for x in rng.integers(0, min(len(text), BLOCK) + 1, 6)) | {min(len(text), BLOCK)})
                pr = subprocess.run([HOST, "crclen", src] + [str(n) for n in lens], capture_output=True)
                assert pr.returncode == 0 and [int(x, 16) for x in pr.stdout.split()] == [zlib.crc32(text[:n]) for n in lens], \
                    "bgzf_host crclen differs from zlib.crc32"
            except AssertionError as e:
                raise fail("the host run of the BGZF writer is wrong", it, seed, notes, text, e) from None
            checked += 3
            if verbose and it % 50 == 49:
                print("iteration %d, %d comparisons, %.0f s" % (it + 1, checked, time.time() - t0), flush=True)
    if verbose:
        print("members: %d stored, %d deflated; largest deflated body / text %.4f; deepest codes %r" % (
            stats["stored"], stats["deflated"], stats["closest"], stats["depth"]))
        print("soak ok: %d iterations, %d comparisons, seed %d" % (iters, checked, seed))
    return checked


def draw_call(rng):
    """One iteration of the device run: the text and how it is handed over (what dump writes and --replay reads)."""
    text, notes = text_of(rng)
    if rng.random() < 0.05:
        text = text[:int(rng.integers(0, 6))]  # a text of 0 .. 5 bytes
    extra = int(rng.choice([0, 0, 1, 17, BLOCK, 3 * BLOCK + 17]))  # bound = length + extra, the length on the device
    return dict(text=text, notes=[list(n) for n in notes], shift=int(rng.integers(0, 16)), eof=bool(rng.integers(2)),
                extra=extra, valid=[None, None, 1, 0][int(rng.integers(4))] if extra else None,
                capacity=str(rng.choice(["bound", "exact", "short"], p=[0.45, 0.45, 0.1])))


def run_call(ctx, c, d, dry_run=False):
    """One drawn call on the device against the sim's image of the same text; raises AssertionError on a difference."""
    text, valid = c["text"], c["valid"]
    image, _ = sim_image(text, d)
    mem = members(image, text)
    if valid == 0:
        image, mem = b"", []
    want = image + (EOF if c["eof"] else b"")
    if dry_run:
        return
    from bgzf_raw import SENTINEL, image_of, raw
    from sickle_amd import capi
    kw = dict(shift=c["shift"], bound=len(text) + c["extra"] if c["extra"] else None,
              dev_len=len(text) if c["extra"] else None, valid=valid)
    if c["capacity"] == "short" and want:
        rc, n, out = raw(ctx, text, c["eof"], capacity=len(want) - 1, **kw)
        assert rc == capi.SK_ESPACE and n["bytes_out"] == len(want), "one byte short: rc %d, counts %r" % (rc, n)
        assert bool((out == SENTINEL).all()), "out was written although the image does not fit"
        return
    # bound: sk_bgzf_bound of what in->bytes says; exact (and a short draw on an empty image): the image's own size
    rc, n, out = raw(ctx, text, c["eof"], capacity=None if c["capacity"] == "bound" else len(want), **kw)
    assert rc == capi.SK_OK, "capacity %s: rc %d, counts %r, the image has %d bytes" % (c["capacity"], rc, n, len(want))
    got = image_of(out, n)  # also: nothing behind bytes_out was written (64 sentinel bytes lie behind the capacity)
    if got != want:
        ga, wa = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        m = min(len(ga), len(wa))
        diff = np.flatnonzero(ga[:m] != wa[:m])
        at = int(diff[0]) if len(diff) else m
        ends = np.cumsum([x[1] for x in mem])
        raise AssertionError("image of %d bytes, the sim's has %d; first difference at byte %d (member %d)"
                             % (len(got), len(want), at, int(np.searchsorted(ends, at, side="right"))))
    want_counts = dict(bytes_in=0 if valid == 0 else len(text), blocks=len(mem), stored_blocks=sum(x[0] for x in mem),
                       bytes_out=len(want))
    assert n == want_counts, "counts %r, expected %r" % (n, want_counts)


def describe(c):
    return {k: v for k, v in c.items() if k != "text"}


def load(d):
    c = json.load(open(os.path.join(d, "case.json")))
    c["text"] = open(os.path.join(d, "text"), "rb").read()
    return c


def run(iters=50, seed=1, verbose=True, dry_run=False, stats=None):
    """The device against the sim's image -> number of comparisons.  stats (dict) counts the capacities drawn."""
    build_tools()
    rng = np.random.default_rng(seed)
    ctx = None
    if not dry_run:
        from sickle_amd import capi
        ctx = capi.Context(0, 2)
    stats = {} if stats is None else stats
    checked, t0 = 0, time.time()
    with tempfile.TemporaryDirectory() as d:
        for it in range(iters):
            c = draw_call(rng)
            try:
                run_call(ctx, c, d, dry_run)
            except AssertionError as e:
                raise fail("the device's BGZF image differs from the sim's", it, seed, describe(c), c["text"], e) from None
            checked += 1
            stats[c["capacity"]] = stats.get(c["capacity"], 0) + 1
            if verbose and it % 50 == 49:
                print("iteration %d, %d comparisons, %.0f s" % (it + 1, checked, time.time() - t0), flush=True)
    if ctx is not None:
        ctx.close()
    if verbose:
        print("capacities: %s" % ", ".join("%s %d" % kv for kv in sorted(stats.items())))
        print("soak ok: %d iterations, %d comparisons, seed %d" % (iters, checked, seed))
    return checked


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--") and a != "host"]
    if "--replay" in sys.argv:
        build_tools()
        from sickle_amd import capi
        with tempfile.TemporaryDirectory() as tmp:
            run_call(capi.Context(0, 2), load(args[0]), tmp)
        print("replay ok")
    else:
        n, seed = int(args[0]) if args else 50, int(args[1]) if len(args) > 1 else 1
        if "host" in sys.argv[1:]:
            run_host(n, seed)
        else:
            run(n, seed, dry_run="--dry" in sys.argv)
