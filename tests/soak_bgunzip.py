"""Soak of the device's BGZF reader (a tool, not collected by pytest): drawn images (members of every kind member() makes,
empty members, drawn block sizes) and drawn damage (bit flips, byte changes, cuts, appended garbage) at a drawn shift,
against tests/bgunzip_model.py.  Valid images must give the text; damaged ones an error at the model's member, or the
text where the damage hit bytes nothing looks at.

    python tests/soak_bgunzip.py [--iterations N] [--seed S] [--dry]

--dry runs the generator and the model only (no GPU): every valid image must also satisfy gzip.decompress."""
import argparse
import gzip
import json
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bgunzip_model as bm  # noqa: E402

SLICE = (150, 1)  # (iterations, seed) of the slice the suite runs: tests/test_gpu_bgunzip.py, and dry in tests/test_bgunzip_model.py
SLICE_STATS = dict(text=66, reasons={"1": 25, "2": 22, "3": 2, "4": 3, "5": 32})  # what the model says of it
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)


def draw_text(rng, n):
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == 1:
        return rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), n).tobytes()
    if kind == 2:
        d = int(rng.integers(1, 300))
        return (rng.integers(0, 256, d, dtype=np.uint8).tobytes() * (n // d + 1))[:n]
    if kind == 3:
        return bytes([int(rng.integers(0, 256))]) * n
    line = rng.integers(33, 75, 101, dtype=np.uint8).tobytes()
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, line[:50], line[50:100]) for i in range(n // 110 + 1))[:n]


def draw_image(rng):
    """-> (image, text)"""
    parts, text = [], []
    for _ in range(int(rng.integers(0, 12))):
        if rng.integers(0, 6) == 0:
            parts.append(bm.EOF)
            continue
        n = int(rng.choice([1, 2, 40, 700, 5000, 65280, 65536])) if rng.integers(0, 2) else int(rng.integers(1, 65537))
        t = draw_text(rng, n)
        level, strategy = int(rng.integers(0, 10)), STRATEGIES[int(rng.integers(0, len(STRATEGIES)))]
        flush = int(rng.integers(50, 3000)) if rng.integers(0, 4) == 0 else 0
        extra = b"XY\x02\x00ab" if rng.integers(0, 5) == 0 else b""
        try:
            parts.append(bm.member(t, level, strategy, flush, extra))
        except AssertionError:  # does not fit a member: store half of it
            t = t[:30000]
            parts.append(bm.member(t, 0))
        text.append(t)
    return b"".join(parts), b"".join(text)


def damage(rng, image):
    image = bytearray(image)
    kind = int(rng.integers(0, 4))
    if kind == 3 or not image:
        return bytes(image) + rng.integers(0, 256, int(rng.integers(1, 60)), dtype=np.uint8).tobytes()
    at = int(rng.integers(0, len(image)))
    if kind == 0:
        image[at] ^= 1 << int(rng.integers(0, 8))
    elif kind == 1:
        image[at] = int(rng.integers(0, 256))
    else:
        del image[at:]
    return bytes(image)


def check_slice(stats, iterations):
    """What a soak slice of the suite must draw: a third at least read to their text, a third at least end in an error,
    and every reason code occurs"""
    assert stats["text"] + sum(stats["reasons"].values()) == iterations
    assert 3 * stats["text"] >= iterations and 3 * sum(stats["reasons"].values()) >= iterations, stats
    assert sorted(stats["reasons"]) == ["1", "2", "3", "4", "5"], stats


def run(iterations, seed, dry=False, verbose=True, stats=None):
    """stats (a dict) gets: text, the iterations the model reads to their text; reasons, those it ends in each reason code;
    stretches_used, the device's sum (0 in a dry run and for BGZF, which has none)"""
    rng = np.random.default_rng(seed)
    stats = {} if stats is None else stats
    stats.update(text=0, reasons={}, stretches_used=0)
    ctx = inflate = None
    if not dry:
        import torch
        torch.cuda.is_available()
        from sickle_amd import capi
        from test_gpu_bgunzip import inflate, text_of
        ctx = capi.Context(device=0)
    done = 0
    for it in range(iterations):
        image, text = draw_image(rng)
        assert gzip.decompress(image) == text if image else text == b""
        if rng.integers(0, 2):
            image = damage(rng, image)
        want = bm.bgunzip(image)
        shift = int(rng.integers(0, 16))  # drawn in a dry run too: the same images
        if want["error"] == 0:
            stats["text"] += 1
        else:
            stats["reasons"][str(want["error"])] = stats["reasons"].get(str(want["error"]), 0) + 1
        if dry:
            assert want["error"] != 0 or want["text"] is not None
        else:
            rc, c, out = inflate(ctx, image, shift=shift)
            if want["error"] == 0:
                assert rc == 0 and text_of(out, c) == want["text"], (seed, it)
            else:
                assert rc == capi.SK_EDATA and c["error_member"] == want["error_member"], (seed, it, c, want["error"])
        done += 1
        if verbose and it % 50 == 0:
            print("iteration %d: %d bytes, model says %d at member %d" % (it, len(image), want["error"], want["error_member"]),
                  flush=True)
    if ctx is not None:
        ctx.close()
    return done


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dry", action="store_true")
    a = ap.parse_args()
    st = {}
    print("%d iterations passed" % run(a.iterations, a.seed, dry=a.dry, stats=st))
    print("soak ok: " + json.dumps(st, sort_keys=True))
