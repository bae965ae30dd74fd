"""Soak of the device's plain-gzip reader (a tool, not collected by pytest): drawn images (members of drawn texts, levels,
strategies, block sizes and header fields, singly and concatenated), drawn damage (bit flips, byte changes, cuts, appended
bytes) and a drawn SK_GZIP_CHUNK and shift, against tests/gunzip_model.py.  Valid images must give the text; damaged ones
the model's reason, member and offset, or the text where the damage hit bytes nothing looks at.

    python tests/soak_gunzip.py [--iterations N] [--seed S] [--dry]

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
import gunzip_model as gm  # noqa: E402
from soak_bgunzip import check_slice, damage, draw_text  # noqa: E402

SLICE = (80, 7)  # (iterations, seed) of the slice the suite runs: tests/test_gpu_gunzip.py, and dry in tests/test_gunzip_model.py.
# The model's walk in Python is what a slice costs (0.14 s an iteration; the device's share is small): 120 iterations took
# 16.6 s on an MI355X host, so the slice has 80.  TRUNCATED is the rare reason (a cut inside a body is DEFLATE): seeds 1 to 5
# do not draw it in 80 iterations, seed 7 draws it twice.
SLICE_STATS = dict(text=43, reasons={"1": 18, "2": 2, "3": 5, "4": 5, "5": 7})  # what the model says of it
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)
KEYS = ("error", "error_member", "error_offset")


def draw_image(rng):
    """-> (image, text)"""
    parts, text = [], []
    for _ in range(int(rng.integers(0, 5))):
        n = int(rng.choice([0, 1, 40, 700, 5000, 40000])) if rng.integers(0, 2) else int(rng.integers(1, 90000))
        t = gm.fastq_text(n, int(rng.integers(0, 1 << 30))) if rng.integers(0, 2) else draw_text(rng, n)
        head = gm.header(extra=b"XY\x02\x00ab" if rng.integers(0, 4) == 0 else b"", name=b"n.fq" if rng.integers(0, 3) == 0 else b"",
                         comment=b"c" if rng.integers(0, 5) == 0 else b"", hcrc=bool(rng.integers(0, 5) == 0))
        parts.append(gm.member(t, int(rng.integers(0, 10)), STRATEGIES[int(rng.integers(0, len(STRATEGIES)))],
                               mem_level=int(rng.choice([1, 1, 2, 8])), flush_every=int(rng.integers(50, 3000)) if rng.integers(0, 4) == 0 else 0,
                               head=head))
        text.append(t)
    return b"".join(parts), b"".join(text)


def run(iterations, seed, dry=False, verbose=True, stats=None):
    """stats (a dict) gets: text, the iterations the model reads to their text; reasons, those it ends in each reason code;
    stretches_used, the device's sum (0 in a dry run)"""
    rng = np.random.default_rng(seed)
    stats = {} if stats is None else stats
    stats.update(text=0, reasons={}, stretches_used=0)
    ctx = inflate = None
    if not dry:
        import torch
        torch.cuda.is_available()
        from sickle_amd import capi
        from test_gpu_gunzip import inflate, text_of
        ctx = capi.Context(device=0)
    done = 0
    for it in range(iterations):
        image, text = draw_image(rng)
        assert gzip.decompress(image) == text if image else text == b""
        if rng.integers(0, 2):
            image = damage(rng, image)
        want = gm.gunzip(image)
        chunk, shift = int(rng.choice([256, 1024, 4096, 32768])), int(rng.integers(0, 16))  # drawn in a dry run too: the same images
        if want["error"] == 0:
            stats["text"] += 1
        else:
            stats["reasons"][str(want["error"])] = stats["reasons"].get(str(want["error"]), 0) + 1
        if dry:
            assert want["error"] != 0 or want["text"] is not None
        else:
            os.environ["SK_GZIP_CHUNK"] = str(chunk)
            # a damaged image gets slack: the text the device counts up to a failing block need not be the model's to
            # the byte, and a text beyond the capacity would skip the decode, where a lower member's failure is found
            slack = 0 if want["error"] == 0 else 1 << 20
            rc, c, out = inflate(ctx, image, shift=shift, capacity=want["bytes_out"] + slack)
            assert tuple(c[k] for k in KEYS) == tuple(want[k] for k in KEYS), (seed, it, c, want["error"])
            stats["stretches_used"] += c["stretches_used"]
            if want["error"] == 0:
                assert rc == 0 and text_of(out, c) == want["text"], (seed, it)
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
