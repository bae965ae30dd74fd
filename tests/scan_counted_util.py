"""TEST INFRASTRUCTURE (uses the oracle, like everything under tests/).  The cases of tests/test_gpu_scan_counted.py:
`offsets` batches of B reads scanned by sk_scan_counted_device_async with the read count in a device word, against the
oracle on the first n reads.  How every case is prepared (Runner.counted):
  - out is pre-filled with SENTINEL, and the entries at or beyond n must still hold it afterwards;
  - in the device copy every qual and seq byte at or beyond offsets[n] is 0x01, out of range in every encoding;
  - offsets[n + 1 ..] is overwritten with a descending sequence of values inside [0, offsets[n]], so a scan that looks
    beyond n gives wrong cuts or a range error, never an address outside the buffers.  No value here points outside an
    allocation, and none may.
A read's cut depends on that read alone, so the oracle runs once per (shape, encoding, -n) on all B reads and its first n
rows are its answer for the first n reads.
Run as a script it is the child process of the regrouped cases (the library reads SK_SORT_MIN once per process):
    SK_SORT_MIN=1 python tests/scan_counted_util.py regrouped"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np

import oracle_bind as ob

SENTINEL = -7
RANGES = {"sanger": (33, 126), "illumina": (64, 110)}  # the legal chars of the two encodings the cases run at
ENCODINGS = tuple(RANGES)
BIG = 20_000
BIG_COUNTS = (0, 1, 63, 64, 65, 8191, 8192, 8193, 16384, BIG - 1, BIG)


def beyond(B):
    """the two words above the bound every shape is also run at: both are taken as B"""
    return (B + 7, 1 << 40)


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.uint64))]).astype(np.uint64)


def lens_of(shape, rng):
    """-> (lengths, the longest-read hint handed to the library: 0 = none)"""
    if shape == "uniform":  # the lane-per-read tile kernel, every tile on the matrix path
        return np.full(BIG, 150), 150
    if shape == "mixed":  # with SK_SORT_MIN=1: regrouped
        return rng.integers(30, 505, size=BIG), 504
    if shape == "ragged":  # no tile fits a wave's buffer: all left to the teams of 16 lanes
        return rng.integers(600, 3001, size=300), 3000
    if shape == "long":  # a hint beyond 4 096: the streaming kernel alone, spans of equal cost
        return rng.integers(5000, 40001, size=40), 40000
    if shape == "handover":  # no hint: tiles 0, 2 and 3 are the tile kernel's, tile 1 (read 70 is 6 kb) the streaming kernel's
        lens = rng.integers(40, 301, size=200)
        lens[70] = 6000
        return lens, 0
    if shape == "all_left":  # no hint and no tile fits: the tile kernel leaves every tile, word 6 says so
        return np.full(130, 5000), 0
    raise ValueError(shape)


def draw(shape, enc, seed=11):
    rng = np.random.default_rng(seed)
    lens, hint = lens_of(shape, rng)
    offs = offsets_of(lens)
    tot = int(offs[-1])
    lo, hi = RANGES[enc]
    # levels that change every 40 bases around the default threshold: cuts on both sides, some reads dropped
    level = np.repeat(rng.integers(lo + 8, lo + 38, size=tot // 40 + 2), 40)[:tot]
    qual = np.clip(level + rng.integers(-6, 7, size=tot), lo, hi).astype(np.uint8)
    qual = np.concatenate([qual, np.full(16, lo, dtype=np.uint8)])  # (spare bytes: never an empty buffer)
    seq = np.frombuffer(b"ACGT" * 60 + b"Nn", dtype=np.uint8)[rng.integers(0, 242, size=len(qual))].copy()
    return dict(shape=shape, enc=enc, lens=lens, offs=offs, qual=qual, seq=seq, hint=hint, B=len(lens), want={})


def want_of(b, tn):
    """the oracle's cuts of all B reads with or without -n, computed once"""
    if tn not in b["want"]:
        cuts, err = ob.oracle_trim_batch(ob.make_params(b["enc"], 20, 20, False, tn), b["qual"], b["seq"], offsets=b["offs"], threads=8)
        assert err is None, err
        b["want"][tn] = cuts
    return b["want"][tn]


def tail_offsets(b, n):
    """offsets[n + 1 ..]: descending, inside [0, offsets[n]]"""
    return np.linspace(int(b["offs"][n]), 0, num=b["B"] - n, dtype=np.uint64)


class Runner:
    def __init__(self, ctx):
        import torch
        from sickle_amd import capi
        self.t, self.capi, self.ctx = torch, capi, ctx

    def upload(self, b):
        t = self.t
        b["dev"] = (t.from_numpy(b["qual"]).cuda(), t.from_numpy(b["seq"]).cuda(), t.from_numpy(b["offs"].view(np.int64)).cuda())

    def prepared(self, b, n, empty_tail=False):
        """device copies of qual, seq and offsets with everything beyond the first n reads spoilt; a fresh out.
        empty_tail: offsets[n + 1 ..] = offsets[n] instead, the empty reads a bound leaves behind the records"""
        t = self.t
        if "dev" not in b:
            self.upload(b)
        dq, ds, do = (x.clone() for x in b["dev"])
        end = int(b["offs"][n])
        dq[end:] = 1
        ds[end:] = 1
        if n < b["B"]:
            do[n + 1:] = int(b["offs"][n]) if empty_tail else t.from_numpy(tail_offsets(b, n).view(np.int64)).cuda()
        out = t.full((b["B"], 2), SENTINEL, dtype=t.int32, device="cuda")
        return dq, ds, do, out

    def word(self, value):
        return self.t.tensor([value], dtype=self.t.int64, device="cuda")

    def enqueue(self, b, tn, bufs, word, stream=None):
        dq, ds, do, out = bufs
        self.ctx.scan_counted_device_async(self.capi.make_params(b["enc"], 20, 20, False, tn), dq.data_ptr(), out.data_ptr(), b["B"],
                                           None if word is None else word.data_ptr(), do.data_ptr(),
                                           seq_ptr=ds.data_ptr() if tn else None, max_read_len=b["hint"], stream=stream)

    def check(self, b, tn, n, out, what):
        got, want = out.cpu().numpy(), want_of(b, tn)
        bad = np.nonzero((got[:n] != want[:n]).any(axis=1))[0]
        assert bad.size == 0, "%s: %s %s -n=%d, n = %d of %d: %d cuts differ from the oracle, first at read %d: %r, not %r" % (
            what, b["shape"], b["enc"], tn, n, b["B"], bad.size, bad[0], got[bad[0]], want[bad[0]])
        touched = np.nonzero((got[n:] != SENTINEL).any(axis=1))[0]
        assert touched.size == 0, "%s: %s %s -n=%d, n = %d of %d: %d entries at or beyond n were written, first %d: %r" % (
            what, b["shape"], b["enc"], tn, n, b["B"], touched.size, n + touched[0], got[n + touched[0]])

    def counted(self, b, tn, word_value, empty_tail=False):
        """one counted scan and its finish; the word may lie above the bound"""
        n = min(word_value, b["B"])
        bufs = self.prepared(b, n, empty_tail)
        word = self.word(word_value)
        self.enqueue(b, tn, bufs, word)
        self.ctx.scan_device_finish()  # (a RangeError: the scan looked at a byte at or beyond offsets[n])
        self.check(b, tn, n, bufs[3], "word %d" % word_value)

    def sweep(self, b, tn, counts):
        for v in tuple(counts) + beyond(b["B"]):
            self.counted(b, tn, v)


def regrouped_child():
    """every count of the mixed shape behind the regrouping, and a uniform batch half full: the empty reads beyond n must
    not make it a mixed one"""
    assert os.environ.get("SK_SORT_MIN") == "1" and os.environ.get("SK_SORT", "1") != "0", "the parent sets SK_SORT_MIN=1"
    import torch
    torch.cuda.is_available()
    from sickle_amd import capi
    ctx = capi.Context(device=0, slots=1)
    run = Runner(ctx)
    scans = 0
    for enc in ENCODINGS:
        mixed, uniform = draw("mixed", enc), draw("uniform", enc)
        for tn in (False, True):
            run.sweep(mixed, tn, BIG_COUNTS)
            run.counted(uniform, tn, 10_000)
            run.counted(uniform, tn, 10_000, empty_tail=True)
            scans += len(BIG_COUNTS) + 4
    ctx.close()
    print("regrouped ok: %d scans" % scans)


if __name__ == "__main__":
    assert sys.argv[1:] == ["regrouped"], sys.argv
    regrouped_child()
