#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (uses the oracle, like everything under tests/).  Soak of the device-side regrouping of ragged
batches (sk_sort.hip + sk_scan_tile_sorted_kernel): `offsets` batches of the length mixes of tests/sort_model.py (reads
under 10 bases, empty reads, one class, 63 classes, reads at and beyond the tiles' longest, one over-long read among
20 000 short ones, one length as far as the sample sees, partial last windows ...) through sk_trim_batch, sk_submit /
sk_wait on one slot, and sk_scan_device_async on the NULL stream and on two streams at once, with every longest-read
hint (none, exact, 640, stale, beyond 4 096) -- bit-exact against the oracle, the outputs pre-filled with -7; every
encoding, thresholds 0 .. 41, -l, -x, with and without -n; in every fourth batch chars out of range (two victims in
different windows and classes, the first and the last read of a window, a read under 10 bases, and one behind the 3'
break that the reference never reads).  Needs SK_SORT_MIN=1 in the environment (read once per process by the library),
or every batch below 65 536 reads would keep the plain kernels; --allow-unsorted lifts that (SK_SORT=0: the off switch).
What the library does with each batch is worked out here, from the offsets (sort_model.verdict), and counted.
usage: soak_sorted.py [--dry] [--allow-unsorted] [iterations] [seed]      --dry: no device, generator and oracle alone"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oracle_bind as ob
import sort_model as sm

RANGES = {"sanger": (33, 126), "solexa": (58, 112), "illumina": (64, 110)}  # the legal chars (reference src/sickle.h:85-91)
# drawn per batch; the mixes the regrouped scan takes come more often than the ones it leaves to the other kernels
MIXES = ("0..9", "0..40", "0..40", "one class", "two lengths", "two lengths", "75..301", "75..301", "k % 624", "around max_len",
         "empty tail", "empty tail", "uniform", "uniform eighths", "last window only", "0..639", "over-long 5000", "over-long 30000")
SHORT_MIXES = ("0..9", "0..40", "around max_len")  # ... with reads under 10 bases
BUDGET = 24_000_000  # bytes of one batch at most


def draw_lens(rng, name, n, fit):
    if name == "0..639":  # around the longest read the tiles take
        return rng.integers(0, 640, size=n)
    if name.startswith("over-long"):  # one over-long read among 20 000 short ones
        lens = rng.integers(30, 152, size=20_000)
        lens[int(rng.integers(0, 20_000))] = int(name.split()[1])
        return lens
    return sm.mix(name, n, fit, rng)


def draw_qual(rng, mode, lens, offs, lo, hi, thr):
    tot = int(offs[-1])
    mid = min(hi - 3, max(lo + 3, lo + thr + int(rng.integers(-4, 12))))
    if mode == 0:
        qual = np.clip(rng.normal(mid, 6, tot).astype(int), lo, hi)
    elif mode == 1:
        qual = np.clip(mid + rng.integers(-2, 3, size=tot), lo, hi)
    elif mode == 2:
        level = np.repeat(rng.integers(lo, hi, size=tot // 40 + 2), 40)[:tot]
        qual = np.clip(level + rng.integers(-3, 4, size=tot), lo, hi)
    elif mode == 3:
        qual = np.where(rng.random(tot) < 0.5, lo, hi)
    else:  # good with a bad start or a bad end, read by read
        qual = np.clip(rng.normal(mid + 8, 4, tot).astype(int), lo, hi)
        for i in rng.choice(len(lens), size=min(len(lens), 300), replace=False):
            a, b = int(offs[i]), int(offs[i + 1])
            if b > a:
                c = a + int(rng.integers(0, b - a))
                if i % 2:
                    qual[c:b] = lo + 2
                else:
                    qual[a:c] = lo + 2
    # (16 spare bytes: a batch of empty reads still has a buffer)
    return np.concatenate([qual.astype(np.uint8), np.full(16, lo, dtype=np.uint8)])


def plant(rng, variant, b):
    """chars out of range; returns whether the reference must see one"""
    lens, offs, qual, lo, hi = b["lens"], b["offs"], b["qual"], b["lo"], b["hi"]
    n = len(lens)
    bad = lambda: int(rng.choice([lo - 1, hi + 1, 200, 10]))
    some = np.flatnonzero(lens > 0)
    if some.size == 0:
        return False

    def hit(r, pos):
        if lens[r] < b["l"]:  # (a read below -l is not scanned at all: reference trim.cpp:21)
            b["l"] = 0
        qual[int(offs[r]) + pos] = bad()

    if variant == 0:  # two victims, in different windows (where there are two) and classes
        r1 = int(rng.choice(some))
        others = some[(sm.class_of(lens[some], 1 << 30) != sm.class_of(lens[r1], 1 << 30)) | (some // sm.WINDOW != r1 // sm.WINDOW)]
        hit(r1, 0)
        if others.size:
            hit(int(rng.choice(others)), 0)
        return True
    if variant == 1:  # the first or the last read of a window, the second or a later one where there is one
        w = int(rng.integers(1, (n - 1) // sm.WINDOW + 1)) if n > sm.WINDOW else 0
        r = w * sm.WINDOW if rng.random() < 0.5 else min(n, (w + 1) * sm.WINDOW) - 1
        if lens[r] == 0:
            r = int(some[np.argmin(np.abs(some - r))])
        hit(r, 0)  # (position 0: read in every mode -- a 3' break cannot lie before it)
        return True
    if variant == 2:  # in a read under 10 bases
        short = np.flatnonzero((lens > 0) & (lens < 10))
        hit(int(rng.choice(short if short.size else some)), 0)
        return True
    # variant 3: behind a 3' break, where the reference never looks: a good start, a bad rest, the last char out of range
    b["thr"] = max(b["thr"], 15)
    b["tn"] = 0
    long_enough = np.flatnonzero(lens >= 60)
    if long_enough.size == 0:
        return False
    r = int(rng.choice(long_enough))
    a, e = int(offs[r]), int(offs[r + 1])
    qual[a:a + 20] = hi
    qual[a + 20:e] = lo
    qual[e - 1] = hi + 1
    return False


def draw_batch(rng, it, name=None, n=None, error=None):
    qt = ["sanger", "solexa", "illumina"][it % 3]
    lo, hi = RANGES[qt]
    fit = int(rng.choice([sm.FIT_DEFAULT, sm.FIT_MAX]))
    name = name or MIXES[int(rng.integers(0, len(MIXES)))]
    if error == 2 and name not in SHORT_MIXES:
        name = SHORT_MIXES[int(rng.integers(0, len(SHORT_MIXES)))]
    n = n or int(rng.choice(sm.NS))
    if error == 0:  # two windows at least, the second one partial or full
        n = int(rng.choice([8193, 9 * 8192 + 5, 70_000]))
    if error == 1:  # ... and a full second window: its reads k = 0 and k = 8191
        n = int(rng.choice([9 * 8192 + 5, 70_000]))
    lens = np.asarray(draw_lens(rng, name, n, fit), dtype=np.int64)
    while lens.sum() > BUDGET:  # (the mixes with long reads, at the large n)
        lens = lens[:len(lens) // 2]
    offs = sm.offsets_of(lens)
    thr = int(rng.choice([0, 2, 15, 20, 25, 30, 41]))
    b = dict(name=name, qt=qt, lo=lo, hi=hi, lens=lens, offs=offs, thr=thr, l=int(rng.choice([0, 20, 100])),
             x=int(rng.integers(0, 2)), tn=int(rng.integers(0, 2)), error=error)
    b["qual"] = draw_qual(rng, int(rng.integers(0, 5)), lens, offs, lo, hi, thr)
    b["seq"] = np.frombuffer(b"ACGT" * 300 + b"Nn", dtype=np.uint8)[rng.integers(0, 1202, size=len(b["qual"]))]
    must = plant(rng, error, b) if error is not None else False
    b["po"] = ob.make_params(qt, b["thr"], b["l"], b["x"], b["tn"])
    b["want"], b["err"] = ob.oracle_trim_batch(b["po"], b["qual"], b["seq"], offsets=offs, threads=8)
    if error is not None:  # a condition on the inputs
        assert (b["err"] is not None) == must, ("the planted chars: the oracle says", b["err"], "variant", error, name, len(lens))
    else:
        assert b["err"] is None, b["err"]
    lmax = int(lens.max())
    b["lmax"] = lmax
    b["hints"] = [0, lmax, 640, max(lmax - 1, 1), 5000]  # none, exact, 640, stale (one below the longest read), beyond 4 096
    b["verdict"] = sm.verdict(offs, lmax)  # what sk_submit makes of it: it works the longest read out itself
    return b


def draw_sequence(rng, it):
    """five batches for one slot / one stream, back to back: mixed -> one length -> mixed -> with a long read -> mixed, n
    growing so that the scratch of the regrouping is allocated again"""
    plan = (("75..301", 2_000), ("uniform", 9_000), ("0..40", 20_000), ("over-long 5000", None), ("two lengths", 9 * 8192 + 5))
    seq = [draw_batch(rng, it, name, n) for name, n in plan]
    # ... and for the run on two streams a copy of one batch's qualities with a char out of range, in a read the reference scans
    for vi in (2, 4, 0):
        v = seq[vi]
        scanned = np.flatnonzero(v["lens"] >= max(v["l"], 1))
        if scanned.size:
            break
    r = int(scanned[scanned.size // 3])
    bad_qual = v["qual"].copy()
    bad_qual[int(v["offs"][r])] = v["hi"] + 1
    _, bad_err = ob.oracle_trim_batch(v["po"], bad_qual, v["seq"], offsets=v["offs"], threads=8)
    assert bad_err is not None and bad_err[0] == r and bad_err[1] == 0, (bad_err, r)
    return seq, (vi, bad_qual, bad_err)


class Device:
    def __init__(self, seed):
        import torch
        from sickle_amd import capi
        self.torch, self.capi = torch, capi
        self.ctx = capi.Context(0, 2)
        self.rng = np.random.default_rng(seed + 1)  # the hints of the back-to-back scans: the batches are the ones --dry draws

    def params(self, b):
        return self.capi.make_params(b["qt"], b["thr"], b["l"], b["x"], b["tn"])

    def compare(self, b, got, what):
        bad = np.nonzero((got != b["want"]).any(axis=1))[0]
        if bad.size:
            r = int(bad[0])
            raise AssertionError("the regrouped scan differs from the oracle: %r" % ((what, b["name"], b["qt"], b["thr"], b["l"], b["x"], b["tn"],
                                 len(b["lens"]), b["verdict"], int(bad.size), bad[:5], got[bad[:5]], b["want"][bad[:5]], b["lens"][bad[:5]],
                                 b["qual"][int(b["offs"][r]):int(b["offs"][r + 1])].tobytes().hex()[:400]),))

    def expect(self, b, fn, what):
        """run fn() -> cuts; the oracle's error must come back in the caller's numbering, or none and its cuts"""
        try:
            got = fn()
        except self.capi.RangeError as e:
            assert b["err"] is not None and (e.read, e.pos, e.ch) == tuple(b["err"]), (what, b["name"], len(b["lens"]), b["err"], (e.read, e.pos, e.ch))
            return
        assert b["err"] is None, ("device missed the error", what, b["name"], len(b["lens"]), b["err"])
        self.compare(b, got, what)

    def upload(self, b):
        t = self.torch
        return (t.from_numpy(b["qual"]).cuda(), t.from_numpy(b["seq"]).cuda(), t.from_numpy(b["offs"].view(np.int64)).cuda(),
                t.full((len(b["lens"]), 2), -7, dtype=t.int32, device="cuda"))

    def enqueue(self, b, dev, hint, stream=None, qual=None):
        dq, ds, do, out = dev
        self.ctx.scan_device_async(self.params(b), (dq if qual is None else qual).data_ptr(), out.data_ptr(), len(b["lens"]),
                                   offsets_ptr=do.data_ptr(), stride=hint, seq_ptr=ds.data_ptr() if b["tn"] else None, stream=stream)

    def batch(self, b):
        """one batch: sk_trim_batch, then the NULL stream with every hint"""
        self.expect(b, lambda: self.ctx.trim_batch(self.params(b), b["qual"], b["seq"], offsets=b["offs"]), "trim_batch")
        dev = self.upload(b)
        for hint in b["hints"]:
            def scan():
                dev[3].fill_(-7)
                self.enqueue(b, dev, hint)
                self.ctx.scan_device_finish()
                return dev[3].cpu().numpy()
            self.expect(b, scan, "device, hint %d" % hint)
        return 1 + len(b["hints"])

    def sequence(self, seq, victim):
        t, rng = self.torch, self.rng
        vi, bad_qual, bad_err = victim
        # sk_submit / sk_wait on one slot, five times in a row
        for b in seq:
            out = np.full((len(b["lens"]), 2), -7, dtype=np.int32)
            self.ctx.submit(1, self.params(b), b["qual"], out, seq=b["seq"], offsets=b["offs"], n_reads=len(b["lens"]))
            self.ctx.wait(1)
            self.compare(b, out, "submit / wait")
        # the NULL stream: five scans enqueued back to back (the two counter sets take turns), distinct outputs, one finish
        devs = [self.upload(b) for b in seq]
        for b, dev in zip(seq, devs):
            self.enqueue(b, dev, int(rng.choice([0, b["lmax"]])))
        self.ctx.scan_device_finish()
        for b, dev in zip(seq, devs):
            self.compare(b, dev[3].cpu().numpy(), "NULL stream, back to back")
        # two streams at once, a char out of range on one of them only: scratch and error word are per stream
        d_bad = t.from_numpy(bad_qual).cuda()
        devs2 = [self.upload(b) for b in seq]
        for dev in devs:
            dev[3].fill_(-7)
        t.cuda.synchronize()
        s1, s2 = t.cuda.Stream(), t.cuda.Stream()
        order2 = [2, 3, 4, 0, 1]
        for i in range(5):
            self.enqueue(seq[i], devs[i], int(rng.choice([0, seq[i]["lmax"]])), stream=s1.cuda_stream, qual=d_bad if i == vi else None)
            j = order2[i]
            self.enqueue(seq[j], devs2[j], int(rng.choice([0, seq[j]["lmax"]])), stream=s2.cuda_stream)
        try:
            self.ctx.scan_device_finish(s1.cuda_stream)
            raise AssertionError("two streams: the stream with the char out of range reports none")
        except self.capi.RangeError as e:
            assert (e.read, e.pos, e.ch) == tuple(bad_err), ("two streams", bad_err, (e.read, e.pos, e.ch))
        self.ctx.scan_device_finish(s2.cuda_stream)  # (a RangeError here: the other stream's error word was written)
        t.cuda.synchronize()
        for i, b in enumerate(seq):
            if i != vi:
                self.compare(b, devs[i][3].cpu().numpy(), "two streams, the one with the error")
            self.compare(b, devs2[i][3].cpu().numpy(), "two streams, the clean one")
        return 5 + 5 + 9 + 1


def run(iters=24, seed=1, verbose=True, dry_run=False, allow_unsorted=False, stats=None):
    if not dry_run and not allow_unsorted and not (os.environ.get("SK_SORT_MIN") == "1" and os.environ.get("SK_SORT", "1") != "0"):
        raise SystemExit("soak_sorted.py: set SK_SORT_MIN=1 (and leave SK_SORT alone): without it no batch below 65 536 reads is regrouped")
    rng = np.random.default_rng(seed)
    dev = None if dry_run else Device(seed)
    t0 = time.time()
    checked = 0
    kinds = {"sorted": 0, "plain": 0, "long": 0}
    for it in range(iters):
        error = (it // 4) % 4 if it % 4 == 3 else None
        # the first batches without planted chars walk through the values of n, largest first (a short run sees list 0 with two windows)
        walk = it - it // 4
        b = draw_batch(rng, it, n=sm.NS[-1 - walk] if error is None and walk < len(sm.NS) else None, error=error)
        kinds[b["verdict"]] += 1
        checked += dev.batch(b) if dev else 1 + len(b["hints"])
        if it % 6 == 5:
            seq, victim = draw_sequence(rng, it)
            for s in seq:
                kinds[s["verdict"]] += 1
            checked += dev.sequence(seq, victim) if dev else 20
        if verbose and it % 10 == 9:
            print("iteration %d, %d comparisons, %.0f s" % (it + 1, checked, time.time() - t0), flush=True)
    if stats is not None:
        stats.update(kinds)
    if verbose:
        print("soak ok: %d iterations, %d comparisons, seed %d; batches by what the library does with them: %d sorted, %d plain, %d long"
              % (iters, checked, seed, kinds["sorted"], kinds["plain"], kinds["long"]))
    return checked


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    run(int(args[0]) if args else 24, int(args[1]) if len(args) > 1 else 1, dry_run="--dry" in sys.argv,
        allow_unsorted="--allow-unsorted" in sys.argv)
