#!/usr/bin/env python3
"""TEST INFRASTRUCTURE (uses the oracle, like everything under tests/).  Soak: random batches and cuts through
sk_trim_device_async on the raw C ABI against tests/trim_model.py, byte for byte -- every layout (fixed stride aligned /
packed / unaligned, with and without per-read lengths, offsets), input pointers shifted by 0 .. 15 bytes, read counts around
the 2 048-read count blocks, uniform / short with runs of empty reads / mixed / a few very long reads, cuts of the oracle or
made by hand (kept share and share of empty records from 0 to 1, only the first / the last / the odd reads kept), every
mode, with and without seq and read_index, capacities exact, generous or one short (SK_ESPACE), invalid kept cuts
(SK_EINVAL).  Every output carries a canary behind its last byte and record.
usage: soak_trim.py [--dry] [iterations] [seed]      --dry: no device, the model against itself (checks the generator)
       soak_trim.py --replay DIR                     one dumped iteration alone"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import oracle_bind as ob
import trim_model as tm
from sickle_amd import capi

NS = [0, 1, 2, 2046, 2047, 2048, 2049, 2050, 4096, 32766, 32767, 32768, 32769, 32770]
NS_P = [0.02, 0.03, 0.03] + [0.92 / 11] * 11
USED = {"se": (0,), "pe_split": (0, 1, 2), "pe_interleaved": (0, 2)}
NO_BAD = 2**64 - 1
ARRAYS = ("qual", "seq", "lens", "starts", "offsets", "cuts")


def draw(rng):
    """One iteration's inputs: a dict of plain values and numpy arrays (what dump() writes and --replay reads)."""
    c = {"mode": tm.MODES[int(rng.integers(3))]}
    n = int(rng.choice(NS, p=NS_P)) if rng.random() < 0.6 else int(rng.integers(3, 6000))
    if c["mode"] != "se":
        n &= ~1
    kind = str(rng.choice(["uniform", "short", "mixed", "long"]))
    if kind == "uniform":
        lens = np.full(n, int(rng.choice([1, 15, 16, 17, 36, 100, 150, 151, 250])), np.int64)
    elif kind == "short":
        lens = rng.integers(0, 41, n)
        for _ in range(int(rng.integers(0, 4))):  # runs of zero-length reads
            a = int(rng.integers(0, max(n, 1)))
            lens[a:a + int(rng.integers(1, 3000))] = 0
    elif kind == "mixed":
        lens = rng.integers(0, 301 if n > 8000 else 2501, n)
    else:
        lens = rng.integers(0, 200, n)
        for _ in range(int(rng.integers(1, 4)) if n else 0):
            lens[int(rng.integers(0, n))] = int(rng.integers(10_000, 200_001))
    lens = lens.astype(np.int64)
    lmax = max(1, int(lens.max()) if n else 1)
    layout = str(rng.choice(["offsets", "stride_aligned", "stride_packed", "stride_unaligned"]))
    stride = {"offsets": 0, "stride_aligned": (lmax + 15) // 16 * 16, "stride_packed": lmax,
              "stride_unaligned": lmax + 1 + 2 * int(rng.integers(0, 4))}[layout]
    if n * stride > 48_000_000:
        layout, stride = "offsets", 0
    with_lengths = layout != "offsets" and (kind != "uniform" or rng.random() < 0.3)
    offsets = None
    if layout == "offsets":
        offsets = np.zeros(n + 1, np.uint64)
        offsets[1:] = np.cumsum(lens)
        starts, total = offsets[:-1].astype(np.int64), int(offsets[-1])
    else:
        starts, total = np.arange(n, dtype=np.int64) * stride, n * stride
    level = np.repeat(rng.integers(36, 71, n), lens) if layout == "offsets" else \
        np.repeat(rng.integers(36, 71, n), stride)
    qual = np.clip(level + rng.integers(-7, 8, total), 33, 74).astype(np.uint8)
    seq = rng.choice(np.frombuffer(b"ACGT" * 40 + b"Nn", np.uint8), total)
    c.update(n=n, kind=kind, layout=layout, stride=stride, with_lengths=bool(with_lengths),
             read_len=0 if (with_lengths or layout == "offsets") else lmax,
             with_seq=bool(rng.random() < 0.7), with_index=bool(rng.random() < 0.7),
             shifts=[int(x) for x in rng.integers(0, 16, 2)], qual=qual, seq=seq, lens=lens, starts=starts,
             offsets=offsets)
    # ---- the cuts
    c["cut_kind"] = str(rng.choice(["oracle", "oracle", "hand", "hand", "first", "last", "odd"])) if n else "hand"
    if c["cut_kind"] == "oracle":
        p = ("sanger", int(rng.choice([0, 2, 20, 25, 30, 41], p=[0.1, 0.1, 0.35, 0.2, 0.2, 0.05])), int(rng.choice([0, 20, 100])), bool(rng.integers(2)),
             bool(rng.integers(2)))
        c["params"] = list(p)
        cuts, err = ob.oracle_trim_batch(ob.make_params(*p), qual, seq, n_reads=n, threads=4, **layout_kw(c))
        assert err is None, err
    else:
        a, b = rng.integers(0, lens + 1), rng.integers(0, lens + 1)
        cuts = np.stack([np.minimum(a, b), np.maximum(a, b)], 1).astype(np.int32).reshape(n, 2)
        c["keep"] = float(rng.choice([0, 0.003, 0.5, 1], p=[0.06, 0.2, 0.44, 0.3]))
        c["empty"] = float(rng.choice([0, 0.003, 0.5, 1], p=[0.4, 0.3, 0.24, 0.06]))
        e = rng.random(n) < c["empty"]
        cuts[e, 1] = cuts[e, 0]
        drop = rng.random(n) >= c["keep"]
        if c["cut_kind"] == "first":
            drop = np.arange(n) != 0
        elif c["cut_kind"] == "last":
            drop = np.arange(n) != n - 1
        elif c["cut_kind"] == "odd":
            drop = np.arange(n) % 2 == 0
        cuts[drop] = (-1, -1)
    c["cuts"] = np.ascontiguousarray(cuts, np.int32)
    # ---- one iteration in twenty: invalid kept cuts
    c["bad"] = []
    if n and rng.random() < 0.05:
        for r in sorted(set(int(x) for x in rng.integers(0, n, int(rng.integers(1, 4))))):
            how = int(rng.integers(3))
            c["cuts"][r] = [(-3, 4), (5, 4), (0, int(lens[r]) + 1)][how]
            c["bad"].append(r)
    # ---- capacities: exact, generous, or one output one byte / one record short
    c["slack"] = [[0, 0]] * 3 if rng.random() < 0.75 else [[int(x) for x in rng.integers(0, 100, 2)] for _ in range(3)]
    c["short"] = [int(rng.choice(USED[c["mode"]])), str(rng.choice(["bytes", "records"]))] if rng.random() < 0.1 else None
    return c


def layout_kw(c):
    if c["layout"] == "offsets":
        return dict(offsets=c["offsets"])
    if c["with_lengths"]:
        return dict(stride=c["stride"], lengths=c["lens"].astype(np.uint32))
    return dict(stride=c["stride"], read_len=c["read_len"])


def model(c):
    """-> what the call must give: dict(rc, need, bad_read, outs, caps (records, bytes per output), short)."""
    if c["bad"]:
        return dict(rc=capi.SK_EINVAL, bad_read=min(c["bad"]), need=None, outs=[None] * 3, short=None,
                    caps=([8] * 3, [64] * 3))
    outs = tm.expected(c["qual"], c["seq"] if c["with_seq"] else None, c["starts"], c["cuts"], c["mode"])
    need = tm.counts_of(outs)
    recs = [need["records"][o] + c["slack"][o][0] for o in range(3)]
    nbytes = [need["bytes"][o] + c["slack"][o][1] for o in range(3)]
    short = None
    if c["short"] is not None:
        o, what = c["short"]
        if what == "bytes" and need["bytes"][o] > 0:
            nbytes[o], short = need["bytes"][o] - 1, o
        elif need["records"][o] > 0:
            recs[o], short = need["records"][o] - 1, o
    return dict(rc=capi.SK_OK if short is None else capi.SK_ESPACE, bad_read=NO_BAD, need=need, outs=outs, short=short,
                caps=(recs, nbytes))


def device(ctx, c, want):
    """The call on the GPU -> dict(rc, counts, outs: per output None (untouched) or dict of host arrays, canaries)."""
    from trim_raw import Raw, dev, host, torch_mod
    torch = torch_mod()

    def shifted(a, shift):
        t = torch.zeros(len(a) + shift + 16, dtype=torch.uint8, device="cuda")
        t[shift:shift + len(a)] = dev(a)
        return t, t.data_ptr() + shift

    n = c["n"]
    tq, pq = shifted(c["qual"], c["shifts"][0])
    ts, ps = shifted(c["seq"], c["shifts"][1]) if c["with_seq"] else (None, None)
    toff = dev(c["offsets"]) if c["layout"] == "offsets" else None
    tlen = dev(c["lens"].astype(np.uint32)) if c["with_lengths"] else None
    tcuts = dev(c["cuts"]) if n else torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    r = Raw(want["caps"][0], want["caps"][1], seq=c["with_seq"], index=c["with_index"])
    nb = capi.lib().sk_trim_workspace_bytes(n)
    ws = torch.empty(nb + 16, dtype=torch.uint8, device="cuda")
    try:
        counts = ctx.trim_device(tcuts.data_ptr(), n, r.outs, ws.data_ptr(), nb, mode=c["mode"], qual_ptr=pq, seq_ptr=ps,
                                 offsets_ptr=None if toff is None else toff.data_ptr(), stride=c["stride"],
                                 read_len=c["read_len"], lengths_ptr=None if tlen is None else tlen.data_ptr())
        rc = capi.SK_OK
    except capi.TrimError as e:
        rc, counts = e.rc, e.counts
    got = dict(rc=rc, counts=counts, outs=[None] * 3, canaries=True)
    for o in range(3):
        if r.untouched(o):
            continue
        R, B = counts["records"][o], counts["bytes"][o]
        q, s, off, idx = r.t[o]
        got["canaries"] = got["canaries"] and r.canaries_intact(o, min(R, want["caps"][0][o]), min(B, want["caps"][1][o]))
        got["outs"][o] = dict(qual=host(q[:B]), seq=None if s is None else host(s[:B]), offsets=host(off[:R + 1]),
                              read_index=None if idx is None else host(idx[:R]))
    del tq, ts
    return got


def dry(c, want):
    """The device stubbed out by the model: what a correct device returns."""
    outs = [None] * 3
    if want["rc"] != capi.SK_EINVAL:
        for o in USED[c["mode"]]:
            if o != want["short"]:
                outs[o] = dict(want["outs"][o], read_index=want["outs"][o]["read_index"] if c["with_index"] else None)
    counts = dict(want["need"] or {"records": [0] * 3, "bytes": [0] * 3}, bad_read=want["bad_read"])
    return dict(rc=want["rc"], counts=counts, outs=outs, canaries=True)


def first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return "shapes %r and %r" % (a.shape, b.shape)
    at = int(np.flatnonzero(a != b)[0])
    return "first at %d: device %r, model %r" % (at, a[at], b[at])


def compare(c, got, want):
    """-> number of comparisons made; raises AssertionError at the first difference."""
    assert got["rc"] == want["rc"], "return code %d, the model says %d" % (got["rc"], want["rc"])
    assert got["canaries"], "a canary behind an output's last byte or record was overwritten"
    assert got["counts"]["bad_read"] == want["bad_read"], "bad_read %d, the model says %d" % (got["counts"]["bad_read"],
                                                                                            want["bad_read"])
    if want["rc"] == capi.SK_EINVAL:
        assert all(o is None for o in got["outs"]), "an output was written although a kept cut is invalid"
        return 1
    for k in ("records", "bytes"):
        assert got["counts"][k] == want["need"][k], "%s %r, the model says %r" % (k, got["counts"][k], want["need"][k])
    checked = 1
    for o in range(3):
        w, g = want["outs"][o], got["outs"][o]
        if w is None or o == want["short"]:
            assert g is None, "output %d was written (%s)" % (o, "not of this mode" if w is None else "it does not fit")
            continue
        assert g is not None, "output %d was not written" % o
        for k in ("offsets", "read_index", "qual", "seq"):
            if k == "read_index" and not c["with_index"]:
                assert g[k] is None
                continue
            if w[k] is None:
                assert g[k] is None, "output %d has %s" % (o, k)
            elif not np.array_equal(np.asarray(g[k]).astype(np.int64), np.asarray(w[k]).astype(np.int64)):
                at = first_diff(np.asarray(g[k]).astype(np.int64), np.asarray(w[k]).astype(np.int64))
                rec = ""
                if k in ("qual", "seq") and at.startswith("first at"):
                    byte = int(at.split()[2].rstrip(":"))
                    j = int(np.searchsorted(w["offsets"], byte, side="right")) - 1
                    rec = ", record %d (read %d), byte %d of it" % (j, int(w["read_index"][j]), byte - int(w["offsets"][j]))
                raise AssertionError("output %d, %s: %s%s" % (o, k, at, rec))
        checked += 1
    return checked


def describe(c):
    return {k: v for k, v in c.items() if k not in ARRAYS}


def dump(c, name):
    d = tempfile.mkdtemp(prefix=name + "_", dir=os.environ.get("SOAK_DUMP_DIR") or None)
    json.dump(describe(c), open(os.path.join(d, "case.json"), "w"))
    np.savez(os.path.join(d, "arrays.npz"), **{k: c[k] for k in ARRAYS if c[k] is not None})
    return d


def load(d):
    c = json.load(open(os.path.join(d, "case.json")))
    z = np.load(os.path.join(d, "arrays.npz"))
    c.update({k: (z[k] if k in z.files else None) for k in ARRAYS})
    return c


def outcome(c, want):
    if want["rc"] != capi.SK_OK:
        return {capi.SK_ESPACE: "SK_ESPACE", capi.SK_EINVAL: "SK_EINVAL"}[want["rc"]]
    return "OK" if sum(want["need"]["bytes"]) > 0 else "OK, empty output"


def run_case(ctx, c, is_dry):
    want = model(c)
    got = dry(c, want) if is_dry else device(ctx, c, want)
    return compare(c, got, want), outcome(c, want)


def run(iters=50, seed=1, verbose=True, dry_run=False, stats=None):
    rng = np.random.default_rng(seed)
    ctx = None if dry_run else capi.Context(0, 2)
    t0 = time.time()
    checked = 0
    stats = {} if stats is None else stats
    for it in range(iters):
        c = draw(rng)
        try:
            k, what = run_case(ctx, c, dry_run)
        except AssertionError as e:
            raise AssertionError("trim differs from the model: iteration %d, seed %d, %r: %s; inputs in %s (replay: "
                                 "soak_trim.py --replay DIR)" % (it, seed, describe(c), e, dump(c, "soak_trim"))) from None
        checked += k
        stats[what] = stats.get(what, 0) + 1
        if verbose and it % 50 == 49:
            print("iteration %d, %d comparisons, %.0f s" % (it + 1, checked, time.time() - t0), flush=True)
    if ctx is not None:
        ctx.close()
    if verbose:
        print("outcomes: %s" % ", ".join("%s %d" % kv for kv in sorted(stats.items())))
        print("soak ok: %d iterations, %d comparisons, seed %d" % (iters, checked, seed))
    return checked


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--replay" in sys.argv:
        is_dry = "--dry" in sys.argv
        print(run_case(None if is_dry else capi.Context(0, 2), load(args[0]), is_dry))
    else:
        run(int(args[0]) if args else 50, int(args[1]) if len(args) > 1 else 1, dry_run="--dry" in sys.argv)
