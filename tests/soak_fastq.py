#!/usr/bin/env python3
"""TEST INFRASTRUCTURE.  Soak: random FASTQ texts through
sk_trim_fastq_device_async on the raw C ABI against tests/fastq_model.py, byte for byte.  The texts are composed of drawn
pieces: name lines of 2 .. 300 bytes, '+' lines of 1 .. 300, reads of 1 .. 20 bases, of Illumina size, of 1 .. 30 kb and,
in some iterations, of 70 .. 300 kb (lines over several 64 KiB framing chunks, chunks without a newline).  In more than a
third of the iterations a name line is padded so that a chosen newline of a record, or the record's first byte, lands on
the last byte of a framing chunk, on the first or on the second byte of the next (the chunks start at the 16-byte boundary
below the text: the placement counts from there in half of the cases, from the text's first byte in the others).
Endings with and without the last newline, 1 .. 3 tail lines, CRLF; degenerate texts (empty, one byte, newlines only, a leading
newline, no newline at all); a malformed record and a quality char out of range at drawn records; every mode (split with
two texts drawn on their own), every encoding, -q, -l, -x, -n, the length hint 0 / exact / too small; capacities exact,
generous or one short.
usage: soak_fastq.py [--dry] [iterations] [seed]     --dry: no device, the model against itself (checks the generator)
       soak_fastq.py --replay DIR                    one dumped iteration alone"""
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import fastq_model as fm
from sickle_amd import capi

CHUNK = 65536
RANGES = {"phred": (11, 60), "sanger": (33, 126), "solexa": (59, 112), "illumina": (64, 110)}  # phred: above '\n'
BAD = {fm.SK_FQ_ID_SHORT: b"@\nACGT\n+\nIIII\n", fm.SK_FQ_ID_NO_AT: b"Xbad\nACGT\n+\nIIII\n",
       fm.SK_FQ_SEQ_EMPTY: b"@bad\n\n+\nIIII\n", fm.SK_FQ_QUAL_EMPTY: b"@bad\nACGT\n+\n\n",
       fm.SK_FQ_LENGTHS: b"@bad\nACGT\n+\nIII\n"}
ROOM = 64
LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789:/_ #", np.uint8)
BASES = np.frombuffer(b"ACGT" * 30 + b"Nn", np.uint8)


def records(rng, qt, thr, n, kind, giants):
    """n records as lists of four lines (no newlines)."""
    lo, hi = RANGES[qt]
    if kind == "tiny":
        lens = rng.integers(1, 21, n)
    elif kind == "illumina":
        lens = np.full(n, int(rng.choice([36, 75, 100, 150, 151, 250, 301]))) if rng.random() < 0.5 else \
            rng.integers(30, 302, n)
    else:
        lens = rng.integers(1000, 30_001, n)
    for _ in range(giants if n else 0):
        lens[int(rng.integers(0, n))] = int(rng.integers(70_000, 300_001))
    short_names = rng.random() < 0.5
    total = int(lens.sum())
    mid = min(hi - 3, max(lo + 3, lo + thr + int(rng.integers(-4, 12))))
    level = np.repeat(np.clip(mid + rng.integers(-8, 9, n), lo, hi), lens)
    qual = np.clip(level + rng.integers(-6, 7, total), lo, hi).astype(np.uint8).tobytes()
    seq = rng.choice(BASES, total).tobytes()
    names = rng.choice(LETTERS, 300 * n + 300).tobytes()
    recs, at = [], 0
    for k in range(n):
        L = int(lens[k])
        a = int(rng.integers(1, 12 if short_names else 300))
        b = int(rng.integers(0, 4 if short_names else 300))
        recs.append([b"@" + names[300 * k:300 * k + a], seq[at:at + L], b"+" + names[300 * k + 150:300 * k + 150 + b][:b],
                     qual[at:at + L]])
        at += L
    return recs


def place(rng, recs, shift):
    """Pads one name line so that a drawn item of a drawn record falls next to a framing-chunk boundary.  -> what it did."""
    sizes = np.array([sum(len(x) + 1 for x in r) for r in recs], np.int64)
    starts = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    total = int(sizes.sum())
    base = shift if rng.random() < 0.5 else 0  # chunks of the kernel (from the 16-byte boundary below) or of the text
    if total + base < CHUNK + 2 or len(recs) < 2:
        return None
    item = int(rng.integers(0, 5))  # 0..3: the '\n' behind that line, 4: the record's first byte
    delta = int(rng.choice([-1, 0, 1]))
    chunk = int(rng.integers(1, (total + base) // CHUNK + 1))
    target = chunk * CHUNK + delta - base  # position in the text
    rel = np.array([0 if item == 4 else sum(len(x) + 1 for x in r[:item + 1]) - 1 for r in recs], np.int64)
    k = int(np.searchsorted(starts + rel, target, side="right")) - 1
    pad_in = k - 1 if item == 4 else k  # the record whose name line grows
    if k < 0 or pad_in < 0:
        return None
    pad = target - int(starts[k] + rel[k])
    recs[pad_in][0] += b"p" * pad
    return dict(item=item, delta=delta, chunk=chunk, base=base, record=k, pad=pad)


def compose(rng, qt, thr, n, kind, giants, shift, placed):
    recs = records(rng, qt, thr, n, kind, giants)
    note = place(rng, recs, shift) if placed else None
    return recs, note


def join(recs):
    return b"".join(x + b"\n" for r in recs for x in r)


def draw(rng):
    """One iteration's inputs: plain values and the texts (what dump() writes and --replay reads)."""
    qt = str(rng.choice(["phred", "sanger", "solexa", "illumina"], p=[0.15, 0.55, 0.15, 0.15]))
    thr = int(rng.choice([0, 2, 15, 20, 25, 30, 41], p=[0.1, 0.1, 0.2, 0.3, 0.16, 0.12, 0.02]))
    c = dict(mode=str(rng.choice(["se", "pe_split", "pe_interleaved"])), shift=int(rng.integers(0, 16)),
             params=[qt, thr, int(rng.choice([0, 20, 100], p=[0.45, 0.5, 0.05])), bool(rng.integers(2)), bool(rng.integers(2))],
             index=bool(rng.random() < 0.7), notes=[])
    lo, hi = RANGES[qt]
    kind = str(rng.choice(["tiny", "illumina", "kb"], p=[0.25, 0.5, 0.25]))
    n = int(rng.integers(1, {"tiny": 6000, "illumina": 2500, "kb": 40}[kind]))
    if rng.random() < 0.1:
        n = int(rng.choice([1, 2, 3, 4, 5]))
    giants = int(rng.integers(1, 4)) if rng.random() < 0.2 else 0
    placed = rng.random() < 0.7
    c.update(kind=kind, giants=giants)
    degenerate = rng.random() < 0.02
    texts = []
    for i in range(2 if c["mode"] == "pe_split" else 1):
        m = n
        if i == 1 and rng.random() < 0.03:
            m = max(0, n + int(rng.choice([-1, 1])))  # unequal record counts: SK_FQ_PAIR_COUNT
        recs, note = compose(rng, qt, thr, m, kind, giants, c["shift"], placed)
        c["notes"].append(note)
        # a malformed record in one iteration out of eight, a quality char out of range in one out of eight
        if rng.random() < (0.125 if c["mode"] != "pe_split" else 0.065):
            why = int(rng.choice(sorted(BAD)))
            k = int(rng.integers(0, max(len(recs), 1)))
            recs[k:k + 1] = [BAD[why][:-1].split(b"\n")]
            c["notes"].append(dict(malformed=why, record=k, input=i))
        if recs and rng.random() < (0.125 if c["mode"] != "pe_split" else 0.065):
            k = int(rng.integers(0, len(recs)))
            q = bytearray(recs[k][3])
            if q:
                at = int(rng.integers(0, len(q)))
                q[at] = int(rng.choice([3 if qt == "phred" else lo - 1, hi + 1, 200, 127]))
                recs[k][3] = bytes(q)
                c["notes"].append(dict(out_of_range=q[at], record=k, pos=at, input=i))
        text = join(recs)
        ending = float(rng.random())
        if ending < 0.2:
            text = text[:-1]  # no last '\n'
        elif ending < 0.4:
            tail = [b"@t", b"AC", b"+"][:int(rng.integers(1, 4))]
            text += b"\n".join(tail) + (b"\n" if rng.random() < 0.5 else b"")
        if rng.random() < 0.02:
            text = text.replace(b"\n", b"\r\n")
            c["notes"].append("crlf")
        if degenerate:
            d = int(rng.integers(0, 9))
            text = [b"", b"A", b"\n", b"\n" * 7, b"\n" * 8, b"\n" * 9, b"\n" * 70_000, b"\n" + text, b"A" * 70_001][d]
            c["notes"].append("degenerate %d" % d)
        texts.append(text)
    c["texts"] = texts
    c["hint"] = str(rng.choice(["none", "exact", "small"], p=[0.5, 0.3, 0.2]))
    c["slack"] = [[0, 0]] * 3 if rng.random() < 0.75 else [[int(x) for x in rng.integers(1, 100, 2)] for _ in range(3)]
    c["short"] = [int(rng.choice(fm.USED[c["mode"]])), str(rng.choice(["bytes", "records"]))] if rng.random() < 0.1 else None
    return c


def model(c):
    """-> fm.expected's dict plus rc, need, caps, short, max_read_len."""
    want = fm.expected(tuple(c["params"]), c["texts"], c["mode"])
    longest = 0
    for t in c["texts"]:
        f = fm.frame(t)
        if f["records"]:
            longest = max(longest, int((f["e3"] - f["e2"] - 1).max()))
    want["max_read_len"] = {"none": 0, "exact": longest, "small": max(1, longest // 2)}[c["hint"]]
    want["short"] = None
    if want["verdict"] is not None or want["range"] is not None:
        want["rc"] = capi.SK_EFORMAT if want["verdict"] is not None else capi.SK_ERANGE
        want["need"] = ([0] * 3, [0] * 3)
        want["caps"] = ([8] * 3, [sum(len(t) for t in c["texts"]) + 2] * 3)
        return want
    used = fm.USED[c["mode"]]
    recs = [len(want["index"][o]) if o in used else 0 for o in range(3)]
    nbytes = [len(want["texts"][o]) if o in used else 0 for o in range(3)]
    want["need"] = (list(recs), list(nbytes))
    rcap = [recs[o] + c["slack"][o][0] for o in range(3)]
    bcap = [nbytes[o] + c["slack"][o][1] for o in range(3)]
    if c["short"] is not None:
        o, what = c["short"]
        if what == "records" and c["index"] and recs[o] > 0:
            rcap[o], want["short"] = recs[o] - 1, o
        elif nbytes[o] > 0:
            bcap[o], want["short"] = nbytes[o] - 1, o
    want["caps"] = (rcap, bcap)
    want["rc"] = capi.SK_OK if want["short"] is None else capi.SK_ESPACE
    return want


def device(ctx, c, want):
    from fastq_raw import SENTINEL, raw
    rcap, bcap = want["caps"]
    rc, counts, keep = raw(ctx, capi.make_params(*c["params"]), c["texts"], c["mode"], caps=list(bcap), rec_caps=list(rcap),
                           shift=c["shift"], max_read_len=want["max_read_len"], index=c["index"], room=ROOM)
    got = dict(rc=rc, counts=counts, texts=[None] * 3, index=[None] * 3, tails=True)
    for o in range(3):
        t, ix = keep[o]
        if bool((t == SENTINEL).all()) and (ix is None or bool((ix == -7).all())):
            continue  # untouched
        B, R = min(counts["bytes"][o], bcap[o]), min(counts["records"][o], rcap[o])
        got["tails"] = got["tails"] and bool((t[B:] == SENTINEL).all()) and (ix is None or bool((ix[R:] == -7).all()))
        got["texts"][o] = t[:B].cpu().numpy().tobytes()
        got["index"][o] = None if ix is None else ix[:R].cpu().numpy()
    return got


def dry(c, want):
    counts = dict(records_in=want["records_in"], tail_lines=want["tail_lines"], dropped_unpaired=want["dropped_unpaired"],
                  records=want["need"][0], bytes=want["need"][1], format_error=0, format_input=0, format_record=0,
                  range=(0, 0, 0))
    got = dict(rc=want["rc"], counts=counts, texts=[None] * 3, index=[None] * 3, tails=True)
    if want["verdict"] is not None:
        counts["format_error"], counts["format_input"], counts["format_record"] = want["verdict"]
    elif want["range"] is not None:
        counts["range"] = tuple(want["range"])
    else:
        for o in fm.USED[c["mode"]]:
            if o != want["short"] and (want["need"][1][o] or (c["index"] and want["need"][0][o])):
                got["texts"][o] = want["texts"][o]
                got["index"][o] = want["index"][o] if c["index"] else None
    return got


def locate(want_text, at):
    """Record and byte within it of byte `at` of an output text (records are four lines)."""
    nl = np.flatnonzero(np.frombuffer(want_text[:at], np.uint8) == 10)
    rec = len(nl) // 4
    start = int(nl[4 * rec - 1]) + 1 if rec else 0
    return "record %d of the output, byte %d of it" % (rec, at - start)


def compare(c, got, want):
    """-> number of comparisons made; raises AssertionError at the first difference."""
    gc = got["counts"]
    assert got["rc"] == want["rc"], "return code %d, the model says %d (counts %r)" % (got["rc"], want["rc"], gc)
    assert got["tails"], "the sentinel behind an output's last byte or record was overwritten"
    for k in ("records_in", "tail_lines", "dropped_unpaired"):
        assert gc[k] == want[k], "%s %r, the model says %r" % (k, gc[k], want[k])
    if want["rc"] in (capi.SK_EFORMAT, capi.SK_ERANGE):
        if want["rc"] == capi.SK_EFORMAT:
            triple = (gc["format_error"], gc["format_input"], gc["format_record"])
            assert triple == tuple(want["verdict"]), "verdict %r, the model says %r" % (triple, want["verdict"])
        else:
            assert tuple(gc["range"]) == tuple(want["range"]), "range error %r, the model says %r" % (gc["range"], want["range"])
        assert all(t is None for t in got["texts"]), "an output was written after an error"
        return 1
    assert (gc["records"], gc["bytes"]) == want["need"], "records, bytes %r, the model says %r" % (
        (gc["records"], gc["bytes"]), want["need"])
    checked = 1
    for o in range(3):
        if o not in fm.USED[c["mode"]] or o == want["short"]:
            assert got["texts"][o] is None, "output %d was written (%s)" % (
                o, "it does not fit" if o == want["short"] else "not of this mode")
            continue
        g, w = got["texts"][o] or b"", want["texts"][o]
        if g != w:
            ga, wa = np.frombuffer(g, np.uint8), np.frombuffer(w, np.uint8)
            m = min(len(ga), len(wa))
            d = np.flatnonzero(ga[:m] != wa[:m])
            at = int(d[0]) if len(d) else m
            raise AssertionError("output %d: %d bytes, the model %d; first difference at byte %d (%s): device %r, model %r"
                                 % (o, len(g), len(w), at, locate(w, at), g[at:at + 12], w[at:at + 12]))
        if c["index"]:
            gi = got["index"][o] if got["index"][o] is not None else np.zeros(0, np.int64)
            if not np.array_equal(gi, want["index"][o]):
                d = np.flatnonzero(gi != want["index"][o])[0] if len(gi) == len(want["index"][o]) else -1
                raise AssertionError("record_index of output %d differs, first at record %d" % (o, d))
        checked += 1
    return checked


def describe(c):
    d = {k: v for k, v in c.items() if k != "texts"}
    d["text_bytes"] = [len(t) for t in c["texts"]]
    return d


def dump(c, name):
    d = tempfile.mkdtemp(prefix=name + "_", dir=os.environ.get("SOAK_DUMP_DIR") or None)
    json.dump(describe(c), open(os.path.join(d, "case.json"), "w"))
    for i, t in enumerate(c["texts"]):
        open(os.path.join(d, "text%d.fastq" % i), "wb").write(t)
    return d


def load(d):
    c = json.load(open(os.path.join(d, "case.json")))
    c["texts"] = [open(os.path.join(d, "text%d.fastq" % i), "rb").read() for i in range(len(c.pop("text_bytes")))]
    return c


def outcome(want):
    if want["rc"] != capi.SK_OK:
        return {capi.SK_ESPACE: "SK_ESPACE", capi.SK_EFORMAT: "SK_EFORMAT", capi.SK_ERANGE: "SK_ERANGE"}[want["rc"]]
    return "OK" if sum(want["need"][1]) > 0 else "OK, empty output"


def run_case(ctx, c, is_dry):
    want = model(c)
    got = dry(c, want) if is_dry else device(ctx, c, want)
    return compare(c, got, want), outcome(want)


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
            raise AssertionError("FASTQ trim differs from the model: iteration %d, seed %d, %r: %s; inputs in %s (replay: "
                                 "soak_fastq.py --replay DIR)" % (it, seed, describe(c), e, dump(c, "soak_fastq"))) from None
        checked += k
        stats[what] = stats.get(what, 0) + 1
        for note in c["notes"]:
            if isinstance(note, dict) and "item" in note:
                stats["placed"] = stats.get("placed", 0) + 1
                break
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
