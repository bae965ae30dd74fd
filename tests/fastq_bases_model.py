"""numpy restatement of sk_trim_fastq_bases_device_async (include/sickle_amd.h): the bases of a text from fastq_model's
framing (the seq lines as fm.packed gives them) and the oracle's cuts, independent of sickle_amd/csrc/sk_fastq_bases.h.
The tests compare the device against it; it never reads anything the device made.  The bases here are a dict:
sk_fastq_bases's members but `reserved` as ints (bases_in, bases_out: lists of six) and, where asked for, pos_in and
pos_out as uint64 arrays of shape (6, pos_bins) and gc_in and gc_out of 101."""
import numpy as np

import fastq_model as fm

CLASSES = ("A", "C", "G", "T", "N", "other")
SCALARS = ("calls", "calls_failed", "reads", "kept", "lower_in", "lower_out", "reads_n_in", "reads_n_out", "gc_none_in",
           "gc_none_out")
LISTS = ("bases_in", "bases_out")
POS_ARRAYS, GC_ARRAYS = ("pos_in", "pos_out"), ("gc_in", "gc_out")
GC_BINS = 101
FRAMING = {"se": "se", "pe_split": "pe_split", "pe_interleaved": "pe_interleaved", "pe_combo_all": "pe_interleaved"}
# the kernel's chunk of packed positions, FQB_CHUNK_BYTES of sickle_amd/csrc/sk_fastq_bases.h: no part of the rule, only
# where the GPU test plants its edges; tests/test_fastq_bases_host.py holds it to the header as compiled
CHUNK_BYTES = 256 * 1024

# the class of every byte value: the table of the issue, written out
CLASS_OF = np.full(256, 5, np.int64)
for _c, _letters in enumerate((b"Aa", b"Cc", b"Gg", b"Tt", b"Nn")):
    for _b in _letters:
        CLASS_OF[_b] = _c
LOWER = np.zeros(256, bool)
LOWER[ord("a"):ord("z") + 1] = True


def zero(pos_bins=0, gc=False):
    r = {k: 0 for k in SCALARS}
    for k in LISTS:
        r[k] = [0] * 6
    if pos_bins:
        for k in POS_ARRAYS:
            r[k] = np.zeros((6, pos_bins), np.uint64)
    if gc:
        for k in GC_ARRAYS:
            r[k] = np.zeros(GC_BINS, np.uint64)
    return r


def add(a, b):
    """what the bases hold after the calls of a and then those of b were added to them"""
    r = {}
    for k, v in a.items():
        r[k] = [x + y for x, y in zip(v, b[k])] if k in LISTS else v + b[k]
    return r


def failed(pos_bins=0, gc=False):
    """what a call with a format or range verdict, or a disagreeing mode, adds"""
    r = zero(pos_bins, gc)
    r["calls_failed"] = 1
    return r


def _per_read(cls, ridx, n):
    """-> (has an N, acgt, C + G) per read from the classes of its bytes"""
    count = lambda sel: np.bincount(ridx[sel], minlength=n)
    return count(cls == 4) > 0, count(cls < 4), count((cls == 1) | (cls == 2))


def _gc(acgt, cg, gc):
    some = acgt > 0
    hist = np.bincount((100 * cg[some]) // acgt[some], minlength=GC_BINS).astype(np.uint64) if gc else None
    return int((~some).sum()), hist


def of_batch(seq, offsets, cuts, pos_bins=0, gc=False):
    """the bases of one valid call from its packed seq lines (bytes, offsets) and its cuts"""
    off = np.asarray(offsets, np.int64)
    cuts = np.asarray(cuts, np.int64).reshape(-1, 2)
    n = len(off) - 1
    L = np.diff(off)
    total = int(off[-1])
    seq = np.asarray(seq, np.uint8)[:total]
    five, three = cuts[:, 0], cuts[:, 1]
    kept = three >= 0
    r = zero(pos_bins, gc)
    r["calls"], r["reads"], r["kept"] = 1, n, int(kept.sum())
    cls, low = CLASS_OF[seq], LOWER[seq]
    ridx = np.repeat(np.arange(n, dtype=np.int64), L)
    p = np.arange(total, dtype=np.int64) - np.repeat(off[:-1], L)
    inside = np.repeat(kept, L) & (p >= np.repeat(five, L)) & (p < np.repeat(three, L))
    r["bases_in"] = [int(x) for x in np.bincount(cls, minlength=6)]
    r["bases_out"] = [int(x) for x in np.bincount(cls[inside], minlength=6)]
    r["lower_in"], r["lower_out"] = int(low.sum()), int(low[inside].sum())
    has_n, acgt, cg = _per_read(cls, ridx, n)
    r["reads_n_in"] = int(has_n.sum())
    r["gc_none_in"], hist = _gc(acgt, cg, gc)
    if gc:
        r["gc_in"] = hist
    has_n, acgt, cg = _per_read(cls[inside], ridx[inside], n)
    r["reads_n_out"] = int(has_n[kept].sum())
    r["gc_none_out"], hist = _gc(acgt[kept], cg[kept], gc)
    if gc:
        r["gc_out"] = hist
    if pos_bins:
        table = lambda c, q: np.bincount(c * pos_bins + np.minimum(q, pos_bins - 1),
                                         minlength=6 * pos_bins).astype(np.uint64).reshape(6, pos_bins)
        r["pos_in"] = table(cls, p)
        r["pos_out"] = table(cls[inside], (p - np.repeat(five, L))[inside])
    return r


def bases(ptuple, texts, mode, pos_bins=0, gc=False, n_reads=None):
    """The bases of one whole-text call with (qualtype, q, l, no5, trunc_n) = ptuple on texts (one, or two for
    "pe_split"); a call with a format or a range verdict gives failed().  n_reads: only the first n_reads reads are the
    call's (an ordered call: the reads inside its batches; a piece: the records it took)."""
    framing = FRAMING[mode]
    if n_reads is None and fm.verdict(texts, framing) is not None:
        return failed(pos_bins, gc)
    buf, recs = fm.reads(texts, framing)
    if n_reads is not None:
        recs = {k: v[:n_reads] for k, v in recs.items()}
        if np.any(fm.reasons(buf, recs)):
            return failed(pos_bins, gc)
    if len(recs["s0"]) == 0:
        r = zero(pos_bins, gc)
        r["calls"] = 1
        return r
    _, seq, offsets = fm.packed(buf, recs)
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    if err is not None:
        return failed(pos_bins, gc)
    return of_batch(seq, offsets, cuts, pos_bins, gc)


def equal(a, b):
    """-> the keys in which two results differ (empty: equal); an array missing on one side counts"""
    bad = []
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            bad.append(k)
        elif isinstance(a[k], np.ndarray) or isinstance(b[k], np.ndarray):
            if not np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)):
                bad.append(k)
        elif a[k] != b[k]:
            bad.append(k)
    return bad
