"""numpy restatement of sk_trim_fastq_report_device_async (include/sickle_amd.h): the report of a text from
fastq_model's framing and the oracle's cuts.  The tests compare the device against it; it never reads anything the device
made.  A report here is a dict: sk_fastq_report's members as ints (pairs: a list of four) and, for the bins asked for, the
six histograms as uint64 arrays."""
import numpy as np

import fastq_model as fm

SCALARS = ("calls", "calls_failed", "reads", "kept", "discarded", "bases_in", "bases_out", "bases_cut5", "bases_cut3",
           "bases_discarded", "reads_cut5", "reads_cut3", "max_len_in", "max_len_out")
MAXIMA = ("max_len_in", "max_len_out")
LEN_ARRAYS, POS_ARRAYS = ("len_in", "len_out"), ("qsum_in", "qcnt_in", "qsum_out", "qcnt_out")
FRAMING = {"se": "se", "pe_split": "pe_split", "pe_interleaved": "pe_interleaved", "pe_combo_all": "pe_interleaved"}


def zero(len_bins=0, pos_bins=0):
    r = {k: 0 for k in SCALARS}
    r["pairs"] = [0, 0, 0, 0]
    for k in LEN_ARRAYS:
        if len_bins:
            r[k] = np.zeros(len_bins, np.uint64)
    for k in POS_ARRAYS:
        if pos_bins:
            r[k] = np.zeros(pos_bins, np.uint64)
    return r


def add(a, b):
    """what a report holds after the calls of a and then those of b were added to it"""
    r = {}
    for k, v in a.items():
        if k in MAXIMA:
            r[k] = max(v, b[k])
        elif k == "pairs":
            r[k] = [x + y for x, y in zip(v, b[k])]
        else:
            r[k] = v + b[k]
    return r


def failed(len_bins=0, pos_bins=0):
    """what a call with a format or range verdict adds"""
    r = zero(len_bins, pos_bins)
    r["calls_failed"] = 1
    return r


def _hist(values, bins, weights=None):
    if not bins:
        return None
    v = np.minimum(np.asarray(values, np.int64), bins - 1)
    if weights is None:
        return np.bincount(v, minlength=bins).astype(np.uint64)
    # float64 sums of bytes are exact far beyond any test's size (2^53 / 255 bytes)
    return np.bincount(v, weights=np.asarray(weights, np.float64), minlength=bins).astype(np.uint64)


def of_batch(qual, offsets, cuts, mode, len_bins=0, pos_bins=0):
    """the report of one valid call from its packed batch (qual bytes, offsets) and its cuts; mode: the call's"""
    off = np.asarray(offsets, np.int64)
    cuts = np.asarray(cuts, np.int64).reshape(-1, 2)
    qual = np.asarray(qual, np.uint8)
    L = np.diff(off)
    five, three = cuts[:, 0], cuts[:, 1]
    kept = three >= 0
    out = np.where(kept, three - five, 0)
    r = zero(len_bins, pos_bins)
    r["calls"] = 1
    r["reads"], r["kept"], r["discarded"] = len(L), int(kept.sum()), int((~kept).sum())
    if FRAMING[mode] != "se":
        k1, k2 = kept[0::2], kept[1::2]
        assert len(k1) == len(k2)
        cls = k1.astype(np.int64) | (k2.astype(np.int64) << 1)
        r["pairs"] = [int((cls == c).sum()) for c in range(4)]
    r["bases_in"], r["bases_out"] = int(L.sum()), int(out.sum())
    r["bases_cut5"], r["bases_cut3"] = int(five[kept].sum()), int((L - three)[kept].sum())
    r["bases_discarded"] = int(L[~kept].sum())
    r["reads_cut5"], r["reads_cut3"] = int((five[kept] != 0).sum()), int((three[kept] != L[kept]).sum())
    r["max_len_in"] = int(L.max()) if len(L) else 0
    r["max_len_out"] = int(out[kept].max()) if kept.any() else 0
    if len_bins:
        r["len_in"], r["len_out"] = _hist(L, len_bins), _hist(out[kept], len_bins)
    if pos_bins:
        total = int(off[-1])
        p = np.arange(total, dtype=np.int64) - np.repeat(off[:-1], L)
        q = qual[:total]
        r["qsum_in"], r["qcnt_in"] = _hist(p, pos_bins, q), _hist(p, pos_bins)
        inside = np.repeat(kept, L) & (p >= np.repeat(five, L)) & (p < np.repeat(three, L))
        po = (p - np.repeat(five, L))[inside]
        r["qsum_out"], r["qcnt_out"] = _hist(po, pos_bins, q[inside]), _hist(po, pos_bins)
    return r


def report(ptuple, texts, mode, len_bins=0, pos_bins=0, n_reads=None):
    """The report of one whole-text call with (qualtype, q, l, no5, trunc_n) = ptuple on texts (one, or two for
    "pe_split"); a call with a format or a range verdict gives failed().  n_reads: only the first n_reads reads are
    the call's (an ordered call: the reads inside its batches; a piece: the records it took)."""
    framing = FRAMING[mode]
    if n_reads is None and fm.verdict(texts, framing) is not None:
        return failed(len_bins, pos_bins)
    buf, recs = fm.reads(texts, framing)
    if n_reads is not None:
        recs = {k: v[:n_reads] for k, v in recs.items()}
        if np.any(fm.reasons(buf, recs)):
            return failed(len_bins, pos_bins)
    if len(recs["s0"]) == 0:
        r = zero(len_bins, pos_bins)
        r["calls"] = 1
        return r
    qual, seq, offsets = fm.packed(buf, recs)
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    if err is not None:
        return failed(len_bins, pos_bins)
    return of_batch(qual, offsets, cuts, mode, len_bins, pos_bins)


def equal(a, b):
    """-> the keys in which two reports differ (empty: equal); a histogram missing on one side counts"""
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


def summary_text(r, mode):
    """the reference's kept / discarded lines (reference src/trim_paired.cpp:468-475, src/trim_single.cpp:347)"""
    if mode == "se":
        return "FastQ records kept: %d\nFastQ records discarded: %d\n\n" % (r["kept"], r["discarded"])
    p0, p1, p2, p3 = r["pairs"]
    lines = ["", "FastQ paired records kept: %d (%d pairs)" % (2 * p3, p3)]
    if mode == "pe_split":
        lines.append("FastQ single records kept: %d (from PE1: %d, from PE2: %d)" % (p1 + p2, p1, p2))
    else:
        lines.append("FastQ single records kept: %d" % (p1 + p2))
    lines.append("FastQ paired records discarded: %d (%d pairs)" % (2 * p0, p0))
    if mode == "pe_split":
        lines.append("FastQ single records discarded: %d (from PE1: %d, from PE2: %d)" % (p1 + p2, p2, p1))
    else:
        lines.append("FastQ single records discarded: %d" % (p1 + p2))
    return "\n".join(lines) + "\n\n"
