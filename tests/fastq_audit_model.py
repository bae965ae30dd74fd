"""Plain Python / numpy restatement of sk_trim_fastq_audit_device_async (include/sickle_amd.h): the audit of a text from
fastq_model's framing, byte by byte, independent of sickle_amd/csrc/sk_fastq_audit.h.  The tests compare the device
against it; it never reads anything the device made.  An audit here is a dict: sk_fastq_audit's members but `reserved` as
ints, and qual_hist as a uint64 array of 256."""
import numpy as np

import fastq_model as fm

NONE = (1 << 64) - 1
NAME_WORDS = ("pairs", "name_mismatch", "first_mismatch", "tags_swapped")
SCALARS = ("calls", "calls_failed") + NAME_WORDS + ("qual_bytes", "qual_min", "qual_max")
FRAMING = {"se": "se", "pe_split": "pe_split", "pe_interleaved": "pe_interleaved", "pe_combo_all": "pe_interleaved"}
ENDS = (0x20, 0x09, 0x0d)
# the quality kernel's chunk of packed qual, FQA_CHUNK_BYTES of sickle_amd/csrc/sk_fastq_audit.h: no part of the rule, only
# where the GPU test plants its extremes; tests/test_fastq_audit_host.py holds it to the header as compiled
CHUNK_BYTES = 256 * 1024


def key(line):
    """(key, tag) of a name line (bytes, without its newline)"""
    line = bytes(line)
    e = len(line)
    for i in range(1, len(line)):
        if line[i] in ENDS:
            e = i
            break
    k = line[1:e]
    if len(k) >= 2 and k[-2:] in (b"/1", b"/2"):
        return k[:-2], int(k[-1:])
    return k, 0


def pair(line1, line2):
    """-> (mismatch, swapped) of a pair from its two name lines"""
    (k1, t1), (k2, t2) = key(line1), key(line2)
    if k1 != k2:
        return True, False
    return False, (t1, t2) == (2, 1)


def zero():
    r = {k: 0 for k in SCALARS}
    r["first_mismatch"] = r["qual_min"] = NONE
    r["qual_hist"] = np.zeros(256, np.uint64)
    return r


def add(a, b):
    """what an audit holds after the calls of a and then those of b were added to it"""
    r = {k: a[k] + b[k] for k in SCALARS if k not in ("first_mismatch", "qual_min", "qual_max")}
    r["first_mismatch"] = min(a["first_mismatch"], NONE if b["first_mismatch"] == NONE else a["pairs"] + b["first_mismatch"])
    r["qual_min"], r["qual_max"] = min(a["qual_min"], b["qual_min"]), max(a["qual_max"], b["qual_max"])
    r["qual_hist"] = a["qual_hist"] + b["qual_hist"]
    return r


def failed():
    r = zero()
    r["calls_failed"] = 1
    return r


def of_records(buf, recs, mode, names=True):
    """the audit of one valid call from its framed records (fastq_model.reads)"""
    r = zero()
    r["calls"] = 1
    n = len(recs["s0"])
    if names and FRAMING[mode] != "se":
        for k in range(n // 2):
            a, b = 2 * k, 2 * k + 1
            mism, swapped = pair(buf[recs["s0"][a]:recs["e0"][a]], buf[recs["s0"][b]:recs["e0"][b]])
            r["pairs"] += 1
            r["name_mismatch"] += mism
            r["tags_swapped"] += swapped
            if mism and r["first_mismatch"] == NONE:
                r["first_mismatch"] = k
    if n:
        qual, _, _ = fm.packed(buf, recs, with_seq=False)
        if len(qual):
            r["qual_bytes"], r["qual_min"], r["qual_max"] = len(qual), int(qual.min()), int(qual.max())
            r["qual_hist"] = np.bincount(qual, minlength=256).astype(np.uint64)
    return r


def audit(ptuple, texts, mode, names=True, n_reads=None):
    """The audit of one whole-text call with (qualtype, q, l, no5, trunc_n) = ptuple on texts (one, or two for
    "pe_split"); a call with a format or a range verdict gives failed().  ptuple None: no scan, so no range verdict.
    names=False: in == NULL.  n_reads: only the first n_reads reads are the call's."""
    framing = FRAMING[mode]
    if n_reads is None and fm.verdict(texts, framing) is not None:
        return failed()
    buf, recs = fm.reads(texts, framing)
    if n_reads is not None:
        recs = {k: v[:n_reads] for k, v in recs.items()}
        if np.any(fm.reasons(buf, recs)):
            return failed()
    if ptuple is not None and len(recs["s0"]):
        _, err = fm.oracle_cuts(ptuple, buf, recs)
        if err is not None:
            return failed()
    return of_records(buf, recs, mode, names)


def equal(a, b, hist=True):
    """-> the keys in which two audits differ (empty: equal)"""
    bad = [k for k in SCALARS if int(a[k]) != int(b[k])]
    if hist and not np.array_equal(np.asarray(a["qual_hist"], np.uint64), np.asarray(b["qual_hist"], np.uint64)):
        bad.append("qual_hist")
    return bad
