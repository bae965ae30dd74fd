"""numpy restatement of sk_trim_fastq_rejects_device_async (include/sickle_amd.h): the rejects text of a text call from
fastq_model's framing and reads and the oracle's cuts, independent of sickle_amd/csrc/sk_fastq_rejects.h.  The tests compare
the device against it; it never reads anything the device made.  A result is a dict: text (bytes), index (int64 read
numbers), records, bytes, reads, valid."""
import numpy as np

import fastq_model as fm

FRAMING = {"se": "se", "pe_split": "pe_split", "pe_interleaved": "pe_interleaved", "pe_combo_all": "pe_interleaved"}
MODES = tuple(FRAMING)
# the gather's chunk of output bytes and its LDS window of records (FQJ_GCHUNK, FQJ_WIN of sk_fastq_rejects.hip): no part
# of the rule, only where the GPU test plants its edges
GCHUNK = 8192
WIN = 128
BLOCK_READS = 2048


def void():
    """a call behind a text call with a verdict, or with a disagreeing mode"""
    return {"text": b"", "index": np.zeros(0, np.int64), "records": 0, "bytes": 0, "reads": 0, "valid": 0}


def select(kept, mode, pairs):
    """-> bool per read: the selection.  kept: bool per read, mates at 2k and 2k + 1 in the pair framings."""
    kept = np.asarray(kept, bool)
    if pairs and FRAMING[mode] == "se":
        raise ValueError("SK_FQ_REJECTS_PAIRS with SK_TRIM_SE is SK_EINVAL")
    sel = ~kept
    if pairs:
        n = len(kept) & ~1
        any_lost = sel[0:n:2] | sel[1:n:2]
        sel = sel.copy()
        sel[0:n:2] = any_lost
        sel[1:n:2] = any_lost
    return sel


def of_reads(buf, recs, cuts, mode, pairs=False):
    """the rejects of one valid call from its reads (fm.reads: offsets into buf, whose last byte is a '\\n') and cuts"""
    cuts = np.asarray(cuts, np.int64).reshape(-1, 2)
    n = len(recs["s0"])
    idx = np.flatnonzero(select(cuts[:n, 1] >= 0, mode, pairs)).astype(np.int64)
    s0, e3 = recs["s0"][idx], recs["e3"][idx]
    nl = len(buf) - 1
    starts = np.stack([s0, np.full_like(s0, nl)], 1)
    lens = np.stack([e3 - s0, np.ones_like(s0)], 1)
    text = fm._gather(buf, starts.reshape(-1), lens.reshape(-1)).tobytes()
    return {"text": text, "index": idx, "records": len(idx), "bytes": int((e3 - s0 + 1).sum()), "reads": n, "valid": 1}


def rejects(ptuple, texts, mode, pairs=False, n_reads=None):
    """The rejects of one whole-text call with (qualtype, q, l, no5, trunc_n) = ptuple on texts (one, or two for
    "pe_split"); a call with a format or a range verdict gives void().  n_reads: only the first n_reads reads are the
    call's (an ordered call: the reads inside its batches; a piece: the records it took)."""
    framing = FRAMING[mode]
    if n_reads is None and fm.verdict(texts, framing) is not None:
        return void()
    buf, recs = fm.reads(texts, framing)
    if n_reads is not None:
        recs = {k: v[:n_reads] for k, v in recs.items()}
        if np.any(fm.reasons(buf, recs)):
            return void()
    if len(recs["s0"]) == 0:
        r = void()
        r["valid"] = 1
        return r
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    if err is not None:
        return void()
    return of_reads(buf, recs, cuts, mode, pairs)


def pieces(ptuple, texts, mode, takes, pairs=False):
    """The piece form: takes[p] = the reads piece p took (a stream driver's pieces cut the file at record, or pair,
    boundaries and every read belongs to one piece).  -> the per-piece results, whose texts concatenated are the
    whole-text result's."""
    framing = FRAMING[mode]
    buf, recs = fm.reads(texts, framing)
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    assert err is None
    out, at = [], 0
    for n in takes:
        part = {k: v[at:at + n] for k, v in recs.items()}
        r = of_reads(buf, part, cuts[at:at + n], mode, pairs)
        r["index"] = r["index"] + at  # in the file's numbering; a piece call numbers from its own first read
        out.append(r)
        at += n
    return out


def equal(got, want):
    """-> the keys in which two results differ (empty: equal); only the keys of `want`"""
    bad = []
    for k, v in want.items():
        if k not in got:
            bad.append(k)
        elif k == "index":
            if got[k] is not None and not np.array_equal(np.asarray(got[k], np.int64), v):
                bad.append(k)
        elif k == "text":
            if bytes(got[k]) != v:
                bad.append(k)
        elif int(got[k]) != v:
            bad.append(k)
    return bad


# ---- the drawn texts: soak_fastq's generator at a fixed seed, the same hundred on the CPU and on the GPU -------------------
DRAWN_SEED, DRAWN = 20261, 100


def drawn():
    """-> the DRAWN cases of soak_fastq.draw at DRAWN_SEED, each with "pairs": the selection the case is run with"""
    import soak_fastq
    rng = np.random.default_rng(DRAWN_SEED)
    cases = []
    for _ in range(DRAWN):
        c = soak_fastq.draw(rng)
        c["pairs"] = bool(rng.integers(2)) and c["mode"] != "se"
        cases.append(c)
    return cases
