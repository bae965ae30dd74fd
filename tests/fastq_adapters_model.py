"""The rule of sk_trim_fastq_adapters_device_async (include/sickle_amd.h) written naively: read by read, start by start and
byte by byte over Python bytes, from fastq_model's framing (the seq lines as fm.packed gives them) and the oracle's cuts,
independent of sickle_amd/csrc/sk_fastq_adapters.h.  The tests compare the device against it; it never reads anything
the device made.  A result here is a dict: sk_fastq_adapters's members but `reserved` as ints (hits: a list of eight),
`clip` (a list with a (adapter, start) pair or None per read of the call) and, where asked for, pos as a uint64 array of
shape (8, pos_bins) and overlap of shape (8, 65)."""
import numpy as np

import fastq_model as fm

SCALARS = ("calls", "calls_failed", "reads", "kept", "reads_hit", "reads_hit_kept", "hits_full", "hits_at_0", "mismatches",
           "bases_behind", "reads_hit_out", "bases_hit_out", "pairs_both", "pairs_one", "pairs_same_clip")
ARRAYS = ("pos", "overlap")
OVERLAP_BINS = 65
FRAMING = {"se": "se", "pe_split": "pe_split", "pe_interleaved": "pe_interleaved", "pe_combo_all": "pe_interleaved"}
CLIP_NONE = 0xFFFFFFFF


def make_set(seqs, min_overlap=3, max_mismatch_permille=100):
    return dict(seqs=[s.encode() if isinstance(s, str) else bytes(s) for s in seqs], min_overlap=min_overlap,
                max_mismatch_permille=max_mismatch_permille)


def zero(pos_bins=0, overlap=False):
    r = {k: 0 for k in SCALARS}
    r["hits"] = [0] * 8
    r["clip"] = []
    if pos_bins:
        r["pos"] = np.zeros((8, pos_bins), np.uint64)
    if overlap:
        r["overlap"] = np.zeros((8, OVERLAP_BINS), np.uint64)
    return r


def failed(pos_bins=0, overlap=False):
    """what a call with a format or range verdict, or a disagreeing mode, adds"""
    return dict(zero(pos_bins, overlap), calls_failed=1)


def add(a, b):
    """what the struct and the arrays hold after the calls of a and then those of b were added; clip is the last call's
    that added (a failed call leaves the words alone)"""
    r = {}
    for k, v in a.items():
        if k == "hits":
            r[k] = [x + y for x, y in zip(v, b[k])]
        elif k == "clip":
            r[k] = list(b[k]) if b["calls"] else list(v)
        else:
            r[k] = v + b[k]
    return r


def matches(b, c):
    """read byte b against adapter byte c, in either case"""
    return (b & 0xDF) == (c & 0xDF)


def hit_of(line, st):
    """-> (a, p, v, m) of the hit of a seq line (bytes), or None"""
    L, mo, pm = len(line), st["min_overlap"], st["max_mismatch_permille"]
    for p in range(0, L - mo + 1):
        for a, ad in enumerate(st["seqs"]):
            v = min(len(ad), L - p)
            if v < mo:
                continue
            allow, m = v * pm // 1000, 0
            for j in range(v):
                if not matches(line[p + j], ad[j]):
                    m += 1
                    if m > allow:
                        break
            if m <= allow:
                return a, p, v, m
    return None


def of_reads(lines, cuts, paired, st, pos_bins=0, overlap=False):
    """the result of one valid call from its seq lines (a list of bytes) and its cuts [(five, three)]"""
    r = zero(pos_bins, overlap)
    r["calls"] = 1
    for line, (five, three) in zip(lines, cuts):
        five, three = int(five), int(three)
        kept = three >= 0
        r["reads"] += 1
        r["kept"] += kept
        h = hit_of(line, st)
        r["clip"].append(None if h is None else (h[0], h[1]))
        if h is None:
            continue
        a, p, v, m = h
        r["reads_hit"] += 1
        r["reads_hit_kept"] += kept
        r["hits"][a] += 1
        r["hits_full"] += v == len(st["seqs"][a])
        r["hits_at_0"] += p == 0
        r["mismatches"] += m
        r["bases_behind"] += len(line) - p
        if kept and p < three:
            r["reads_hit_out"] += 1
            r["bases_hit_out"] += three - max(p, five)
        if pos_bins:
            r["pos"][a][min(p, pos_bins - 1)] += 1
        if overlap:
            r["overlap"][a][v] += 1
    if paired:
        for k in range(len(lines) // 2):
            h1, h2 = r["clip"][2 * k], r["clip"][2 * k + 1]
            r["pairs_both"] += h1 is not None and h2 is not None
            r["pairs_one"] += (h1 is None) != (h2 is None)
            r["pairs_same_clip"] += h1 is not None and h2 is not None and h1[1] == h2[1]
    return r


def adapters(ptuple, texts, mode, st, pos_bins=0, overlap=False, n_reads=None):
    """The result of one whole-text call with (qualtype, q, l, no5, trunc_n) = ptuple on texts (one, or two for
    "pe_split"); a call with a format or a range verdict gives failed().  n_reads: only the first n_reads reads are the
    call's (an ordered call: the reads inside its batches; a piece: the records it took)."""
    framing = FRAMING[mode]
    if n_reads is None and fm.verdict(texts, framing) is not None:
        return failed(pos_bins, overlap)
    buf, recs = fm.reads(texts, framing)
    if n_reads is not None:
        recs = {k: v[:n_reads] for k, v in recs.items()}
        if np.any(fm.reasons(buf, recs)):
            return failed(pos_bins, overlap)
    if len(recs["s0"]) == 0:
        return dict(zero(pos_bins, overlap), calls=1)
    _, seq, offsets = fm.packed(buf, recs)
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    if err is not None:
        return failed(pos_bins, overlap)
    seq = np.asarray(seq, np.uint8).tobytes()
    off = [int(x) for x in offsets]
    lines = [seq[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    return of_reads(lines, np.asarray(cuts, np.int64).reshape(-1, 2), framing != "se", st, pos_bins, overlap)


def clip_words(r):
    """the clip array of a result, as the device words it"""
    return [CLIP_NONE if h is None else (h[0] << 24 | h[1]) for h in r["clip"]]


def equal(a, b, clip=False):
    """-> the keys in which two results differ (empty: equal); an array missing on one side counts; clip only on demand"""
    bad = []
    for k in sorted((set(a) | set(b)) - (set() if clip else {"clip"})):
        if k not in a or k not in b:
            bad.append(k)
        elif isinstance(a[k], np.ndarray) or isinstance(b[k], np.ndarray):
            if not np.array_equal(np.asarray(a[k], np.uint64), np.asarray(b[k], np.uint64)):
                bad.append(k)
        elif list(a[k]) != list(b[k]) if isinstance(a[k], (list, tuple)) else a[k] != b[k]:
            bad.append(k)
    return bad


def plant(rng, text, seqs, rate=0.5):
    """text with adapters planted into drawn seq lines at drawn starts (behind drawn inserts), overwriting bases in place
    so that every line keeps its length; the planted copy carries drawn mismatches, lower case and an N now and then"""
    lines = text.split(b"\n")
    for i in range(1, len(lines), 4):
        n = len(lines[i])
        if n == 0 or rng.random() >= rate:
            continue
        ad = bytearray(seqs[int(rng.integers(0, len(seqs)))])
        for _ in range(int(rng.integers(0, 3))):
            j = int(rng.integers(0, len(ad)))
            ad[j] = int(rng.choice(list(b"ACGTNacgt")))
        p = int(rng.integers(0, n))
        line = bytearray(lines[i])
        line[p:p + len(ad)] = ad[:n - p]
        lines[i] = bytes(line[:n])
    return b"\n".join(lines)
