"""What sk_trim_fastq_clipped_device_async has to give (include/sickle_amd.h): fastq_model with the packed length of a read
replaced by min(L, p), where p is the start of the read's 3' adapter hit as fastq_adapters_model.hit_of finds it on the
seq line the record descriptor names.  The framing, the verdict, the oracle's cuts, the pair rule and the emission are
fastq_model's (combo_all_model's for "pe_combo_all"), the report is fastq_report_model's over the clipped batch.  The
tests compare the device against it; it never reads anything the device made."""
import numpy as np

import combo_all_model as cm
import fastq_adapters_model as am
import fastq_model as fm
import fastq_report_model as rm
import oracle_bind as ob

FRAMING = am.FRAMING
CLIP_NONE = am.CLIP_NONE
SCALARS = ("calls", "calls_failed", "reads", "reads_clipped", "reads_emptied", "bases_clipped")
make_set = am.make_set


def zero():
    return dict({k: 0 for k in SCALARS}, hits=[0] * 8)


def failed():
    """what a call with a format or range verdict adds to the stats"""
    return dict(zero(), calls_failed=1)


def add(a, b):
    return {k: ([x + y for x, y in zip(v, b[k])] if k == "hits" else v + b[k]) for k, v in a.items()}


def seq_lines(buf, recs):
    """the seq line of every read, from its descriptor: the bytes between the name line's end and the seq line's end"""
    data = bytes(buf)
    return [data[int(a) + 1:int(b)] for a, b in zip(recs["e0"], recs["e1"])]


def hits_of(buf, recs, st):
    """-> per read (a, p) or None"""
    out = []
    for line in seq_lines(buf, recs):
        h = am.hit_of(line, st)
        out.append(None if h is None else (h[0], h[1]))
    return out


def words(hits):
    """the clip words as the device writes them"""
    return [CLIP_NONE if h is None else (h[0] << 24 | h[1]) for h in hits]


def lengths(recs, hits):
    """the packed length of every read: min(L, p) with a hit, L without"""
    L = (recs["e3"] - recs["e2"] - 1).astype(np.int64)
    p = np.array([L[i] if h is None else h[1] for i, h in enumerate(hits)], np.int64).reshape(len(L))
    return np.minimum(L, p)


def packed(buf, recs, L):
    """fastq_model.packed with the lengths given: the first L[r] bytes of every qual and seq line"""
    offsets = np.zeros(len(L) + 1, np.uint64)
    np.cumsum(L, out=offsets[1:])
    return fm._gather(buf, recs["e2"] + 1, L), fm._gather(buf, recs["e0"] + 1, L), offsets


def stats_of(recs, hits):
    """the stats of one valid call"""
    r = dict(zero(), calls=1, reads=len(hits))
    L = recs["e1"] - recs["e0"] - 1
    for i, h in enumerate(hits):
        if h is None:
            continue
        r["reads_clipped"] += 1
        r["reads_emptied"] += h[1] == 0
        r["bases_clipped"] += int(L[i]) - h[1]
        r["hits"][h[0]] += 1
    return r


def expected(ptuple, texts, mode, st, n_reads=None):
    """The whole clipped call on the host: fastq_model.expected's dict (verdict, range, texts, index, the counts), and
    clip: the stats the call adds; words: its clip words; cuts; batch: (qual, seq, offsets) as the scan saw them; buf and
    recs: fastq_model.reads'.  n_reads:
    only the first n_reads reads are the call's (a piece: the records it took)."""
    framing = FRAMING[mode]
    fr = [fm.frame(t) for t in texts]
    res = {"records_in": [f["records"] for f in fr] + [0] * (2 - len(fr)),
           "tail_lines": [f["tail_lines"] for f in fr] + [0] * (2 - len(fr)),
           "dropped_unpaired": fr[0]["records"] & 1 if framing == "pe_interleaved" else 0,
           "verdict": fm.verdict(texts, framing), "range": None, "texts": None, "index": None, "clip": failed(), "words": None,
           "cuts": None, "batch": None, "buf": None, "recs": None}
    if res["verdict"] is not None:
        return res
    buf, recs = fm.reads(texts, framing)
    if n_reads is not None:
        recs = {k: v[:n_reads] for k, v in recs.items()}
    hits = hits_of(buf, recs, st)
    res["words"] = words(hits)
    L = lengths(recs, hits)
    qual, seq, offsets = packed(buf, recs, L)
    res["batch"] = (qual, seq, offsets)
    res["buf"], res["recs"] = buf, recs
    if len(L) == 0:
        cuts, err = np.zeros((0, 2), np.int32), None
    else:
        cuts, err = ob.oracle_trim_batch(ob.make_params(*ptuple), qual, seq, offsets=offsets)
    if err is not None:
        res["range"] = err
        return res
    res["cuts"] = np.asarray(cuts, np.int64).reshape(-1, 2)
    res["clip"] = stats_of(recs, hits)
    if mode == "pe_combo_all":
        rec = cm.records_of(buf, recs, res["cuts"], ptuple[0])
        res["texts"], res["index"] = [b"".join(rec), None, None], [np.arange(len(rec), dtype=np.int64), None, None]
    else:
        res["texts"], res["index"] = fm.emit(buf, recs, res["cuts"], framing)
    return res


def report(want, mode, len_bins=0, pos_bins=0):
    """the report's model fed the clipped lengths: of a result of expected()"""
    if want["cuts"] is None:
        return rm.failed(len_bins, pos_bins)
    qual, _, offsets = want["batch"]
    return rm.of_batch(qual, offsets, want["cuts"], mode, len_bins, pos_bins)


def truncated(texts, mode, st):
    """-> the texts whose reads with a hit have seq and qual cut to p bytes, or None where a read has p == 0 (which no
    valid text holds).  Every line, every tail line and the ending stay as they are."""
    out = []
    split = [t.split(b"\n") for t in texts]
    n_recs = [(len(lines) - (lines[-1] == b"")) // 4 for lines in split]  # (behind the last '\n' there is no line)
    R = min(n_recs) if FRAMING[mode] == "pe_split" else n_recs[0] & ~1 if FRAMING[mode] == "pe_interleaved" else n_recs[0]
    for lines in split:
        for i in range(1, 4 * R, 4):  # the reads of the call alone: a dropped odd record stays as it is
            h = am.hit_of(lines[i], st)
            if h is None:
                continue
            if h[1] == 0:
                return None
            lines[i], lines[i + 2] = lines[i][:h[1]], lines[i + 2][:h[1]]
        out.append(b"\n".join(lines))
    return out


def plant(rng, text, seqs, rate=0.5, min_start=1):
    """fastq_adapters_model.plant with the drawn starts held to min_start or more: adapters written over drawn seq lines in
    place, with drawn mismatches, lower case and an N now and then; a line of min_start bases or fewer is left alone"""
    lines = text.split(b"\n")
    for i in range(1, len(lines), 4):
        n = len(lines[i])
        if n <= min_start or rng.random() >= rate:
            continue
        ad = bytearray(seqs[int(rng.integers(0, len(seqs)))])
        for _ in range(int(rng.integers(0, 3))):
            j = int(rng.integers(0, len(ad)))
            ad[j] = int(rng.choice(list(b"ACGTNacgt")))
        p = int(rng.integers(min_start, n))
        line = bytearray(lines[i])
        line[p:p + len(ad)] = ad[:n - p]
        lines[i] = bytes(line[:n])
    return b"\n".join(lines)


TRUSEQ = b"AGATCGGAAGAGC"
DRAWN_SET = dict(seqs=[TRUSEQ], min_overlap=13, max_mismatch_permille=0)


def drawn(seed):
    """Case `seed` of the drawn texts: soak_fastq's records (tiny and Illumina-sized reads, every encoding, drawn -q, -l,
    -x, -n), composed into a text per input of a drawn mode, with TruSeq planted at starts >= 1 in half of the reads.
    -> (ptuple, texts, mode)"""
    import soak_fastq
    rng = np.random.default_rng(1000 + seed)
    qt = str(rng.choice(["phred", "sanger", "solexa", "illumina"], p=[0.15, 0.55, 0.15, 0.15]))
    thr = int(rng.choice([0, 2, 15, 20, 25, 30]))
    ptuple = (qt, thr, int(rng.choice([0, 20, 50])), bool(rng.integers(2)), bool(rng.integers(2)))
    mode = str(rng.choice(["se", "pe_split", "pe_interleaved", "pe_combo_all"]))
    kind = str(rng.choice(["tiny", "illumina"], p=[0.25, 0.75]))
    n = int(rng.integers(1, 40))
    if mode in ("pe_interleaved", "pe_combo_all"):
        n += n & 1
    texts = []
    for _ in range(2 if mode == "pe_split" else 1):
        text = soak_fastq.join(soak_fastq.records(rng, qt, thr, n, kind, 0))
        if rng.random() < 0.3:
            text = text[:-1]  # no last '\n'
        texts.append(plant(rng, text, DRAWN_SET["seqs"], 0.5, 1))
    return ptuple, texts, mode


# ---- the truth table: every expectation below is written out by hand ---------------------------------------------------------
TRUTH_SET = dict(seqs=[TRUSEQ], min_overlap=5, max_mismatch_permille=0)
_A = TRUSEQ + b"ACGT"            # 17 bases, the adapter at 0: emptied
_B = b"ACGTACGTACGTACGT"         # 16 bases, no hit: kept whole
_C = b"ACGTACGTAC" + TRUSEQ      # 23 bases, a hit inside the read at 10: ACGTACGTAC stays
_D = b"ACGTACGTACGT" + b"AGATC"  # 17 bases, a hit at the last start, 12 = L - min_overlap: ACGTACGTACGT stays
_E = b"ACGT" + TRUSEQ            # 17 bases, a hit at 4: four bases stay, below -l 5
TRUTH_READS = [_A, _B, _C, _A, _B, _D, _E, _A]  # pairs (A, B), (C, A), (B, D), (E, A): a mate emptied first, second, none, both fail
TRUTH_STATS = dict(calls=1, calls_failed=0, reads=8, reads_clipped=6, reads_emptied=3, bases_clipped=3 * 17 + 13 + 5 + 13,
                   hits=[6, 0, 0, 0, 0, 0, 0, 0])
TRUTH_WORDS = [0, CLIP_NONE, 10, 0, CLIP_NONE, 12, 4, 0]


def _hi(qualtype):
    return bytes([cm.Q_BYTE[qualtype] + 40])


def truth_params(qualtype, trunc_n=False):
    return (qualtype, 20, 5, False, trunc_n)


def truth(qualtype, mode):
    """-> (texts, want texts [3], want index [3]) of the eight reads under truth_params(qualtype) and TRUTH_SET"""
    hi, lo = _hi(qualtype), bytes([cm.Q_BYTE[qualtype]])
    rec = lambda r, seq: b"@r%d\n%s\n+\n%s\n" % (r, seq, hi * len(seq))
    inputs = [rec(r, s) for r, s in enumerate(TRUTH_READS)]
    r1, r2, r4, r5 = rec(1, b"ACGTACGTACGTACGT"), rec(2, b"ACGTACGTAC"), rec(4, b"ACGTACGTACGTACGT"), rec(5, b"ACGTACGTACGT")
    n = lambda r: b"@r%d\nN\n+\n%s\n" % (r, lo)
    if mode == "se":
        return [b"".join(inputs)], [r1 + r2 + r4 + r5, None, None], [[1, 2, 4, 5], None, None]
    if mode == "pe_interleaved":
        return [b"".join(inputs)], [r4 + r5, None, r1 + r2], [[4, 5], None, [1, 2]]
    if mode == "pe_split":
        return [b"".join(inputs[0::2]), b"".join(inputs[1::2])], [r4, r5, r1 + r2], [[4], [5], [1, 2]]
    assert mode == "pe_combo_all"
    return [b"".join(inputs)], [n(0) + r1 + r2 + n(3) + r4 + r5 + n(6) + n(7), None, None], [list(range(8)), None, None]


def truth_range(qualtype, front):
    """one SE read, _C, with a quality byte below the type's range at base 3 (front: SK_ERANGE at read 0, position 3) or at
    base 15, behind the clip point 10 (SK_OK, and ACGTACGTAC is written) -> (text, want text or None, the bad byte)"""
    hi, bad = _hi(qualtype), cm.Q_BYTE[qualtype] - 1
    at = 3 if front else 15
    qual = hi * at + bytes([bad]) + hi * (22 - at)
    text = b"@x\n" + _C + b"\n+\n" + qual + b"\n"
    return text, None if front else b"@x\nACGTACGTAC\n+\n" + hi * 10 + b"\n", bad


def truth_n(qualtype):
    """three SE reads under -n (truth_params(qualtype, True)), whose rule is the reference's, bugs included: an 'N' anywhere
    in the read discards it, an 'n' at base i cuts it to i - 1 bases.  An N behind the clip point does not exist, and
    ACGTACGTAC stays; an N in front of it, at base 6, discards the read; an n there leaves ACGTA -> (text, want text)"""
    hi = _hi(qualtype)
    rec = lambda name, seq: b"@" + name + b"\n" + seq + b"\n+\n" + hi * len(seq) + b"\n"
    text = rec(b"behind", _C + b"NAC") + rec(b"front", b"ACGTACNTAC" + TRUSEQ) + rec(b"lower", b"ACGTACnTAC" + TRUSEQ)
    return text, rec(b"behind", b"ACGTACGTAC") + rec(b"lower", b"ACGTA")
