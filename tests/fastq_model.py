"""numpy restatement of sk_trim_fastq_device_async (include/sickle_amd.h): framing, the record checks and their verdict,
tail lines and the odd-interleaved drop, and the output texts from the cuts of a scan.  Vectorised like
trim_model.expected, so it takes millions of records.  The tests compare the device against it; it never reads anything
the device made."""
import numpy as np

import oracle_bind as ob

SK_FQ_OK, SK_FQ_ID_SHORT, SK_FQ_ID_NO_AT, SK_FQ_SEQ_EMPTY, SK_FQ_QUAL_EMPTY, SK_FQ_LENGTHS, SK_FQ_TOO_LONG, \
    SK_FQ_PAIR_COUNT = range(8)
SK_MAX_READ_LEN = 1 << 24
USED = {"se": (0,), "pe_split": (0, 1, 2), "pe_interleaved": (0, 2)}


def _u8(text):
    return np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text, np.uint8)


def frame(text):
    """-> dict(s0, e0, e1, e2, e3: int64 per complete record (name start, end of each line), records, tail_lines).
    Lines end at '\\n' only; a last line without one ends at the end of the text."""
    buf = _u8(text)
    ends = np.flatnonzero(buf == 10).astype(np.int64)
    if len(buf) and buf[-1] != 10:
        ends = np.append(ends, len(buf))
    starts = np.concatenate(([0], ends[:-1] + 1)).astype(np.int64) if len(ends) else ends
    R = len(ends) // 4
    f = {"records": R, "tail_lines": len(ends) % 4, "s0": starts[0:4 * R:4]}
    for k in range(4):
        f["e%d" % k] = ends[k:4 * R:4]
    return f


def reasons(text, f):
    """SK_FQ_* of every record: the first failing check, in the reference's order (src/FQEntry.cpp:53-97)."""
    buf = _u8(text)
    name = f["e0"] - f["s0"]
    seq = f["e1"] - f["e0"] - 1
    qual = f["e3"] - f["e2"] - 1
    first = buf[np.minimum(f["s0"], max(len(buf) - 1, 0))] if len(buf) else np.zeros(0, np.uint8)
    return np.select([name <= 1, first != ord("@"), seq == 0, qual == 0, qual != seq, qual > SK_MAX_READ_LEN],
                     [SK_FQ_ID_SHORT, SK_FQ_ID_NO_AT, SK_FQ_SEQ_EMPTY, SK_FQ_QUAL_EMPTY, SK_FQ_LENGTHS, SK_FQ_TOO_LONG],
                     SK_FQ_OK).astype(np.int64)


def verdict(texts, mode):
    """-> None, or (reason, input, record) of the lowest malformed record in read order (split: PAIR_COUNT at the
    first record without a mate counts as one)."""
    fr = [frame(t) for t in texts]
    cands = []
    for i, (t, f) in enumerate(zip(texts, fr)):
        why = reasons(t, f)
        bad = np.flatnonzero(why)
        if len(bad):
            k = int(bad[0])
            read = 2 * k + i if mode == "pe_split" else k
            cands.append((read, int(why[k]), i, k))
    if mode == "pe_split" and fr[0]["records"] != fr[1]["records"]:
        r0, r1 = fr[0]["records"], fr[1]["records"]
        i, k = (1, r0) if r0 < r1 else (0, r1)
        cands.append((2 * k + i, SK_FQ_PAIR_COUNT, i, k))
    if not cands:
        return None
    _, why, i, k = min(cands)
    return why, i, k


def reads(texts, mode):
    """-> (buf, recs): one byte buffer holding every input (then one '\\n' for the synthesized newlines) and the
    framed records in read order as int64 arrays (s0, e0, e1, e2, e3 as offsets into buf).  Interleaved: an odd last
    record is dropped.  Split: mates at 2k, 2k + 1."""
    fr = [frame(t) for t in texts]
    base = np.cumsum([0] + [len(t) for t in texts])
    buf = np.concatenate([_u8(t) for t in texts] + [np.array([10], np.uint8)])
    keys = ("s0", "e0", "e1", "e2", "e3")
    if mode == "pe_split":
        n = min(fr[0]["records"], fr[1]["records"])
        recs = {k: np.empty(2 * n, np.int64) for k in keys}
        for k in keys:
            recs[k][0::2] = fr[0][k][:n] + base[0]
            recs[k][1::2] = fr[1][k][:n] + base[1]
    else:
        n = fr[0]["records"] & ~1 if mode == "pe_interleaved" else fr[0]["records"]
        recs = {k: fr[0][k][:n] for k in keys}
    return buf, recs


def _gather(buf, starts, lens, piece_chunk=1 << 22):
    """buf[starts[j] : starts[j] + lens[j]] for every j, back to back (in chunks of pieces: bounded memory)."""
    lens = lens.astype(np.int64)
    out = []
    for a in range(0, len(lens), piece_chunk):
        ln, st = lens[a:a + piece_chunk], starts[a:a + piece_chunk]
        total = int(ln.sum())
        if total:
            cum = np.concatenate(([0], np.cumsum(ln)[:-1]))
            out.append(buf[np.repeat(st - cum, ln) + np.arange(total, dtype=np.int64)])
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def packed(buf, recs, with_seq=True):
    """qual (and seq) lines packed back to back -> (qual, seq, offsets): the batch the scan sees."""
    L = recs["e3"] - recs["e2"] - 1
    offsets = np.zeros(len(L) + 1, np.uint64)
    np.cumsum(L, out=offsets[1:])
    qual = _gather(buf, recs["e2"] + 1, L)
    seq = _gather(buf, recs["e0"] + 1, L) if with_seq else None
    return qual, seq, offsets


def oracle_cuts(params_tuple, buf, recs):
    qual, seq, offsets = packed(buf, recs)
    if len(offsets) == 1:
        return np.zeros((0, 2), np.int32), None
    return ob.oracle_trim_batch(ob.make_params(*params_tuple), qual, seq, offsets=offsets)


def dests(cuts, mode):
    kept = np.asarray(cuts)[:, 1] >= 0
    if mode == "se":
        return np.where(kept, 0, -1).astype(np.int8)
    d = np.full(len(kept), -1, dtype=np.int8)
    k1, k2 = kept[0::2], kept[1::2]
    both = k1 & k2
    d1, d2 = d[0::2], d[1::2]
    d1[both] = 0
    d2[both] = 1 if mode == "pe_split" else 0
    d1[k1 & ~k2] = 2
    d2[k2 & ~k1] = 2
    return d


def emit(buf, recs, cuts, mode):
    """-> [text0, text1, text2] (bytes, None where the mode has no such output) and [index0, ...] (read numbers):
    name '\\n' seq[five:three] '\\n' plus '\\n' qual[five:three] '\\n' of every kept record, routed by the pair rule."""
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1, 2)
    d = dests(cuts, mode)
    nl = len(buf) - 1
    texts, index = [None] * 3, [None] * 3
    for o in USED[mode]:
        idx = np.flatnonzero(d == o)
        s0, e0, e1, e2 = (recs[k][idx] for k in ("s0", "e0", "e1", "e2"))
        five, three = cuts[idx, 0], cuts[idx, 1]
        m = three - five
        starts = np.stack([s0, e0 + 1 + five, np.full_like(s0, nl), e1 + 1, e2 + 1 + five, np.full_like(s0, nl)], 1)
        lens = np.stack([e0 - s0 + 1, m, np.ones_like(m), e2 - e1, m, np.ones_like(m)], 1)
        texts[o] = _gather(buf, starts.reshape(-1), lens.reshape(-1)).tobytes()
        index[o] = idx.astype(np.int64)
    return texts, index


def expected(params_tuple, texts, mode):
    """The whole call on the host: -> dict(verdict, range, texts, index, counts)."""
    fr = [frame(t) for t in texts]
    res = {"records_in": [f["records"] for f in fr] + [0] * (2 - len(fr)),
           "tail_lines": [f["tail_lines"] for f in fr] + [0] * (2 - len(fr)),
           "dropped_unpaired": fr[0]["records"] & 1 if mode == "pe_interleaved" else 0,
           "verdict": verdict(texts, mode), "range": None, "texts": None, "index": None}
    if res["verdict"] is not None:
        return res
    buf, recs = reads(texts, mode)
    cuts, err = oracle_cuts(params_tuple, buf, recs)
    if err is not None:
        res["range"] = err
        return res
    res["texts"], res["index"] = emit(buf, recs, cuts, mode)
    return res
