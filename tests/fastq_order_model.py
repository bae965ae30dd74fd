"""What sk_trim_fastq_ordered_device_async has to give (include/sickle_amd.h), from the restatement of the reference's
reader and queues in tests/fastq_util.py (reference_batches, expected_se_output, expected_pe_outputs), the framing of
tests/fastq_model.py and the oracle's cuts.  It never reads anything the device made."""
import numpy as np

import fastq_model as fm
import fastq_util as fu

SK_ELONGLINE = -8
NONE = (1 << 64) - 1
LINES_PER_UNIT = {"se": 4, "pe_split": 4, "pe_interleaved": 8}


def lines_of(text):
    """the lines of a text; a last line without a newline ends at the end of the text"""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def batch_tables(line_lists, mode, batch_len, limit=0):
    """line_lists: the lines (or just their lengths as bytes objects) of each input -> dict(batches: per input the list
    of line lists, first_unit, units, last_batch_units, batched_lines, stopped_on_mismatch)."""
    m = LINES_PER_UNIT[mode]
    per = [fu.reference_batches(lines, batch_len, m) for lines in line_lists]
    n, mismatch = len(per[0]), 0
    if mode == "pe_split":
        n = 0
        while n < len(per[0]) and n < len(per[1]):
            if len(per[0][n]) != len(per[1][n]):
                mismatch = 1
                break
            n += 1
    if limit:
        if n >= limit:
            mismatch = 0  # the call never looks at batch `limit`
        n = min(n, limit)
    per = [p[:n] for p in per]
    sizes = [len(b) // m for b in per[0]]
    return {"batches": per, "first_unit": [int(x) for x in np.concatenate(([0], np.cumsum(sizes)))] if sizes else [0],
            "units": sum(sizes), "last_batch_units": sizes[-1] if sizes else 0,
            "batched_lines": [sum(len(b) for b in p) for p in per], "stopped_on_mismatch": mismatch}


def unit_order(n, threads, se):
    """the units of a batch of n in the order the queues are written (fastq_util.expected_*_output's loops)"""
    out = []
    for q in range(threads):
        out.extend(range((q + threads - 1) % threads if se else q, n, threads))
    return out


def read_order(first_unit, threads, mode):
    """every read inside the batches in emission order, in the library's read numbering"""
    order = []
    for b in range(len(first_unit) - 1):
        base, n = first_unit[b], first_unit[b + 1] - first_unit[b]
        for k in unit_order(n, threads, mode == "se"):
            order.extend([base + k] if mode == "se" else [2 * (base + k), 2 * (base + k) + 1])
    return np.array(order, dtype=np.int64)


def long_line(texts, batch_len):
    """(input, line) of the lowest line of batch_len - 1 bytes or more of the lowest input that has one, or None"""
    for i, t in enumerate(texts):
        for l, line in enumerate(lines_of(t)):
            if len(line) >= batch_len - 1:
                return i, l
    return None


def expected(ptuple, texts, mode, threads, batch_len, limit=0):
    """-> dict(long_line, order: the order counts, verdict, range, texts, index, records_in, tail_lines)."""
    fr = [fm.frame(t) for t in texts]
    res = {"records_in": [f["records"] for f in fr] + [0] * (2 - len(fr)),
           "tail_lines": [f["tail_lines"] for f in fr] + [0] * (2 - len(fr)),
           "long_line": long_line(texts, batch_len), "verdict": None, "range": None, "texts": None, "index": None,
           "error_batch": NONE}
    tabs = batch_tables([lines_of(t) for t in texts], mode, batch_len, limit)
    res["tables"] = tabs
    res["order"] = {"batches": len(tabs["first_unit"]) - 1, "units": tabs["units"],
                    "last_batch_units": tabs["last_batch_units"], "stopped_on_mismatch": tabs["stopped_on_mismatch"],
                    "records_unbatched": [res["records_in"][i] - tabs["batched_lines"][i] // 4 if i < len(texts) else 0
                                          for i in range(2)]}
    if res["long_line"] is not None:
        return res
    units, first_unit = tabs["units"], tabs["first_unit"]
    per_unit = 1 if mode == "se" else 2
    n_reads = units * per_unit
    # the records inside the batches, in read order
    buf, recs = fm.reads(texts, mode)
    recs = {k: v[:n_reads] for k, v in recs.items()}
    why = fm.reasons(buf, recs)
    bad = np.flatnonzero(why)
    if len(bad):
        read = int(bad[0])
        i, k = (read & 1, read >> 1) if mode == "pe_split" else (0, read)
        res["verdict"] = (int(why[read]), i, k)
        res["error_batch"] = int(np.searchsorted(first_unit, read // per_unit, side="right") - 1)
        return res
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    if err is not None:
        res["range"] = tuple(int(x) for x in err)
        res["error_batch"] = int(np.searchsorted(first_unit, int(err[0]) // per_unit, side="right") - 1)
        return res
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1, 2)
    order = read_order(first_unit, threads, mode)
    assert len(order) == n_reads
    permuted = {k: v[order] for k, v in recs.items()}
    out_texts, index = fm.emit(buf, permuted, cuts[order], mode)
    res["texts"] = out_texts
    res["index"] = [None if ix is None else order[ix] for ix in index]
    # the same from fastq_util's restatement of the reference's queues
    if all(t.endswith(b"\n") or not t for t in texts):
        if mode == "se":
            want = [b"".join(fu.expected_se_output(tabs["batches"][0], lambda f, r: cuts[r], threads)), None, None]
        elif mode == "pe_split":
            ch = fu.expected_pe_outputs(tabs["batches"][0], tabs["batches"][1], lambda f, r: cuts[2 * r + f], threads)
            want = [b"".join(c[j] for c in ch) for j in range(3)]
        else:
            ch = fu.expected_pe_outputs(tabs["batches"][0], None, lambda f, r: cuts[r], threads, interleaved=True)
            want = [b"".join(c[0] for c in ch), None, b"".join(c[2] for c in ch)]
        assert want == out_texts, "the two restatements of the emission order disagree"
    return res


def random_case(rng):
    """A valid text (or pair of texts) for the randomized tests: up to 300 records, read lengths 1..80, no malformed
    record, no quality out of range, no line of batch_len - 1 bytes or more.  rng: random.Random.
    -> (ptuple, texts, mode, threads, batch_len)"""
    mode = rng.choice(["se", "pe_split", "pe_interleaved"])
    n = rng.randrange(0, 301)
    top = rng.choice([1, 2, 5, 18, 40, 80])
    longest = 1

    def record(k, tag):
        nonlocal longest
        length = rng.randrange(1, top + 1)
        name = b"@%d%s" % (k, tag)
        kind = rng.random()
        if kind < 0.3:
            qual = bytes([35]) * length
        elif kind < 0.6:
            qual = bytes([73]) * length
        else:
            qual = bytes(rng.choice((35, 50, 60, 73)) for _ in range(length))
        seq = bytes(rng.choice(b"ACGTN") for _ in range(length))
        plus = b"+" + (name[1:] if rng.random() < 0.2 else b"")
        longest = max(longest, length, len(name), len(plus))
        return name + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n"

    if mode == "pe_split":
        n2 = n if rng.random() < 0.7 else rng.randrange(0, 301)
        texts = [b"".join(record(k, b"/1") for k in range(n)), b"".join(record(k, b"/2") for k in range(n2))]
    else:
        texts = [b"".join(record(k, b"") for k in range(n))]
    lo = max(20, longest + 2)
    batch_len = rng.choice([lo, rng.randrange(lo, 200), rng.randrange(lo, 4001)])
    ptuple = ("sanger", rng.choice([2, 20, 30]), rng.choice([1, 5, 20]), rng.random() < 0.3, rng.random() < 0.3)
    return ptuple, texts, mode, rng.randrange(1, 41), batch_len
