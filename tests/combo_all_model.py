"""What mode "pe_combo_all" (SK_TRIM_PE_COMBO_ALL, sickle's -M) of the FASTQ text calls has to give (include/sickle_amd.h),
built on the framing and the oracle's cuts of tests/fastq_model.py: every read of every framed pair, a kept one as the
record every mode writes, one that is not kept as its name line and N / + / Q.  Plain Python per record, so that it
shares no code with the emission of fastq_model.emit.  It never reads anything the device made."""
import numpy as np

import fastq_model as fm
import fastq_order_model as om

MODE = "pe_combo_all"
FRAMING = "pe_interleaved"  # input, framing, checks, pieces and units are this mode's
# the lowest quality byte of each type (reference src/sickle.h:85-91), == sk_quality_constants(qualtype)[1]
Q_BYTE = {"phred": 4, "sanger": 33, "solexa": 58, "illumina": 64}
CLASSES = ("kept/kept", "kept/failed", "failed/kept", "failed/failed")


def record(buf, s0, e0, e1, e2, five, three, q):
    """one emitted record (bytes); buf: bytes, with a '\\n' at e0 and at e2"""
    name = buf[s0:e0 + 1]
    if three < 0:
        return name + b"N\n+\n" + bytes([q]) + b"\n"
    return name + buf[e0 + 1 + five:e0 + 1 + three] + b"\n" + buf[e1 + 1:e2 + 1] + buf[e2 + 1 + five:e2 + 1 + three] + b"\n"


def records_of(buf, recs, cuts, qualtype):
    """-> the emitted record of every read, in read order"""
    data, q = bytes(buf), Q_BYTE[qualtype]
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1, 2)
    return [record(data, int(recs["s0"][r]), int(recs["e0"][r]), int(recs["e1"][r]), int(recs["e2"][r]), int(cuts[r, 0]),
                   int(cuts[r, 1]), q) for r in range(len(cuts))]


def pair_class(cuts):
    """class of every pair: index into CLASSES"""
    kept = np.asarray(cuts, dtype=np.int64).reshape(-1, 2)[:, 1] >= 0
    return (2 * (~kept[0::2]).astype(np.int64) + (~kept[1::2]).astype(np.int64))


def expected(ptuple, text):
    """The whole call on one interleaved text: -> fastq_model.expected's dict for the framing mode (verdict, range,
    records_in, tail_lines, dropped_unpaired), with texts = [text0, None, None], index likewise, and, when there is no
    error: pairs (the bytes of every pair, in read order: their join is text0), records (per read), cuts, classes."""
    res = fm.expected(ptuple, [text], FRAMING)
    res["pairs"] = res["records"] = res["cuts"] = res["classes"] = None
    if res["verdict"] is not None or res["range"] is not None:
        res["texts"] = res["index"] = None
        return res
    buf, recs = fm.reads([text], FRAMING)
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    assert err is None
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1, 2)
    rec = records_of(buf, recs, cuts, ptuple[0])
    res["records"], res["cuts"], res["classes"] = rec, cuts, pair_class(cuts)
    res["pairs"] = [rec[2 * k] + rec[2 * k + 1] for k in range(len(rec) // 2)]
    res["texts"] = [b"".join(res["pairs"]), None, None]
    res["index"] = [np.arange(len(rec), dtype=np.int64), None, None]
    return res


def ordered(ptuple, text, threads, batch_len, limit=0):
    """The ordered call on a text without an error: -> (text0, index0, order counts): the records of the reads inside the
    reference's batches, in its -a threads order (fastq_order_model.read_order)."""
    want = expected(ptuple, text)
    assert want["texts"] is not None and om.long_line([text], batch_len) is None
    tabs = om.batch_tables([om.lines_of(text)], FRAMING, batch_len, limit)
    order = om.read_order(tabs["first_unit"], threads, FRAMING)
    assert len(order) == 2 * tabs["units"]
    counts = {"batches": len(tabs["first_unit"]) - 1, "units": tabs["units"], "last_batch_units": tabs["last_batch_units"]}
    return b"".join(want["records"][r] for r in order), order, counts


TRUTH_PARAMS = ("sanger", 20, 5, False, False)


def _name(tag, name_len):
    """a name line of name_len bytes ('@' included) that ends in tag where there is room for it"""
    return b"@" + (b"x" * name_len + tag)[-(name_len - 1):]


def truth_text(n_pairs, name_len, qualtype="sanger", crlf_names=False):
    """n_pairs pairs that walk the four classes kept/kept, kept/failed, failed/kept, failed/failed (pair k has class
    k % 4) under (qualtype, 20, 5, False, False), every name line name_len bytes long (>= 2; a '\\r' at its end on
    demand, which makes it one longer).  Kept reads: 12 bases of which 10 stay, a '+' line with a comment on every other
    one.  Failed reads take turns: 11 bases of the lowest quality with a '+' comment, and one base with an empty '+'
    line (the record an N record is one byte longer than)."""
    lo = Q_BYTE[qualtype]
    hi, low = bytes([lo + 40]), bytes([lo + 2 if lo + 2 != 10 else lo + 3])
    assert 10 not in hi + low
    out, failed = [], 0
    for k in range(n_pairs):
        for mate in (0, 1):
            tag = b"%d/%d" % (k, mate + 1)
            name = _name(tag, name_len) + (b"\r" if crlf_names else b"")
            keep = not ((k % 4) >> (1 - mate)) & 1
            if keep:
                plus = b"+" + (name[1:] if (k + mate) & 1 else b"")
                out.append(name + b"\nACGTNACGTACG\n" + plus + b"\n" + hi * 10 + low * 2 + b"\n")
            elif failed & 1:
                out.append(name + b"\nA\n\n" + low + b"\n")
                failed += 1
            else:
                out.append(name + b"\nACGTACGTACG\n+" + name[1:] + b" lost\n" + low * 11 + b"\n")
                failed += 1
    return b"".join(out)


def bound(text_bytes, records):
    """the most bytes the mode's output can have (include/sickle_amd.h)"""
    return text_bytes + records + 1
