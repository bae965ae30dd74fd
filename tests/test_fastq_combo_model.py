"""CPU: the model of mode "pe_combo_all" (tests/combo_all_model.py) that the GPU tests compare against, pinned three ways
(a truth table written out by hand, the quality constants of the library, the reference's recorded -c runs), and the
record rule of sickle_amd/csrc/sk_fastq_record.h run on the host against it (tests/fastq_combo: a stand-alone program,
plain and under the address and undefined-behaviour sanitizers)."""
import hashlib
import os
import random
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

import combo_all_model as cm
import cli_util as cu
import fastq_model as fm
import fastq_order_model as om
import fastq_piece_model as pm
import trim_model as tm
from sickle_amd import capi
from test_fastq_api import golden_texts

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_combo")

# sanger, -q 20 -l 5: I = 40, # = 2
TRUTH_IN = (
    b"@p0/1 first\nACGTACGTAC\n+p0/1 first\nIIIIIIII##\n"   # kept (its last two bases go), '+' comment stays
    b"@p0/2\nACGTACGTAC\n+\nIIIIIIIIII\n"                     # kept whole
    b"@p1/1\r\nACGTAC\n+p1/1\r\nIIIIII\n"                     # kept, a '\r' in the name and in the '+' line
    b"@p1/2 lost\r\nACGTACGTAC\n+p1/2 lost\n##########\n"     # failed: name line verbatim, a bare '+'
    b"@p2/1\nA\n\n#\n"                                        # failed: one base, an empty '+' line: N record one byte longer
    b"@p2/2 c\nACGTACG\n+c\nIIIIIII\n"                        # kept
    b"@p3/1\nACGT\n+\nIIII\n"                                 # failed: shorter than -l
    b"@p3/2\nACGTACGT\n+x\n########\n"                        # failed
    b"@odd\nACGTACGT\n+\nIIIIIIII\n"                          # no mate: checked, dropped
)
TRUTH_OUT = [
    b"@p0/1 first\nACGTACGT\n+p0/1 first\nIIIIIIII\n" b"@p0/2\nACGTACGTAC\n+\nIIIIIIIIII\n",
    b"@p1/1\r\nACGTAC\n+p1/1\r\nIIIIII\n" b"@p1/2 lost\r\nN\n+\n!\n",
    b"@p2/1\nN\n+\n!\n" b"@p2/2 c\nACGTACG\n+c\nIIIIIII\n",
    b"@p3/1\nN\n+\n!\n" b"@p3/2\nN\n+\n!\n",
]


def test_truth_table_by_hand():
    want = cm.expected(cm.TRUTH_PARAMS, TRUTH_IN)
    assert want["verdict"] is None and want["range"] is None
    assert want["pairs"] == TRUTH_OUT
    assert want["texts"] == [b"".join(TRUTH_OUT), None, None]
    assert want["classes"].tolist() == [0, 1, 2, 3]
    assert want["records_in"] == [9, 0] and want["dropped_unpaired"] == 1
    assert want["index"][0].tolist() == list(range(8))
    # the N record of the 1-base read with an empty '+' line is one byte longer than the record
    assert len(b"@p2/1\nN\n+\n!\n") == len(b"@p2/1\nA\n\n#\n") + 1
    # the other three qualities' Q, and the generated truth table has the classes it says
    for qt, q in (("phred", b"\x04"), ("solexa", b":"), ("illumina", b"@")):
        got = cm.expected((qt, 20, 5, False, False), cm.truth_text(4, 7, qt))
        assert got["classes"].tolist() == [0, 1, 2, 3]
        assert got["records"][3].endswith(b"\nN\n+\n" + q + b"\n") and got["records"][4].endswith(b"\nN\n+\n" + q + b"\n")
    for name_len in range(2, 35):
        text = cm.truth_text(5, name_len)
        got = cm.expected(cm.TRUTH_PARAMS, text)
        assert got["classes"].tolist() == [0, 1, 2, 3, 0]
        assert all(text.startswith(b"@") and len(r.split(b"\n")[0]) == name_len for r in got["records"])


def test_q_is_the_librarys_lowest_quality():
    L = capi.lib()
    for qt, code in capi.QUALTYPES.items():
        assert cm.Q_BYTE[qt] == L.sk_quality_constants(code)[1], qt
    assert cm.Q_BYTE == {"phred": 4, "sanger": 33, "solexa": 58, "illumina": 64}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_combo_model")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


# (the replayable ones: tm.golden_params() marks the run whose reader takes no record, which has nothing to tie to)
COMBO_RUNS = [p for p in tm.golden_params() if "-c" in p.values[1]["argv"] and not p.marks]


@pytest.mark.parametrize("name,rec", COMBO_RUNS)
def test_model_is_tied_to_the_reference_runs(workdir, name, rec):
    """Every recorded -c run of the reference: the model's records of the pairs with both mates kept are om.fastq, the kept
    records of the pairs with one mate kept are os.fastq (md5 and size), and nothing else but N records is in the text."""
    mode, texts, files = golden_texts(rec["argv"], workdir)
    assert mode == "pe_interleaved"
    ptuple = tm.run_params(rec["argv"])
    want = cm.expected(ptuple, texts[0])
    assert want["verdict"] is None and want["range"] is None
    recs, cls, kept = want["records"], want["classes"], want["cuts"][:, 1] >= 0
    assert len(recs) == 2 * (want["records_in"][0] // 2)
    both = b"".join(recs[2 * k] + recs[2 * k + 1] for k in np.flatnonzero(cls == 0))
    single = b"".join(recs[2 * k + (0 if cls[k] == 1 else 1)] for k in np.flatnonzero((cls == 1) | (cls == 2)))
    assert "om.fastq" in rec["outputs"]
    for fname, text in (("om.fastq", both), ("os.fastq", single)):
        if fname not in rec["outputs"]:
            continue  # a run without -s records no singles file
        w = rec["outputs"][fname]
        assert (hashlib.md5(text).hexdigest(), len(text)) == (w["md5"], w["size"]), fname
    q = bytes([cm.Q_BYTE[ptuple[0]]])
    for r in np.flatnonzero(~kept):
        head, tail = recs[r].split(b"\n", 1)
        assert tail == b"N\n+\n" + q + b"\n" and texts[0].count(head + b"\n") >= 1
    assert sum(len(r) for r in recs) == len(want["texts"][0]) <= cm.bound(len(texts[0]), len(recs))


def test_model_in_pieces_and_in_order():
    """The per-pair strings joined through the take rule of a piece and in read_order are the streamed and the -a T texts:
    each piece of fastq_piece_model's stream frames the pairs the whole text has, in order."""
    text = cm.truth_text(41, 9) + b"@odd\nACGTACGT\n+\nIIIIIIII\n"
    want = cm.expected(cm.TRUTH_PARAMS, text)
    at, carried, pos, pieces = 0, b"", 0, 0
    while True:
        carried += text[pos:pos + 300]
        pos += 300
        more = pos < len(text)
        p = pm.piece(cm.TRUTH_PARAMS, [carried], cm.FRAMING, more)
        u = p["records_in"][0] - p["dropped_unpaired"]
        assert u % 2 == 0 and (u == pm.take([carried.count(b"\n") // 4], cm.FRAMING) or not more)
        # the piece's own text, as the mode gives it on the window, is the next u records of the whole text's
        assert cm.expected(cm.TRUTH_PARAMS, carried[:p["consumed"][0]])["texts"][0] == b"".join(want["records"][at:at + u])
        at, carried, pieces = at + u, carried[p["consumed"][0]:], pieces + 1
        if not more:
            break
    assert at == len(want["records"]) == 82 and pieces > 5 and p["dropped_unpaired"] == 1
    for threads in (1, 3, 16):
        got, order, counts = cm.ordered(cm.TRUTH_PARAMS, text, threads, 1000)
        assert counts["batches"] >= 3 and sorted(order.tolist()) == list(range(len(order)))
        assert (got == want["texts"][0][:len(got)]) == (order.tolist() == sorted(order.tolist())) == (threads != 3)
        # the interleaved mode's ordered output 0 is this text without the pairs that are not kept/kept
        ref = om.expected(cm.TRUTH_PARAMS, [text], cm.FRAMING, threads, 1000)
        assert b"".join(want["pairs"][r >> 1] for r in order[0::2] if want["classes"][r >> 1] == 0) == ref["texts"][0]


# ---- the record rule on the host --------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["combo_host", "combo_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def _padded(b):
    return struct.pack("<Q", len(b)) + b + b"\0" * (-len(b) % 8)


def host_case(ptuple, text, combo_all=True):
    """one case of tests/fastq_combo/combo_host.cpp: the text, its framed reads with the oracle's cuts, the model's text"""
    want = cm.expected(ptuple, text)
    _, recs = fm.reads([text], cm.FRAMING)
    out = [_padded(text), struct.pack("<QQQ", len(want["cuts"]), cm.Q_BYTE[ptuple[0]], int(combo_all))]
    for r, (five, three) in enumerate(want["cuts"].tolist()):
        out.append(struct.pack("<5Q2q", *(int(recs[k][r]) for k in ("s0", "e0", "e1", "e2", "e3")), five, three))
    model = want["texts"][0] if combo_all else b"".join(x for x, c in zip(want["records"], want["cuts"]) if c[1] >= 0)
    out.append(_padded(model))
    return b"".join(out)


def test_record_rule_on_the_host(tool, tmp_path):
    cases = [host_case(cm.TRUTH_PARAMS, TRUTH_IN), host_case(cm.TRUTH_PARAMS, TRUTH_IN[:-1]),  # the last line unterminated
             host_case(cm.TRUTH_PARAMS, TRUTH_IN, combo_all=False), host_case(cm.TRUTH_PARAMS, b"")]
    for qt in capi.QUALTYPES:
        for name_len in (2, 3, 9, 15, 16, 17, 34):
            cases.append(host_case((qt, 20, 5, False, False), cm.truth_text(4, name_len, qt, crlf_names=name_len == 9)))
    cases.append(host_case(cm.TRUTH_PARAMS, b"@a\nA\n\n#\n" * 64))  # every record one byte longer: the bound is met
    src = tmp_path / "cases.bin"
    src.write_bytes(struct.pack("<Q", len(cases)) + b"".join(cases))
    pr = subprocess.run([tool, str(src)], capture_output=True)
    assert pr.returncode == 0, pr.stderr.decode()
    assert pr.stdout.split()[:2] == [b"ok", b"%d" % len(cases)]
    # the program sees a wrong text
    bad = host_case(cm.TRUTH_PARAMS, TRUTH_IN).replace(b"N\n+\n!\n", b"N\n+\n#\n", 1)
    src.write_bytes(struct.pack("<Q", 1) + bad)
    assert subprocess.run([tool, str(src)], capture_output=True).returncode == 1


# ---- the drawn texts of the GPU test ----------------------------------------------------------------------------------
SEED, DRAWS = 20240, 100


def drawn_case(rng):
    """One interleaved text for the randomized GPU test: up to 300 records, read lengths 1..80, names of 2..40 bytes, '+'
    lines empty, bare or with a comment, qualities (never byte 10) drawn so that each pair class occurs.
    -> (ptuple, text, threads, batch_len)"""
    n = rng.randrange(0, 301)
    top = rng.choice([1, 2, 5, 18, 40, 80])
    qt = rng.choice(sorted(cm.Q_BYTE))
    lo = cm.Q_BYTE[qt]
    good, poor = lo + 40, (lo + 2 if lo + 2 != 10 else lo + 3)
    longest, recs = 1, []
    for k in range(n):
        length = rng.randrange(1, top + 1)
        name = b"@" + (b"%d" % k).rjust(rng.randrange(1, 40), b"n") + (b"\r" if rng.random() < 0.05 else b"")
        kind = rng.random()
        if kind < 0.35:
            qual = bytes([poor]) * length
        elif kind < 0.7:
            qual = bytes([good]) * length
        else:
            qual = bytes(rng.choice((poor, good, lo + 20)) for _ in range(length))
        plus = rng.choice((b"", b"+", b"+" + name[1:]))
        longest = max(longest, length, len(name), len(plus))
        recs.append(name + b"\n" + bytes(rng.choice(b"ACGTN") for _ in range(length)) + b"\n" + plus + b"\n" + qual + b"\n")
    text = b"".join(recs)
    if text and rng.random() < 0.2:
        text = text[:-1]
    floor = max(20, longest + 2)
    batch_len = rng.choice([floor, rng.randrange(floor, 200), rng.randrange(floor, 4001)])
    ptuple = (qt, rng.choice([2, 20, 30]), rng.choice([1, 5, 20]), rng.random() < 0.3, rng.random() < 0.3)
    return ptuple, text, rng.randrange(1, 41), batch_len


def test_the_drawn_cases_hit_every_class():
    """the seed of tests/test_gpu_fastq_combo.py's randomized test draws each of the four pair classes, a text that
    outgrows its input, and none with byte 10 as a quality"""
    rng = random.Random(SEED)
    hit, longer = Counter(), 0
    for _ in range(DRAWS):
        ptuple, text, threads, batch_len = drawn_case(rng)
        want = cm.expected(ptuple, text)
        assert want["verdict"] is None and want["range"] is None
        hit.update(cm.CLASSES[c] for c in want["classes"].tolist())
        longer += len(want["texts"][0]) > len(text)
        assert len(want["texts"][0]) <= cm.bound(len(text), len(want["records"]))
        assert len(want["texts"][0]) <= capi.fastq_output_bound(len(text), cm.MODE)
    print(dict(hit), "texts longer than their input:", longer)
    assert all(hit[c] > 0 for c in cm.CLASSES) and longer > 0
