"""tests/fastq_rejects_model.py pinned four ways: by a truth table written out by hand, by conservation against the
reference's recorded runs (tests/golden/e2e.json), by an identity that needs no model of the trim (with -l above every
read length the rejects ARE the input), and by the report's model on drawn texts.  No device."""
import collections
import hashlib
import os
import re

import numpy as np
import pytest

import fastq_model as fm
import fastq_rejects_model as jm
import fastq_report_model as rm
import trim_model as tm
from test_fastq_report_model import golden_case, golden_tmp  # noqa: F401 (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")

# ---- the hand truth table ---------------------------------------------------------------------------------------------------
# Under ("sanger", 20, 5, ..): 'I' is quality 40, '#' quality 2 (test_fastq_report_model.py has the cuts by hand).  A record
# here is its four lines; K is kept, X is not.
P5 = ("sanger", 20, 5, False, False)
P1 = ("sanger", 20, 1, False, False)
# phred: quality = the byte, 4..60, so a '\r' (13) in the quality line is a low base and no range error; '(' is 40
PH = ("phred", 20, 5, False, False)


def K(name, plus=b"+"):
    return (b"@" + name, b"ACGTACGTACGT", plus, b"IIIIIIIIII##")


def X(name, plus=b"+"):
    return (b"@" + name, b"ACGTACGTACG", plus, b"###########")


def text_of(records, last_newline=True):
    out = b"".join(line + b"\n" for r in records for line in r)
    return out if last_newline else out[:-1]


def want_of(records, chosen):
    """the rejects text by the rule as it is written: the four lines of each chosen record, each with its '\\n'"""
    return b"".join(line + b"\n" for k in chosen for line in records[k])


PAIRS = [K(b"a/1"), K(b"a/2"), K(b"b/1"), X(b"b/2"), X(b"c/1"), K(b"c/2"), X(b"d/1"), X(b"d/2")]
CR_K = (b"@k\r", b"ACGTACGTACG\r", b"+\r", b"(((((((((((\r")
CR_X = (b"@x comment\r", b"ACGTACGTACG\r", b"+x\r", b"\x05\x05\x05\x05\x05\x05\x05\x05\x05\x05\x05\r")
ONE = (b"@one", b"A", b"+", b"I")
LONG_PLUS = b"+" + b"p" * 300
# (id, params, texts by mode, the records in read order, the reads of the call, rejected by hand, rejected with PAIRS)
TABLE = [
    ("four_patterns", P5, PAIRS, 8, [3, 4, 6, 7], [2, 3, 4, 5, 6, 7]),
    ("all_kept", P5, [K(b"a"), K(b"b")], 2, [], []),
    ("none_kept", P5, [X(b"a"), X(b"b")], 2, [0, 1], [0, 1]),
    ("cr_in_every_line", PH, [CR_K, CR_X], 2, [1], [0, 1]),
    ("cr_both_lost", PH, [CR_X, CR_X], 2, [0, 1], [0, 1]),
    ("one_base_lost", P5, [K(b"a"), ONE], 2, [1], [0, 1]),
    ("one_base_kept", P1, [X(b"a"), ONE], 2, [0], [0, 1]),
    ("empty_plus", P5, [X(b"a", b""), K(b"b", b"")], 2, [0], [0, 1]),
    ("long_plus", P5, [K(b"a", LONG_PLUS), X(b"b", LONG_PLUS)], 2, [1], [0, 1]),
]


def texts_for(records, mode, last_newline=True):
    if mode == "pe_split":
        return [text_of(records[0::2], last_newline), text_of(records[1::2], last_newline)]
    return [text_of(records, last_newline)]


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
@pytest.mark.parametrize("mode", jm.MODES)
def test_hand_truth_table(case, mode):
    _, params, records, reads, lost, lost_pairs = case
    for pairs in ((False,) if mode == "se" else (False, True)):
        chosen = lost_pairs if pairs else lost
        r = jm.rejects(params, texts_for(records, mode), mode, pairs)
        want = want_of(records, chosen)
        assert r["text"] == want and r["index"].tolist() == chosen
        assert (r["records"], r["bytes"], r["reads"], r["valid"]) == (len(chosen), len(want), reads, 1)


def test_hand_unterminated_last_line():
    """a rejected last record whose quality line has no '\\n' gains it; so does each text of a split pair"""
    records = [K(b"a"), X(b"b")]
    r = jm.rejects(P5, [text_of(records, last_newline=False)], "se")
    assert r["text"] == want_of(records, [1]) and r["bytes"] == len(text_of([X(b"b")]))
    pair = [X(b"a/1"), X(b"a/2")]
    for pairs in (False, True):
        r = jm.rejects(P5, texts_for(pair, "pe_split", last_newline=False), "pe_split", pairs)
        assert r["text"] == want_of(pair, [0, 1]) and r["bytes"] == len(text_of(pair))
    # a kept unterminated last record: nothing of it
    assert jm.rejects(P5, [text_of([X(b"a"), K(b"b")], last_newline=False)], "se")["text"] == want_of([X(b"a")], [0])


def test_hand_odd_record():
    """the odd last record of an interleaved text is no read: it is not in the rejects though nothing kept it"""
    records = [K(b"a/1"), X(b"a/2"), X(b"odd")]
    for mode in ("pe_interleaved", "pe_combo_all"):
        r = jm.rejects(P5, [text_of(records)], mode)
        assert (r["text"], r["reads"], r["index"].tolist()) == (want_of(records, [1]), 2, [1])
        r = jm.rejects(P5, [text_of(records)], mode, pairs=True)
        assert (r["text"], r["reads"], r["index"].tolist()) == (want_of(records, [0, 1]), 2, [0, 1])
    assert jm.rejects(P5, [text_of(records)], "se")["index"].tolist() == [1, 2]


def test_hand_void_calls_and_pairs_with_se():
    bad_format = text_of([X(b"a")]) + b"@x\n\n+\n\n"
    bad_range = text_of([X(b"a"), (b"@r", b"ACGTACGTACGT", b"+", b"\xc8IIIIIIIIIII")])
    for text in (bad_format, bad_range):
        assert jm.equal(jm.rejects(P5, [text], "se"), jm.void()) == []
    empty = jm.rejects(P5, [b""], "se")
    assert (empty["text"], empty["valid"], empty["reads"]) == (b"", 1, 0)
    with pytest.raises(ValueError):
        jm.rejects(P5, [text_of(PAIRS)], "se", pairs=True)


def test_hand_pieces_concatenate():
    """the piece form: whatever the pieces take, as long as pairs stay whole, the texts concatenated are the whole call's"""
    whole = jm.rejects(P5, [text_of(PAIRS)], "pe_interleaved", pairs=True)
    for takes in ([8], [2, 6], [2, 2, 2, 2], [4, 0, 4]):
        parts = jm.pieces(P5, [text_of(PAIRS)], "pe_interleaved", takes, pairs=True)
        assert b"".join(p["text"] for p in parts) == whole["text"]
        assert np.concatenate([p["index"] for p in parts]).tolist() == whole["index"].tolist()
        assert sum(p["reads"] for p in parts) == 8


# ---- conservation against the reference's recorded runs ---------------------------------------------------------------------
REPLAYABLE = [name for name, _ in tm.golden_runs() if name not in tm.UNREPLAYABLE]
FILES = {"pe_split": {"o1.fastq": 0, "o2.fastq": 1, "os.fastq": 2}, "pe_interleaved": {"om.fastq": 0, "os.fastq": 2}}


def names_of(text):
    """the multiset of the name lines of a FASTQ text"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return collections.Counter(lines[0::4])


def recorded(stdout, what):
    return int(re.search(r"FastQ %s: (\d+)" % what, stdout).group(1))


def test_replayable_runs_are_the_recorded_ones():
    assert len(REPLAYABLE) == 18 and "pe_problem1_inter" not in REPLAYABLE


@pytest.mark.parametrize("name", REPLAYABLE)
def test_conservation_against_golden_runs(golden_tmp, name):
    """What the reference wrote plus the rejects is what it read.  The reference's output files are the emission model's
    texts, held here to the recorded md5 and size of each file.  A run without -s has no file for its kept singles: the
    reference drops them too, so they are added from the model, their number held to the recorded summary line."""
    params, texts, mode, n_reads, stdout = golden_case(golden_tmp, name)
    assert n_reads is None
    rec = dict(tm.golden_runs())[name]
    res = fm.expected(params, texts, mode)
    written = collections.Counter()
    for fname, o in FILES[mode].items():
        if fname in rec["outputs"]:
            got, want = res["texts"][o], rec["outputs"][fname]
            assert (hashlib.md5(got).hexdigest(), len(got)) == (want["md5"], want["size"]), fname
        else:
            assert fname == "os.fastq" and len(res["index"][o]) == recorded(stdout, "single records kept")
        written += names_of(res["texts"][o])
    r = jm.rejects(params, texts, mode)
    assert r["valid"] == 1
    read = collections.Counter()
    for t in texts:
        read += names_of(t)
    assert written + names_of(r["text"]) == read
    kept = recorded(stdout, "paired records kept") + recorded(stdout, "single records kept")
    assert r["records"] + kept == r["reads"] == sum(read.values())
    assert r["records"] == recorded(stdout, "paired records discarded") + recorded(stdout, "single records discarded")


# ---- a model-free identity --------------------------------------------------------------------------------------------------
GOLDEN_INPUTS = ["test.fastq", "test.f.fastq", "test.r.fastq", "problem1.fastq"]


def _read(name):
    return open(os.path.join(INPUTS, name), "rb").read()


def interleave(a, b):
    """the record-wise interleaving of two FASTQ texts that end in '\\n'"""
    la, lb = a.split(b"\n")[:-1], b.split(b"\n")[:-1]
    assert len(la) == len(lb) and len(la) % 4 == 0
    out = []
    for k in range(0, len(la), 4):
        out += la[k:k + 4] + lb[k:k + 4]
    return b"".join(line + b"\n" for line in out)


@pytest.mark.parametrize("name", GOLDEN_INPUTS)
def test_everything_rejected_is_the_input(name):
    """-l above every read length: every read is rejected whatever its qualities (the reference src/trim.cpp discards on the
    length alone), so the rejects text is the input text"""
    text = _read(name)
    assert text.endswith(b"\n")
    f = fm.frame(text)
    params = ("sanger" if name == "problem1.fastq" else "illumina", 20, int((f["e3"] - f["e2"]).max()) + 1, False, False)
    r = jm.rejects(params, [text], "se")
    assert r["text"] == text and r["records"] == r["reads"] == f["records"] and r["bytes"] == len(text)
    if f["records"] % 2 == 0:
        for mode in ("pe_interleaved", "pe_combo_all"):
            for pairs in (False, True):
                assert jm.rejects(params, [text], mode, pairs)["text"] == text


def test_everything_rejected_split_is_the_interleaving():
    a, b = _read("test.f.fastq"), _read("test.r.fastq")
    for pairs in (False, True):
        r = jm.rejects(("illumina", 20, 1000, False, False), [a, b], "pe_split", pairs)
        assert r["text"] == interleave(a, b) and r["bytes"] == len(a) + len(b)
        assert r["index"].tolist() == list(range(r["reads"]))


# ---- the report's model on drawn texts --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn_results():
    out = []
    for c in jm.drawn():
        out.append((c, jm.rejects(tuple(c["params"]), c["texts"], c["mode"], c["pairs"]),
                    jm.rejects(tuple(c["params"]), c["texts"], c["mode"], False)))
    return out


def test_drawn_texts_against_the_report(drawn_results):
    """records == the report's discarded, bytes == the line lengths of the discarded reads with their four '\\n'"""
    for c, _, r in drawn_results:
        rep = rm.report(tuple(c["params"]), c["texts"], c["mode"], 0, 0)
        assert r["valid"] == rep["calls"] and (not r["valid"]) == rep["calls_failed"]
        if not r["valid"]:
            assert jm.equal(r, jm.void()) == []
            continue
        assert r["records"] == rep["discarded"] and r["reads"] == rep["reads"]
        buf, recs = fm.reads(c["texts"], c["mode"])
        lines = [recs["e0"] - recs["s0"], recs["e1"] - recs["e0"] - 1, recs["e2"] - recs["e1"] - 1, recs["e3"] - recs["e2"] - 1]
        per_read = sum(lines) + 4
        assert r["bytes"] == int(per_read[r["index"]].sum()) == len(r["text"])
        assert int(lines[3][r["index"]].sum()) == rep["bases_discarded"]


def test_drawn_texts_pairs_hold_the_plain_rejects(drawn_results):
    for c, p, r in drawn_results:
        if not c["pairs"] or not r["valid"]:
            continue
        assert set(r["index"].tolist()) <= set(p["index"].tolist())
        idx = p["index"]
        assert len(idx) % 2 == 0 and np.array_equal(idx[0::2] + 1, idx[1::2]) and not np.any(idx[0::2] & 1)


def test_drawn_texts_are_worth_running(drawn_results):
    assert len(drawn_results) == jm.DRAWN == 100
    assert sum(1 for _, _, r in drawn_results if not r["valid"]) <= 30
    assert sum(1 for _, p, _ in drawn_results if len(p["text"]) > 0) >= 50
