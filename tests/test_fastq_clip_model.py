"""tests/fastq_clip_model.py pinned three ways: by a truth table written out by hand, by the truncated-text identity (the
clipped call on a text is the plain call on the text whose hit reads were cut to p bytes) on the golden inputs and on a
hundred drawn texts, and by stats counted from the texts with bytes.find.  No device."""
import os

import numpy as np
import pytest

import fastq_adapters_model as am
import fastq_clip_model as clm
import fastq_model as fm
import fastq_report_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
MODES = ("se", "pe_split", "pe_interleaved", "pe_combo_all")
QUALTYPES = ("phred", "sanger", "solexa", "illumina")
GOLDEN_SET = clm.make_set([clm.TRUSEQ], 13, 0)
GOLDEN = [("se", ["test.fastq"]), ("se", ["problem1.fastq"]), ("pe_split", ["test.f.fastq", "test.r.fastq"]),
          ("pe_interleaved", ["test.fastq"]), ("pe_combo_all", ["test.fastq"]), ("se", ["test.f.fastq"]),
          ("se", ["test.r.fastq"])]
GOLDEN_PARAMS = ("sanger", 20, 20, False, False)


def golden_texts(names):
    return [open(os.path.join(INPUTS, n), "rb").read() for n in names]


# ---- the truth table ------------------------------------------------------------------------------------------------------
def test_truth_hits_by_hand():
    st = clm.make_set(**clm.TRUTH_SET)
    assert [am.hit_of(r, st) for r in clm.TRUTH_READS] == [(0, 0, 13, 0), None, (0, 10, 13, 0), (0, 0, 13, 0), None,
                                                             (0, 12, 5, 0), (0, 4, 13, 0), (0, 0, 13, 0)]
    assert am.hit_of(clm.TRUTH_READS[5][:-1], st) is None  # one base less and the last start holds four bases: no hit


@pytest.mark.parametrize("qualtype", QUALTYPES)
@pytest.mark.parametrize("mode", MODES)
def test_truth_table(mode, qualtype):
    texts, want_texts, want_index = clm.truth(qualtype, mode)
    got = clm.expected(clm.truth_params(qualtype), texts, mode, clm.make_set(**clm.TRUTH_SET))
    assert got["verdict"] is None and got["range"] is None
    assert got["texts"] == want_texts
    assert [None if ix is None else list(ix) for ix in got["index"]] == want_index
    assert got["clip"] == clm.TRUTH_STATS and got["words"] == clm.TRUTH_WORDS
    # the lengths the scan saw, and with them -l: the read clipped to four bases is not kept, nor are the emptied ones
    assert list(np.diff(got["batch"][2].astype(np.int64))) == [0, 16, 10, 0, 16, 12, 4, 0]
    assert [int(c) for c in got["cuts"][:, 1]] == [-1, 16, 10, -1, 16, 12, -1, -1]


@pytest.mark.parametrize("qualtype", QUALTYPES)
def test_truth_range_behind_and_in_front(qualtype):
    st = clm.make_set(**clm.TRUTH_SET)
    text, want, bad = clm.truth_range(qualtype, front=False)
    got = clm.expected(clm.truth_params(qualtype), [text], "se", st)
    assert got["range"] is None and got["texts"][0] == want and got["clip"]["bases_clipped"] == 13
    assert fm.expected(clm.truth_params(qualtype), [text], "se")["range"] is not None  # unclipped, the byte is an error
    text, want, bad = clm.truth_range(qualtype, front=True)
    got = clm.expected(clm.truth_params(qualtype), [text], "se", st)
    assert got["texts"] is None and got["clip"] == clm.failed()
    assert tuple(int(x) for x in got["range"][:3]) == (0, 3, bad)


@pytest.mark.parametrize("qualtype", QUALTYPES)
def test_truth_n_behind_and_in_front(qualtype):
    text, want = clm.truth_n(qualtype)
    got = clm.expected(clm.truth_params(qualtype, True), [text], "se", clm.make_set(**clm.TRUTH_SET))
    assert got["texts"][0] == want and got["words"] == [10, 10, 10]
    assert [tuple(int(x) for x in c) for c in got["cuts"]] == [(0, 10), (-1, -1), (0, 5)]
    # unclipped, the N behind the clip point discards the first read too
    assert [int(c) for c in fm.oracle_cuts(clm.truth_params(qualtype, True), *fm.reads([text], "se"))[0][:, 1]] == [-1, -1, 5]


def test_emptied_read_is_no_format_error():
    """SK_FQ_SEQ_EMPTY stays a property of the text alone: a read that is all adapter gives no verdict"""
    text = b"@a\n" + clm.TRUSEQ + b"\n+\n" + b"I" * 13 + b"\n"
    got = clm.expected(("sanger", 20, 0, False, False), [text], "se", clm.make_set(**clm.TRUTH_SET))
    assert got["verdict"] is None and got["texts"][0] == b"" and got["clip"]["reads_emptied"] == 1
    assert clm.truncated([text], "se", clm.make_set(**clm.TRUTH_SET)) is None


# ---- the truncated-text identity ------------------------------------------------------------------------------------------
def identity(ptuple, texts, mode, st):
    """-> whether the input could be truncated; asserts the identity where it could"""
    cut = clm.truncated(texts, mode, st)
    if cut is None:
        return False
    got = clm.expected(ptuple, texts, mode, st)
    if mode == "pe_combo_all":
        import combo_all_model as cm
        want = cm.expected(ptuple, cut[0])
    else:
        want = fm.expected(ptuple, cut, mode)
    for k in ("records_in", "tail_lines", "dropped_unpaired", "verdict", "texts"):
        assert got[k] == want[k], k
    assert (got["range"] is None) == (want["range"] is None)
    if got["range"] is not None:
        assert tuple(got["range"]) == tuple(want["range"])
    else:
        for a, b in zip(got["index"], want["index"]):
            assert (a is None) == (b is None) and (a is None or np.array_equal(a, b))
    return True


@pytest.mark.parametrize("mode,names", GOLDEN, ids=["%s-%s" % (m, n[0]) for m, n in GOLDEN])
def test_identity_on_the_golden_inputs(mode, names):
    assert identity(GOLDEN_PARAMS, golden_texts(names), mode, GOLDEN_SET), "a golden input holds a read that is all adapter"


def test_identity_on_a_hundred_drawn_texts():
    st = clm.make_set(**clm.DRAWN_SET)
    skipped, clipped, modes = [], 0, set()
    for seed in range(100):
        ptuple, texts, mode = clm.drawn(seed)
        if not identity(ptuple, texts, mode, st):
            skipped.append(seed)
        clipped += clm.expected(ptuple, texts, mode, st)["clip"]["reads_clipped"]
        modes.add(mode)
    assert skipped == [], "none of the chosen inputs may be skipped"
    assert clipped > 300 and modes == set(MODES)  # the planting took, in every mode


# ---- the stats, counted from the texts -------------------------------------------------------------------------------------
def stats_by_find(texts, mode):
    """the stats for one exact adapter with min_overlap = its length: the lowest start is bytes.find's"""
    buf, recs = fm.reads(texts, clm.FRAMING[mode])
    data = bytes(buf)
    r = dict(clm.zero(), calls=1)
    for e0, e1 in zip(recs["e0"], recs["e1"]):
        line = data[int(e0) + 1:int(e1)].upper()
        at = line.find(clm.TRUSEQ)
        r["reads"] += 1
        if at >= 0:
            r["reads_clipped"] += 1
            r["reads_emptied"] += at == 0
            r["bases_clipped"] += len(line) - at
            r["hits"][0] += 1
    return r


@pytest.mark.parametrize("mode,names", GOLDEN, ids=["%s-%s" % (m, n[0]) for m, n in GOLDEN])
def test_stats_on_the_golden_inputs(mode, names):
    texts = golden_texts(names)
    got = clm.expected(GOLDEN_PARAMS, texts, mode, GOLDEN_SET)
    assert got["clip"] == stats_by_find(texts, mode)
    # the report behind the clip: bases_in after the clip, the difference is bases_clipped
    plain = rm.report(GOLDEN_PARAMS, texts, mode)
    assert clm.report(got, mode)["bases_in"] + got["clip"]["bases_clipped"] == plain["bases_in"]


def test_stats_on_drawn_texts():
    st = clm.make_set(**clm.DRAWN_SET)
    for seed in range(0, 100, 5):
        ptuple, texts, mode = clm.drawn(seed)
        got = clm.expected(ptuple, texts, mode, st)
        if got["range"] is None:
            assert got["clip"] == stats_by_find(texts, mode), seed


def test_add_and_failed():
    a = clm.add(clm.TRUTH_STATS, clm.failed())
    assert a["calls"] == 1 and a["calls_failed"] == 1 and a["hits"][0] == 6
    assert clm.add(a, clm.TRUTH_STATS)["bases_clipped"] == 2 * 82
