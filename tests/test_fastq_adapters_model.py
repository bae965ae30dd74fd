"""tests/fastq_adapters_model.py pinned three ways: by a truth table written out by hand, by the golden inputs (numbers
computed from the texts alone, with bytes.find), and by consistency with the report's model.  No device."""
import os

import numpy as np
import pytest

import fastq_adapters_model as am
import fastq_report_model as rm
import soak_fastq
from test_fastq_report_model import GOLDEN_SUMMARY_RUNS, fastq, golden_case, golden_tmp  # noqa: F401 (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
TRUSEQ = b"AGATCGGAAGAGC"
P5 = ("sanger", 20, 5, False, False)
# twelve-base reads under P5 (a window of one base): the cut by hand
ALL = b"IIIIIIIIIIII"     # (0, 12)
END = b"IIIIIIIIII##"     # (0, 10)
HEAD = b"IIIII#######"    # (0, 5)
TAIL = b"#######IIIII"    # (7, 12)
LOW = b"############"     # not kept
NOT = (-1, -1)


def mutated(line, n):
    """line with its first n bases replaced by another base each"""
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    return b"".join(other[b] for b in line[:n]) + line[n:]


def full(v):
    return (b"ACGT" * 16)[:v]


# ---- one line: (id, seqs, min_overlap, permille, line, (a, p, v, m) or None), every result worked out by hand -----------
LINES = [
    ("shorter_than_min_overlap_1", [TRUSEQ], 5, 100, b"A", None),
    ("shorter_than_min_overlap_4", [TRUSEQ], 5, 100, b"AGAT", None),
    ("as_long_as_min_overlap", [TRUSEQ], 5, 100, b"AGATC", (0, 0, 5, 0)),
    ("as_long_as_min_overlap_no_hit", [TRUSEQ], 5, 100, b"AGATG", None),
    ("hit_at_0", [TRUSEQ], 5, 100, TRUSEQ + b"TTTT", (0, 0, 13, 0)),
    ("hit_at_the_last_start", [TRUSEQ], 5, 100, b"TTTTTTTAGATC", (0, 7, 5, 0)),
    ("one_base_behind_the_last_start", [TRUSEQ], 5, 100, b"TTTTTTTTAGAT", None),
    ("lower_case_read", [b"ACGTACGTAC"], 10, 100, b"acgtacgtac", (0, 0, 10, 0)),
    ("lower_case_adapter", [b"acgtacgtac"], 10, 100, b"ACGTACGTAC", (0, 0, 10, 0)),
    ("one_N_is_one_mismatch", [b"ACGTACGTAC"], 10, 100, b"ACGTNCGTAC", (0, 0, 10, 1)),
    ("two_N_are_too_many", [b"ACGTACGTAC"], 10, 100, b"ACGTNCGTNC", None),
    ("n_matches_nothing", [b"ACGTACGTAC"], 10, 0, b"ACGTnCGTAC", None),
    ("carriage_return_mismatches", [b"ACGTACGTAC"], 10, 100, b"ACGTACGTA\r", (0, 0, 10, 1)),
    ("carriage_return_at_0_permille", [b"ACGTACGTAC"], 10, 0, b"ACGTACGTA\r", None),
    ("iupac_and_high_bytes", [b"ACGTACGTAC"], 10, 200, b"RCGTACGTA\xc3", (0, 0, 10, 2)),  # 0xc3 & 0xdf = 0xc3, no 'C'
    ("two_adapters_at_one_start", [b"ACGTA", b"ACGTACC"], 5, 0, b"GGACGTACCGG", (0, 2, 5, 0)),
    ("adapter_1_at_a_lower_start", [b"TTTTT", b"GGACG"], 5, 0, b"GGACGTTTTTT", (1, 0, 5, 0)),
    ("adapter_7_alone", [b"CCCCC"] * 7 + [b"GATTACA"], 5, 0, b"AAAGATTACA", (7, 3, 7, 0)),
    ("partial_overlap_at_the_end", [b"GATTACA"], 5, 0, b"CCCCCCCGATTA", (0, 7, 5, 0)),
    ("one_base_adapter", [b"G"], 1, 0, b"ACCGT", (0, 3, 1, 0)),
    ("one_base_adapter_none", [b"G"], 1, 500, b"ACCTT", None),
    # the lowest start wins over a better match further on: 1 of 10 at start 0, 0 of 10 at start 4
    ("lowest_start_wins", [b"ACGTACGTAC"], 10, 100, b"ACGAACGTACGTAC", (0, 0, 10, 1)),
]
# m exactly at, and one above, floor(v / 10) for overlaps of 9, 10, 19, 20 and 64 at 100 permille: 0, 1, 1, 2, 6
for _v, _allow in ((9, 0), (10, 1), (19, 1), (20, 2), (64, 6)):
    assert _allow == _v // 10
    LINES.append(("allowance_v%d_at" % _v, [full(_v)], _v, 100, mutated(full(_v), _allow), (0, 0, _v, _allow)))
    LINES.append(("allowance_v%d_above" % _v, [full(_v)], _v, 100, mutated(full(_v), _allow + 1), None))
# the same through a partial overlap: a 64-base adapter of which the line's last 19 and 20 bases are the head
for _v, _allow in ((19, 1), (20, 2)):
    _line = b"T" * 30 + mutated(full(64)[:_v], _allow)
    LINES.append(("allowance_partial_v%d_at" % _v, [full(64)], 19, 100, _line, (0, 30, _v, _allow)))
    LINES.append(("allowance_partial_v%d_above" % _v, [full(64)], 19, 100, b"T" * 30 + mutated(full(64)[:_v], _allow + 1), None))


@pytest.mark.parametrize("case", LINES, ids=[c[0] for c in LINES])
def test_hand_lines(case):
    _, seqs, mo, pm, line, want = case
    assert am.hit_of(line, am.make_set(seqs, mo, pm)) == want


# ---- whole calls by hand --------------------------------------------------------------------------------------------------
GAT = am.make_set([b"GATTACA"], 5, 0)
#        seq               qual  cut        hit (a, p, v, m)   three - max(p, five) where the hit is in the output
READS = [(b"ACGTAGATTACA", ALL),   # (0, 12)  (0, 5, 7, 0)       7: the cut behind the hit
         (b"CCCCCGATTACA", END),   # (0, 10)  (0, 5, 7, 0)       5: the cut inside the hit
         (b"GATTACACCCCC", ALL),   # (0, 12)  (0, 0, 7, 0)       12: no insert
         (b"CCCCCCCGATTA", ALL),   # (0, 12)  (0, 7, 5, 0)       5: a partial overlap
         (b"CCCCCCCCCCCC", ALL),   # (0, 12)  none
         (b"ACGTAGATTACA", LOW),   # not kept (0, 5, 7, 0)
         (b"ACGTAGATTACA", HEAD),  # (0, 5)   (0, 5, 7, 0)       the cut in front of the hit: nothing survives
         (b"ACGTAGATTACA", TAIL)]  # (7, 12)  (0, 5, 7, 0)       5: five inside the hit
CUTS = [(0, 12), (0, 10), (0, 12), (0, 12), (0, 12), NOT, (0, 5), (7, 12)]
HAND = dict(calls=1, calls_failed=0, reads=8, kept=7, reads_hit=7, reads_hit_kept=6, hits=[7, 0, 0, 0, 0, 0, 0, 0],
            hits_full=6, hits_at_0=1, mismatches=0, bases_behind=7 + 7 + 12 + 5 + 7 + 7 + 7, reads_hit_out=5,
            bases_hit_out=7 + 5 + 12 + 5 + 5)
#   pairs: (0, 1) both at 5; (2, 3) both, 0 and 7; (4, 5) one; (6, 7) both at 5
HAND_PAIRS = dict(pairs_both=3, pairs_one=1, pairs_same_clip=2)
HAND_CLIP = [(0, 5), (0, 5), (0, 0), (0, 7), None, (0, 5), (0, 5), (0, 5)]


def texts_of(reads, mode):
    return [fastq(reads[0::2]), fastq(reads[1::2])] if mode == "pe_split" else [fastq(reads)]


@pytest.mark.parametrize("mode", ["se", "pe_split", "pe_interleaved", "pe_combo_all"])
def test_hand_call(mode):
    r = am.adapters(P5, texts_of(READS, mode), mode, GAT, pos_bins=7, overlap=True)
    want = dict(HAND, **(HAND_PAIRS if mode != "se" else dict(pairs_both=0, pairs_one=0, pairs_same_clip=0)))
    assert {k: r[k] for k in want} == want
    assert r["clip"] == HAND_CLIP and am.clip_words(r)[3:5] == [7, 0xFFFFFFFF]
    pos = np.zeros((8, 7), np.uint64)
    pos[0][0], pos[0][5], pos[0][6] = 1, 5, 1  # start 7 in the last bin, 6
    ov = np.zeros((8, 65), np.uint64)
    ov[0][7], ov[0][5] = 6, 1
    assert np.array_equal(r["pos"], pos) and np.array_equal(r["overlap"], ov)
    # the cuts the table claims are the oracle's
    assert am.equal(r, am.of_reads([s for s, _ in READS], CUTS, mode != "se", GAT, 7, True), clip=True) == []


def test_mismatches_and_adapters_are_summed():
    st = am.make_set([b"ACGTACGTAC", b"GATTACA"], 7, 100)
    reads = [(b"TTACGAACGTAC", ALL), (b"TTTTTGATTACA", ALL)]  # adapter 0 at 2 with one mismatch; adapter 1 at 5
    r = am.adapters(P5, [fastq(reads)], "pe_interleaved", st, overlap=True)
    assert (r["hits"][:2], r["mismatches"], r["hits_full"], r["pairs_both"], r["pairs_same_clip"]) == ([1, 1], 1, 2, 1, 0)
    assert r["overlap"][0][10] == 1 and r["overlap"][1][7] == 1 and am.clip_words(r) == [2, 1 << 24 | 5]


def test_failed_calls_add_nothing():
    bad_format = fastq(READS[:2]) + b"@x\n\n+\n\n"
    bad_range = fastq(READS[:2] + [(b"ACGTACGTACGT", b"\xc8IIIIIIIIIII")])
    for text in (bad_format, bad_range):
        r = am.adapters(P5, [text], "se", GAT, 8, True)
        assert am.equal(r, am.failed(8, True), clip=True) == [] and (r["calls"], r["calls_failed"]) == (0, 1)
    a, b = am.adapters(P5, [fastq(READS[:4])], "se", GAT, 8), am.adapters(P5, [fastq(READS[4:])], "se", GAT, 8)
    two = am.add(am.add(a, am.failed(8)), b)
    assert am.equal(two, dict(am.adapters(P5, [fastq(READS)], "se", GAT, 8), calls=2, calls_failed=1)) == []
    assert two["clip"] == b["clip"] and am.add(a, am.failed(8))["clip"] == a["clip"]
    e = am.adapters(P5, [b""], "se", GAT, 4, True)
    assert am.equal(e, dict(am.zero(4, True), calls=1), clip=True) == []


# ---- the golden inputs: numbers computed from the texts alone ---------------------------------------------------------------
PG = ("illumina", 20, 20, False, False)
EXACT = am.make_set([TRUSEQ], 13, 0)


def _read(name):
    return open(os.path.join(INPUTS, name), "rb").read()


def finds(text):
    """per seq line of a FASTQ text (every fourth line from the second): where bytes.find sees the adapter, or -1"""
    return [line.find(TRUSEQ) for line in text.split(b"\n")[1::4]]


@pytest.mark.parametrize("name", ["test.fastq", "test.f.fastq", "test.r.fastq"])
def test_golden_inputs(name):
    text = _read(name)
    found = finds(text)
    n = sum(f >= 0 for f in found)
    assert n > 0
    for mode in (("se", "pe_interleaved", "pe_combo_all") if name == "test.fastq" else ("se",)):
        r = am.adapters(PG, [text], mode, EXACT, pos_bins=151, overlap=True)
        assert r["calls"] == 1 and r["reads"] == len(found) and r["reads_hit"] == n == r["hits"][0] == r["hits_full"]
        assert [(-1 if h is None else h[1]) for h in r["clip"]] == found and r["mismatches"] == 0
        assert int(r["pos"][0].sum()) == n == int(r["overlap"][0][13])


def test_golden_split_is_the_interleaved_row():
    f, r = _read("test.f.fastq"), _read("test.r.fastq")
    s = am.adapters(PG, [f, r], "pe_split", EXACT, 151, True)
    assert am.equal(s, am.adapters(PG, [_read("test.fastq")], "pe_interleaved", EXACT, 151, True), clip=True) == []
    ff, fr = finds(f), finds(r)
    assert s["reads_hit"] == sum(x >= 0 for x in ff) + sum(x >= 0 for x in fr)
    assert s["pairs_both"] == sum(a >= 0 and b >= 0 for a, b in zip(ff, fr))
    assert s["pairs_one"] == sum((a >= 0) != (b >= 0) for a, b in zip(ff, fr))
    assert s["pairs_same_clip"] == sum(a >= 0 and a == b for a, b in zip(ff, fr))


# ---- consistency with the report's model ------------------------------------------------------------------------------------
def consistent(a, r):
    """the equalities between an adapters result and a report of the same call, and the result's own"""
    assert (a["calls"], a["calls_failed"], a["reads"], a["kept"]) == (r["calls"], r["calls_failed"], r["reads"], r["kept"])
    assert sum(a["hits"]) == a["reads_hit"] <= a["reads"] and a["reads_hit_out"] <= a["reads_hit_kept"] <= a["reads_hit"]
    assert a["hits_full"] <= a["reads_hit"] and a["hits_at_0"] <= a["reads_hit"]
    assert a["bases_hit_out"] <= r["bases_out"] and a["bases_behind"] <= r["bases_in"]
    assert a["pairs_same_clip"] <= a["pairs_both"] and 2 * a["pairs_both"] + a["pairs_one"] <= a["reads_hit"]
    if "pos" in a:
        assert a["pos"].sum(axis=1).tolist() == a["hits"]
    if "overlap" in a:
        assert a["overlap"].sum(axis=1).tolist() == a["hits"]


SOAK_SEQS = [TRUSEQ, b"CTGTCTCTTATACACATCTCCGAGCCCACGAGAC", b"TGGAATTCTCGGGTGCCAAGG"]


@pytest.mark.parametrize("name", GOLDEN_SUMMARY_RUNS)
def test_consistent_with_the_report_on_golden_runs(golden_tmp, name):
    params, texts, mode, n_reads, _ = golden_case(golden_tmp, name)
    a = am.adapters(params, texts, mode, am.make_set(SOAK_SEQS, 5, 100), 64, True, n_reads=n_reads)
    assert a["calls"] == 1
    consistent(a, rm.report(params, texts, mode, 0, 0, n_reads=n_reads))


@pytest.mark.parametrize("part", range(10))
def test_consistent_with_the_report_on_drawn_texts(part):
    """100 drawn texts with adapters planted at drawn starts behind drawn inserts"""
    rng = np.random.default_rng(7700 + part)
    hit = 0
    for _ in range(10):
        c = soak_fastq.draw(rng)
        texts = [am.plant(rng, t, SOAK_SEQS) for t in c["texts"]]
        st = am.make_set(SOAK_SEQS, int(rng.integers(1, 14)), int(rng.choice([0, 100, 200])))
        bins = int(rng.integers(1, 200))
        a = am.adapters(tuple(c["params"]), texts, c["mode"], st, bins, True)
        consistent(a, rm.report(tuple(c["params"]), texts, c["mode"], 0, 0))
        if not a["calls"]:
            assert am.equal(a, am.failed(bins, True), clip=True) == []
        hit += a["reads_hit"]
    assert hit > 0
