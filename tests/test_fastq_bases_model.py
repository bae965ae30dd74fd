"""tests/fastq_bases_model.py pinned three ways: by a truth table written out by hand, by the golden inputs (numbers
computed from the texts alone), and by consistency with the report's model.  No device."""
import os

import numpy as np
import pytest

import fastq_bases_model as bm
import fastq_report_model as rm
import soak_fastq
from test_fastq_report_model import GOLDEN_SUMMARY_RUNS, TABLE, fastq, golden_case, golden_tmp  # noqa: F401 (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")
NOT = (-1, -1)
ALL = b"IIIIIIIIIIII"   # twelve bases of quality 40: the cut is (0, 12)
END = b"IIIIIIIIII##"   # two bases go at the 3' end: (0, 10)
START = b"##IIIIIIIIII"  # two at the 5' end: (2, 12)
LOW = b"############"   # not kept
P5 = ("sanger", 20, 5, False, False)


def class_of(byte):
    """the issue's table as it is written"""
    for c, letters in enumerate(("Aa", "Cc", "Gg", "Tt", "Nn")):
        if chr(byte) in letters:
            return c
    return 5


def fold(rows, pos_bins, gc=True):
    """The bases of rows = [(seq, five, three)] by the rule of include/sickle_amd.h, read by read and byte by byte in plain
    Python: nothing shared with the model's numpy."""
    r = bm.zero(pos_bins, gc)
    r["calls"] = 1
    for seq, five, three in rows:
        r["reads"] += 1
        kept = three >= 0
        r["kept"] += kept
        sides = [("in", list(enumerate(seq)))]
        if kept:
            sides.append(("out", [(p - five, b) for p, b in enumerate(seq) if five <= p < three]))
        for side, line in sides:
            n = [0] * 6
            for p, b in line:
                c = class_of(b)
                n[c] += 1
                r["bases_" + side][c] += 1
                r["lower_" + side] += ord("a") <= b <= ord("z")
                r["pos_" + side][c][min(p, pos_bins - 1)] += 1
            r["reads_n_" + side] += n[4] > 0
            acgt = n[0] + n[1] + n[2] + n[3]
            if acgt:
                r["gc_" + side][100 * (n[1] + n[2]) // acgt] += 1
            else:
                r["gc_none_" + side] += 1
    return r


# (id, params, mode, texts, the reads that count, their cuts by hand): the report's table, whose reads are ACGT with an n
# or an N for -n, and the cases of this rule
EVERY = (b"ACGTNacgtnRU", END)                # each class in both cases, two of class 5; cut (0, 10)
OTHER = (b"A.\x80\xff\rUYRacgt", START)       # '.', bytes >= 0x80, '\r', IUPAC codes; cut (2, 12)
ONLY_N = (b"NNNNNNNNNNNN", END)               # no byte of class 0-3: gc_none, in and out
N_LAST = (b"ACGTACGTACGN", END)               # its only N is cut off: reads_n_in but not reads_n_out
N_FIRST = (b"NCGTACGTACGT", START)            # likewise at the 5' end
GC = [(b"AAAAAAAAAAAA", ALL),                 # 0
      (b"GATGATGATGAT", ALL),                 # 4 / 12: 33
      (b"GCATGCATGCAT", ALL),                 # 50
      (b"GCAGCAGCAGCA", ALL),                 # 8 / 12 = 66.67: 66
      (b"GCGCGCGCGCGC", ALL),                 # 100
      (b"GAAAAAAAAAAA", ALL),                 # 1 / 12 = 8.33: 8
      (b"GCNNNNNNNNNA", ALL),                 # 2 / 3 of the bytes that count: 66
      (b"gcgcgcaNNNNN", ALL),                 # 6 / 7 = 85.7: 85, lower case
      (b"AAAAAAAAAAGC", END)]                 # 2 / 12 = 16 in, 0 / 10 = 0 out
GC_CUTS = [(0, 12)] * 8 + [(0, 10)]
GC_BINS_IN = [0, 33, 50, 66, 100, 8, 66, 85, 16]
MINE = [
    ("classes", P5, "se", [fastq([EVERY, OTHER])], [EVERY, OTHER], [(0, 10), (2, 12)]),
    ("classes_split", P5, "pe_split", [fastq([EVERY]), fastq([OTHER])], [EVERY, OTHER], [(0, 10), (2, 12)]),
    ("only_n", P5, "se", [fastq([ONLY_N, (ONLY_N[0], LOW)])], [ONLY_N, (ONLY_N[0], LOW)], [(0, 10), NOT]),
    ("n_cut_off", P5, "pe_interleaved", [fastq([N_LAST, N_FIRST])], [N_LAST, N_FIRST], [(0, 10), (2, 12)]),
    ("gc", P5, "se", [fastq(GC)], GC, GC_CUTS),
    ("gc_combo_all", P5, "pe_combo_all", [fastq(GC + [(GC[0][0], LOW)])], GC + [(GC[0][0], LOW)], GC_CUTS + [NOT]),
]
CASES = list(TABLE) + MINE


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("pos_bins", [16, 1, 5, 12])
def test_hand_truth_table(case, pos_bins):
    _, params, mode, texts, reads, cuts = case
    want = fold([(s, f, t) for (s, _), (f, t) in zip(reads, cuts)], pos_bins)
    assert bm.equal(bm.bases(params, texts, mode, pos_bins, gc=True), want) == []


def test_hand_numbers():
    """a few of the table's results as literal numbers"""
    r = bm.bases(P5, [fastq([EVERY, OTHER])], "se", 16, gc=True)
    assert (r["calls"], r["calls_failed"], r["reads"], r["kept"]) == (1, 0, 2, 2)
    # EVERY: A a C c G g T t N n R U; OTHER: A . 80 ff \r U Y R a c g t
    assert r["bases_in"] == [4, 3, 3, 3, 2, 9]
    # EVERY[0:10] = ACGTNacgtn, OTHER[2:12] = 80 ff \r U Y R a c g t
    assert r["bases_out"] == [3, 3, 3, 3, 2, 6]
    assert (r["lower_in"], r["lower_out"]) == (9, 9)
    assert (r["reads_n_in"], r["reads_n_out"], r["gc_none_in"], r["gc_none_out"]) == (1, 1, 0, 0)
    assert r["pos_in"][:, 0].tolist() == [2, 0, 0, 0, 0, 0] and r["pos_in"][:, 1].tolist() == [0, 1, 0, 0, 0, 1]
    assert r["pos_out"][:, 0].tolist() == [1, 0, 0, 0, 0, 1]  # 'A' of EVERY, 0x80 of OTHER (its position 2)
    assert r["pos_in"][:, 4].tolist() == [0, 0, 0, 0, 1, 1] and r["pos_in"][:, 12:].sum() == 0
    # EVERY: 4 of 8 in and out; OTHER: acgt in both: 2 of 5 in (A a c g t), 2 of 4 out
    assert r["gc_in"][50] == 1 and r["gc_in"][40] == 1 and r["gc_out"][50] == 2
    g = bm.bases(P5, [fastq(GC)], "se", 0, gc=True)
    assert sorted(np.flatnonzero(g["gc_in"]).tolist()) == sorted(set(GC_BINS_IN)) and g["gc_in"][66] == 2
    assert g["gc_out"][0] == 2 and g["gc_out"][16] == 0 and "pos_in" not in g
    n = bm.bases(P5, [fastq([ONLY_N, N_LAST, N_FIRST])], "se")
    assert (n["reads_n_in"], n["reads_n_out"], n["gc_none_in"], n["gc_none_out"]) == (3, 1, 1, 1)
    assert "gc_in" not in n and "pos_in" not in n


def test_trunc_n_discards_and_truncates():
    """-n: a lower-case n truncates in front of it, an upper-case N discards; the `in` side is the text's either way"""
    row = [c for c in TABLE if c[0] == "trunc_n"][0]
    off = [c for c in TABLE if c[0] == "trunc_n_off"][0]
    a, b = bm.bases(row[1], row[3], "se", 16), bm.bases(off[1], off[3], "se", 16)
    assert a["bases_in"] == b["bases_in"] and a["reads_n_in"] == b["reads_n_in"] == 3
    assert (a["kept"], a["reads_n_out"]) == (2, 0) and (b["kept"], b["reads_n_out"]) == (4, 3)
    assert a["bases_out"][4] == 0 and b["bases_out"][4] == 3 and a["lower_out"] == 0 and b["lower_out"] == 2


def test_failed_calls_add_nothing():
    bad_format = fastq([EVERY]) + b"@x\n\n+\n\n"
    bad_range = fastq([EVERY, (b"ACGTACGTACGT", b"\xc8IIIIIIIIIII")])
    for text in (bad_format, bad_range):
        r = bm.bases(P5, [text], "se", 8, gc=True)
        assert bm.equal(r, bm.failed(8, True)) == [] and (r["calls"], r["calls_failed"]) == (0, 1)
    two = bm.add(bm.add(bm.bases(P5, [fastq([EVERY])], "se", 8), bm.failed(8)), bm.bases(P5, [fastq([OTHER])], "se", 8))
    assert bm.equal(two, dict(bm.bases(P5, [fastq([EVERY, OTHER])], "se", 8), calls=2, calls_failed=1)) == []
    e = bm.bases(P5, [b""], "se", 4, gc=True)
    assert bm.equal(e, dict(bm.zero(4, True), calls=1)) == []


# ---- the golden inputs: numbers computed from the texts alone ---------------------------------------------------------------
#          reads  bases_in A, C, G, T, N, other                   reads_n_in  position 0: A, C, G, T, N  gc_in[50]
GOLDEN = {
    "test.fastq": (2500, [85489, 102443, 101356, 84487, 1225, 0], 343, [516, 688, 639, 457, 200], 91),
    "test.f.fastq": (1250, [42642, 51598, 50622, 42429, 209, 0], 202, [237, 309, 298, 206, 200], 43),
    "test.r.fastq": (1250, [42847, 50845, 50734, 42058, 1016, 0], 141, [279, 379, 341, 251, 0], 48),
}
PG = ("illumina", 20, 20, False, False)


def _read(name):
    return open(os.path.join(INPUTS, name), "rb").read()


def _numbers(r):
    return r["reads"], r["bases_in"], r["reads_n_in"], r["pos_in"][:5, 0].tolist(), int(r["gc_in"][50])


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_golden_inputs(name):
    modes = ("se", "pe_interleaved", "pe_combo_all") if name == "test.fastq" else ("se",)
    for mode in modes:
        r = bm.bases(PG, [_read(name)], mode, 151, gc=True)
        assert _numbers(r) == GOLDEN[name] and r["calls"] == 1
        assert r["pos_in"][5].sum() == 0 and r["pos_in"][:, 150].sum() == 0  # 150 bases a read


def test_golden_split_is_the_interleaved_row():
    r = bm.bases(PG, [_read("test.f.fastq"), _read("test.r.fastq")], "pe_split", 151, gc=True)
    assert _numbers(r) == GOLDEN["test.fastq"]
    assert bm.equal(r, bm.bases(PG, [_read("test.fastq")], "pe_interleaved", 151, gc=True)) == []


# ---- consistency with the report's model ------------------------------------------------------------------------------------
def consistent(b, r):
    """the equalities between the bases and a report of the same call at equal pos_bins"""
    assert (b["calls"], b["calls_failed"], b["reads"], b["kept"]) == (r["calls"], r["calls_failed"], r["reads"], r["kept"])
    assert sum(b["bases_in"]) == r["bases_in"] and sum(b["bases_out"]) == r["bases_out"]
    if "pos_in" in b:
        assert np.array_equal(b["pos_in"].sum(axis=0), r["qcnt_in"]) and np.array_equal(b["pos_out"].sum(axis=0), r["qcnt_out"])
        assert b["pos_in"].sum(axis=1).tolist() == b["bases_in"] and b["pos_out"].sum(axis=1).tolist() == b["bases_out"]
    if "gc_in" in b:
        assert int(b["gc_in"].sum()) + b["gc_none_in"] == b["reads"] and int(b["gc_out"].sum()) + b["gc_none_out"] == b["kept"]
    assert b["reads_n_in"] <= b["reads"] and b["reads_n_out"] <= min(b["kept"], b["reads_n_in"])
    assert b["lower_out"] <= b["lower_in"] <= sum(b["bases_in"])


@pytest.mark.parametrize("name", GOLDEN_SUMMARY_RUNS)
def test_consistent_with_the_report_on_golden_runs(golden_tmp, name):
    params, texts, mode, n_reads, _ = golden_case(golden_tmp, name)
    b = bm.bases(params, texts, mode, 64, gc=True, n_reads=n_reads)
    assert b["calls"] == 1
    consistent(b, rm.report(params, texts, mode, 0, 64, n_reads=n_reads))


@pytest.mark.parametrize("part", range(10))
def test_consistent_with_the_report_on_drawn_texts(part):
    rng = np.random.default_rng(7100 + part)
    for _ in range(10):
        c = soak_fastq.draw(rng)
        bins = int(rng.integers(1, 200))
        b = bm.bases(tuple(c["params"]), c["texts"], c["mode"], bins, gc=True)
        consistent(b, rm.report(tuple(c["params"]), c["texts"], c["mode"], 0, bins))
        if not b["calls"]:
            assert bm.equal(b, bm.failed(bins, True)) == []
