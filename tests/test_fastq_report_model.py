"""tests/fastq_report_model.py against a truth table written out by hand, against the reference's recorded summaries
(tests/golden/e2e.json), and against its own invariants.  No device."""
import os

import numpy as np
import pytest

import cli_util as cu
import fastq_order_model as fo
import fastq_report_model as rm
import fastq_util as fu
import trim_model as tm

# ---- the hand truth table -------------------------------------------------------------------------------------------
# Under ("sanger", 20, L, no5, trunc_n): 'I' is quality 40, '#' quality 2.  Reads of 12 bases have a window of one base
# (0.1 * 12), so the 5' cut is the first base of quality >= 20 and the 3' cut the first one below it behind that.
#            seq              qual             cut (five, three) by hand
A = (b"ACGTACGTACGT", b"IIIIIIIIII##")  # (0, 10): two bases go at the 3' end
B = (b"ACGTACGTACGT", b"##IIIIIIIIII")  # (2, 12): two bases go at the 5' end; with -x the first window, which is low, is
#                                         the 3' cut (reference src/trim.cpp:61-67): (0, 0), not kept
C = (b"ACGTACGTACG", b"###########")    # not kept: no window reaches the threshold
D = (b"A", b"I")                        # a 1-base read: (0, 1) with -l 1, not kept with -l 5
E = (b"ACGTACnGTACG", b"IIIIIIIIII##")  # (0, 10); with -n the n at 6 truncates to the base before it (reference
#                                         src/trim.cpp:96-98: three = npos - 1): (0, 5), still 5 or more
F = (b"ACGnACGTACGT", b"IIIIIIIIII##")  # (0, 10); with -n (0, 2) is below -l 5: not kept
G = (b"ACGTACNGTACG", b"IIIIIIIIII##")  # (0, 10); with -n an upper-case N alone discards the read (src/trim.cpp:92-93)
NOT = (-1, -1)
P5 = ("sanger", 20, 5, False, False)


def fastq(reads, names=None, last_newline=True):
    out = b"".join(b"@" + (names[i] if names else b"r%d" % i) + b"\n" + s + b"\n+\n" + q + b"\n" for i, (s, q) in enumerate(reads))
    return out if last_newline else out[:-1]


def fold(rows, paired, len_bins, pos_bins):
    """The report of rows = [(qual, five, three)] by the rule of include/sickle_amd.h, read by read and byte by byte in
    plain Python: nothing shared with the model's numpy."""
    r = rm.zero(len_bins, pos_bins)
    r["calls"] = 1
    for q, five, three in rows:
        n = len(q)
        r["reads"] += 1
        r["bases_in"] += n
        r["max_len_in"] = max(r["max_len_in"], n)
        r["len_in"][min(n, len_bins - 1)] += 1
        for p, byte in enumerate(q):
            r["qsum_in"][min(p, pos_bins - 1)] += byte
            r["qcnt_in"][min(p, pos_bins - 1)] += 1
        if three < 0:
            r["discarded"] += 1
            r["bases_discarded"] += n
            continue
        r["kept"] += 1
        r["bases_out"] += three - five
        r["bases_cut5"] += five
        r["bases_cut3"] += n - three
        r["reads_cut5"] += five != 0
        r["reads_cut3"] += three != n
        r["max_len_out"] = max(r["max_len_out"], three - five)
        r["len_out"][min(three - five, len_bins - 1)] += 1
        for p in range(five, three):
            r["qsum_out"][min(p - five, pos_bins - 1)] += q[p]
            r["qcnt_out"][min(p - five, pos_bins - 1)] += 1
    if paired:
        for k in range(len(rows) // 2):
            r["pairs"][(rows[2 * k][2] >= 0) | ((rows[2 * k + 1][2] >= 0) << 1)] += 1
    return r


def rows_of(reads, cuts):
    return [(q, f, t) for (_, q), (f, t) in zip(reads, cuts)]


# (id, params, mode, texts, the reads that count, their cuts by hand)
PAIRS = [A, B, A, C, C, B, C, C]
PAIR_CUTS = [(0, 10), (2, 12), (0, 10), NOT, NOT, (2, 12), NOT, NOT]
TABLE = [
    ("se", P5, "se", [fastq([A, B, C])], [A, B, C], [(0, 10), (2, 12), NOT]),
    ("se_all_kept", P5, "se", [fastq([A, A])], [A, A], [(0, 10), (0, 10)]),
    ("se_none_kept", P5, "se", [fastq([C, C, C])], [C, C, C], [NOT, NOT, NOT]),
    ("pairs_interleaved", P5, "pe_interleaved", [fastq(PAIRS)], PAIRS, PAIR_CUTS),
    ("pairs_combo_all", P5, "pe_combo_all", [fastq(PAIRS)], PAIRS, PAIR_CUTS),
    ("pairs_split", P5, "pe_split", [fastq(PAIRS[0::2]), fastq(PAIRS[1::2])], PAIRS, PAIR_CUTS),
    ("no5", ("sanger", 20, 5, True, False), "se", [fastq([B, A])], [B, A], [NOT, (0, 10)]),
    ("trunc_n", ("sanger", 20, 5, False, True), "se", [fastq([E, F, A, G])], [E, F, A, G], [(0, 5), NOT, (0, 10), NOT]),
    ("trunc_n_off", P5, "se", [fastq([E, F, A, G])], [E, F, A, G], [(0, 10), (0, 10), (0, 10), (0, 10)]),
    ("one_base_kept", ("sanger", 20, 1, False, False), "se", [fastq([D, A])], [D, A], [(0, 1), (0, 10)]),
    ("one_base_short", P5, "se", [fastq([D, A])], [D, A], [NOT, (0, 10)]),
    # the odd last record of an interleaved text is dropped by the framing: it is in no count
    ("odd_interleaved", P5, "pe_interleaved", [fastq([A, C, A])], [A, C], [(0, 10), NOT]),
    ("unterminated", P5, "se", [fastq([A, B], last_newline=False)], [A, B], [(0, 10), (2, 12)]),
    ("long_names", P5, "pe_interleaved", [fastq([A, B], names=[b"x" * 33, b"y"])], [A, B], [(0, 10), (2, 12)]),
]


@pytest.mark.parametrize("case", TABLE, ids=[c[0] for c in TABLE])
@pytest.mark.parametrize("bins", [(16, 16), (1, 1), (11, 5), (13, 12)])
def test_hand_truth_table(case, bins):
    _, params, mode, texts, reads, cuts = case
    want = fold(rows_of(reads, cuts), mode != "se", *bins)
    got = rm.report(params, texts, mode, *bins)
    assert rm.equal(got, want) == []


def test_hand_numbers():
    """a few of the table's reports as literal numbers"""
    r = rm.report(P5, [fastq([A, B, C])], "se", 16, 16)
    assert (r["calls"], r["calls_failed"], r["reads"], r["kept"], r["discarded"]) == (1, 0, 3, 2, 1)
    assert r["pairs"] == [0, 0, 0, 0]
    assert (r["bases_in"], r["bases_out"], r["bases_cut5"], r["bases_cut3"], r["bases_discarded"]) == (35, 20, 2, 2, 11)
    assert (r["reads_cut5"], r["reads_cut3"], r["max_len_in"], r["max_len_out"]) == (1, 1, 12, 10)
    assert r["len_in"].tolist() == [0] * 11 + [1, 2, 0, 0, 0] and r["len_out"].tolist() == [0] * 10 + [2] + [0] * 5
    assert r["qcnt_in"].tolist() == [3] * 11 + [2] + [0] * 4 and r["qcnt_out"].tolist() == [2] * 10 + [0] * 6
    # position 0: 'I' + '#' + '#' in, 'I' + 'I' out (B's output starts at its third base)
    assert (int(r["qsum_in"][0]), int(r["qsum_out"][0])) == (73 + 35 + 35, 73 + 73)
    assert int(r["qsum_in"][11]) == 35 + 73 and int(r["qsum_out"][9]) == 73 + 73
    p = rm.report(P5, [fastq(PAIRS)], "pe_interleaved")
    assert p["pairs"] == [1, 1, 1, 1] and (p["reads"], p["kept"], p["discarded"]) == (8, 4, 4)
    assert rm.summary_text(p, "pe_interleaved") == ("\nFastQ paired records kept: 2 (1 pairs)\nFastQ single records kept: 2\n"
                                                    "FastQ paired records discarded: 2 (1 pairs)\n"
                                                    "FastQ single records discarded: 2\n\n")
    assert rm.summary_text(p, "pe_split") == ("\nFastQ paired records kept: 2 (1 pairs)\n"
                                              "FastQ single records kept: 2 (from PE1: 1, from PE2: 1)\n"
                                              "FastQ paired records discarded: 2 (1 pairs)\n"
                                              "FastQ single records discarded: 2 (from PE1: 1, from PE2: 1)\n\n")
    assert rm.summary_text(r, "se") == "FastQ records kept: 2\nFastQ records discarded: 1\n\n"


def test_failed_calls_add_nothing():
    bad_format = fastq([A]) + b"@x\n\n+\n\n"                 # an empty seq line
    bad_range = fastq([A, (b"ACGTACGTACGT", b"\xc8IIIIIIIIIII")])  # a quality byte above the type's highest
    for text in (bad_format, bad_range):
        r = rm.report(P5, [text], "se", 8, 8)
        assert rm.equal(r, rm.failed(8, 8)) == [] and r["calls_failed"] == 1 and r["calls"] == 0
    assert rm.report(P5, [fastq(PAIRS[0::2]), fastq(PAIRS[1::2][:-1])], "pe_split")["calls_failed"] == 1  # SK_FQ_PAIR_COUNT
    two = rm.add(rm.report(P5, [fastq([A, B, C])], "se", 8, 8), rm.report(P5, [bad_format], "se", 8, 8))
    assert (two["calls"], two["calls_failed"], two["reads"]) == (1, 1, 3)


# ---- the reference's recorded summaries -----------------------------------------------------------------------------
# every run of tests/golden/e2e.json whose stdout holds the kept / discarded lines: all sixteen of "runs" and the three of
# "long_reads" (the runs of "thread_order" were recorded without their stdout)
GOLDEN_SUMMARY_RUNS = [
    "pe_fr_illumina", "pe_fr_illumina_n", "pe_fr_illumina_x_q30_l50", "pe_fr_sanger_q60", "pe_fr_solexa_q25", "pe_fr_gz_illumina",
    "pe_inter_illumina", "pe_inter_illumina_nosingles", "pe_inter_illumina_n_l30", "se_equiv_selfpair_illumina",
    "se_equiv_selfpair_sanger", "pe_problem1_inter", "pe_syn_fr_sanger", "pe_syn_fr_sanger_n", "pe_syn_mixed_inter_illumina_n",
    "pe_syn_mixed_inter_gz_illumina_n", "pe_long_inter_sanger", "pe_long_inter_sanger_n_q25", "pe_long_inter_sanger_x_l2000"]


def golden_case(tmp, name):
    """-> (params tuple, texts, mode, n_reads, recorded stdout) of a recorded run.  n_reads: None, but for the run whose
    reader ends at its first batch (trim_model.UNREPLAYABLE): there the reads are those inside the reference's batches,
    none, as the ordered call takes them."""
    g = cu.e2e()
    rec = g["runs"][name] if name in g["runs"] else g["long_reads"][name]
    argv = [a.format(tmp=str(tmp), inputs=cu.INPUTS) for a in rec["argv"]]
    paths = [argv[argv.index("-c") + 1]] if "-c" in argv else [argv[argv.index("-f") + 1], argv[argv.index("-r") + 1]]
    mode = "pe_interleaved" if "-c" in argv else "pe_split"
    texts = []
    for p in paths:
        raw = open(p, "rb").read()
        if p.endswith(".gz"):
            import gzip
            raw = gzip.decompress(raw)
        texts.append(raw)
    n_reads = None
    if name in tm.UNREPLAYABLE:
        batch_len = fu.reference_batch_len(os.path.getsize(paths[0]), paired=True)
        n_reads = 2 * fo.batch_tables([fo.lines_of(t) for t in texts], mode, batch_len)["units"]
    return tm.run_params(rec["argv"]), texts, mode, n_reads, rec["stdout"]


def test_golden_list_is_complete():
    g = cu.e2e()
    have = [name for sec in ("runs", "thread_order", "long_reads") for name, rec in g[sec].items()
            if isinstance(rec, dict) and "records kept" in rec.get("stdout", "")]
    assert sorted(have) == sorted(GOLDEN_SUMMARY_RUNS)


@pytest.fixture(scope="module")
def golden_tmp(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("report_golden")
    cu.prepare_inputs(tmp)
    cu.prepare_long_inputs(tmp)
    return tmp


@pytest.mark.parametrize("name", GOLDEN_SUMMARY_RUNS)
def test_golden_summaries(golden_tmp, name):
    params, texts, mode, n_reads, stdout = golden_case(golden_tmp, name)
    r = rm.report(params, texts, mode, 64, 64, n_reads=n_reads)
    assert r["calls"] == 1
    text = rm.summary_text(r, mode)
    assert text.startswith("\nFastQ paired records kept: ") and text in stdout
    # invariants: len_out summed is kept, the position counts summed are the bases
    assert int(r["len_out"].sum()) == r["kept"] and int(r["len_in"].sum()) == r["reads"]
    assert int(r["qcnt_in"].sum()) == r["bases_in"] and int(r["qcnt_out"].sum()) == r["bases_out"]
    assert r["reads"] == r["kept"] + r["discarded"] == 2 * sum(r["pairs"])
    assert r["bases_in"] == r["bases_out"] + r["bases_cut5"] + r["bases_cut3"] + r["bases_discarded"]


def test_invariants_on_drawn_texts():
    rng = np.random.default_rng(5)
    for _ in range(20):
        reads = []
        for _ in range(int(rng.integers(1, 40))):
            n = int(rng.integers(1, 60))
            reads.append((bytes(rng.choice(list(b"ACGTN"), n).astype(np.uint8)), bytes(rng.integers(33, 74, n).astype(np.uint8))))
        mode = ("se", "pe_interleaved")[int(rng.integers(0, 2))]
        lb, pb = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        params = ("sanger", int(rng.integers(2, 41)), int(rng.integers(1, 30)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)))
        r = rm.report(params, [fastq(reads)], mode, lb, pb)
        n_reads = len(reads) if mode == "se" else len(reads) & ~1
        assert r["reads"] == n_reads == r["kept"] + r["discarded"]
        assert int(r["len_out"].sum()) == r["kept"] and int(r["len_in"].sum()) == r["reads"]
        assert int(r["qcnt_in"].sum()) == r["bases_in"] and int(r["qcnt_out"].sum()) == r["bases_out"]
        assert r["bases_in"] == r["bases_out"] + r["bases_cut5"] + r["bases_cut3"] + r["bases_discarded"]
        if mode != "se":
            assert sum(r["pairs"]) == n_reads // 2 and r["kept"] == 2 * r["pairs"][3] + r["pairs"][1] + r["pairs"][2]
