"""CPU: the rule of sk_trim_fastq_ordered_piece_device_async as tests/fastq_order_piece_model.py states it, checked against
tests/fastq_order_model.py on the whole text: a text streamed over pieces of any size, with a batch table of any size,
gives the whole file's batches, outputs in the -a T order, read numbers and counts.  This checks the rule itself (the
state suffices, PE split and its mismatch included) before any device is held to it."""
import hashlib
import os
import random

import pytest

import cli_util as cu
import fastq_model as fm
import fastq_order_model as om
import fastq_order_piece_model as opm
import fastq_util as fu
import trim_model as tm
from test_fastq_api import golden_texts

SIZES = (1, 7, 64, 500, 4096, 70001)
CAPS = (1, 2, 1 << 20)
PT = ("sanger", 20, 20, False, False)
REC = lambda k, n=10, q=b"I": b"@r%d\n" % k + b"ACGT" * n + b"\n+\n" + q * (4 * n) + b"\n"


def same(got, want, mode):
    """a streamed run against om.expected on the whole text"""
    if want["long_line"] is not None:
        assert got["error"] is not None and got["error"][0] == "long"
        return
    assert got["error"] is None and want["verdict"] is None and want["range"] is None
    assert got["first_unit"] == want["tables"]["first_unit"]
    for o in fm.USED[mode]:
        assert got["texts"][o] == want["texts"][o], "output %d" % o
        assert got["index"][o] == [int(x) for x in want["index"][o]]
        assert got["records"][o] == len(want["index"][o]) and got["bytes"][o] == len(want["texts"][o])
    st, oc = got["state"], want["order"]
    assert (st["batches"], st["units"], st["last_batch_units"], st["stopped_on_mismatch"]) == \
        (oc["batches"], oc["units"], oc["last_batch_units"], oc["stopped_on_mismatch"])
    assert st["ended"] == 1 and st["failed"] == 0
    n_in = 2 if mode == "pe_split" else 1
    assert got["records_in"][:n_in] == [x // 4 for x in want["tables"]["batched_lines"]]


def test_random_cases_streamed():
    """300 draws of the ordered call's generator (all three modes; split inputs of different record counts among them,
    which end the run or stop it on a mismatch), every chunk size and every table."""
    rng = random.Random(90210)
    seen, stops, batches = {"se": 0, "pe_split": 0, "pe_interleaved": 0}, 0, 0
    for it in range(300):
        ptuple, texts, mode, threads, batch_len = om.random_case(rng)
        want = om.expected(ptuple, texts, mode, threads, batch_len)
        seen[mode] += 1
        stops += want["order"]["stopped_on_mismatch"]
        batches += want["order"]["batches"]
        for size in SIZES:
            for cap in CAPS:
                same(opm.stream(ptuple, texts, mode, threads, batch_len, size, cap), want, mode)
    assert min(seen.values()) >= 60 and stops >= 10 and batches > 1000


def test_fast_path_is_the_piece():
    """stream() skips pieces that cannot commit; with keep_pieces every piece is worked out: the same run, and every piece
    is consistent with the state it was handed."""
    rng = random.Random(5)
    for it in range(12):
        ptuple, texts, mode, threads, batch_len = om.random_case(rng)
        for size, cap in ((1, 2), (64, 1), (500, 1 << 20)):
            fast = opm.stream(ptuple, texts, mode, threads, batch_len, size, cap)
            full = opm.stream(ptuple, texts, mode, threads, batch_len, size, cap, keep_pieces=True)
            assert len(full["pieces"]) == full["n_pieces"] == fast["n_pieces"]
            for key in ("texts", "index", "first_unit", "state", "records_in", "error"):
                assert fast[key] == full[key], key
            m = om.LINES_PER_UNIT[mode]
            for p in full["pieces"]:
                assert p["ok"] == 1 and all(k < m for k in p["state"]["carried"])
                assert not (p["table_full"] and p["order"]["batches"] != cap)
                assert p["undetermined"] + p["table_full"] + p["state"]["ended"] == 1  # why the walk stopped


def test_forced_mismatch_and_limit():
    a = b"".join(REC(k) for k in range(60))
    b = b"".join(REC(k) if k != 31 else REC(k, n=60) for k in range(60))  # one longer record: the batches drift apart
    L = 400
    want = om.expected(PT, [a, b], "pe_split", 3, L)
    assert want["order"]["stopped_on_mismatch"] == 1 and 0 < want["order"]["batches"]
    for size in SIZES:
        for cap in CAPS:
            got = opm.stream(PT, [a, b], "pe_split", 3, L, size, cap)
            same(got, want, "pe_split")
            # pieces behind the end take nothing and leave the state alone
            on = opm.stream(PT, [a, b], "pe_split", 3, L, size, cap, stop_at_end=False)
            assert on["texts"] == got["texts"] and on["state"] == got["state"] and on["n_pieces"] >= got["n_pieces"]
    for limit in (1, 2, 5):
        want = om.expected(PT, [a], "se", 4, L, limit)
        assert want["order"]["batches"] == limit
        for size in SIZES:
            for cap in CAPS:
                same(opm.stream(PT, [a], "se", 4, L, size, cap, limit), want, "se")


def test_errors_are_stream_wide_and_only_from_committed_records():
    recs = [REC(k) for k in range(40)]
    bad = list(recs)
    bad[23] = b"@bad\nACGT\n+\nIII\n"
    L = 300
    want = om.expected(PT, [b"".join(bad)], "se", 2, L)
    for size in (64, 500, 4096):
        got = opm.stream(PT, [b"".join(bad)], "se", 2, L, size, 1 << 20)
        assert got["error"] == ("format", fm.SK_FQ_LENGTHS, 0, 23, want["error_batch"])
    # the malformed record behind the last batch is never looked at, in pieces or whole
    tail = b"".join(recs[:8]) + bad[23]
    want = om.expected(PT, [tail], "pe_interleaved", 2, 10 ** 6)
    assert want["verdict"] is None and want["order"]["batches"] == 1 and want["order"]["records_unbatched"] == [1, 0]
    same(opm.stream(PT, [tail], "pe_interleaved", 2, 10 ** 6, 64, 4), want, "pe_interleaved")
    # a line of batch_len - 1 bytes refuses the stream at the piece that first holds it whole
    long_text = b"".join(recs[:20]) + b"@" + b"x" * (L - 2) + b"\nA\n+\nI\n"
    assert om.expected(PT, [long_text], "se", 2, L)["long_line"] == (0, 80)
    assert opm.stream(PT, [long_text], "se", 2, L, 500, 8)["error"][0] == "long"


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_order_piece_model")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


def _golden_inputs():
    """one run per distinct set of input files among the golden runs"""
    seen, out = set(), []
    for name, rec in tm.golden_runs():
        files = tuple(a[:-3] if a.endswith(".gz") else a  # (a .gz input is the same text)
                      for a in rec["argv"] if "{" in a and "o" not in a.split("/")[-1][:2])
        if files not in seen:
            seen.add(files)
            out.append(pytest.param(name, rec, id=name))
    return out


@pytest.mark.parametrize("name,rec", _golden_inputs())
def test_golden_inputs_streamed(workdir, name, rec):
    """Every golden input, in its run's mode and text[0] as SE, at the reference's own budget for the file: every chunk
    size and every table."""
    mode, texts, _ = golden_texts(rec["argv"], workdir)
    pt = tm.run_params(rec["argv"])
    for m, tx, threads in ((mode, texts, 4), ("se", texts[:1], 16)):
        batch_len = fu.reference_batch_len(len(tx[0]), paired=m != "se")
        want = om.expected(pt, tx, m, threads, batch_len)
        for size in SIZES:
            for cap in CAPS:
                same(opm.stream(pt, tx, m, threads, batch_len, size, cap), want, m)


@pytest.mark.parametrize("name", sorted(cu.e2e()["thread_order"].keys()) + ["pe_problem1_inter"])
def test_streamed_model_reproduces_thread_order_goldens(workdir, name):
    """The recorded outputs of the reference's -a T runs, byte for byte, from the model streamed in pieces."""
    e2e = cu.e2e()
    rec = e2e["thread_order"].get(name) or e2e["runs"][name]
    argv = rec["argv"]
    mode, texts, files = golden_texts(argv, workdir)
    first = argv[argv.index("-c" if "-c" in argv else "-f") + 1].format(inputs=cu.INPUTS, tmp=str(workdir))
    batch_len = fu.reference_batch_len(os.path.getsize(first), paired=True)
    for size, cap in ((4096, 1 << 20), (70001, 2), (500, 1)):
        got = opm.stream(tm.run_params(argv), texts, mode, int(argv[argv.index("-a") + 1]), batch_len, size, cap)
        assert got["error"] is None and got["state"]["batches"] == rec.get("batches", 0)
        for fname, want in rec["outputs"].items():
            text = got["texts"][files[fname]]
            assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname
