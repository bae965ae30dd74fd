"""CPU: the piece rule of sk_trim_fastq_piece_device_async as tests/fastq_piece_model.py states it, checked against
tests/fastq_model.py: a text streamed over pieces of any size gives what the whole text gives.  This checks the rule
itself (include/sickle_amd.h) before any device is held to it."""
import pytest

import cli_util as cu
import fastq_model as fm
import fastq_piece_model as pm
import trim_model as tm
from test_fastq_api import golden_texts

PT = ("sanger", 20, 20, False, False)
REC = lambda k, n=30, q=b"I": b"@r%d\n" % k + b"ACGT" * n + b"\n+\n" + q * (4 * n) + b"\n"
LOW = b"@low\n" + b"ACGT" * 10 + b"\n+\nII\x1f" + b"I" * 37 + b"\n"  # a quality byte below sanger's range
SIZES = (1, 7, 997, 4096, 70001)


def test_take_and_consumed():
    text = b"".join(REC(k) for k in range(5))
    one = len(REC(0))
    p = pm.piece(PT, [text + b"@r5\nACG"], "se", True)
    assert p["u"] == 5 and p["consumed"] == [5 * one, 0] and p["carried"] == [7, 0] and p["tail_lines"] == [1, 0]
    p = pm.piece(PT, [text], "pe_interleaved", True)  # the odd record is carried, whole: 4 lines
    assert p["u"] == 4 and p["consumed"][0] == 4 * one and p["tail_lines"] == [4, 0] and p["dropped_unpaired"] == 0
    p = pm.piece(PT, [text, text[:2 * one + 9]], "pe_split", True)
    assert p["u"] == 2 and p["consumed"] == [2 * one, 2 * one] and p["tail_lines"] == [12, 1]
    assert p["res"]["verdict"] is None  # no SK_FQ_PAIR_COUNT
    p = pm.piece(PT, [b"no newline at all"], "se", True)
    assert p["u"] == 0 and p["consumed"] == [0, 0] and p["carried"] == [17, 0] and p["res"]["verdict"] is None
    # the same windows as the stream's last piece: the whole call
    p = pm.piece(PT, [text + b"@r5\nACG"], "se", False)
    assert p["records_in"] == [5, 0] and p["tail_lines"] == [2, 0] and p["consumed"][0] == len(text) + 7
    p = pm.piece(PT, [text], "pe_interleaved", False)
    assert p["dropped_unpaired"] == 1 and p["records_in"] == [5, 0]


def test_errors_only_from_consumed_records():
    bad = b"@bad\nACGT\n+\nIII\n"
    low = LOW
    for rec, key in ((bad, "verdict"), (low, "range")):
        p = pm.piece(PT, [REC(0) + REC(1) + rec[:-1]], "se", True)  # in the carry: its last '\n' is not in the window
        assert p["u"] == 2 and p["res"]["verdict"] is None and p["res"]["range"] is None
        p = pm.piece(PT, [rec + REC(2)], "se", True)
        assert p["res"][key] is not None
    p = pm.piece(PT, [REC(0) + REC(1) + bad], "pe_interleaved", True)  # a whole record carried: still no error
    assert p["u"] == 2 and p["res"]["verdict"] is None


def test_carry_status_is_sticky():
    assert pm.carry(10, 1, 64, 100) == (54, 164, 1, 0)
    assert pm.carry(0, 1, 64, 0) == (64, 64, 1, 0)
    assert pm.carry(10, 0, 64, 100) == (64, 64, 0, 1)
    assert pm.carry(65, 1, 64, 100) == (64, 64, 0, 2)
    assert pm.carry(64, 1, 64, 100, chunk_valid=0) == (64, 64, 0, 3)
    assert pm.carry(65, 0, 64, 100, chunk_valid=0) == (64, 64, 0, 1)  # the first that applies
    assert pm.carry(0, 1, 64, 100, prev_status=3) == (64, 64, 0, 3)
    assert pm.carry(0, 1, 64, 100, other_status=2) == (64, 64, 0, 2)
    assert pm.carry(0, 0, 64, 100, prev_status=2, other_status=3) == (64, 64, 0, 2)


def test_stream_errors_are_stream_wide():
    recs = [REC(k) for k in range(40)]
    bad = list(recs)
    bad[23] = b"@bad\nACGT\n+\nIII\n"
    assert pm.stream(PT, [b"".join(bad)], "se", 500)["error"] == ("format", fm.SK_FQ_LENGTHS, 0, 23)
    low = list(recs)
    low[31] = LOW
    assert pm.stream(PT, [b"".join(low)], "se", 500)["error"] == ("range", 31, 2, 0x1f)
    assert pm.stream(PT, [b"".join(low), b"".join(recs)], "pe_split", 300)["error"] == ("range", 62, 2, 0x1f)
    # a range error in an earlier piece comes before a format error in a later one (the whole call says format)
    both = list(low)
    both[35] = bad[23]
    assert pm.stream(PT, [b"".join(both)], "se", 500)["error"][0] == "range"
    assert fm.expected(PT, [b"".join(both)], "se")["verdict"] is not None
    assert pm.stream(PT, [b"".join(recs)], "se", 64, room=64)["error"] == ("room", 0)  # a record is longer than room


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_piece_model")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


def _same(got, want, mode):
    assert got["error"] is None and want["verdict"] is None and want["range"] is None
    for o in fm.USED[mode]:
        assert got["texts"][o] == want["texts"][o], "output %d" % o
        assert got["index"][o] == [int(x) for x in want["index"][o]]
    assert got["records_in"] == want["records_in"] and got["tail_lines"] == want["tail_lines"]
    assert got["dropped_unpaired"] == want["dropped_unpaired"]


_WHOLE = {}


@pytest.mark.parametrize("name,rec", [pytest.param(n, r, id=n) for n, r in tm.golden_runs()])
def test_streamed_model_reproduces_whole_text(workdir, name, rec):
    """Every golden run's inputs, in the run's own mode and text[0] as SE, streamed over pieces of 1, 7, 997, 4 096 and
    70 001 bytes: outputs, read numbers and counts are those of the whole text.  (The two smallest sizes once per distinct
    set of input files: the cut points, not the parameters, are what they vary.)"""
    mode, texts, _ = golden_texts(rec["argv"], workdir)
    pt = tm.run_params(rec["argv"])
    files = tuple(a for a in rec["argv"] if "{" in a and "o" not in a.split("/")[-1][:2])
    first = _WHOLE.setdefault(files, name) == name
    for m, tx in ((mode, texts), ("se", texts[:1])):
        want = fm.expected(pt, tx, m)
        for size in SIZES:
            if size < 100 and not first:
                continue
            got = pm.stream(pt, tx, m, size, room=1 << 30)
            _same(got, want, m)
            assert got["pieces"] == max(1, -(-max(len(t) for t in tx) // size))
