"""The batch walk of an ordered piece without a device: fqo_chain_piece of sickle_amd/csrc/sk_fastq_order.h run on the
host over descriptor tables (tests/fastq_order_piece/piece_host, and piece_host_san: the same stand-alone program under
the address and undefined-behaviour sanitizers) against the walk of tests/fastq_order_piece_model.py, window after window
with the state handed on; the windows' tables together are fastq_order_model.batch_tables on the whole file.  CPU only."""
import os
import random
import subprocess

import numpy as np
import pytest

import cli_util as cu
import fastq_order_model as om
import fastq_order_piece_model as opm
from test_fastq_order_host import random_lines

DIR = os.path.join(cu.ROOT, "tests", "fastq_order_piece")
MODES = {(1, 4): "se", (1, 8): "pe_interleaved", (2, 4): "pe_split"}


@pytest.fixture(scope="module", params=["piece_host", "piece_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def case(windows, firsts, m, batch_len, capacity, limit, more, state):
    w = [len(windows), m, batch_len, capacity, limit, int(more), state["carried"][0], state["carried"][1], state["batches"],
         state["ended"]]
    for lines, first in zip(windows, firsts):
        w += [first, len(lines)] + [len(l) for l in lines]
    return w


def run(tool, cases, d):
    src, dst = str(d / "cases.bin"), str(d / "results.bin")
    np.array([x for c in cases for x in c], dtype="<u8").tofile(src)
    pr = subprocess.run([tool, src, dst], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    words, out, at = np.fromfile(dst, dtype="<u8"), [], 0
    while at < len(words):
        n = int(words[at])
        out.append([int(x) for x in words[at + 1:at + 1 + n]])
        at += 1 + n
    assert len(out) == len(cases)
    return out


def model_words(w, n_in):
    nb = len(w["first_unit"]) - 1
    last = w["first_unit"][-1] - w["first_unit"][-2] if nb else 0
    pad = lambda xs: list(xs) + [0] * (2 - n_in)
    return [nb, w["first_unit"][-1], last, w["mismatch"], w["ended"], w["table_full"], w["undetermined"]] + pad(w["a"]) + \
        pad(w["carried"]) + w["first_unit"]


def streamed(rng, line_lists, m, batch_len, capacity, limit, cases, wants):
    """the whole file window after window: random numbers of new lines per window (every input its own), closing windows
    repeated while the table was full.  Appends a case and the model's answer per window; -> the stream's table."""
    n_in = len(line_lists)
    mode = MODES[(n_in, m)]
    at, carried = [0] * n_in, [[] for _ in line_lists]
    state = {"carried": [0, 0], "batches": 0, "ended": 0}
    table = [0]
    step = rng.choice([1, 3, 17, 200])
    for _ in range(10000):
        for i in range(n_in):
            n = rng.randrange(0, step + 1)
            carried[i] = carried[i] + line_lists[i][at[i]:at[i] + n]
            at[i] += n
        more = any(at[i] < len(line_lists[i]) for i in range(n_in))
        w = opm.walk(carried, mode, batch_len, capacity, limit, state, more)
        cases.append(case(carried, [rng.choice([0, 1, 16, 12345]) for _ in carried], m, batch_len, capacity, limit, more, state))
        wants.append(model_words(w, n_in))
        table += [table[-1] + x for x in w["first_unit"][1:]]
        state = {"carried": w["carried"] + [0] * (2 - n_in), "batches": state["batches"] + len(w["first_unit"]) - 1,
                 "ended": w["ended"]}
        carried = [c[a:] for c, a in zip(carried, w["a"])]
        if not more and not w["table_full"]:
            assert w["ended"] == 1
            return table, state
    raise AssertionError("the stream does not end")


def test_random_line_tables_streamed(tool, tmp_path):
    rng = random.Random(31337)
    cases, wants, batches, mism = [], [], 0, 0
    for it in range(1500):
        batch_len = rng.choice([20, 20, 21, 24, 33, 64, 100, 257, 1000])
        n_in, m = rng.choice([(1, 4), (1, 8), (2, 4)])
        a = random_lines(rng, batch_len)
        lists = [a]
        if n_in == 2:
            b = list(a)
            for _ in range(rng.randrange(0, 3)):  # a few lines of another length, or a shorter file
                if b and rng.random() < 0.7:
                    b[rng.randrange(len(b))] = b"x" * rng.randrange(0, batch_len - 1)
                else:
                    b = b[:rng.randrange(0, len(b) + 1)]
            lists.append(b)
        limit = rng.choice([0, 0, 0, 1, 2, 5])
        capacity = rng.choice([1, 2, 1000])
        table, state = streamed(rng, lists, m, batch_len, capacity, limit, cases, wants)
        whole = om.batch_tables(lists, MODES[(n_in, m)], batch_len, limit)
        assert table == whole["first_unit"]  # the model's windows together are the whole file
        batches += len(table) - 1
    got = run(tool, cases, tmp_path)
    for k, (g, w) in enumerate(zip(got, wants)):
        assert g == w, (k, cases[k][:10])
    assert batches > 1500 and len(cases) > 5000


def test_crafted_windows(tool, tmp_path):
    """the stop line's '\\n' in and out of the window, a window that commits nothing, the carried lines k = 1, 2, 3 and
    5..7, a full table, an ended run, the limit"""
    L = 100
    rec = [b"x" * 11] * 4  # 44 bytes of content per record: the budget is used up on line 9 (10 lines: 110 bytes)
    start = {"carried": [0, 0], "batches": 0, "ended": 0}
    cases, wants = [], []

    def add(windows, m, cap, limit, more, state, mode):
        w = opm.walk(windows, mode, L, cap, limit, state, more)
        cases.append(case(windows, [7] * len(windows), m, L, cap, limit, more, state))
        wants.append(model_words(w, len(windows)))
        return w
    w = add([rec * 2 + rec[:1]], 4, 8, 0, True, start, "se")  # 9 lines: 99 bytes, undetermined
    assert w["undetermined"] == 1 and w["a"] == [0]
    w = add([rec * 2 + rec[:2]], 4, 8, 0, True, start, "se")  # the tenth line is there: e = 10, batch of 8, k = 2
    assert w["a"] == [8] and w["carried"] == [2] and w["undetermined"] == 1
    for k in (1, 2, 3):
        w = add([rec[:k] + rec * 3], 4, 8, 0, True, {"carried": [k, 0], "batches": 3, "ended": 0}, "se")
        assert w["a"][0] > 0
    for k in (5, 6, 7):
        w = add([(rec * 2)[:k] + rec * 5], 8, 8, 0, True, {"carried": [k, 0], "batches": 1, "ended": 0}, "pe_interleaved")
        assert w["a"][0] % 8 == 0 and w["a"][0] > 0
    w = add([rec * 40], 4, 1, 0, False, start, "se")
    assert w["table_full"] == 1 and len(w["first_unit"]) == 2
    w = add([rec * 40], 4, 64, 0, True, {"carried": [0, 0], "batches": 9, "ended": 1}, "se")
    assert w["a"] == [0] and w["ended"] == 1
    w = add([rec * 40], 4, 64, 3, True, {"carried": [0, 0], "batches": 1, "ended": 0}, "se")
    assert len(w["first_unit"]) - 1 == 2 and w["ended"] == 1
    w = add([rec * 10, rec * 2 + [b"x" * 60] + rec * 10], 4, 64, 0, True, start, "pe_split")
    assert w["mismatch"] == 1 and w["ended"] == 1
    w = add([[b"x" * 50, b"x" * 50] + rec * 3], 4, 64, 0, True, start, "se")  # two lines use the budget up: an empty batch
    assert w["ended"] == 1 and w["a"] == [0] and w["mismatch"] == 0
    w = add([[], []], 4, 64, 0, False, start, "pe_split")
    assert w["ended"] == 1
    got = run(tool, cases, tmp_path)
    assert got == wants
