"""The batch chain and the rank map of the device's ordered FASTQ emission without a device: the functions of
sickle_amd/csrc/sk_fastq_order.h run on the host, lane after lane, over a descriptor table (tests/fastq_order/order_host,
and order_host_san: the same stand-alone program under the address and undefined-behaviour sanitizers) against
fastq_util.reference_batches and the queue loops of fastq_util.expected_se_output / expected_pe_outputs.  CPU only."""
import os
import random
import subprocess

import numpy as np
import pytest

import cli_util as cu
import fastq_order_model as om
import fastq_util as fu

DIR = os.path.join(cu.ROOT, "tests", "fastq_order")
MODES = {4: "se", 8: "pe_interleaved"}


@pytest.fixture(scope="module", params=["order_host", "order_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def chain_case(line_lists, m, batch_len, capacity, limit=0, threads=1, se=True):
    w = [1, len(line_lists), m, batch_len, capacity, limit, threads, int(se)]
    for lines in line_lists:
        w.append(len(lines))
        w.extend(len(l) for l in lines)
    return w


def walk_case(threads, se, first_unit):
    return [2, threads, int(se), len(first_unit) - 1] + list(first_unit)


def run(tool, cases, d):
    src, dst = str(d / "cases.bin"), str(d / "results.bin")
    np.array([x for c in cases for x in c], dtype="<u8").tofile(src)
    pr = subprocess.run([tool, src, dst], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    words, out, at = np.fromfile(dst, dtype="<u8"), [], 0
    while at < len(words):
        n = int(words[at])
        out.append(words[at + 1:at + 1 + n].astype(np.int64))
        at += 1 + n
    assert len(out) == len(cases)
    return out


def split_chain(res):
    """-> (dict of the counts, table, units in emission order)"""
    keys = ("batches", "units", "last_units", "mismatch", "overflow", "lines0", "lines1")
    c = dict(zip(keys, (int(x) for x in res[:7])))
    nb = c["batches"]
    return c, [int(x) for x in res[7:8 + nb]], [int(x) for x in res[8 + nb:]]


def want_units(first_unit, threads, se):
    out = []
    for b in range(len(first_unit) - 1):
        out.extend(first_unit[b] + k for k in om.unit_order(first_unit[b + 1] - first_unit[b], threads, se))
    return out


def check_chain(res, line_lists, mode, batch_len, limit=0, threads=1):
    c, tab, units = split_chain(res)
    want = om.batch_tables(line_lists, mode, batch_len, limit)
    assert tab == want["first_unit"] and c["units"] == want["units"] and c["last_units"] == want["last_batch_units"]
    assert c["mismatch"] == want["stopped_on_mismatch"] and c["overflow"] == 0
    assert [c["lines0"], c["lines1"]][:len(line_lists)] == want["batched_lines"]
    assert units == want_units(tab, threads, mode == "se")
    return c, tab


def bundled(name):
    return fu.file_lines(open(os.path.join(cu.INPUTS, name), "rb").read())


# ---- the bundled inputs at the budgets of the thread_order goldens ------------------------------------------------------
def test_bundled_inputs_at_the_golden_budgets(tool, tmp_path):
    f, r, inter, p1 = (bundled(n) for n in ("test.f.fastq", "test.r.fastq", "test.fastq", "problem1.fastq"))
    size = lambda n: os.path.getsize(os.path.join(cu.INPUTS, n))
    Lf, Li, Lp = (fu.reference_batch_len(size(n), paired=True) for n in ("test.f.fastq", "test.fastq", "problem1.fastq"))
    assert (Lf, Lp) == (55152, 205)
    cases = [chain_case([f, r], 4, Lf, 64, threads=4, se=False), chain_case([f, r], 4, Lf, 8, threads=3, se=False),
             chain_case([inter], 8, Li, 64, threads=5, se=False), chain_case([p1], 8, Lp, 64, threads=2, se=False),
             chain_case([inter], 4, fu.reference_batch_len(size("test.fastq")), 64, threads=16, se=True)]
    got = run(tool, cases, tmp_path)
    c, tab = check_chain(got[0], [f, r], "pe_split", Lf, threads=4)
    assert c["batches"] == 8 and np.diff(tab).max() == 158 and np.diff(tab).min() == 144
    check_chain(got[1], [f, r], "pe_split", Lf, threads=3)  # a table of exactly the batches
    c, tab = check_chain(got[2], [inter], "pe_interleaved", Li, threads=5)
    assert c["batches"] == 8 and np.diff(tab).max() * 2 == 316 and np.diff(tab).min() * 2 == 288
    c, tab = check_chain(got[3], [p1], "pe_interleaved", Lp, threads=2)
    assert c["batches"] == 0 and tab == [0]  # the reference's reader ends this run at its first batch
    check_chain(got[4], [inter], "se", fu.reference_batch_len(size("test.fastq")), threads=16)


def test_synthetic_golden_inputs(tool, tmp_path):
    cu.prepare_inputs(tmp_path)
    lines = {n: fu.file_lines(open(str(tmp_path / n), "rb").read()) for n in ("syn_R1.fastq", "syn_R2.fastq",
                                                                              "syn_mixed_inter.fastq")}
    L1 = fu.reference_batch_len(os.path.getsize(str(tmp_path / "syn_R1.fastq")), paired=True)
    L3 = fu.reference_batch_len(os.path.getsize(str(tmp_path / "syn_mixed_inter.fastq")), paired=True)
    pair = [lines["syn_R1.fastq"], lines["syn_R2.fastq"]]
    got = run(tool, [chain_case(pair, 4, L1, 32, threads=16, se=False),
                     chain_case([lines["syn_mixed_inter.fastq"]], 8, L3, 32, threads=7, se=False)], tmp_path)
    assert check_chain(got[0], pair, "pe_split", L1, threads=16)[0]["batches"] == 8
    assert check_chain(got[1], [lines["syn_mixed_inter.fastq"]], "pe_interleaved", L3, threads=7)[0]["batches"] == 8


# ---- random line tables ------------------------------------------------------------------------------------------------
def random_lines(rng, batch_len):
    """line lengths from 0 to batch_len - 2 (the longest the call takes), with runs of empty lines and of lines at
    batch_len - 2; every so often one of batch_len - 1, which only the chain (not the call) takes"""
    n = rng.randrange(0, 200)
    top = batch_len - 2
    kind = rng.randrange(4)
    out = []
    for _ in range(n):
        x = rng.random()
        if x < 0.15:
            k = 0
        elif x < 0.19:
            k = top
        elif x < 0.20:
            k = top + 1
        elif kind < 2:
            k = rng.randrange(0, min(top, 6) + 1)
        elif kind == 2:
            k = rng.randrange(0, top // 3 + 1)
        else:
            k = rng.randrange(0, top + 1)
        out.append(b"x" * k)
    return out


def test_random_line_tables(tool, tmp_path):
    rng = random.Random(20260)
    cases, params = [], []
    for it in range(2400):
        batch_len = rng.choice([20, 20, 21, 24, 33, 64, 100, 257, 1000])
        m = rng.choice([4, 8])
        threads = rng.randrange(1, 12)
        lines = random_lines(rng, batch_len)
        limit = rng.choice([0, 0, 0, 1, 2, 5])
        cases.append(chain_case([lines], m, batch_len, len(lines) // m + 2, limit, threads, se=m == 4))
        params.append((lines, m, batch_len, limit, threads))
    got = run(tool, cases, tmp_path)
    batches = 0
    for res, (lines, m, batch_len, limit, threads) in zip(got, params):
        batches += check_chain(res, [lines], MODES[m], batch_len, limit, threads)[0]["batches"]
    assert batches > 2400  # the generator: more than one batch per table on average


def test_table_too_small(tool, tmp_path):
    lines = [b"x" * 5] * 400  # 100 records of 20 bytes at a budget of 20: a batch per record
    want = om.batch_tables([lines], "se", 20)
    nb = len(want["first_unit"]) - 1
    assert nb > 10
    got = run(tool, [chain_case([lines], 4, 20, nb), chain_case([lines], 4, 20, nb - 1), chain_case([lines], 4, 20, 1)],
              tmp_path)
    assert split_chain(got[0])[0]["overflow"] == 0 and split_chain(got[0])[1] == want["first_unit"]
    for res, cap in ((got[1], nb - 1), (got[2], 1)):
        c, tab, _ = split_chain(res)
        assert c["overflow"] == 1 and c["batches"] == cap and tab == want["first_unit"][:cap + 1]


# ---- PE split ------------------------------------------------------------------------------------------------------------
def records(n, length):
    return [b"x" * length] * (4 * n)


@pytest.mark.parametrize("where", ["batch0", "middle", "ends_first", "same"])
def test_split_tables(tool, tmp_path, where):
    L = 100
    a = records(40, 11)
    if where == "batch0":
        b = [b"x" * 60] + a[1:]
    elif where == "middle":
        b = a[:60] + [b"x" * 60] + a[61:]
    elif where == "ends_first":
        b = a[:80]
    else:
        b = list(a)
    got = run(tool, [chain_case([a, b], 4, L, 64, threads=3, se=False)], tmp_path)
    c, tab = check_chain(got[0], [a, b], "pe_split", L, threads=3)
    want = {"batch0": (0, 1), "middle": (None, 1), "ends_first": (None, 0), "same": (None, 0)}[where]
    assert c["mismatch"] == want[1]
    if want[0] is not None:
        assert c["batches"] == want[0]
    if where == "middle":
        assert 0 < c["batches"] < split_chain(run(tool, [chain_case([a, a], 4, L, 64, se=False)], tmp_path)[0])[0]["batches"]
    if where == "ends_first":
        assert c["batches"] > 0 and c["lines1"] <= 80 and c["lines0"] == c["lines1"]


def test_random_split_tables(tool, tmp_path):
    rng = random.Random(977)
    cases, params = [], []
    for it in range(300):
        batch_len = rng.choice([20, 33, 100, 257])
        a = random_lines(rng, batch_len)
        b = list(a)
        for _ in range(rng.randrange(0, 3)):  # a few lines of another length, or a shorter file
            if b and rng.random() < 0.7:
                b[rng.randrange(len(b))] = b"x" * rng.randrange(0, batch_len - 1)
            else:
                b = b[:rng.randrange(0, len(b) + 1)]
        threads = rng.randrange(1, 9)
        cases.append(chain_case([a, b], 4, batch_len, max(len(a), len(b)) // 4 + 2, 0, threads, se=False))
        params.append(([a, b], batch_len, threads))
    for res, (ll, batch_len, threads) in zip(run(tool, cases, tmp_path), params):
        check_chain(res, ll, "pe_split", batch_len, 0, threads)


# ---- the rank map ---------------------------------------------------------------------------------------------------------
def order_by_the_model(n, threads, se):
    """the order in which fastq_util's restatement of the reference writes a batch of n units"""
    lines = []
    for k in range(n):
        lines += [b"@%d" % k, b"A", b"+", b"I"]
    if se:
        text = b"".join(fu.expected_se_output([lines], lambda f, r: (0, 1), threads))
    else:
        text = b"".join(c[0] for c in fu.expected_pe_outputs([lines], [lines], lambda f, r: (0, 1), threads))
    return [int(x[1:]) for x in text.split(b"\n")[0::4] if x]


def test_unit_order_is_the_models():
    for threads in (1, 2, 3, 7, 70):
        for n in (0, 1, 2, 6, 7, 8, 69, 70, 71, 200):
            for se in (True, False):
                assert om.unit_order(n, threads, se) == order_by_the_model(n, threads, se)


def test_rank_map(tool, tmp_path):
    """T 1..70, n 0..200, both orders: every batch size as one batch of a table, so the lanes also step across batch
    ends at every offset; and n = 0 as the empty table."""
    first_unit = [int(x) for x in np.concatenate(([0], np.cumsum(np.arange(1, 201))))]
    cases = [walk_case(t, se, fu_) for t in range(1, 71) for se in (True, False) for fu_ in (first_unit, [0])]
    got = run(tool, cases, tmp_path)
    i = 0
    for t in range(1, 71):
        for se in (True, False):
            assert [int(x) for x in got[i]] == want_units(first_unit, t, se), (t, se)
            assert len(got[i + 1]) == 0
            i += 2


# ---- the model against the reference's recorded runs ----------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cu.e2e()["thread_order"].keys()) + ["pe_problem1_inter"])
def test_model_reproduces_thread_order_goldens(tmp_path, name):
    """What the GPU suite holds the device to is the reference's behaviour: the model, from the input files as they are,
    writes every recorded output of the -a T runs byte for byte."""
    import hashlib
    import trim_model as tm
    from test_fastq_api import golden_texts
    cu.prepare_inputs(tmp_path)
    e2e = cu.e2e()
    rec = e2e["thread_order"].get(name) or e2e["runs"][name]
    argv = rec["argv"]
    mode, texts, files = golden_texts(argv, tmp_path)
    first = argv[argv.index("-c" if "-c" in argv else "-f") + 1].format(inputs=cu.INPUTS, tmp=str(tmp_path))
    batch_len = fu.reference_batch_len(os.path.getsize(first), paired=True)
    res = om.expected(tm.run_params(argv), texts, mode, int(argv[argv.index("-a") + 1]), batch_len)
    assert res["order"]["batches"] == rec.get("batches", 0)
    for fname, want in rec["outputs"].items():
        text = res["texts"][files[fname]]
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname


# ---- the generator of the randomized GPU test ------------------------------------------------------------------------
def test_random_cases_are_valid_and_varied():
    """Every case of the GPU suite's randomized test has outputs to compare: no long line, no verdict, no range error."""
    rng = random.Random(4711)
    seen = {"se": 0, "pe_split": 0, "pe_interleaved": 0}
    batches = stops = kept = 0
    for it in range(100):
        ptuple, texts, mode, threads, batch_len = om.random_case(rng)
        assert 20 <= batch_len <= 4000 and 1 <= threads <= 40
        want = om.expected(ptuple, texts, mode, threads, batch_len)
        assert want["long_line"] is None and want["verdict"] is None and want["range"] is None
        assert want["texts"] is not None
        seen[mode] += 1
        batches += want["order"]["batches"]
        stops += want["order"]["stopped_on_mismatch"]
        kept += sum(len(t) for t in want["texts"] if t)
    assert min(seen.values()) >= 20 and batches > 300 and stops >= 3 and kept > 50000
