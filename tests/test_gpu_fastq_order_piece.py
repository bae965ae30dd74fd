"""GPU: the FASTQ trim in pieces in the reference's -a T order (sk_trim_fastq_ordered_piece_device_async): raw pieces, all
enqueued on one stream before the first finish, each held to tests/fastq_order_piece_model.py (the state it wrote, what
it consumed, ok, the counts, every output and record_index); crafted cuts; failures and the void pieces behind them; and
the drivers Context.trim_fastq_stream / trim_gz_stream / trim_gzip_stream with order= against the reference's recorded
-a T runs and against Context.trim_fastq(order=) on the whole text."""
import ctypes as C
import gzip
import hashlib
import os
import random
import zlib

import numpy as np
import pytest

import cli_util as cu
import fastq_model as fm
import fastq_order_model as om
import fastq_order_piece_model as opm
import fastq_util as fu
import trim_model as tm
from bgzf_raw import surrounded, to_device
from fastq_raw import SENTINEL, torch_mod
from sickle_amd import capi
from test_fastq_api import golden_texts
from test_gpu_fastq_chain import place

pytestmark = pytest.mark.gpu
PT = ("sanger", 20, 5, False, False)  # -l 5: the crafted records of 11 bases are kept
GUARD = 64
BAD = b"@bad\nACGT\n+\nIII\n"
LOW = b"@low\n" + b"ACGT" * 10 + b"\n+\nII\x1f" + b"I" * 37 + b"\n"  # a quality byte below sanger's range


def rec(k, n=11):
    """a record of four lines of n bytes each (k < 10 ** (n - 2))"""
    name = (b"@%d" % k).ljust(n, b"x")
    return name + b"\n" + (b"ACGT" * n)[:n] + b"\n+" + name[2:] + b"x\n" + b"I" * n + b"\n"


# ---- the harness: a sequence of raw pieces on the same buffers -----------------------------------------------------------
def model_sequence(ptuple, texts, mode, threads, batch_len, capacity, steps, limit=0, short=None):
    """the model's piece for every step (see run_sequence), each from the state and behind the carry of the one before;
    every piece behind a range error finds the stream's word set, since no finish comes in between"""
    n_in = len(texts)
    want, state, base, range_set = [], None, [0] * n_in, False
    for j, (ns, more) in enumerate(steps):
        windows = [texts[i][base[i]:ns[i]] for i in range(n_in)]
        p = opm.piece(ptuple, windows, mode, more, threads, batch_len, capacity, limit, state, range_set,
                      fits=not (short and j in short))
        p["base"], p["ns"] = list(base), list(ns)
        want.append(p)
        state = p["state"]
        range_set = range_set or p["range"] is not None
        base = [base[i] + p["consumed"][i] for i in range(n_in)]
    return want


def run_sequence(ctx, ptuple, texts, mode, threads, batch_len, capacity, steps, limit=0, short=None, shift=3, ws=None,
                 seen=None, surround=None):
    """steps: [(n per input, more)]: piece j's window is [what piece j - 1 did not consume, n) of each text: its start is
    the consumed word piece j - 1 published, its end a device word, so the windows are the stream's (the carry and the
    next chunk).  Piece j reads state j and writes state j + 1.  Every piece is enqueued before the first finish.  short:
    {piece: output} whose capacity is one byte less than it needs.  Each piece is compared with opm.piece on the
    model's own windows.  ws: one workspace tensor per step, each used as it is (the byte count handed to the library stays
    the formula's); seen: a list that takes, per piece, (rc, counts, the state it wrote, the words it published, every
    output tensor as bytes).  -> the model's pieces."""
    torch = torch_mod()
    L = capi.lib()
    params = capi.make_params(*ptuple)
    n_in = len(texts)
    want = model_sequence(ptuple, texts, mode, threads, batch_len, capacity, steps, limit, short)  # also: what a short output needs
    if surround is None:
        bufs = [place(t, shift + 5 * i) for i, t in enumerate(texts)]
    else:  # what lies around the texts (bgzf_raw.surrounded)
        bufs = [surrounded(t, (shift + 5 * i) % 16, 0, surround) for i, t in enumerate(texts)]
    order = capi.FastqOrder(threads, 0, batch_len, capacity, limit)
    states = torch.zeros((len(steps) + 1, 8), dtype=torch.int64, device="cuda")
    ends = torch.tensor([list(ns) + [0] * (2 - n_in) for ns, _ in steps], dtype=torch.int64, device="cuda")
    calls = []
    for j, (ns, more) in enumerate(steps):
        T = sum(ns)
        ws_bytes = L.sk_trim_fastq_ordered_piece_workspace_bytes(T, params.trunc_n, capacity)
        step_ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda") if ws is None else ws[j]
        cap, rcap = T + 64, T // 4 + 4
        outs, keep, caps = [], [], []
        for o in range(3):
            c = cap
            if short and short.get(j) == o:
                c = len(want[j]["texts"][o]) - 1
            t = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
            ix = torch.full((rcap + GUARD,), -7, dtype=torch.int64, device="cuda")
            outs.append(capi.FastqOutput(t.data_ptr(), c, ix.data_ptr(), rcap))
            keep.append((t, ix))
            caps.append(c)
        prev = calls[-1]["ws"].data_ptr() if calls else None
        starts = [capi.Context.trim_fastq_piece_words(prev, i)[0] if prev else None for i in range(n_in)]
        ctx.trim_fastq_ordered_piece_device_async(params, [b[1] for b in bufs], list(ns), order, states[j].data_ptr(),
                                                  states[j + 1].data_ptr(), outs, step_ws.data_ptr(), ws_bytes,
                                                  bytes_dev_ptrs=[ends[j, i:].data_ptr() for i in range(n_in)],
                                                  start_dev_ptrs=starts, more=more, mode=mode)
        calls.append({"ws": step_ws, "keep": keep, "caps": caps, "cap": cap, "rcap": rcap})
    host_states = None
    for j, (call, p) in enumerate(zip(calls, want)):
        rc, _, counts = ctx._ordered_piece_finish(call["ws"].data_ptr(), None)
        if host_states is None:
            host_states = states.cpu().numpy()  # everything has run now
        tag = "piece %d of %d" % (j, len(steps))
        if p["inherited_range"]:
            rc_want = capi.SK_ERANGE
        elif p["inherited_failure"]:
            rc_want = capi.SK_OK
        elif p["long_line"] is not None:
            rc_want = capi.SK_ELONGLINE
        elif p["verdict"] is not None:
            rc_want = capi.SK_EFORMAT
        elif p["range"] is not None:
            rc_want = capi.SK_ERANGE
        else:
            rc_want = capi.SK_OK if p["ok"] else capi.SK_ESPACE
        assert rc == rc_want, (tag, capi.lib().sk_last_error(ctx._h))
        assert counts["records_in"] == p["records_in"] and counts["tail_lines"] == p["tail_lines"], tag
        assert counts["dropped_unpaired"] == 0, tag
        pc, oc, opc = counts["piece"], counts["order"], counts["order_piece"]
        assert pc["consumed"][:n_in] == [p["base"][i] + p["consumed"][i] for i in range(n_in)], tag
        assert pc["carried_bytes"][:n_in] == p["carried_bytes"][:n_in], tag
        assert pc["ok"] == p["ok"] and pc["inherited_range"] == p["inherited_range"], tag
        for key in ("batches", "units", "last_batch_units", "records_unbatched", "stopped_on_mismatch"):
            assert oc[key] == p["order"][key], (tag, key)
        assert oc["error_batch"] == p["error_batch"], tag
        assert (opc["table_full"], opc["undetermined"], opc["inherited_failure"]) == \
            (p["table_full"], p["undetermined"], p["inherited_failure"]), tag
        assert opc["state"] == p["state"], tag
        dev_state = capi.FastqOrderState.from_buffer_copy(host_states[j + 1].tobytes()).as_dict()
        assert dev_state == p["state"], tag  # what the next piece started from
        published = []
        for i in range(n_in):  # the words a carry would go by
            words = capi.Context.trim_fastq_piece_words(call["ws"].data_ptr(), i)
            hdr = call["ws"][:256].cpu().numpy().view(np.uint64)
            got = [int(hdr[(w - call["ws"].data_ptr()) // 8]) for w in words]
            assert got == [p["base"][i] + p["consumed"][i], p["ns"][i], p["ok"]], tag
            published.append(got)
        if seen is not None:
            seen.append((rc, counts, host_states[j + 1].tobytes(), published,
                         [(t.cpu().numpy().tobytes(), ix.cpu().numpy().tobytes()) for t, ix in call["keep"]]))
        if p["long_line"] is not None and not p["inherited_range"] and not p["inherited_failure"]:
            assert (oc["long_line_input"], oc["long_line"]) == p["long_line"], tag
        if rc == capi.SK_EFORMAT:
            assert (counts["format_error"], counts["format_input"], counts["format_record"]) == p["verdict"], tag
        if rc == capi.SK_ERANGE:
            assert p["inherited_range"] or counts["range"] == tuple(p["range"]), tag
        for t, ix in call["keep"]:
            assert bool((t[call["cap"]:] == SENTINEL).all()) and bool((ix[call["rcap"]:] == -7).all()), "a guard was written"
        if rc not in (capi.SK_OK, capi.SK_ESPACE) or p["inherited_failure"]:
            for t, ix in call["keep"]:
                assert bool((t == SENTINEL).all()) and bool((ix == -7).all()), (tag, "written after an error")
            continue
        for o in range(3):
            t, ix = call["keep"][o]
            if o not in fm.USED[mode]:
                assert bool((t == SENTINEL).all())
                continue
            assert counts["records"][o] == len(p["index"][o]) and counts["bytes"][o] == len(p["texts"][o]), (tag, o)
            if call["caps"][o] < len(p["texts"][o]):  # the output that did not fit is not written (the others are, as in
                assert rc == capi.SK_ESPACE          # every FASTQ call)
                assert bool((t == SENTINEL).all()) and bool((ix == -7).all()), (tag, "written beyond its capacity")
                continue
            n, r = counts["bytes"][o], counts["records"][o]
            assert t[:n].cpu().numpy().tobytes() == p["texts"][o], (tag, "output %d" % o)
            assert bool((t[n:] == SENTINEL).all()) and bool((ix[r:] == -7).all()), tag
            assert np.array_equal(ix[:r].cpu().numpy(), p["index"][o]), (tag, "record_index %d" % o)
    return want


def chunked(texts, chunk):
    """the steps of a stream cut into chunks of `chunk` bytes, every input alike (closing pieces are added by the caller)"""
    longest = max(len(t) for t in texts)
    n = max(1, -(-longest // chunk))
    return [([min((k + 1) * chunk, len(t)) for t in texts], k + 1 < n) for k in range(n)]


def with_closing(ptuple, texts, mode, threads, batch_len, capacity, steps, limit=0):
    """steps plus the closing pieces a caller repeats while the table was full (the model tells how many)"""
    got = opm.stream(ptuple, texts, mode, threads, batch_len, max(steps[0][0]) if len(steps) > 1 else max(len(t) for t in texts) or 1,
                     capacity, limit, stop_at_end=False, keep_pieces=True)
    extra = len(got["pieces"]) - len(steps) if got["error"] is None else 0
    return steps + [steps[-1]] * max(extra, 0)


# ---- 1 drawn texts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", range(4))
@pytest.mark.parametrize("chunk", [64, 500, 4096])
def test_raw_pieces_on_drawn_texts(sk_ctx, chunk, group):
    """324 draws of the ordered call's generator (T 1..40, batch_len from its longest line + 2 to 4 000), 27 per case:
    the whole stream enqueued, then every piece against the model, and the pieces' outputs together against the whole
    text's."""
    rng = random.Random(1000 * chunk + group)
    for it in range(27):
        ptuple, texts, mode, threads, batch_len = om.random_case(rng)
        capacity = rng.choice([1, 2, 5, 1000])
        steps = with_closing(ptuple, texts, mode, threads, batch_len, capacity, chunked(texts, chunk))
        pieces = run_sequence(sk_ctx, ptuple, texts, mode, threads, batch_len, capacity, steps, shift=it % 16)
        whole = om.expected(ptuple, texts, mode, threads, batch_len)
        for o in fm.USED[mode]:
            assert b"".join(p["texts"][o] for p in pieces) == whole["texts"][o], (it, o)
        assert pieces[-1]["state"]["batches"] == whole["order"]["batches"] and pieces[-1]["state"]["ended"] == 1


# ---- 2 crafted cuts -------------------------------------------------------------------------------------------------------
def test_carried_lines_of_every_count(sk_ctx):
    """uniform records of 44 bytes of content: budgets that leave k = 1, 2, 3 lines taken beyond a batch (m = 4), and
    5, 6, 7 (m = 8)"""
    text = b"".join(rec(k) for k in range(64))
    for mode, budgets, wanted in (("se", (45, 100, 75), {1, 2, 3}), ("pe_interleaved", (133, 150, 160), {5, 6, 7})):
        seen = set()
        for L in budgets:
            steps = with_closing(PT, [text], mode, 3, L, 64, chunked([text], 300))
            pieces = run_sequence(sk_ctx, PT, [text], mode, 3, L, 64, steps)
            seen |= {p["state"]["carried"][0] for p in pieces[:-1]}
        assert wanted <= seen, (mode, seen)


def test_window_end_swept_across_a_stop_line(sk_ctx):
    """L = 100 on lines of 11 bytes: the budget is used up on line 9, whose '\\n' is byte 119.  One byte before, the batch
    is undetermined and the piece commits nothing; from that byte on it commits lines [0, 8) and carries two."""
    text = b"".join(rec(k) for k in range(8))
    for n in range(110, 125):
        p = run_sequence(sk_ctx, PT, [text], "se", 2, 100, 8, [([n], True)])[0]
        assert p["undetermined"] == 1
        assert (p["order"]["batches"], p["state"]["carried"][0], p["consumed"][0]) == ((0, 0, 0) if n < 120 else (1, 2, 96)), n
    # the same sweep inside a stream: the first piece ends around the stop line, the second one takes up from its state
    for n in (118, 119, 120, 121):
        ps = run_sequence(sk_ctx, PT, [text], "se", 2, 100, 8, [([n], True), ([len(text)], False)])
        assert b"".join(p["texts"][0] for p in ps) == om.expected(PT, [text], "se", 2, 100)["texts"][0]


def test_full_table_and_repeated_closing_pieces(sk_ctx):
    text = b"".join(rec(k) for k in range(40))
    whole = om.expected(PT, [text], "se", 5, 100)
    assert whole["order"]["batches"] >= 15
    # everything in one closing piece, then closing pieces on the carry alone until one is not full
    steps = with_closing(PT, [text], "se", 5, 100, 1, [([len(text)], False)])
    assert len(steps) == whole["order"]["batches"]
    ps = run_sequence(sk_ctx, PT, [text], "se", 5, 100, 1, steps)
    assert all(p["table_full"] == 1 and p["order"]["batches"] == 1 and p["ok"] == 1 for p in ps[:-1])
    assert ps[-1]["table_full"] == 0 and ps[-1]["state"]["ended"] == 1
    assert b"".join(p["texts"][0] for p in ps) == whole["texts"][0]
    # a table of one in every piece of a stream
    steps = with_closing(PT, [text], "se", 5, 100, 1, chunked([text], 500))
    ps = run_sequence(sk_ctx, PT, [text], "se", 5, 100, 1, steps)
    assert b"".join(p["texts"][0] for p in ps) == whole["texts"][0]


def test_run_ends_mid_stream(sk_ctx):
    """an empty batch (two lines use the budget up) and a split mismatch: the pieces behind take nothing and stay ok"""
    head = b"".join(rec(k) for k in range(20))
    tail = b"".join(rec(k) for k in range(20, 40))
    stop = b"@" + b"x" * 59 + b"\n" + b"A" * 60 + b"\n+\n" + b"I" * 60 + b"\n"  # lines of 60 bytes at L = 100
    text = head + stop + tail
    steps = chunked([text], 400)
    ps = run_sequence(sk_ctx, PT, [text], "se", 2, 100, 64, steps)
    first = next(j for j, p in enumerate(ps) if p["state"]["ended"])
    assert 0 < first < len(ps) - 2 and ps[first]["state"]["stopped_on_mismatch"] == 0
    for p in ps[first + 1:]:
        assert p["ok"] == 1 and p["order"]["batches"] == 0 and p["consumed"][0] == 0 and p["state"] == ps[first]["state"]
    assert b"".join(p["texts"][0] for p in ps) == om.expected(PT, [text], "se", 2, 100)["texts"][0]
    a = b"".join(rec(k) for k in range(60))
    b = b"".join(rec(k) if k != 31 else rec(k, 40) for k in range(60))
    whole = om.expected(PT, [a, b], "pe_split", 3, 100)
    assert whole["order"]["stopped_on_mismatch"] == 1
    ps = run_sequence(sk_ctx, PT, [a, b], "pe_split", 3, 100, 64, chunked([a, b], 400))
    first = next(j for j, p in enumerate(ps) if p["state"]["ended"])
    assert 0 < first < len(ps) - 2 and ps[first]["order"]["stopped_on_mismatch"] == 1
    for p in ps[first + 1:]:
        assert p["ok"] == 1 and p["order"]["batches"] == 0 and p["order"]["stopped_on_mismatch"] == 0
        assert p["state"]["stopped_on_mismatch"] == 1
    for o in range(3):
        assert b"".join(p["texts"][o] for p in ps) == whole["texts"][o]


def test_batch_limit_reached_in_the_third_piece(sk_ctx):
    text = b"".join(rec(k) for k in range(40))
    steps = chunked([text], 130)  # a batch is 8 lines of 12 bytes: about one per piece
    ps = run_sequence(sk_ctx, PT, [text], "se", 4, 100, 64, steps, limit=3)
    assert [p["state"]["ended"] for p in ps[:3]] == [0, 0, 1] and ps[2]["state"]["batches"] == 3
    assert all(p["order"]["batches"] == 0 and p["ok"] == 1 for p in ps[3:])
    assert b"".join(p["texts"][0] for p in ps) == om.expected(PT, [text], "se", 4, 100, 3)["texts"][0]


# ---- 3 failures ------------------------------------------------------------------------------------------------------------
def test_malformed_record_in_a_batch_and_in_the_carry(sk_ctx):
    recs = [rec(k) for k in range(30)]
    text = b"".join(recs[:17]) + BAD + b"".join(recs[17:])
    at = len(b"".join(recs[:17]))
    # the first piece ends inside the record behind BAD: BAD is complete but no batch that holds it can be told yet
    steps = [([at + len(BAD) + 5], True), ([len(text)], True), ([len(text)], True), ([len(text)], False)]
    ps = run_sequence(sk_ctx, PT, [text], "se", 2, 200, 64, steps)
    assert ps[0]["ok"] == 1 and ps[0]["verdict"] is None and ps[0]["order"]["batches"] > 0
    assert ps[0]["tail_lines"][0] >= 4  # BAD sits in the carry
    assert ps[1]["verdict"] == (fm.SK_FQ_LENGTHS, 0, 17 - ps[0]["records_in"][0])
    assert ps[1]["error_batch"] == om.expected(PT, [text], "se", 2, 200)["error_batch"]  # stream-wide
    for p in ps[2:]:  # two void pieces behind the failure
        assert p["inherited_failure"] == 1 and p["ok"] == 0 and p["state"]["failed"] == 1 and p["records_in"] == [0, 0]


def test_range_error_with_pieces_in_flight(sk_ctx):
    recs = [rec(k) for k in range(30)]
    text = b"".join(recs[:9]) + LOW + b"".join(recs[9:])
    steps = [([400], True), ([900], True), ([1200], True), ([len(text)], False)]
    ps = run_sequence(sk_ctx, PT, [text], "se", 2, 100, 64, steps)
    j = next(j for j, p in enumerate(ps) if p["range"] is not None)
    assert j in (1, 2) and ps[j]["range"][1:] == (2, 0x1f) and ps[j]["error_batch"] >= ps[j - 1]["state"]["batches"]
    for p in ps[j + 1:]:
        assert p["inherited_range"] == 1 and p["inherited_failure"] == 1 and p["ok"] == 0 and p["state"]["failed"] == 1
    assert len(ps[j + 1:]) >= 1
    # the finishes cleared the stream's word: a fresh stream runs
    ps = run_sequence(sk_ctx, PT, [b"".join(recs)], "se", 2, 100, 64, [([len(b"".join(recs))], False)])
    assert ps[0]["ok"] == 1


def test_long_lines(sk_ctx):
    recs = [rec(k) for k in range(30)]
    L = 100
    long_rec = b"@" + b"y" * (L - 2) + b"\nACGT\n+\nIIII\n"  # a name line of batch_len - 1 bytes
    # in a carried line: the first piece ends right behind the long line, in front of any batch that could hold it
    text = b"".join(recs[:12]) + long_rec + b"".join(recs[12:])
    at = len(b"".join(recs[:12]))
    steps = [([at + L], True), ([at + 300], True), ([len(text)], True), ([len(text)], False)]
    ps = run_sequence(sk_ctx, PT, [text], "se", 2, L, 64, steps)
    assert ps[0]["long_line"] is not None and ps[0]["long_line"][0] == 0 and ps[0]["ok"] == 0
    assert all(p["inherited_failure"] == 1 for p in ps[1:])
    # one byte shorter passes
    ok_rec = b"@" + b"y" * (L - 3) + b"\nACGT\n+\nIIII\n"
    text2 = b"".join(recs[:12]) + ok_rec + b"".join(recs[12:])
    ps = run_sequence(sk_ctx, PT, [text2], "se", 2, L, 64, [([at + L], True), ([len(text2)], False)])
    assert all(p["ok"] == 1 for p in ps)
    # behind the run's end: two lines of 60 bytes end the run, the long line comes later and is still refused
    stop = b"@" + b"x" * 59 + b"\n" + b"A" * 60 + b"\n+\n" + b"I" * 60 + b"\n"
    text3 = b"".join(recs[:8]) + stop + b"".join(recs[8:12]) + long_rec + b"".join(recs[12:])
    cut = len(b"".join(recs[:8]) + stop + b"".join(recs[8:12]))
    ps = run_sequence(sk_ctx, PT, [text3], "se", 2, L, 64, [([cut], True), ([len(text3)], True), ([len(text3)], False)])
    assert ps[0]["state"]["ended"] == 1 and ps[0]["ok"] == 1
    assert ps[1]["long_line"] is not None and ps[1]["ok"] == 0 and ps[2]["inherited_failure"] == 1


def test_output_one_byte_short(sk_ctx):
    a = b"".join(rec(k) for k in range(30))
    for mode, texts, out in (("se", [a], 0), ("pe_split", [a, a], 1), ("pe_interleaved", [a], 0)):
        steps = [([600] * len(texts), True), ([1200] * len(texts), True), ([len(a)] * len(texts), True), ([len(a)] * len(texts), False)]
        ps = run_sequence(sk_ctx, PT, texts, mode, 3, 100, 64, steps, short={1: out})
        assert ps[0]["ok"] == 1 and ps[1]["ok"] == 0 and len(ps[1]["texts"][out]) > 1
        assert ps[1]["state"] == dict(ps[0]["state"], failed=1)
        assert all(p["inherited_failure"] == 1 and p["state"]["failed"] == 1 for p in ps[2:])


# ---- 4 the drivers ---------------------------------------------------------------------------------------------------------
def run_stream(stream):
    parts = list(stream)
    return [None if parts[0][o] is None else b"".join(p[o] for p in parts) for o in range(3)], stream


def inflate_all(data):
    """every gzip member of data, one after the other, with Python's zlib (empty members included)"""
    out = []
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        assert d.eof
        data = d.unused_data
    return b"".join(out)


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_order_piece")
    cu.prepare_inputs(d)
    return d


@pytest.mark.parametrize("name", sorted(cu.e2e()["thread_order"].keys()) + ["pe_problem1_inter"])
def test_streams_reproduce_the_thread_order_goldens(sk_ctx, workdir, name):
    e2e = cu.e2e()
    run = e2e["thread_order"].get(name) or e2e["runs"][name]
    argv = run["argv"]
    mode, texts, files = golden_texts(argv, workdir)
    first = argv[argv.index("-c" if "-c" in argv else "-f") + 1].format(inputs=cu.INPUTS, tmp=str(workdir))
    order = (int(argv[argv.index("-a") + 1]), fu.reference_batch_len(os.path.getsize(first), paired=True))
    params = capi.make_params(*tm.run_params(argv))
    dev = [to_device(t) for t in texts]
    whole, counts = sk_ctx.trim_fastq(params, dev[0], dev[1] if len(dev) > 1 else None, mode=mode, order=order)
    whole = [None if w is None else w.cpu().numpy().tobytes() for w in whole]
    room = 2 * order[1] + 65536
    second = texts[1] if len(texts) > 1 else None

    def check(got, st):
        for fname, want in run["outputs"].items():
            text = got[files[fname]]
            assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname
        for o in fm.USED[mode]:
            assert got[o] == whole[o], "output %d" % o
        for key in ("batches", "units", "last_batch_units", "stopped_on_mismatch"):
            assert st.counts["order"][key] == counts["order"][key], key
        assert st.counts["order"]["batches"] == run.get("batches", 0)
        assert st.counts["records"] == counts["records"] and st.counts["bytes"] == counts["bytes"]
    for piece_bytes in (4096, 70001):
        got, st = run_stream(sk_ctx.trim_fastq_stream(params, texts[0], second, mode=mode, piece_bytes=piece_bytes, room=room,
                                                      order=order))
        check(got, st)
    # a table of two batches per piece: shorter pieces, repeated closing pieces, the same files
    got, st = run_stream(sk_ctx.trim_fastq_stream(params, texts[0], second, mode=mode, piece_bytes=70001, room=room,
                                                  order=order, batch_capacity=2))
    check(got, st)
    # BGZF in, BGZF out; plain gzip in
    images = [sk_ctx.bgzf(d).cpu().numpy().tobytes() for d in dev]
    got, st = run_stream(sk_ctx.trim_gz_stream(params, images[0], images[1] if len(images) > 1 else None, mode=mode,
                                               piece_bytes=70001, room=room, order=order))
    check([None if g is None else inflate_all(g) for g in got], st)
    plain = [gzip.compress(t, 6) for t in texts]
    got, st = run_stream(sk_ctx.trim_gzip_stream(params, plain[0], plain[1] if len(plain) > 1 else None, mode=mode,
                                                 piece_bytes=262144, room=room, order=order))
    check([None if g is None else inflate_all(g) for g in got], st)


def test_stream_without_order_is_unchanged(sk_ctx):
    """order=None enqueues the unordered piece call, as before: read order, no order counts"""
    text = b"".join(rec(k) for k in range(200))
    got, st = run_stream(sk_ctx.trim_fastq_stream(capi.make_params(*PT), text, piece_bytes=1000))
    assert got[0] == fm.expected(PT, [text], "se")["texts"][0] and "order" not in st.counts and st.order is None


def test_stall_names_batch_len(sk_ctx):
    params = capi.make_params(*PT)
    with pytest.raises(capi.TrimError, match="batch_len") as e:  # lines that never use the budget up
        run_stream(sk_ctx.trim_fastq_stream(params, b"\n" * 20000, piece_bytes=1024, order=(4, 100)))
    assert e.value.rc == capi.SK_ESPACE
    text = b"".join(rec(k) for k in range(400))
    with pytest.raises(capi.TrimError, match="batch_len"):  # a budget no piece can hold
        run_stream(sk_ctx.trim_fastq_stream(params, text, piece_bytes=1024, order=(4, 5000)))
    got, st = run_stream(sk_ctx.trim_fastq_stream(params, text, piece_bytes=1024, room=8192, order=(4, 5000)))
    assert got[0] == om.expected(PT, [text], "se", 4, 5000)["texts"][0]
