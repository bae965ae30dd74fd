"""GPU: FASTQ text trimmed on the device in the reference's -a T batch order (sk_trim_fastq_ordered_device_async / finish,
Context.trim_fastq(order=...)) against the reference's recorded -a T output files and against tests/fastq_order_model.py:
fastq_util's restatement of the reference's reader and queues on the oracle's cuts."""
import ctypes as C
import hashlib
import os
import random
import zlib

import numpy as np
import pytest

import cli_util as cu
import fastq_order_model as om
import fastq_util as fu
import trim_model as tm
from sickle_amd import capi
from fastq_raw import SENTINEL, texts_of, torch_mod, untouched, upload
from test_fastq_api import golden_texts

pytestmark = pytest.mark.gpu


def to_dev(text):
    return torch_mod().from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()


def raw(ctx, params, texts, mode, threads, batch_len, capacity=None, limit=0, caps=None, shift=0, ws=None, surround=None):
    """One ordered async + finish on raw pointers, every output pre-filled with SENTINEL.  ws: the workspace tensor, used
    as it is (the byte count handed to the library stays the formula's); surround: what lies around the texts.
    -> (rc, counts with "order", keep, table of first units)"""
    torch = torch_mod()
    bufs = [upload(t, shift, surround) for t in texts]
    T = sum(len(t) for t in texts)
    capacity = capacity or T // batch_len + 16
    L = capi.lib()
    ws_bytes = L.sk_trim_fastq_ordered_workspace_bytes(T, params.trunc_n, capacity)
    assert ws_bytes == L.sk_trim_fastq_workspace_bytes(T, params.trunc_n) + (8 * (capacity + 1) + 15) // 16 * 16
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    caps = caps or [T + 64] * 3
    outs, keep = [], []
    for o in range(3):
        t = torch.full((max(caps[o], 16),), SENTINEL, dtype=torch.uint8, device="cuda")
        ix = torch.full((T // 4 + 4,), -7, dtype=torch.int64, device="cuda")
        outs.append(capi.FastqOutput(t.data_ptr(), caps[o], ix.data_ptr(), T // 4 + 4))
        keep.append((t, ix))
    inp = capi.FastqInput((C.c_void_p * 2)(*([b[1] for b in bufs] + [None] * (2 - len(bufs)))),
                          (C.c_uint64 * 2)(*([len(t) for t in texts] + [0] * (2 - len(texts)))), 0)
    order = capi.FastqOrder(threads, 0, batch_len, capacity, limit)
    rc = L.sk_trim_fastq_ordered_device_async(ctx._h, C.byref(params), C.byref(inp), capi.TRIM_MODES[mode], C.byref(order),
                                              (capi.FastqOutput * 3)(*outs), ws.data_ptr(), ws_bytes, None)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    c, oc = capi.FastqCounts(), capi.FastqOrderCounts()
    rc = L.sk_trim_fastq_ordered_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(oc))
    counts = dict(c.as_dict(), order=oc.as_dict())
    nb = min(counts["order"]["batches"], capacity)
    at = capi.Context.trim_fastq_ordered_batches(ws.data_ptr()) - ws.data_ptr()
    assert at == 256
    table = ws[at:at + 8 * (nb + 1)].cpu().numpy().view(np.uint64).astype(np.int64).tolist()
    return rc, counts, keep, table


def check(ctx, ptuple, texts, mode, threads, batch_len, limit=0, **kw):
    """The device against the model: the order counts and the table, then the verdict, the range error or every output
    text, index and count."""
    want = om.expected(ptuple, texts, mode, threads, batch_len, limit)
    rc, counts, keep, table = raw(ctx, capi.make_params(*ptuple), texts, mode, threads, batch_len, limit=limit, **kw)
    assert counts["records_in"] == want["records_in"] and counts["tail_lines"] == want["tail_lines"]
    assert counts["dropped_unpaired"] == 0
    oc = counts["order"]
    assert {k: oc[k] for k in want["order"]} == want["order"]
    assert table == want["tables"]["first_unit"]
    assert oc["error_batch"] == want["error_batch"]
    if want["long_line"] is not None:
        assert rc == capi.SK_ELONGLINE and (oc["long_line_input"], oc["long_line"]) == want["long_line"]
        assert counts["records"] == [0, 0, 0] and counts["bytes"] == [0, 0, 0]
        untouched(keep)
        return rc, counts, None
    if want["verdict"] is not None:
        assert rc == capi.SK_EFORMAT
        assert (counts["format_error"], counts["format_input"], counts["format_record"]) == want["verdict"]
        untouched(keep)
        return rc, counts, None
    if want["range"] is not None:
        assert rc == capi.SK_ERANGE and counts["range"] == want["range"]
        untouched(keep)
        return rc, counts, None
    assert rc == capi.SK_OK, capi.lib().sk_last_error(ctx._h)
    got = texts_of(keep, counts)
    for o in range(3):
        if want["texts"][o] is None:
            assert counts["records"][o] == 0 and bool((keep[o][0] == SENTINEL).all())
            continue
        assert got[o] == want["texts"][o], "output %d" % o
        assert counts["records"][o] == len(want["index"][o]) and counts["bytes"][o] == len(want["texts"][o])
        assert np.array_equal(keep[o][1][:counts["records"][o]].cpu().numpy(), want["index"][o]), "index %d" % o
        assert bool((keep[o][0][counts["bytes"][o]:] == SENTINEL).all()) and bool((keep[o][1][counts["records"][o]:] == -7).all())
    return rc, counts, got


# ---- 1 the reference's -a T runs -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_order_gpu")
    cu.prepare_inputs(d)
    return d


def budget(argv, workdir):
    first = argv[argv.index("-c" if "-c" in argv else "-f") + 1]
    return fu.reference_batch_len(os.path.getsize(first.format(inputs=cu.INPUTS, tmp=str(workdir))), paired=True)


@pytest.mark.parametrize("name", sorted(cu.e2e()["thread_order"].keys()) + ["pe_problem1_inter"])
def test_reference_thread_order_runs_from_fastq_text(sk_ctx, workdir, name):
    """The input files uploaded byte for byte, trimmed in the order of the run's -a T at the reader's budget for the
    file's size: the recorded md5 and size of every output.  pe_problem1_inter: the reference's reader ends the run at
    its first batch, so both outputs are empty."""
    e2e = cu.e2e()
    rec = e2e["thread_order"].get(name) or e2e["runs"][name]
    argv = rec["argv"]
    mode, texts, files = golden_texts(argv, workdir)
    threads = int(argv[argv.index("-a") + 1])
    tt = [to_dev(t) for t in texts]
    outs, counts = sk_ctx.trim_fastq(capi.make_params(*tm.run_params(argv)), tt[0], tt[1] if len(tt) > 1 else None,
                                     mode=mode, order=(threads, budget(argv, workdir)))
    assert counts["order"]["batches"] == rec.get("batches", 0)
    for fname, want in rec["outputs"].items():
        text = outs[files[fname]].cpu().numpy().tobytes()
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname


# ---- 2 SE at many T ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def test_fastq():
    return open(os.path.join(cu.INPUTS, "test.fastq"), "rb").read()


SE_PARAMS = ("illumina", 20, 20, False, False)


@pytest.mark.parametrize("threads", [1, 2, 3, 5, 16, 64, 1000])
def test_se_thread_counts(sk_ctx, test_fastq, threads):
    batch_len = fu.reference_batch_len(len(test_fastq))
    _, counts, got = check(sk_ctx, SE_PARAMS, [test_fastq], "se", threads, batch_len)
    assert counts["order"]["batches"] == 8


def test_one_thread_one_batch_is_the_unordered_call(sk_ctx, test_fastq):
    _, counts, got = check(sk_ctx, SE_PARAMS, [test_fastq], "se", 1, len(test_fastq) + 1)
    assert counts["order"]["batches"] == 1
    outs, _ = sk_ctx.trim_fastq(capi.make_params(*SE_PARAMS), to_dev(test_fastq), mode="se")
    assert got[0] == outs[0].cpu().numpy().tobytes()


# ---- 3 block and lane edges ------------------------------------------------------------------------------------------
def edge_record(k, tag=b""):
    """47 bytes of lines; every third read is dropped, so some pairs lose a mate"""
    qual = (b"#" if k % 3 == 2 else b"I") * 20
    return b"@r%04d%s\n" % (k, tag) + b"ACGTTGCAACGTTGCAACGT\n+\n" + qual + b"\n"


@pytest.fixture(scope="module")
def edge_texts():
    se = b"".join(edge_record(k) for k in range(5000))
    # mates 2k, 2k + 1 of the same 5 000 reads: 47 bytes of lines each (the tag replaces a digit)
    split = [b"".join(edge_record(k)[:2] + b"a" + edge_record(k)[3:] for k in range(0, 5000, 2)),
             b"".join(edge_record(k)[:2] + b"b" + edge_record(k)[3:] for k in range(1, 5000, 2))]
    return {"se": [se], "pe_split": split, "pe_interleaved": [se]}


EDGE_PARAMS = ("sanger", 20, 20, False, False)
# (mode, units per batch, T): batch ends on the blocks' edges (2 048 reads = 1 024 pairs), just before and behind them
# and inside one lane's ranks; last batches shorter than T (906 reads, 454 / 452 pairs); batches of one unit
EDGES = [("se", 2047, 2), ("se", 2048, 7), ("se", 2049, 2048), ("se", 2043, 2049), ("se", 1, 7),
         ("pe_split", 2047, 2), ("pe_split", 1024, 7), ("pe_split", 1025, 2048), ("pe_split", 1023, 2049),
         ("pe_split", 1, 2), ("pe_interleaved", 2047, 7), ("pe_interleaved", 1024, 2), ("pe_interleaved", 1025, 2049),
         ("pe_interleaved", 1023, 2048), ("pe_interleaved", 1, 7)]


@pytest.mark.parametrize("mode,per_batch,threads", EDGES)
def test_block_and_lane_edges(sk_ctx, edge_texts, mode, per_batch, threads):
    batch_len = 47 * per_batch * (2 if mode == "pe_interleaved" else 1)
    _, counts, got = check(sk_ctx, EDGE_PARAMS, edge_texts[mode], mode, threads, batch_len)
    units = 5000 if mode == "se" else 2500
    oc = counts["order"]
    assert oc["units"] == units and oc["batches"] == -(-units // per_batch)
    assert oc["last_batch_units"] == (units % per_batch or per_batch)
    assert counts["records"][0] > 0 and (mode == "se" or counts["records"][2] > 0)


# ---- 4 PE split whose tables differ ---------------------------------------------------------------------------------------
def split_pair(plant_format=None, plant_range=None):
    """40 pairs, ten to a batch at a budget of 470; text 2's record 25 has a name 54 bytes longer, so its batch 2 uses
    the budget up inside record 28 and holds eight records.  plant_*: the pair whose mate 1 starts with 'X' / whose mate 2 has a quality below the range."""
    a = [edge_record(3 * k) for k in range(40)]
    b = [edge_record(3 * k + 1) for k in range(40)]
    b[25] = b"@r0076" + b"_" * 54 + b"\n" + b[25].split(b"\n", 1)[1]
    if plant_format is not None:
        a[plant_format] = b"X" + a[plant_format][1:]
    if plant_range is not None:
        r = b[plant_range].split(b"\n")
        r[3] = r[3][:7] + b"\x1f" + r[3][8:]
        b[plant_range] = b"\n".join(r)
    return [b"".join(a), b"".join(b)]


def test_split_stops_at_the_first_different_batch(sk_ctx):
    for texts in (split_pair(), split_pair(plant_format=33, plant_range=31)):
        rc, counts, got = check(sk_ctx, EDGE_PARAMS, texts, "pe_split", 3, 470)
        oc = counts["order"]
        assert rc == capi.SK_OK and (oc["batches"], oc["units"], oc["stopped_on_mismatch"]) == (2, 20, 1)
        assert oc["records_unbatched"] == [20, 20] and got[0].count(b"\n") == 4 * counts["records"][0] > 0


def test_split_errors_inside_the_batches(sk_ctx):
    rc, counts, _ = check(sk_ctx, EDGE_PARAMS, split_pair(plant_format=12, plant_range=15), "pe_split", 3, 470)
    assert rc == capi.SK_EFORMAT and counts["order"]["error_batch"] == 1
    assert (counts["format_error"], counts["format_input"], counts["format_record"]) == (capi.SK_FQ_ID_NO_AT, 0, 12)
    rc, counts, _ = check(sk_ctx, EDGE_PARAMS, split_pair(plant_range=15), "pe_split", 3, 470)
    assert rc == capi.SK_ERANGE and counts["order"]["error_batch"] == 1 and counts["range"][0] == 2 * 15 + 1


# ---- 5 error paths and table sizing -----------------------------------------------------------------------------------------
def long_name_text(name_bytes):
    """record 17: a long name, one base and an empty '+' line, so that at name_bytes = batch_len - 2 the record is a
    batch of its own (any longer line behind such a name ends the reader's run)"""
    recs = [edge_record(k) for k in range(30)]
    recs[17] = b"@" + b"n" * (name_bytes - 1) + b"\nA\n\nI\n"
    return b"".join(recs)


LONG_PARAMS = ("sanger", 20, 1, False, False)


def test_long_line(sk_ctx):
    L = 200
    rc, counts, _ = check(sk_ctx, LONG_PARAMS, [long_name_text(L - 1)], "se", 4, L)
    assert rc == capi.SK_ELONGLINE and (counts["order"]["long_line_input"], counts["order"]["long_line"]) == (0, 4 * 17)
    rc, counts, got = check(sk_ctx, LONG_PARAMS, [long_name_text(L - 2)], "se", 4, L)
    assert rc == capi.SK_OK and b"@" + b"n" * (L - 3) + b"\n" in got[0]
    # in the second text of a pair, behind the first one's last record
    pair = [b"".join(edge_record(k) for k in range(8)), long_name_text(L - 1)]
    rc, counts, _ = check(sk_ctx, LONG_PARAMS, pair, "pe_split", 4, L)
    assert rc == capi.SK_ELONGLINE and (counts["order"]["long_line_input"], counts["order"]["long_line"]) == (1, 4 * 17)


def test_batch_table_one_too_small(sk_ctx, test_fastq):
    batch_len = fu.reference_batch_len(len(test_fastq))
    params = capi.make_params(*SE_PARAMS)
    rc, counts, keep, table = raw(sk_ctx, params, [test_fastq], "se", 5, batch_len, capacity=7)
    assert rc == capi.SK_ESPACE and counts["order"]["batches"] == 8 and counts["records"] == [0, 0, 0]
    assert counts["order"]["error_batch"] == om.NONE
    untouched(keep)
    want = om.expected(SE_PARAMS, [test_fastq], "se", 5, batch_len)
    assert table == want["tables"]["first_unit"][:8]
    rc, counts, keep, table = raw(sk_ctx, params, [test_fastq], "se", 5, batch_len, capacity=8)
    assert rc == capi.SK_OK and counts["order"]["batches"] == 8 and texts_of(keep, counts)[0] == want["texts"][0]


def test_python_grows_the_batch_table(sk_ctx):
    """400 records of 19 bytes at a budget of 20: the two lines carried into every batch use up so much of it that each
    batch is one record, more batches than bytes / batch_len + 16"""
    text = b"".join(b"@" + bytes([65 + k % 26]) + b"\nACGTAC\n+\nIIIIII\n" for k in range(400))
    ptuple = ("sanger", 20, 1, False, False)
    want = om.expected(ptuple, [text], "se", 3, 20)
    assert want["order"]["batches"] > len(text) // 20 + 16
    outs, counts = sk_ctx.trim_fastq(capi.make_params(*ptuple), to_dev(text), mode="se", order=(3, 20))
    assert counts["order"]["batches"] == want["order"]["batches"] and outs[0].cpu().numpy().tobytes() == want["texts"][0]


def test_batch_limit(sk_ctx, test_fastq):
    batch_len = fu.reference_batch_len(len(test_fastq))
    _, counts, got = check(sk_ctx, SE_PARAMS, [test_fastq], "se", 5, batch_len, limit=3)
    whole = om.expected(SE_PARAMS, [test_fastq], "se", 5, batch_len)
    first3 = whole["tables"]["first_unit"][3]
    assert counts["order"]["batches"] == 3 and counts["order"]["units"] == first3
    assert counts["order"]["records_unbatched"][0] == whole["records_in"][0] - first3
    assert whole["texts"][0].startswith(got[0]) and len(got[0]) < len(whole["texts"][0])


def test_bad_order_arguments(sk_ctx):
    L = capi.lib()
    text = edge_record(0)
    buf, ptr = upload(text)
    params = capi.make_params(*EDGE_PARAMS)
    inp = capi.FastqInput((C.c_void_p * 2)(ptr, None), (C.c_uint64 * 2)(len(text), 0), 0)
    outs = (capi.FastqOutput * 3)()
    nbytes = L.sk_trim_fastq_ordered_workspace_bytes(len(text), 0, 4)
    ws = torch_mod().empty(nbytes, dtype=torch_mod().uint8, device="cuda")
    call = lambda order, n=nbytes: L.sk_trim_fastq_ordered_device_async(sk_ctx._h, C.byref(params), C.byref(inp), capi.SK_TRIM_SE,
                                                                       order, outs, ws.data_ptr(), n, None)
    for bad in (capi.FastqOrder(0, 0, 20, 4, 0), capi.FastqOrder(1, 1, 20, 4, 0), capi.FastqOrder(1, 0, 19, 4, 0),
                capi.FastqOrder(1, 0, 20, 0, 0)):
        assert call(C.byref(bad)) == capi.SK_EINVAL
    assert call(None) == capi.SK_EINVAL
    assert call(C.byref(capi.FastqOrder(1, 0, 100, 4, 0)), nbytes - 1) == capi.SK_EINVAL
    assert call(C.byref(capi.FastqOrder(1, 0, 100, 4, 0))) == capi.SK_OK
    c, oc = capi.FastqCounts(), capi.FastqOrderCounts()
    assert L.sk_trim_fastq_ordered_device_finish(sk_ctx._h, ws.data_ptr(), None, C.byref(c), C.byref(oc)) == capi.SK_OK
    assert (oc.batches, oc.units, list(c.records)) == (1, 1, [1, 0, 0])


# ---- 6 alignment and the BGZF chain ------------------------------------------------------------------------------------
def test_shifted_text(sk_ctx, edge_texts):
    check(sk_ctx, EDGE_PARAMS, edge_texts["pe_split"], "pe_split", 7, 47 * 100, shift=9)
    check(sk_ctx, EDGE_PARAMS, edge_texts["se"], "se", 3, 47 * 333, shift=9)


def gunzip_members(image):
    out, data = [], bytes(image)
    while data:
        d = zlib.decompressobj(31)
        out.append(d.decompress(data))
        data = d.unused_data
    return b"".join(out)


def test_ordered_bgzf_chain(sk_ctx, edge_texts):
    texts = edge_texts["pe_interleaved"]
    want = om.expected(EDGE_PARAMS, texts, "pe_interleaved", 7, 94 * 100)
    images, counts = sk_ctx.trim_fastq_gz(capi.make_params(*EDGE_PARAMS), to_dev(texts[0]), mode="pe_interleaved",
                                          order=(7, 94 * 100))
    assert counts["order"]["batches"] == 25 and images[1] is None
    for o in (0, 2):
        assert gunzip_members(images[o].cpu().numpy().tobytes()) == want["texts"][o]


def test_ordered_from_gzip_images(sk_ctx):
    texts = [open(os.path.join(cu.INPUTS, n), "rb").read() for n in ("test.f.fastq", "test.r.fastq")]
    images = []
    for t in texts:
        z = zlib.compressobj(6, zlib.DEFLATED, 31)
        images.append(z.compress(t) + z.flush())
    ptuple = ("illumina", 20, 20, False, False)
    batch_len = fu.reference_batch_len(len(images[0]), paired=True)  # the reference sizes it by the compressed file
    want = om.expected(ptuple, texts, "pe_split", 4, batch_len)
    assert want["order"]["batches"] > 8
    out, counts = sk_ctx.trim_gz(capi.make_params(*ptuple), to_dev(images[0]), to_dev(images[1]), mode="pe_split",
                                 order=(4, batch_len))
    assert counts["order"]["batches"] == want["order"]["batches"]
    for o in range(3):
        assert gunzip_members(out[o].cpu().numpy().tobytes()) == want["texts"][o]


# ---- 7 randomized -----------------------------------------------------------------------------------------------------------
def test_randomized(sk_ctx):
    rng = random.Random(4711)  # the cases tests/test_fastq_order_host.py holds to the model
    for it in range(100):
        ptuple, texts, mode, threads, batch_len = om.random_case(rng)
        rc, counts, got = check(sk_ctx, ptuple, texts, mode, threads, batch_len)
        assert rc == capi.SK_OK and got is not None, it
