"""GPU: trimming on the device (sk_trim_device_async / sk_trim_device_finish, Context.trim_reads_device) against the
numpy model of tests/trim_model.py on the oracle's cuts, and against the reference's recorded output files."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import cli_util as cu
import oracle_bind as ob
import trim_model as tm
from sickle_amd import capi, synth
from trim_raw import Raw, dev, host, raw_call, torch_mod

pytestmark = pytest.mark.gpu


def check_outputs(got, want, mode):
    for o in range(3):
        if want[o] is None:
            assert got[o] is None
            continue
        q, s, off, idx = (host(x) for x in got[o])
        w = want[o]
        assert np.array_equal(off.astype(np.int64), w["offsets"]), "offsets of output %d" % o
        assert np.array_equal(idx, w["read_index"]), "read_index of output %d" % o
        assert np.array_equal(q, w["qual"]), "qual bytes of output %d" % o
        if w["seq"] is None:
            assert s is None
        else:
            assert np.array_equal(s, w["seq"]), "seq bytes of output %d" % o


def trim(ctx, qual, seq, cuts, mode, offsets=None, stride=0, read_len=0, lengths=None):
    return ctx.trim_reads_device(None, dev(qual), dev(seq), offsets=dev(offsets), stride=stride, read_len=read_len,
                                 lengths=dev(lengths), mode=mode, cuts=dev(np.ascontiguousarray(cuts, dtype=np.int32)))


# ---- 1 the reference runs ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_gpu")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


@pytest.mark.parametrize("name,rec", tm.golden_params())
def test_reference_runs_through_device_trim(sk_ctx, workdir, name, rec):
    """Scan and trim on the device, the output files rebuilt from the input's name and '+' lines by read_index: the
    recorded md5 and size of every output of the reference's -a 1 run."""
    argv = rec["argv"]
    mode, recs, files = tm.run_batch(argv, workdir)
    qual, seq, offsets = tm.pack(recs)
    params = capi.make_params(*tm.run_params(argv))
    got = sk_ctx.trim_reads_device(params, dev(qual), dev(seq), offsets=dev(offsets), mode=mode)
    as_dicts = [None if g is None else dict(zip(("qual", "seq", "offsets", "read_index"), (host(x) for x in g)))
                for g in got]
    for fname, want in rec["outputs"].items():
        text = tm.fastq_text(recs, as_dicts[files[fname]])
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname
    if name.startswith("se_equiv_selfpair"):  # o1 of a self-paired run == SK_TRIM_SE over file 1
        recs1 = recs[0::2]
        q1, s1, off1 = tm.pack(recs1)
        got = sk_ctx.trim_reads_device(params, dev(q1), dev(s1), offsets=dev(off1), mode="se")
        d = dict(zip(("qual", "seq", "offsets", "read_index"), (host(x) for x in got[0])))
        text = tm.fastq_text(recs1, d)
        want = rec["outputs"]["o1.fastq"]
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"])


# ---- 2 layouts x parameters against numpy --------------------------------------------------------------------------
def _layouts():
    """name -> (qual, seq, starts, layout kwargs, lens); all with an even number of reads."""
    L = {}
    s, q = synth.make_reads(11, 3000, 150, "sanger", lower_n_frac=0.01)
    L["stride152"] = (synth.pack_fixed(q, 152), synth.pack_fixed(s, 152), np.arange(3000) * 152,
                      dict(stride=152, read_len=150), np.full(3000, 150))
    L["packed150"] = (q.reshape(-1), s.reshape(-1), np.arange(3000) * 150, dict(stride=150, read_len=150),
                      np.full(3000, 150))
    lens = np.random.default_rng(12).integers(0, 151, 3000).astype(np.uint32)
    L["stride152_lengths"] = (synth.pack_fixed(q, 152), synth.pack_fixed(s, 152), np.arange(3000) * 152,
                              dict(stride=152, lengths=lens), lens)
    s, q, off = synth.make_ragged_reads(13, 4000, 1, 2500, "sanger")
    L["ragged1_2500"] = (q, s, off[:-1].astype(np.int64), dict(offsets=off), np.diff(off.astype(np.int64)))
    s, q, off = synth.make_long_reads(14, 40, 1, 100_000)
    L["ragged1_100k"] = (q, s, off[:-1].astype(np.int64), dict(offsets=off), np.diff(off.astype(np.int64)))
    # reads of length 0 between others, and an odd total byte count
    lens = np.random.default_rng(15).integers(0, 40, 1002)
    lens[::7] = 0
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    rng = np.random.default_rng(16)
    q = rng.integers(33, 75, int(off[-1])).astype(np.uint8)
    s = rng.choice(np.frombuffer(b"ACGTNn", dtype=np.uint8), int(off[-1]))
    L["ragged_zero_len"] = (q, s, off[:-1].astype(np.int64), dict(offsets=off), lens)
    return L


LAYOUTS = _layouts()
PARAMS = [("sanger", 20, 20, False, False), ("sanger", 20, 20, True, True), ("sanger", 30, 0, False, False),
          ("sanger", 0, 0, False, False)]


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("pi", range(len(PARAMS)))
def test_layouts_and_parameters_against_numpy(sk_ctx, layout, pi):
    qual, seq, starts, kw, lens = LAYOUTS[layout]
    p = PARAMS[pi]
    n = len(starts)
    ok = ob.oracle_trim_batch(ob.make_params(*p), qual, seq, n_reads=n, **kw)
    cuts, err = ok
    assert err is None
    for mode in tm.MODES:
        for with_seq in (True, False):
            s = seq if with_seq else None
            want = tm.expected(qual, s, starts, cuts, mode)
            got = trim(sk_ctx, qual, s, cuts, mode, **kw)
            check_outputs(got, want, mode)


def test_hand_cuts_empty_records_all_and_none(sk_ctx):
    """Valid hand-made cuts: records of length 0 (five == three), every read discarded, none discarded."""
    qual, seq, starts, kw, lens = LAYOUTS["ragged1_2500"]
    rng = np.random.default_rng(21)
    n = len(starts)
    a = rng.integers(0, lens + 1)
    b = rng.integers(0, lens + 1)
    cuts = np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1).astype(np.int32)
    cuts[rng.random(n) < 0.2] = (-1, -1)
    cuts[::5, 1] = cuts[::5, 0]  # empty kept records
    variants = {"mixed": cuts, "all_discarded": np.full((n, 2), -1, np.int32),
                "none_discarded": np.stack([np.zeros(n), lens], axis=1).astype(np.int32)}
    for name, c in variants.items():
        for mode in tm.MODES:
            check_outputs(trim(sk_ctx, qual, seq, c, mode, **kw), tm.expected(qual, seq, starts, c, mode), mode)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_batches(sk_ctx, n):
    s, q = synth.make_reads(31, max(n, 1), 150, "sanger")
    cuts = np.array([[3, 77], [0, 150]][:n], dtype=np.int32).reshape(n, 2)
    qual, seq = q.reshape(-1)[:n * 150], s.reshape(-1)[:n * 150]
    for mode in tm.MODES:
        if mode != "se" and n % 2:
            continue
        got = trim(sk_ctx, qual, seq, cuts, mode, stride=150, read_len=150)
        check_outputs(got, tm.expected(qual, seq, np.arange(n) * 150, cuts, mode), mode)


# ---- 3 at size ---------------------------------------------------------------------------------------------------
def _fixed_expected(q2d, s2d, cuts, mode, first_read):
    """tm.expected for reads of one length in rows: a boolean mask over the rows instead of an index per byte."""
    d = tm.dests(cuts, mode)
    col = np.arange(q2d.shape[1])[None, :]
    res = [None, None, None]
    for o in {"se": (0,), "pe_split": (0, 1, 2)}[mode]:
        idx = np.nonzero(d == o)[0]
        five, three = cuts[idx, 0][:, None], cuts[idx, 1][:, None]
        m = (col >= five) & (col < three)
        offsets = np.zeros(len(idx) + 1, dtype=np.int64)
        np.cumsum(three[:, 0] - five[:, 0], out=offsets[1:])
        res[o] = dict(qual=q2d[idx][m], seq=s2d[idx][m], offsets=offsets, read_index=idx.astype(np.int64) + first_read)
    return res


def test_at_size_se_and_pe_split(sk_ctx):
    """10 M x 150 bp with seq through SK_TRIM_SE, and the same batch as 5 M pairs in SK_TRIM_PE_SPLIT; numpy in chunks."""
    torch = torch_mod()
    n, L = 10_000_000, 150
    rng = np.random.default_rng(41)
    qtab = np.where(np.arange(256) < 200, 60 + np.arange(256) % 15, 33 + np.arange(256) % 20).astype(np.uint8)
    stab = np.frombuffer((b"ACGT" * 64)[:252] + b"NNNN", dtype=np.uint8)
    qual = qtab[rng.integers(0, 256, n * L, dtype=np.uint8)]
    seq = stab[rng.integers(0, 256, n * L, dtype=np.uint8)]
    cuts, err = ob.oracle_trim_batch(ob.make_params("sanger", 20, 50, False, True), qual, seq, stride=L, read_len=L,
                                     n_reads=n, threads=16)
    assert err is None
    q2d, s2d = qual.reshape(n, L), seq.reshape(n, L)
    dq, ds, dc = dev(qual), dev(seq), dev(cuts)
    for mode in ("se", "pe_split"):
        got = sk_ctx.trim_reads_device(None, dq, ds, stride=L, read_len=L, mode=mode, cuts=dc)
        got = [None if g is None else [host(x) for x in g] for g in got]
        base_r, base_b = [0, 0, 0], [0, 0, 0]
        step = 500_000
        for a in range(0, n, step):
            b = min(n, a + step)
            want = _fixed_expected(q2d[a:b], s2d[a:b], cuts[a:b], mode, a)
            for o in range(3):
                if want[o] is None:
                    continue
                q, s, off, idx = got[o]
                R, B = len(want[o]["read_index"]), int(want[o]["offsets"][-1])
                r0, b0 = base_r[o], base_b[o]
                assert np.array_equal(off[r0:r0 + R + 1] - b0, want[o]["offsets"])
                assert np.array_equal(idx[r0:r0 + R], want[o]["read_index"])
                assert np.array_equal(q[b0:b0 + B], want[o]["qual"])
                assert np.array_equal(s[b0:b0 + B], want[o]["seq"])
                base_r[o] += R
                base_b[o] += B
        for o in range(3):
            if got[o] is not None:
                assert len(got[o][3]) == base_r[o] and len(got[o][0]) == base_b[o]
                assert 0 < base_r[o] < n
    del dq, ds, dc
    torch.cuda.empty_cache()


def test_offsets_beyond_4_gib(sk_ctx):
    """An `offsets` batch of 45 000 reads of 100 kb, 4.5e9 bytes of qual built on the device from one tile of 500 reads, no
    seq, hand-made cuts that keep most of every read (2 % of the reads dropped), SK_TRIM_SE: input and output offsets
    beyond 2^32.  Compared tile by tile, so the host never holds an index per byte of the batch."""
    torch = torch_mod()
    L, tile, reps = 100_000, 500, 90
    n = tile * reps
    rng = np.random.default_rng(51)
    base = rng.integers(33, 75, tile * L, dtype=np.uint8)
    dq = dev(base).repeat(reps)
    assert dq.numel() > 1 << 32
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(L)
    cuts = np.stack([rng.integers(0, 500, n), L - rng.integers(0, 500, n)], axis=1).astype(np.int32)
    cuts[rng.random(n) < 0.02] = (-1, -1)
    got = sk_ctx.trim_reads_device(None, dq, None, offsets=dev(off), mode="se", cuts=dev(cuts))
    assert got[1] is None and got[2] is None
    q, s, o, idx = got[0]
    assert s is None
    o_h, idx_h = host(o), host(idx)
    q2d = base.reshape(tile, L)
    r0 = b0 = 0
    for t in range(reps):
        want = _fixed_expected(q2d, q2d, cuts[t * tile:(t + 1) * tile], "se", t * tile)[0]
        R, B = len(want["read_index"]), int(want["offsets"][-1])
        assert np.array_equal(o_h[r0:r0 + R + 1] - b0, want["offsets"]), t
        assert np.array_equal(idx_h[r0:r0 + R], want["read_index"]), t
        assert np.array_equal(host(q[b0:b0 + B]), want["qual"]), t
        r0 += R
        b0 += B
    assert r0 == len(idx_h) and b0 == q.numel() and b0 > 1 << 32 and 0 < r0 < n
    del dq, q, o, idx, got
    torch.cuda.empty_cache()


# ---- 4 capacity, 5 bad cuts: the raw C ABI ------------------------------------------------------------------------
def test_capacity_one_short_and_count_only(sk_ctx):
    qual, seq, starts, kw, lens = LAYOUTS["ragged1_2500"]
    off = kw["offsets"]
    n = len(starts)
    cuts, _ = ob.oracle_trim_batch(ob.make_params("sanger", 20, 20, False, False), qual, seq, offsets=off)
    want = tm.expected(qual, seq, starts, cuts, "pe_split")
    need = tm.counts_of(want)
    dq, ds, doff, dc = dev(qual), dev(seq), dev(off), dev(cuts)
    # count only: every offsets NULL
    counts = raw_call(sk_ctx, dq, ds, doff, dc, n, [capi.TrimOutput() for _ in range(3)], "pe_split")
    assert {k: counts[k] for k in ("records", "bytes")} == need and counts["bad_read"] == 2**64 - 1
    # exact capacities: OK and the same counts
    r = Raw(need["records"], need["bytes"])
    assert raw_call(sk_ctx, dq, ds, doff, dc, n, r.outs, "pe_split") == counts
    # one byte short in output 0, one record short in output 2: SK_ESPACE, those two untouched, output 1 written
    for o, short in ((0, "bytes"), (2, "records")):
        recs, nbytes = list(need["records"]), list(need["bytes"])
        (nbytes if short == "bytes" else recs)[o] -= 1
        r = Raw(recs, nbytes)
        with pytest.raises(capi.TrimError) as e:
            raw_call(sk_ctx, dq, ds, doff, dc, n, r.outs, "pe_split")
        assert e.value.rc == capi.SK_ESPACE
        assert {k: e.value.counts[k] for k in ("records", "bytes")} == need
        assert r.untouched(o)
        for p in range(3):
            if p != o:
                assert not r.untouched(p)


def test_bad_cuts_einval_lowest_read(sk_ctx):
    qual, seq, starts, kw, lens = LAYOUTS["ragged1_2500"]
    off = kw["offsets"]
    n = len(starts)
    cuts, _ = ob.oracle_trim_batch(ob.make_params("sanger", 20, 20, False, False), qual, seq, offsets=off)
    need = tm.counts_of(tm.expected(qual, seq, starts, cuts, "se"))
    for kind in ("five_neg", "five_gt_three", "three_gt_len"):
        c = cuts.copy()
        for r in (3001, 2100, 3999):  # the lowest is 2100, in another count block than 3001 (2048 reads a block)
            if kind == "five_neg":
                c[r] = (-3, 4)
            elif kind == "five_gt_three":
                c[r] = (5, 4)
            else:
                c[r] = (0, lens[r] + 1)
        r = Raw(need["records"], [b + 64 for b in need["bytes"]])
        with pytest.raises(capi.TrimError) as e:
            raw_call(sk_ctx, dev(qual), dev(seq), dev(off), dev(c), n, r.outs, "se")
        assert e.value.rc == capi.SK_EINVAL and e.value.counts["bad_read"] == 2100, kind
        assert r.untouched(0)


def test_argument_checks_with_device(sk_ctx):
    torch = torch_mod()
    q = torch.zeros(64, dtype=torch.uint8, device="cuda")
    c = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    off = torch.tensor([0, 4, 8, 12, 16], dtype=torch.int64, device="cuda")
    ws = torch.empty(4096, dtype=torch.uint8, device="cuda")
    L = capi.lib()

    def call(n=4, tiles=None, mode=capi.SK_TRIM_SE, outs=(), ws_bytes=4096):
        b = capi.Batch(q.data_ptr(), None, off.data_ptr(), 0, 0, None, n, tiles, 1 if tiles else 0)
        arr = (capi.TrimOutput * 3)(*outs)
        return L.sk_trim_device_async(sk_ctx._h, C.byref(b), c.data_ptr(), mode, arr, ws.data_ptr(), ws_bytes, None)

    assert call(tiles=0x4000) == capi.SK_EINVAL and b"segmented" in L.sk_last_error(sk_ctx._h)
    assert call(n=3, mode=capi.SK_TRIM_PE_SPLIT) == capi.SK_EINVAL and b"even" in L.sk_last_error(sk_ctx._h)
    out = capi.TrimOutput(q.data_ptr() + 1, None, off.data_ptr(), None, 16, 4)
    assert call(outs=[out]) == capi.SK_EINVAL and b"16-byte" in L.sk_last_error(sk_ctx._h)
    out = capi.TrimOutput(q.data_ptr(), q.data_ptr(), off.data_ptr(), None, 16, 4)
    assert call(outs=[out]) == capi.SK_EINVAL and b"batch->seq" in L.sk_last_error(sk_ctx._h)
    assert call(ws_bytes=100) == capi.SK_EINVAL and b"workspace" in L.sk_last_error(sk_ctx._h)


# ---- 6 reuse -----------------------------------------------------------------------------------------------------
def test_one_workspace_three_times_and_two_streams(sk_ctx):
    torch = torch_mod()
    qual, seq, starts, kw, lens = LAYOUTS["ragged1_2500"]
    off = kw["offsets"]
    n = len(starts)
    cuts, _ = ob.oracle_trim_batch(ob.make_params("sanger", 20, 20, False, False), qual, seq, offsets=off)
    dq, ds, doff, dc = dev(qual), dev(seq), dev(off), dev(cuts)
    nb = capi.lib().sk_trim_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    for mode in ("pe_interleaved", "se", "pe_split"):  # one workspace, back to back on one stream
        want = tm.expected(qual, seq, starts, cuts, mode)
        need = tm.counts_of(want)
        r = Raw(need["records"], need["bytes"])
        counts = raw_call(sk_ctx, dq, ds, doff, dc, n, r.outs, mode, ws=ws)
        assert {k: counts[k] for k in ("records", "bytes")} == need
        for o in range(3):
            if want[o] is None:
                continue
            q, s, o_, idx = r.t[o]
            R, B = need["records"][o], need["bytes"][o]
            assert np.array_equal(host(q[:B]), want[o]["qual"]) and np.array_equal(host(s[:B]), want[o]["seq"])
            assert np.array_equal(host(o_[:R + 1]), want[o]["offsets"]) and np.array_equal(host(idx[:R]), want[o]["read_index"])
    # two workspaces on two streams in flight at once
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    modes = ["se", "pe_split"]
    wss = [torch.empty(nb, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    raws, wants = [], []
    for st, w, mode in zip(streams, wss, modes):
        want = tm.expected(qual, seq, starts, cuts, mode)
        need = tm.counts_of(want)
        r = Raw(need["records"], need["bytes"])
        torch.cuda.synchronize()
        sk_ctx.trim_device_async(dc.data_ptr(), n, r.outs, w.data_ptr(), nb, mode=mode, qual_ptr=dq.data_ptr(),
                                 seq_ptr=ds.data_ptr(), offsets_ptr=doff.data_ptr(), stream=st.cuda_stream)
        raws.append(r)
        wants.append((want, need))
    for st, w, r, (want, need) in zip(streams, wss, raws, wants):
        counts = sk_ctx.trim_device_finish(w.data_ptr(), st.cuda_stream)
        assert {k: counts[k] for k in ("records", "bytes")} == need
        for o in range(3):
            if want[o] is not None:
                B = need["bytes"][o]
                assert np.array_equal(host(r.t[o][0][:B]), want[o]["qual"])
                assert np.array_equal(host(r.t[o][2][:need["records"][o] + 1]), want[o]["offsets"])


def test_trim_output_is_a_valid_offsets_batch(sk_ctx):
    """The packed output of a trim, fed straight back into sk_scan_device_async as an `offsets` batch: the oracle's
    cuts of those trimmed reads."""
    torch = torch_mod()
    qual, seq, starts, kw, lens = LAYOUTS["ragged1_2500"]
    p = ("sanger", 20, 20, False, True)
    got = sk_ctx.trim_reads_device(capi.make_params(*p), dev(qual), dev(seq), offsets=dev(kw["offsets"]), mode="se")
    q, s, off, idx = got[0]
    R = idx.numel()
    assert R > 0
    p2 = ("sanger", 30, 10, False, True)  # a second, stricter pass
    out = torch.empty((R, 2), dtype=torch.int32, device="cuda")
    sk_ctx.scan_device_async(capi.make_params(*p2), q.data_ptr(), out.data_ptr(), R, seq_ptr=s.data_ptr(),
                             offsets_ptr=off.data_ptr())
    sk_ctx.scan_device_finish()
    want, err = ob.oracle_trim_batch(ob.make_params(*p2), host(q), host(s), offsets=host(off).astype(np.uint64))
    assert err is None
    assert np.array_equal(host(out), want)


# ---- 7 block boundaries and tiny outputs -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
@pytest.mark.parametrize("total", [1, 15, 16, 17, 47])
def test_only_the_last_read_or_pair_kept(sk_ctx, n, total):
    """Reads are counted in blocks of 2 048: n reads (SK_TRIM_SE) or n pairs (the PE modes) of which only the last one is
    kept, `total` bytes of it -- a count block whose only kept record is its last, an output smaller than one 16-byte
    granule, one granule, and a few."""
    rng = np.random.default_rng(n * 100 + total)
    for mode in tm.MODES:
        reads = n if mode == "se" else 2 * n
        lens = rng.integers(47, 120, reads)
        off = np.zeros(reads + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        qual = rng.integers(33, 75, int(off[-1])).astype(np.uint8)
        seq = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), int(off[-1]))
        cuts = np.full((reads, 2), -1, np.int32)
        for r in range(reads - (1 if mode == "se" else 2), reads):
            five = int(rng.integers(0, lens[r] - total + 1))
            cuts[r] = (five, five + total)
        want = tm.expected(qual, seq, off[:-1].astype(np.int64), cuts, mode)
        assert tm.counts_of(want)["bytes"][0] == (total if mode != "pe_interleaved" else 2 * total)
        check_outputs(trim(sk_ctx, qual, seq, cuts, mode, offsets=off), want, mode)


TRIM_SOAK = (100, 290)  # iterations, comparisons


def test_trim_soak(sk_ctx):
    """tests/soak_trim.py: random batches, layouts, alignments, cuts, modes and capacities through the raw C ABI against
    tests/trim_model.py (the same draws without a device give the same number of comparisons: soak_trim.py --dry)."""
    import soak_trim
    assert soak_trim.run(TRIM_SOAK[0], 2028, verbose=False) == TRIM_SOAK[1]
