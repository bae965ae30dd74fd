"""GPU: FASTQ text on the device (sk_trim_fastq_device_async / finish, Context.trim_fastq) against the reference's recorded
output files and against the numpy model of tests/fastq_model.py on the oracle's cuts."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import cli_util as cu
import fastq_model as fm
import trim_model as tm
from sickle_amd import capi, synth
from fastq_raw import SENTINEL, check, raw, texts_of, torch_mod, untouched, upload
from test_fastq_api import golden_texts

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- 1 the reference runs ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_gpu")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


@pytest.mark.parametrize("name,rec", tm.golden_params())
def test_reference_runs_from_fastq_text(sk_ctx, workdir, name, rec):
    """The input files uploaded byte for byte, trimmed on the device: the recorded md5 and size of every output."""
    mode, texts, files = golden_texts(rec["argv"], workdir)
    tt = [torch_mod().from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in texts]
    outs, counts = sk_ctx.trim_fastq(capi.make_params(*tm.run_params(rec["argv"])), tt[0], tt[1] if len(tt) > 1 else None,
                                     mode=mode)
    for fname, want in rec["outputs"].items():
        text = outs[files[fname]].cpu().numpy().tobytes()
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname


def test_se_equals_selfpair_mate1(sk_ctx, workdir):
    """SE over test.fastq writes what `sickle pe -f X -r copy-of-X` writes to file 1."""
    runs = [(n, r) for n, r in tm.golden_runs() if n.startswith("se_equiv_selfpair")]
    assert runs
    for name, rec in runs:
        argv = rec["argv"]
        text = open(tm._plain(argv[argv.index("-f") + 1], workdir), "rb").read()
        t = torch_mod().from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
        outs, _ = sk_ctx.trim_fastq(capi.make_params(*tm.run_params(argv)), t, mode="se")
        got = outs[0].cpu().numpy().tobytes()
        want = rec["outputs"]["o1.fastq"]
        assert (hashlib.md5(got).hexdigest(), len(got)) == (want["md5"], want["size"]), name


# ---- 2 range errors ----------------------------------------------------------------------------------------------
def good_record(ptuple, k, L=12):
    lo, hi = {"phred": (4, 60), "sanger": (33, 126), "solexa": (58, 112), "illumina": (64, 110)}[ptuple[0]]
    return b"@good%d\n%s\n+\n%s\n" % (k, b"ACGT" * (L // 4), bytes([(lo + hi) // 2]) * L)


def test_range_errors_of_reference_cases(sk_ctx):
    cases = json.load(open(os.path.join(GOLDEN, "errors.json")))
    assert len(cases) == 57
    for case in cases:
        p = case["params"]
        ptuple = (p["qualtype"], p["q"], p["l"], p["no5"], p["trunc_n"])
        rec = (case["name"].encode() + b"\n" + case["seq"].encode() + b"\n+\n" + bytes.fromhex(case["qual_hex"]) + b"\n")
        n = 9
        for k in (0, n // 2, n - 1):
            text = b"".join(good_record(ptuple, j) for j in range(k)) + rec + \
                b"".join(good_record(ptuple, j) for j in range(k + 1, n))
            rc, counts, _ = check(sk_ctx, ptuple, [text], "se")
            if case["rc"]:
                assert rc == capi.SK_ERANGE, case["desc"]
                read, pos, ch = counts["range"]
                assert read == k
                assert "Quality value (%d)" % (ch if ch >= 0 else ch + 256) in case["stderr"] or \
                    "Quality value (%d)" % ch in case["stderr"], case["desc"]
                assert "Quality position: %d\n" % (pos + 1) in case["stderr"], case["desc"]
            else:
                assert rc == capi.SK_OK, case["desc"]


# ---- 3 format errors ---------------------------------------------------------------------------------------------
BAD = {capi.SK_FQ_ID_SHORT: b"@\nACGT\n+\nIIII\n", capi.SK_FQ_ID_NO_AT: b"Xbad\nACGT\n+\nIIII\n",
       capi.SK_FQ_SEQ_EMPTY: b"@bad\n\n+\nIIII\n", capi.SK_FQ_QUAL_EMPTY: b"@bad\nACGT\n+\n\n",
       capi.SK_FQ_LENGTHS: b"@bad\nACGT\n+\nIII\n"}


# a quality char below Sanger's range at the end of a read the scan reads to its end (it is longer than -l 20)
RANGE_BAD = b"@range\n" + b"ACGT" * 6 + b"\n+\n" + b"I" * 23 + b" \n"


def many_good(n, L=150, seed=0):
    rng = np.random.default_rng(seed)
    q = rng.integers(35, 75, size=(n, L), dtype=np.uint8).tobytes()
    return [b"@r%d\n%s\n+\n%s\n" % (k, b"ACGT" * (L // 4) + b"AC"[:L % 4], q[k * L:(k + 1) * L]) for k in range(n)]


def test_format_errors_first_straddling_last(sk_ctx):
    pt = ("sanger", 20, 20, False, False)
    good = many_good(600)
    # the record that straddles the first 64 KiB framing chunk boundary
    at, k_mid = 0, 0
    while at + len(good[k_mid]) <= 65536 - 3:
        at += len(good[k_mid])
        k_mid += 1
    for why, bad in BAD.items():
        for k in (0, k_mid, len(good)):
            recs = good[:k] + [bad] + good[k:]
            _, counts, _ = check(sk_ctx, pt, [b"".join(recs)], "se")
            assert counts["format_error"] == why and counts["format_record"] == k
    # too long: a qual line beyond SK_MAX_READ_LEN
    L = (1 << 24) + 1
    bad = b"@long\n" + b"A" * L + b"\n+\n" + b"I" * L + b"\n"
    _, counts, _ = check(sk_ctx, pt, [b"".join(good[:3]) + bad + b"".join(good[3:6])], "se")
    assert counts["format_error"] == capi.SK_FQ_TOO_LONG and counts["format_record"] == 3


def test_format_error_precedence_and_pairs(sk_ctx):
    pt = ("sanger", 20, 20, False, False)
    good = many_good(40)
    two = good[:5] + [BAD[capi.SK_FQ_LENGTHS]] + good[5:20] + [BAD[capi.SK_FQ_ID_SHORT]] + good[20:]
    _, c, _ = check(sk_ctx, pt, [b"".join(two)], "se")
    assert (c["format_error"], c["format_record"]) == (capi.SK_FQ_LENGTHS, 5)
    # a malformed record after a range error: the format error wins
    _, c, _ = check(sk_ctx, pt, [b"".join(good[:3] + [RANGE_BAD] + good[3:30] + [BAD[capi.SK_FQ_SEQ_EMPTY]])], "se")
    assert c["format_error"] == capi.SK_FQ_SEQ_EMPTY and c["format_record"] == 31
    # split inputs with different record counts, either way round
    for a, b in ((31, 30), (30, 31)):
        _, c, _ = check(sk_ctx, pt, [b"".join(good[:a]), b"".join(good[:b])], "pe_split")
        assert c["format_error"] == capi.SK_FQ_PAIR_COUNT


# ---- 4 edge cases ------------------------------------------------------------------------------------------------
def test_edges_small_texts(sk_ctx):
    pt = ("sanger", 20, 20, False, False)
    good = many_good(7, L=60)
    one = good[0]
    for text in (b"", one, one[:-1], b"".join(good)[:-1]):
        check(sk_ctx, pt, [text], "se")
    for tail in (b"@t\n", b"@t\nAC\n", b"@t\nAC\n+\n"):  # 1-3 tail lines
        _, c, _ = check(sk_ctx, pt, [b"".join(good) + tail], "se")
        assert c["tail_lines"][0] == tail.count(b"\n")
    _, c, _ = check(sk_ctx, pt, [b"".join(good)], "pe_interleaved")
    assert c["dropped_unpaired"] == 1
    # CRLF: the '\r' belongs to its line; in a quality line the scan reads to the end it is a range error, as in the CLI
    check(sk_ctx, pt, [b"".join(good).replace(b"\n", b"\r\n")], "se")
    rc, c, _ = check(sk_ctx, pt, [b"".join(good[:3]) + b"@c\r\n" + b"ACGT" * 6 + b"\r\n+\r\n" + b"I" * 24 + b"\r\n"], "se")
    assert rc == capi.SK_ERANGE and c["range"] == (3, 24, 13)


def test_edges_alignment_names_and_tiny_records(sk_ctx):
    rng = np.random.default_rng(5)
    recs = []
    for k in range(3000):
        L = int(rng.integers(1, 21))
        name = b"@" + bytes(rng.integers(97, 123, size=int(rng.integers(1, 301)), dtype=np.uint8))
        plus = b"+" + bytes(rng.integers(97, 123, size=int(rng.integers(0, 300)), dtype=np.uint8))
        seq = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=L))
        qual = bytes(rng.integers(33, 75, size=L, dtype=np.uint8))
        recs.append(name + b"\n" + seq + b"\n" + plus + b"\n" + qual + b"\n")
    text = b"".join(recs)
    for shift in range(16):
        check(sk_ctx, ("sanger", 20, 0 if shift % 2 else 5, shift % 4 == 1, shift % 3 == 0), [text], "se", shift=shift)
    # tiny records only (names of 2 bytes, empty '+' lines), -l 0 with and without -x
    tiny = b"".join(b"@%c\n%s\n+\n%s\n" % (97 + k % 26, b"A" * (1 + k % 20), bytes([35 + (k * 7) % 40]) * (1 + k % 20))
                    for k in range(5000))
    for no5 in (False, True):
        for mode in ("se", "pe_interleaved"):
            check(sk_ctx, ("sanger", 30, 0, no5, False), [tiny], mode, shift=3)


def test_edges_mixed_lengths_and_hint(sk_ctx):
    rng = np.random.default_rng(11)
    lens = np.concatenate([rng.integers(1, 300, size=3000), rng.integers(2000, 20001, size=60)])
    rng.shuffle(lens)
    q = [bytes(rng.integers(33, 75, size=int(L), dtype=np.uint8)) for L in lens]
    text = b"".join(b"@m%d\n%s\n+\n%s\n" % (k, b"C" * len(x), x) for k, x in enumerate(q))
    pt = ("sanger", 20, 20, False, True)
    _, _, a = check(sk_ctx, pt, [text], "se", max_read_len=0)
    _, _, b = check(sk_ctx, pt, [text], "se", max_read_len=int(lens.max()))
    assert a == b


# ---- 5 at size ---------------------------------------------------------------------------------------------------
def synth_text(n, L, seed, lmax=None, lower_n=0.0, chunk=500_000):
    """n FASTQ records ("@r" + 9 digits, seq, "+", qual) of synth's reads, of length L or uniform in [L, lmax]."""
    rng = np.random.default_rng(seed)
    W = lmax or L
    parts = []
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        seq, qual = synth.make_reads(seed * 1000 + a // chunk, m, W, "sanger", lower_n_frac=lower_n)
        lens = rng.integers(L, W + 1, size=m) if lmax else np.full(m, L)
        k = np.arange(a, a + m)
        name = np.empty((m, 12), np.uint8)
        name[:, 0], name[:, 1], name[:, 11] = ord("@"), ord("r"), 10
        for p in range(9):
            name[:, 10 - p] = 48 + (k // 10 ** p) % 10
        nl = np.full((m, 1), 10, np.uint8)
        rows = np.concatenate([name, seq.reshape(m, W), nl, np.tile(np.frombuffer(b"+\n", np.uint8), (m, 1)),
                               qual.reshape(m, W), nl], 1)
        col = np.arange(rows.shape[1])[None, :]
        keep = ~(((col >= 12) & (col < 12 + W) & (col >= 12 + lens[:, None])) |
                 ((col >= 15 + W) & (col < 15 + 2 * W) & (col >= 15 + W + lens[:, None])))
        parts.append(rows[keep])
    return np.concatenate(parts).tobytes()


@pytest.mark.parametrize("kind", ["se_10M_150", "split_5M_150_n", "inter_4M_mixed"])
def test_at_size(sk_ctx, kind):
    if kind == "se_10M_150":
        check(sk_ctx, ("sanger", 20, 20, False, False), [synth_text(10_000_000, 150, 1)], "se", index=False)
    elif kind == "split_5M_150_n":
        t1, t2 = synth_text(5_000_000, 150, 2, lower_n=0.01), synth_text(5_000_000, 150, 3, lower_n=0.01)
        check(sk_ctx, ("sanger", 20, 20, False, True), [t1, t2], "pe_split", index=False)
    else:
        check(sk_ctx, ("sanger", 20, 20, False, False), [synth_text(4_000_000, 75, 4, lmax=301)], "pe_interleaved",
              index=False)


def _tile_10kb(seed, n=3000, L=10_000):
    """n records of L bases whose quality stays above -q 20, one read in ten with a bad tail from a drawn position on (so it
    is cut there) and one in fifty bad throughout (dropped): most of the text is kept."""
    rng = np.random.default_rng(seed)
    qual = rng.integers(55, 75, (n, L), dtype=np.uint8)
    tail = np.where(rng.random(n) < 0.1, rng.integers(100, L, n), L)
    tail[rng.random(n) < 0.02] = 0
    qual[np.arange(L)[None, :] >= tail[:, None]] = 35
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, L))]
    name = np.empty((n, 12), np.uint8)
    name[:, 0], name[:, 1], name[:, 11] = ord("@"), ord("t"), 10
    for p in range(9):
        name[:, 10 - p] = 48 + (np.arange(n) * 7 + seed) // 10 ** p % 10
    nl = np.full((n, 1), 10, np.uint8)
    return np.concatenate([name, seq, nl, np.tile(np.frombuffer(b"+\n", np.uint8), (n, 1)), qual, nl], 1).tobytes()


def test_text_beyond_4_gib(sk_ctx):
    """A text of more than 2^32 bytes of 10 kb reads, SK_TRIM_SE, built on the device from three different tiles of 3 000
    records in a fixed pattern.  Records are independent and stay in order, so the model's output is the tiles' outputs in
    that pattern: its MD5 is computed tile by tile (a slice of records each) and compared with the MD5 of the device's
    output read back in pieces, plus the counts.  Text, framing tables and output offsets all pass 2^32."""
    torch = torch_mod()
    pt = ("sanger", 20, 20, False, False)
    tiles = [_tile_10kb(60 + k) for k in range(3)]
    wants = [fm.expected(pt, [t], "se") for t in tiles]
    assert all(w["verdict"] is None and w["range"] is None and 2500 < len(w["index"][0]) < 3000 for w in wants)
    reps = (1 << 32) // min(len(w["texts"][0]) for w in wants) + 2  # the output, too, passes 2^32 bytes
    pattern = [(7 * k) % 3 for k in range(reps)]
    dt = [torch.from_numpy(np.frombuffer(t, dtype=np.uint8).copy()).cuda() for t in tiles]
    text = torch.cat([dt[k] for k in pattern])
    del dt
    total = sum(len(tiles[k]) for k in pattern)
    assert text.numel() == total > 1 << 32
    outs, counts = sk_ctx.trim_fastq(capi.make_params(*pt), text, mode="se")
    del text
    want_md5, want_bytes, want_records = hashlib.md5(), 0, 0
    for k in pattern:
        want_md5.update(wants[k]["texts"][0])
        want_bytes += len(wants[k]["texts"][0])
        want_records += len(wants[k]["index"][0])
    assert counts["records_in"] == [3000 * reps, 0] and counts["tail_lines"] == [0, 0]
    assert counts["records"][0] == want_records and counts["bytes"][0] == want_bytes == outs[0].numel()
    assert want_bytes > 1 << 32
    got_md5 = hashlib.md5()
    for a in range(0, want_bytes, 1 << 28):
        got_md5.update(outs[0][a:a + (1 << 28)].cpu().numpy().tobytes())
    assert got_md5.hexdigest() == want_md5.hexdigest()
    del outs
    torch.cuda.empty_cache()


# ---- 6 capacity --------------------------------------------------------------------------------------------------
def test_capacity(sk_ctx):
    pt = ("sanger", 20, 20, False, False)
    texts = [b"".join(many_good(300, L=100, seed=7)), b"".join(many_good(300, L=100, seed=8))]
    want = fm.expected(pt, texts, "pe_split")
    need = [len(want["texts"][o]) for o in range(3)]
    recs = [len(want["index"][o]) for o in range(3)]
    assert min(recs) > 0
    params = capi.make_params(*pt)
    # count only
    rc, c, _ = raw(sk_ctx, params, texts, "pe_split", caps=[None] * 3)
    assert rc == capi.SK_OK and c["bytes"] == need and c["records"] == recs
    for o in range(3):
        for short in ("bytes", "records"):
            caps, rcaps = [n + 16 for n in need], [r + 1 for r in recs]
            if short == "bytes":
                caps[o] = need[o] - 1
            else:
                rcaps[o] = recs[o] - 1
            rc, c, keep = raw(sk_ctx, params, texts, "pe_split", caps=caps, rec_caps=rcaps)
            assert rc == capi.SK_ESPACE and c["bytes"] == need and c["records"] == recs
            untouched([keep[o]])
            got = texts_of(keep, c)
            for p in range(3):
                if p != o:
                    assert got[p] == want["texts"][p]
    # exact fit with record_index
    rc, c, keep = raw(sk_ctx, params, texts, "pe_split", caps=need, rec_caps=recs)
    assert rc == capi.SK_OK and texts_of(keep, c) == want["texts"]
    for o in range(3):
        assert np.array_equal(keep[o][1].cpu().numpy(), want["index"][o])


# ---- 7 reuse and clean-up ----------------------------------------------------------------------------------------
def test_reuse_streams_and_error_word(sk_ctx):
    torch = torch_mod()
    pt = ("sanger", 20, 20, False, False)
    params = capi.make_params(*pt)
    texts = [b"".join(many_good(n, seed=n)) for n in (500, 300, 700)]
    ws = torch.empty(capi.lib().sk_trim_fastq_workspace_bytes(max(map(len, texts)), 0), dtype=torch.uint8, device="cuda")
    for t in texts:  # one workspace, three calls
        rc, c, keep = raw(sk_ctx, params, [t], "se", ws=ws)
        assert rc == capi.SK_OK and texts_of(keep, c)[0] == fm.expected(pt, [t], "se")["texts"][0]
    # two streams, two workspaces in flight at once
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a = raw(sk_ctx, params, [texts[0]], "se", stream=s1.cuda_stream, finish=False)
    b = raw(sk_ctx, params, [texts[2]], "se", stream=s2.cuda_stream, finish=False)
    for (ws_, keep, _), s, t in ((a, s1, texts[0]), (b, s2, texts[2])):
        c = capi.FastqCounts()
        assert capi.lib().sk_trim_fastq_device_finish(sk_ctx._h, ws_.data_ptr(), s.cuda_stream, C.byref(c)) == capi.SK_OK
        assert texts_of(keep, c.as_dict())[0] == fm.expected(pt, [t], "se")["texts"][0]
    # a range error is reported once: the scan's own finish on that stream then says SK_OK
    bad = texts[1] + RANGE_BAD
    rc, c, _ = raw(sk_ctx, params, [bad], "se", stream=s1.cuda_stream)
    assert rc == capi.SK_ERANGE and c["range"][0] == 300
    assert capi.lib().sk_scan_device_finish(sk_ctx._h, s1.cuda_stream, C.byref(capi.Err())) == capi.SK_OK


def test_trim_fastq_raises(sk_ctx):
    torch = torch_mod()
    t = torch.from_numpy(np.frombuffer(b"@a\nAC\n+\nII\n@\nA\n+\nI\n", np.uint8).copy()).cuda()
    with pytest.raises(capi.FormatError) as e:
        sk_ctx.trim_fastq(capi.make_params(), t)
    assert (e.value.reason, e.value.input, e.value.record) == (capi.SK_FQ_ID_SHORT, 0, 1)
    t = torch.from_numpy(np.frombuffer(RANGE_BAD, np.uint8).copy()).cuda()
    with pytest.raises(capi.RangeError):
        sk_ctx.trim_fastq(capi.make_params(), t)
    t = torch.from_numpy(np.frombuffer(b"".join(many_good(10)), np.uint8).copy()).cuda()
    outs, counts = sk_ctx.trim_fastq(capi.make_params(), t, mode="pe_interleaved", record_index=True)
    assert outs[1] is None and outs[0][1].numel() == counts["records"][0]


# ---- 8 lines over several framing chunks, newlines on chunk boundaries, degenerate texts ----------------------------
def _record(rng, k, L, name=b""):
    q = bytes(rng.integers(35, 75, size=L, dtype=np.uint8))
    s = bytearray(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=L))
    if k % 10 == 3 and L < 1000:
        s[int(rng.integers(0, L))] = ord("N")
    return [b"@r%d%s" % (k, name), bytes(s), b"+", q]


def _join(recs):
    return b"".join(x + b"\n" for r in recs for x in r)


def test_lines_over_several_chunks(sk_ctx):
    """A valid text whose reads of 70 000, 131 072 and 200 000 bases each cover 64 KiB framing chunks without any '\\n',
    among short reads, with -n, at text addresses 0, 1 and 15 past a 16-byte boundary."""
    rng = np.random.default_rng(81)
    lens = [int(x) for x in rng.integers(30, 152, 400)]
    for at, L in ((7, 70_000), (120, 131_072), (121, 200_000), (399, 131_072)):
        lens[at] = L
    text = _join([_record(rng, k, L) for k, L in enumerate(lens)])
    for shift in (0, 1, 15):
        for mode in ("se", "pe_interleaved"):
            rc, counts, _ = check(sk_ctx, ("sanger", 20, 20, False, True), [text], mode, shift=shift)
            assert rc == capi.SK_OK and counts["records_in"][0] == 400 and sum(counts["bytes"]) > 400_000


@pytest.mark.parametrize("item", ["name_nl", "seq_nl", "plus_nl", "qual_nl", "first_byte"])
@pytest.mark.parametrize("byte", [65535, 65536])
@pytest.mark.parametrize("shift", [0, 9])
def test_newline_on_a_chunk_boundary(sk_ctx, item, byte, shift):
    """Each of the four '\\n' of a record, and the record's first byte, on the last byte of the second 64 KiB framing chunk
    and on the first byte of the third (a name line padded to put it there).  The kernel's chunks start at the 16-byte
    boundary below the text: at shift 9 the byte lies on the kernel's chunk edge and not on the text's."""
    rng = np.random.default_rng(82)
    recs = [_record(rng, k, 100) for k in range(1200)]
    i = ["name_nl", "seq_nl", "plus_nl", "qual_nl", "first_byte"].index(item)
    target, at, k = 65536 + byte - shift, 0, 0
    while True:  # the last record whose item lies at or before the target
        size = sum(len(x) + 1 for x in recs[k])
        if at + size + (0 if i == 4 else sum(len(x) + 1 for x in recs[k + 1][:i + 1]) - 1) > target:
            break
        at += size
        k += 1
    pos = at if i == 4 else at + sum(len(x) + 1 for x in recs[k][:i + 1]) - 1
    recs[k - 1 if i == 4 else k][0] += b"p" * (target - pos)
    text = _join(recs)
    assert (text[target] == 10) if i < 4 else (text[target] == ord("@") and text[target - 1] == 10)
    for mode in ("se", "pe_interleaved"):
        rc, counts, _ = check(sk_ctx, ("sanger", 20, 20, False, False), [text], mode, shift=shift)
        assert rc == capi.SK_OK and counts["records_in"][0] == 1200


@pytest.mark.parametrize("name", ["empty", "one_byte", "nl_1", "nl_7", "nl_8", "nl_9", "nl_70000", "leading_nl", "no_nl"])
def test_degenerate_texts(sk_ctx, name):
    """Texts without a record, of newlines only, with a leading newline, and one line longer than a chunk without any
    newline: the counts and the verdict of the model, nothing written."""
    good = b"".join(many_good(50, L=60))
    text = {"empty": b"", "one_byte": b"A", "nl_1": b"\n", "nl_7": b"\n" * 7, "nl_8": b"\n" * 8, "nl_9": b"\n" * 9,
            "nl_70000": b"\n" * 70_000, "leading_nl": b"\n" + good, "no_nl": b"A" * 70_001}[name]
    pt = ("sanger", 20, 20, False, False)
    want = fm.expected(pt, [text], "se")
    if name in ("empty", "one_byte", "nl_1", "no_nl"):  # fewer than four lines: no record, so nothing to judge
        assert want["verdict"] is None and want["records_in"][0] == 0
    else:
        assert want["verdict"] == (capi.SK_FQ_ID_SHORT, 0, 0)
    for mode in ("se", "pe_interleaved"):
        for shift in (0, 9):
            check(sk_ctx, pt, [text], mode, shift=shift)


FASTQ_SOAK = (120, 316)  # iterations, comparisons


def test_fastq_soak(sk_ctx):
    """tests/soak_fastq.py: random FASTQ texts (placed newlines, lines over chunks, endings, malformed records, every mode
    and encoding, capacities) against tests/fastq_model.py (the same draws without a device give the same number of
    comparisons: soak_fastq.py --dry)."""
    import soak_fastq
    assert soak_fastq.run(FASTQ_SOAK[0], 2028, verbose=False) == FASTQ_SOAK[1]
