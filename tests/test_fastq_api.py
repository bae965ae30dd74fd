"""CPU: FASTQ text on the device (sk_trim_fastq_*, include/sickle_amd.h): the symbols, the workspace formula, the
argument checks that need no device, and the numpy model the GPU tests compare against, pinned to the reference runs."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import cli_util as cu
import fastq_model as fm
import trim_model as tm
from sickle_amd import capi


def test_fastq_symbols_exported():
    L = capi.lib()
    for name in ("sk_trim_fastq_workspace_bytes", "sk_trim_fastq_device_async", "sk_trim_fastq_device_finish"):
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.sk_abi_version() == 2
    assert capi.SK_EFORMAT == -6
    assert (capi.SK_FQ_ID_SHORT, capi.SK_FQ_LENGTHS, capi.SK_FQ_PAIR_COUNT) == (1, 5, 7)


def header_formula(T, trunc_n):
    """The formula include/sickle_amd.h states."""
    H, G = (T + 2) // 16, (T + 7) // 8
    return (464 + 80 * G + 64 * H + 16 * (T // 65536) + 64 * -(-(H + 1) // 1024)
            + (2 if trunc_n else 1) * 16 * -(-T // 32))


def test_workspace_formula_monotone_and_exact():
    ws = capi.lib().sk_trim_fastq_workspace_bytes
    sizes = [0, 1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 1000, 65535, 65536, 65537, 10 ** 6, 3_400_000_000,
             (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 5 << 30]
    for n in (0, 1):
        got = [ws(T, n) for T in sizes]
        assert got == sorted(got)
        for T, b in zip(sizes, got):
            assert b == header_formula(T, n), (T, n)
            assert b % 16 == 0
        for T in range(0, 3000, 3):
            assert ws(T, n) <= ws(T + 1, n)
    assert ws(1 << 30, 0) < 14.6 * (1 << 30) and ws(1 << 30, 1) < 15.1 * (1 << 30)


def _call(ctx=None, params=True, inp=True, mode=capi.SK_TRIM_SE, text=(0x1000, None), nbytes=(64, 0), outs=None,
          ws=0x100000, ws_bytes=1 << 30):
    p = capi.make_params()
    i = capi.FastqInput((C.c_void_p * 2)(*text), (C.c_uint64 * 2)(*nbytes), 0)
    arr = (capi.FastqOutput * 3)(*(outs or []))
    return capi.lib().sk_trim_fastq_device_async(ctx, C.byref(p) if params else None, C.byref(i) if inp else None, mode,
                                                 arr, ws, ws_bytes, None)


def test_fastq_argument_checks_without_device():
    """Every one of these returns SK_EINVAL before anything touches a device (the pointers are never dereferenced)."""
    L = capi.lib()
    E = capi.SK_EINVAL
    assert _call() == E  # NULL ctx
    assert _call(params=False) == E and _call(inp=False) == E
    assert _call(mode=7) == E
    assert _call(mode=capi.SK_TRIM_PE_SPLIT) == E  # text[1] missing
    assert _call(text=(0x1000, 0x2000), nbytes=(64, 64)) == E  # text[1] in SE
    assert _call(mode=capi.SK_TRIM_PE_INTERLEAVED, text=(0x1000, 0x2000), nbytes=(64, 64)) == E
    assert _call(text=(None, None), nbytes=(64, 0)) == E  # NULL text with bytes
    assert _call(outs=[capi.FastqOutput(0x5001, 64, None, 0)]) == E  # unaligned out.text
    assert _call(outs=[capi.FastqOutput(0x5000, 64, 0x6004, 4)]) == E  # unaligned record_index
    assert _call(ws_bytes=16) == E  # workspace too small
    assert _call(ws=0x100008) == E  # unaligned workspace
    c = capi.FastqCounts()
    assert L.sk_trim_fastq_device_finish(None, 0x10000, None, C.byref(c)) == E
    assert L.sk_trim_fastq_device_finish(None, None, None, None) == E


# ---- the model ---------------------------------------------------------------------------------------------------
def test_model_framing_and_checks():
    t = b"@r1\nACGT\n+\nIIII\n@r2\nAC\n+x\nII"  # last line unterminated
    f = fm.frame(t)
    assert f["records"] == 2 and f["tail_lines"] == 0
    assert fm.verdict([t], "se") is None
    assert fm.frame(t + b"\n@r3\nA")["tail_lines"] == 2
    bad = {b"@\nA\n+\nI\n": 1, b"xr\nA\n+\nI\n": 2, b"@r\n\n+\nI\n": 3, b"@r\nA\n+\n\n": 4, b"@r\nAC\n+\nI\n": 5,
           b"rx\n\n+\n\n": 2, b"\n\n\n\n": 1}
    good = b"@ok\nAC\n+\nII\n"
    for rec, why in bad.items():
        assert fm.verdict([good + rec + good], "se") == (why, 0, 1), rec
    # two malformed records: the lowest wins; split: read order interleaves the inputs
    assert fm.verdict([good + b"@r\n\n+\nI\n" + b"@\nA\n+\nI\n"], "se") == (3, 0, 1)
    assert fm.verdict([good * 3 + b"@\nA\n+\nI\n", good * 3], "pe_split") == (fm.SK_FQ_ID_SHORT, 0, 3)
    assert fm.verdict([good * 2, good * 3], "pe_split") == (fm.SK_FQ_PAIR_COUNT, 1, 2)
    assert fm.verdict([good * 3, good + b"@r\n\n+\nI\n" + good], "pe_split") == (3, 1, 1)
    # a CRLF text frames like any other: the '\r' stays in its line
    assert fm.verdict([b"@r\r\nA\r\n+\r\nI\r\n"], "se") is None


def test_model_emission_by_mode():
    t = b"".join(b"@r%d\nACGTA\n+\nIIIII\n" % k for k in range(4))
    buf, recs = fm.reads([t], "se")
    cuts = np.array([[0, 5], [1, 3], [-1, -1], [0, 0]], np.int32)
    texts, idx = fm.emit(buf, recs, cuts, "se")
    assert texts[0] == b"@r0\nACGTA\n+\nIIIII\n@r1\nCG\n+\nII\n@r3\n\n+\n\n"
    assert idx[0].tolist() == [0, 1, 3]
    texts, idx = fm.emit(buf, recs, cuts, "pe_interleaved")
    assert idx[0].tolist() == [0, 1] and idx[2].tolist() == [3]
    buf, recs = fm.reads([t, t.replace(b"@r", b"@s")], "pe_split")
    texts, idx = fm.emit(buf, recs, np.array([[0, 5], [0, 5], [0, 1], [-1, -1]] * 2, np.int32), "pe_split")
    assert texts[1].startswith(b"@s0\nACGTA\n") and idx[2].tolist() == [2, 6]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_model")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


def golden_texts(argv, workdir):
    """(mode, [input texts], {file name: output index}) of a -a 1 run: the input files as they are."""
    if "-c" in argv:
        return "pe_interleaved", [open(tm._plain(argv[argv.index("-c") + 1], workdir), "rb").read()], \
            {"om.fastq": 0, "os.fastq": 2}
    return "pe_split", [open(tm._plain(argv[argv.index(f) + 1], workdir), "rb").read() for f in ("-f", "-r")], \
        {"o1.fastq": 0, "o2.fastq": 1, "os.fastq": 2}


@pytest.mark.parametrize("name,rec", tm.golden_params())
def test_model_reproduces_reference_runs(workdir, name, rec):
    """The model, from the input files as they are and the oracle's cuts, writes every recorded output file of the
    reference's -a 1 runs byte for byte: what the GPU test holds the device to is the reference's behaviour."""
    mode, texts, files = golden_texts(rec["argv"], workdir)
    res = fm.expected(tm.run_params(rec["argv"]), texts, mode)
    assert res["verdict"] is None and res["range"] is None
    for fname, want in rec["outputs"].items():
        text = res["texts"][files[fname]]
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname
