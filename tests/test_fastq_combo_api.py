"""CPU: mode SK_TRIM_PE_COMBO_ALL ("pe_combo_all", sickle's -M) of the FASTQ text calls (include/sickle_amd.h): the
constant, the argument checks of all five calls that need no device, sk_trim_device_async's refusal, and the output
bound the Python drivers size by, held against the model."""
import ctypes as C

import combo_all_model as cm
from sickle_amd import capi

COMBO = 3


def test_the_mode_exists():
    assert capi.SK_TRIM_PE_COMBO_ALL == COMBO
    assert "pe_combo_all" in capi.TRIM_MODES and capi.TRIM_MODES["pe_combo_all"] == COMBO
    assert capi.TRIM_OUTPUTS["pe_combo_all"] == (0,)
    assert capi.lib().sk_abi_version() == 2  # the mode is an addition: no new export, no struct changed


def _calls(ctx, mode, text=(0x1000, None), nbytes=(64, 0), ws_bytes=1 << 30):
    """the five text calls with made-up pointers that are never dereferenced -> their return values, by name"""
    L = capi.lib()
    p = capi.make_params()
    i = capi.FastqInput((C.c_void_p * 2)(*text), (C.c_uint64 * 2)(*nbytes), 0)
    ln = capi.FastqLengths((C.c_void_p * 2)(None, None), (C.c_void_p * 2)(None, None))
    pc = capi.FastqPiece((C.c_void_p * 2)(None, None), 1, 0)
    o = capi.FastqOrder(4, 0, 100, 8, 0)
    arr = (capi.FastqOutput * 3)()
    ws = 0x100000
    P, I, LN, PC, O = C.byref(p), C.byref(i), C.byref(ln), C.byref(pc), C.byref(o)
    return {
        "plain": L.sk_trim_fastq_device_async(ctx, P, I, mode, arr, ws, ws_bytes, None),
        "chained": L.sk_trim_fastq_chained_device_async(ctx, P, I, LN, mode, None, arr, ws, ws_bytes, None),
        "chained+order": L.sk_trim_fastq_chained_device_async(ctx, P, I, LN, mode, O, arr, ws, ws_bytes, None),
        "piece": L.sk_trim_fastq_piece_device_async(ctx, P, I, LN, PC, mode, arr, ws, ws_bytes, None),
        "ordered": L.sk_trim_fastq_ordered_device_async(ctx, P, I, mode, O, arr, ws, ws_bytes, None),
        "ordered piece": L.sk_trim_fastq_ordered_piece_device_async(ctx, P, I, LN, PC, O, 0x600000, 0x600040, mode, arr, ws,
                                                                  ws_bytes, None),
    }


def test_argument_checks_without_device():
    """SK_EINVAL before anything touches a device: the context is a zeroed block that only takes the error text."""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    E = capi.SK_EINVAL
    # a second text is only for SK_TRIM_PE_SPLIT
    for name, rc in _calls(ctx, COMBO, text=(0x1000, 0x2000), nbytes=(64, 64)).items():
        assert rc == E, name
        assert b"text[1]" in L.sk_last_error(ctx), name
    for name, rc in _calls(ctx, COMBO, text=(0x1000, None), nbytes=(64, 64)).items():
        assert rc == E, name
    # an unknown mode stays unknown
    for name, rc in _calls(ctx, 7).items():
        assert rc == E, name
        assert b"unknown" in L.sk_last_error(ctx), name
    for name, rc in _calls(ctx, 4).items():
        assert rc == E, name
    # the mode itself is known: with everything else in order the first complaint is the workspace's size
    for name, rc in _calls(ctx, COMBO, ws_bytes=16).items():
        assert rc == E, name
        assert b"workspace" in L.sk_last_error(ctx) and b"unknown" not in L.sk_last_error(ctx), name


def test_packed_trim_refuses_the_mode():
    """sk_trim_device_async takes packed reads, which have no name line: mode 3 is SK_EINVAL there"""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    b = capi.Batch(0x1000, None, 0x2000, 0, 0, None, 2)
    arr = (capi.TrimOutput * 3)()
    assert L.sk_trim_device_async(ctx, C.byref(b), 0x3000, COMBO, arr, 0x100000, 1 << 20, None) == capi.SK_EINVAL
    assert b"FASTQ text calls" in L.sk_last_error(ctx)
    assert L.sk_trim_device_async(ctx, C.byref(b), 0x3000, 7, arr, 0x100000, 1 << 20, None) == capi.SK_EINVAL
    assert b"unknown" in L.sk_last_error(ctx)


def test_output_bound():
    """capi.fastq_output_bound: the other modes' outputs never exceed the text by more than the two newlines; the new
    mode's can, by one byte per record, and the bound is met to within those two bytes by 1-base reads with empty '+'
    lines that all fail"""
    for mode in ("se", "pe_split", "pe_interleaved"):
        assert [capi.fastq_output_bound(T, mode) for T in (0, 1, 64, 1 << 32)] == [2, 3, 66, (1 << 32) + 2]
    for n in (2, 64, 1000):
        for tail in (b"\n", b""):  # the last line with and without its newline
            text = (b"@a\nA\n\n#\n" * n)[:-1] + tail
            want = cm.expected(cm.TRUTH_PARAMS, text)
            assert want["classes"].tolist() == [3] * (n // 2)
            out = want["texts"][0]
            assert out == b"@a\nN\n+\n!\n" * n
            assert len(out) == 8 * n + n == cm.bound(len(text), n) - len(tail)
            b = capi.fastq_output_bound(len(text), "pe_combo_all")
            assert len(out) <= b <= len(out) + 2
    # monotone, and never below the text plus its records plus one
    prev = 0
    for T in range(0, 4000):
        b = capi.fastq_output_bound(T, "pe_combo_all")
        assert b >= prev and b >= cm.bound(T, (T + 1) // 8)
        prev = b
