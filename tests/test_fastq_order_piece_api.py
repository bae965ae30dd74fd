"""CPU: the ordered FASTQ trim in pieces (sk_trim_fastq_ordered_piece_workspace_bytes,
sk_trim_fastq_ordered_piece_device_async, sk_trim_fastq_ordered_piece_device_finish, include/sickle_amd.h): the symbols,
the structs, the workspace formula and the argument checks that need no device."""
import ctypes as C
import inspect

from sickle_amd import capi

NEW = ("sk_trim_fastq_ordered_piece_workspace_bytes", "sk_trim_fastq_ordered_piece_device_async",
       "sk_trim_fastq_ordered_piece_device_finish")


def test_symbols_and_structs():
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.sk_abi_version() == 2
    assert C.sizeof(capi.FastqOrderState) == 64
    assert [(f[0], getattr(capi.FastqOrderState, f[0]).offset) for f in capi.FastqOrderState._fields_] == \
        [("carried_lines", 0), ("batches", 16), ("units", 24), ("last_batch_units", 32), ("ended", 40),
         ("stopped_on_mismatch", 44), ("failed", 48), ("reserved0", 52), ("reserved1", 56)]
    assert C.sizeof(capi.FastqOrderPieceCounts) == 80
    assert [(f[0], getattr(capi.FastqOrderPieceCounts, f[0]).offset) for f in capi.FastqOrderPieceCounts._fields_] == \
        [("table_full", 0), ("undetermined", 4), ("inherited_failure", 8), ("reserved", 12), ("state", 16)]
    for name in ("trim_fastq_ordered_piece_device_async", "trim_fastq_ordered_piece_device_finish"):
        assert hasattr(capi.Context, name), name
    for name in ("trim_fastq_stream", "trim_gz_stream", "trim_gzip_stream"):
        sig = inspect.signature(getattr(capi.Context, name)).parameters
        assert sig["order"].default is None and sig["batch_capacity"].default is None, name


def test_workspace_formula():
    """the ordered call's workspace plus the 256-byte block of the order words; existing formulas as they were"""
    L = capi.lib()
    for text_bytes in (0, 1, 4096, 70001, 1 << 20, (1 << 30) + 5):
        for trunc_n in (0, 1):
            plain = L.sk_trim_fastq_workspace_bytes(text_bytes, trunc_n)
            for cap in (1, 2, 16, 1001, 1 << 20):
                ordered = L.sk_trim_fastq_ordered_workspace_bytes(text_bytes, trunc_n, cap)
                assert ordered == plain + ((8 * (cap + 1) + 15) & ~15)
                assert L.sk_trim_fastq_ordered_piece_workspace_bytes(text_bytes, trunc_n, cap) == ordered + 256


def _call(ctx=0x10, mode=capi.SK_TRIM_SE, text=(0x1000, None), nbytes=(64, 0), lengths=((None, None), (None, None)),
          starts=(None, None), more=1, reserved=0, piece=True, order=(4, 0, 100, 8, 0), state_in=0x600000, state_out=0x600040,
          ws=0x100000, ws_bytes=1 << 30, outs=True):
    p = capi.make_params()
    i = capi.FastqInput((C.c_void_p * 2)(*text), (C.c_uint64 * 2)(*nbytes), 0)
    ln = capi.FastqLengths((C.c_void_p * 2)(*lengths[0]), (C.c_void_p * 2)(*lengths[1]))
    pc = capi.FastqPiece((C.c_void_p * 2)(*starts), more, reserved)
    o = capi.FastqOrder(*order) if order is not None else None
    arr = (capi.FastqOutput * 3)()
    return capi.lib().sk_trim_fastq_ordered_piece_device_async(ctx, C.byref(p), C.byref(i), C.byref(ln),
                                                               C.byref(pc) if piece else None,
                                                               C.byref(o) if o is not None else None, state_in, state_out,
                                                               mode, arr if outs else None, ws, ws_bytes, None)


def test_argument_checks_without_device():
    """Every one of these returns SK_EINVAL before anything touches a device: the context is a zeroed block that only
    takes the error text, the other pointers are made up and never dereferenced."""
    E = capi.SK_EINVAL
    assert _call(ctx=None) == E
    fake = C.create_string_buffer(1 << 16)  # set_error writes its text into the context
    ctx = C.addressof(fake)
    # the new arguments
    assert _call(ctx, piece=False) == E and _call(ctx, order=None) == E and _call(ctx, state_out=None) == E
    assert _call(ctx, state_in=0x600040) == E  # state_in == state_out
    assert _call(ctx, state_in=0x600004) == E and _call(ctx, state_out=0x600044) == E  # not 8-byte aligned
    need = capi.lib().sk_trim_fastq_ordered_piece_workspace_bytes(64, 0, 8)
    assert _call(ctx, ws_bytes=need - 1) == E
    assert _call(ctx, ws_bytes=capi.lib().sk_trim_fastq_ordered_workspace_bytes(64, 0, 8)) == E  # the ordered call's is short
    # those of the ordered call
    assert _call(ctx, order=(0, 0, 100, 8, 0)) == E and _call(ctx, order=(4, 1, 100, 8, 0)) == E
    assert _call(ctx, order=(4, 0, 19, 8, 0)) == E and _call(ctx, order=(4, 0, 100, 0, 0)) == E
    assert _call(ctx, order=(4, 0, 100, (1 << 40) + 1, 0)) == E
    # those of the piece call
    assert _call(ctx, reserved=1) == E
    assert _call(ctx, starts=(0x2004, None)) == E
    assert _call(ctx, mode=capi.SK_TRIM_PE_SPLIT, text=(0x1000, 0x5000), nbytes=(64, 64), starts=(0x2000, 0x3001)) == E
    assert _call(ctx, starts=(0x2000, 0x3000)) == E  # a start word for text[1] outside SK_TRIM_PE_SPLIT
    assert _call(ctx, mode=capi.SK_TRIM_PE_INTERLEAVED, starts=(None, 0x3000)) == E
    # those of the chained call and of the text call
    assert _call(ctx, lengths=((0x2004, None), (None, None))) == E
    assert _call(ctx, lengths=((0x2000, 0x3000), (None, None))) == E
    assert _call(ctx, mode=7) == E and _call(ctx, ws_bytes=16) == E and _call(ctx, ws=0x100008) == E and _call(ctx, ws=None) == E
    assert _call(ctx, text=(0x1000, 0x5000)) == E  # text[1] outside SK_TRIM_PE_SPLIT
    assert _call(ctx, text=(None, None)) == E and _call(ctx, outs=False) == E
    assert _call(ctx, mode=capi.SK_TRIM_PE_SPLIT, text=(0x1000, None), nbytes=(64, 64)) == E


def test_finish_argument_checks_without_device():
    L = capi.lib()
    c = capi.FastqCounts()
    assert L.sk_trim_fastq_ordered_piece_device_finish(None, 0x100000, None, C.byref(c), None, None, None) == capi.SK_EINVAL
    fake = C.create_string_buffer(1 << 16)
    assert L.sk_trim_fastq_ordered_piece_device_finish(C.addressof(fake), None, None, C.byref(c), None, None, None) == capi.SK_EINVAL
    assert L.sk_trim_fastq_ordered_piece_device_finish(C.addressof(fake), 0x100000, None, None, None, None, None) == capi.SK_EINVAL


def test_existing_piece_words_work_on_the_new_workspace():
    """sk_trim_fastq_piece_words and sk_trim_fastq_output_words hand out header words, which an ordered piece keeps where
    they are (sk_device.h): below the header's 32 words, in front of the block of the order words."""
    base = 0x7f0000001000
    for i in (0, 1):
        assert all(base <= x < base + 256 for x in capi.Context.trim_fastq_piece_words(base, i))
    for o in range(3):
        assert all(base <= x < base + 256 for x in capi.Context.trim_fastq_output_words(base, o))
