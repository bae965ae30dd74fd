"""CPU: the FASTQ trim in pieces (sk_trim_fastq_piece_device_async, sk_trim_fastq_piece_words,
sk_trim_fastq_piece_device_finish, sk_fastq_carry_device_async, include/sickle_amd.h): the symbols, the structs, the
argument checks that need no device and the header words a piece hands out."""
import ctypes as C
import inspect

from sickle_amd import capi

NEW = ("sk_trim_fastq_piece_device_async", "sk_trim_fastq_piece_words", "sk_trim_fastq_piece_device_finish",
       "sk_fastq_carry_device_async")


def test_piece_symbols_and_structs():
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.sk_abi_version() == 2
    assert C.sizeof(capi.FastqPiece) == 24
    assert [(f[0], getattr(capi.FastqPiece, f[0]).offset) for f in capi.FastqPiece._fields_] == \
        [("start_dev", 0), ("more", 16), ("reserved", 20)]
    assert C.sizeof(capi.FastqPieceCounts) == 40
    assert [(f[0], getattr(capi.FastqPieceCounts, f[0]).offset) for f in capi.FastqPieceCounts._fields_] == \
        [("consumed", 0), ("carried_bytes", 16), ("ok", 32), ("inherited_range", 36)]
    assert C.sizeof(capi.FastqCarryWords) == 32
    assert [(f[0], getattr(capi.FastqCarryWords, f[0]).offset) for f in capi.FastqCarryWords._fields_] == \
        [("start", 0), ("end", 8), ("valid", 16), ("status", 24)]
    for name in ("trim_fastq_piece_device_async", "trim_fastq_piece_device_finish", "trim_fastq_piece_words",
                 "fastq_carry_device_async", "trim_fastq_stream", "trim_gz_stream"):
        assert hasattr(capi.Context, name), name
    sig = inspect.signature(capi.Context.trim_fastq_stream).parameters
    assert sig["room"].default is None and sig["gz"].default is False and sig["mode"].default == "se"


def _piece(ctx=0x10, mode=capi.SK_TRIM_SE, text=(0x1000, None), nbytes=(64, 0), lengths=((None, None), (None, None)),
           starts=(None, None), more=1, reserved=0, piece=True, ws=0x100000, ws_bytes=1 << 30):
    p = capi.make_params()
    i = capi.FastqInput((C.c_void_p * 2)(*text), (C.c_uint64 * 2)(*nbytes), 0)
    ln = capi.FastqLengths((C.c_void_p * 2)(*lengths[0]), (C.c_void_p * 2)(*lengths[1]))
    pc = capi.FastqPiece((C.c_void_p * 2)(*starts), more, reserved)
    arr = (capi.FastqOutput * 3)()
    return capi.lib().sk_trim_fastq_piece_device_async(ctx, C.byref(p), C.byref(i), C.byref(ln), C.byref(pc) if piece else None,
                                                       mode, arr, ws, ws_bytes, None)


def test_piece_argument_checks_without_device():
    """Every one of these returns SK_EINVAL before anything touches a device: the context is a zeroed block that only
    takes the error text, the other pointers are made up and never dereferenced."""
    E = capi.SK_EINVAL
    assert _piece(ctx=None) == E and _piece(ctx=None, piece=False) == E  # NULL ctx
    fake = C.create_string_buffer(1 << 16)  # set_error writes its text into the context
    ctx = C.addressof(fake)
    assert _piece(ctx, reserved=1) == E
    assert _piece(ctx, starts=(0x2004, None)) == E  # a start word that is not 8-byte aligned
    assert _piece(ctx, mode=capi.SK_TRIM_PE_SPLIT, text=(0x1000, 0x5000), nbytes=(64, 64), starts=(0x2000, 0x3001)) == E
    assert _piece(ctx, starts=(0x2000, 0x3000)) == E  # a start word for text[1] outside SK_TRIM_PE_SPLIT
    assert _piece(ctx, mode=capi.SK_TRIM_PE_INTERLEAVED, starts=(None, 0x3000)) == E
    # those of the chained call
    assert _piece(ctx, lengths=((0x2004, None), (None, None))) == E
    assert _piece(ctx, lengths=((0x2000, 0x3000), (None, None))) == E
    assert _piece(ctx, mode=7) == E and _piece(ctx, ws_bytes=16) == E and _piece(ctx, ws=0x100008) == E
    assert _piece(ctx, text=(0x1000, 0x5000)) == E  # text[1] outside SK_TRIM_PE_SPLIT
    assert _piece(ctx, piece=False, ws_bytes=16) == E


def _carry(ctx, prev_ws=0x100000, input=0, prev_text=0x200000, prev_bytes=4096, next_text=0x300000, room=4096,
           nb_dev=None, chunk=100, valid_dev=None, prev_words=0x400000, other=None, words=0x400020):
    return capi.lib().sk_fastq_carry_device_async(ctx, prev_ws, input, prev_text, prev_bytes, next_text, room, nb_dev, chunk,
                                                  valid_dev, prev_words, other, words, None)


def test_carry_argument_checks_without_device():
    E = capi.SK_EINVAL
    assert _carry(None) == E
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    assert _carry(ctx, next_text=None) == E and _carry(ctx, words=None) == E
    assert _carry(ctx, input=2) == E and _carry(ctx, input=-1) == E
    assert _carry(ctx, prev_text=None) == E
    assert _carry(ctx, room=4100) == E  # not a multiple of 16
    assert _carry(ctx, words=0x400024) == E and _carry(ctx, prev_words=0x400004) == E and _carry(ctx, nb_dev=0x500001) == E
    assert _carry(ctx, valid_dev=0x500002) == E and _carry(ctx, other=0x400044) == E
    assert _carry(ctx, words=0x400000) == E and _carry(ctx, other=0x400020) == E  # words is one of the previous words
    # [next_text, next_text + room) meets [prev_text, prev_text + prev_bytes)
    assert _carry(ctx, next_text=0x200000) == E
    assert _carry(ctx, next_text=0x200fff) == E
    assert _carry(ctx, next_text=0x1ff001) == E


def test_piece_words():
    """No device is touched: the workspace address is made up.  The words lie in the header (sk_device.h: consumed 25 / 26,
    end 23 / 24, ok 27), below its 32 words."""
    L = capi.lib()
    base = 0x7f0000001000
    a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.sk_trim_fastq_piece_words(None, 0, C.byref(a), C.byref(b), C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_piece_words(base, 2, C.byref(a), C.byref(b), C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_piece_words(base, -1, C.byref(a), C.byref(b), C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_piece_words(base, 0, None, C.byref(b), C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_piece_words(base, 0, C.byref(a), None, C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_piece_words(base, 0, C.byref(a), C.byref(b), None) == capi.SK_EINVAL
    for i in (0, 1):
        assert capi.Context.trim_fastq_piece_words(base, i) == (base + 8 * (25 + i), base + 8 * (23 + i), base + 8 * 27)
        assert all(base <= x < base + 256 for x in capi.Context.trim_fastq_piece_words(base, i))
