"""CPU: the device-length chain (sk_trim_fastq_chained_device_async, sk_bgzf_inflate_output_words,
sk_gzip_inflate_output_words, include/sickle_amd.h): the symbols, the struct, the argument checks that need no device and
the header words the two readers hand out."""
import ctypes as C
import inspect

from sickle_amd import capi

NEW = ("sk_trim_fastq_chained_device_async", "sk_bgzf_inflate_output_words", "sk_gzip_inflate_output_words")


def test_chain_symbols_exported():
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.sk_abi_version() == 2
    assert C.sizeof(capi.FastqLengths) == 32
    assert [f[0] for f in capi.FastqLengths._fields_] == ["bytes_dev", "valid_dev"]
    assert capi.FastqLengths.valid_dev.offset == 16
    for name in ("trim_fastq_chained_device_async", "bgzf_inflate_output_words", "gzip_inflate_output_words"):
        assert hasattr(capi.Context, name), name
    sig = inspect.signature(capi.Context.trim_gz).parameters
    assert sig["text_capacity"].default is None and sig["kind"].default is None


def _call(ctx=None, mode=capi.SK_TRIM_SE, text=(0x1000, None), nbytes=(64, 0), lengths=((None, None), (None, None)),
          order=None, ws=0x100000, ws_bytes=1 << 30):
    p = capi.make_params()
    i = capi.FastqInput((C.c_void_p * 2)(*text), (C.c_uint64 * 2)(*nbytes), 0)
    ln = None if lengths is None else capi.FastqLengths((C.c_void_p * 2)(*lengths[0]), (C.c_void_p * 2)(*lengths[1]))
    arr = (capi.FastqOutput * 3)()
    return capi.lib().sk_trim_fastq_chained_device_async(ctx, C.byref(p), C.byref(i), None if ln is None else C.byref(ln),
                                                         mode, None if order is None else C.byref(order), arr, ws, ws_bytes,
                                                         None)


def test_chained_argument_checks_without_device():
    """Every one of these returns SK_EINVAL before anything touches a device: the pointers are made up and never
    dereferenced.  (tests/test_gpu_fastq_chain.py repeats the two new checks with a real context and looks at the
    workspace afterwards.)"""
    E = capi.SK_EINVAL
    assert _call() == E and _call(lengths=None) == E  # NULL ctx
    assert _call(lengths=((0x2004, None), (None, None))) == E  # a word that is not 8-byte aligned
    assert _call(lengths=((None, None), (0x2001, None))) == E
    assert _call(lengths=((0x2000, 0x3000), (None, None))) == E  # a word for text[1] outside SK_TRIM_PE_SPLIT
    assert _call(mode=capi.SK_TRIM_PE_INTERLEAVED, lengths=((0x2000, None), (None, 0x3000))) == E
    assert _call(mode=capi.SK_TRIM_PE_SPLIT, text=(0x1000, 0x5000), nbytes=(64, 64),
                 lengths=((0x2000, 0x3002), (None, None))) == E
    assert _call(mode=7) == E and _call(ws_bytes=16) == E and _call(ws=0x100008) == E
    assert _call(order=capi.FastqOrder(0, 0, 100, 4, 0)) == E  # the ordered call's checks: threads 0
    assert _call(order=capi.FastqOrder(3, 0, 10, 4, 0)) == E   # batch_len < 20


def test_reader_output_words():
    """No device is touched: the workspace address is made up.  The words are bytes_out and the written word of each
    reader's header (sk_device.h: SK_INFLATE_H_BYTES_OUT 2 / SK_INFLATE_H_WRITTEN 8; sk_gunzip_block.h: SKG_H_BYTES_OUT 2 /
    SKG_H_WRITTEN 11)."""
    L = capi.lib()
    base = 0x7f0000001000
    for fn, words in ((L.sk_bgzf_inflate_output_words, (2, 8)), (L.sk_gzip_inflate_output_words, (2, 11))):
        b, w = C.c_void_p(), C.c_void_p()
        assert fn(None, C.byref(b), C.byref(w)) == capi.SK_EINVAL
        assert fn(base, None, C.byref(w)) == capi.SK_EINVAL
        assert fn(base, C.byref(b), None) == capi.SK_EINVAL
        assert fn(base, C.byref(b), C.byref(w)) == capi.SK_OK
        assert (b.value, w.value) == (base + 8 * words[0], base + 8 * words[1])
    assert capi.Context.bgzf_inflate_output_words(base) == (base + 16, base + 64)
    assert capi.Context.gzip_inflate_output_words(base) == (base + 16, base + 88)
