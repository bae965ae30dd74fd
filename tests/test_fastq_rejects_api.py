"""sk_trim_fastq_rejects_device_async without a device: the exports, the constant, the struct layout, the workspace formula
against its stated bound and every SK_EINVAL of include/sickle_amd.h before anything touches a device."""
import ctypes as C
import os
import re

import pytest

from sickle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sickle_amd.h")).read()
NAMES = ("sk_trim_fastq_rejects_workspace_bytes", "sk_trim_fastq_rejects_device_async", "sk_trim_fastq_rejects_device_finish",
         "sk_trim_fastq_rejects_output_words", "sk_trim_fastq_rejects_bound")


def test_symbols_and_constant():
    L = capi.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in capi.EXPORTS
        assert re.search(r"\b(int|size_t|uint64_t) %s\(" % name, HEADER)
    assert capi.SK_FQ_REJECTS_PAIRS == int(re.search(r"#define\s+SK_FQ_REJECTS_PAIRS\s+(\d+)\b", HEADER).group(1)) == 1
    assert capi._rejects_flags(True) == 0 and capi._rejects_flags("pairs") == capi.SK_FQ_REJECTS_PAIRS
    with pytest.raises(ValueError):
        capi._rejects_flags("pair")


def test_abi_version_stays():
    assert capi.lib().sk_abi_version() == 2


def test_struct_layout():
    """the header's struct, member by member, against the ctypes one: three uint64_t and two uint32_t, 32 bytes"""
    S = capi.FastqRejectsCounts
    names = ["records", "bytes", "reads", "valid", "flags"]
    assert [n for n, _ in S._fields_] == names and C.sizeof(S) == 32
    assert [getattr(S, n).offset for n in names] == [0, 8, 16, 24, 28]
    body = re.search(r"typedef struct \{([^}]*)\} sk_fastq_rejects_counts;", HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    assert re.findall(r"(\w+)\s*[,;]", body) == names
    assert re.search(r"uint64_t records, bytes;", body) and re.search(r"uint64_t reads;", body)
    assert re.search(r"uint32_t valid;", body) and re.search(r"uint32_t flags;", body)
    assert S().as_dict() == dict.fromkeys(names, 0)


def _reads_bound(t):
    return 2 * ((t + 2) // 16) + 2


@pytest.mark.parametrize("t", [0, 1, 13, 14, 15, 16, 29, 30, 4095, 4096, 16381, 16382, 16383, 16384, 65536, (1 << 20) + 7,
                               3_160_000_000, (1 << 35) - 1])
def test_workspace_formula(t):
    """a pure function of text_bytes: 16 N, a block table and a header, N the reads of the text call's layout; and the
    text bound T + 2"""
    L = capi.lib()
    n = _reads_bound(t)
    blocks = -(-n // 2048)
    got = L.sk_trim_fastq_rejects_workspace_bytes(t)
    assert got == 128 + 16 * blocks + 16 * n
    assert got % 16 == 0 and got <= 16 * n + 16 * (n // 2048 + 1) + 128
    # the emission's cost: what the text call's own workspace spends on its emit section and block table, or less
    assert got <= L.sk_trim_fastq_workspace_bytes(t, 0)
    assert L.sk_trim_fastq_rejects_bound(t) == t + 2


def _call(ctx, src_ws=0x100000, kind=0, trunc_n=0, text_bytes=4096, cap=0, reserved=0, flags=0, src=True, mode=2,
          texts=(0x400000, None), bounds=(4096, 0), inp=True, out=(0x600000, 8192, 0x700000, 64), ws=0x800000, ws_bytes=None):
    s = capi.FastqReportSource(src_ws, kind, trunc_n, text_bytes, cap, reserved)
    i = capi.FastqInput((C.c_void_p * 2)(*texts), (C.c_uint64 * 2)(*bounds), 0)
    o = capi.FastqOutput(*out) if out is not None else None
    if ws_bytes is None:
        ws_bytes = capi.lib().sk_trim_fastq_rejects_workspace_bytes(text_bytes)
    return capi.lib().sk_trim_fastq_rejects_device_async(ctx, C.byref(s) if src else None, C.byref(i) if inp else None, mode,
                                                         C.byref(o) if o is not None else None, flags, ws, ws_bytes, None)


def test_argument_checks_without_device():
    """SK_EINVAL before anything touches a device: the context is a zeroed block that only takes the error text."""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    E = capi.SK_EINVAL
    split = capi.SK_TRIM_PE_SPLIT

    def bad(word, **kw):
        assert _call(ctx, **kw) == E, kw
        assert word in L.sk_last_error(ctx), (kw, L.sk_last_error(ctx))

    assert L.sk_trim_fastq_rejects_device_async(None, None, None, 0, None, 0, None, 0, None) == E
    bad(b"required", src=False)
    bad(b"required", src_ws=None)
    bad(b"required", inp=False)
    bad(b"required", ws=None)
    bad(b"src->workspace must be 16-byte", src_ws=0x100008)
    bad(b"workspace must be 16-byte", ws=0x800008)
    bad(b"out->text must be 16-byte", out=(0x600008, 8192, None, 0))
    bad(b"record_index must be 8-byte", out=(0x600000, 8192, 0x700004, 64))
    bad(b"kind", kind=4)
    bad(b"kind", kind=0xffffffff)
    bad(b"mode", mode=4)
    bad(b"mode", mode=-1)
    bad(b"flags", flags=2)
    bad(b"flags", flags=3)
    bad(b"flags", flags=-1)
    bad(b"pair mode", flags=capi.SK_FQ_REJECTS_PAIRS, mode=capi.SK_TRIM_SE)
    bad(b"reserved", reserved=1)
    bad(b"text[1]", mode=split)                                                   # split without text[1]
    for mode in (capi.SK_TRIM_SE, capi.SK_TRIM_PE_INTERLEAVED, capi.TRIM_MODES["pe_combo_all"]):
        bad(b"text[1]", mode=mode, texts=(0x400000, 0x500000), bounds=(4096, 4096))  # another mode with one
        bad(b"text[0]", mode=mode, texts=(None, None))                            # a text NULL with bytes != 0
    bad(b"text[0]", mode=split, texts=(None, 0x500000), bounds=(4096, 4096))
    bad(b"bytes[1] != 0", mode=capi.SK_TRIM_SE, bounds=(4096, 1))
    need = L.sk_trim_fastq_rejects_workspace_bytes(4096)
    bad(b"must hold", ws_bytes=need - 1)
    bad(b"must hold", ws_bytes=0)
    bad(b"must hold", text_bytes=1 << 20, ws_bytes=need)                          # sized for another text
    bad(b"beyond", text_bytes=(1 << 35) + 1)


def test_finish_and_words_refuse_null():
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    c = capi.FastqRejectsCounts()
    assert L.sk_trim_fastq_rejects_device_finish(None, 0x100000, None, C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_rejects_device_finish(ctx, None, None, C.byref(c)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_rejects_device_finish(ctx, 0x100000, None, None) == capi.SK_EINVAL
    b, w = C.c_void_p(), C.c_void_p()
    assert L.sk_trim_fastq_rejects_output_words(None, C.byref(b), C.byref(w)) == capi.SK_EINVAL
    assert L.sk_trim_fastq_rejects_output_words(0x100000, None, C.byref(w)) == capi.SK_EINVAL
    # two words of the workspace's header, 8-byte aligned, not the same word
    assert capi.Context.trim_fastq_rejects_output_words(0x100000) == (0x100000 + 8 * 7, 0x100000 + 8 * 6)
