"""sk_trim_fastq_bases_device_async without a device: the export, the constants, the two struct layouts and every
SK_EINVAL of include/sickle_amd.h before anything touches a device."""
import ctypes as C
import os
import re

from sickle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sickle_amd.h")).read()


def _define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, HEADER).group(1))


def test_symbol_and_constants():
    L = capi.lib()
    assert hasattr(L, "sk_trim_fastq_bases_device_async")
    assert "sk_trim_fastq_bases_device_async" in capi.EXPORTS
    assert re.search(r"\bint sk_trim_fastq_bases_device_async\(", HEADER)
    assert capi.SK_FQ_BASES_RESET == _define("SK_FQ_BASES_RESET") == 1
    assert capi.SK_FQ_BASES_MAX_POS_BINS == _define("SK_FQ_BASES_MAX_POS_BINS") == 1024
    assert capi.SK_FQ_BASES_GC_BINS == _define("SK_FQ_BASES_GC_BINS") == 101
    assert capi.BASES_CLASSES == ("A", "C", "G", "T", "N", "other")


def test_abi_version_stays():
    assert capi.lib().sk_abi_version() == 2


def _members(struct):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return body, re.findall(r"\*?(\w+)(\[\d+\])?\s*[,;]", body)


def test_struct_layout():
    """the header's struct, member by member, against the ctypes one: 24 words, 192 bytes of uint64_t"""
    B = capi.FastqBases
    assert C.sizeof(B) == 192 and capi.BASES_WORDS == 24
    names = ["calls", "calls_failed", "reads", "kept", "bases_in", "bases_out", "lower_in", "lower_out", "reads_n_in",
             "reads_n_out", "gc_none_in", "gc_none_out", "reserved"]
    assert [n for n, _ in B._fields_] == names
    assert [getattr(B, n).offset for n in names] == [0, 8, 16, 24, 32, 80, 128, 136, 144, 152, 160, 168, 176]
    assert B.bases_in.size == B.bases_out.size == 48 and B.reserved.size == 16
    body, members = _members("sk_fastq_bases")
    assert [m for m, _ in members] == names
    assert {m: n for m, n in members if n} == {"bases_in": "[6]", "bases_out": "[6]", "reserved": "[2]"}
    assert "uint64_t" in body and not re.search(r"\b(u?int32_t|int|void)\b", body)
    d = B().as_dict()
    assert set(d) == set(names) - {"reserved"} and d["bases_in"] == [0] * 6 == d["bases_out"]


def test_hists_layout():
    H = capi.FastqBasesHists
    names = ["pos_in", "pos_out", "pos_bins", "gc_in", "gc_out"]
    assert [n for n, _ in H._fields_] == names and C.sizeof(H) == 40
    assert [getattr(H, n).offset for n in names] == [0, 8, 16, 24, 32]
    body, members = _members("sk_fastq_bases_hists")
    assert [m for m, _ in members] == names
    assert re.search(r"uint64_t \*pos_in, \*pos_out;", body) and re.search(r"uint64_t pos_bins;", body)
    assert re.search(r"uint64_t \*gc_in, \*gc_out;", body)


def _call(ctx, ws=0x100000, kind=0, trunc_n=0, text_bytes=4096, cap=0, reserved=0, bases=0x200000, flags=0, src=True, mode=2,
          texts=(0x400000, None), bounds=(4096, 0), inp=True, hists=None):
    s = capi.FastqReportSource(ws, kind, trunc_n, text_bytes, cap, reserved)
    i = capi.FastqInput((C.c_void_p * 2)(*texts), (C.c_uint64 * 2)(*bounds), 0)
    h = capi.FastqBasesHists(*hists) if hists is not None else None
    return capi.lib().sk_trim_fastq_bases_device_async(ctx, C.byref(s) if src else None, C.byref(i) if inp else None, mode,
                                                       bases, C.byref(h) if h is not None else None, flags, None)


def test_argument_checks_without_device():
    """SK_EINVAL before anything touches a device: the context is a zeroed block that only takes the error text."""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    E = capi.SK_EINVAL

    def bad(word, **kw):
        assert _call(ctx, **kw) == E, kw
        assert word in L.sk_last_error(ctx), (kw, L.sk_last_error(ctx))

    assert L.sk_trim_fastq_bases_device_async(None, None, None, 0, None, None, 0, None) == E
    bad(b"required", src=False)
    bad(b"required", ws=None)
    bad(b"required", bases=None)
    bad(b"required", inp=False)                                                   # unlike the audit: the texts are the data
    bad(b"16-byte", ws=0x100008)
    bad(b"bases_dev must be 8-byte", bases=0x200004)
    for at in range(4):                                                           # each array misaligned in turn
        arrays = [0x300000, 0x310000, 0x320000, 0x330000]
        arrays[at] += 4
        bad(b"arrays must be 8-byte", hists=(arrays[0], arrays[1], 64, arrays[2], arrays[3]))
    bad(b"kind", kind=4)
    bad(b"kind", kind=0xffffffff)
    bad(b"mode", mode=4)
    bad(b"mode", mode=-1)
    bad(b"flags", flags=2)
    bad(b"flags", flags=-1)
    bad(b"reserved", reserved=1)
    bad(b"text[1]", mode=capi.SK_TRIM_PE_SPLIT)                                   # split without text[1]
    for mode in (capi.SK_TRIM_SE, capi.SK_TRIM_PE_INTERLEAVED, capi.TRIM_MODES["pe_combo_all"]):
        bad(b"text[1]", mode=mode, texts=(0x400000, 0x500000), bounds=(4096, 4096))  # another mode with one
        bad(b"text[0]", mode=mode, texts=(None, None))                            # SK_TRIM_SE too: it has seq lines
    bad(b"pos_bins is 0", hists=(0x300000, None, 0, None, None))
    bad(b"pos_bins is 0", hists=(None, 0x300000, 0, None, None))
    bad(b"above", hists=(0x300000, 0x310000, capi.SK_FQ_BASES_MAX_POS_BINS + 1, None, None))
    bad(b"above", hists=(None, None, capi.SK_FQ_BASES_MAX_POS_BINS + 1, 0x300000, None))


def test_buffers_reject_unknown_keys():
    import pytest
    with pytest.raises(ValueError):
        capi._BasesBuffers({"len_bins": 4}, "cpu")
