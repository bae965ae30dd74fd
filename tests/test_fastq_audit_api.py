"""sk_trim_fastq_audit_device_async without a device: the export, the constants, the struct layout, every SK_EINVAL of
include/sickle_amd.h before anything touches a device, and qualtypes_consistent."""
import ctypes as C
import os
import re

from sickle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sickle_amd.h")).read()


def test_symbol_and_constants():
    L = capi.lib()
    assert hasattr(L, "sk_trim_fastq_audit_device_async")
    assert "sk_trim_fastq_audit_device_async" in capi.EXPORTS
    assert re.search(r"\bint sk_trim_fastq_audit_device_async\(", HEADER)
    assert capi.SK_FQ_AUDIT_RESET == int(re.search(r"#define\s+SK_FQ_AUDIT_RESET\s+(\d+)", HEADER).group(1)) == 1
    assert capi.AUDIT_NONE == 2 ** 64 - 1


def test_abi_version_stays():
    assert capi.lib().sk_abi_version() == 2


def test_struct_layout():
    """the header's struct, member by member, against the ctypes one: 128 bytes of uint64_t"""
    A = capi.FastqAudit
    assert C.sizeof(A) == 128 and capi.AUDIT_WORDS == 16
    names = ["calls", "calls_failed", "pairs", "name_mismatch", "first_mismatch", "tags_swapped", "qual_bytes", "qual_min",
             "qual_max", "reserved"]
    assert [n for n, _ in A._fields_] == names
    assert [getattr(A, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72]
    assert A.reserved.size == 56
    body = re.search(r"typedef struct \{([^}]*)\} sk_fastq_audit;", HEADER).group(1)
    members = re.findall(r"(\w+)(\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert [m for m, _ in members] == names and members[-1][1] == "[7]"
    assert "uint64_t" in body and not re.search(r"\b(u?int32_t|int|void)\b", body)
    assert set(A().as_dict()) == set(names) - {"reserved"}


def _call(ctx, ws=0x100000, kind=0, trunc_n=0, text_bytes=4096, cap=0, reserved=0, audit=0x200000, hist=0x300000, flags=0,
          src=True, mode=2, texts=(0x400000, None), bounds=(4096, 0), inp=True):
    s = capi.FastqReportSource(ws, kind, trunc_n, text_bytes, cap, reserved)
    i = capi.FastqInput((C.c_void_p * 2)(*texts), (C.c_uint64 * 2)(*bounds), 0)
    return capi.lib().sk_trim_fastq_audit_device_async(ctx, C.byref(s) if src else None, C.byref(i) if inp else None, mode,
                                                       audit, hist, flags, None)


def test_argument_checks_without_device():
    """SK_EINVAL before anything touches a device: the context is a zeroed block that only takes the error text."""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    E = capi.SK_EINVAL

    def bad(word, **kw):
        assert _call(ctx, **kw) == E, kw
        assert word in L.sk_last_error(ctx), (kw, L.sk_last_error(ctx))

    assert L.sk_trim_fastq_audit_device_async(None, None, None, 0, None, None, 0, None) == E
    bad(b"required", src=False)
    bad(b"required", ws=None)
    bad(b"required", audit=None)
    bad(b"16-byte", ws=0x100008)
    bad(b"audit_dev must be 8-byte", audit=0x200004)
    bad(b"qual_hist_dev must be 8-byte", hist=0x300004)
    bad(b"kind", kind=4)
    bad(b"kind", kind=0xffffffff)
    bad(b"mode", mode=4)
    bad(b"mode", mode=-1)
    bad(b"mode", mode=4, inp=False)
    bad(b"text[1]", mode=capi.SK_TRIM_PE_SPLIT)                                   # split without text[1]
    for mode in (capi.SK_TRIM_SE, capi.SK_TRIM_PE_INTERLEAVED, capi.TRIM_MODES["pe_combo_all"]):
        bad(b"text[1]", mode=mode, texts=(0x400000, 0x500000), bounds=(4096, 4096))  # another mode with one
    bad(b"text[0]", texts=(None, None))
    bad(b"flags", flags=2)
    bad(b"flags", flags=-1)
    bad(b"reserved", reserved=1)


def test_qualtypes_consistent():
    q = lambda lo, hi, n=10: capi.qualtypes_consistent({"qual_bytes": n, "qual_min": lo, "qual_max": hi})
    assert q(33, 73) == ["sanger"]
    assert q(66, 105) == ["sanger", "solexa", "illumina"]      # tests/golden/inputs/test.fastq
    assert q(59, 104) == ["sanger", "solexa"]
    assert q(64, 110) == ["sanger", "solexa", "illumina"]
    assert q(64, 111) == ["sanger", "solexa"]
    assert q(58, 112) == ["sanger", "solexa"]
    assert q(57, 112) == ["sanger"]
    assert q(33, 126) == ["sanger"]
    assert q(32, 126) == [] and q(33, 127) == [] and q(0x80, 0xff) == []
    assert q(capi.AUDIT_NONE, 0, n=0) == ["sanger", "solexa", "illumina"]
    a = capi.FastqAudit()
    a.qual_bytes, a.qual_min, a.qual_max = 5, 70, 80
    assert capi.qualtypes_consistent(a) == ["sanger", "solexa", "illumina"]
