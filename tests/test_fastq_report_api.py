"""sk_trim_fastq_report_device_async without a device: the export, the constants, the struct layouts, and every SK_EINVAL
of include/sickle_amd.h before anything touches a device."""
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
    assert hasattr(L, "sk_trim_fastq_report_device_async")
    assert "sk_trim_fastq_report_device_async" in capi.EXPORTS
    assert capi.SK_FQ_REPORT_RESET == _define("SK_FQ_REPORT_RESET") == 1
    assert capi.SK_FQ_REPORT_MAX_LEN_BINS == _define("SK_FQ_REPORT_MAX_LEN_BINS")
    assert capi.SK_FQ_REPORT_MAX_POS_BINS == _define("SK_FQ_REPORT_MAX_POS_BINS")
    # the LDS tables fit beside each other: 32-bit length counters and 64-bit position words, two tables each
    assert 2 * 4 * capi.SK_FQ_REPORT_MAX_LEN_BINS + 2 * 8 * capi.SK_FQ_REPORT_MAX_POS_BINS <= 64 * 1024
    kinds = re.search(r"enum \{ (SK_FQ_REPORT_PLAIN[^}]*)\}", HEADER).group(1)
    want = {"SK_FQ_REPORT_PLAIN": "plain", "SK_FQ_REPORT_PIECE": "piece", "SK_FQ_REPORT_ORDERED": "ordered",
            "SK_FQ_REPORT_ORDERED_PIECE": "ordered_piece"}
    for item in kinds.split(","):
        name, value = (x.strip() for x in item.split("="))
        assert capi.REPORT_KINDS[want[name]] == int(value)


def test_abi_version_stays():
    assert capi.lib().sk_abi_version() == 2


def test_struct_sizes():
    """the header's structs, member by member, against the ctypes ones"""
    assert C.sizeof(capi.FastqReport) == 18 * 8 == 144
    assert [n for n, _ in capi.FastqReport._fields_] == [
        "calls", "calls_failed", "reads", "kept", "discarded", "pairs", "bases_in", "bases_out", "bases_cut5", "bases_cut3",
        "bases_discarded", "reads_cut5", "reads_cut3", "max_len_in", "max_len_out"]
    assert capi.FastqReport.pairs.offset == 40 and capi.FastqReport.pairs.size == 32
    assert capi.FastqReport.max_len_out.offset == 136
    body = re.search(r"typedef struct \{([^}]*)\} sk_fastq_report;", HEADER).group(1)
    members = re.findall(r"(\w+)(\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body))
    assert [m for m, _ in members] == [n for n, _ in capi.FastqReport._fields_]
    assert "uint64_t" in body and not re.search(r"\b(u?int32_t|int|void)\b", body)  # every member is a uint64_t
    assert C.sizeof(capi.FastqReportSource) == 40
    assert (capi.FastqReportSource.kind.offset, capi.FastqReportSource.trunc_n.offset, capi.FastqReportSource.text_bytes.offset,
            capi.FastqReportSource.batch_capacity.offset, capi.FastqReportSource.reserved.offset) == (8, 12, 16, 24, 32)
    assert C.sizeof(capi.FastqReportHists) == 64
    assert (capi.FastqReportHists.len_bins.offset, capi.FastqReportHists.qsum_in.offset,
            capi.FastqReportHists.pos_bins.offset) == (16, 24, 56)


def _call(ctx, ws=0x100000, kind=0, trunc_n=0, text_bytes=4096, cap=0, reserved=0, report=0x200000, hists=None, flags=0, src=True):
    s = capi.FastqReportSource(ws, kind, trunc_n, text_bytes, cap, reserved)
    return capi.lib().sk_trim_fastq_report_device_async(ctx, C.byref(s) if src else None, report,
                                                        C.byref(hists) if hists is not None else None, flags, None)


def test_argument_checks_without_device():
    """SK_EINVAL before anything touches a device: the context is a zeroed block that only takes the error text."""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    E = capi.SK_EINVAL
    H = capi.FastqReportHists
    A = 0x300000

    def bad(word, **kw):
        assert _call(ctx, **kw) == E, kw
        assert word in L.sk_last_error(ctx), (kw, L.sk_last_error(ctx))

    assert L.sk_trim_fastq_report_device_async(None, None, None, None, 0, None) == E
    bad(b"required", src=False)
    bad(b"required", ws=None)
    bad(b"required", report=None)
    bad(b"16-byte", ws=0x100008)
    bad(b"8-byte", report=0x200004)
    bad(b"kind", kind=4)
    bad(b"kind", kind=0xffffffff)
    bad(b"reserved", reserved=1)
    bad(b"flags", flags=2)
    bad(b"flags", flags=-1)
    # bins of 0 with an array given
    bad(b"len_bins", hists=H(A, None, 0, None, None, None, None, 0))
    bad(b"len_bins", hists=H(None, A, 0, A, A, A, A, 8))
    for j in range(4):
        arrays = [A if i == j else None for i in range(4)]
        bad(b"pos_bins", hists=H(None, None, 0, *arrays, 0))
    # bins above the limits, with or without an array
    bad(b"len_bins", hists=H(A, A, capi.SK_FQ_REPORT_MAX_LEN_BINS + 1, None, None, None, None, 0))
    bad(b"pos_bins", hists=H(None, None, 0, A, A, A, A, capi.SK_FQ_REPORT_MAX_POS_BINS + 1))
    bad(b"pos_bins", hists=H(None, None, 0, None, None, None, None, 1 << 40))
    # an array that is not 8-byte aligned: each of the six
    for j in range(6):
        p = [A + 4 if i == j else A for i in range(6)]
        bad(b"8-byte", hists=H(p[0], p[1], 8, p[2], p[3], p[4], p[5], 8))


def test_summary_text():
    """capi.summary_text: the reference's lines, byte for byte (reference src/trim_paired.cpp:468-475, trim_single.cpp:347)"""
    r = {"kept": 7, "discarded": 3, "pairs": [2, 17, 5, 1233]}
    assert capi.summary_text(r, "se") == "FastQ records kept: 7\nFastQ records discarded: 3\n\n"
    assert capi.summary_text(r, "pe_split") == (
        "\nFastQ paired records kept: 2466 (1233 pairs)\nFastQ single records kept: 22 (from PE1: 17, from PE2: 5)\n"
        "FastQ paired records discarded: 4 (2 pairs)\nFastQ single records discarded: 22 (from PE1: 5, from PE2: 17)\n\n")
    inter = ("\nFastQ paired records kept: 2466 (1233 pairs)\nFastQ single records kept: 22\n"
             "FastQ paired records discarded: 4 (2 pairs)\nFastQ single records discarded: 22\n\n")
    assert capi.summary_text(r, "pe_interleaved") == inter == capi.summary_text(r, "pe_combo_all")
    rep = capi.FastqReport()
    rep.kept, rep.discarded = 7, 3
    assert capi.summary_text(rep, "se") == capi.summary_text(r, "se")
