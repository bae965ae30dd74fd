"""sk_trim_fastq_adapters_device_async without a device: the export, the constants, the three struct layouts and every
SK_EINVAL of include/sickle_amd.h before anything touches a device."""
import ctypes as C
import os
import re

import pytest

from sickle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sickle_amd.h")).read()


def _define(name):
    return int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, HEADER).group(1), 0)


def test_symbol_and_constants():
    L = capi.lib()
    assert hasattr(L, "sk_trim_fastq_adapters_device_async")
    assert "sk_trim_fastq_adapters_device_async" in capi.EXPORTS
    assert re.search(r"\bint sk_trim_fastq_adapters_device_async\(", HEADER)
    assert capi.SK_FQ_ADAPTERS_RESET == _define("SK_FQ_ADAPTERS_RESET") == 1
    assert capi.SK_FQ_ADAPTERS_MAX == _define("SK_FQ_ADAPTERS_MAX") == 8
    assert capi.SK_FQ_ADAPTER_MAX_LEN == _define("SK_FQ_ADAPTER_MAX_LEN") == 64
    assert capi.SK_FQ_ADAPTERS_MAX_POS_BINS == _define("SK_FQ_ADAPTERS_MAX_POS_BINS") == 2048
    assert capi.SK_FQ_ADAPTERS_OVERLAP_BINS == _define("SK_FQ_ADAPTERS_OVERLAP_BINS") == 65
    assert capi.SK_FQ_CLIP_NONE == _define("SK_FQ_CLIP_NONE") == 0xFFFFFFFF


def test_abi_version_stays():
    assert capi.lib().sk_abi_version() == 2


def _members(struct):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return body, re.findall(r"\*?(\w+)((?:\[\d+\])*)\s*[,;]", body)


def test_struct_layout():
    """the header's struct, member by member, against the ctypes one: 24 words, 192 bytes of uint64_t"""
    A = capi.FastqAdapters
    assert C.sizeof(A) == 192 and capi.ADAPTERS_WORDS == 24
    names = ["calls", "calls_failed", "reads", "kept", "reads_hit", "reads_hit_kept", "hits", "hits_full", "hits_at_0",
             "mismatches", "bases_behind", "reads_hit_out", "bases_hit_out", "pairs_both", "pairs_one", "pairs_same_clip",
             "reserved"]
    assert [n for n, _ in A._fields_] == names
    assert [getattr(A, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 112, 120, 128, 136, 144, 152, 160, 168, 176, 184]
    assert A.hits.size == 64 and A.reserved.size == 8
    body, members = _members("sk_fastq_adapters")
    assert [m for m, _ in members] == names
    assert {m: n for m, n in members if n} == {"hits": "[8]"}
    assert "uint64_t" in body and not re.search(r"\b(u?int32_t|int|void)\b", body)
    d = A().as_dict()
    assert set(d) == set(names) - {"reserved"} and d["hits"] == [0] * 8


def test_set_layout():
    S = capi.FastqAdapterSet
    names = ["n", "len", "seq", "min_overlap", "max_mismatch_permille", "reserved"]
    assert [n for n, _ in S._fields_] == names and C.sizeof(S) == 560
    assert [getattr(S, n).offset for n in names] == [0, 4, 36, 548, 552, 556]
    body, members = _members("sk_fastq_adapter_set")
    assert [m for m, _ in members] == names
    assert {m: n for m, n in members if n} == {"len": "[8]", "seq": "[8][64]"}
    assert re.search(r"uint8_t seq\[8\]\[64\];", body) and re.search(r"uint32_t len\[8\];", body)
    st = capi.adapter_set(["ACGT", b"gattaca"], 3, 250)
    assert (st.n, st.min_overlap, st.max_mismatch_permille, st.reserved) == (2, 3, 250, 0)
    assert list(st.len) == [4, 7, 0, 0, 0, 0, 0, 0] and bytes(st.seq[1])[:8] == b"gattaca\0" and bytes(st.seq[0])[:5] == b"ACGT\0"
    with pytest.raises(ValueError):
        capi.adapter_set(["A"] * 9)
    with pytest.raises(ValueError):
        capi.adapter_set(["A" * 65])


def test_out_layout():
    O = capi.FastqAdaptersOut
    names = ["pos", "pos_bins", "overlap", "clip", "clip_capacity"]
    assert [n for n, _ in O._fields_] == names and C.sizeof(O) == 40
    assert [getattr(O, n).offset for n in names] == [0, 8, 16, 24, 32]
    body, members = _members("sk_fastq_adapters_out")
    assert [m for m, _ in members] == names
    assert re.search(r"uint64_t \*pos;", body) and re.search(r"uint64_t pos_bins;", body)
    assert re.search(r"uint64_t \*overlap;", body) and re.search(r"uint32_t \*clip;", body)
    assert re.search(r"uint64_t clip_capacity;", body)


GOOD = dict(seqs=["AGATCGGAAGAGC"], min_overlap=3, max_mismatch_permille=100)


def _call(ctx, ws=0x100000, kind=0, trunc_n=0, text_bytes=4096, cap=0, reserved=0, adapters=0x200000, flags=0, src=True,
          mode=2, texts=(0x400000, None), bounds=(4096, 0), inp=True, out=None, st=GOOD, patch=None):
    s = capi.FastqReportSource(ws, kind, trunc_n, text_bytes, cap, reserved)
    i = capi.FastqInput((C.c_void_p * 2)(*texts), (C.c_uint64 * 2)(*bounds), 0)
    o = capi.FastqAdaptersOut(*out) if out is not None else None
    a = capi.adapter_set(**st) if st is not None else None
    if patch:
        patch(a)
    return capi.lib().sk_trim_fastq_adapters_device_async(ctx, C.byref(s) if src else None, C.byref(i) if inp else None, mode,
                                                          C.byref(a) if a is not None else None, adapters,
                                                          C.byref(o) if o is not None else None, flags, None)


def test_argument_checks_without_device():
    """SK_EINVAL before anything touches a device: the context is a zeroed block that only takes the error text."""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    E = capi.SK_EINVAL

    def bad(word, **kw):
        assert _call(ctx, **kw) == E, kw
        assert word in L.sk_last_error(ctx), (kw, L.sk_last_error(ctx))

    assert L.sk_trim_fastq_adapters_device_async(None, None, None, 0, None, None, None, 0, None) == E
    # the bases' cases
    bad(b"required", src=False)
    bad(b"required", ws=None)
    bad(b"required", adapters=None)
    bad(b"required", inp=False)
    bad(b"required", st=None)
    bad(b"16-byte", ws=0x100008)
    bad(b"adapters_dev must be 8-byte", adapters=0x200004)
    bad(b"kind", kind=4)
    bad(b"kind", kind=0xffffffff)
    bad(b"mode", mode=4)
    bad(b"mode", mode=-1)
    bad(b"flags", flags=2)
    bad(b"flags", flags=-1)
    bad(b"reserved", reserved=1)
    bad(b"text[1]", mode=capi.SK_TRIM_PE_SPLIT)
    for mode in (capi.SK_TRIM_SE, capi.SK_TRIM_PE_INTERLEAVED, capi.TRIM_MODES["pe_combo_all"]):
        bad(b"text[1]", mode=mode, texts=(0x400000, 0x500000), bounds=(4096, 4096))
        bad(b"text[0]", mode=mode, texts=(None, None))
    # the arrays
    bad(b"8-byte", out=(0x300004, 64, None, None, 0))
    bad(b"8-byte", out=(None, 0, 0x300004, None, 0))
    bad(b"pos_bins is 0", out=(0x300000, 0, None, None, 0))
    bad(b"above", out=(0x300000, capi.SK_FQ_ADAPTERS_MAX_POS_BINS + 1, None, None, 0))
    bad(b"above", out=(None, capi.SK_FQ_ADAPTERS_MAX_POS_BINS + 1, None, None, 0))
    bad(b"clip must be 4-byte", out=(None, 0, None, 0x300002, 16))
    bad(b"clip must be 4-byte", out=(None, 0, None, 0x300001, 16))
    bad(b"clip_capacity is 0", out=(None, 0, None, 0x300000, 0))
    # the set
    bad(b"set: n ", st=dict(seqs=[]))
    bad(b"set: n ", patch=lambda a: setattr(a, "n", 9))
    bad(b"set: reserved", patch=lambda a: setattr(a, "reserved", 1))
    bad(b"set: every len", st=dict(seqs=["ACGT", ""], min_overlap=1))
    bad(b"set: every len", patch=lambda a: a.len.__setitem__(0, 65))
    bad(b"set: min_overlap must be at least", st=dict(GOOD, min_overlap=0))
    bad(b"set: min_overlap must not exceed", st=dict(GOOD, min_overlap=14))
    bad(b"set: min_overlap must not exceed", st=dict(seqs=["AGATCGGAAGAGC", "ACG"], min_overlap=4))
    bad(b"set: max_mismatch_permille", st=dict(GOOD, max_mismatch_permille=501))
    for letter in ("N", "n", "U", "R", "\r", " ", "@"):
        bad(b"set: seq bytes", st=dict(seqs=["ACG" + letter + "ACGT"]))
    bad(b"set: seq bytes", st=dict(seqs=[b"ACGT\xc1CGT"]))
    bad(b"set: seq bytes", st=dict(seqs=["ACGT", "ACGTN"], min_overlap=4))


def test_buffers_refuse_what_they_cannot_hold():
    with pytest.raises(ValueError):
        capi._AdaptersBuffers({"seqs": ["ACGT"], "len_bins": 4}, "cpu")
    with pytest.raises(ValueError):
        capi._AdaptersBuffers({"min_overlap": 4}, "cpu")
    with pytest.raises(ValueError):
        capi._AdaptersBuffers(True, "cpu")
    with pytest.raises(ValueError):
        capi._AdaptersBuffers({"seqs": ["ACGT"], "clip": True}, "cpu")  # the drivers that do not know their reads
    b = capi._AdaptersBuffers({"seqs": ["ACGT"], "pos_bins": 5, "overlap": True}, "cpu")
    assert b.buf.numel() == 24 + 40 + 8 * 65 and b.out.pos_bins == 5 and b.out.clip is None
