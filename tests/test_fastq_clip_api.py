"""sk_trim_fastq_clipped_device_async without a device: the exports, the constants, the struct layouts,
sk_trim_fastq_clip_extra_bytes against its formula and every SK_EINVAL of include/sickle_amd.h before anything touches a
device."""
import ctypes as C
import os
import re

import pytest

from sickle_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "sickle_amd.h")).read()


def _define(name):
    return int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u?\b" % name, HEADER).group(1), 0)


def test_symbols_and_constants():
    L = capi.lib()
    for name in ("sk_trim_fastq_clipped_device_async", "sk_trim_fastq_clip_extra_bytes"):
        assert hasattr(L, name) and name in capi.EXPORTS
    assert re.search(r"\bint sk_trim_fastq_clipped_device_async\(", HEADER)
    assert re.search(r"\bsize_t sk_trim_fastq_clip_extra_bytes\(uint64_t text_bytes\);", HEADER)
    assert capi.SK_FQ_CLIP_RESET == _define("SK_FQ_CLIP_RESET") == 1
    assert capi.SK_FQ_CLIP_NONE == _define("SK_FQ_CLIP_NONE") == 0xFFFFFFFF
    assert hasattr(capi.Context, "trim_fastq_clipped_device_async") and callable(capi.fastq_clip_extra_bytes)


def test_abi_version_stays():
    assert capi.lib().sk_abi_version() == 2 and _define("SK_ABI_VERSION") == 2


def _members(struct):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, HEADER).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return body, re.findall(r"\*?(\w+)((?:\[\d+\])*)\s*[,;]", body)


def test_stats_layout():
    """the header's struct, member by member, against the ctypes one: 16 words, 128 bytes of uint64_t"""
    S = capi.FastqClipStats
    assert C.sizeof(S) == 128 and capi.CLIP_WORDS == 16
    names = ["calls", "calls_failed", "reads", "reads_clipped", "reads_emptied", "bases_clipped", "hits", "reserved"]
    assert [n for n, _ in S._fields_] == names
    assert [getattr(S, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 112]
    assert S.hits.size == 64 and S.reserved.size == 16
    body, members = _members("sk_fastq_clip_stats")
    assert [m for m, _ in members] == names
    assert {m: n for m, n in members if n} == {"hits": "[8]", "reserved": "[2]"}
    assert "uint64_t" in body and not re.search(r"\b(u?int32_t|int|void)\b", body)
    d = S().as_dict()
    assert set(d) == set(names) - {"reserved"} and d["hits"] == [0] * 8


def test_clip_layout():
    K = capi.FastqClip
    names = ["set", "lengths", "piece", "order", "state_in", "state_out", "stats_dev", "clip_words_dev", "flags", "reserved"]
    assert [n for n, _ in K._fields_] == names and C.sizeof(K) == 72
    assert [getattr(K, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68]
    body, members = _members("sk_fastq_clip")
    assert [m for m, _ in members] == names
    assert re.search(r"const sk_fastq_adapter_set \*set;", body) and re.search(r"const uint32_t \*\*clip_words_dev;", body)
    assert re.search(r"sk_fastq_clip_stats \*stats_dev;", body) and re.search(r"uint32_t flags, reserved;", body)
    assert re.search(r"const sk_fastq_order_state \*state_in;", body) and re.search(r"\bsk_fastq_order_state \*state_out;", body)


@pytest.mark.parametrize("T", [0, 1, 13, 14, 15, 16, 29, 30, 31, 1000, 65536, (1 << 20) + 7, (1 << 32) - 1])
def test_extra_bytes_formula(T):
    """a 128-byte stats block plus 4 * (2H + 2) bytes of clip words, rounded up to 16, H as in the header's formula"""
    H = (T + 2) // 16
    want = (128 + 4 * (2 * H + 2) + 15) // 16 * 16
    assert capi.lib().sk_trim_fastq_clip_extra_bytes(T) == want == capi.fastq_clip_extra_bytes(T)
    assert want % 16 == 0 and want >= 128 + 8


def test_clip_words_cover_the_packed_reads():
    """the section holds a word for every read the packed batch can hold: (b + 1) / 8 records a text"""
    for b0 in list(range(0, 200)) + [4095, 4096, 65535]:
        for b1 in (0, b0, b0 + 9):
            words = (capi.lib().sk_trim_fastq_clip_extra_bytes(b0 + b1) - 128) // 4
            assert words >= (b0 + 1) // 8 + (b1 + 1) // 8


GOOD = dict(seqs=["AGATCGGAAGAGC"], min_overlap=3, max_mismatch_permille=100)
T = 4096


def _ws_need(order_cap=None, piece=False):
    L = capi.lib()
    if order_cap is None:
        base = L.sk_trim_fastq_workspace_bytes(T, 0)
    elif piece:
        base = L.sk_trim_fastq_ordered_piece_workspace_bytes(T, 0, order_cap)
    else:
        base = L.sk_trim_fastq_ordered_workspace_bytes(T, 0, order_cap)
    return base + L.sk_trim_fastq_clip_extra_bytes(T)


def _call(ctx, st=GOOD, patch=None, clip=True, params=True, inp=True, outs=True, mode=0, texts=(0x400000, None),
          bounds=(T, 0), ws=0x100000, ws_bytes=None, stats=0x200000, flags=0, reserved=0, lengths=None, piece=None,
          order=None, state_in=None, state_out=None, q=20, out_text=None):
    keep = []
    a = capi.adapter_set(**st) if st is not None else None
    if patch:
        patch(a)
    k = capi.FastqClip()
    k.set = C.pointer(a) if a is not None else None
    if lengths is not None:
        keep.append(capi._fastq_lengths(*lengths))
        k.lengths = C.addressof(keep[-1])
    if piece is not None:
        keep.append(capi.FastqPiece((C.c_void_p * 2)(*piece[0]), piece[1], piece[2]))
        k.piece = C.addressof(keep[-1])
    cap = None
    if order is not None:
        keep.append(capi.FastqOrder(*order))
        k.order = C.addressof(keep[-1])
        cap = order[3]
    k.state_in, k.state_out, k.stats_dev, k.flags, k.reserved = state_in, state_out, stats, flags, reserved
    words = C.c_void_p()
    k.clip_words_dev = C.pointer(words)
    p = capi.make_params("sanger", q, 20)
    i = capi.FastqInput((C.c_void_p * 2)(*texts), (C.c_uint64 * 2)(*bounds), 0)
    o = (capi.FastqOutput * 3)()
    if out_text is not None:
        o[0].text = out_text
    if ws_bytes is None:
        ws_bytes = _ws_need(cap, state_out is not None)
    return capi.lib().sk_trim_fastq_clipped_device_async(ctx, C.byref(p) if params else None, C.byref(i) if inp else None,
                                                         C.byref(k) if clip else None, mode, o if outs else None, ws, ws_bytes,
                                                         None)


def test_argument_checks_without_device():
    """SK_EINVAL before anything touches a device: the context is a zeroed block that only takes the error text."""
    L = capi.lib()
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    E = capi.SK_EINVAL

    def bad(word, **kw):
        assert _call(ctx, **kw) == E, kw
        assert word in L.sk_last_error(ctx), (kw, L.sk_last_error(ctx))

    assert L.sk_trim_fastq_clipped_device_async(None, None, None, None, 0, None, None, 0, None) == E
    # the clip's own
    bad(b"clip and clip->set are required", clip=False)
    bad(b"clip and clip->set are required", st=None)
    bad(b"reserved must be 0", reserved=1)
    bad(b"flags", flags=2)
    bad(b"flags", flags=0x80000000)
    bad(b"stats_dev must be 8-byte", stats=0x200004)
    bad(b"stats_dev must be 8-byte", stats=0x200001)
    # the set, as the adapters' call refuses it
    bad(b"set: n ", st=dict(seqs=[]))
    bad(b"set: n ", patch=lambda a: setattr(a, "n", 9))
    bad(b"set: reserved", patch=lambda a: setattr(a, "reserved", 1))
    bad(b"set: every len", st=dict(seqs=["ACGT", ""], min_overlap=1))
    bad(b"set: every len", patch=lambda a: a.len.__setitem__(0, 65))
    bad(b"set: min_overlap must be at least", st=dict(GOOD, min_overlap=0))
    bad(b"set: min_overlap must not exceed", st=dict(GOOD, min_overlap=14))
    bad(b"set: max_mismatch_permille", st=dict(GOOD, max_mismatch_permille=501))
    for letter in ("N", "n", "U", "\r", " "):
        bad(b"set: seq bytes", st=dict(seqs=["ACG" + letter + "ACGT"]))
    # the workspace: the kind's size plus the extra, for every kind
    order, states = (4, 0, 64, 8, 0), dict(state_in=0x600000, state_out=0x600040)
    pc = ((None, None), 0, 0)
    for kind in (dict(), dict(lengths=((), ())), dict(piece=pc), dict(order=order), dict(order=order, piece=pc, **states)):
        cap = order[3] if "order" in kind else None
        need = _ws_need(cap, "state_out" in kind)
        bad(b"workspace must be 16-byte aligned and hold", ws_bytes=need - 1, **kind)
        bad(b"sk_trim_fastq_clip_extra_bytes", ws_bytes=need - L.sk_trim_fastq_clip_extra_bytes(T), **kind)  # the kind's own size
        bad(b"workspace must be 16-byte aligned and hold", ws=0x100008, **kind)
        bad(b"workspace must be 16-byte aligned and hold", ws=None, **kind)
    # what the kinds refuse
    bad(b"required", params=False)
    bad(b"required", inp=False)
    bad(b"required", outs=False)
    bad(b"mode", mode=4)
    bad(b"mode", mode=-1)
    bad(b"text[1]", mode=capi.SK_TRIM_PE_SPLIT)
    bad(b"text[1]", texts=(0x400000, 0x500000), bounds=(T, T))
    bad(b"text[0]", texts=(None, None))
    bad(b"out[0].text must be 16-byte", out_text=0x700008)
    bad(b"bytes_dev and valid_dev must be 8-byte", lengths=((0x800004,), ()))
    bad(b"bytes_dev[1]", lengths=((0x800000, 0x800008), ()))
    bad(b"piece->reserved", piece=((None, None), 0, 1))
    bad(b"start_dev must be 8-byte", piece=((0x800004, None), 0, 0))
    bad(b"start_dev[1]", piece=((0x800000, 0x800008), 0, 0))
    bad(b"order needs", order=(0, 0, 64, 8, 0))
    bad(b"order needs", order=(4, 0, 19, 8, 0))
    bad(b"order needs", order=(4, 0, 64, 0, 0))
    bad(b"order needs", order=(4, 1, 64, 8, 0))
    # the members name the kind: state_out needs both piece and order, and piece with order needs state_out
    bad(b"an ordered piece needs piece, order and state_out", state_out=0x600040)
    bad(b"an ordered piece needs piece, order and state_out", state_out=0x600040, piece=pc)
    bad(b"an ordered piece needs piece, order and state_out", state_out=0x600040, order=order)
    bad(b"an ordered piece needs piece, order and state_out", state_in=0x600000, piece=pc, order=order)
    bad(b"an ordered piece needs piece, order and state_out", piece=pc, order=order)
    bad(b"state_in and state_out must be 8-byte aligned and differ", order=order, piece=pc, state_in=0x600040, state_out=0x600040)
    bad(b"state_in and state_out must be 8-byte aligned and differ", order=order, piece=pc, state_in=None, state_out=0x600044)
    # the scan's parameters, before anything is enqueued
    assert _call(ctx, q=-1) == E


def test_buffers_refuse_what_they_cannot_hold():
    with pytest.raises(ValueError):
        capi._ClipBuffers({"seqs": ["ACGT"], "pos_bins": 4}, "cpu")
    with pytest.raises(ValueError):
        capi._ClipBuffers({"min_overlap": 4}, "cpu")
    with pytest.raises(ValueError):
        capi._ClipBuffers(True, "cpu")
    with pytest.raises(ValueError):
        capi._ClipBuffers({"seqs": ["ACGT"], "clip": True}, "cpu")  # the drivers that do not hand the words out
    b = capi._ClipBuffers({"seqs": ["ACGT"], "clip": True}, "cpu", clip_ok=True)
    assert b.buf.numel() == 16 and b.reset and b.want_clip and b.read()["hits"] == [0] * 8
