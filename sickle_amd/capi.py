"""ctypes view of the C ABI in include/sickle_amd.h (libsickle_amd.so, built in-tree by
sickle_amd/csrc/Makefile).  No fallback of any kind: a missing library or a missing gfx950
device raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsickle_amd.so")

SK_OK, SK_ERANGE, SK_EINVAL, SK_ENODEV, SK_EHIP, SK_EBUSY, SK_ESPACE, SK_EFORMAT, SK_EDATA = 0, 1, -1, -2, -3, -4, -5, -6, -7
SK_ELONGLINE = -8  # sk_trim_fastq_ordered_device_finish: a line the reference's reader would split
# why a BGZF image is not valid (sk_bgzf_inflate_device_finish)
SK_GZ_OK, SK_GZ_HEADER, SK_GZ_TRUNCATED, SK_GZ_DEFLATE, SK_GZ_LENGTH, SK_GZ_CRC = range(6)
# why a FASTQ record is malformed (sk_trim_fastq_device_finish), in the order the reference checks
(SK_FQ_OK, SK_FQ_ID_SHORT, SK_FQ_ID_NO_AT, SK_FQ_SEQ_EMPTY, SK_FQ_QUAL_EMPTY, SK_FQ_LENGTHS, SK_FQ_TOO_LONG,
 SK_FQ_PAIR_COUNT) = range(8)
SK_TRIM_SE, SK_TRIM_PE_SPLIT, SK_TRIM_PE_INTERLEAVED, SK_TRIM_PE_COMBO_ALL = 0, 1, 2, 3
# "pe_combo_all" (sickle's -M) is a mode of the FASTQ text calls only
TRIM_MODES = {"se": SK_TRIM_SE, "pe_split": SK_TRIM_PE_SPLIT, "pe_interleaved": SK_TRIM_PE_INTERLEAVED,
              "pe_combo_all": SK_TRIM_PE_COMBO_ALL}
# the outputs each mode uses
TRIM_OUTPUTS = {"se": (0,), "pe_split": (0, 1, 2), "pe_interleaved": (0, 2), "pe_combo_all": (0,)}


def fastq_output_bound(text_bytes, mode):
    """The most bytes one output of a FASTQ text call can need for text_bytes bytes of text, without a look at the text
    (include/sickle_amd.h): the text plus the '\\n' an unterminated last line of each input gains; "pe_combo_all" adds one
    byte per record, since an N record is one byte longer than a 1-base read with an empty '+' line, and a valid record
    has 8 bytes or more (7 for an unterminated last one)."""
    return text_bytes + 2 + ((text_bytes + 1) // 8 if mode == "pe_combo_all" else 0)
QUALTYPES = {"phred": 0, "sanger": 1, "solexa": 2, "illumina": 3}

# every entry point include/sickle_amd.h declares
EXPORTS = ("sk_quality_constants", "sk_typename", "sk_abi_version", "sk_device_count", "sk_create",
           "sk_destroy", "sk_last_error", "sk_device", "sk_host_alloc", "sk_host_free",
           "sk_scan_device_async", "sk_scan_device_finish", "sk_trim_batch", "sk_submit", "sk_wait",
           "sk_kernel_for", "sk_kernel_name", "sk_seg_classes", "sk_probe_read_bandwidth",
           "sk_count_pairs_device_async", "sk_count_pairs_device_finish", "sk_bgzf_deflate", "sk_bgzf_host_alloc", "sk_bgzf_host_free",
           "sk_bgzf_last_error", "sk_trim_workspace_bytes", "sk_trim_device_async", "sk_trim_device_finish",
           "sk_trim_fastq_workspace_bytes", "sk_trim_fastq_device_async", "sk_trim_fastq_device_finish",
           "sk_trim_fastq_output_words", "sk_bgzf_bound", "sk_bgzf_workspace_bytes", "sk_bgzf_workspace_bytes_flags", "sk_bgzf_device_async",
           "sk_bgzf_device_finish", "sk_bgzf_inflate_workspace_bytes", "sk_bgzf_inflate_device_async",
           "sk_bgzf_inflate_device_finish", "sk_gzip_inflate_workspace_bytes", "sk_gzip_inflate_device_async",
           "sk_gzip_inflate_device_finish", "sk_trim_fastq_ordered_workspace_bytes", "sk_trim_fastq_ordered_device_async",
           "sk_trim_fastq_ordered_device_finish", "sk_trim_fastq_ordered_batches",
           "sk_trim_fastq_chained_device_async", "sk_bgzf_inflate_output_words", "sk_gzip_inflate_output_words",
           "sk_scan_counted_device_async", "sk_trim_fastq_piece_device_async", "sk_trim_fastq_piece_words",
           "sk_trim_fastq_piece_device_finish", "sk_fastq_carry_device_async", "sk_gzip_inflate_piece_workspace_bytes",
           "sk_gzip_inflate_piece_device_async", "sk_gzip_inflate_piece_device_finish",
           "sk_trim_fastq_ordered_piece_workspace_bytes", "sk_trim_fastq_ordered_piece_device_async",
           "sk_trim_fastq_ordered_piece_device_finish", "sk_trim_fastq_report_device_async",
           "sk_trim_fastq_audit_device_async", "sk_trim_fastq_bases_device_async",
           "sk_trim_fastq_rejects_workspace_bytes", "sk_trim_fastq_rejects_bound", "sk_trim_fastq_rejects_device_async",
           "sk_trim_fastq_rejects_device_finish", "sk_trim_fastq_rejects_output_words",
           "sk_trim_fastq_adapters_device_async", "sk_trim_fastq_clip_extra_bytes", "sk_trim_fastq_clipped_device_async")
# sk_trim_fastq_adapters_device_async (include/sickle_amd.h)
SK_FQ_ADAPTERS_RESET = 1
SK_FQ_ADAPTERS_MAX = 8
SK_FQ_ADAPTER_MAX_LEN = 64
SK_FQ_ADAPTERS_MAX_POS_BINS = 2048
SK_FQ_ADAPTERS_OVERLAP_BINS = 65
SK_FQ_CLIP_NONE = 0xFFFFFFFF
# sk_trim_fastq_clipped_device_async (include/sickle_amd.h)
SK_FQ_CLIP_RESET = 1
# sk_trim_fastq_rejects_device_async (include/sickle_amd.h)
SK_FQ_REJECTS_PAIRS = 1
# sk_trim_fastq_bases_device_async (include/sickle_amd.h)
SK_FQ_BASES_RESET = 1
SK_FQ_BASES_MAX_POS_BINS = 1024
SK_FQ_BASES_GC_BINS = 101
BASES_CLASSES = ("A", "C", "G", "T", "N", "other")
# sk_trim_fastq_audit_device_async (include/sickle_amd.h)
SK_FQ_AUDIT_RESET = 1
# sk_trim_fastq_report_device_async (include/sickle_amd.h)
SK_FQ_REPORT_RESET = 1
SK_FQ_REPORT_MAX_LEN_BINS = 4096
SK_FQ_REPORT_MAX_POS_BINS = 2048
REPORT_KINDS = {"plain": 0, "piece": 1, "ordered": 2, "ordered_piece": 3}
SK_GZIP_PIECE_STATE_BYTES = 128 + 32768
SK_BGZF_EOF = 1
SK_BGZF_SEARCH = 2


class Params(C.Structure):
    _fields_ = [("qualtype", C.c_int32), ("qual_threshold", C.c_int32), ("length_threshold", C.c_int32),
                ("no_fiveprime", C.c_int32), ("trunc_n", C.c_int32)]


class Err(C.Structure):
    _fields_ = [("read", C.c_uint32), ("pos", C.c_uint32), ("ch", C.c_int32)]


class Tile(C.Structure):
    _fields_ = [("byte_off", C.c_uint64), ("slot0", C.c_uint32), ("stride", C.c_uint32), ("rows", C.c_uint16),
                ("read_len", C.c_uint16), ("reserved", C.c_uint32)]


TILE_DTYPE = np.dtype([("byte_off", "<u8"), ("slot0", "<u4"), ("stride", "<u4"), ("rows", "<u2"), ("read_len", "<u2"),
                       ("reserved", "<u4")])


class Batch(C.Structure):
    _fields_ = [("qual", C.c_void_p), ("seq", C.c_void_p), ("offsets", C.c_void_p), ("stride", C.c_uint32),
                ("read_len", C.c_uint32), ("lengths", C.c_void_p), ("n_reads", C.c_uint64),
                ("tiles", C.c_void_p), ("n_tiles", C.c_uint32), ("out_index", C.c_void_p),
                ("classes", C.c_void_p), ("n_classes", C.c_uint32), ("cuts_in_slot_order", C.c_uint32)]


class SegClass(C.Structure):
    _fields_ = [("first_tile", C.c_uint32), ("n_tiles", C.c_uint32), ("max_stride", C.c_uint32), ("wide", C.c_uint32)]


def seg_classes(tiles, max_classes=16):
    """sk_seg_classes on a numpy TILE_DTYPE array -> (ctypes array, count); count 0 = pass no table."""
    arr = (SegClass * max_classes)()
    n = lib().sk_seg_classes(tiles.ctypes.data, len(tiles), arr, max_classes)
    return arr, n


class PairCounts(C.Structure):
    _fields_ = [("both", C.c_uint64), ("only_first", C.c_uint64), ("only_second", C.c_uint64), ("none", C.c_uint64)]


class TrimOutput(C.Structure):
    _fields_ = [("qual", C.c_void_p), ("seq", C.c_void_p), ("offsets", C.c_void_p), ("read_index", C.c_void_p),
                ("byte_capacity", C.c_uint64), ("record_capacity", C.c_uint64)]


class TrimCounts(C.Structure):
    _fields_ = [("records", C.c_uint64 * 3), ("bytes", C.c_uint64 * 3), ("bad_read", C.c_uint64)]

    def as_dict(self):
        return {"records": list(self.records), "bytes": list(self.bytes), "bad_read": int(self.bad_read)}


class FastqInput(C.Structure):
    _fields_ = [("text", C.c_void_p * 2), ("bytes", C.c_uint64 * 2), ("max_read_len", C.c_uint32)]


class FastqLengths(C.Structure):
    _fields_ = [("bytes_dev", C.c_void_p * 2), ("valid_dev", C.c_void_p * 2)]


class FastqOutput(C.Structure):
    _fields_ = [("text", C.c_void_p), ("capacity", C.c_uint64), ("record_index", C.c_void_p),
                ("record_capacity", C.c_uint64)]


class FastqCounts(C.Structure):
    _fields_ = [("records_in", C.c_uint64 * 2), ("tail_lines", C.c_uint64 * 2), ("dropped_unpaired", C.c_uint64),
                ("records", C.c_uint64 * 3), ("bytes", C.c_uint64 * 3), ("format_error", C.c_int32),
                ("format_input", C.c_uint32), ("format_record", C.c_uint64), ("range", Err)]

    def as_dict(self):
        return {"records_in": list(self.records_in), "tail_lines": list(self.tail_lines),
                "dropped_unpaired": int(self.dropped_unpaired), "records": list(self.records),
                "bytes": list(self.bytes), "format_error": int(self.format_error),
                "format_input": int(self.format_input), "format_record": int(self.format_record),
                "range": (int(self.range.read), int(self.range.pos), int(self.range.ch))}


class FastqReport(C.Structure):
    """sk_fastq_report: every member is a uint64_t"""
    _fields_ = [("calls", C.c_uint64), ("calls_failed", C.c_uint64), ("reads", C.c_uint64), ("kept", C.c_uint64),
                ("discarded", C.c_uint64), ("pairs", C.c_uint64 * 4), ("bases_in", C.c_uint64), ("bases_out", C.c_uint64),
                ("bases_cut5", C.c_uint64), ("bases_cut3", C.c_uint64), ("bases_discarded", C.c_uint64),
                ("reads_cut5", C.c_uint64), ("reads_cut3", C.c_uint64), ("max_len_in", C.c_uint64),
                ("max_len_out", C.c_uint64)]

    def as_dict(self):
        return {name: (list(getattr(self, name)) if name == "pairs" else int(getattr(self, name))) for name, _ in self._fields_}


REPORT_WORDS = C.sizeof(FastqReport) // 8
HIST_ARRAYS = ("len_in", "len_out", "qsum_in", "qcnt_in", "qsum_out", "qcnt_out")


class FastqReportSource(C.Structure):
    _fields_ = [("workspace", C.c_void_p), ("kind", C.c_uint32), ("trunc_n", C.c_int32), ("text_bytes", C.c_uint64),
                ("batch_capacity", C.c_uint64), ("reserved", C.c_uint64)]


class FastqReportHists(C.Structure):
    _fields_ = [("len_in", C.c_void_p), ("len_out", C.c_void_p), ("len_bins", C.c_uint64), ("qsum_in", C.c_void_p),
                ("qcnt_in", C.c_void_p), ("qsum_out", C.c_void_p), ("qcnt_out", C.c_void_p), ("pos_bins", C.c_uint64)]


def summary_text(report, mode):
    """The kept / discarded lines the reference prints at the end of a run (reference src/trim_paired.cpp:468-475,
    src/trim_single.cpp:347), byte for byte, from a report (a dict as the drivers return it, or a FastqReport).  mode
    "se": "FastQ records kept: ..\nFastQ records discarded: ..\n\n".  The pair modes: from "\nFastQ paired records
    kept" through the "single records discarded" line, in the interleaved wording when the input is one text
    ("pe_interleaved", "pe_combo_all") and with "from PE1 / from PE2" for "pe_split".  The reference's "Total input
    FastQ records" line is left out: it is not a property of the text."""
    r = report.as_dict() if isinstance(report, FastqReport) else report
    if mode == "se":
        return "FastQ records kept: %d\nFastQ records discarded: %d\n\n" % (r["kept"], r["discarded"])
    if mode not in TRIM_MODES:
        raise ValueError("summary_text: unknown mode %r" % (mode,))
    p = r["pairs"]
    kept_p, discard_p, s1, s2 = 2 * p[3], 2 * p[0], p[1], p[2]  # kept_s1 = discard_s2 = pairs[1], kept_s2 = discard_s1 = pairs[2]
    text = "\nFastQ paired records kept: %d (%d pairs)\n" % (kept_p, kept_p // 2)
    if mode == "pe_split":
        text += "FastQ single records kept: %d (from PE1: %d, from PE2: %d)\n" % (s1 + s2, s1, s2)
    else:
        text += "FastQ single records kept: %d\n" % (s1 + s2)
    text += "FastQ paired records discarded: %d (%d pairs)\n" % (discard_p, discard_p // 2)
    if mode == "pe_split":
        text += "FastQ single records discarded: %d (from PE1: %d, from PE2: %d)\n\n" % (s1 + s2, s2, s1)
    else:
        text += "FastQ single records discarded: %d\n\n" % (s1 + s2)
    return text


class _ReportBuffers:
    """The device words of one report= of a driver: the sk_fastq_report, then the histograms report=dict(len_bins=..,
    pos_bins=..) asks for (all six arrays of the bins given), in one tensor."""

    def __init__(self, report, dev):
        import torch
        opts = report if isinstance(report, dict) else {}
        unknown = set(opts) - {"len_bins", "pos_bins"}
        if unknown:
            raise ValueError("report: unknown keys %r" % sorted(unknown))
        self.len_bins, self.pos_bins = int(opts.get("len_bins", 0)), int(opts.get("pos_bins", 0))
        self.buf = torch.empty(REPORT_WORDS + 2 * self.len_bins + 4 * self.pos_bins, dtype=torch.int64, device=dev)
        self.ptr = self.buf.data_ptr()
        self.hists = None
        if self.len_bins or self.pos_bins:
            at = lambda words: self.ptr + 8 * (REPORT_WORDS + words)
            L, P = self.len_bins, self.pos_bins
            self.hists = FastqReportHists(at(0) if L else None, at(L) if L else None, L,
                                          *[at(2 * L + j * P) if P else None for j in range(4)], P)

    def read(self):
        """-> the report as a dict: sk_fastq_report's members, and a uint64 array per histogram asked for"""
        w = self.buf.cpu().numpy().view(np.uint64)
        rep = FastqReport.from_buffer_copy(w[:REPORT_WORDS].tobytes()).as_dict()
        at, L, P = REPORT_WORDS, self.len_bins, self.pos_bins
        for name in HIST_ARRAYS:
            n = L if name.startswith("len") else P
            if n:
                rep[name] = w[at:at + n].copy()
            at += n
        return rep


class FastqAudit(C.Structure):
    """sk_fastq_audit: every member is a uint64_t"""
    _fields_ = [("calls", C.c_uint64), ("calls_failed", C.c_uint64), ("pairs", C.c_uint64), ("name_mismatch", C.c_uint64),
                ("first_mismatch", C.c_uint64), ("tags_swapped", C.c_uint64), ("qual_bytes", C.c_uint64),
                ("qual_min", C.c_uint64), ("qual_max", C.c_uint64), ("reserved", C.c_uint64 * 7)]

    def as_dict(self):
        """the members but `reserved`, as ints"""
        return {name: int(getattr(self, name)) for name, _ in self._fields_ if name != "reserved"}


AUDIT_WORDS = C.sizeof(FastqAudit) // 8
AUDIT_NONE = (1 << 64) - 1  # first_mismatch without a mismatch, qual_min without a byte


def qualtypes_consistent(audit):
    """The names among "sanger", "solexa" and "illumina" whose quality range (sk_quality_constants: [min, max] as bytes)
    contains the audit's [qual_min, qual_max]; all three when it saw no quality byte.  audit: a dict as the drivers
    return it, or a FastqAudit.  Bytes that fit "illumina" in a run made with -t sanger are the sign of an offset-64
    (CASAVA 1.3-1.7) file, which that run trimmed as if every quality were 31 higher."""
    a = audit.as_dict() if isinstance(audit, FastqAudit) else audit
    names = ("sanger", "solexa", "illumina")
    if a["qual_bytes"] == 0:
        return list(names)
    out = []
    for name in names:
        k = lib().sk_quality_constants(QUALTYPES[name])  # {offset, min, max}
        if k[1] <= a["qual_min"] and a["qual_max"] <= k[2]:
            out.append(name)
    return out


class _AuditBuffers:
    """The device words of one audit=True of a driver: the sk_fastq_audit, then the 256 histogram words, in one tensor."""

    def __init__(self, dev):
        import torch
        self.buf = torch.empty(AUDIT_WORDS + 256, dtype=torch.int64, device=dev)
        self.ptr = self.buf.data_ptr()
        self.hist_ptr = self.ptr + 8 * AUDIT_WORDS

    def read(self):
        """-> the audit as a dict: sk_fastq_audit's members but `reserved`, and qual_hist as 256 ints"""
        w = self.buf.cpu().numpy().view(np.uint64)
        a = FastqAudit.from_buffer_copy(w[:AUDIT_WORDS].tobytes()).as_dict()
        a["qual_hist"] = [int(x) for x in w[AUDIT_WORDS:]]
        return a


class FastqBases(C.Structure):
    """sk_fastq_bases: every member is a uint64_t"""
    _fields_ = [("calls", C.c_uint64), ("calls_failed", C.c_uint64), ("reads", C.c_uint64), ("kept", C.c_uint64),
                ("bases_in", C.c_uint64 * 6), ("bases_out", C.c_uint64 * 6), ("lower_in", C.c_uint64),
                ("lower_out", C.c_uint64), ("reads_n_in", C.c_uint64), ("reads_n_out", C.c_uint64),
                ("gc_none_in", C.c_uint64), ("gc_none_out", C.c_uint64), ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        """the members but `reserved`, as ints; bases_in and bases_out as lists of six, in the order of BASES_CLASSES"""
        return {name: (list(getattr(self, name)) if name.startswith("bases") else int(getattr(self, name)))
                for name, _ in self._fields_ if name != "reserved"}


BASES_WORDS = C.sizeof(FastqBases) // 8


class FastqBasesHists(C.Structure):
    _fields_ = [("pos_in", C.c_void_p), ("pos_out", C.c_void_p), ("pos_bins", C.c_uint64), ("gc_in", C.c_void_p),
                ("gc_out", C.c_void_p)]


class _BasesBuffers:
    """The device words of one bases= of a driver: the sk_fastq_bases, then the arrays bases=dict(pos_bins=.., gc=True)
    asks for (both position tables of the bins given, both GC histograms), in one tensor."""

    def __init__(self, bases, dev):
        import torch
        opts = bases if isinstance(bases, dict) else {}
        unknown = set(opts) - {"pos_bins", "gc"}
        if unknown:
            raise ValueError("bases: unknown keys %r" % sorted(unknown))
        self.pos_bins, self.gc = int(opts.get("pos_bins", 0)), bool(opts.get("gc", False))
        G = SK_FQ_BASES_GC_BINS if self.gc else 0
        self.buf = torch.empty(BASES_WORDS + 12 * self.pos_bins + 2 * G, dtype=torch.int64, device=dev)
        self.ptr = self.buf.data_ptr()
        self.hists = None
        if self.pos_bins or G:
            at = lambda words: self.ptr + 8 * (BASES_WORDS + words)
            P = self.pos_bins
            self.hists = FastqBasesHists(at(0) if P else None, at(6 * P) if P else None, P, at(12 * P) if G else None,
                                         at(12 * P + G) if G else None)

    def read(self):
        """-> the bases as a dict: sk_fastq_bases's members but `reserved`; pos_in and pos_out as uint64 arrays of shape
        (6, pos_bins), gc_in and gc_out of 101, where asked for"""
        w = self.buf.cpu().numpy().view(np.uint64)
        b = FastqBases.from_buffer_copy(w[:BASES_WORDS].tobytes()).as_dict()
        at, P = BASES_WORDS, self.pos_bins
        if P:
            b["pos_in"], b["pos_out"] = w[at:at + 6 * P].reshape(6, P).copy(), w[at + 6 * P:at + 12 * P].reshape(6, P).copy()
        at += 12 * P
        if self.gc:
            G = SK_FQ_BASES_GC_BINS
            b["gc_in"], b["gc_out"] = w[at:at + G].copy(), w[at + G:at + 2 * G].copy()
        return b


class FastqAdapterSet(C.Structure):
    """sk_fastq_adapter_set (host memory)"""
    _fields_ = [("n", C.c_uint32), ("len", C.c_uint32 * 8), ("seq", (C.c_uint8 * 64) * 8), ("min_overlap", C.c_uint32),
                ("max_mismatch_permille", C.c_uint32), ("reserved", C.c_uint32)]


def adapter_set(seqs, min_overlap=3, max_mismatch_permille=100):
    """-> the FastqAdapterSet of up to eight adapter sequences (str or bytes).  Only what the struct cannot hold is
    refused here (ValueError); everything else is the call's to refuse (SK_EINVAL)."""
    seqs = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in seqs]
    if len(seqs) > SK_FQ_ADAPTERS_MAX or any(len(s) > SK_FQ_ADAPTER_MAX_LEN for s in seqs):
        raise ValueError("adapters: at most %d sequences of at most %d bases" % (SK_FQ_ADAPTERS_MAX, SK_FQ_ADAPTER_MAX_LEN))
    st = FastqAdapterSet()
    st.n, st.min_overlap, st.max_mismatch_permille = len(seqs), int(min_overlap), int(max_mismatch_permille)
    for a, s in enumerate(seqs):
        st.len[a] = len(s)
        for j, b in enumerate(s):
            st.seq[a][j] = b
    return st


class FastqAdapters(C.Structure):
    """sk_fastq_adapters: every member is a uint64_t"""
    _fields_ = [("calls", C.c_uint64), ("calls_failed", C.c_uint64), ("reads", C.c_uint64), ("kept", C.c_uint64),
                ("reads_hit", C.c_uint64), ("reads_hit_kept", C.c_uint64), ("hits", C.c_uint64 * 8),
                ("hits_full", C.c_uint64), ("hits_at_0", C.c_uint64), ("mismatches", C.c_uint64),
                ("bases_behind", C.c_uint64), ("reads_hit_out", C.c_uint64), ("bases_hit_out", C.c_uint64),
                ("pairs_both", C.c_uint64), ("pairs_one", C.c_uint64), ("pairs_same_clip", C.c_uint64),
                ("reserved", C.c_uint64)]

    def as_dict(self):
        """the members but `reserved`, as ints; hits as a list of eight"""
        return {name: (list(getattr(self, name)) if name == "hits" else int(getattr(self, name)))
                for name, _ in self._fields_ if name != "reserved"}


ADAPTERS_WORDS = C.sizeof(FastqAdapters) // 8


class FastqAdaptersOut(C.Structure):
    """sk_fastq_adapters_out"""
    _fields_ = [("pos", C.c_void_p), ("pos_bins", C.c_uint64), ("overlap", C.c_void_p), ("clip", C.c_void_p),
                ("clip_capacity", C.c_uint64)]


def _decode_clip_words(words):
    """clip words (an int32 tensor, a word per read) -> (clip, adapter): int64 tensors with the start per read and the
    adapter's number, each -1 where the word is SK_FQ_CLIP_NONE"""
    import torch
    words = words.to(torch.int64) & 0xFFFFFFFF
    none = words == SK_FQ_CLIP_NONE
    return (torch.where(none, torch.full_like(words, -1), words & 0xFFFFFF),
            torch.where(none, torch.full_like(words, -1), words >> 24))


class _AdaptersBuffers:
    """The set and the device words of one adapters=dict(seqs=[..], min_overlap=3, max_mismatch_permille=100,
    pos_bins=None, overlap=False, clip=False) of a driver: the sk_fastq_adapters, then pos and overlap where asked for, in
    one tensor; the clip words are a tensor of their own, which only a driver that knows its reads gives (with_clip)."""

    def __init__(self, adapters, dev, clip_ok=False):
        import torch
        if not isinstance(adapters, dict) or "seqs" not in adapters:
            raise ValueError("adapters: a dict with seqs=[...]")
        unknown = set(adapters) - {"seqs", "min_overlap", "max_mismatch_permille", "pos_bins", "overlap", "clip"}
        if unknown:
            raise ValueError("adapters: unknown keys %r" % sorted(unknown))
        self.set = adapter_set(adapters["seqs"], adapters.get("min_overlap", 3), adapters.get("max_mismatch_permille", 100))
        self.pos_bins, self.overlap = int(adapters.get("pos_bins") or 0), bool(adapters.get("overlap", False))
        self.want_clip = bool(adapters.get("clip", False))
        if self.want_clip and not clip_ok:
            raise ValueError("adapters: clip=True is trim_fastq's alone")
        V = 8 * SK_FQ_ADAPTERS_OVERLAP_BINS if self.overlap else 0
        self.buf = torch.empty(ADAPTERS_WORDS + 8 * self.pos_bins + V, dtype=torch.int64, device=dev)
        self.ptr, self.dev, self.clip = self.buf.data_ptr(), dev, None
        self._out()

    def _out(self):
        at = lambda words: self.ptr + 8 * (ADAPTERS_WORDS + words)
        P = self.pos_bins
        self.out = None
        if P or self.overlap or self.clip is not None:
            self.out = FastqAdaptersOut(at(0) if P else None, P, at(8 * P) if self.overlap else None,
                                        self.clip.data_ptr() if self.clip is not None else None,
                                        self.clip.numel() if self.clip is not None else 0)

    def with_clip(self, reads):
        """a clip word per read of a call of at most `reads` reads"""
        import torch
        self.clip = torch.empty(max(int(reads), 1), dtype=torch.int32, device=self.dev)
        self._out()

    def read(self):
        """-> the adapters as a dict: sk_fastq_adapters's members but `reserved`; pos as a uint64 array of shape
        (8, pos_bins) and overlap of shape (8, 65), where asked for; with clip words: clip, an int64 tensor with the start
        per read (-1: no hit), and adapter, an int64 tensor with the adapter's number (-1: no hit)"""
        w = self.buf.cpu().numpy().view(np.uint64)
        d = FastqAdapters.from_buffer_copy(w[:ADAPTERS_WORDS].tobytes()).as_dict()
        at, P = ADAPTERS_WORDS, self.pos_bins
        if P:
            d["pos"] = w[at:at + 8 * P].reshape(8, P).copy()
        at += 8 * P
        if self.overlap:
            d["overlap"] = w[at:at + 8 * SK_FQ_ADAPTERS_OVERLAP_BINS].reshape(8, SK_FQ_ADAPTERS_OVERLAP_BINS).copy()
        if self.clip is not None:
            d["clip"], d["adapter"] = _decode_clip_words(self.clip[:d["reads"]])
        return d


class FastqClipStats(C.Structure):
    """sk_fastq_clip_stats: every member is a uint64_t"""
    _fields_ = [("calls", C.c_uint64), ("calls_failed", C.c_uint64), ("reads", C.c_uint64), ("reads_clipped", C.c_uint64),
                ("reads_emptied", C.c_uint64), ("bases_clipped", C.c_uint64), ("hits", C.c_uint64 * 8),
                ("reserved", C.c_uint64 * 2)]

    def as_dict(self):
        """the members but `reserved`, as ints; hits as a list of eight"""
        return {name: (list(getattr(self, name)) if name == "hits" else int(getattr(self, name)))
                for name, _ in self._fields_ if name != "reserved"}


CLIP_WORDS = C.sizeof(FastqClipStats) // 8


class FastqClip(C.Structure):
    """sk_fastq_clip"""
    _fields_ = [("set", C.POINTER(FastqAdapterSet)), ("lengths", C.c_void_p), ("piece", C.c_void_p), ("order", C.c_void_p),
                ("state_in", C.c_void_p), ("state_out", C.c_void_p), ("stats_dev", C.c_void_p),
                ("clip_words_dev", C.POINTER(C.c_void_p)), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


def fastq_clip_extra_bytes(text_bytes):
    """sk_trim_fastq_clip_extra_bytes: what a clipped call's workspace holds behind its kind's own"""
    return lib().sk_trim_fastq_clip_extra_bytes(text_bytes)


class _ClipBuffers:
    """The set and the device words of one clip_adapters=dict(seqs=[..], min_overlap=3, max_mismatch_permille=100,
    clip=False) of a driver: a sk_fastq_clip_stats, which the driver's clipped calls add to.  reset: whether the next call
    zeroes it first (the drivers set it in front of each call)."""

    def __init__(self, clip_adapters, dev, clip_ok=False):
        import torch
        if not isinstance(clip_adapters, dict) or "seqs" not in clip_adapters:
            raise ValueError("clip_adapters: a dict with seqs=[...]")
        unknown = set(clip_adapters) - {"seqs", "min_overlap", "max_mismatch_permille", "clip"}
        if unknown:
            raise ValueError("clip_adapters: unknown keys %r" % sorted(unknown))
        self.set = adapter_set(clip_adapters["seqs"], clip_adapters.get("min_overlap", 3),
                               clip_adapters.get("max_mismatch_permille", 100))
        self.want_clip = bool(clip_adapters.get("clip", False))
        if self.want_clip and not clip_ok:
            raise ValueError("clip_adapters: clip=True is trim_fastq's alone")
        self.buf = torch.zeros(CLIP_WORDS, dtype=torch.int64, device=dev)
        self.ptr, self.reset, self.words_ptr = self.buf.data_ptr(), True, None

    def read(self):
        """-> sk_fastq_clip_stats's members but `reserved`, as ints"""
        return FastqClipStats.from_buffer_copy(self.buf.cpu().numpy().tobytes()).as_dict()


class FastqRejectsCounts(C.Structure):
    """sk_fastq_rejects_counts"""
    _fields_ = [("records", C.c_uint64), ("bytes", C.c_uint64), ("reads", C.c_uint64), ("valid", C.c_uint32),
                ("flags", C.c_uint32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def _rejects_flags(rejects):
    """rejects=True | "pairs" (or the flags themselves) -> the flags of sk_trim_fastq_rejects_device_async"""
    if rejects is True:
        return 0
    if rejects == "pairs":
        return SK_FQ_REJECTS_PAIRS
    if isinstance(rejects, int) and not isinstance(rejects, bool):
        return rejects
    raise ValueError("rejects: False, True or \"pairs\", not %r" % (rejects,))


class _SideCalls:
    """What one call of a driver runs beside its text call, from the driver's own keywords: the buffer objects of report=,
    audit=, bases=, adapters= and clip_adapters= (rep, aud, bas, adp, clp: None where the option is off, and nothing is
    allocated for it) and the flags of rejects= (rej_flags: None where off).  Built in front of everything a driver
    allocates or enqueues, so a bad option raises its ValueError with nothing in flight.  clip_ok: whether the driver hands
    clip words out (trim_fastq alone does); mode: the driver's."""

    def __init__(self, dev, clip_ok, mode, report=False, audit=False, bases=False, rejects=False, adapters=False,
                 clip_adapters=None):
        self.mode = mode
        self.clp = _ClipBuffers(clip_adapters, dev, clip_ok=clip_ok) if clip_adapters is not None else None
        self.rep = _ReportBuffers(report, dev) if report else None
        self.aud = _AuditBuffers(dev) if audit else None
        self.bas = _BasesBuffers(bases, dev) if bases else None
        self.adp = _AdaptersBuffers(adapters, dev, clip_ok=clip_ok) if adapters else None
        self.rej_flags = _rejects_flags(rejects) if rejects else None
        if rejects and self.rej_flags & SK_FQ_REJECTS_PAIRS and mode == "se":
            raise ValueError("rejects=\"pairs\" needs a pair mode")

    def rewind(self):
        """in front of a driver's second run (_with_batch_table): what the first run left in the objects goes, as if they
        had been built anew; what accumulates on the device is zeroed by the run's own reset"""
        if self.clp:
            self.clp.reset, self.clp.words_ptr = True, None
        if self.adp and self.adp.clip is not None:
            self.adp.clip = None
            self.adp._out()

    def enqueue(self, ctx, ws_ptr, ptrs, bounds, trunc_n, kind, order, reset, stream, writing=True, rejects_ws=None,
                rejects_out=None):
        """What follows a driver's text call on its stream, over its workspace and its texts: behind a writing pass the
        report, the audit and the bases, then the rejects, then the adapter search (writing=False: a counting pass, which
        only the rejects follow).  rejects_ws: the rejects call's workspace tensor (None: no rejects call), rejects_out: its
        FastqOutput or None (it only counts).  kind: "plain" or "piece"; order: the text call's FastqOrder or None; reset:
        zero what accumulates (not the rejects, which do not).  The audit does without the names when a text is empty (no
        pointer); the bases, the rejects and the adapters, which need `in`, give an empty text their own buffer's address
        with the bound 0, of which no byte is loaded."""
        kind, cap = _source_kind(kind, order)
        total, mode = sum(bounds), self.mode
        own = lambda ptr: ([ptr if p is None else p for p in ptrs], [0 if p is None else b for p, b in zip(ptrs, bounds)])
        rep, aud, bas, adp = (self.rep, self.aud, self.bas, self.adp) if writing else (None,) * 4
        if rep:
            ctx.trim_fastq_report_device_async(ws_ptr, total, trunc_n, rep.ptr, kind=kind, batch_capacity=cap, hists=rep.hists,
                                               reset=reset, stream=stream)
        if aud:
            ctx.trim_fastq_audit_device_async(ws_ptr, total, trunc_n, aud.ptr,
                                              text_ptrs=None if any(p is None for p in ptrs) else ptrs, text_bounds=bounds,
                                              mode=mode, kind=kind, batch_capacity=cap, qual_hist_ptr=aud.hist_ptr, reset=reset,
                                              stream=stream)
        if bas:
            p, b = own(bas.ptr)
            ctx.trim_fastq_bases_device_async(ws_ptr, total, trunc_n, bas.ptr, p, b, mode=mode, kind=kind, batch_capacity=cap,
                                              hists=bas.hists, reset=reset, stream=stream)
        if rejects_ws is not None:
            p, b = own(rejects_ws.data_ptr())
            ctx.trim_fastq_rejects_device_async(ws_ptr, total, trunc_n, p, b, rejects_out, rejects_ws.data_ptr(),
                                                rejects_ws.numel(), mode=mode, kind=kind, batch_capacity=cap,
                                                pairs=self.rej_flags, stream=stream)
        if adp:
            p, b = own(adp.ptr)
            ctx.trim_fastq_adapters_device_async(ws_ptr, total, trunc_n, adp.ptr, p, b, adp.set, mode=mode, kind=kind,
                                                 batch_capacity=cap, out=adp.out, reset=reset, stream=stream)

    def collect(self, counts):
        """once the stream has been waited for: the audit, the bases, the adapters and the clip stats into counts, each
        under its option's name where the option is on; -> the report as a dict, or None"""
        for key, b in (("audit", self.aud), ("bases", self.bas), ("adapters", self.adp), ("clip", self.clp)):
            if b:
                counts[key] = b.read()
        return self.rep.read() if self.rep else None


class _Writers:
    """The BGZF writers behind a text call whose outputs are sized without a look at the text: per used output the
    trimmed text's buffer of `cap` bytes (outs: the call's FastqOutput entries over them) and, with gz, its image and
    its writer's workspace.  alloc(n): a uint8 device tensor of n bytes (16 at least)."""

    def __init__(self, used, cap, search, alloc, gz=True):
        self.cap, self.search = cap, search
        new = lambda n: [alloc(n) if o in used else None for o in range(3)]
        self.text = new(cap)
        if gz:
            self.bound = lib().sk_bgzf_bound(cap, SK_BGZF_EOF)
            self.ws_bytes = lib().sk_bgzf_workspace_bytes_flags(cap, SK_BGZF_SEARCH if search else 0)
            self.images, self.ws = new(self.bound), new(self.ws_bytes)
        self.outs = [FastqOutput() if t is None else FastqOutput(t.data_ptr(), cap, None, 0) for t in self.text]

    def enqueue(self, ctx, workspace_ptr, stream, eof=True, words=None):
        """a writer per used output, in output order, fed by the device words of the trim whose workspace this is (words:
        trim_fastq_rejects_output_words where it is a rejects call's, whose one text is output 0)"""
        for o, t in enumerate(self.text):
            if t is not None:
                nbytes, written = words(workspace_ptr) if words else ctx.trim_fastq_output_words(workspace_ptr, o)
                ctx.bgzf_device_async(t.data_ptr(), self.cap, self.images[o].data_ptr(), self.bound, self.ws[o].data_ptr(),
                                      self.ws_bytes, eof=eof, bytes_dev_ptr=nbytes, valid_dev_ptr=written, stream=stream,
                                      search=self.search)

    def finish(self, ctx, stream):
        """the writers' finishes -> the three images narrowed to their bytes (None where the output is not used)"""
        return tuple(None if im is None else im[:ctx.bgzf_device_finish(w.data_ptr(), stream)["bytes_out"]]
                     for im, w in zip(self.images, self.ws))


class FastqPiece(C.Structure):
    _fields_ = [("start_dev", C.c_void_p * 2), ("more", C.c_uint32), ("reserved", C.c_uint32)]


class FastqPieceCounts(C.Structure):
    _fields_ = [("consumed", C.c_uint64 * 2), ("carried_bytes", C.c_uint64 * 2), ("ok", C.c_uint32),
                ("inherited_range", C.c_uint32)]

    def as_dict(self):
        return {"consumed": list(self.consumed), "carried_bytes": list(self.carried_bytes), "ok": int(self.ok),
                "inherited_range": int(self.inherited_range)}


class FastqCarryWords(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("valid", C.c_uint64), ("status", C.c_uint64)]


class FastqOrder(C.Structure):
    _fields_ = [("threads", C.c_uint32), ("reserved", C.c_uint32), ("batch_len", C.c_uint64),
                ("batch_capacity", C.c_uint64), ("batch_limit", C.c_uint64)]


class FastqOrderCounts(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("units", C.c_uint64), ("last_batch_units", C.c_uint64),
                ("records_unbatched", C.c_uint64 * 2), ("stopped_on_mismatch", C.c_uint32), ("long_line_input", C.c_uint32),
                ("long_line", C.c_uint64), ("error_batch", C.c_uint64)]

    def as_dict(self):
        return {"batches": int(self.batches), "units": int(self.units), "last_batch_units": int(self.last_batch_units),
                "records_unbatched": list(self.records_unbatched), "stopped_on_mismatch": int(self.stopped_on_mismatch),
                "long_line_input": int(self.long_line_input), "long_line": int(self.long_line),
                "error_batch": int(self.error_batch)}


class FastqOrderState(C.Structure):
    """sk_fastq_order_state: lives in device memory; this is its layout (and the host copy a finish hands out)"""
    _fields_ = [("carried_lines", C.c_uint64 * 2), ("batches", C.c_uint64), ("units", C.c_uint64),
                ("last_batch_units", C.c_uint64), ("ended", C.c_uint32), ("stopped_on_mismatch", C.c_uint32),
                ("failed", C.c_uint32), ("reserved0", C.c_uint32), ("reserved1", C.c_uint64)]

    def as_dict(self):
        return {"carried": list(self.carried_lines), "batches": int(self.batches), "units": int(self.units),
                "last_batch_units": int(self.last_batch_units), "ended": int(self.ended),
                "stopped_on_mismatch": int(self.stopped_on_mismatch), "failed": int(self.failed)}


class FastqOrderPieceCounts(C.Structure):
    _fields_ = [("table_full", C.c_uint32), ("undetermined", C.c_uint32), ("inherited_failure", C.c_uint32),
                ("reserved", C.c_uint32), ("state", FastqOrderState)]

    def as_dict(self):
        return {"table_full": int(self.table_full), "undetermined": int(self.undetermined),
                "inherited_failure": int(self.inherited_failure), "state": self.state.as_dict()}


class BgzfInput(C.Structure):
    _fields_ = [("text", C.c_void_p), ("bytes", C.c_uint64), ("bytes_dev", C.c_void_p), ("valid_dev", C.c_void_p)]


class BgzfCounts(C.Structure):
    _fields_ = [("bytes_in", C.c_uint64), ("blocks", C.c_uint64), ("stored_blocks", C.c_uint64), ("bytes_out", C.c_uint64)]

    def as_dict(self):
        return {"bytes_in": int(self.bytes_in), "blocks": int(self.blocks), "stored_blocks": int(self.stored_blocks),
                "bytes_out": int(self.bytes_out)}


class BgzfInflateCounts(C.Structure):
    _fields_ = [("bytes_in", C.c_uint64), ("members", C.c_uint64), ("bytes_out", C.c_uint64), ("error", C.c_int32),
                ("reserved", C.c_uint32), ("error_member", C.c_uint64), ("error_offset", C.c_uint64)]

    def as_dict(self):
        return {"bytes_in": int(self.bytes_in), "members": int(self.members), "bytes_out": int(self.bytes_out),
                "error": int(self.error), "error_member": int(self.error_member), "error_offset": int(self.error_offset)}


class GzipInflateCounts(C.Structure):
    _fields_ = [("bytes_in", C.c_uint64), ("members", C.c_uint64), ("bytes_out", C.c_uint64), ("stretches", C.c_uint64),
                ("stretches_used", C.c_uint64), ("error", C.c_int32), ("reserved", C.c_uint32), ("error_member", C.c_uint64),
                ("error_offset", C.c_uint64)]

    def as_dict(self):
        return {"bytes_in": int(self.bytes_in), "members": int(self.members), "bytes_out": int(self.bytes_out),
                "stretches": int(self.stretches), "stretches_used": int(self.stretches_used), "error": int(self.error),
                "error_member": int(self.error_member), "error_offset": int(self.error_offset)}


class GzipPieceState(C.Structure):
    """sk_gzip_piece_state: lives in device memory; this is its layout (and the host copy tests read)"""
    _fields_ = [(n, C.c_uint64) for n in ("pos_bit", "in_member", "member_text", "member_crc", "members", "text_bytes", "status",
                                          "error", "error_member", "error_offset", "done")] + \
               [("reserved", C.c_uint64 * 5), ("history", C.c_uint8 * 32768)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:11]}


class GzipPiece(C.Structure):
    _fields_ = [("image_offset", C.c_uint64), ("window_bytes", C.c_uint64), ("last", C.c_uint32), ("reserved", C.c_uint32)]


class GzipPieceCounts(C.Structure):
    _fields_ = [("pos_bit", C.c_uint64), ("in_member", C.c_uint64), ("image_bytes_consumed", C.c_uint64),
                ("window_limited", C.c_uint32), ("inherited", C.c_uint32), ("done", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:6]}


class SickleError(RuntimeError):
    pass


class GzDataError(SickleError):
    """sk_bgzf_inflate_device_finish returned SK_EDATA: member `member` at byte `offset` of the image is bad, `reason`
    (SK_GZ_*) says why.  SK_GZ_HEADER at member 0 is what a plain, non-BGZF gzip file gives: decode it on the host."""

    def __init__(self, reason, member, offset, counts=None):
        super().__init__("not valid BGZF: member %d at byte %d (reason %d)" % (member, offset, reason))
        self.reason, self.member, self.offset, self.counts = reason, member, offset, counts


class TrimError(SickleError):
    """sk_trim_device_finish returned SK_ESPACE or SK_EINVAL: `rc` says which, `counts` (dict) what it needs."""

    def __init__(self, msg, rc, counts):
        super().__init__(msg)
        self.rc, self.counts = rc, counts


class FormatError(SickleError):
    """sk_trim_fastq_device_finish returned SK_EFORMAT: `reason` (SK_FQ_*) of record `record` of input `input`."""

    def __init__(self, reason, input, record, counts=None):
        super().__init__("malformed FASTQ record %d of input %d (reason %d)" % (record, input, reason))
        self.reason, self.input, self.record, self.counts = reason, input, record, counts


class LongLineError(SickleError):
    """sk_trim_fastq_ordered_device_finish returned SK_ELONGLINE: line `line` of input `input` has batch_len - 1 bytes or
    more, which the reference's reader would split."""

    def __init__(self, input, line, counts=None):
        super().__init__("line %d of input %d is as long as the batch budget" % (line, input))
        self.input, self.line, self.counts = input, line, counts


class RangeError(SickleError):
    """A quality char outside the encoding's range (the reference's exit(1) path)."""

    def __init__(self, read, pos, ch):
        super().__init__("quality value %d out of range at read %d, position %d" % (ch, read, pos + 1))
        self.read, self.pos, self.ch = read, pos, ch


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SickleError("%s is missing: build it with `make -C sickle_amd/csrc` "
                              "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        # torch (when installed) bundles its own copy of the HIP runtime, and a process can only
        # initialise one: whichever copy is loaded first wins and the other then sees no device.
        # Load torch's first, so that a later `import torch` in the same process (bench.py, the
        # tests) still works; libsickle_amd.so binds to the copy that is already there.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.sk_quality_constants.restype = C.POINTER(C.c_int32)
        L.sk_quality_constants.argtypes = [C.c_int32]
        L.sk_typename.restype = C.c_char_p
        L.sk_typename.argtypes = [C.c_int32]
        L.sk_abi_version.restype = C.c_int
        L.sk_device_count.restype = C.c_int
        L.sk_create.restype = C.c_int
        L.sk_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.sk_destroy.restype = None
        L.sk_destroy.argtypes = [C.c_void_p]
        L.sk_last_error.restype = C.c_char_p
        L.sk_last_error.argtypes = [C.c_void_p]
        L.sk_device.restype = C.c_int
        L.sk_device.argtypes = [C.c_void_p]
        L.sk_host_alloc.restype = C.c_void_p
        L.sk_host_alloc.argtypes = [C.c_void_p, C.c_size_t]
        L.sk_host_free.restype = None
        L.sk_host_free.argtypes = [C.c_void_p, C.c_void_p]
        L.sk_scan_device_async.restype = C.c_int
        L.sk_scan_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Batch), C.c_void_p, C.c_void_p]
        L.sk_scan_counted_device_async.restype = C.c_int
        L.sk_scan_counted_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Batch), C.c_void_p, C.c_void_p,
                                                   C.c_void_p]
        L.sk_scan_device_finish.restype = C.c_int
        L.sk_scan_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Err)]
        L.sk_trim_batch.restype = C.c_int
        L.sk_trim_batch.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(Batch), C.c_void_p, C.POINTER(Err)]
        L.sk_submit.restype = C.c_int
        L.sk_submit.argtypes = [C.c_void_p, C.c_int, C.POINTER(Params), C.POINTER(Batch), C.c_void_p]
        L.sk_wait.restype = C.c_int
        L.sk_wait.argtypes = [C.c_void_p, C.c_int, C.POINTER(Err)]
        L.sk_kernel_for.restype = C.c_int
        L.sk_kernel_for.argtypes = [C.POINTER(Batch)]
        L.sk_kernel_name.restype = C.c_char_p
        L.sk_kernel_name.argtypes = [C.c_int]
        L.sk_probe_read_bandwidth.restype = C.c_int
        L.sk_probe_read_bandwidth.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.POINTER(C.c_double)]
        L.sk_count_pairs_device_async.restype = C.c_int
        L.sk_count_pairs_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.sk_count_pairs_device_finish.restype = C.c_int
        L.sk_count_pairs_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(PairCounts)]
        L.sk_seg_classes.restype = C.c_uint32
        L.sk_seg_classes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.sk_bgzf_deflate.restype = C.c_int
        L.sk_bgzf_deflate.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.sk_bgzf_last_error.restype = C.c_char_p
        L.sk_trim_workspace_bytes.restype = C.c_size_t
        L.sk_trim_workspace_bytes.argtypes = [C.c_uint64]
        L.sk_trim_device_async.restype = C.c_int
        L.sk_trim_device_async.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_int, C.POINTER(TrimOutput),
                                           C.c_void_p, C.c_size_t, C.c_void_p]
        L.sk_trim_device_finish.restype = C.c_int
        L.sk_trim_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TrimCounts)]
        L.sk_trim_fastq_workspace_bytes.restype = C.c_size_t
        L.sk_trim_fastq_workspace_bytes.argtypes = [C.c_uint64, C.c_int32]
        L.sk_trim_fastq_device_async.restype = C.c_int
        L.sk_trim_fastq_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FastqInput), C.c_int,
                                                 C.POINTER(FastqOutput), C.c_void_p, C.c_size_t, C.c_void_p]
        L.sk_trim_fastq_device_finish.restype = C.c_int
        L.sk_trim_fastq_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FastqCounts)]
        L.sk_trim_fastq_ordered_workspace_bytes.restype = C.c_size_t
        L.sk_trim_fastq_ordered_workspace_bytes.argtypes = [C.c_uint64, C.c_int32, C.c_uint64]
        L.sk_trim_fastq_ordered_device_async.restype = C.c_int
        L.sk_trim_fastq_ordered_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FastqInput), C.c_int,
                                                         C.POINTER(FastqOrder), C.POINTER(FastqOutput), C.c_void_p,
                                                         C.c_size_t, C.c_void_p]
        L.sk_trim_fastq_ordered_device_finish.restype = C.c_int
        L.sk_trim_fastq_ordered_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FastqCounts),
                                                          C.POINTER(FastqOrderCounts)]
        L.sk_trim_fastq_ordered_batches.restype = C.c_int
        L.sk_trim_fastq_ordered_batches.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        L.sk_trim_fastq_chained_device_async.restype = C.c_int
        L.sk_trim_fastq_chained_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FastqInput),
                                                         C.POINTER(FastqLengths), C.c_int, C.POINTER(FastqOrder),
                                                         C.POINTER(FastqOutput), C.c_void_p, C.c_size_t, C.c_void_p]
        L.sk_trim_fastq_piece_device_async.restype = C.c_int
        L.sk_trim_fastq_piece_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FastqInput),
                                                       C.POINTER(FastqLengths), C.POINTER(FastqPiece), C.c_int,
                                                       C.POINTER(FastqOutput), C.c_void_p, C.c_size_t, C.c_void_p]
        L.sk_trim_fastq_piece_words.restype = C.c_int
        L.sk_trim_fastq_piece_words.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_void_p)]
        L.sk_trim_fastq_piece_device_finish.restype = C.c_int
        L.sk_trim_fastq_piece_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FastqCounts),
                                                        C.POINTER(FastqPieceCounts)]
        L.sk_trim_fastq_ordered_piece_workspace_bytes.restype = C.c_size_t
        L.sk_trim_fastq_ordered_piece_workspace_bytes.argtypes = [C.c_uint64, C.c_int32, C.c_uint64]
        L.sk_trim_fastq_ordered_piece_device_async.restype = C.c_int
        L.sk_trim_fastq_ordered_piece_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FastqInput),
                                                               C.POINTER(FastqLengths), C.POINTER(FastqPiece),
                                                               C.POINTER(FastqOrder), C.c_void_p, C.c_void_p, C.c_int,
                                                               C.POINTER(FastqOutput), C.c_void_p, C.c_size_t, C.c_void_p]
        L.sk_trim_fastq_ordered_piece_device_finish.restype = C.c_int
        L.sk_trim_fastq_ordered_piece_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FastqCounts),
                                                                C.POINTER(FastqOrderCounts), C.POINTER(FastqPieceCounts),
                                                                C.POINTER(FastqOrderPieceCounts)]
        L.sk_fastq_carry_device_async.restype = C.c_int
        L.sk_fastq_carry_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                                  C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p]
        L.sk_bgzf_inflate_output_words.restype = C.c_int
        L.sk_bgzf_inflate_output_words.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.sk_gzip_inflate_output_words.restype = C.c_int
        L.sk_gzip_inflate_output_words.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.sk_trim_fastq_output_words.restype = C.c_int
        L.sk_trim_fastq_output_words.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        L.sk_bgzf_bound.restype = C.c_uint64
        L.sk_bgzf_bound.argtypes = [C.c_uint64, C.c_int]
        L.sk_bgzf_workspace_bytes.restype = C.c_size_t
        L.sk_bgzf_workspace_bytes.argtypes = [C.c_uint64]
        L.sk_bgzf_workspace_bytes_flags.restype = C.c_size_t
        L.sk_bgzf_workspace_bytes_flags.argtypes = [C.c_uint64, C.c_int]
        L.sk_bgzf_device_async.restype = C.c_int
        L.sk_bgzf_device_async.argtypes = [C.c_void_p, C.POINTER(BgzfInput), C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                           C.c_size_t, C.c_void_p]
        L.sk_bgzf_device_finish.restype = C.c_int
        L.sk_bgzf_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BgzfCounts)]
        L.sk_bgzf_inflate_workspace_bytes.restype = C.c_size_t
        L.sk_bgzf_inflate_workspace_bytes.argtypes = [C.c_uint64]
        L.sk_bgzf_inflate_device_async.restype = C.c_int
        L.sk_bgzf_inflate_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                   C.c_size_t, C.c_void_p]
        L.sk_bgzf_inflate_device_finish.restype = C.c_int
        L.sk_bgzf_inflate_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(BgzfInflateCounts)]
        L.sk_gzip_inflate_workspace_bytes.restype = C.c_size_t
        L.sk_gzip_inflate_workspace_bytes.argtypes = [C.c_uint64, C.c_uint64]
        L.sk_gzip_inflate_device_async.restype = C.c_int
        L.sk_gzip_inflate_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                                   C.c_size_t, C.c_void_p]
        L.sk_gzip_inflate_device_finish.restype = C.c_int
        L.sk_gzip_inflate_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GzipInflateCounts)]
        L.sk_gzip_inflate_piece_workspace_bytes.restype = C.c_size_t
        L.sk_gzip_inflate_piece_workspace_bytes.argtypes = [C.c_uint64, C.c_uint64]
        L.sk_gzip_inflate_piece_device_async.restype = C.c_int
        L.sk_gzip_inflate_piece_device_async.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(GzipPiece), C.c_void_p,
                                                         C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p]
        L.sk_gzip_inflate_piece_device_finish.restype = C.c_int
        L.sk_gzip_inflate_piece_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(GzipInflateCounts),
                                                          C.POINTER(GzipPieceCounts)]
        L.sk_trim_fastq_report_device_async.restype = C.c_int
        L.sk_trim_fastq_report_device_async.argtypes = [C.c_void_p, C.POINTER(FastqReportSource), C.c_void_p,
                                                        C.POINTER(FastqReportHists), C.c_int, C.c_void_p]
        L.sk_trim_fastq_bases_device_async.restype = C.c_int
        L.sk_trim_fastq_bases_device_async.argtypes = [C.c_void_p, C.POINTER(FastqReportSource), C.POINTER(FastqInput),
                                                       C.c_int, C.c_void_p, C.POINTER(FastqBasesHists), C.c_int, C.c_void_p]
        L.sk_trim_fastq_adapters_device_async.restype = C.c_int
        L.sk_trim_fastq_adapters_device_async.argtypes = [C.c_void_p, C.POINTER(FastqReportSource), C.POINTER(FastqInput),
                                                          C.c_int, C.POINTER(FastqAdapterSet), C.c_void_p,
                                                          C.POINTER(FastqAdaptersOut), C.c_int, C.c_void_p]
        L.sk_trim_fastq_clip_extra_bytes.restype = C.c_size_t
        L.sk_trim_fastq_clip_extra_bytes.argtypes = [C.c_uint64]
        L.sk_trim_fastq_clipped_device_async.restype = C.c_int
        L.sk_trim_fastq_clipped_device_async.argtypes = [C.c_void_p, C.POINTER(Params), C.POINTER(FastqInput), C.POINTER(FastqClip),
                                                         C.c_int, C.POINTER(FastqOutput), C.c_void_p, C.c_size_t, C.c_void_p]
        L.sk_trim_fastq_audit_device_async.restype = C.c_int
        L.sk_trim_fastq_audit_device_async.argtypes =[C.c_void_p, C.POINTER(FastqReportSource), C.POINTER(FastqInput),
                                                       C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.sk_trim_fastq_rejects_workspace_bytes.restype = C.c_size_t
        L.sk_trim_fastq_rejects_workspace_bytes.argtypes = [C.c_uint64]
        L.sk_trim_fastq_rejects_bound.restype = C.c_uint64
        L.sk_trim_fastq_rejects_bound.argtypes = [C.c_uint64]
        L.sk_trim_fastq_rejects_device_async.restype = C.c_int
        L.sk_trim_fastq_rejects_device_async.argtypes = [C.c_void_p, C.POINTER(FastqReportSource), C.POINTER(FastqInput),
                                                         C.c_int, C.POINTER(FastqOutput), C.c_int, C.c_void_p, C.c_size_t,
                                                         C.c_void_p]
        L.sk_trim_fastq_rejects_device_finish.restype = C.c_int
        L.sk_trim_fastq_rejects_device_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(FastqRejectsCounts)]
        L.sk_trim_fastq_rejects_output_words.restype = C.c_int
        L.sk_trim_fastq_rejects_output_words.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
        _lib = L
    return _lib


def make_params(qualtype="sanger", q=20, l=20, no5=False, trunc_n=False):
    qt = QUALTYPES[qualtype] if isinstance(qualtype, str) else int(qualtype)
    return Params(qt, int(q), int(l), int(bool(no5)), int(bool(trunc_n)))


def _np_ptr(a):
    return None if a is None else a.ctypes.data


# ---- the structs of the FASTQ text calls, from the one or two entries per input the wrappers take --------------------------
def _two(xs, fill):
    return list(xs) + [fill] * (2 - len(xs))


def _fastq_input(text_ptrs, text_bytes, max_read_len=0):
    return FastqInput((C.c_void_p * 2)(*_two(text_ptrs, None)), (C.c_uint64 * 2)(*_two(text_bytes, 0)), max_read_len)


def _fastq_lengths(bytes_dev_ptrs, valid_dev_ptrs):
    return FastqLengths((C.c_void_p * 2)(*_two(bytes_dev_ptrs, None)), (C.c_void_p * 2)(*_two(valid_dev_ptrs, None)))


def _fastq_piece(start_dev_ptrs, more):
    return FastqPiece((C.c_void_p * 2)(*_two(start_dev_ptrs, None)), 1 if more else 0, 0)


def _fastq_outputs(outs):
    return (FastqOutput * 3)(*list(outs)[:3])


def _report_source(workspace_ptr, kind, trunc_n, text_bytes, batch_capacity):
    return FastqReportSource(workspace_ptr, REPORT_KINDS.get(kind, kind), int(trunc_n), text_bytes, batch_capacity, 0)


def _source_kind(kind, order):
    """kind ("plain" or "piece") and order (a FastqOrder or None) of a driver's text call -> the kind and batch_capacity
    of the sk_fastq_report_source over its workspace"""
    if order is None:
        return kind, 0
    return {"plain": "ordered", "piece": "ordered_piece"}[kind], order.batch_capacity


def _text_ptrs(texts):
    """texts (uint8 tensors) -> (ptrs, sizes) as the text calls take them: an empty text has no pointer"""
    return [t.data_ptr() if t.numel() else None for t in texts], [t.numel() for t in texts]


def _alloc_on(dev):
    """-> alloc(n): an uninitialised uint8 tensor of n bytes, 16 at least, on dev"""
    import torch
    return lambda n: torch.empty(max(n, 16), dtype=torch.uint8, device=dev)


def _fastq_ws_bytes(sizes, trunc_n, order, clip=None):
    """the workspace of a whole-text call on texts of these sizes; order: a FastqOrder or None; clip: not None = a clipped
    call, whose clip section follows"""
    extra = lib().sk_trim_fastq_clip_extra_bytes(sum(sizes)) if clip is not None else 0
    if order is None:
        return lib().sk_trim_fastq_workspace_bytes(sum(sizes), trunc_n) + extra
    return lib().sk_trim_fastq_ordered_workspace_bytes(sum(sizes), trunc_n, order.batch_capacity) + extra


class Context:
    """One sk_ctx.  Raises SickleError when no gfx950 device is usable."""

    def __init__(self, device=-1, slots=2):
        self._h = C.c_void_p()
        rc = lib().sk_create(device, slots, C.byref(self._h))
        if rc != SK_OK:
            raise SickleError("sk_create(device=%d) failed with %d: no usable gfx950 device "
                              "(this library has no CPU path)" % (device, rc))

    def close(self):
        if self._h:
            lib().sk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, err=None):
        if rc == SK_OK:
            return
        if rc == SK_ERANGE:
            raise RangeError(err.read, err.pos, err.ch)
        raise SickleError("libsickle_amd call failed (%d): %s" % (rc, lib().sk_last_error(self._h).decode()))

    def _check_fastq(self, rc, c, counts, record_base=0, read_base=0):
        """the rc of a text call's finish: LongLineError, FormatError, RangeError, TrimError (SK_ESPACE) or _check's.  c: its
        FastqCounts; counts: the dict the exception carries; record_base, read_base: what makes a piece's record and read
        numbers the stream's"""
        if rc == SK_ELONGLINE:
            raise LongLineError(counts["order"]["long_line_input"], counts["order"]["long_line"], counts)
        if rc == SK_EFORMAT:
            raise FormatError(int(c.format_error), int(c.format_input), int(c.format_record) + record_base, counts)
        if rc == SK_ERANGE:
            raise RangeError(int(c.range.read) + read_base, int(c.range.pos), int(c.range.ch))
        if rc == SK_ESPACE:
            raise TrimError("fastq trim failed (%d): %s" % (rc, lib().sk_last_error(self._h).decode()), rc, counts)
        self._check(rc)

    # ---- host buffers (numpy) -------------------------------------------------------------
    def trim_segmented(self, params, qual, tiles, out_index, max_stride, seq=None, slot_order=False):
        """sk_trim_batch on a segmented batch (tiles: numpy array of TILE_DTYPE) -> cuts[n,2] int32
        in the caller's read order (out_index), or in slot order with slot_order=True."""
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        seq = None if seq is None else np.ascontiguousarray(seq, dtype=np.uint8)
        tiles = np.ascontiguousarray(tiles, dtype=TILE_DTYPE)
        out_index = np.ascontiguousarray(out_index, dtype=np.uint32)
        n = len(out_index)
        out = np.full((n, 2), -7, dtype=np.int32)
        b = Batch(_np_ptr(qual), _np_ptr(seq), None, max_stride, 0, None, n, tiles.ctypes.data, len(tiles),
                  out_index.ctypes.data, None, 0, 1 if slot_order else 0)
        err = Err()
        rc = lib().sk_trim_batch(self._h, C.byref(params), C.byref(b), out.ctypes.data, C.byref(err))
        self._check(rc, err)
        return out

    def trim_batch(self, params, qual, seq=None, offsets=None, stride=0, read_len=0, lengths=None, n_reads=None):
        """sk_trim_batch on numpy host arrays -> cuts[n,2] int32.  Raises RangeError like the
        reference exits."""
        qual = np.ascontiguousarray(qual, dtype=np.uint8)
        seq = None if seq is None else np.ascontiguousarray(seq, dtype=np.uint8)
        if offsets is not None:
            offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
            n = len(offsets) - 1
        else:
            n = n_reads if n_reads is not None else (len(lengths) if lengths is not None else qual.size // stride)
        lengths = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint32)
        out = np.full((n, 2), -7, dtype=np.int32)
        b = Batch(_np_ptr(qual), _np_ptr(seq), _np_ptr(offsets), stride, read_len, _np_ptr(lengths), n)
        err = Err()
        rc = lib().sk_trim_batch(self._h, C.byref(params), C.byref(b), out.ctypes.data, C.byref(err))
        self._check(rc, err)
        return out

    def submit(self, slot, params, qual, out, seq=None, offsets=None, stride=0, read_len=0, lengths=None, n_reads=0):
        b = Batch(_np_ptr(qual), _np_ptr(seq), _np_ptr(offsets), stride, read_len, _np_ptr(lengths), n_reads)
        self._check(lib().sk_submit(self._h, slot, C.byref(params), C.byref(b), out.ctypes.data))

    def wait(self, slot):
        err = Err()
        self._check(lib().sk_wait(self._h, slot, C.byref(err)), err)

    # ---- device-resident buffers (raw device pointers, e.g. torch .data_ptr()) --------------
    def scan_device_async(self, params, qual_ptr, out_ptr, n_reads, stride=0, read_len=0, seq_ptr=None,
                          offsets_ptr=None, lengths_ptr=None, stream=None):
        b = Batch(qual_ptr, seq_ptr, offsets_ptr, stride, read_len, lengths_ptr, n_reads)
        self._check(lib().sk_scan_device_async(self._h, C.byref(params), C.byref(b), out_ptr, stream))

    def scan_counted_device_async(self, params, qual_ptr, out_ptr, n_reads_bound, n_reads_dev_ptr, offsets_ptr, seq_ptr=None,
                                  max_read_len=0, stream=None):
        """sk_scan_counted_device_async on raw device pointers: an `offsets` batch of at most n_reads_bound reads whose
        read count is the 8-byte device word at n_reads_dev_ptr, read on the stream (None: the bound is the count).
        Cuts are written for the reads below min(word, bound) only; max_read_len is the longest-read hint (0 = unknown)."""
        b = Batch(qual_ptr, seq_ptr, offsets_ptr, max_read_len, 0, None, n_reads_bound)
        self._check(lib().sk_scan_counted_device_async(self._h, C.byref(params), C.byref(b), n_reads_dev_ptr, out_ptr, stream))

    def probe_read_bandwidth(self, dev_ptr, nbytes, launches=20, stream=None):
        """GB/s of a read-only stream over [dev_ptr, dev_ptr + nbytes) on this device."""
        g = C.c_double()
        self._check(lib().sk_probe_read_bandwidth(self._h, dev_ptr, nbytes, launches, stream, C.byref(g)))
        return g.value

    def count_pairs_device(self, cuts_ptr, n_pairs, classes_ptr=None, stream=None):
        """Pair classes of the cuts at cuts_ptr (mates at 2k, 2k+1) -> (both, only_first, only_second, none)."""
        self._check(lib().sk_count_pairs_device_async(self._h, cuts_ptr, n_pairs, classes_ptr, stream))
        c = PairCounts()
        self._check(lib().sk_count_pairs_device_finish(self._h, stream, C.byref(c)))
        return c.both, c.only_first, c.only_second, c.none

    def scan_device_finish(self, stream=None):
        err = Err()
        self._check(lib().sk_scan_device_finish(self._h, stream, C.byref(err)), err)

    def trim_device_async(self, cuts_ptr, n_reads, outs, workspace_ptr, workspace_bytes, mode="se", qual_ptr=None,
                          seq_ptr=None, offsets_ptr=None, stride=0, read_len=0, lengths_ptr=None, stream=None):
        """sk_trim_device_async on raw device pointers; outs: up to three TrimOutput (missing ones are not produced)."""
        arr = (TrimOutput * 3)(*list(outs)[:3])
        b = Batch(qual_ptr, seq_ptr, offsets_ptr, stride, read_len, lengths_ptr, n_reads)
        self._check(lib().sk_trim_device_async(self._h, C.byref(b), cuts_ptr, TRIM_MODES.get(mode, mode), arr,
                                               workspace_ptr, workspace_bytes, stream))

    def trim_device_finish(self, workspace_ptr, stream=None):
        """sk_trim_device_finish -> counts (dict); raises TrimError (with .counts) on SK_ESPACE / SK_EINVAL."""
        c = TrimCounts()
        rc = lib().sk_trim_device_finish(self._h, workspace_ptr, stream, C.byref(c))
        if rc in (SK_ESPACE, SK_EINVAL):
            raise TrimError("trim failed (%d): %s" % (rc, lib().sk_last_error(self._h).decode()), rc, c.as_dict())
        self._check(rc)
        return c.as_dict()

    def trim_device(self, cuts_ptr, n_reads, outs, workspace_ptr, workspace_bytes, mode="se", stream=None, **batch):
        """trim_device_async + trim_device_finish: the counts, or TrimError."""
        self.trim_device_async(cuts_ptr, n_reads, outs, workspace_ptr, workspace_bytes, mode=mode, stream=stream, **batch)
        return self.trim_device_finish(workspace_ptr, stream)

    def trim_reads_device(self, params, qual, seq=None, offsets=None, stride=0, read_len=0, lengths=None, mode="se",
                          cuts=None):
        """Scan (unless `cuts`, a device int32 [n, 2] tensor, is given), trim and finish a device-resident batch of torch
        tensors (uint8 qual / seq, uint64-valued int64 offsets, int32 lengths) on the current stream.  Returns a tuple of
        three entries, one per output of the mode (None where the mode has no such output): (qual, seq, offsets,
        read_index) tensors narrowed to their counts (seq None without seq).  A count-only pass sizes the outputs."""
        import torch
        dev = qual.device
        if offsets is not None:
            n = offsets.numel() - 1
        elif lengths is not None:
            n = lengths.numel()
        else:
            n = qual.numel() // stride if stride else 0
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        batch = dict(qual_ptr=ptr(qual), seq_ptr=ptr(seq), offsets_ptr=ptr(offsets), stride=stride, read_len=read_len,
                     lengths_ptr=ptr(lengths))
        if cuts is None:
            cuts = torch.empty((max(n, 1), 2), dtype=torch.int32, device=dev)
            if n:
                self.scan_device_async(params, ptr(qual), cuts.data_ptr(), n, stride=stride, read_len=read_len,
                                       seq_ptr=ptr(seq) if params.trunc_n else None, offsets_ptr=ptr(offsets),
                                       lengths_ptr=ptr(lengths), stream=stream)
                self.scan_device_finish(stream)
        ws_bytes = lib().sk_trim_workspace_bytes(n)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        counts = self.trim_device(cuts.data_ptr(), n, [TrimOutput() for _ in range(3)], ws.data_ptr(), ws_bytes,
                                  mode=mode, stream=stream, **batch)
        used = TRIM_OUTPUTS[mode]
        bufs, outs = [None] * 3, [TrimOutput() for _ in range(3)]
        for o in used:
            R, B = counts["records"][o], counts["bytes"][o]
            q = torch.empty(max(B, 1), dtype=torch.uint8, device=dev)
            s = torch.empty(max(B, 1), dtype=torch.uint8, device=dev) if seq is not None else None
            off = torch.empty(R + 1, dtype=torch.int64, device=dev)
            idx = torch.empty(max(R, 1), dtype=torch.int64, device=dev)
            bufs[o] = (q, s, off, idx)
            outs[o] = TrimOutput(q.data_ptr(), ptr(s), off.data_ptr(), idx.data_ptr(), B, R)
        counts = self.trim_device(cuts.data_ptr(), n, outs, ws.data_ptr(), ws_bytes, mode=mode, stream=stream, **batch)
        res = [None] * 3
        for o in used:
            q, s, off, idx = bufs[o]
            R, B = counts["records"][o], counts["bytes"][o]
            res[o] = (q[:B], None if s is None else s[:B], off, idx[:R])
        return tuple(res)

    # ---- FASTQ text on the device -------------------------------------------------------------
    def trim_fastq_clipped_device_async(self, params, text_ptrs, text_bounds, set, outs, workspace_ptr, workspace_bytes,
                                        mode="se", bytes_dev_ptrs=None, valid_dev_ptrs=None, start_dev_ptrs=None, more=False,
                                        piece=False, order=None, state_in_ptr=None, state_out_ptr=None, stats_ptr=None,
                                        reset=False, max_read_len=0, stream=None, flags=None, reserved=0):
        """sk_trim_fastq_clipped_device_async on raw device pointers: the text call of the kind the arguments name, with
        every read clipped at its 3' adapter hit in front of the scan.  set: a FastqAdapterSet (adapter_set(seqs, ..)).
        bytes_dev_ptrs / valid_dev_ptrs given (lists, as the chained call's): device lengths; piece=True (or start_dev_ptrs
        given): a piece, with `more`; order: a FastqOrder; state_out_ptr: an ordered piece.  stats_ptr: a
        sk_fastq_clip_stats in device memory or None; reset: SK_FQ_CLIP_RESET (flags: the raw word instead).  The workspace
        holds the kind's bytes plus fastq_clip_extra_bytes; the finish is the kind's.  -> the device address of this call's
        clip words in its workspace."""
        inp = _fastq_input(text_ptrs, text_bounds, max_read_len)
        keep = []
        clip = FastqClip()
        clip.set = C.pointer(set) if set is not None else None
        if bytes_dev_ptrs is not None or valid_dev_ptrs is not None:
            keep.append(_fastq_lengths(bytes_dev_ptrs or (), valid_dev_ptrs or ()))
            clip.lengths = C.addressof(keep[-1])
        if piece or start_dev_ptrs is not None:
            keep.append(_fastq_piece(start_dev_ptrs or (), more))
            clip.piece = C.addressof(keep[-1])
        if order is not None:
            clip.order = C.addressof(order)
        clip.state_in, clip.state_out, clip.stats_dev = state_in_ptr, state_out_ptr, stats_ptr
        words = C.c_void_p()
        clip.clip_words_dev = C.pointer(words)
        clip.flags = (SK_FQ_CLIP_RESET if reset else 0) if flags is None else flags
        clip.reserved = reserved
        self._check(lib().sk_trim_fastq_clipped_device_async(self._h, C.byref(params), C.byref(inp), C.byref(clip),
                                                             TRIM_MODES.get(mode, mode), _fastq_outputs(outs), workspace_ptr,
                                                             workspace_bytes, stream))
        return words.value

    def _clipped(self, clip, params, text_ptrs, text_bounds, outs, workspace_ptr, workspace_bytes, **kind):
        """a driver's text call as the clipped call of its kind; clip: its _ClipBuffers"""
        clip.words_ptr = self.trim_fastq_clipped_device_async(params, text_ptrs, text_bounds, clip.set, outs, workspace_ptr,
                                                              workspace_bytes, stats_ptr=clip.ptr, reset=clip.reset, **kind)

    def trim_fastq_device_async(self, params, text_ptrs, text_bytes, outs, workspace_ptr, workspace_bytes, mode="se",
                                max_read_len=0, stream=None, clip=None):
        """sk_trim_fastq_device_async on raw device pointers; text_ptrs / text_bytes: one or two entries, outs: up to
        three FastqOutput (missing ones are not produced).  clip (the drivers' own, as in the four calls below): a
        _ClipBuffers, and the call is sk_trim_fastq_clipped_device_async of this kind."""
        if clip is not None:
            return self._clipped(clip, params, text_ptrs, text_bytes, outs, workspace_ptr, workspace_bytes, mode=mode,
                                 max_read_len=max_read_len, stream=stream)
        inp = _fastq_input(text_ptrs, text_bytes, max_read_len)
        self._check(lib().sk_trim_fastq_device_async(self._h, C.byref(params), C.byref(inp), TRIM_MODES.get(mode, mode),
                                                     _fastq_outputs(outs), workspace_ptr, workspace_bytes, stream))

    def trim_fastq_device_finish(self, workspace_ptr, stream=None):
        """sk_trim_fastq_device_finish -> counts (dict); raises FormatError, RangeError or TrimError (SK_ESPACE)."""
        c = FastqCounts()
        rc = lib().sk_trim_fastq_device_finish(self._h, workspace_ptr, stream, C.byref(c))
        counts = c.as_dict()
        self._check_fastq(rc, c, counts)
        return counts

    def trim_fastq_report_device_async(self, workspace_ptr, text_bytes, trunc_n, report_ptr, kind="plain", batch_capacity=0,
                                       hists=None, reset=False, stream=None):
        """sk_trim_fastq_report_device_async on raw device pointers: the report over the workspace of a text call already
        enqueued on `stream`.  kind: "plain", "piece", "ordered" or "ordered_piece" (or SK_FQ_REPORT_*); text_bytes,
        trunc_n, batch_capacity: what that call's workspace formula took; report_ptr: a sk_fastq_report in device memory;
        hists: a FastqReportHists or None.  Only enqueues."""
        src = _report_source(workspace_ptr, kind, trunc_n, text_bytes, batch_capacity)
        self._check(lib().sk_trim_fastq_report_device_async(self._h, C.byref(src), report_ptr,
                                                            C.byref(hists) if hists is not None else None,
                                                            SK_FQ_REPORT_RESET if reset else 0, stream))

    def trim_fastq_audit_device_async(self, workspace_ptr, text_bytes, trunc_n, audit_ptr, text_ptrs=None, text_bounds=None,
                                      mode="se", kind="plain", batch_capacity=0, qual_hist_ptr=None, reset=False, stream=None):
        """sk_trim_fastq_audit_device_async on raw device pointers: the audit over the workspace and the texts of a text
        call already enqueued on `stream`.  kind, text_bytes, trunc_n, batch_capacity: as trim_fastq_report_device_async's;
        text_ptrs, text_bounds: the text call's (None: in == NULL, the names are not looked at); mode: the text call's;
        audit_ptr: a sk_fastq_audit in device memory; qual_hist_ptr: 256 uint64 in device memory or None.  Only enqueues."""
        src = _report_source(workspace_ptr, kind, trunc_n, text_bytes, batch_capacity)
        inp = None if text_ptrs is None else C.byref(_fastq_input(text_ptrs, text_bounds))
        self._check(lib().sk_trim_fastq_audit_device_async(self._h, C.byref(src), inp, TRIM_MODES.get(mode, mode), audit_ptr,
                                                           qual_hist_ptr, SK_FQ_AUDIT_RESET if reset else 0, stream))

    def trim_fastq_bases_device_async(self, workspace_ptr, text_bytes, trunc_n, bases_ptr, text_ptrs, text_bounds, mode="se",
                                      kind="plain", batch_capacity=0, hists=None, reset=False, stream=None):
        """sk_trim_fastq_bases_device_async on raw device pointers: the bases over the workspace and the texts of a text
        call already enqueued on `stream`.  kind, text_bytes, trunc_n, batch_capacity: as trim_fastq_report_device_async's;
        text_ptrs, text_bounds, mode: the text call's (text_ptrs None: in == NULL, which is refused: the texts are the
        data); bases_ptr: a sk_fastq_bases in device memory; hists: a FastqBasesHists or None.  Only enqueues."""
        src = _report_source(workspace_ptr, kind, trunc_n, text_bytes, batch_capacity)
        inp = None if text_ptrs is None else C.byref(_fastq_input(text_ptrs, text_bounds))
        self._check(lib().sk_trim_fastq_bases_device_async(self._h, C.byref(src), inp, TRIM_MODES.get(mode, mode), bases_ptr,
                                                           C.byref(hists) if hists is not None else None,
                                                           SK_FQ_BASES_RESET if reset else 0, stream))

    def trim_fastq_adapters_device_async(self, workspace_ptr, text_bytes, trunc_n, adapters_ptr, text_ptrs, text_bounds, set,
                                         mode="se", kind="plain", batch_capacity=0, out=None, reset=False, stream=None):
        """sk_trim_fastq_adapters_device_async on raw device pointers: the adapter search over the workspace and the texts
        of a text call already enqueued on `stream`.  kind, text_bytes, trunc_n, batch_capacity: as
        trim_fastq_report_device_async's; text_ptrs, text_bounds, mode: the text call's; set: a FastqAdapterSet
        (adapter_set(seqs, ..)); adapters_ptr: a sk_fastq_adapters in device memory; out: a FastqAdaptersOut or None.
        Only enqueues."""
        src = _report_source(workspace_ptr, kind, trunc_n, text_bytes, batch_capacity)
        inp = None if text_ptrs is None else C.byref(_fastq_input(text_ptrs, text_bounds))
        self._check(lib().sk_trim_fastq_adapters_device_async(self._h, C.byref(src), inp, TRIM_MODES.get(mode, mode),
                                                              C.byref(set) if set is not None else None, adapters_ptr,
                                                              C.byref(out) if out is not None else None,
                                                              SK_FQ_ADAPTERS_RESET if reset else 0, stream))

    def trim_fastq_rejects_device_async(self, src_workspace_ptr, text_bytes, trunc_n, text_ptrs, text_bounds, out, workspace_ptr,
                                        workspace_bytes, mode="se", kind="plain", batch_capacity=0, pairs=False, stream=None):
        """sk_trim_fastq_rejects_device_async on raw device pointers: the records of the reads that were not kept, over
        the workspace and the texts of a text call already enqueued on `stream`.  kind, text_bytes, trunc_n,
        batch_capacity: as trim_fastq_report_device_async's; text_ptrs, text_bounds, mode: the text call's; out: a
        FastqOutput or None (the call only counts); workspace_ptr, workspace_bytes: the rejects call's own workspace
        (sk_trim_fastq_rejects_workspace_bytes(text_bytes)); pairs: SK_FQ_REJECTS_PAIRS (or the flags as an int).
        Only enqueues."""
        src = _report_source(src_workspace_ptr, kind, trunc_n, text_bytes, batch_capacity)
        inp = None if text_ptrs is None else C.byref(_fastq_input(text_ptrs, text_bounds))
        flags = pairs if isinstance(pairs, int) and not isinstance(pairs, bool) else (SK_FQ_REJECTS_PAIRS if pairs else 0)
        self._check(lib().sk_trim_fastq_rejects_device_async(self._h, C.byref(src), inp, TRIM_MODES.get(mode, mode),
                                                             C.byref(out) if out is not None else None, flags, workspace_ptr,
                                                             workspace_bytes, stream))

    def trim_fastq_rejects_device_finish(self, workspace_ptr, stream=None):
        """sk_trim_fastq_rejects_device_finish -> counts (dict); raises TrimError (with .counts, the needs) on SK_ESPACE."""
        c = FastqRejectsCounts()
        rc = lib().sk_trim_fastq_rejects_device_finish(self._h, workspace_ptr, stream, C.byref(c))
        if rc == SK_ESPACE:
            raise TrimError("fastq rejects failed (%d): %s" % (rc, lib().sk_last_error(self._h).decode()), rc, c.as_dict())
        self._check(rc)
        return c.as_dict()

    @staticmethod
    def trim_fastq_rejects_output_words(rejects_workspace_ptr):
        """sk_trim_fastq_rejects_output_words -> (bytes_dev, written_dev), device addresses for bgzf_device_async's
        bytes_dev_ptr and valid_dev_ptr"""
        b, w = C.c_void_p(), C.c_void_p()
        rc = lib().sk_trim_fastq_rejects_output_words(rejects_workspace_ptr, C.byref(b), C.byref(w))
        if rc != SK_OK:
            raise SickleError("sk_trim_fastq_rejects_output_words failed (%d)" % rc)
        return b.value, w.value

    def trim_fastq_ordered_device_async(self, params, text_ptrs, text_bytes, order, outs, workspace_ptr, workspace_bytes,
                                        mode="se", max_read_len=0, stream=None, clip=None):
        """sk_trim_fastq_ordered_device_async on raw device pointers; order: a FastqOrder; the rest as
        trim_fastq_device_async."""
        if clip is not None:
            return self._clipped(clip, params, text_ptrs, text_bytes, outs, workspace_ptr, workspace_bytes, mode=mode,
                                 order=order, max_read_len=max_read_len, stream=stream)
        inp = _fastq_input(text_ptrs, text_bytes, max_read_len)
        self._check(lib().sk_trim_fastq_ordered_device_async(self._h, C.byref(params), C.byref(inp), TRIM_MODES.get(mode, mode),
                                                             C.byref(order), _fastq_outputs(outs), workspace_ptr,
                                                             workspace_bytes, stream))

    def trim_fastq_ordered_device_finish(self, workspace_ptr, stream=None):
        """sk_trim_fastq_ordered_device_finish -> counts (dict, with the order counts under "order"); raises
        LongLineError, FormatError, RangeError or TrimError (SK_ESPACE: the batch table when counts["order"]["batches"]
        is batch_capacity + 1, else an output)."""
        c, oc = FastqCounts(), FastqOrderCounts()
        rc = lib().sk_trim_fastq_ordered_device_finish(self._h, workspace_ptr, stream, C.byref(c), C.byref(oc))
        counts = dict(c.as_dict(), order=oc.as_dict())
        self._check_fastq(rc, c, counts)
        return counts

    def trim_fastq_chained_device_async(self, params, text_ptrs, text_bounds, outs, workspace_ptr, workspace_bytes,
                                        bytes_dev_ptrs=(), valid_dev_ptrs=(), mode="se", order=None, max_read_len=0,
                                        stream=None, clip=None):
        """sk_trim_fastq_chained_device_async on raw device pointers: text_bounds are upper bounds on the texts' lengths,
        bytes_dev_ptrs / valid_dev_ptrs (up to two entries each, None = not given) the device words that hold the lengths
        and their validity, e.g. those of bgzf_inflate_output_words.  order: a FastqOrder or None (read order); the
        workspace and the finish are those of trim_fastq_ordered_device_async / trim_fastq_device_async accordingly."""
        if clip is not None:
            return self._clipped(clip, params, text_ptrs, text_bounds, outs, workspace_ptr, workspace_bytes, mode=mode,
                                 bytes_dev_ptrs=list(bytes_dev_ptrs), valid_dev_ptrs=list(valid_dev_ptrs), order=order,
                                 max_read_len=max_read_len, stream=stream)
        inp, lengths = _fastq_input(text_ptrs, text_bounds, max_read_len), _fastq_lengths(bytes_dev_ptrs, valid_dev_ptrs)
        self._check(lib().sk_trim_fastq_chained_device_async(self._h, C.byref(params), C.byref(inp), C.byref(lengths),
                                                             TRIM_MODES.get(mode, mode),
                                                             None if order is None else C.byref(order), _fastq_outputs(outs),
                                                             workspace_ptr, workspace_bytes, stream))

    # ---- FASTQ text in pieces ------------------------------------------------------------------
    def trim_fastq_piece_device_async(self, params, text_ptrs, text_bounds, outs, workspace_ptr, workspace_bytes,
                                      bytes_dev_ptrs=(), valid_dev_ptrs=(), start_dev_ptrs=(), more=False, mode="se",
                                      max_read_len=0, stream=None, piece=True, clip=None):
        """sk_trim_fastq_piece_device_async on raw device pointers: trim_fastq_chained_device_async (read order) on the
        window that starts at the device words start_dev_ptrs (None = 0); more: more text follows, so only whole records
        (pairs) are taken and the rest is the carry.  piece=False passes piece == NULL: the chained call itself."""
        if clip is not None:
            return self._clipped(clip, params, text_ptrs, text_bounds, outs, workspace_ptr, workspace_bytes, mode=mode,
                                 bytes_dev_ptrs=list(bytes_dev_ptrs), valid_dev_ptrs=list(valid_dev_ptrs),
                                 start_dev_ptrs=list(start_dev_ptrs) if piece else None, more=more, piece=piece,
                                 max_read_len=max_read_len, stream=stream)
        inp, lengths = _fastq_input(text_ptrs, text_bounds, max_read_len), _fastq_lengths(bytes_dev_ptrs, valid_dev_ptrs)
        pc = _fastq_piece(start_dev_ptrs, more)
        self._check(lib().sk_trim_fastq_piece_device_async(self._h, C.byref(params), C.byref(inp), C.byref(lengths),
                                                           C.byref(pc) if piece else None, TRIM_MODES.get(mode, mode),
                                                           _fastq_outputs(outs), workspace_ptr, workspace_bytes, stream))

    def _piece_finish(self, workspace_ptr, stream):
        c, pc = FastqCounts(), FastqPieceCounts()
        rc = lib().sk_trim_fastq_piece_device_finish(self._h, workspace_ptr, stream, C.byref(c), C.byref(pc))
        return rc, c, dict(c.as_dict(), piece=pc.as_dict())

    def trim_fastq_piece_device_finish(self, workspace_ptr, stream=None):
        """sk_trim_fastq_piece_device_finish -> counts (dict, with the piece counts under "piece"); raises FormatError,
        RangeError (an inherited one too: counts["piece"]["inherited_range"] is not seen then) or TrimError (SK_ESPACE)."""
        rc, c, counts = self._piece_finish(workspace_ptr, stream)
        self._check_fastq(rc, c, counts)
        return counts

    def trim_fastq_ordered_piece_device_async(self, params, text_ptrs, text_bounds, order, state_in_ptr, state_out_ptr, outs,
                                              workspace_ptr, workspace_bytes, bytes_dev_ptrs=(), valid_dev_ptrs=(),
                                              start_dev_ptrs=(), more=False, mode="se", max_read_len=0, stream=None,
                                              clip=None):
        """sk_trim_fastq_ordered_piece_device_async on raw device pointers: trim_fastq_piece_device_async whose records are
        the batches the piece can commit, in the -a T order.  order: a FastqOrder; state_in_ptr (None: the start of a
        stream) and state_out_ptr: FastqOrderState in device memory."""
        if clip is not None:
            return self._clipped(clip, params, text_ptrs, text_bounds, outs, workspace_ptr, workspace_bytes, mode=mode,
                                 bytes_dev_ptrs=list(bytes_dev_ptrs), valid_dev_ptrs=list(valid_dev_ptrs),
                                 start_dev_ptrs=list(start_dev_ptrs), more=more, piece=True, order=order,
                                 state_in_ptr=state_in_ptr, state_out_ptr=state_out_ptr, max_read_len=max_read_len,
                                 stream=stream)
        inp, lengths = _fastq_input(text_ptrs, text_bounds, max_read_len), _fastq_lengths(bytes_dev_ptrs, valid_dev_ptrs)
        pc = _fastq_piece(start_dev_ptrs, more)
        self._check(lib().sk_trim_fastq_ordered_piece_device_async(self._h, C.byref(params), C.byref(inp), C.byref(lengths),
                                                                   C.byref(pc), C.byref(order), state_in_ptr, state_out_ptr,
                                                                   TRIM_MODES.get(mode, mode), _fastq_outputs(outs),
                                                                   workspace_ptr, workspace_bytes, stream))

    def _ordered_piece_finish(self, workspace_ptr, stream):
        c, oc, pc, opc = FastqCounts(), FastqOrderCounts(), FastqPieceCounts(), FastqOrderPieceCounts()
        rc = lib().sk_trim_fastq_ordered_piece_device_finish(self._h, workspace_ptr, stream, C.byref(c), C.byref(oc),
                                                             C.byref(pc), C.byref(opc))
        return rc, c, dict(c.as_dict(), order=oc.as_dict(), piece=pc.as_dict(), order_piece=opc.as_dict())

    def trim_fastq_ordered_piece_device_finish(self, workspace_ptr, stream=None):
        """sk_trim_fastq_ordered_piece_device_finish -> counts (dict, with "order", "piece" and "order_piece"); raises
        LongLineError, FormatError, RangeError (an inherited one too) or TrimError (SK_ESPACE: an output)."""
        rc, c, counts = self._ordered_piece_finish(workspace_ptr, stream)
        self._check_fastq(rc, c, counts)
        return counts

    @staticmethod
    def trim_fastq_piece_words(workspace_ptr, input):
        """sk_trim_fastq_piece_words -> (consumed_dev, end_dev, ok_dev) device addresses of a piece's words."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if lib().sk_trim_fastq_piece_words(workspace_ptr, input, C.byref(a), C.byref(b), C.byref(c)) != SK_OK:
            raise SickleError("sk_trim_fastq_piece_words: bad arguments")
        return a.value, b.value, c.value

    def fastq_carry_device_async(self, prev_workspace_ptr, input, prev_text_ptr, prev_bytes, next_text_ptr, room, words_ptr,
                                 chunk_bytes=0, chunk_bytes_dev_ptr=None, chunk_valid_dev_ptr=None, prev_words_ptr=None,
                                 other_prev_words_ptr=None, stream=None):
        """sk_fastq_carry_device_async on raw device pointers (words: a FastqCarryWords in device memory)."""
        self._check(lib().sk_fastq_carry_device_async(self._h, prev_workspace_ptr, input, prev_text_ptr, prev_bytes,
                                                      next_text_ptr, room, chunk_bytes_dev_ptr, chunk_bytes,
                                                      chunk_valid_dev_ptr, prev_words_ptr, other_prev_words_ptr, words_ptr,
                                                      stream))

    def trim_fastq_stream(self, params, chunks, chunks2=None, mode="se", piece_bytes=64 << 20, room=None, gz=False,
                          search=False, max_read_len=0, order=None, batch_capacity=None, report=False, audit=False, bases=False,
                          rejects=False, adapters=False, clip_adapters=None):
        """FASTQ text of any length on the host -> trimmed FASTQ text, piece by piece (sk_trim_fastq_piece_device_async
        and sk_fastq_carry_device_async) on the current stream.  chunks (chunks2 for mode "pe_split"): a bytes-like object
        or an iterable of bytes-like objects of any sizes; they are re-cut into pieces of piece_bytes.  Returns a
        FastqStream: iterating it yields, per piece, the tuple of the three outputs as bytes (None where the mode has no
        such output); with gz=True each is a run of BGZF members, and only the last piece's carries the EOF member, so the
        concatenation per output is one valid .gz file.  Afterwards .counts holds the summed counts (tail_lines and
        dropped_unpaired are the last piece's) and .pieces the number of pieces; .device_bytes is what the driver
        allocated, a function of piece_bytes and room alone: two text buffers per input, two workspaces, two sets of
        outputs sized by the one-pass rule (and of images and writer workspaces), all reused.
        Piece k + 1 is enqueued before piece k is finished and drained.  room (default piece_bytes, rounded up to 16) is
        the longest carry: a record longer than it (or, in "pe_split", inputs that drift apart by more) ends the stream
        with TrimError (SK_ESPACE) that names room.  A format or range error raises FormatError / RangeError at the first
        failing piece, with stream-wide record / read numbers.  Unlike trim_fastq, a format error does not beat a range
        error in an EARLIER piece: pieces are framed one by one, as the reference frames batch by batch.
        order=(threads, batch_len): the records in the order the reference writes them at -a threads with its reader's
        byte budget batch_len, as trim_fastq(order=) gives them on the whole text (sk_trim_fastq_ordered_piece_device_async:
        every piece takes the batches it can tell, two states on the device alternate).  batch_capacity: the entries of a
        piece's batch table, by default (room + piece_bytes) // batch_len + 16; a full table only makes a shorter piece, and
        behind a closing piece whose table was full further closing pieces run on the carry alone (with gz=True each of
        them ends in an EOF member, which readers step over).  .counts["order"] holds the summed order counts.  A piece
        must hold a batch: a batch_len that piece_bytes and room cannot hold, or lines that never use the budget up, end the
        stream with TrimError (SK_ESPACE) that names batch_len.  LongLineError counts its line within the piece.  When the
        run ends before the text does (an empty batch, a split mismatch) the stream ends there, as the reference does.
        report=True or dict(len_bins=.., pos_bins=..): sk_trim_fastq_report_device_async is enqueued behind every piece's
        emission, zeroing the report in front of the first piece only; the report of the whole file (trim_fastq's dict)
        is read back once, after the last piece's finish, into .report (None until then, and after a failure).
        audit=True: sk_trim_fastq_audit_device_async likewise behind every piece, over the piece's workspace and its text
        buffers, with the reset in front of the first piece only; the audit of the whole file (trim_fastq's
        counts["audit"]) is read back once into .audit: first_mismatch is the pair's number in the file.
        bases=True or dict(pos_bins=.., gc=True): sk_trim_fastq_bases_device_async likewise behind every piece, over the
        piece's workspace and its text buffers, with the reset in front of the first piece only; the bases of the whole
        file (trim_fastq's counts["bases"]) are read back once into .bases (None until then, and after a failure).
        rejects=True or "pairs": sk_trim_fastq_rejects_device_async behind every piece, over the piece's workspace and its
        text buffers before they rotate, into two more output buffers (and, with gz=True, images and writer workspaces)
        that .device_bytes includes.  Every yielded tuple gains a fourth entry, the piece's rejects as bytes: the records
        of the reads the piece did not keep ("pairs": both mates of every pair with such a mate), the input's own four
        lines, in read order also with order=; with gz=True BGZF members written through the call's output words, of which
        only the last piece's carry the EOF member.  The entries concatenated are the rejects of the whole file.  .rejects
        holds the summed records and bytes after the last piece (None until then, and after a failure).
        adapters=dict(seqs=[..], ..) as trim_fastq's, without clip: sk_trim_fastq_adapters_device_async behind every piece,
        over the piece's workspace and its text buffers, with the reset in front of the first piece only; the struct and
        the histograms of the whole file are read back once into .adapters (None until then, and after a failure).
        clip_adapters=dict(seqs=[..], ..) as trim_fastq's, without clip: every piece is the clipped call of its kind
        (sk_trim_fastq_clipped_device_async), and the stats of the whole file are read back once into .clip (None until then,
        and after a failure).  None: the pieces are the calls they were, and nothing is allocated."""
        side = _SideCalls("cuda", False, mode, report, audit, bases, rejects, adapters, clip_adapters)
        srcs = [_TextSource(chunks)] + ([] if chunks2 is None else [_TextSource(chunks2)])
        return FastqStream(self, params, srcs, mode, piece_bytes, room, gz, search, max_read_len, order, batch_capacity, side)

    def trim_gz_stream(self, params, image, image2=None, mode="se", piece_bytes=64 << 20, room=None, gz=True, search=False,
                       max_read_len=0, order=None, batch_capacity=None, report=False, audit=False, bases=False, rejects=False,
                       adapters=False, clip_adapters=None):
        """trim_fastq_stream for BGZF image(s) on the host (bytes-like): the host walks the members' BSIZE fields and cuts
        each image into groups of whole members of at most piece_bytes of text (ISIZE sums; piece_bytes >= 65536), every
        group is uploaded and inflated by sk_bgzf_inflate_device_async straight behind the carry, and the reader's device
        words give the carry the chunk's length and validity.  Raises GzDataError for a bad group (member numbers and
        offsets count within the group) and what trim_fastq_stream raises.  Plain gzip cannot be cut at members: ValueError
        (use trim_gz).  order, batch_capacity, report, audit, bases, rejects, adapters, clip_adapters: as in
        trim_fastq_stream."""
        side = _SideCalls("cuda", False, mode, report, audit, bases, rejects, adapters, clip_adapters)
        srcs = [_BgzfSource(image, piece_bytes)] + ([] if image2 is None else [_BgzfSource(image2, piece_bytes)])
        return FastqStream(self, params, srcs, mode, piece_bytes, room, gz, search, max_read_len, order, batch_capacity, side)

    def trim_gzip_stream(self, params, image, image2=None, mode="se", piece_bytes=64 << 20, window_bytes=None, room=None, gz=True,
                         search=False, max_read_len=0, order=None, batch_capacity=None, report=False, audit=False, bases=False,
                         rejects=False, adapters=False, clip_adapters=None):
        """trim_gz_stream for ANY gzip image (bytes or uint8 arrays on the host; plain gzip, what gzip, pigz and zlib
        write, and BGZF too): a FastqStream.  Each image is uploaded once, whole (device_bytes includes it: the memory
        depends on the piece size and on the COMPRESSED file's size, not on the text's), and read by one
        sk_gzip_inflate_piece_device_async per FASTQ piece, straight in front of the carry, over window_bytes of the
        image and into at most the text that FASTQ piece may take.  window_bytes defaults to piece_bytes // 3, a guess at
        FASTQ's compression ratio and not a measurement: a smaller window only makes shorter pieces.  A piece whose first
        deflate block does not end inside the window raises GzDataError naming window_bytes, one whose first stretch holds
        more text than the piece may take raises TrimError naming piece_bytes (split inputs are steered down to half a
        piece, so piece_bytes of twice the largest stretch's text is enough); neither is retried.  The host learns of
        the stream's end from a finished reader piece, so the last FASTQ piece is an empty closing one.  order,
        batch_capacity, report, audit, bases, rejects, adapters, clip_adapters: as in trim_fastq_stream."""
        side = _SideCalls("cuda", False, mode, report, audit, bases, rejects, adapters, clip_adapters)
        window = max(piece_bytes // 3, 1) if window_bytes is None else window_bytes
        sources = [_GzipPieceSource(im, window, piece_bytes) for im in ([image] if image2 is None else [image, image2])]
        st = FastqStream(self, params, sources, mode, piece_bytes, room, gz, search, max_read_len, order, batch_capacity, side)
        st.device_bytes += sum(s.device_bytes for s in sources)
        return st

    @staticmethod
    def trim_fastq_ordered_batches(workspace_ptr):
        """sk_trim_fastq_ordered_batches -> the device address of the table of first units (batches + 1 entries)."""
        t = C.c_void_p()
        if lib().sk_trim_fastq_ordered_batches(workspace_ptr, C.byref(t)) != SK_OK:
            raise SickleError("sk_trim_fastq_ordered_batches: bad arguments")
        return t.value

    @staticmethod
    def _order_tables(order, sizes):
        """order = (threads, batch_len) -> the FastqOrder of the first call, and of the second one if the first one's
        table was too small: a batch holds four lines at least, so an input of b bytes has b / 4 + 1 batches at most."""
        threads, batch_len = order
        return [FastqOrder(threads, 0, batch_len, cap, 0) for cap in (sum(sizes) // batch_len + 16, max(sizes) // 4 + 2)]

    def _with_batch_table(self, order, sizes, call, side):
        """call(FastqOrder or None); once more with the larger table if the first one was too small, behind side.rewind():
        side is the _SideCalls the call uses in both runs"""
        if order is None:
            return call(None)
        first, second = self._order_tables(order, sizes)
        try:
            return call(first)
        except TrimError as e:
            # only the trim's own SK_ESPACE for the batch table is retried: a reader's (its counts have no "order") goes up
            if e.rc != SK_ESPACE or "order" not in e.counts or e.counts["order"]["batches"] != first.batch_capacity + 1 or \
                    second.batch_capacity <= first.batch_capacity:
                raise
        side.rewind()
        return call(second)

    def trim_fastq(self, params, text, text2=None, mode="se", max_read_len=0, record_index=False, order=None, report=False,
                   audit=False, bases=False, rejects=False, adapters=False, clip_adapters=None):
        """FASTQ text in device memory (uint8 torch tensors; text2 for mode "pe_split") -> trimmed FASTQ text, on the
        current stream.  A count-only pass sizes the outputs, a second one writes them.  Returns (outputs, counts):
        three entries, None where the mode has no such output, each a uint8 tensor narrowed to its bytes, or with
        record_index=True a pair (text, index) with the read number of each record (int64).  Raises FormatError,
        RangeError or TrimError.
        mode "pe_combo_all" (sickle's -M, SK_TRIM_PE_COMBO_ALL): an interleaved text in, every pair out in output 0, a mate
        that is not kept as its name line and N / + / the lowest quality byte; every driver below takes it too.
        order=(threads, batch_len): the records in the order the reference writes them at -a threads with its reader's
        byte budget batch_len (sk_trim_fastq_ordered_device_async); counts then has the order counts under "order", and
        LongLineError may be raised.  A batch table that was too small shows in the count-only pass, which is then
        repeated once with the larger table; the writing pass runs once, with the table that fitted, so nothing is
        written twice.  order=None: read order, the -a 1 order.
        report=True or dict(len_bins=.., pos_bins=..): the trim report of the writing pass (sk_trim_fastq_report_device_async,
        enqueued behind it) is returned as a third entry, a dict of sk_fastq_report's members and, for the bins given, the
        histograms as uint64 arrays; summary_text(report, mode) gives the reference's closing lines.  report=False: the
        call is what it was, to the launch.
        audit=True: the audit of the writing pass (sk_trim_fastq_audit_device_async, enqueued behind it, over its workspace
        and the texts) is returned as counts["audit"]: sk_fastq_audit's members as ints (first_mismatch and qual_min are
        AUDIT_NONE where there is none) and qual_hist, 256 ints; qualtypes_consistent(counts["audit"]) names the quality
        types its bytes allow.  Nothing raises on a mismatch.  audit=False: the call is what it was, to the launch.
        bases=True or dict(pos_bins=.., gc=True): the bases of the writing pass (sk_trim_fastq_bases_device_async, enqueued
        behind it, over its workspace and the texts) are returned as counts["bases"]: sk_fastq_bases's members as ints
        (bases_in and bases_out: six, in the order of BASES_CLASSES) and, where asked for, pos_in and pos_out as uint64
        arrays of shape (6, pos_bins) and gc_in and gc_out of 101.  bases=False: the call is what it was, to the launch.
        rejects=True or "pairs": the records of the reads that were not kept (sk_trim_fastq_rejects_device_async; "pairs":
        both mates of every pair with such a mate, SK_FQ_REJECTS_PAIRS), the input's own four lines, in read order.  A
        counting rejects call behind the counting pass sizes the buffer, the writing one goes behind the writing pass and
        in front of its finish.  counts["rejects"] = {"text": uint8 tensor, "index": int64 tensor of read numbers (None
        without record_index=True), "records", "bytes", "reads"}.  rejects=False: the call is what it was, to the launch.
        adapters=dict(seqs=[..], min_overlap=3, max_mismatch_permille=100, pos_bins=None, overlap=False, clip=False): the
        3' adapter search of the writing pass (sk_trim_fastq_adapters_device_async, enqueued behind it, over its workspace
        and the texts) is returned as counts["adapters"]: sk_fastq_adapters's members as ints (hits: eight) and, where
        asked for, pos as a uint64 array of shape (8, pos_bins) and overlap of shape (8, 65); with clip=True also clip, an
        int64 tensor on the device with every read's clip point (-1: no hit), and adapter, the hit's adapter likewise.
        Nothing acts on the result.  adapters=False: the call is what it was, to the launch, and nothing is allocated.
        clip_adapters=dict(seqs=[..], min_overlap=3, max_mismatch_permille=100, clip=False): both passes are the clipped
        call (sk_trim_fastq_clipped_device_async): every read is clipped at its 3' adapter hit in front of the quality
        trim, and everything above describes the clipped reads.  counts["clip"] holds sk_fastq_clip_stats's members of the
        writing pass as ints (hits: eight); with clip=True also clip and adapter, int64 tensors as adapters=dict(clip=True)'s.
        None: nothing is launched, nothing extra is allocated, and the calls are the ones they were."""
        side = _SideCalls(text.device, True, mode, report, audit, bases, rejects, adapters, clip_adapters)
        texts = [text] if text2 is None else [text, text2]
        return self._with_batch_table(order, [t.numel() for t in texts],
                                      lambda o: self._trim_fastq(params, texts, mode, max_read_len, record_index, o, side), side)

    def _text_async(self, params, ptrs, sizes, order, outs, workspace_ptr, workspace_bytes, **kw):
        """a driver's whole-text call: trim_fastq_device_async, or with order (a FastqOrder) the ordered one"""
        if order is None:
            return self.trim_fastq_device_async(params, ptrs, sizes, outs, workspace_ptr, workspace_bytes, **kw)
        return self.trim_fastq_ordered_device_async(params, ptrs, sizes, order, outs, workspace_ptr, workspace_bytes, **kw)

    def _text_finish(self, order, workspace_ptr, stream):
        """the finish of _text_async's call, and of the chained call of that order"""
        finish = self.trim_fastq_device_finish if order is None else self.trim_fastq_ordered_device_finish
        return finish(workspace_ptr, stream)

    def _trim_fastq(self, params, texts, mode, max_read_len, record_index, order, side):
        import torch
        dev = texts[0].device
        ptrs, sizes = _text_ptrs(texts)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = _fastq_ws_bytes(sizes, params.trunc_n, order, side.clp)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        rejects, rws, rej_out = side.rej_flags is not None, None, [None]
        if rejects:
            rws = torch.empty(lib().sk_trim_fastq_rejects_workspace_bytes(sum(sizes)), dtype=torch.uint8, device=dev)

        def run(outs, final=False):
            self._text_async(params, ptrs, sizes, order, outs, ws.data_ptr(), ws_bytes, mode=mode, max_read_len=max_read_len,
                             stream=stream, clip=side.clp)
            # the report, the audit and the bases go behind the writing pass's emission and in front of its finish, which
            # is the wait; the rejects: a counting call behind the counting pass, the writing one behind the writing pass
            side.enqueue(self, ws.data_ptr(), ptrs, sizes, params.trunc_n, "plain", order, True, stream, writing=final,
                         rejects_ws=rws, rejects_out=rej_out[0])
            return self._text_finish(order, ws.data_ptr(), stream)
        counts = run([FastqOutput() for _ in range(3)])
        if rejects:
            need = self.trim_fastq_rejects_device_finish(rws.data_ptr(), stream)
            rej_text = torch.empty(max(need["bytes"], 16), dtype=torch.uint8, device=dev)
            rej_idx = torch.empty(max(need["records"], 1), dtype=torch.int64, device=dev) if record_index else None
            rej_out[0] = FastqOutput(rej_text.data_ptr(), need["bytes"], rej_idx.data_ptr() if record_index else None,
                                     need["records"])
        used = TRIM_OUTPUTS[mode]
        bufs, outs = [None] * 3, [FastqOutput() for _ in range(3)]
        for o in used:
            R, B = counts["records"][o], counts["bytes"][o]
            t = torch.empty(max(B, 16), dtype=torch.uint8, device=dev)
            idx = torch.empty(max(R, 1), dtype=torch.int64, device=dev) if record_index else None
            bufs[o] = (t, idx)
            outs[o] = FastqOutput(t.data_ptr(), B, idx.data_ptr() if record_index else None, R)
        if side.adp and side.adp.want_clip:  # the counting pass has told the reads: a record of each input is a read at most
            side.adp.with_clip(sum(counts["records_in"]))
        counts = run(outs, True)
        res = [None] * 3
        for o in used:
            t, idx = bufs[o]
            R, B = counts["records"][o], counts["bytes"][o]
            res[o] = (t[:B], idx[:R]) if record_index else t[:B]
        report = side.collect(counts)  # every call zeroed the clip stats first: they are the writing pass's
        if side.clp and side.clp.want_clip:  # the words lie in the workspace: a copy that outlives it
            at = side.clp.words_ptr - ws.data_ptr()
            counts["clip"]["clip"], counts["clip"]["adapter"] = \
                _decode_clip_words(ws[at:at + 4 * counts["clip"]["reads"]].view(torch.int32))
        if rejects:
            got = self.trim_fastq_rejects_device_finish(rws.data_ptr(), stream)
            counts["rejects"] = {"text": rej_text[:got["bytes"]], "index": rej_idx[:got["records"]] if record_index else None,
                                 "records": got["records"], "bytes": got["bytes"], "reads": got["reads"]}
        return (tuple(res), counts) if report is None else (tuple(res), counts, report)

    # ---- BGZF on the device -------------------------------------------------------------------
    def bgzf_device_async(self, text_ptr, text_bytes, out_ptr, capacity, workspace_ptr, workspace_bytes, eof=True,
                          bytes_dev_ptr=None, valid_dev_ptr=None, stream=None, search=False):
        """sk_bgzf_device_async on raw device pointers: text_bytes is the text's length, or with bytes_dev_ptr its bound.
        search: SK_BGZF_SEARCH (the workspace then holds sk_bgzf_workspace_bytes_flags bytes)."""
        inp = BgzfInput(text_ptr, text_bytes, bytes_dev_ptr, valid_dev_ptr)
        flags = (SK_BGZF_EOF if eof else 0) | (SK_BGZF_SEARCH if search else 0)
        self._check(lib().sk_bgzf_device_async(self._h, C.byref(inp), out_ptr, capacity, flags, workspace_ptr, workspace_bytes,
                                               stream))

    def bgzf_device_finish(self, workspace_ptr, stream=None):
        """sk_bgzf_device_finish -> counts (dict); raises TrimError (with .counts) on SK_ESPACE."""
        c = BgzfCounts()
        rc = lib().sk_bgzf_device_finish(self._h, workspace_ptr, stream, C.byref(c))
        if rc == SK_ESPACE:
            raise TrimError("bgzf failed (%d): %s" % (rc, lib().sk_last_error(self._h).decode()), rc, c.as_dict())
        self._check(rc)
        return c.as_dict()

    def bgzf(self, text, eof=True, search=False):
        """Text in device memory (a uint8 torch tensor) -> its BGZF image (a uint8 tensor, a valid .gz file as it stands),
        on the current stream.  search: encode with the match search (SK_BGZF_SEARCH): a smaller image, a slower call."""
        import torch
        dev, n = text.device, text.numel()
        stream = torch.cuda.current_stream(dev).cuda_stream
        cap = lib().sk_bgzf_bound(n, SK_BGZF_EOF if eof else 0)
        ws_bytes = lib().sk_bgzf_workspace_bytes_flags(n, SK_BGZF_SEARCH if search else 0)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        out = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
        self.bgzf_device_async(text.data_ptr() if n else None, n, out.data_ptr(), cap, ws.data_ptr(), ws_bytes, eof=eof,
                               stream=stream, search=search)
        return out[:self.bgzf_device_finish(ws.data_ptr(), stream)["bytes_out"]]

    def trim_fastq_gz(self, params, text, text2=None, mode="se", max_read_len=0, order=None, search=False, report=False,
                      audit=False, bases=False, adapters=False, clip_adapters=None):
        """FASTQ text in device memory -> the trimmed texts as BGZF images (.fastq.gz files as they stand), in one pass on
        the current stream: the outputs are sized by the inputs (fastq_output_bound: a trimmed text never exceeds them by more
        than one newline each, and by one byte per record in mode "pe_combo_all"), every produced output's image is enqueued behind the trim, fed by the trim's device words, and
        only then does anything wait.  Returns (images, counts) like trim_fastq; raises what it raises.  order: as
        trim_fastq's (a batch table that was too small is seen at the end only: the pass then runs once more).  search:
        as bgzf's.  report: as trim_fastq's, a third entry.  audit: as trim_fastq's, counts["audit"].  bases: as
        trim_fastq's, counts["bases"].  adapters: as trim_fastq's, counts["adapters"], without clip.  clip_adapters: as
        trim_fastq's, counts["clip"], without clip."""
        side = _SideCalls(text.device, False, mode, report, audit, bases, False, adapters, clip_adapters)
        return self._trim_fastq_gz(params, [text] if text2 is None else [text, text2], mode, max_read_len, order, search, side)

    def _trim_fastq_gz(self, params, texts, mode, max_read_len, order, search, side):
        """trim_fastq_gz behind its keywords; order: the pair, or None"""
        return self._with_batch_table(order, [t.numel() for t in texts],
                                      lambda o: self._trim_fastq_gz_pass(params, texts, mode, max_read_len, o, search, side), side)

    def _trim_fastq_gz_pass(self, params, texts, mode, max_read_len, order, search, side):
        import torch
        dev = texts[0].device
        ptrs, sizes = _text_ptrs(texts)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = _fastq_ws_bytes(sizes, params.trunc_n, order, side.clp)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        writers = _Writers(TRIM_OUTPUTS[mode], fastq_output_bound(sum(sizes), mode), search, _alloc_on(dev))
        self._text_async(params, ptrs, sizes, order, writers.outs, ws.data_ptr(), ws_bytes, mode=mode, max_read_len=max_read_len,
                         stream=stream, clip=side.clp)
        side.enqueue(self, ws.data_ptr(), ptrs, sizes, params.trunc_n, "plain", order, True, stream)
        writers.enqueue(self, ws.data_ptr(), stream)
        res = writers.finish(self, stream)
        counts = self._text_finish(order, ws.data_ptr(), stream)
        report = side.collect(counts)
        return (res, counts) if report is None else (res, counts, report)

    # ---- BGZF read on the device --------------------------------------------------------------
    def bgzf_inflate_device_async(self, image_ptr, image_bytes, out_ptr, capacity, workspace_ptr, workspace_bytes, stream=None):
        """sk_bgzf_inflate_device_async on raw device pointers; out_ptr None with capacity 0 only counts."""
        self._check(lib().sk_bgzf_inflate_device_async(self._h, image_ptr, image_bytes, out_ptr, capacity, workspace_ptr,
                                                       workspace_bytes, stream))

    def bgzf_inflate_device_finish(self, workspace_ptr, stream=None):
        """sk_bgzf_inflate_device_finish -> counts (dict); raises GzDataError, or TrimError (with .counts) on SK_ESPACE."""
        c = BgzfInflateCounts()
        rc = lib().sk_bgzf_inflate_device_finish(self._h, workspace_ptr, stream, C.byref(c))
        if rc == SK_EDATA:
            raise GzDataError(int(c.error), int(c.error_member), int(c.error_offset), c.as_dict())
        if rc == SK_ESPACE:
            raise TrimError("bgzf inflate failed (%d): %s" % (rc, lib().sk_last_error(self._h).decode()), rc, c.as_dict())
        self._check(rc)
        return c.as_dict()

    def bgunzip(self, image):
        """A BGZF image in device memory (a uint8 torch tensor) -> its text (a uint8 tensor), on the current stream: a
        count-only pass sizes the text, a second one writes it.  Raises GzDataError."""
        import torch
        dev, n = image.device, image.numel()
        stream = torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = lib().sk_bgzf_inflate_workspace_bytes(n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ptr = image.data_ptr() if n else None
        self.bgzf_inflate_device_async(ptr, n, None, 0, ws.data_ptr(), ws_bytes, stream=stream)
        need = self.bgzf_inflate_device_finish(ws.data_ptr(), stream)["bytes_out"]
        out = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        self.bgzf_inflate_device_async(ptr, n, out.data_ptr(), need, ws.data_ptr(), ws_bytes, stream=stream)
        self.bgzf_inflate_device_finish(ws.data_ptr(), stream)
        return out[:need]

    # ---- plain gzip read on the device -------------------------------------------------------
    def gzip_inflate_device_async(self, image_ptr, image_bytes, out_ptr, capacity, workspace_ptr, workspace_bytes, stream=None):
        """sk_gzip_inflate_device_async on raw device pointers; out_ptr None with capacity 0 only counts."""
        self._check(lib().sk_gzip_inflate_device_async(self._h, image_ptr, image_bytes, out_ptr, capacity, workspace_ptr,
                                                       workspace_bytes, stream))

    def gzip_inflate_device_finish(self, workspace_ptr, stream=None):
        """sk_gzip_inflate_device_finish -> counts (dict); raises GzDataError, or TrimError (with .counts) on SK_ESPACE."""
        c = GzipInflateCounts()
        rc = lib().sk_gzip_inflate_device_finish(self._h, workspace_ptr, stream, C.byref(c))
        if rc == SK_EDATA:
            raise GzDataError(int(c.error), int(c.error_member), int(c.error_offset), c.as_dict())
        if rc == SK_ESPACE:
            raise TrimError("gzip inflate failed (%d): %s" % (rc, lib().sk_last_error(self._h).decode()), rc, c.as_dict())
        self._check(rc)
        return c.as_dict()

    def gunzip(self, image):
        """Any gzip image in device memory (a uint8 torch tensor) -> its text (a uint8 tensor), on the current stream: a
        count-only pass sizes the text, a second one writes it.  Raises GzDataError."""
        import torch
        dev, n = image.device, image.numel()
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = image.data_ptr() if n else None
        ws_bytes = lib().sk_gzip_inflate_workspace_bytes(n, 0)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        self.gzip_inflate_device_async(ptr, n, None, 0, ws.data_ptr(), ws_bytes, stream=stream)
        need = self.gzip_inflate_device_finish(ws.data_ptr(), stream)["bytes_out"]
        del ws
        ws_bytes = lib().sk_gzip_inflate_workspace_bytes(n, need)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        self.gzip_inflate_device_async(ptr, n, out.data_ptr(), need, ws.data_ptr(), ws_bytes, stream=stream)
        self.gzip_inflate_device_finish(ws.data_ptr(), stream)
        return out[:need]

    # ---- plain gzip read on the device, in pieces -----------------------------------------------
    def gzip_inflate_piece_device_async(self, image_ptr, image_bytes, state_in_ptr, state_out_ptr, out_ptr, capacity, workspace_ptr,
                                        workspace_bytes, window_bytes, image_offset=0, last=True, stream=None, reserved=0):
        """sk_gzip_inflate_piece_device_async on raw device pointers."""
        piece = GzipPiece(image_offset, window_bytes, int(bool(last)), reserved)
        self._check(lib().sk_gzip_inflate_piece_device_async(self._h, image_ptr, image_bytes, C.byref(piece), state_in_ptr,
                                                             state_out_ptr, out_ptr, capacity, workspace_ptr, workspace_bytes, stream))

    def gzip_inflate_piece_device_finish(self, workspace_ptr, stream=None, window_bytes=None, capacity=None):
        """sk_gzip_inflate_piece_device_finish -> counts (dict: the reader's counts and the piece's).  Raises GzDataError
        (.counts["window_limited"]: the failure may be the window's end; the message then names window_bytes), or
        TrimError (with .counts) on SK_ESPACE: the capacity, which a driver derives from piece_bytes, is less than the
        piece's first stretch needs."""
        c, pc = GzipInflateCounts(), GzipPieceCounts()
        rc = lib().sk_gzip_inflate_piece_device_finish(self._h, workspace_ptr, stream, C.byref(c), C.byref(pc))
        counts = dict(c.as_dict(), **pc.as_dict())
        if rc == SK_EDATA:
            e = GzDataError(int(c.error), int(c.error_member), int(c.error_offset), counts)
            if pc.window_limited:
                e.args = ("%s; the piece's window ends before its first block does: window_bytes=%s may be too small"
                          % (e.args[0], window_bytes),)
            raise e
        if rc == SK_ESPACE:
            raise TrimError("gzip piece: its first stretch holds %d bytes of text, beyond the capacity%s: piece_bytes is too small"
                            % (counts["bytes_out"], "" if capacity is None else " of %d" % capacity), rc, counts)
        self._check(rc)
        return counts

    def gunzip_stream(self, image, window_bytes=16 << 20, text_capacity=None):
        """Any gzip image in device memory (a uint8 torch tensor) -> an iterator over its text, piece by piece (uint8
        tensors; each is valid, for work on the current stream, until the next is asked for): sk_gzip_inflate_piece_device_async over windows of
        window_bytes of the image, each piece's text at most text_capacity bytes (default: 4 * window_bytes, a guess at
        FASTQ's ratio and not a measurement; a piece ends earlier where the capacity says so).  The next piece is enqueued
        before the previous one is finished: two workspaces, two text buffers and two states alternate, and the state
        stays on the device.  Raises GzDataError (a window_limited failure is not retried: pass a larger window_bytes),
        or TrimError when text_capacity is less than one stretch needs."""
        import torch
        dev, n = image.device, image.numel()
        stream = torch.cuda.current_stream(dev).cuda_stream
        cap = 4 * window_bytes if text_capacity is None else text_capacity
        ws_bytes = lib().sk_gzip_inflate_piece_workspace_bytes(window_bytes, cap)
        ws = [torch.empty(ws_bytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        out = [torch.empty(max(cap, 16), dtype=torch.uint8, device=dev) for _ in range(2)]
        states = torch.zeros((2, SK_GZIP_PIECE_STATE_BYTES), dtype=torch.uint8, device=dev)
        ptr = image.data_ptr() if n else None

        def enqueue(k):
            s = k & 1
            self.gzip_inflate_piece_device_async(ptr, n, states[s].data_ptr(), states[s ^ 1].data_ptr(), out[s].data_ptr(), cap,
                                                 ws[s].data_ptr(), ws_bytes, window_bytes, stream=stream)

        enqueue(0)
        k = 0
        while True:
            enqueue(k + 1)  # from the state piece k publishes; void if k fails, empty if k ends the stream
            counts = self.gzip_inflate_piece_device_finish(ws[k & 1].data_ptr(), stream, window_bytes, cap)
            if counts["bytes_out"]:
                yield out[k & 1][:counts["bytes_out"]]
            if counts["done"]:
                torch.cuda.current_stream(dev).synchronize()  # piece k + 1, empty, still reads its buffers
                return
            k += 1

    def _gunzip_any(self, image):
        """bgunzip, and for an image the BGZF reader refuses at member 0 although it begins as gzip does, gunzip"""
        try:
            return self.bgunzip(image)
        except GzDataError as e:
            if (e.reason, e.member) != (SK_GZ_HEADER, 0) or image[:3].cpu().tolist() != [0x1f, 0x8b, 8]:
                raise
        return self.gunzip(image)

    @staticmethod
    def bgzf_inflate_output_words(workspace_ptr):
        """sk_bgzf_inflate_output_words -> (bytes_dev, written_dev) device addresses of a BGZF reader's call."""
        b, w = C.c_void_p(), C.c_void_p()
        if lib().sk_bgzf_inflate_output_words(workspace_ptr, C.byref(b), C.byref(w)) != SK_OK:
            raise SickleError("sk_bgzf_inflate_output_words: bad arguments")
        return b.value, w.value

    @staticmethod
    def gzip_inflate_output_words(workspace_ptr):
        """sk_gzip_inflate_output_words -> (bytes_dev, written_dev) device addresses of a gzip reader's call."""
        b, w = C.c_void_p(), C.c_void_p()
        if lib().sk_gzip_inflate_output_words(workspace_ptr, C.byref(b), C.byref(w)) != SK_OK:
            raise SickleError("sk_gzip_inflate_output_words: bad arguments")
        return b.value, w.value

    @staticmethod
    def _gz_kind(image):
        """"bgzf" for an image whose first member begins 1f 8b 08 04 with B C 02 00 at bytes 12-15, else "gzip" (the gzip
        reader reads BGZF too: a BC subfield that does not come first is slow, not wrong)."""
        head = bytes(image[:16].cpu().tolist())
        return "bgzf" if head[:4] == b"\x1f\x8b\x08\x04" and head[12:16] == b"BC\x02\x00" else "gzip"

    def _trim_gz_chained(self, params, images, capacities, kinds, mode, max_read_len, order, search, side):
        """One pass: a decoding reader call per image into a buffer of its capacity, the chained trim fed by the readers'
        words, the BGZF writers fed by the trim's words, and only then the finishes: readers, writers, trim."""
        import torch
        dev = images[0].device
        stream = torch.cuda.current_stream(dev).cuda_stream
        L = lib()
        texts, readers, nbytes, valid = [], [], [], []
        for image, cap, kind in zip(images, capacities, kinds):
            n = image.numel()
            text = torch.empty(max(cap, 16), dtype=torch.uint8, device=dev)
            if kind == "bgzf":
                rws_bytes = L.sk_bgzf_inflate_workspace_bytes(n)
                run, fin, words = self.bgzf_inflate_device_async, self.bgzf_inflate_device_finish, self.bgzf_inflate_output_words
            else:
                rws_bytes = L.sk_gzip_inflate_workspace_bytes(n, cap)
                run, fin, words = self.gzip_inflate_device_async, self.gzip_inflate_device_finish, self.gzip_inflate_output_words
            rws = torch.empty(max(rws_bytes, 16), dtype=torch.uint8, device=dev)
            run(image.data_ptr() if n else None, n, text.data_ptr(), cap, rws.data_ptr(), rws_bytes, stream=stream)
            b, w = words(rws.data_ptr())
            texts.append(text)
            readers.append((fin, rws))
            nbytes.append(b)
            valid.append(w)
        ws_bytes = _fastq_ws_bytes(capacities, params.trunc_n, order, side.clp)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
        writers = _Writers(TRIM_OUTPUTS[mode], fastq_output_bound(sum(capacities), mode), search, _alloc_on(dev))
        ptrs = [t.data_ptr() for t in texts]
        self.trim_fastq_chained_device_async(params, ptrs, capacities, writers.outs, ws.data_ptr(), ws_bytes,
                                             bytes_dev_ptrs=nbytes, valid_dev_ptrs=valid, mode=mode, order=order,
                                             max_read_len=max_read_len, stream=stream, clip=side.clp)
        side.enqueue(self, ws.data_ptr(), ptrs, capacities, params.trunc_n, "plain", order, True, stream)
        writers.enqueue(self, ws.data_ptr(), stream)
        failed, reader_counts = None, []
        for fin, rws in readers:  # GzDataError, or TrimError (SK_ESPACE) whose counts["bytes_out"] is the need
            try:
                reader_counts.append(fin(rws.data_ptr(), stream))
            except (GzDataError, TrimError) as e:
                failed = failed or e
                reader_counts.append(e.counts)
        if failed is not None:
            try:  # the trim saw an empty text for that image; its finish still reads and clears the stream's error word
                self._text_finish(order, ws.data_ptr(), stream)
            except SickleError:
                pass
            failed.readers = reader_counts  # every image's counts, so that two short capacities are learnt in one call
            raise failed
        res = writers.finish(self, stream)
        counts = self._text_finish(order, ws.data_ptr(), stream)
        report = side.collect(counts)
        return (res, counts) if report is None else (res, counts, report)

    def trim_gz(self, params, image, image2=None, mode="se", max_read_len=0, order=None, search=False, text_capacity=None,
                kind=None, report=False, audit=False, bases=False, adapters=False, clip_adapters=None):
        """.fastq.gz image(s) in device memory, BGZF or plain gzip -> the trimmed texts as BGZF images, every byte of work
        on the device.  Returns what trim_fastq_gz returns; raises GzDataError and what it raises.  order: as
        trim_fastq's (the reference takes batch_len from the compressed file's size).  search: as bgzf's.
        text_capacity=None: two passes: bgunzip (gunzip for plain gzip), each a count-only call, a host wait and a decoding
        call, then trim_fastq_gz on texts whose lengths the host has seen.
        text_capacity given (an int, or a pair for two images: an upper bound on each image's text): one pass with one
        wait at its end.  Each image gets one decoding reader call into a buffer of that capacity,
        sk_trim_fastq_chained_device_async takes the lengths from the readers' device words and the writers theirs from
        the trim's; then the finishes run: the readers' (GzDataError, or TrimError with SK_ESPACE whose
        counts["bytes_out"] is the capacity that image needs: call again with it), the writers', the trim's.  The error
        raised is the first image's that failed; its `readers` attribute lists every image's counts (bytes_out: its need),
        so two short capacities are learnt from one call.  `order` does not change this: only the trim's own SK_ESPACE
        for a batch table that was too small is retried.  Every
        per-read step of the trim is sized by the capacity, so a tight bound is a fast call.  kind: "bgzf" or "gzip"
        names the reader (one value, or a pair); None looks at the first 16 bytes of each image before anything is
        enqueued.  An ordered call whose batch table was too small is seen at the end and the pass runs once more.
        report: as trim_fastq's, a third entry.  audit: as trim_fastq's, counts["audit"].  bases: as trim_fastq's,
        counts["bases"].  adapters: as trim_fastq_gz's, counts["adapters"].  clip_adapters: as trim_fastq_gz's,
        counts["clip"]."""
        side = _SideCalls(image.device, False, mode, report, audit, bases, False, adapters, clip_adapters)
        if text_capacity is not None:
            images = [image] if image2 is None else [image, image2]
            caps = [int(text_capacity)] * len(images) if np.isscalar(text_capacity) else [int(c) for c in text_capacity]
            kinds = list(kind) if isinstance(kind, (tuple, list)) else [kind] * len(images)
            if len(caps) != len(images) or len(kinds) != len(images):
                raise SickleError("trim_gz: text_capacity and kind take one entry per image")
            kinds = [self._gz_kind(im) if k is None else k for im, k in zip(images, kinds)]
            if any(k not in ("bgzf", "gzip") for k in kinds):
                raise SickleError("trim_gz: kind is \"bgzf\", \"gzip\" or None")
            return self._with_batch_table(order, caps, lambda o: self._trim_gz_chained(params, images, caps, kinds, mode,
                                                                                       max_read_len, o, search, side), side)
        texts = [self._gunzip_any(im) for im in ([image] if image2 is None else [image, image2])]
        return self._trim_fastq_gz(params, texts, mode, max_read_len, order, search, side)

    @staticmethod
    def trim_fastq_output_words(fastq_workspace_ptr, output):
        """sk_trim_fastq_output_words -> (bytes_dev, written_dev) device addresses of a trim's output `output`."""
        b, w = C.c_void_p(), C.c_void_p()
        if lib().sk_trim_fastq_output_words(fastq_workspace_ptr, output, C.byref(b), C.byref(w)) != SK_OK:
            raise SickleError("sk_trim_fastq_output_words: bad arguments")
        return b.value, w.value


class _TextSource:
    """bytes-like chunks of any sizes, re-cut on demand"""
    compressed = False
    pieces = False

    def __init__(self, chunks):
        if isinstance(chunks, (bytes, bytearray, memoryview, np.ndarray)):
            chunks = [chunks]
        self._it, self._buf, self._at = iter(chunks), None, 0

    def more(self):
        while self._buf is None or self._at >= len(self._buf):
            try:
                c = next(self._it)
            except StopIteration:
                return False
            self._buf, self._at = (c if isinstance(c, np.ndarray) else np.frombuffer(c, dtype=np.uint8)).reshape(-1), 0
        return True

    def take(self, n):
        """-> up to n bytes (uint8 array) and the text bytes they are"""
        parts, got = [], 0
        while got < n and self.more():
            p = self._buf[self._at:self._at + (n - got)]
            self._at += len(p)
            got += len(p)
            parts.append(p)
        a = np.concatenate(parts) if len(parts) > 1 else (parts[0].copy() if parts else np.zeros(0, np.uint8))
        return a, len(a)  # (a copy: the caller's buffer may be read-only)


class _BgzfSource:
    """a BGZF image on the host, cut into groups of whole members by their BSIZE and ISIZE fields"""
    compressed = True
    pieces = False

    def __init__(self, image, piece_bytes):
        self._im = (image if isinstance(image, np.ndarray) else np.frombuffer(image, dtype=np.uint8)).reshape(-1)
        self._at = 0
        self.group_cap = int(lib().sk_bgzf_bound(piece_bytes, SK_BGZF_EOF)) + 65536  # compressed bytes of a group
        if piece_bytes < 65536:
            raise ValueError("trim_gz_stream: piece_bytes must hold a BGZF member's text (65536)")
        head = self._im[:16].tobytes()
        if len(self._im) and not (head[:4] == b"\x1f\x8b\x08\x04" and head[12:16] == b"BC\x02\x00"):
            raise ValueError("trim_gz_stream: not a BGZF image; plain gzip cannot be cut into pieces, use trim_gz")

    def more(self):
        return self._at < len(self._im)

    def _member(self, at):
        """-> (size, isize) of the member at `at`, or None if it does not frame (the reader will say why)"""
        im = self._im
        if at + 26 > len(im) or im[at:at + 4].tobytes() != b"\x1f\x8b\x08\x04" or im[at + 12:at + 16].tobytes() != b"BC\x02\x00":
            return None
        size = int(im[at + 16]) + (int(im[at + 17]) << 8) + 1
        if size < 26 or at + size > len(im):
            return None
        return size, int.from_bytes(im[at + size - 4:at + size].tobytes(), "little")

    def take(self, n):
        """-> whole members of at most n bytes of text (one at least) and their ISIZE sum.  Bytes that do not frame as
        described above go to the reader as they are, which reports them."""
        start, text = self._at, 0
        while self._at < len(self._im):
            m = self._member(self._at)
            if m is None:
                if self._at == start:
                    self._at = min(len(self._im), start + self.group_cap)
                break
            if self._at > start and (text + m[1] > n or self._at + m[0] - start > self.group_cap):
                break
            self._at += m[0]
            text += m[1]
        return self._im[start:self._at].copy(), text


class _GzipPieceSource:
    """any gzip image, uploaded once and read by sk_gzip_inflate_piece_device_async piece by piece: two states on the
    device alternate, and a reader workspace per FASTQ slot.  The host learns that the stream has ended when a finished
    reader piece says so."""
    compressed = False  # nothing is cut or uploaded per piece
    pieces = True

    def __init__(self, image, window_bytes, piece_bytes):
        import torch
        im = (image if isinstance(image, np.ndarray) else np.frombuffer(image, dtype=np.uint8)).reshape(-1)
        self.n, self.window, self.piece_bytes = len(im), int(window_bytes), int(piece_bytes)
        if self.window < 1:
            raise ValueError("trim_gzip_stream: window_bytes must be positive")
        self.image = torch.from_numpy(im.copy()).cuda() if self.n else None
        self.states = torch.zeros((2, SK_GZIP_PIECE_STATE_BYTES), dtype=torch.uint8, device="cuda")
        self.ws_bytes = lib().sk_gzip_inflate_piece_workspace_bytes(self.window, self.piece_bytes)
        self.ws = [torch.empty(self.ws_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.device_bytes = max(self.n, 0) + self.states.numel() + 2 * self.ws_bytes
        self.k, self.done, self.last_taken, self._cap = 0, False, self.piece_bytes, [0, 0]

    def more(self):
        return not self.done

    def enqueue(self, ctx, slot, out_ptr, capacity, stream):
        ctx.gzip_inflate_piece_device_async(self.image.data_ptr() if self.n else None, self.n, self.states[self.k & 1].data_ptr(),
                                            self.states[(self.k + 1) & 1].data_ptr(), out_ptr, capacity, self.ws[slot].data_ptr(),
                                            self.ws_bytes, self.window, stream=stream)
        self.k += 1
        self._cap[slot] = capacity

    def finish(self, ctx, slot, stream):
        """-> the text bytes the piece took; raises GzDataError (naming window_bytes when the window may be the cause) or
        TrimError (naming piece_bytes)"""
        counts = ctx.gzip_inflate_piece_device_finish(self.ws[slot].data_ptr(), stream, self.window, self._cap[slot])
        self.done = self.done or bool(counts["done"])
        self.last_taken = counts["bytes_out"]
        return counts["bytes_out"]


class FastqStream:
    """What Context.trim_fastq_stream / trim_gz_stream return: an iterator over the pieces' outputs, see there."""

    def __init__(self, ctx, params, sources, mode, piece_bytes, room, gz, search, max_read_len, order, batch_capacity, side):
        """side: the _SideCalls of the entry point's keywords, built in front of the sources"""
        import torch
        if mode not in TRIM_MODES or len(sources) != (2 if mode == "pe_split" else 1):
            raise SickleError("trim_fastq_stream: mode \"pe_split\" takes two inputs, the other modes one")
        if piece_bytes < 1:
            raise ValueError("piece_bytes must be positive")
        self.ctx, self.params, self.src, self.mode = ctx, params, sources, mode
        self.piece_bytes = int(piece_bytes)
        self.room = ((self.piece_bytes if room is None else int(room)) + 15) & ~15
        self.gz, self.search, self.max_read_len = gz, search, max_read_len
        self.used = TRIM_OUTPUTS[mode]
        self.counts = {"records_in": [0, 0], "tail_lines": [0, 0], "dropped_unpaired": 0, "records": [0, 0, 0],
                       "bytes": [0, 0, 0]}
        self.pieces = 0
        L, n_in, dev = lib(), len(sources), "cuda"
        self.device_bytes = 0

        def alloc(n):
            self.device_bytes += max(n, 16)
            return torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
        cap_in = self.room + self.piece_bytes
        self.text = [[alloc(cap_in + 16) for _ in range(2)] for _ in range(n_in)]
        self.order = None
        if order is not None:
            threads, batch_len = order
            cap = cap_in // max(int(batch_len), 1) + 16 if batch_capacity is None else int(batch_capacity)
            self.order = FastqOrder(threads, 0, batch_len, cap, 0)
            self.counts["order"] = {"batches": 0, "units": 0, "last_batch_units": 0, "stopped_on_mismatch": 0}
            self.states = torch.zeros((2, 8), dtype=torch.int64, device=dev)  # two sk_fastq_order_state, alternating
            self.device_bytes += 128
            self.ws_bytes = L.sk_trim_fastq_ordered_piece_workspace_bytes(n_in * cap_in, params.trunc_n, cap)
        else:
            self.ws_bytes = L.sk_trim_fastq_workspace_bytes(n_in * cap_in, params.trunc_n)
        self._side = side  # (its buffers' few words are not in device_bytes)
        self.report = self.audit = self.bases = self.adapters = self.clip = self.rejects = None
        if side.clp:  # every piece's clip section lies behind ITS kind's bytes, which its bounds make no more than these
            self.ws_bytes += L.sk_trim_fastq_clip_extra_bytes(n_in * cap_in)
        self.ws = [alloc(self.ws_bytes) for _ in range(2)]
        # per slot: the outputs sized by the one-pass rule and, with gz, their images and writer workspaces
        self.out = [_Writers(self.used, fastq_output_bound(n_in * cap_in, mode), search, alloc, gz) for _ in range(2)]
        self.words = torch.zeros((n_in, 2, 4), dtype=torch.int64, device=dev)
        self.device_bytes += self.words.numel() * 8
        if sources[0].compressed:
            self.rws_bytes = L.sk_bgzf_inflate_workspace_bytes(sources[0].group_cap)
            self.comp = [[alloc(sources[0].group_cap) for _ in range(2)] for _ in range(n_in)]
            self.rws = [[alloc(self.rws_bytes) for _ in range(2)] for _ in range(n_in)]
        self.stream = torch.cuda.current_stream().cuda_stream
        self._rej = side.rej_flags is not None
        if self._rej:  # a workspace and a text buffer (an image, a writer workspace) per slot, sized by the slot's text buffers
            self._rej_sum = {"records": 0, "bytes": 0}
            self.jws = [alloc(L.sk_trim_fastq_rejects_workspace_bytes(n_in * cap_in)) for _ in range(2)]
            self.jout = [_Writers((0,), L.sk_trim_fastq_rejects_bound(n_in * cap_in), search, alloc, gz) for _ in range(2)]
        self._gen = self._run()

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._gen)

    def _words_ptr(self, i, slot):
        return self.words.data_ptr() + 32 * (2 * i + slot)

    def _enqueue(self, k, carried):
        """upload (and inflate) the next chunk of every input, then carry and piece k (and its writers)"""
        import torch
        c, slot, prev = self.ctx, k & 1, (k - 1) & 1
        n_in = len(self.src)
        bounds, readers, taken = [], [], [0, 0]
        # split inputs: an input that carries more than the other gets that much less text, or the one with the shorter
        # records piles its carry up; of the inputs that still have text the one that carries least gets a whole piece, so
        # the stream always moves on
        active = [carried[i] for i, s in enumerate(self.src) if s.more()]
        least = min(active) if active else 0
        for i, s in enumerate(self.src):
            target = max(self.piece_bytes - max(carried[i] - least, 0), 0)
            buf = self.text[i][slot]
            nb_dev = valid_dev = None
            if s.pieces:  # a reader piece straight to next_text + room, its capacity the text this piece may take
                data, text_bytes, chunk = None, 0, 0
                # an input steered below half a piece sits this piece out (its carry is ahead of the other's): a capacity
                # that small could be less than one stretch's text, which is an error only of piece_bytes itself
                if 2 * target >= self.piece_bytes and not s.done:
                    chunk, text_bytes = target, min(s.last_taken, target)  # in flight: it has not told what it took
                    s.enqueue(c, slot, buf.data_ptr() + self.room, target, self.stream)
                    nb_dev, valid_dev = c.gzip_inflate_output_words(s.ws[slot].data_ptr())
                    readers.append((i, s))
            else:
                data, text_bytes = s.take(target) if target or s.compressed else (np.zeros(0, np.uint8), 0)
            taken[i] = text_bytes
            if s.compressed:
                if text_bytes > self.piece_bytes:
                    raise ValueError("trim_gz_stream: a member holds %d bytes of text, beyond piece_bytes" % text_bytes)
                chunk = self.piece_bytes if len(data) else 0
                if len(data):
                    self.comp[i][slot][:len(data)].copy_(torch.from_numpy(data), non_blocking=False)
                    c.bgzf_inflate_device_async(self.comp[i][slot].data_ptr(), len(data), buf.data_ptr() + self.room, chunk,
                                                self.rws[i][slot].data_ptr(), self.rws_bytes, stream=self.stream)
                    nb_dev, valid_dev = c.bgzf_inflate_output_words(self.rws[i][slot].data_ptr())
                    readers.append((i, self.rws[i][slot]))
            elif not s.pieces:
                chunk = len(data)
                if chunk:
                    buf[self.room:self.room + chunk].copy_(torch.from_numpy(data), non_blocking=False)
            c.fastq_carry_device_async(self.ws[prev].data_ptr() if k else None, i, self.text[i][prev].data_ptr() if k else None,
                                       self._bounds[i] if k else 0, buf.data_ptr(), self.room, self._words_ptr(i, slot),
                                       chunk_bytes=chunk, chunk_bytes_dev_ptr=nb_dev, chunk_valid_dev_ptr=valid_dev,
                                       prev_words_ptr=self._words_ptr(i, prev) if k else None,
                                       other_prev_words_ptr=self._words_ptr(1 - i, prev) if k and n_in == 2 else None,
                                       stream=self.stream)
            bounds.append(self.room + chunk)
        self._bounds = bounds
        more = any(s.more() for s in self.src)
        outs, side = self.out[slot].outs, self._side
        words = dict(bytes_dev_ptrs=[self._words_ptr(i, slot) + 8 for i in range(n_in)],
                     valid_dev_ptrs=[self._words_ptr(i, slot) + 16 for i in range(n_in)],
                     start_dev_ptrs=[self._words_ptr(i, slot) for i in range(n_in)], more=more, mode=self.mode,
                     max_read_len=self.max_read_len, stream=self.stream)
        if side.clp:  # the stats are zeroed in front of the first piece only
            side.clp.reset = k == 0
            words["clip"] = side.clp
        ptrs, ws_ptr = [self.text[i][slot].data_ptr() for i in range(n_in)], self.ws[slot].data_ptr()
        if self.order is None:
            c.trim_fastq_piece_device_async(self.params, ptrs, bounds, outs, ws_ptr, self.ws_bytes, **words)
        else:  # piece k starts from the state piece k - 1 wrote
            c.trim_fastq_ordered_piece_device_async(self.params, ptrs, bounds, self.order, self.states[k & 1].data_ptr(),
                                                    self.states[(k + 1) & 1].data_ptr(), outs, ws_ptr, self.ws_bytes, **words)
        # Behind the piece's emission, over its workspace (whose sections lie where ITS bounds put them, which a short chunk
        # makes less than the workspace's) and the slot's text buffers, which piece k + 2 fills again behind these calls.
        # What accumulates is zeroed in front of the first piece only; the rejects go into the slot's own workspace and text
        # buffer (and through its words into the writer).
        side.enqueue(c, ws_ptr, ptrs, bounds, self.params.trunc_n, "piece", self.order, k == 0, self.stream,
                     rejects_ws=self.jws[slot] if self._rej else None, rejects_out=self.jout[slot].outs[0] if self._rej else None)
        if self._rej and self.gz:
            self.jout[slot].enqueue(c, self.jws[slot].data_ptr(), self.stream, eof=not more, words=c.trim_fastq_rejects_output_words)
        if self.gz:
            self.out[slot].enqueue(c, ws_ptr, self.stream, eof=not more)
        return {"k": k, "slot": slot, "more": more, "readers": readers, "taken": taken}

    def _finish(self, p):
        """wait for piece p, raise what it met, sum its counts; -> (outputs, bytes carried per input)"""
        c, slot = self.ctx, p["slot"]
        for i, rws in p["readers"]:
            if self.src[i].pieces:
                p["taken"][i] = rws.finish(c, slot, self.stream)  # what the piece took, now that it has told
            else:
                c.bgzf_inflate_device_finish(rws.data_ptr(), self.stream)
        rc, raw, counts = self._raw_finish(slot)
        status = [int(x) for x in self.words[:, slot, 3].cpu().tolist()]
        if 2 in status and self.order is not None:
            raise TrimError("fastq stream: input %d carries more than room = %d bytes into piece %d without a batch to take: "
                            "piece_bytes (%d) and room must hold one batch of batch_len = %d bytes (or the text's lines never "
                            "use the budget up)" % (status.index(2), self.room, p["k"], self.piece_bytes,
                                                    self.order.batch_len), SK_ESPACE, counts)
        if 2 in status:
            raise TrimError("fastq stream: input %d carries more than room = %d bytes into piece %d (a longer record, or "
                            "split inputs that drift apart): pass a larger room" % (status.index(2), self.room, p["k"]),
                            SK_ESPACE, counts)
        base_reads = self._reads
        per_input = base_reads // 2 if self.mode == "pe_split" else base_reads
        # stream-wide numbers: the records and reads before the piece (an inherited range error keeps its call's read number)
        c._check_fastq(rc, raw, counts, record_base=per_input, read_base=0 if counts["piece"]["inherited_range"] else base_reads)
        if any(status):
            raise SickleError("fastq stream: piece %d follows a failed carry (status %r)" % (p["k"], status))
        host = lambda t: None if t is None else t.cpu().numpy().tobytes()
        if self.gz:
            res = [host(im) for im in self.out[slot].finish(c, self.stream)]
        else:
            res = [host(t if t is None else t[:counts["bytes"][o]]) for o, t in enumerate(self.out[slot].text)]
        for key in ("records_in", "records", "bytes"):
            self.counts[key] = [a + b for a, b in zip(self.counts[key], counts[key])]
        self.counts["tail_lines"], self.counts["dropped_unpaired"] = counts["tail_lines"], counts["dropped_unpaired"]
        if self.order is not None:
            oc, mine = counts["order"], self.counts["order"]
            mine["batches"] += oc["batches"]
            mine["units"] += oc["units"]
            mine["last_batch_units"] = oc["last_batch_units"] if oc["batches"] else mine["last_batch_units"]
            mine["stopped_on_mismatch"] |= oc["stopped_on_mismatch"]
            self._table_full = bool(counts["order_piece"]["table_full"])
            self._ended = bool(counts["order_piece"]["state"]["ended"])
        self._reads += counts["records_in"][0] * (2 if self.mode == "pe_split" else 1)
        if not p["more"] and self.mode in ("pe_interleaved", "pe_combo_all"):
            self._reads -= counts["dropped_unpaired"]
        self.pieces += 1
        carried = counts["piece"]["carried_bytes"]
        # what the piece consumed of each input: what it was handed (the carry before it and its chunk) less what it carried
        self._known = (p["k"], carried, [a + b - c for a, b, c in zip(self._carried_in, p["taken"], carried)])
        self._carried_in = carried
        if self._rej:
            got = c.trim_fastq_rejects_device_finish(self.jws[slot].data_ptr(), self.stream)
            res.append(host(self.jout[slot].finish(c, self.stream)[0] if self.gz else self.jout[slot].text[0][:got["bytes"]]))
            self._rej_sum["records"] += got["records"]
            self._rej_sum["bytes"] += got["bytes"]
        return tuple(res)

    def _raw_finish(self, slot):
        if self.order is None:
            return self.ctx._piece_finish(self.ws[slot].data_ptr(), self.stream)
        return self.ctx._ordered_piece_finish(self.ws[slot].data_ptr(), self.stream)

    def _eof_members(self, last):
        """what closes the outputs when the run ended in a piece that was not a closing one"""
        if not self.gz or not last["more"]:
            return []
        return [tuple(BGZF_EOF_MEMBER if o in self.used else None for o in range(3)) + ((BGZF_EOF_MEMBER,) if self._rej else ())]

    def _estimate(self, last):
        """bytes each input carries into the piece behind piece `last` (enqueued): what the last finished piece carried,
        and, if that is the piece before `last`, plus last's chunk less what the finished piece consumed (the steady
        state's consumption: a piece in flight has not told yet)"""
        k, carried, consumed = self._known
        if k == last["k"]:
            return carried
        return [max(c + t - u, 0) for c, t, u in zip(carried, last["taken"], consumed)]

    def _run(self):
        yield from self._run_pieces()
        got = {}  # every piece has been finished: the stream has been waited for
        self.report = self._side.collect(got)
        self.audit, self.bases, self.adapters, self.clip = [got.get(key) for key in ("audit", "bases", "adapters", "clip")]
        if self._rej:
            self.rejects = dict(self._rej_sum)

    def _run_pieces(self):
        self._reads, self._bounds, self._carried_in, self._known = 0, [0, 0], [0, 0], (-1, [0, 0], [0, 0])
        self._table_full = self._ended = False  # ordered streams: the last finished piece's
        estimate, pending, k = [0, 0], None, 0
        try:
            while True:
                nxt = self._enqueue(k, estimate)
                if pending is not None:
                    done, pending = pending, nxt
                    yield self._finish(done)
                    if self._ended:  # the run is over: the piece in flight takes nothing, and no further one is needed
                        pending = None
                        yield self._finish(nxt)
                        yield from self._eof_members(nxt)
                        return
                pending = nxt
                if not nxt["more"]:
                    break
                if k == 0 and len(self.src) == 2:  # split inputs: piece 1 is sized by what piece 0 carried, not by a guess
                    done, pending = pending, None
                    yield self._finish(done)
                    if self._ended:
                        yield from self._eof_members(done)
                        return
                estimate = self._estimate(nxt) if self._known[0] >= 0 else [0, 0]
                k += 1
            if pending is not None:
                done, pending = pending, None
                yield self._finish(done)
            while self._table_full and not self._ended:  # a closing piece's table was full: go on, on the carry alone
                k += 1
                done = self._enqueue(k, self._carried_in)
                yield self._finish(done)
        finally:
            if pending is not None:  # a piece still in flight behind a failure: wait for it and clear the stream's error word
                for i, rws in pending["readers"]:
                    try:
                        if self.src[i].pieces:
                            rws.finish(self.ctx, pending["slot"], self.stream)
                        else:
                            self.ctx.bgzf_inflate_device_finish(rws.data_ptr(), self.stream)
                    except SickleError:
                        pass
                self._raw_finish(pending["slot"])


BGZF_INPUT = 65280   # bytes of text per BGZF block
BGZF_EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BGZF_SLOT = 65536    # bytes of output slot per block


def bgzf_deflate(data, device=0):
    """sk_bgzf_deflate on a bytes object -> the BGZF file image (framing done here, like the
    writer of the CLI does it).  Tests only."""
    import struct
    import zlib
    n_blocks = max(1, (len(data) + BGZF_INPUT - 1) // BGZF_INPUT)
    text = np.zeros(n_blocks * BGZF_INPUT, dtype=np.uint8)
    text[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    sizes = np.array([min(BGZF_INPUT, len(data) - b * BGZF_INPUT) for b in range(n_blocks)], dtype=np.uint32)
    out = np.zeros(n_blocks * BGZF_SLOT, dtype=np.uint8)
    out_sizes = np.zeros(n_blocks, dtype=np.uint32)
    rc = lib().sk_bgzf_deflate(device, text.ctypes.data, sizes.ctypes.data, n_blocks, out.ctypes.data, out_sizes.ctypes.data)
    if rc != 0:
        raise SickleError("sk_bgzf_deflate: %d %s" % (rc, lib().sk_bgzf_last_error().decode()))
    blob = bytearray()
    for b in range(n_blocks):
        piece = data[b * BGZF_INPUT:b * BGZF_INPUT + int(sizes[b])]
        c = int(out_sizes[b])
        if c == 0 or c >= len(piece) + 5:
            n = len(piece)
            body = bytes([1, n & 0xff, n >> 8, ~n & 0xff, (~n >> 8) & 0xff]) + piece
        else:
            body = out[b * BGZF_SLOT:b * BGZF_SLOT + c].tobytes()
        total = 18 + len(body) + 8
        blob += b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + body
        blob += struct.pack("<II", zlib.crc32(piece) & 0xffffffff, len(piece))
    return bytes(blob)
