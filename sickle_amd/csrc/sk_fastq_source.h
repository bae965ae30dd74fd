// sk_fastq_source.h -- the view of a finished FASTQ text call that every call running behind it takes (the report, audit,
// bases, adapters and rejects calls and the clip commit): where the call's header and sections lie, the
// caller's texts, the bounds of both, whether the call adds, and where a read's descriptor sends it in its text.
//
// The promise of every behind-call is kept here and nowhere else: a source that names the wrong layout or the wrong texts
// gives wrong numbers, no load outside the workspace and the texts.  Every descriptor index is bounded by slot_bound, every
// offset into a text by bytes[i], every read by n_bound, every byte of a packed section by q_bound; a kernel that takes
// its reads from fqs_reads and its text positions from the lookups below needs no clamp of its own.
// No HIP: the kernels call these on the device, sk_launch_* and tests/fastq_source/source_host.cpp on the host.
#ifndef SK_FASTQ_SOURCE_H
#define SK_FASTQ_SOURCE_H

#include <stdint.h>

#include "sickle_amd.h"
#include "sk_fastq_order.h"
#include "sk_fastq_words.h"

#ifdef __HIPCC__
#define FQS_FN __host__ __device__ static inline
#else
#define FQS_FN static inline
#endif

#define FQS_NO_MODE (-1) // fqs_view.mode of a call that has no mode to compare (the report)

struct sk_cut_dev; // sk_device.h

struct fqs_view {
    const uint64_t *hdr;         // the text call's header
    const uint64_t *order_words; // ordered kinds: where the SK_FQO_H_* words lie (the header, or a piece's extension block)
    const uint64_t *desc;        // 5 words per slot, input 0's slots0 slots first
    const uint64_t *offsets;
    const sk_cut_dev *cuts;
    const uint8_t *pq; // the packed qual
    const uint8_t *text[2];
    uint64_t bytes[2];
    uint64_t slots0;     // input 0's slots: input 1's descriptors lie behind them
    uint64_t slot_bound; // slots of the descriptor section
    uint64_t n_bound;    // the most reads the packed batch can hold: N of sk_fq_layout_of, what offsets and cuts are sized by
    uint64_t q_bound;    // bytes of a packed section
    int32_t kind;        // SK_FQ_REPORT_*
    int32_t mode;        // the framing mode of the call behind, or FQS_NO_MODE
};

FQS_FN uint64_t fqs_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
FQS_FN uint64_t fqs_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// SK_TRIM_PE_COMBO_ALL frames, pairs and orders as SK_TRIM_PE_INTERLEAVED: what the text call records in SK_FQ_H_MODE
FQS_FN int fqs_framing_mode(int mode) { return mode == SK_TRIM_PE_COMBO_ALL ? SK_TRIM_PE_INTERLEAVED : mode; }

// The words the validity reads: the header, the order words by kind, the kind and the mode (the call's, or FQS_NO_MODE).
// All the clip commit needs.
static inline void fqs_fill_validity(const void *workspace, uint32_t kind, int mode, fqs_view *v)
{
    const uint8_t *base = static_cast<const uint8_t *>(workspace);
    v->hdr = reinterpret_cast<const uint64_t *>(base);
    v->order_words = nullptr;
    if (kind == SK_FQ_REPORT_ORDERED) v->order_words = v->hdr;
    else if (kind == SK_FQ_REPORT_ORDERED_PIECE) v->order_words = reinterpret_cast<const uint64_t *>(base + SK_FQOP_EXT_BYTES_AT);
    v->kind = (int32_t)kind;
    v->mode = mode == FQS_NO_MODE ? FQS_NO_MODE : fqs_framing_mode(mode);
}

// The whole view of src, which has passed check_source (sk_capi.hip), and of the texts, which have passed check_texts.
// in: NULL = no texts (the report; an audit that does not look at names): text NULL, bytes 0.  A NULL text[i] has 0 bytes;
// text[1] is taken in split framing alone.
// slots0 is by in->bytes[0] as it stands, since that is where the text call put input 1's descriptors (fq_make_args,
// sk_fastq.hip).  Three of the five calls used to take it from the bytes[0] that a NULL text[0] had zeroed: the same
// number, because check_texts refuses a NULL text[0] with bytes[0] != 0 wherever names or bases are read.
static inline void fqs_fill(const sk_fastq_report_source *src, const sk_fastq_input *in, int mode, fqs_view *v)
{
    sk_fq_layout L;
    sk_fq_layout_of(src->text_bytes, src->trunc_n, &L);
    fqs_fill_validity(src->workspace, src->kind, mode, v);
    uint64_t shift = 0;
    if (src->kind == SK_FQ_REPORT_ORDERED) shift = sk_fq_order_shift(src->batch_capacity);
    else if (src->kind == SK_FQ_REPORT_ORDERED_PIECE) shift = sk_fq_order_piece_shift(src->batch_capacity);
    const uint8_t *ws = static_cast<const uint8_t *>(src->workspace) + shift;
    v->desc = reinterpret_cast<const uint64_t *>(ws + L.desc);
    v->offsets = reinterpret_cast<const uint64_t *>(ws + L.offsets);
    v->cuts = reinterpret_cast<const sk_cut_dev *>(ws + L.cuts);
    v->pq = ws + L.qual;
    v->slot_bound = (L.offsets - L.desc) / 40;
    v->n_bound = (L.blocks - L.cuts) / 8;
    v->q_bound = L.seq - L.qual;
    const int n_in = in && v->mode == SK_TRIM_PE_SPLIT ? 2 : in ? 1 : 0;
    for (int i = 0; i < 2; ++i) {
        v->text[i] = i < n_in ? in->text[i] : nullptr;
        v->bytes[i] = i < n_in && in->text[i] ? in->bytes[i] : 0;
    }
    v->slots0 = sk_fq_slots(in ? in->bytes[0] : 0);
}

// ---- validity --------------------------------------------------------------------------------------
// Validity of the call behind a workspace, from its header words.  fmt: SK_FQ_H_FMT; range: SK_FQ_H_RANGE; range0: the
// piece kinds' SK_FQP_H_RANGE0 (~0 for the others); refused: the ordered kinds' long-line word differs from ~0, or the
// ordered call's table overflowed (0 for the others): such a call wrote nothing, as after a format verdict.
FQS_FN bool fqs_call_valid(uint64_t fmt, uint64_t range, uint64_t range0, bool refused)
{
    return fmt == ~0ull && range == ~0ull && range0 == ~0ull && !refused;
}

// whether the call behind the view adds: fqs_call_valid on its words (a void ordered piece, SK_FQOP_X_INHERITED, is
// refused too), and, where the view has a mode, the framing mode the text call recorded
FQS_FN bool fqs_valid(const fqs_view &v)
{
    const uint64_t *h = v.hdr;
    const bool piece = v.kind == SK_FQ_REPORT_PIECE || v.kind == SK_FQ_REPORT_ORDERED_PIECE;
    const uint64_t range0 = piece ? h[SK_FQP_H_RANGE0] : ~0ull;
    bool refused = false;
    if (v.order_words) {
        refused = v.order_words[SK_FQO_H_LONG] != ~0ull || v.order_words[SK_FQO_H_OVERFLOW] != 0;
        if (v.kind == SK_FQ_REPORT_ORDERED_PIECE && v.order_words[SK_FQOP_X_INHERITED]) refused = true; // void
    }
    if (v.mode != FQS_NO_MODE && (int64_t)h[SK_FQ_H_MODE] != (int64_t)v.mode) return false;
    return fqs_call_valid(h[SK_FQ_H_FMT], h[SK_FQ_H_RANGE], range0, refused);
}

// the reads of the call, never more than the sections hold
FQS_FN uint64_t fqs_reads(const fqs_view &v) { return fqs_min(v.hdr[SK_FQ_H_NREAL], v.n_bound); }

// ---- the descriptor lookups ---------------------------------------------------------------------------
// the text read r lies in: in split framing reads 2k and 2k + 1 are record k of text 0 and of text 1
FQS_FN int fqs_input(const fqs_view &v, uint64_t r) { return v.mode == SK_TRIM_PE_SPLIT ? (int)(r & 1) : 0; }

// read r's descriptor slot: 5 words at desc + 5 * *slot, the name line's start and the ends of the record's four lines,
// as offsets in text *i.  false: the section has no slot for it, and desc is not to be indexed.
FQS_FN bool fqs_slot(const fqs_view &v, uint64_t r, int *i, uint64_t *slot)
{
    *i = fqs_input(v, r);
    const uint64_t k = v.mode == SK_TRIM_PE_SPLIT ? r >> 1 : r;
    *slot = (*i ? v.slots0 : 0) + k;
    return *slot < v.slot_bound;
}

// [at, at + len) of a text of `bytes` bytes for two words of a descriptor, a start and an end: that span in a call that
// is valid, and a span inside the text whatever the two words hold
FQS_FN void fqs_span(uint64_t start, uint64_t end, uint64_t bytes, uint64_t *at, uint64_t *len)
{
    const uint64_t a = fqs_min(start, bytes);
    *at = a;
    *len = fqs_max(fqs_min(end, bytes), a) - a;
}

// the name line of read r: its text, bounded by the text's bytes.  false: no descriptor slot for it.
FQS_FN bool fqs_name_line(const fqs_view &v, uint64_t r, const uint8_t *&p, uint64_t &len)
{
    int i;
    uint64_t slot, s;
    if (!fqs_slot(v, r, &i, &slot)) return false;
    const uint64_t *d = v.desc + 5 * slot;
    fqs_span(d[0], d[1], v.bytes[i], &s, &len);
    p = v.text[i] + s;
    return true;
}

// where the seq line of read r starts in its text, never beyond the text; the text's length: no descriptor slot for it
FQS_FN uint64_t fqs_seq_start(const fqs_view &v, uint64_t r)
{
    int i;
    uint64_t slot;
    if (!fqs_slot(v, r, &i, &slot)) return v.bytes[i];
    return fqs_min(fqs_min(v.desc[5 * slot + 1], v.bytes[i]) + 1, v.bytes[i]);
}

// read r's text and its whole record's span in it (without the closing '\n'): through the descriptor slot, or an empty
// span at the text's end where there is none
FQS_FN int fqs_record(const fqs_view &v, uint64_t r, uint64_t *at, uint64_t *len)
{
    int i;
    uint64_t slot;
    uint64_t s0 = 0, e3 = 0;
    if (fqs_slot(v, r, &i, &slot)) {
        s0 = v.desc[5 * slot];
        e3 = v.desc[5 * slot + 4];
    } else {
        s0 = e3 = v.bytes[i];
    }
    fqs_span(s0, e3, v.bytes[i], at, len);
    return i;
}

#endif
