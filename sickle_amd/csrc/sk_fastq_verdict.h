// sk_fastq_verdict.h -- what the finish of a FASTQ text call tells from the workspace's words: the counts, the return code
// and the message, for the four kinds of call (include/sickle_amd.h states each finish's order of precedence).  A plain
// function of integers, no HIP: sk_capi.hip's fastq_finish copies the words back and calls it, and
// tests/fastq_verdict/verdict_host.cpp runs it on the host.
#ifndef SK_FASTQ_VERDICT_H
#define SK_FASTQ_VERDICT_H

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "sickle_amd.h"
#include "sk_fastq_order.h"
#include "sk_fastq_words.h"

// a range-error word (~0 = none) -> SK_OK, or SK_ERANGE with *err (may be NULL) filled
static inline int decode_error(unsigned long long word, sk_err *err)
{
    if (word == ~0ull) return SK_OK;
    if (err) {
        err->read = (uint32_t)(word >> 32);
        err->pos = (uint32_t)((word >> 8) & 0xffffffu);
        err->ch = (int32_t)(int8_t)(word & 0xff);
    }
    return SK_ERANGE;
}

// the kinds of text call: sk_trim_fastq_device_async (and the chained call in read order), .._ordered_.., .._piece_.. and
// .._ordered_piece_..
enum { SK_FQV_PLAIN = 0, SK_FQV_ORDERED = 1, SK_FQV_PIECE = 2, SK_FQV_ORDERED_PIECE = 3 };
static inline bool fqv_is_piece(int kind) { return kind == SK_FQV_PIECE || kind == SK_FQV_ORDERED_PIECE; }
static inline bool fqv_is_ordered(int kind) { return kind == SK_FQV_ORDERED || kind == SK_FQV_ORDERED_PIECE; }

// The range word a kind's finish judges: a piece takes every verdict from its own workspace, so the word its emission
// captured; a whole-text call the stream's live word as it is when finish reads it.
static inline uint64_t fqv_range_word(int kind, const uint64_t *h, uint64_t live)
{
    return fqv_is_piece(kind) ? h[SK_FQ_H_RANGE] : live;
}

// h: the header's SK_FQ_HDR_WORDS words.  x: the order words, at SK_FQO_H_*: h itself for the ordered call, the extension
// block (SK_FQOP_X_* too) for the ordered piece; not read for the other kinds.  range: fqv_range_word.  oc, pc, opc may be
// NULL and are filled only for the kinds that have them.  msg is written only with a return other than SK_OK.
static inline int fqv_verdict(int kind, const uint64_t *h, const uint64_t *x, uint64_t range, sk_fastq_counts *counts,
                              sk_fastq_order_counts *oc, sk_fastq_piece_counts *pc, sk_fastq_order_piece_counts *opc, char *msg,
                              size_t msg_bytes)
{
    const bool piece = fqv_is_piece(kind), ordered = fqv_is_ordered(kind);
    const bool split = h[SK_FQ_H_MODE] == SK_TRIM_PE_SPLIT, interleaved = h[SK_FQ_H_MODE] == SK_TRIM_PE_INTERLEAVED;
    const bool more = piece && h[SK_FQP_H_MORE] != 0, inherited_range = piece && h[SK_FQP_H_RANGE0] != ~0ull;
    const bool inherited = kind == SK_FQV_ORDERED_PIECE && x[SK_FQOP_X_INHERITED] != 0;
    const uint64_t fmt = h[SK_FQ_H_FMT], lng = ordered ? x[SK_FQO_H_LONG] : ~0ull;
    const bool overflow = kind == SK_FQV_ORDERED && x[SK_FQO_H_OVERFLOW] != 0; // (a piece's full table is no error)
    const bool refused = lng != ~0ull || overflow, bad = fmt != ~0ull || refused;
    memset(counts, 0, sizeof *counts);
    for (int i = 0; i < 2; ++i) {
        counts->records_in[i] = h[SK_FQ_H_RECORDS + i];
        // a piece carries whole records too
        counts->tail_lines[i] = piece ? h[SK_FQ_H_LINES + i] - 4 * h[SK_FQ_H_RECORDS + i] : h[SK_FQ_H_LINES + i] & 3;
    }
    // (an ordered call counts the odd record in records_unbatched; a piece with more to come carries it)
    counts->dropped_unpaired = !ordered && !more && interleaved ? (h[SK_FQ_H_RECORDS] & 1) : 0;
    for (int o = 0; o < 3; ++o) {
        counts->records[o] = bad ? 0 : h[SK_FQ_H_OUT_RECORDS + o];
        counts->bytes[o] = bad ? 0 : h[SK_FQ_H_OUT_BYTES + o];
    }
    if (oc && ordered) {
        memset(oc, 0, sizeof *oc);
        oc->batches = x[SK_FQO_H_BATCHES];
        oc->units = x[SK_FQO_H_UNITS];
        oc->last_batch_units = x[SK_FQO_H_LAST_UNITS];
        oc->records_unbatched[0] = x[SK_FQO_H_UNBATCHED];
        oc->records_unbatched[1] = x[SK_FQO_H_UNBATCHED + 1];
        oc->stopped_on_mismatch = (uint32_t)x[SK_FQO_H_MISMATCH];
        // a piece's batch numbers are its own: the stream's are those plus the batches before it
        oc->error_batch = refused || x[SK_FQO_H_ERROR_BATCH] == ~0ull
                              ? UINT64_MAX
                              : (piece ? x[SK_FQOP_X_BASE_BATCHES] : 0) + x[SK_FQO_H_ERROR_BATCH];
        if (lng != ~0ull) {
            oc->long_line_input = (uint32_t)(lng >> 63);
            oc->long_line = lng & ~(1ull << 63);
        }
    }
    if (pc && piece) {
        memset(pc, 0, sizeof *pc);
        for (int i = 0; i < 2; ++i) {
            pc->consumed[i] = h[SK_FQP_H_CONSUMED + i];
            pc->carried_bytes[i] = h[SK_FQP_H_END + i] - h[SK_FQP_H_CONSUMED + i];
        }
        pc->ok = (uint32_t)h[SK_FQP_H_OK];
        pc->inherited_range = inherited_range;
    }
    if (opc && kind == SK_FQV_ORDERED_PIECE) {
        memset(opc, 0, sizeof *opc);
        opc->table_full = (uint32_t)x[SK_FQOP_X_TABLE_FULL];
        opc->undetermined = (uint32_t)x[SK_FQOP_X_UNDETERMINED];
        opc->inherited_failure = inherited;
        memcpy(&opc->state, x + SK_FQOP_X_STATE, sizeof opc->state);
    }
    if (inherited_range) {
        decode_error(h[SK_FQP_H_RANGE0], &counts->range);
        snprintf(msg, msg_bytes, "fastq: an earlier call on the stream left a range error (read %u of that call); the piece took no record",
                 counts->range.read);
        return SK_ERANGE;
    }
    if (inherited) return SK_OK; // void: the first failing piece is the one that reports
    if (lng != ~0ull) {
        snprintf(msg, msg_bytes, "fastq: input %u, line %llu%s has batch_len - 1 bytes or more", (unsigned)(lng >> 63),
                 (unsigned long long)(lng & ~(1ull << 63)), piece ? " of the piece" : "");
        return SK_ELONGLINE;
    }
    if (overflow) {
        snprintf(msg, msg_bytes, "fastq: the text has more batches than batch_capacity");
        return SK_ESPACE;
    }
    if (bad) {
        const uint64_t read = fmt >> 3;
        counts->format_error = (int32_t)(fmt & 7);
        counts->format_input = split ? (uint32_t)(read & 1) : 0u;
        counts->format_record = split ? read >> 1 : read;
        snprintf(msg, msg_bytes, "fastq: input %u, record %llu is malformed (reason %d)", counts->format_input,
                 (unsigned long long)counts->format_record, counts->format_error);
        return SK_EFORMAT;
    }
    if (decode_error(range, &counts->range) == SK_ERANGE) {
        snprintf(msg, msg_bytes, "fastq: quality value %d out of range in read %u at position %u", counts->range.ch,
                 counts->range.read, counts->range.pos + 1);
        return SK_ERANGE;
    }
    for (int o = 0; o < 3; ++o)
        if (h[SK_FQ_H_PRODUCED + o] && !h[SK_FQ_H_FIT + o]) {
            snprintf(msg, msg_bytes, "fastq: an output's buffers are too small for what it needs");
            return SK_ESPACE;
        }
    return SK_OK;
}

#endif
