// sk_fastq_rejects.h -- which reads of a finished text call go to the rejects text and what their records are
// (sk_trim_fastq_rejects_device_async, include/sickle_amd.h), as plain functions of integers.
//
// Reads are the report's (sk_fastq_report.h): read r of the packed batch, below SK_FQ_H_NREAL, kept iff its cut has
// three >= 0; in the pair framings reads 2k and 2k + 1 are pair k.  Selected: every read that is not kept; with
// SK_FQ_REJECTS_PAIRS both mates of every pair with a mate that is not kept.  A record is the input's own four lines,
// bytes [s0, e3) of the record's text, and one '\n' that is never loaded: e3 - s0 + 1 bytes.  s0 and e3 come from the text
// call's descriptors; the source view's fqs_record (sk_fastq_source.h) holds them to the text, so that whatever the
// descriptors say no byte at or beyond text + bytes is asked for.
// sk_fastq_rejects.hip calls these from its four kernels; tests/fastq_rejects/rejects_host.cpp walks them on the host in
// the kernels' shape.
#ifndef SK_FASTQ_REJECTS_H
#define SK_FASTQ_REJECTS_H

#include <stdint.h>

#include "sickle_amd.h"
#include "sk_fastq_source.h"

#ifdef __HIPCC__
#define FQJ_FN __host__ __device__ static inline
#else
#define FQJ_FN static inline
#endif

#define FQJ_IMM (~0ull) // fqj_piece.at of the immediate piece

// The workspace of a rejects call (16-byte sections): the header, then FQJ_BLOCK_WORDS words per block of
// SK_FQ_BLOCK_READS reads (selected records and their bytes; exclusive bases behind the scan), then two words per read of
// the bound N: output offset and read number of every selected record.
#define FQJ_HDR_WORDS 16u
#define FQJ_BLOCK_READS 2048u // == SK_FQ_BLOCK_READS of sk_device.h
#define FQJ_BLOCK_WORDS 2u
#define FQJ_H_RECORDS 0    // selected records (0 in a void call)
#define FQJ_H_BYTES 1      // their bytes: what the text needs
#define FQJ_H_READS 2      // NREAL (0 in a void call)
#define FQJ_H_VALID 3
#define FQJ_H_FLAGS 4
#define FQJ_H_PRODUCED 5   // out->text was given
#define FQJ_H_WRITTEN 6    // valid, produced and within both capacities: place and gather write  (the `written` word)
#define FQJ_H_OUT_BYTES 7  // FQJ_H_BYTES where FQJ_H_WRITTEN, else 0                                (the `bytes` word)

// reads of the bound: N of sk_fq_layout_of, what the text call's offsets and cuts sections hold
FQJ_FN uint64_t fqj_reads_bound(uint64_t text_bytes) { return 2 * ((text_bytes + 2) / 16) + 2; }
FQJ_FN uint64_t fqj_blocks(uint64_t text_bytes) { return (fqj_reads_bound(text_bytes) + FQJ_BLOCK_READS - 1) / FQJ_BLOCK_READS; }
FQJ_FN uint64_t fqj_blocks_at(void) { return 8ull * FQJ_HDR_WORDS; }
FQJ_FN uint64_t fqj_table_at(uint64_t text_bytes) { return fqj_blocks_at() + 8ull * FQJ_BLOCK_WORDS * fqj_blocks(text_bytes); }
FQJ_FN uint64_t fqj_workspace_bytes(uint64_t text_bytes) { return fqj_table_at(text_bytes) + 16 * fqj_reads_bound(text_bytes); }

// A text of T bytes holds records whose spans [s0, e3) are disjoint and lie in it, and every '\n' between two records is
// a byte of the text that no span holds, but for the last record's: the rejects of flags 0 and of SK_FQ_REJECTS_PAIRS are
// at most T + 1 bytes (T + 2 over two texts).
FQJ_FN uint64_t fqj_bound(uint64_t text_bytes) { return text_bytes + 2; }

// ---- selection -----------------------------------------------------------------------------------
FQJ_FN bool fqj_kept(int32_t three) { return three >= 0; } // == fqr_kept, fqp_kept

// pairs: SK_FQ_REJECTS_PAIRS in a pair framing; mate_kept: of read r ^ 1 (true where there is no mate)
FQJ_FN bool fqj_selected(bool kept, bool mate_kept, bool pairs) { return !kept || (pairs && !mate_kept); }

// ---- the record -----------------------------------------------------------------------------------
// fqs_span under the name tests/fastq_rejects/rejects_host.cpp walks it by
FQJ_FN void fqj_span(uint64_t s0, uint64_t e3, uint64_t bytes, uint64_t *at, uint64_t *len) { fqs_span(s0, e3, bytes, at, len); }

// bytes of the record: the span and its '\n'
FQJ_FN uint64_t fqj_record_bytes(uint64_t span_len) { return span_len + 1; }

struct fqj_piece {
    uint64_t at;  // offset in the record's text, or FQJ_IMM
    uint64_t len;
    uint64_t imm; // FQJ_IMM: the piece's one byte
};

// the piece table of a record: one text span and one immediate
FQJ_FN void fqj_pieces(uint64_t at, uint64_t span_len, fqj_piece (&pc)[2])
{
    pc[0] = {at, span_len, 0};
    pc[1] = {FQJ_IMM, 1, (uint64_t)'\n'};
}

// ---- validity: the source view's fqs_valid (sk_fastq_source.h) --------------------------------------
// the verdict of the scan kernel: what is written where
FQJ_FN bool fqj_fits(bool valid, bool produced, uint64_t bytes, uint64_t capacity, bool index, uint64_t records, uint64_t record_capacity)
{
    return valid && produced && bytes <= capacity && (!index || records <= record_capacity);
}

#endif
