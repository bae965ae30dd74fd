// sk_fastq_words.h -- the words of the header of a FASTQ text call's workspace and where its sections lie (sk_device.h
// describes the workspace).  No HIP: sk_device.h includes it for the kernels, sk_fastq_verdict.h and sk_fastq_source.h for
// the host.
#ifndef SK_FASTQ_WORDS_H
#define SK_FASTQ_WORDS_H

#include <stdint.h>

#include "sickle_amd.h"

#define SK_FQ_HDR_WORDS 32u
#define SK_FQ_H_LINES 0        // [2] lines of each input
#define SK_FQ_H_RECORDS 2      // [2] complete records of each input
#define SK_FQ_H_FMT 4          // (read << 3) | SK_FQ_* of the lowest malformed record, or ~0
#define SK_FQ_H_NREAL 5        // reads of the packed batch that are records (the rest are empty)
#define SK_FQ_H_PACKED 6       // bytes of the packed qual (and seq)
#define SK_FQ_H_OUT_RECORDS 7  // [3]
#define SK_FQ_H_OUT_BYTES 10   // [3]
#define SK_FQ_H_FIT 13         // [3] produced, no error, within its capacities: the emission writes it
#define SK_FQ_H_PRODUCED 16    // [3] out[o].text != NULL for an output of the mode
#define SK_FQ_H_RANGE 19       // the stream's range-error word as the emission saw it
#define SK_FQ_H_MODE 20        // the call's framing mode (SK_TRIM_PE_INTERLEAVED for SK_TRIM_PE_COMBO_ALL)
// Piece calls (sk_trim_fastq_piece_device_async with piece != NULL) use words 21..29, which are otherwise the ordered
// calls' (sk_fastq_order.h); an ordered piece keeps these here and its order words in an extension block (sk_device.h).
#define SK_FQP_H_START 21      // [2] s_i: the window's first byte, offset in text[i]
#define SK_FQP_H_END 23        // [2] n_i: the window's end (sk_trim_fastq_piece_words' end)
#define SK_FQP_H_CONSUMED 25   // [2] offset in text[i] of the first byte the piece did not consume
#define SK_FQP_H_OK 27         // 1 iff no format error, the range-error word clear at both looks, every produced output fitted
#define SK_FQP_H_RANGE0 28     // the stream's range-error word as the frame scan saw it, before the piece's own scan
#define SK_FQP_H_MORE 29       // the piece's `more`

// the sections of the workspace (sk_device.h's comment on sk_launch_fastq_front has the sizes and why they suffice)
#define SK_FQ_CHUNK_BYTES 65536u
#define SK_FQ_BLOCK_READS 2048u
#define SK_FQ_BLOCK_WORDS 8u
struct sk_fq_layout {
    uint64_t chunks, desc, offsets, cuts, blocks, emit, qual, seq, total; // byte offsets of the sections, total size
};
static inline uint64_t sk_fq_slots(uint64_t bytes) { return bytes / 4 + 1; }
// reads of the packed batch: the most valid records the text(s) can hold
static inline uint64_t sk_fq_pack_reads(uint64_t bytes0, uint64_t bytes1, int mode)
{
    const uint64_t r0 = (bytes0 + 1) / 8, r1 = (bytes1 + 1) / 8;
    return mode == SK_TRIM_PE_SPLIT ? 2 * (r0 < r1 ? r0 : r1) : r0;
}
static inline void sk_fq_layout_of(uint64_t text_bytes, int trunc_n, sk_fq_layout *L)
{
    const uint64_t H = (text_bytes + 2) / 16, S = 2 * ((text_bytes + 7) / 8) + 2, N = 2 * H + 2; // S >= b0 / 4 + b1 / 4 + 2
    const uint64_t NC = text_bytes / SK_FQ_CHUNK_BYTES + 3, NB = (N + SK_FQ_BLOCK_READS - 1) / SK_FQ_BLOCK_READS;
    const uint64_t Q = 16 * ((text_bytes + 31) / 32);
    L->chunks = 8 * SK_FQ_HDR_WORDS;
    L->desc = L->chunks + 16 * NC;
    L->offsets = L->desc + 40 * S;
    L->cuts = L->offsets + 8 * (N + 2);
    L->blocks = L->cuts + 8 * N;
    L->emit = L->blocks + 64 * NB;
    L->qual = L->emit + 16 * N;
    L->seq = L->qual + Q;
    L->total = L->seq + (trunc_n ? Q : 0);
}
// Ordered calls (sk_trim_fastq_ordered_device_async, sk_fastq_order.h): the same header (its words 21.. are theirs), then
// the table of first units (8 * (batch_capacity + 1), rounded up to 16), then the sections above, shifted by the table.
static inline uint64_t sk_fq_order_shift(uint64_t batch_capacity) { return (8 * (batch_capacity + 1) + 15) & ~15ull; }
// Ordered pieces (sk_trim_fastq_ordered_piece_device_async): the header with the PIECE's words 21.. (SK_FQP_H_*), then an
// extension block of 256 bytes that holds the order words at their usual indices and the piece's own (sk_fastq_order.h:
// SK_FQOP_*), then the table of first units, then the sections, shifted by block and table.
static inline uint64_t sk_fq_order_piece_shift(uint64_t batch_capacity) { return 256 + sk_fq_order_shift(batch_capacity); }

#endif
