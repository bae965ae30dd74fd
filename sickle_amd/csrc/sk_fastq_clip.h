// sk_fastq_clip.h -- what a 3' adapter hit does to a read of a clipped text call (sk_trim_fastq_clipped_device_async,
// include/sickle_amd.h), as plain functions of integers.  The hit itself is sk_fastq_adapters.h's, unchanged.
//
// The seq line of a read lies between the ends of its name line and of its seq line, e0 and e1 of its record descriptor:
// it starts at e0 + 1 and holds L = e1 - e0 - 1 bases (fqc_line).  The read's hit (p, a) is the rule's of DESIGN 4.21 on
// those L bases, its clip word a << 24 | p or SK_FQ_CLIP_NONE (fqd_clip_word), and its packed length min(L, p) with a hit
// and L without (fqc_packed_len): the scan, and everything that takes a read's length from the packed batch's offsets,
// sees the first p bases alone.
// sk_fastq_adapters.hip calls these from sk_fq_clip_kernel and sk_fastq.hip from the pack; tests/fastq_clip/clip_host.cpp
// walks them on the host in the kernel's shape.
#ifndef SK_FASTQ_CLIP_H
#define SK_FASTQ_CLIP_H

#include <stdint.h>

#include "sickle_amd.h"
#include "sk_fastq_adapters.h"

#define FQC_FN FQD_FN

// sk_fastq_clip_stats as 8-byte words, in the order of the struct (the kernels add by word)
enum {
    FQC_W_CALLS = 0,
    FQC_W_CALLS_FAILED,
    FQC_W_READS,
    FQC_W_READS_CLIPPED,
    FQC_W_READS_EMPTIED,
    FQC_W_BASES_CLIPPED,
    FQC_W_HITS, // [8]
    FQC_W_RESERVED = FQC_W_HITS + 8, // [2], zero
    FQC_WORDS = FQC_W_RESERVED + 2
};
#define FQC_STATS_BYTES 128u
#ifdef __cplusplus
static_assert(sizeof(sk_fastq_clip_stats) == 8 * FQC_WORDS && 8 * FQC_WORDS == FQC_STATS_BYTES, "sk_fastq_clip_stats is FQC_WORDS words");
#endif

// ---- the workspace -----------------------------------------------------------------------------------
// the clip words a text of text_bytes can need: N of sk_fq_layout_of, the reads its offsets section holds
FQC_FN uint64_t fqc_words_bound(uint64_t text_bytes) { return 2 * ((text_bytes + 2) / 16) + 2; }

// the clip section: the call-local stats block, then the words, rounded up to 16
FQC_FN uint64_t fqc_extra_bytes(uint64_t text_bytes) { return (FQC_STATS_BYTES + 4 * fqc_words_bound(text_bytes) + 15) & ~15ull; }

// ---- one line ----------------------------------------------------------------------------------------
struct fqc_span {
    uint64_t sq, L; // where the seq line starts in its text, its length
};

// The seq line of a record from its descriptor words e0 (the name line's end) and e1 (the seq line's end) in a text of
// `bytes` bytes: never a byte at or beyond the text's end, never more than SK_MAX_READ_LEN bases, whatever the words
// hold.  Of a record that has passed the format checks it is [e0 + 1, e1).
FQC_FN fqc_span fqc_line(uint64_t e0, uint64_t e1, uint64_t bytes)
{
    fqc_span s;
    const uint64_t b = e0 < bytes ? e0 : bytes, e = e1 < bytes ? e1 : bytes;
    s.sq = b + 1 < bytes ? b + 1 : bytes;
    s.L = e > s.sq ? e - s.sq : 0;
    if (s.L > SK_MAX_READ_LEN) s.L = SK_MAX_READ_LEN;
    return s;
}

// ---- one read ----------------------------------------------------------------------------------------
// the packed length of a read whose line holds len bytes, from its clip word
FQC_FN uint64_t fqc_packed_len(uint64_t len, uint32_t word)
{
    const uint64_t p = word & 0xFFFFFFu;
    return word == SK_FQ_CLIP_NONE || p > len ? len : p;
}

// what one read adds to word w of the stats, FQC_W_READS <= w < FQC_W_RESERVED (r->L: the line's length before the clip)
FQC_FN uint64_t fqc_read_word(uint32_t w, const fqd_read *r)
{
    if (w == FQC_W_READS) return 1;
    if (!r->hit) return 0;
    if (w == FQC_W_READS_CLIPPED) return 1;
    if (w == FQC_W_READS_EMPTIED) return r->p == 0;
    if (w == FQC_W_BASES_CLIPPED) return r->L - r->p;
    if (w >= FQC_W_HITS && w < FQC_W_HITS + 8) return w - FQC_W_HITS == r->a;
    return 0;
}

#endif
