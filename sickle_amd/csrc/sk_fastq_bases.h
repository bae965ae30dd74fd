// sk_fastq_bases.h -- what the seq bytes of a finished text call add to a sk_fastq_bases and its arrays
// (sk_trim_fastq_bases_device_async, include/sickle_amd.h), as plain functions of bytes and integers.
//
// Classes of a seq byte b: 0 'A' 'a'; 1 'C' 'c'; 2 'G' 'g'; 3 'T' 't'; 4 'N' 'n'; 5 everything else (IUPAC codes, '.',
// 'U', '\r', bytes >= 0x80).  A byte is LOWER iff it lies in 'a'..'z', whatever its class.
// Reads are the report's (sk_fastq_report.h): read r of the packed batch, below SK_FQ_H_NREAL, with the cut {five, three}
// of the workspace; kept iff three >= 0, and then its output is bytes [five, three) (fqp_out_byte).
// The seq line of read r is found as the audit finds name lines: descriptor slot r, or in split mode slot r >> 1 of input
// r & 1 with input 1's slots behind input 0's sk_fq_slots; it is text bytes [d[1] + 1, d[2]) counted from text[i].  In a
// call that adds its length is offsets[r + 1] - offsets[r].  Position p counts from the line's first byte; an output
// byte's position counts from five.  The bytes are always the text's.
// Summed: bytes per class (all reads / output bytes of kept reads), LOWER bytes, reads with a class-4 byte, reads with no
// byte of class 0-3 (an empty output is one), class c at position bin fqp_bin(p, pos_bins), and reads with acgt > 0 bytes
// of class 0-3 in bin floor(100 * (C + G) / acgt) of 101.
// sk_fastq_bases.hip calls these from its kernels; tests/fastq_bases/bases_host.cpp runs them on the host in the
// kernels' shape.
#ifndef SK_FASTQ_BASES_H
#define SK_FASTQ_BASES_H

#include <stdint.h>

#include "sickle_amd.h"

#ifdef __HIPCC__
#define FQB_FN __host__ __device__ static inline
#else
#define FQB_FN static inline
#endif

#define FQB_CLASSES 6

// sk_fastq_bases as 8-byte words, in the order of the struct (the kernels add by word)
enum {
    FQB_W_CALLS = 0,
    FQB_W_CALLS_FAILED,
    FQB_W_READS,
    FQB_W_KEPT,
    FQB_W_BASES_IN,                                // [6]
    FQB_W_BASES_OUT = FQB_W_BASES_IN + FQB_CLASSES, // [6]
    FQB_W_LOWER_IN = FQB_W_BASES_OUT + FQB_CLASSES,
    FQB_W_LOWER_OUT,
    FQB_W_READS_N_IN,
    FQB_W_READS_N_OUT,
    FQB_W_GC_NONE_IN,
    FQB_W_GC_NONE_OUT,
    FQB_W_RESERVED, // [2], zero
    FQB_WORDS = 24
};
#ifdef __cplusplus
static_assert(sizeof(sk_fastq_bases) == 8 * FQB_WORDS, "sk_fastq_bases is FQB_WORDS words");
static_assert(FQB_W_RESERVED == 22, "the members are 22 words");
#endif

// The pass (sk_fq_bases_kernel): a workgroup takes FQB_CHUNK_BYTES of the packed batch's positions, which number the seq
// bytes as they number the quality bytes, and counts in 32-bit LDS halves and 32-bit registers before it flushes them:
// no count of a workgroup exceeds its chunk.  (The read it finishes beyond its chunk adds to the two words of that read
// only, which hold a read's length.)
#define FQB_CHUNK_BYTES (256u * 1024u)
#ifdef __cplusplus
static_assert((uint64_t)FQB_CHUNK_BYTES < (1ull << 32), "a chunk's counts fit 32 bits");
static_assert(FQB_CHUNK_BYTES % 4096u == 0, "a chunk is whole steps of 256 lanes x 16 bytes");
static_assert(2u * FQB_CLASSES * 4u * SK_FQ_BASES_MAX_POS_BINS == 48u * 1024u, "the position tables are 48 KiB of LDS");
static_assert(SK_FQ_BASES_MAX_POS_BINS % 32 == 0, "the largest table is whole groups of fqp_slot");
#endif

// ---- one byte: the rule as it is written -------------------------------------------------------
FQB_FN uint32_t fqb_class(uint8_t b)
{
    switch (b) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    case 'N': case 'n': return 4;
    default: return 5;
    }
}

FQB_FN bool fqb_lower(uint8_t b) { return b >= 'a' && b <= 'z'; }

// ---- sixteen bytes at once -----------------------------------------------------------------------
// 0x80 in every byte of x that is zero, exactly (no carries between bytes)
FQB_FN uint64_t fqb_zero_bytes(uint64_t x)
{
    const uint64_t m = 0x7f7f7f7f7f7f7f7full;
    return ~(((x & m) + m) | x | m);
}

// the 0x80 flags of eight bytes (one in each byte's top bit, or none) as eight bits, byte j to bit j: the eight partial
// products land on eight different bits of the top byte and on no bit twice, so nothing carries
FQB_FN uint32_t fqb_flag_bits(uint64_t flags) { return (uint32_t)(((flags >> 7) * 0x0102040810204080ull) >> 56); }

// 0x80 in every byte of w that is the letter `lower_case` in either case: w | 0x20 equals it for those two bytes only
FQB_FN uint64_t fqb_letter(uint64_t w, uint8_t lower_case)
{
    return fqb_zero_bytes((w | 0x2020202020202020ull) ^ (0x0101010101010101ull * lower_case));
}

// 0x80 in every byte of w in 'a'..'z': below 0x80, at or above 'a' and not above 'z'; the sums stay below 0x100 a byte
FQB_FN uint64_t fqb_lower_bytes(uint64_t w)
{
    const uint64_t h = 0x8080808080808080ull, y = w & ~h;
    const uint64_t ge_a = y + 0x0101010101010101ull * (0x80 - 'a'), gt_z = y + 0x0101010101010101ull * (0x80 - 'z' - 1);
    return ge_a & ~gt_z & ~w & h;
}

// bits [lo, hi) of sixteen, for any lo and hi
FQB_FN uint32_t fqb_range16(int64_t lo, int64_t hi)
{
    if (lo < 0) lo = 0;
    if (hi > 16) hi = 16;
    return lo < hi ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

// Bytes [at, at + 16) of a text of `bytes` bytes, byte j in bits 8 (j & 7) of w[j >> 3]; the bytes at or beyond `bytes`
// are 0.  Nothing at or beyond text + bytes is loaded, whatever `at` is.
FQB_FN void fqb_load16(const uint8_t *text, uint64_t bytes, uint64_t at, uint64_t *w)
{
    uint64_t lo = 0, hi = 0; // (two names, no index: they live in registers on the device)
    if (at < bytes) {
        if (bytes - at >= 16) {
            __builtin_memcpy(&lo, text + at, 8);
            __builtin_memcpy(&hi, text + at + 8, 8);
        } else {
            for (uint64_t j = 0; j < bytes - at; ++j) {
                const uint64_t x = (uint64_t)text[at + j] << (8 * (j & 7));
                if (j < 8) lo |= x; else hi |= x;
            }
        }
    }
    w[0] = lo;
    w[1] = hi;
}

// what a segment is made of: n (1..16) consecutive bytes of one read's seq line, the first at position p0
struct fqb_seg {
    uint32_t m[FQB_CLASSES]; // bit j: byte j has this class
    uint32_t lower;          // bit j: byte j is LOWER
    uint32_t out;            // bit j: byte j is an output byte of a kept read
    uint64_t code[2];        // byte j of the pair: byte j's class
};

// the bytes of w that are the letter of class c: their mask, their flags into `known`, c into their codes
FQB_FN void fqb_letter_class(const uint64_t *w, uint8_t lower_case, uint32_t c, uint32_t valid, uint64_t *known, fqb_seg *s)
{
    const uint64_t f0 = fqb_letter(w[0], lower_case), f1 = fqb_letter(w[1], lower_case);
    s->m[c] = (fqb_flag_bits(f0) | fqb_flag_bits(f1) << 8) & valid;
    known[0] |= f0;
    known[1] |= f1;
    s->code[0] += (f0 >> 7) * (uint64_t)c; // a byte has one class: a byte's code never reaches 6
    s->code[1] += (f1 >> 7) * (uint64_t)c;
}

// w: the sixteen bytes loaded at the segment's first (fqb_load16); the bytes behind the n-th play no part
FQB_FN void fqb_segment(const uint64_t *w, uint32_t n, uint64_t p0, int32_t five, int32_t three, fqb_seg *s)
{
    const uint32_t valid = fqb_range16(0, n);
    uint64_t known[2] = {0, 0};
    s->code[0] = s->code[1] = 0;
    fqb_letter_class(w, 'a', 0, valid, known, s);
    fqb_letter_class(w, 'c', 1, valid, known, s);
    fqb_letter_class(w, 'g', 2, valid, known, s);
    fqb_letter_class(w, 't', 3, valid, known, s);
    fqb_letter_class(w, 'n', 4, valid, known, s);
    const uint64_t h = 0x8080808080808080ull;
    s->code[0] += ((~known[0] & h) >> 7) * 5u;
    s->code[1] += ((~known[1] & h) >> 7) * 5u;
    s->m[5] = valid & ~(s->m[0] | s->m[1] | s->m[2] | s->m[3] | s->m[4]);
    s->lower = (fqb_flag_bits(fqb_lower_bytes(w[0])) | fqb_flag_bits(fqb_lower_bytes(w[1])) << 8) & valid;
    // fqp_out_byte for the sixteen positions p0 + j at once (p0 < 2^63: a position of a text in memory)
    s->out = three >= 0 ? fqb_range16((int64_t)five - (int64_t)p0, (int64_t)three - (int64_t)p0) & valid : 0u;
}

FQB_FN uint32_t fqb_code_at(const fqb_seg *s, uint32_t j) { return (uint32_t)(s->code[j >> 3] >> (8 * (j & 7))) & 7u; }

// ---- one read ------------------------------------------------------------------------------------
// A read's (or its output's) whole-line figures in one word, so that the segments of a read that lanes share add to it
// with one add each: acgt, its bytes of class 0-3, in bits 0..24; C + G in bits 25..49; bit 63: a byte of class 4.  A read
// has at most SK_MAX_READ_LEN = 2^24 bytes, so neither sum carries into the field above it.
#define FQB_R_GC_SHIFT 25
#define FQB_R_MASK ((1ull << FQB_R_GC_SHIFT) - 1)
#define FQB_R_N (1ull << 63)
#ifdef __cplusplus
static_assert((uint64_t)SK_MAX_READ_LEN <= FQB_R_MASK, "a read's counts fit their fields");
#endif

// what the bytes `sel` of a segment add to such a word (the flag is OR-ed, the rest added: fqb_read_add)
FQB_FN uint64_t fqb_read_part(const fqb_seg *s, uint32_t sel)
{
    const uint64_t acgt = (uint64_t)__builtin_popcount((s->m[0] | s->m[1] | s->m[2] | s->m[3]) & sel);
    const uint64_t gc = (uint64_t)__builtin_popcount((s->m[1] | s->m[2]) & sel);
    return acgt | gc << FQB_R_GC_SHIFT | ((s->m[4] & sel) ? FQB_R_N : 0);
}

FQB_FN uint64_t fqb_read_add(uint64_t word, uint64_t part) { return ((word & ~FQB_R_N) + (part & ~FQB_R_N)) | ((word | part) & FQB_R_N); }

// the GC bin of a finished word, -1 where it has no byte of class 0-3
FQB_FN int32_t fqb_gc_bin(uint64_t word)
{
    const uint32_t acgt = (uint32_t)(word & FQB_R_MASK), gc = (uint32_t)((word >> FQB_R_GC_SHIFT) & FQB_R_MASK);
    return acgt ? (int32_t)(100u * gc / acgt) : -1; // 100 * 2^24 < 2^32
}

FQB_FN uint32_t fqb_has_n(uint64_t word) { return (uint32_t)(word >> 63); }

#endif
