// sk_fastq_audit.h -- what one pair of name lines and the quality bytes of a finished text call add to an audit
// (sk_trim_fastq_audit_device_async, include/sickle_amd.h), as plain functions of bytes and integers.
//
// Key of a name line.  The name line is the record's first line without its '\n'; byte 0 is '@' in any call that adds.
// The key is bytes [1, e), e the index of the first byte at or after index 1 that is ' ', '\t' or '\r', or the line's
// length.  Then, once: a key of 2 bytes or more whose last but one byte is '/' and whose last is '1' or '2' loses those two
// bytes, and the tag is that digit; otherwise the tag is 0.  An empty key is a key.
// Pair k is reads 2k and 2k + 1 of the packed batch, only where both lie below SK_FQ_H_NREAL (sk_fastq_report.h's
// fqp_pair_at).  It matches iff the two keys have the same length and bytes; it is tag-swapped iff it matches, mate 1's
// tag is 2 and mate 2's is 1.
// Quality bytes: bytes [0, offsets[NREAL]) of the packed qual, as unsigned.
// sk_fastq_audit.hip calls these from its kernels; tests/fastq_audit/audit_host.cpp runs them on the host.
#ifndef SK_FASTQ_AUDIT_H
#define SK_FASTQ_AUDIT_H

#include <stdint.h>

#include "sickle_amd.h"

#ifdef __HIPCC__
#define FQA_FN __host__ __device__ static inline
#else
#define FQA_FN static inline
#endif

// sk_fastq_audit as 8-byte words, in the order of the struct
enum {
    FQA_W_CALLS = 0,
    FQA_W_CALLS_FAILED,
    FQA_W_PAIRS,
    FQA_W_NAME_MISMATCH,
    FQA_W_FIRST_MISMATCH,
    FQA_W_TAGS_SWAPPED,
    FQA_W_QUAL_BYTES,
    FQA_W_QUAL_MIN,
    FQA_W_QUAL_MAX,
    FQA_W_CALL_FIRST, // reserved[0]: the lowest mismatching pair of the call in flight, ~0 between calls
    FQA_W_CALL_PAIRS, // reserved[1]: the pairs of the call in flight, 0 between calls
    FQA_WORDS = 16
};
#ifdef __cplusplus
static_assert(sizeof(sk_fastq_audit) == 8 * FQA_WORDS, "sk_fastq_audit is FQA_WORDS words");
#endif

// The quality pass: a workgroup takes FQA_CHUNK_BYTES of the packed qual and counts byte values in 32-bit LDS counters.
#define FQA_CHUNK_BYTES (256u * 1024u)
#define FQA_TABLES 16u       // private tables of a workgroup: lane t adds to table t % FQA_TABLES
#define FQA_TABLE_STRIDE 257u // words between tables: one value's 16 counters lie in 16 different banks
#ifdef __cplusplus
static_assert((uint64_t)FQA_CHUNK_BYTES < (1ull << 32), "a chunk's counts fit 32 bits");
static_assert(FQA_CHUNK_BYTES % 4096u == 0, "a chunk is whole steps of 256 lanes x 16 bytes");
#endif

// the value that starts qual_min and first_mismatch
#define FQA_NONE (~0ull)

// 0x80 in every byte of x that is zero, exactly (no carries between bytes)
FQA_FN uint64_t fqa_zero_bytes(uint64_t x)
{
    const uint64_t m = 0x7f7f7f7f7f7f7f7full;
    return ~(((x & m) + m) | x | m);
}

// 0x80 in every byte of x that ends a key: ' ', '\t' or '\r'
FQA_FN uint64_t fqa_end_bytes(uint64_t x)
{
    return fqa_zero_bytes(x ^ 0x2020202020202020ull) | fqa_zero_bytes(x ^ 0x0909090909090909ull) |
           fqa_zero_bytes(x ^ 0x0d0d0d0d0d0d0d0dull);
}

// index of the lowest non-zero byte of x (x != 0)
FQA_FN uint32_t fqa_low_byte(uint64_t x) { return (uint32_t)__builtin_ctzll(x) >> 3; }

// bytes [at, at + 8) of a line of len bytes at p, byte j in bits 8j; the bytes at or beyond len are 0.  Nothing at or
// beyond p + len is loaded.
FQA_FN uint64_t fqa_load8(const uint8_t *p, uint64_t len, uint64_t at)
{
    uint64_t v = 0;
    if (at + 8 <= len) {
        __builtin_memcpy(&v, p + at, 8);
    } else {
        for (uint64_t j = 0; at + j < len; ++j) v |= (uint64_t)p[at + j] << (8 * j);
    }
    return v;
}

// the tag rule on a key of len bytes whose last two are y (last but one) and z (last): the tag, 0 if there is none
FQA_FN uint32_t fqa_tag(uint64_t len, uint8_t y, uint8_t z)
{
    return len >= 2 && y == '/' && (z == '1' || z == '2') ? (uint32_t)(z - '0') : 0u;
}

// what fqa_pair finds: bit 0 the keys differ, bit 1 the pair is tag-swapped
#define FQA_MISMATCH 1u
#define FQA_SWAPPED 2u

// One pair: name line 1 is the len1 bytes at n1, name line 2 the len2 bytes at n2 (without the '\n').  The two lines are
// walked once, side by side, 8 bytes a step: the walk finds each key's end and the lowest index at which the lines
// differ, and ends when both keys have ended; it is bounded by the longer line.  A line shorter than 1 byte has the empty
// key (no call that adds has one).
FQA_FN uint32_t fqa_pair(const uint8_t *n1, uint64_t len1, const uint8_t *n2, uint64_t len2)
{
    const uint64_t none = ~0ull;
    uint64_t e1 = len1 < 1 ? 1 : none, e2 = len2 < 1 ? 1 : none, diff = none;
    const uint64_t longer = len1 > len2 ? len1 : len2;
    for (uint64_t at = 1; at < longer && (e1 == none || e2 == none); at += 8) {
        const uint64_t a = fqa_load8(n1, len1, at), b = fqa_load8(n2, len2, at);
        if (e1 == none) {
            const uint64_t m = fqa_end_bytes(a);
            if (m) e1 = at + fqa_low_byte(m);
        }
        if (e2 == none) {
            const uint64_t m = fqa_end_bytes(b);
            if (m) e2 = at + fqa_low_byte(m);
        }
        if (diff == none && a != b) diff = at + fqa_low_byte(a ^ b);
    }
    // an end beyond the line (the zero fill holds no end byte, but the line may simply have run out) is the line's length
    if (e1 > len1) e1 = len1 < 1 ? 1 : len1;
    if (e2 > len2) e2 = len2 < 1 ? 1 : len2;
    uint64_t k1 = e1 - 1, k2 = e2 - 1; // the keys' lengths
    const uint32_t t1 = k1 >= 2 ? fqa_tag(k1, n1[e1 - 2], n1[e1 - 1]) : 0u;
    const uint32_t t2 = k2 >= 2 ? fqa_tag(k2, n2[e2 - 2], n2[e2 - 1]) : 0u;
    if (t1) k1 -= 2;
    if (t2) k2 -= 2;
    // the keys are bytes [1, 1 + k): they differ iff their lengths do or the lines differ below 1 + k
    if (k1 != k2 || diff < 1 + k1) return FQA_MISMATCH;
    return t1 == 2 && t2 == 1 ? FQA_SWAPPED : 0u;
}

// A granule of 16 packed bytes (byte i in bits 8 (i & 3) of word[i >> 2]) of which only the first n (1 <= n < 16) are
// quality bytes, the batch's last: the bytes behind them become copies of the first, which changes no extreme.
FQA_FN void fqa_fill_tail(uint32_t *word, uint32_t n)
{
    const uint32_t q0 = word[0] & 0xffu;
    for (uint32_t i = 1; i < 16; ++i)
        if (i >= n) word[i >> 2] = (word[i >> 2] & ~(0xffu << (8 * (i & 3)))) | (q0 << (8 * (i & 3)));
}

// byte i of a granule
FQA_FN uint32_t fqa_byte(const uint32_t *word, uint32_t i) { return (word[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// where value q lies in the LDS tables of a workgroup, for lane t
FQA_FN uint32_t fqa_table_slot(uint32_t t, uint32_t q) { return (t % FQA_TABLES) * FQA_TABLE_STRIDE + q; }

// the minimum and the maximum of the four bytes of w, folded into lo and hi (the kernel does this on packed halves)
FQA_FN void fqa_minmax4(uint32_t w, uint32_t *lo, uint32_t *hi)
{
    for (int j = 0; j < 4; ++j) {
        const uint32_t q = (w >> (8 * j)) & 0xffu;
        if (q < *lo) *lo = q;
        if (q > *hi) *hi = q;
    }
}

// The fold behind a call's names pass: the call's lowest mismatching pair and its pair count, which the pass left in the
// two reserved words, go into first_mismatch and pairs, and the two words return to their rest values.
FQA_FN void fqa_fold(uint64_t *w)
{
    const uint64_t first = w[FQA_W_CALL_FIRST], pairs = w[FQA_W_CALL_PAIRS];
    if (first != FQA_NONE) {
        const uint64_t at = w[FQA_W_PAIRS] + first;
        if (at < w[FQA_W_FIRST_MISMATCH]) w[FQA_W_FIRST_MISMATCH] = at;
        w[FQA_W_CALL_FIRST] = FQA_NONE;
    }
    if (pairs) {
        w[FQA_W_PAIRS] += pairs;
        w[FQA_W_CALL_PAIRS] = 0;
    }
}

// a reset struct
FQA_FN uint64_t fqa_reset_word(uint32_t i)
{
    return i == FQA_W_FIRST_MISMATCH || i == FQA_W_QUAL_MIN || i == FQA_W_CALL_FIRST ? FQA_NONE : 0;
}

#endif
