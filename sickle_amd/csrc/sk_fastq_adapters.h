// sk_fastq_adapters.h -- where a read runs into a 3' adapter and what that adds to a sk_fastq_adapters and its arrays
// (sk_trim_fastq_adapters_device_async, include/sickle_amd.h), as plain functions of bytes and integers.
//
// A read byte b matches the adapter base c (upper case) iff (b & 0xDF) == c.  Adapter a of length A hits at start p,
// 0 <= p <= L - min_overlap, iff the overlap v = min(A, L - p) is at least min_overlap and the mismatches m among
// read[p .. p + v) against adapter[0 .. v) number at most floor(v * max_mismatch_permille / 1000).  The read's hit is the
// one with the lowest p, among the adapters at that p the lowest a.
// The search works on three bit planes, one bit per base: the two bits of a base's code (A 0, C 1, G 2, T 3) and a VALID
// bit that only the eight letters have.  Sixty-four consecutive bases are one word per plane (fqd_planes); an adapter is
// one word of either code plane (fqd_codes).  The window of 64 bases that starts s bases into a word is a funnel shift of
// that word and the next (fqd_funnel); the mismatches are one popcount over (lo ^ lo') | (hi ^ hi') | ~valid, masked to
// the overlap (fqd_mismatches).  A base that is not VALID, and every base at or beyond the line's end, mismatches.
// sk_fastq_adapters.hip calls these from its kernel, a wave a read and a lane a start; tests/fastq_adapters/
// adapters_host.cpp runs them on the host in the kernel's shape.
#ifndef SK_FASTQ_ADAPTERS_H
#define SK_FASTQ_ADAPTERS_H

#include <stdint.h>

#include "sickle_amd.h"

#ifdef __HIPCC__
#define FQD_FN __host__ __device__ static inline
#else
#define FQD_FN static inline
#endif

// sk_fastq_adapters as 8-byte words, in the order of the struct (the kernel adds by word)
enum {
    FQD_W_CALLS = 0,
    FQD_W_CALLS_FAILED,
    FQD_W_READS,
    FQD_W_KEPT,
    FQD_W_READS_HIT,
    FQD_W_READS_HIT_KEPT,
    FQD_W_HITS, // [8]
    FQD_W_HITS_FULL = FQD_W_HITS + 8,
    FQD_W_HITS_AT_0,
    FQD_W_MISMATCHES,
    FQD_W_BASES_BEHIND,
    FQD_W_READS_HIT_OUT,
    FQD_W_BASES_HIT_OUT,
    FQD_W_PAIRS_BOTH,
    FQD_W_PAIRS_ONE,
    FQD_W_PAIRS_SAME_CLIP,
    FQD_W_RESERVED, // zero
    FQD_WORDS
};
#ifdef __cplusplus
static_assert(sizeof(sk_fastq_adapters) == 8 * FQD_WORDS && FQD_WORDS == 24, "sk_fastq_adapters is FQD_WORDS words");
static_assert(sizeof(sk_fastq_adapter_set) == 560, "sk_fastq_adapter_set has no padding");
static_assert(SK_FQ_ADAPTER_MAX_LEN == 64 && SK_FQ_ADAPTERS_OVERLAP_BINS == SK_FQ_ADAPTER_MAX_LEN + 1, "an adapter is one word a plane");
static_assert((uint64_t)SK_MAX_READ_LEN <= (1u << 24), "a start fits the clip word's 24 bits");
#endif

// ---- the set ---------------------------------------------------------------------------------------
// why a set is refused, as text; NULL: it is in bounds
FQD_FN const char *fqd_set_error(const sk_fastq_adapter_set *s)
{
    if (s->n < 1 || s->n > SK_FQ_ADAPTERS_MAX) return "n must be 1 .. SK_FQ_ADAPTERS_MAX";
    if (s->reserved != 0) return "reserved must be 0";
    if (s->max_mismatch_permille > 500) return "max_mismatch_permille must be 0 .. 500";
    if (s->min_overlap < 1) return "min_overlap must be at least 1";
    for (uint32_t a = 0; a < s->n; ++a) {
        if (s->len[a] < 1 || s->len[a] > SK_FQ_ADAPTER_MAX_LEN) return "every len must be 1 .. SK_FQ_ADAPTER_MAX_LEN";
        if (s->min_overlap > s->len[a]) return "min_overlap must not exceed any len";
        for (uint32_t j = 0; j < s->len[a]; ++j) {
            const uint8_t c = s->seq[a][j] & 0xDF;
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') return "seq bytes must be from ACGTacgt";
        }
    }
    return 0;
}

// ---- one byte --------------------------------------------------------------------------------------
// the code of a seq byte: 0 .. 3 for A C G T in either case, 4 for every other byte (no adapter base matches it)
FQD_FN uint32_t fqd_code(uint8_t b)
{
    const uint32_t u = b & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// ---- the planes ------------------------------------------------------------------------------------
struct fqd_planes {
    uint64_t lo, hi, valid; // bit j: base j's code bit 0, its code bit 1, whether it is one of the eight letters
};

// what the kernels take by value: the set's adapters as code planes (bases behind len are zero bits; the mask cuts them)
struct fqd_codes {
    uint64_t lo[8], hi[8];
    uint32_t len[8];
    uint32_t n, min_overlap, permille, reserved;
};

// of a set that fqd_set_error has passed
FQD_FN void fqd_encode_set(const sk_fastq_adapter_set *s, fqd_codes *c)
{
    c->n = s->n;
    c->min_overlap = s->min_overlap;
    c->permille = s->max_mismatch_permille;
    c->reserved = 0;
    for (uint32_t a = 0; a < 8; ++a) {
        c->lo[a] = c->hi[a] = 0;
        c->len[a] = a < s->n ? s->len[a] : 0;
        for (uint32_t j = 0; j < c->len[a]; ++j) {
            const uint64_t code = fqd_code(s->seq[a][j]);
            c->lo[a] |= (code & 1) << j;
            c->hi[a] |= ((code >> 1) & 1) << j;
        }
    }
}

// bits [s & 31, (s & 31) + 32) of hi:lo (one v_alignbit_b32 on the device)
FQD_FN uint32_t fqd_alignbit(uint32_t hi, uint32_t lo, uint32_t s)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_alignbit(hi, lo, s);
#else
    return (uint32_t)(((uint64_t)hi << 32 | lo) >> (s & 31u));
#endif
}

// The 64 bits that start s bits (0 .. 63) into w0, continued by w1: of the four 32-bit words the three that hold them (a
// choice by s >= 32, which a lane of the kernel makes with selects), then two 32-bit funnel shifts by s & 31.
FQD_FN uint64_t fqd_funnel(uint64_t w0, uint64_t w1, uint32_t s)
{
    const uint32_t d0 = (uint32_t)w0, d1 = (uint32_t)(w0 >> 32), d2 = (uint32_t)w1, d3 = (uint32_t)(w1 >> 32);
    const bool up = s >= 32u;
    const uint32_t e0 = up ? d1 : d0, e1 = up ? d2 : d1, e2 = up ? d3 : d2;
    return (uint64_t)fqd_alignbit(e2, e1, s) << 32 | fqd_alignbit(e1, e0, s);
}

FQD_FN uint64_t fqd_low_mask(uint32_t v) { return v >= 64u ? ~0ull : (1ull << v) - 1ull; } // the lowest v bits, v <= 64

FQD_FN uint32_t fqd_popcount(uint64_t x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popcll(x);
#else
    return (uint32_t)__builtin_popcountll(x);
#endif
}

// the window's bases under `mask` that do not match the adapter's
FQD_FN uint32_t fqd_mismatches_under(uint64_t win_lo, uint64_t win_hi, uint64_t win_valid, uint64_t ad_lo, uint64_t ad_hi, uint64_t mask)
{
    return fqd_popcount(((win_lo ^ ad_lo) | (win_hi ^ ad_hi) | ~win_valid) & mask);
}

// the window's bases 0 .. v - 1 that do not match the adapter's
FQD_FN uint32_t fqd_mismatches(uint64_t win_lo, uint64_t win_hi, uint64_t win_valid, uint64_t ad_lo, uint64_t ad_hi, uint32_t v)
{
    return fqd_mismatches_under(win_lo, win_hi, win_valid, ad_lo, ad_hi, fqd_low_mask(v));
}

// ---- one start ---------------------------------------------------------------------------------------
FQD_FN uint32_t fqd_overlap(uint32_t A, uint64_t L, uint64_t p) { return L - p < A ? (uint32_t)(L - p) : A; } // p <= L

// a * b for a, b < 2^24 (one full-rate v_mul_u32_u24 on the device)
FQD_FN uint32_t fqd_mul24(uint32_t a, uint32_t b)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __umul24(a, b);
#else
    return a * b;
#endif
}

// m <= floor(v * permille / 1000), without the division: v <= 64, m <= 64, permille <= 500
FQD_FN bool fqd_is_hit(uint32_t v, uint32_t m, uint32_t min_overlap, uint32_t permille)
{
    return v >= min_overlap && fqd_mul24(m, 1000u) <= fqd_mul24(v, permille);
}

// Start p of a line of L bases against every adapter, from the planes' windows at p: the lowest adapter that hits there,
// or FQD_NO_ADAPTER.  (p <= L - min_overlap is the caller's.)  The read's hit is the lowest start that names an adapter.
// The mask of an overlap min(A, L - p) is the mask of the line's rest, one per start, under the mask of A, one per adapter.
#define FQD_NO_ADAPTER 8u
// n: c->n (the kernel's is a constant, so that the loop unrolls and the planes stay in scalar registers)
FQD_FN uint32_t fqd_start(const fqd_codes *c, uint32_t n, uint64_t win_lo, uint64_t win_hi, uint64_t win_valid, uint64_t L, uint64_t p)
{
    const uint32_t rest = fqd_overlap(SK_FQ_ADAPTER_MAX_LEN, L, p);
    const uint64_t rest_mask = fqd_low_mask(rest);
    uint32_t best = FQD_NO_ADAPTER;
#pragma unroll
    for (uint32_t a = n; a-- > 0;) { // downwards: the lowest adapter is the last to write
        const uint32_t v = rest < c->len[a] ? rest : c->len[a];
        const uint32_t m = fqd_mismatches_under(win_lo, win_hi, win_valid, c->lo[a], c->hi[a], rest_mask & fqd_low_mask(c->len[a]));
        if (fqd_is_hit(v, m, c->min_overlap, c->permille)) best = a;
    }
    return best;
}

// ---- one read ----------------------------------------------------------------------------------------
struct fqd_read {
    uint64_t L;   // the line's length
    int32_t five, three;
    uint32_t hit; // 0: none, and then p, a, v, m, A are 0
    uint32_t a, v, m, A;
    uint64_t p;
};

FQD_FN bool fqd_kept(const fqd_read *r) { return r->three >= 0; }

FQD_FN uint32_t fqd_clip_word(const fqd_read *r) { return r->hit ? (r->a << 24) | (uint32_t)r->p : SK_FQ_CLIP_NONE; }

// what a read without a hit adds to word w: it is a read, and kept or not (the kernel's short way for most reads)
FQD_FN uint64_t fqd_miss_word(uint32_t w, const fqd_read *r) { return w == FQD_W_READS ? 1u : w == FQD_W_KEPT ? fqd_kept(r) : 0u; }

// what one read adds to word w of the struct, FQD_W_READS <= w <= FQD_W_BASES_HIT_OUT (the pair words: fqd_pair_word)
FQD_FN uint64_t fqd_read_word(uint32_t w, const fqd_read *r)
{
    const bool kept = fqd_kept(r), hit = r->hit != 0;
    const bool out = hit && kept && r->p < (uint64_t)r->three; // three >= 0 here
    if (!hit || w == FQD_W_READS || w == FQD_W_KEPT) return fqd_miss_word(w, r);
    if (w == FQD_W_READS_HIT) return 1;
    if (w == FQD_W_READS_HIT_KEPT) return kept;
    if (w >= FQD_W_HITS && w < FQD_W_HITS + 8) return w - FQD_W_HITS == r->a;
    if (w == FQD_W_HITS_FULL) return r->v == r->A;
    if (w == FQD_W_HITS_AT_0) return r->p == 0;
    if (w == FQD_W_MISMATCHES) return r->m;
    if (w == FQD_W_BASES_BEHIND) return r->L - r->p;
    if (w == FQD_W_READS_HIT_OUT) return out;
    if (w == FQD_W_BASES_HIT_OUT) {
        const uint64_t five = (uint64_t)(r->five > 0 ? r->five : 0);
        return out ? (uint64_t)r->three - (r->p > five ? r->p : five) : 0;
    }
    return 0;
}

// what pair (r1, r2) adds to word w, FQD_W_PAIRS_BOTH <= w <= FQD_W_PAIRS_SAME_CLIP
FQD_FN uint64_t fqd_pair_word(uint32_t w, const fqd_read *r1, const fqd_read *r2)
{
    const bool h1 = r1->hit != 0, h2 = r2->hit != 0;
    if (w == FQD_W_PAIRS_BOTH) return h1 && h2;
    if (w == FQD_W_PAIRS_ONE) return h1 != h2;
    if (w == FQD_W_PAIRS_SAME_CLIP) return h1 && h2 && r1->p == r2->p;
    return 0;
}

#endif
