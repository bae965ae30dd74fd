// sk_bgzf_search.h -- a match search for the block encoder of sk_deflate_block.h (SK_BGZF_SEARCH), written like it as
// PHASES that the 64 lanes of one wavefront run in step (a barrier between phases).  Only the tokens change: everything
// after the tokenizer (codes, header, sizing, placing, emitting) is sk_deflate_block.h as it stands.
//
// 1 candidates, position-parallel.  The block is walked in CHUNKS of SKS_CHUNK bytes.  For chunk c every lane takes
//   positions of the chunk, hashes the 4 bytes there, reads the SKS_WAYS ways of the hash's bucket, verifies each by
//   comparing bytes (hashes collide) and keeps the longest match (<= 258 bytes, <= 32 768 back, not past the end of the
//   position's line), the nearest among equals: one word per position in the block's candidate scratch.  After a barrier
//   the lanes insert the chunk's positions into way c mod SKS_WAYS of their buckets.
// 2 tokens, line-parallel: skd_phase_tokenize with a third offer at every position it reaches, the stored candidate.
//
// DETERMINISM.  The table is a function of the text alone: after chunk c, way w of bucket h holds the LATEST position
// with hash h among the chunks <= c that are congruent to w (mod SKS_WAYS), or nothing.  Insertion is an atomic MAX and
// nothing else, which commutes, so neither the order of the lanes nor the order of their positions matters; a chunk is
// searched before it is inserted (a barrier on either side), so a search sees whole chunks only.  Two ways share a
// 32-bit word (16 bits each: position + 1, 0 = empty).  During the insertion of chunk c only way c mod SKS_WAYS
// changes, so the OTHER half of the word is stable and every lane reads the same value of it; positions only grow from
// chunk to chunk, so every value offered to the MAX, (stable half, new position), exceeds the word as it stood and they
// differ in the inserted half alone: the MAX leaves the stable half as it was and the largest position in the other.
// The candidate words are written once each, by the lane that owns the position, and the tokens are a function of the
// text, the line table and the candidate words.  On the host the lanes run one after the other, in any order
// (tests/bgzf_search/search_host.cpp), and give the same bytes.
#ifndef SK_BGZF_SEARCH_H
#define SK_BGZF_SEARCH_H

#include "sk_deflate_block.h"

#ifdef __HIPCC__
#define SKS_ATOMIC_MAX(p, v) atomicMax((p), (v))
#else
#define SKS_ATOMIC_MAX(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#endif

#define SKS_BUCKET_BITS 11
#define SKS_BUCKETS (1u << SKS_BUCKET_BITS)
#define SKS_WAYS 4u   /* even: two ways to a word */
#define SKS_CHUNK 64u /* a multiple of SKD_LANES */
#define SKS_MIN_MATCH 5
#define SKS_MAX_MATCH 258u
#define SKS_MAX_DIST 32768u

// the bucket table: LDS on the device (16 KiB)
struct sks_shared {
    uint32_t way2[SKS_BUCKETS * SKS_WAYS / 2]; // bucket h, ways 2k (low half) and 2k + 1 (high half) at [h * WAYS / 2 + k]
};

SKD_FN uint32_t sks_hash(const uint8_t *p)
{
    const uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return (v * 2654435761u) >> (32 - SKS_BUCKET_BITS);
}

// the table holds nothing from the block before
SKD_FN void sks_phase_clear(sks_shared *ss, int lane)
{
    for (uint32_t i = (uint32_t)lane; i < SKS_BUCKETS * SKS_WAYS / 2; i += SKD_LANES) ss->way2[i] = 0;
}

// the end of the line that holds position j (lines as skd_phase_close_lines left them: the last one runs to n)
SKD_FN uint32_t sks_line_end(const skd_shared *sh, uint32_t j)
{
    uint32_t lo = 0, hi = sh->n_lines; // line_start[lo] <= j < line_start[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (sh->line_start[mid] <= j) lo = mid;
        else hi = mid;
    }
    return sh->line_start[hi];
}

// ---- phase S1: the candidates of chunk c, from the chunks before it
SKD_FN void sks_phase_candidates(const skd_shared *sh, const sks_shared *ss, const uint8_t *p, uint32_t n, uint32_t c,
                                 uint32_t *cand, int lane)
{
    const uint32_t base = c * SKS_CHUNK;
    for (uint32_t q = (uint32_t)lane; q < SKS_CHUNK && base + q < n; q += SKD_LANES) {
        const uint32_t j = base + q;
        uint32_t best = 0, best_dist = 0;
        uint32_t lim = sks_line_end(sh, j) - j;
        if (lim > SKS_MAX_MATCH) lim = SKS_MAX_MATCH;
        if (lim >= SKS_MIN_MATCH && c > 0) { // j + 4 <= n follows
            const uint32_t *w2 = ss->way2 + sks_hash(p + j) * (SKS_WAYS / 2);
            for (uint32_t w = 0; w < SKS_WAYS; ++w) {
                const uint32_t e = (w2[w >> 1] >> (16 * (w & 1))) & 0xffffu;
                if (!e) continue;
                const uint32_t r = e - 1, dist = j - r; // r lies in an earlier chunk: r < j
                if (dist > SKS_MAX_DIST) continue;
                uint32_t m = 0;
                while (m < lim && p[r + m] == p[j + m]) ++m;
                if (m > best || (m == best && dist < best_dist)) {
                    best = m;
                    best_dist = dist;
                }
            }
        }
        cand[j] = best >= SKS_MIN_MATCH ? skd_match(best, best_dist) : 0u;
    }
}

// ---- phase S2: chunk c into way c mod SKS_WAYS (positions with 4 bytes of text behind them)
SKD_FN void sks_phase_insert(sks_shared *ss, const uint8_t *p, uint32_t n, uint32_t c, int lane)
{
    const uint32_t base = c * SKS_CHUNK, w = c % SKS_WAYS;
    for (uint32_t q = (uint32_t)lane; q < SKS_CHUNK && base + q + 4 <= n; q += SKD_LANES) {
        const uint32_t j = base + q;
        uint32_t *word = ss->way2 + sks_hash(p + j) * (SKS_WAYS / 2) + (w >> 1);
        const uint32_t keep = *word; // its other half is stable during this phase
        SKS_ATOMIC_MAX(word, (w & 1) ? ((j + 1) << 16 | (keep & 0xffffu)) : ((keep & 0xffff0000u) | (j + 1)));
    }
}

// ---- phase 1 with the search: skd_phase_tokenize, and at each position the lane reaches the stored candidate as a third
// offer.  The longest offer that passes its minimum wins (6 for a column copy, 5 for a run, 5 for a candidate); among
// equals the column copy, then the run, as without the search.
SKD_FN void sks_phase_tokenize(skd_shared *sh, const uint8_t *p, const uint32_t *cand, uint32_t *tok, int lane)
{
    const uint32_t L = sh->n_lines;
    for (uint32_t l = (uint32_t)lane; l < L; l += SKD_LANES) {
        const uint32_t i = sh->line_start[l], end = sh->line_start[l + 1];
        uint32_t *t = tok + i;
        uint32_t nt = 0;
        const bool has_ref = l >= 4;
        const uint32_t ref_line = has_ref ? sh->line_start[l - 4] : 0, ref_end = has_ref ? sh->line_start[l - 3] : 0;
        bool use_ref = false;
        if (has_ref && i - ref_line <= 32768) {
            uint32_t head = SKD_MIN_ALIGNED;
            if (end - i < head) head = end - i;
            if (ref_end - ref_line < head) head = ref_end - ref_line;
            use_ref = head > 0;
            for (uint32_t k = 0; k < head && use_ref; ++k) use_ref = p[i + k] == p[ref_line + k];
        }
        int shift = 0;
        uint32_t j = i;
        while (j < end) {
            uint32_t best = 0, best_ref = 0;
            if (use_ref) {
                const int tries[5] = {0, 1, -1, 2, -2};
                for (int q = 0; q < 5; ++q) {
                    const int col = (int)(j - i) + shift + tries[q];
                    if (col < 0) continue;
                    const uint32_t r = ref_line + (uint32_t)col;
                    if (r >= ref_end || j - r > 32768) continue;
                    uint32_t lim = end - j;
                    if (ref_end - r < lim) lim = ref_end - r;
                    if (lim > 258) lim = 258;
                    uint32_t m = 0;
                    while (m < lim && p[r + m] == p[j + m]) ++m;
                    if (m > best) {
                        best = m;
                        best_ref = r;
                    }
                    if (best >= SKD_MIN_ALIGNED) break;
                }
            }
            uint32_t run = 0;
            if (j > 0 && p[j] == p[j - 1]) {
                uint32_t lim = end - j;
                if (lim > 258) lim = 258;
                run = 1;
                while (run < lim && p[j + run] == p[j]) ++run;
            }
            const uint32_t offer = cand[j];
            uint32_t found = offer ? ((offer >> 15) & 0xff) + 3 : 0; // >= SKS_MIN_MATCH, within the line
            if (best < SKD_MIN_ALIGNED) best = 0;
            if (run < SKD_MIN_RUN) run = 0;
            uint32_t token;
            if (found > best && found > run) {
                token = offer;
                j += found;
            } else if (best && best >= run) {
                token = skd_match(best, j - best_ref);
                shift = (int)best_ref - (int)ref_line - (int)(j - i);
                j += best;
            } else if (run) {
                token = skd_match(run, 1);
                j += run;
            } else {
                token = p[j];
                ++j;
            }
            t[nt++] = token;
            if (token >> 31) {
                uint32_t s, eb, ex;
                skd_len_code(((token >> 15) & 0xff) + 3, &s, &eb, &ex);
                SKD_ATOMIC_ADD(&sh->lfreq[257 + s], 1u);
                skd_dist_code((token & 0x7fff) + 1, &s, &eb, &ex);
                SKD_ATOMIC_ADD(&sh->dfreq[s], 1u);
            } else {
                SKD_ATOMIC_ADD(&sh->lfreq[token], 1u);
            }
        }
        sh->line_tokens[l] = nt;
    }
}

#endif
