// sk_fastq_order.h -- the reference's ingest batches and its -a T emission order for FASTQ text on the device
// (sk_trim_fastq_ordered_device_async; the rule is stated in include/sickle_amd.h and DESIGN 4.7.1).
//
// Two pieces, both plain functions of integers and of the descriptor table the framing kernels of sk_fastq.hip write
// (5 words per record: name start, then the end of each of its four lines):
//   fqo_chain    GZReader's byte-budget rule (reference src/GZReader.cpp:59-132) walked batch after batch: the table of
//                first units (batch b holds units [tab[b], tab[b + 1])) and the counts.  One walker; per batch and input
//                one binary search over the prefix content(l) = start(l) - l, the bytes of lines [0, l) without their
//                newlines.  The walk ends after batch_capacity + 1 steps at the latest.
//   fqo_unit_of  rank j of a batch of n units at T threads -> the unit: the queues of reference
//                src/trim_single.cpp:263-298 (read k to queue (k + 1) mod T) and src/trim_paired.cpp:388-403 (pair k to
//                queue k mod T), written one after the other.
// sk_fastq.hip calls them from its kernels; tests/fastq_order/order_host.cpp runs them on the host.
#ifndef SK_FASTQ_ORDER_H
#define SK_FASTQ_ORDER_H

#include <stdint.h>

#ifdef __HIPCC__
#define FQO_FN __host__ __device__ static inline
#else
#define FQO_FN static inline
#endif

// words of the workspace header (sk_device.h: SK_FQ_H_* end at 20) that only ordered calls write
#define SK_FQO_H_BATCHES 21     // batches trimmed; batch_capacity + 1 = more than the table holds
#define SK_FQO_H_UNITS 22       // reads (SE) or pairs in them
#define SK_FQO_H_LAST_UNITS 23  // units of the last batch
#define SK_FQO_H_UNBATCHED 24   // [2] complete records of each input behind the last batch
#define SK_FQO_H_MISMATCH 26    // PE split: the two inputs' batches differed in line count
#define SK_FQO_H_LONG 27        // (input << 63) | line of the lowest line gzgets would split, or ~0
#define SK_FQO_H_ERROR_BATCH 28 // batch of the record behind the format / range error, or ~0
#define SK_FQO_H_OVERFLOW 29    // the table was too small
#define SK_FQO_TABLE_BYTES_AT 256u // the table of first units follows the header's 32 words
#define SK_FQO_MIN_BATCH_LEN 20u

// start of line l of a text framed into desc (l <= the lines it holds): one load
FQO_FN uint64_t fqo_line_start(const uint64_t *desc, uint64_t l)
{
    if (l == 0) return 0;
    const uint64_t p = l - 1;
    return desc[5 * (p >> 2) + 1 + (p & 3)] + 1;
}

// bytes of lines [0, l) without their newlines
FQO_FN uint64_t fqo_content(const uint64_t *desc, uint64_t l) { return fqo_line_start(desc, l) - l; }

// The reader's next stop: the smallest line number e > c (c < nl) at which lines [a, e) hold batch_len bytes or more,
// or nl with *ended set when the text ends first.
FQO_FN uint64_t fqo_next_end(const uint64_t *desc, uint64_t nl, uint64_t a, uint64_t c, uint64_t batch_len, bool *ended)
{
    const uint64_t base = fqo_content(desc, a);
    if (fqo_content(desc, nl) - base < batch_len) {
        *ended = true;
        return nl;
    }
    uint64_t lo = c, hi = nl; // the budget is used up at hi; lo is not a candidate
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (fqo_content(desc, mid) - base >= batch_len) hi = mid; else lo = mid;
    }
    return hi;
}

struct fqo_chain_result {
    uint64_t batches, units, last_units;
    uint64_t batched_lines[2]; // lines of each input inside the batches
    uint32_t mismatch, overflow;
};

// n_in texts (2 for PE split) of nl[i] lines each; m lines per unit and text (4; 8 for interleaved pairs).  tab gets
// batches + 1 entries (capacity + 1 at most).  limit: 0, or the most batches that exist for the call.
FQO_FN void fqo_chain(const uint64_t *const desc[2], const uint64_t nl[2], int n_in, uint32_t m, uint64_t batch_len,
                      uint64_t capacity, uint64_t limit, uint64_t *tab, fqo_chain_result *res)
{
    uint64_t a[2] = {0, 0}, c[2] = {0, 0};
    bool ended[2] = {false, false};
    fqo_chain_result r = {0, 0, 0, {0, 0}, 0, 0};
    tab[0] = 0;
    for (;;) {
        if (limit && r.batches == limit) break;
        uint64_t e[2] = {0, 0}, len[2] = {0, 0};
        bool end_now[2] = {false, false};
#pragma unroll
        for (int i = 0; i < 2; ++i) { // constant bounds: the state stays in registers
            if (i >= n_in || ended[i]) continue; // no batch behind the end of the text
            if (c[i] == nl[i]) {
                e[i] = c[i];
                end_now[i] = true;
            } else {
                e[i] = fqo_next_end(desc[i], nl[i], a[i], c[i], batch_len, &end_now[i]);
            }
            len[i] = (e[i] - a[i]) - (e[i] - a[i]) % m;
        }
        if (!len[0] || (n_in == 2 && !len[1])) break; // an empty batch ends the run
        if (n_in == 2 && len[0] != len[1]) {
            r.mismatch = 1;
            break;
        }
        if (r.batches == capacity) {
            r.overflow = 1;
            break;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= n_in) continue;
            a[i] += len[i];
            c[i] = e[i];
            ended[i] = end_now[i];
        }
        r.last_units = len[0] / m;
        r.units += r.last_units;
        tab[++r.batches] = r.units;
    }
    r.batched_lines[0] = a[0];
    r.batched_lines[1] = a[1];
    *res = r;
}

// Rank j (< n) of a batch of n units written by T queues -> the unit's number in the batch.  Residues below n % T hold
// n / T + 1 units, the others n / T; PE writes residues 0 .. T - 1, SE residue T - 1 first, then 0 .. T - 2.
FQO_FN uint64_t fqo_unit_of(uint64_t j, uint64_t n, uint64_t T, bool se)
{
    const uint64_t big = n % T, lo = n / T, hi = lo + 1;
    if (se) {
        if (j < lo) return (T - 1) + j * T; // residue T - 1 is never one of the longer ones
        j -= lo;
    }
    if (j < big * hi) return j / hi + (j % hi) * T;
    j -= big * hi;
    return big + j / lo + (j % lo) * T; // lo != 0: ranks remain
}

// the batch of unit u: tab[b] <= u < tab[b + 1], u < tab[batches]
FQO_FN uint64_t fqo_batch_of(const uint64_t *tab, uint64_t batches, uint64_t u)
{
    uint64_t lo = 0, hi = batches;
    while (hi - lo > 1) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (tab[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

// Walks consecutive ranks: the batch is searched once, then ranks step across batch ends.
struct fqo_cursor {
    uint64_t b, base, n, j;
};

FQO_FN fqo_cursor fqo_cursor_at(const uint64_t *tab, uint64_t batches, uint64_t rank)
{
    fqo_cursor cu;
    cu.b = fqo_batch_of(tab, batches, rank);
    cu.base = tab[cu.b];
    cu.n = tab[cu.b + 1] - cu.base;
    cu.j = rank - cu.base;
    return cu;
}

// the unit at the cursor's rank; the cursor moves to the next rank (batches: no step behind the last batch)
FQO_FN uint64_t fqo_cursor_next(fqo_cursor &cu, const uint64_t *tab, uint64_t batches, uint64_t T, bool se)
{
    const uint64_t unit = cu.base + fqo_unit_of(cu.j, cu.n, T, se);
    if (++cu.j == cu.n && cu.b + 1 < batches) {
        ++cu.b;
        cu.base += cu.n;
        cu.n = tab[cu.b + 1] - cu.base;
        cu.j = 0;
    }
    return unit;
}

// What one lane of the emission owns: the units at the N consecutive ranks from `rank`; ~0 at ranks at or beyond `ranks`
// (<= tab[batches]).
template <int N>
FQO_FN void fqo_lane_units(const uint64_t *tab, uint64_t batches, uint64_t T, bool se, uint64_t rank, uint64_t ranks,
                           uint64_t (&units)[N])
{
#pragma unroll
    for (int j = 0; j < N; ++j) units[j] = ~0ull;
    if (rank >= ranks) return;
    fqo_cursor cu = fqo_cursor_at(tab, batches, rank);
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (rank + j < ranks) units[j] = fqo_cursor_next(cu, tab, batches, T, se);
}

#endif
