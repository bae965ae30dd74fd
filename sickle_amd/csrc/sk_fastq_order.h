// sk_fastq_order.h -- the reference's ingest batches and its -a T emission order for FASTQ text on the device
// (sk_trim_fastq_ordered_device_async; the rule is stated in include/sickle_amd.h and DESIGN 4.7.1).
//
// Two pieces, both plain functions of integers and of the descriptor table the framing kernels of sk_fastq.hip write
// (5 words per record: name start, then the end of each of its four lines):
//   fqo_chain    GZReader's byte-budget rule (reference src/GZReader.cpp:59-132) walked batch after batch: the table of
//                first units (batch b holds units [tab[b], tab[b + 1])) and the counts.  One walker; per batch and input
//                one binary search over the prefix content(l) = start(l) - l, the bytes of lines [0, l) without their
//                newlines.  The walk ends after batch_capacity + 1 steps at the latest.
//   fqo_chain_piece  the same walk over a WINDOW of the text from a state (sk_trim_fastq_ordered_piece_device_async, DESIGN
//                4.15): it commits the batches whose stop line is complete in the window and hands the state on.
//                tests/fastq_order_piece/piece_host.cpp runs it on the host.
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

// ---- ordered pieces (sk_trim_fastq_ordered_piece_device_async) -------------------------------------------------------
// The workspace of an ordered piece: the header's words 21.. are the piece's (SK_FQP_H_*, sk_device.h), so the order words
// live in an extension block of 32 words behind the header, at the same indices (SK_FQO_H_* above); the block's other
// words are the piece's own.  The table of first units follows the block.
#define SK_FQOP_EXT_BYTES_AT 256u   // the extension block
#define SK_FQOP_EXT_BYTES 256u
#define SK_FQOP_TABLE_BYTES_AT (SK_FQOP_EXT_BYTES_AT + SK_FQOP_EXT_BYTES)
#define SK_FQOP_X_STATE 0       // [8] the host's copy of *state_out (sk_fastq_order_state)
#define SK_FQOP_X_TABLE_FULL 8  // the walk stopped at a full table
#define SK_FQOP_X_UNDETERMINED 9 // the walk stopped at a batch whose stop line is not in the window yet
#define SK_FQOP_X_INHERITED 10  // state_in->failed: the piece is void
#define SK_FQOP_X_CONSUMED 11   // [2] start of the first line behind the last committed batch, offset in text[i]
#define SK_FQOP_X_BASE_BATCHES 13 // state_in->batches: local batch numbers + this are stream-wide
#define SK_FQOP_X_LAST_UNITS 14 // units of the stream's last batch so far
#define SK_FQOP_X_ENDED 15      // the run is over, at this piece's end
#define SK_FQOP_X_STICKY_MISMATCH 16 // the run ended on a PE-split mismatch, in this piece or before

// start of line l of a window whose first line starts at `first`
FQO_FN uint64_t fqo_line_start_from(const uint64_t *desc, uint64_t l, uint64_t first)
{
    return l == 0 ? first : fqo_line_start(desc, l);
}

struct fqo_piece_state { // what sk_fastq_order_state hands from piece to piece, as the walk needs it
    uint64_t carried[2];  // k_i = c_i - a_i
    uint64_t batches;     // stream-wide, for batch_limit
    uint32_t ended;
};

struct fqo_piece_result {
    uint64_t batches, units, last_units; // the piece's own; last_units 0 when it committed nothing
    uint64_t batched_lines[2];           // a_i: lines of each input inside the committed batches
    uint64_t carried[2];                 // the new k_i
    uint32_t mismatch, ended, table_full, undetermined;
};

// The reader's rule on a WINDOW (include/sickle_amd.h, sk_trim_fastq_ordered_piece_device_async): fqo_chain from a_i = 0,
// c_i = st->carried[i], over the nl[i] complete lines of each window, whose first line starts at first[i].  more: text
// follows, so a stop exists only where the budget is used up on a line of the window; else the batch is undetermined and
// the walk ends in front of it.  !more: the text's end is the reader's end of input, as in fqo_chain.  A full table ends the
// walk too (no error).  One binary search per batch and input; capacity + 1 steps at most.
FQO_FN void fqo_chain_piece(const uint64_t *const desc[2], const uint64_t nl[2], const uint64_t first[2], int n_in, uint32_t m,
                            uint64_t batch_len, uint64_t capacity, uint64_t limit, const fqo_piece_state *st, bool more,
                            uint64_t *tab, fqo_piece_result *res)
{
    uint64_t a[2] = {0, 0}, c[2] = {st->carried[0] < nl[0] ? st->carried[0] : nl[0], st->carried[1] < nl[1] ? st->carried[1] : nl[1]};
    bool fin[2] = {false, false}; // !more only: the input has ended inside a committed batch
    fqo_piece_result r = {0, 0, 0, {0, 0}, {0, 0}, 0, st->ended, 0, 0};
    tab[0] = 0;
    while (!r.ended) {
        if (limit && st->batches + r.batches >= limit) {
            r.ended = 1;
            break;
        }
        uint64_t e[2] = {0, 0}, len[2] = {0, 0};
        bool end_now[2] = {false, false}, open[2] = {false, false}; // open: undetermined
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= n_in || fin[i]) continue; // no batch behind the end of the text
            const uint64_t base = fqo_line_start_from(desc[i], a[i], first[i]) - a[i];
            if (c[i] == nl[i] || fqo_line_start_from(desc[i], nl[i], first[i]) - nl[i] - base < batch_len) {
                if (more) {
                    open[i] = true;
                    continue;
                }
                e[i] = nl[i];
                end_now[i] = true;
            } else {
                uint64_t lo = c[i], hi = nl[i]; // the budget is used up at hi; lo is not a candidate
                while (hi - lo > 1) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (fqo_line_start(desc[i], mid) - mid - base >= batch_len) hi = mid; else lo = mid; // mid > 0
                }
                e[i] = hi;
            }
            len[i] = (e[i] - a[i]) - (e[i] - a[i]) % m;
        }
        // fqo_chain's order of tests, each one only on determined batches
        if (!open[0] && !len[0]) {
            r.ended = 1;
            break;
        }
        if (open[0] || (n_in == 2 && open[1])) {
            r.undetermined = 1;
            break;
        }
        if (n_in == 2 && !len[1]) {
            r.ended = 1;
            break;
        }
        if (n_in == 2 && len[0] != len[1]) {
            r.mismatch = r.ended = 1;
            break;
        }
        if (r.batches == capacity) {
            r.table_full = 1;
            break;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if (i >= n_in) continue;
            a[i] += len[i];
            c[i] = e[i];
            fin[i] = end_now[i];
        }
        r.last_units = len[0] / m;
        r.units += r.last_units;
        tab[++r.batches] = r.units;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        r.batched_lines[i] = a[i];
        r.carried[i] = c[i] - a[i];
    }
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
