// sk_fastq_rejects.hip -- the rejects text over a finished text call's workspace and texts
// (sk_trim_fastq_rejects_device_async): the rule of sk_fastq_rejects.h, the records of the reads that were not kept copied
// out whole.
//
// Launches on the text call's stream, behind its emission; no inter-workgroup waiting, and the result does not depend on
// the order of workgroups.  The shape is the emission's (sk_fastq.hip, steps 9 to 12):
//   1 count   per block of SK_FQ_BLOCK_READS reads: the selected records and their bytes.  A lane takes eight consecutive
//             reads, the first even, so a pair lies in one lane.  Uniform exit (zeros) on a void call and at or beyond NREAL.
//   2 scan    one workgroup: block bases in place, the totals, the fit verdict against both capacities; it writes the
//             whole header, the two output words among it, whatever the call's validity.
//   3 place   the output offset and read of every selected record into the table, and out->record_index; only when
//             the scan said the call writes.
//   4 gather  partitioned by OUTPUT bytes, as fq_gather: a workgroup takes chunks of FQJ_GCHUNK output bytes, finds the
//             first record by a 64-ary search in the table and stages the offsets and the text positions of the next
//             FQJ_WIN records in LDS (further ones are searched in global memory).  A lane builds an aligned 16-byte
//             granule from aligned 16-byte loads funnel-shifted by v_alignbyte (fqj_load_window, a copy of sk_fastq.hip's
//             fq_load_window) and stores it with one aligned 16-byte store; only the output's last granule is stored by
//             bytes, so nothing beyond `bytes` is written.  No 16-byte block without a wanted byte is loaded; a record's
//             closing '\n' is an immediate.  A record's length is off(k + 1) - off(k): the gather loads one descriptor
//             word per staged record, the name start.
// The grids are sized from text_bytes on the host.  Every descriptor index is bounded by the slots of the section, every
// text byte by in->bytes[i] (fqj_span, and once more at the load), every read by the bound N.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_fastq_order.h"
#include "sk_fastq_rejects.h"

namespace {

typedef unsigned fqj_u4 __attribute__((ext_vector_type(4)));
typedef unsigned __int128 fqj_u128;

#define FQJ_THREADS 256
#define FQJ_PER_THREAD (FQJ_BLOCK_READS / FQJ_THREADS) // consecutive reads of one lane (even: pairs stay whole)
#define FQJ_GPL 2                                      // 16-byte granules per lane and chunk
#define FQJ_GCHUNK (FQJ_THREADS * 16u * FQJ_GPL)
#define FQJ_WIN 128 // records of a gather chunk staged in LDS

static_assert(FQJ_BLOCK_READS == SK_FQ_BLOCK_READS, "the blocks are the emission's");
static_assert(FQJ_PER_THREAD % 2 == 0, "a lane must hold whole pairs");

struct fqj_args {
    const uint64_t *hdr;         // the text call's header
    const uint64_t *order_words; // ordered kinds: where the SK_FQO_H_* words lie
    const uint64_t *desc;        // 5 words per slot, input 0's slots first
    const sk_cut_dev *cuts;
    uint64_t *my;  // FQJ_HDR_WORDS
    uint64_t *blk; // FQJ_BLOCK_WORDS per block
    uint64_t *tab; // 2 words per selected record: output offset, read
    const uint8_t *text[2];
    uint64_t bytes[2];
    uint64_t slots0;     // input 0's slots: input 1's descriptors lie behind them
    uint64_t slot_bound; // slots of the descriptor section
    uint64_t n_bound;    // the most reads the packed batch can hold
    uint64_t n_blocks;
    uint8_t *out;
    uint64_t cap;
    uint64_t *index;
    uint64_t rec_cap;
    int32_t kind;
    int32_t mode;  // the call's mode
    int32_t split; // its framing mode is SK_TRIM_PE_SPLIT
    int32_t pairs; // SK_FQ_REJECTS_PAIRS
    int32_t flags;
};

__device__ __forceinline__ bool fqj_valid(const fqj_args &a)
{
    const uint64_t *h = a.hdr;
    const bool piece = a.kind == SK_FQ_REPORT_PIECE || a.kind == SK_FQ_REPORT_ORDERED_PIECE;
    const uint64_t range0 = piece ? h[SK_FQP_H_RANGE0] : ~0ull;
    bool refused = false;
    if (a.order_words) {
        refused = a.order_words[SK_FQO_H_LONG] != ~0ull || a.order_words[SK_FQO_H_OVERFLOW] != 0;
        if (a.kind == SK_FQ_REPORT_ORDERED_PIECE && a.order_words[SK_FQOP_X_INHERITED]) refused = true; // void
    }
    return fqj_call_valid(h[SK_FQ_H_FMT], h[SK_FQ_H_RANGE], range0, refused, h[SK_FQ_H_MODE], a.mode);
}

// the reads of the call, never more than the sections hold
__device__ __forceinline__ uint64_t fqj_reads(const fqj_args &a) { return min(a.hdr[SK_FQ_H_NREAL], a.n_bound); }

// read r's text and its span in it: through the descriptor slot, or an empty span at the text's end where there is none
__device__ __forceinline__ int fqj_record(const fqj_args &a, uint64_t r, uint64_t *at, uint64_t *len)
{
    const int i = a.split ? (int)(r & 1) : 0;
    const uint64_t k = a.split ? r >> 1 : r;
    const uint64_t slot = (i ? a.slots0 : 0) + k;
    uint64_t s0 = a.bytes[i], e3 = a.bytes[i];
    if (slot < a.slot_bound) {
        s0 = a.desc[5 * slot];
        e3 = a.desc[5 * slot + 4];
    }
    fqj_span(s0, e3, a.bytes[i], at, len);
    return i;
}

// the FQJ_PER_THREAD reads of this lane (first even): bytes of the record of a selected read, 0 for the others
__device__ __forceinline__ void fqj_lane_reads(const fqj_args &a, uint64_t first, uint64_t R, uint64_t (&bytes)[FQJ_PER_THREAD])
{
    bool is_read[FQJ_PER_THREAD], kept[FQJ_PER_THREAD];
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        is_read[j] = first + j < R;
        kept[j] = true;
        if (is_read[j]) kept[j] = fqj_kept(a.cuts[first + j].three);
    }
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        bytes[j] = 0;
        const bool mate_kept = !is_read[j ^ 1] || kept[j ^ 1];
        if (is_read[j] && fqj_selected(kept[j], mate_kept, a.pairs != 0)) {
            uint64_t at, len;
            fqj_record(a, first + j, &at, &len);
            bytes[j] = fqj_record_bytes(len);
        }
    }
}

// exclusive prefix sums of two values over the workgroup; total[] = the sums over it.  lds: 8 words.  (== fq_block_scan<2>)
__device__ __forceinline__ void fqj_block_scan(uint64_t (&v)[2], uint64_t (&total)[2], uint64_t *lds)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc[2] = {v[0], v[1]};
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const uint64_t t = __shfl_up(inc[i], d);
            if (lane >= d) inc[i] += t;
        }
    }
    if (lane == 63) {
        lds[w * 2] = inc[0];
        lds[w * 2 + 1] = inc[1];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        uint64_t base = 0, tot = 0;
#pragma unroll
        for (int ww = 0; ww < FQJ_THREADS / 64; ++ww) {
            const uint64_t x = lds[ww * 2 + i];
            base += ww < w ? x : 0;
            tot += x;
        }
        v[i] = base + inc[i] - v[i];
        total[i] = tot;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------
// 1 count
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQJ_THREADS) sk_fq_rejects_count_kernel(fqj_args a)
{
    __shared__ uint64_t lds[8];
    uint64_t *blk = a.blk + (uint64_t)blockIdx.x * FQJ_BLOCK_WORDS;
    const bool valid = fqj_valid(a); // uniform
    const uint64_t R = valid ? fqj_reads(a) : 0;
    if ((uint64_t)blockIdx.x * FQJ_BLOCK_READS >= R) { // uniform
        if (threadIdx.x < FQJ_BLOCK_WORDS) blk[threadIdx.x] = 0;
        return;
    }
    const uint64_t first = (uint64_t)blockIdx.x * FQJ_BLOCK_READS + threadIdx.x * FQJ_PER_THREAD;
    uint64_t bytes[FQJ_PER_THREAD];
    fqj_lane_reads(a, first, R, bytes);
    uint64_t v[2] = {0, 0}, tot[2];
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        v[0] += bytes[j] != 0; // a record has its '\n' at least
        v[1] += bytes[j];
    }
    fqj_block_scan(v, tot, lds);
    if (threadIdx.x == 0) {
        blk[0] = tot[0];
        blk[1] = tot[1];
    }
}

// ------------------------------------------------------------------------------------------
// 2 scan
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQJ_THREADS) sk_fq_rejects_scan_kernel(fqj_args a)
{
    __shared__ uint64_t lds[8];
    const bool valid = fqj_valid(a); // uniform
    uint64_t run[2] = {0, 0};
    if (valid) {
        for (uint64_t b0 = 0; b0 < a.n_blocks; b0 += FQJ_THREADS) {
            const uint64_t b = b0 + threadIdx.x;
            uint64_t v[2], tot[2];
            v[0] = b < a.n_blocks ? a.blk[b * FQJ_BLOCK_WORDS] : 0;
            v[1] = b < a.n_blocks ? a.blk[b * FQJ_BLOCK_WORDS + 1] : 0;
            fqj_block_scan(v, tot, lds);
            if (b < a.n_blocks) {
                a.blk[b * FQJ_BLOCK_WORDS] = run[0] + v[0];
                a.blk[b * FQJ_BLOCK_WORDS + 1] = run[1] + v[1];
            }
            run[0] += tot[0];
            run[1] += tot[1];
        }
    }
    if (threadIdx.x < FQJ_HDR_WORDS) {
        const bool produced = a.out != nullptr;
        const bool fit = fqj_fits(valid, produced, run[1], a.cap, a.index != nullptr, run[0], a.rec_cap);
        uint64_t x = 0;
        switch (threadIdx.x) {
        case FQJ_H_RECORDS: x = run[0]; break;
        case FQJ_H_BYTES: x = run[1]; break;
        case FQJ_H_READS: x = valid ? fqj_reads(a) : 0; break;
        case FQJ_H_VALID: x = valid; break;
        case FQJ_H_FLAGS: x = (uint64_t)(uint32_t)a.flags; break;
        case FQJ_H_PRODUCED: x = produced; break;
        case FQJ_H_WRITTEN: x = fit; break;
        case FQJ_H_OUT_BYTES: x = fit ? run[1] : 0; break;
        default: break;
        }
        a.my[threadIdx.x] = x;
    }
}

// ------------------------------------------------------------------------------------------
// 3 place
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQJ_THREADS) sk_fq_rejects_place_kernel(fqj_args a)
{
    __shared__ uint64_t lds[8];
    if (!a.my[FQJ_H_WRITTEN]) return; // uniform: void, counting, or beyond a capacity
    const uint64_t R = fqj_reads(a);
    if ((uint64_t)blockIdx.x * FQJ_BLOCK_READS >= R) return; // uniform
    const uint64_t n_rec = min(a.my[FQJ_H_RECORDS], a.n_bound);
    const uint64_t first = (uint64_t)blockIdx.x * FQJ_BLOCK_READS + threadIdx.x * FQJ_PER_THREAD;
    uint64_t bytes[FQJ_PER_THREAD];
    fqj_lane_reads(a, first, R, bytes);
    uint64_t v[2] = {0, 0}, tot[2];
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        v[0] += bytes[j] != 0;
        v[1] += bytes[j];
    }
    fqj_block_scan(v, tot, lds);
    const uint64_t *blk = a.blk + (uint64_t)blockIdx.x * FQJ_BLOCK_WORDS;
    uint64_t k = v[0] + blk[0], b = v[1] + blk[1];
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        if (!bytes[j]) continue;
        if (k < n_rec) { // always, in a workspace nobody else writes: the table and the index hold n_rec
            a.tab[2 * k] = b;
            a.tab[2 * k + 1] = first + j;
            if (a.index) a.index[k] = first + j;
        }
        ++k;
        b += bytes[j];
    }
}

// ------------------------------------------------------------------------------------------
// 4 gather
// ------------------------------------------------------------------------------------------
// the n (1..16) bytes at p as the first bytes of a granule, from aligned 16-byte loads only (== fq_load_window of
// sk_fastq.hip): both blocks touched hold a byte of [p, p + n)
__device__ __forceinline__ fqj_u4 fqj_load_window(const uint8_t *p, int n)
{
    const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
    const fqj_u4 *blk = reinterpret_cast<const fqj_u4 *>(ad & ~(uintptr_t)15);
    const int sh = (int)(ad & 15);
    const fqj_u4 lo = blk[0];
    if (sh == 0) return lo;
    const fqj_u4 hi = sh + n > 16 ? blk[1] : lo;
    const int s4 = sh >> 2, sb = sh & 3;
    const uint32_t x0 = lo.x, x1 = lo.y, x2 = lo.z, x3 = lo.w, x4 = hi.x, x5 = hi.y, x6 = hi.z, x7 = hi.w;
    const uint32_t y0 = s4 == 0 ? x0 : s4 == 1 ? x1 : s4 == 2 ? x2 : x3;
    const uint32_t y1 = s4 == 0 ? x1 : s4 == 1 ? x2 : s4 == 2 ? x3 : x4;
    const uint32_t y2 = s4 == 0 ? x2 : s4 == 1 ? x3 : s4 == 2 ? x4 : x5;
    const uint32_t y3 = s4 == 0 ? x3 : s4 == 1 ? x4 : s4 == 2 ? x5 : x6;
    const uint32_t y4 = s4 == 0 ? x4 : s4 == 1 ? x5 : s4 == 2 ? x6 : x7;
    fqj_u4 r;
    r.x = __builtin_amdgcn_alignbyte(y1, y0, sb);
    r.y = __builtin_amdgcn_alignbyte(y2, y1, sb);
    r.z = __builtin_amdgcn_alignbyte(y3, y2, sb);
    r.w = __builtin_amdgcn_alignbyte(y4, y3, sb);
    return r;
}

__device__ __forceinline__ fqj_u128 fqj_to_u128(fqj_u4 v)
{
    return (fqj_u128)v.x | ((fqj_u128)v.y << 32) | ((fqj_u128)v.z << 64) | ((fqj_u128)v.w << 96);
}

__device__ __forceinline__ fqj_u4 fqj_from_u128(fqj_u128 v)
{
    fqj_u4 r;
    r.x = (uint32_t)v;
    r.y = (uint32_t)(v >> 32);
    r.z = (uint32_t)(v >> 64);
    r.w = (uint32_t)(v >> 96);
    return r;
}

// bytes [0, n) of x to bytes [d, d + n) of acc (d + n <= 16)
__device__ __forceinline__ void fqj_put(fqj_u128 &acc, fqj_u128 x, int d, int n)
{
    const fqj_u128 m = n >= 16 ? ~(fqj_u128)0 : (((fqj_u128)1 << (8 * n)) - 1);
    acc |= (x & m) << (8 * d);
}

__device__ __forceinline__ void fqj_store_granule(uint8_t *dst, uint64_t g, fqj_u128 x, int n)
{
    if (n == 16) {
        __builtin_nontemporal_store(fqj_from_u128(x), reinterpret_cast<fqj_u4 *>(dst + g));
    } else {
        for (int i = 0; i < n; ++i) dst[g + i] = (uint8_t)(x >> (8 * i));
    }
}

// where record k's span starts: its text (bit 63) and the offset in it
#define FQJ_SRC_INPUT (1ull << 63)
__device__ __forceinline__ uint64_t fqj_source(const fqj_args &a, uint64_t read)
{
    uint64_t at, len;
    const int i = fqj_record(a, min(read, a.n_bound), &at, &len);
    return at | (i ? FQJ_SRC_INPUT : 0);
}

// bytes [rel, rel + n) of a record of `rec` bytes whose span starts at src to bytes [d, d + n) of acc: the table of
// fqj_pieces, a span of rec - 1 bytes and the immediate
__device__ __forceinline__ void fqj_fill(const fqj_args &a, uint64_t src, uint64_t rec, uint64_t rel, int d, int n, fqj_u128 &acc)
{
    const int i = (src & FQJ_SRC_INPUT) ? 1 : 0;
    fqj_piece pc[2];
    fqj_pieces(src & ~FQJ_SRC_INPUT, rec - 1, pc);
    if (rel < pc[0].len) {
        const uint64_t p = pc[0].at + rel;
        int t = (int)min((uint64_t)n, pc[0].len - rel);
        const uint64_t room = a.bytes[i] - min(a.bytes[i], p); // == the span's rest, or more, wherever place saw this descriptor
        if ((uint64_t)t <= room) fqj_put(acc, fqj_to_u128(fqj_load_window(a.text[i] + p, t)), d, t);
        rel += t;
        d += t;
        n -= t;
    }
    if (n > 0 && rel == pc[0].len) fqj_put(acc, (fqj_u128)pc[1].imm, d, 1);
}

__global__ void __launch_bounds__(FQJ_THREADS) sk_fq_rejects_gather_kernel(fqj_args a)
{
    __shared__ uint64_t s_off[FQJ_WIN + 1];
    __shared__ uint64_t s_src[FQJ_WIN];
    __shared__ uint64_t s_cur;
    const int t = threadIdx.x, lane = t & 63;
    if (!a.my[FQJ_H_WRITTEN]) return; // uniform
    const uint64_t total = min(a.my[FQJ_H_BYTES], a.cap), R = min(a.my[FQJ_H_RECORDS], a.n_bound);
    if (total == 0 || R == 0) return;
    const uint64_t n_chunks = (total + FQJ_GCHUNK - 1) / FQJ_GCHUNK;
    const uint64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * per, c1 = min(c0 + per, n_chunks);
    if (c0 >= c1) return; // uniform
    // offset of record k (k <= R; off(R) = total)
    auto off = [&](uint64_t k) { return k < R ? a.tab[2 * k] : total; };
    // the record holding the span's first byte: a 64-ary search by wave 0 (the last k < R with off(k) <= x)
    if (t < 64) {
        const uint64_t x = c0 * FQJ_GCHUNK;
        uint64_t lo = 0, hi = R;
        while (hi - lo > 1) {
            const uint64_t step = (hi - lo + 63) / 64, p = lo + lane * step;
            const uint64_t mk = __builtin_amdgcn_ballot_w64(p < hi && off(p) <= x) | 1ull; // lane 0's probe holds: off(lo) <= x
            lo += (uint64_t)(63 - __builtin_clzll(mk)) * step;
            hi = min(hi, lo + step);
        }
        if (t == 0) s_cur = lo;
    }
    __syncthreads();
    uint64_t cur = s_cur;
    for (uint64_t c = c0; c < c1; ++c) {
        if (t <= FQJ_WIN) s_off[t] = cur + t <= R ? off(cur + t) : ~0ull;
        if (t < FQJ_WIN && cur + t < R) s_src[t] = fqj_source(a, a.tab[2 * (cur + t) + 1]);
        __syncthreads();
        const uint64_t win_end = s_off[FQJ_WIN];
        uint64_t k_last = cur;
#pragma unroll
        for (int u = 0; u < FQJ_GPL; ++u) {
            const uint64_t g = c * FQJ_GCHUNK + (uint64_t)u * (FQJ_THREADS * 16) + 16u * t;
            if (g >= total) break;
            uint64_t k;
            if (g < win_end) {
                int lo = 0, hi = FQJ_WIN; // s_off[lo] <= g < s_off[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_off[mid] <= g) lo = mid; else hi = mid;
                }
                k = cur + lo;
            } else {
                uint64_t lo = min(cur + FQJ_WIN, R - 1), hi = R; // off(lo) <= g < off(hi)
                while (hi - lo > 1) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (off(mid) <= g) lo = mid; else hi = mid;
                }
                k = lo;
            }
            k_last = k;
            const uint64_t end = min(g + 16, total);
            fqj_u128 acc = 0;
            uint64_t pos = g;
            while (pos < end && k < R) { // a record has a byte at least: at most 16 turns
                const uint64_t i = k - cur;
                const uint64_t b = i < FQJ_WIN ? s_off[i] : off(k);
                const uint64_t e = i < FQJ_WIN ? s_off[i + 1] : off(k + 1);
                if (e <= pos) { // the record ended
                    ++k;
                    continue;
                }
                if (pos < b) break; // only where the table is no table
                const uint64_t src = i < FQJ_WIN ? s_src[i] : fqj_source(a, a.tab[2 * k + 1]);
                const uint64_t pe = min(e, end);
                fqj_fill(a, src, e - b, pos - b, (int)(pos - g), (int)(pe - pos), acc);
                pos = pe;
            }
            fqj_store_granule(a.out, g, acc, (int)(end - g));
        }
        // the next chunk starts at or after the record of the last lane's last granule
        if (t == FQJ_THREADS - 1) s_cur = min(k_last, R - 1);
        __syncthreads();
        cur = s_cur;
    }
}

} // namespace

// the arguments have passed the checks of sk_trim_fastq_rejects_device_async (sk_capi.hip)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_rejects(const sk_fastq_report_source *src,
                                                                                    const sk_fastq_input *in, int mode,
                                                                                    const sk_fastq_output *out, int flags,
                                                                                    void *workspace, int cu_count,
                                                                                    hipStream_t stream)
{
    sk_fq_layout L;
    sk_fq_layout_of(src->text_bytes, src->trunc_n, &L);
    const uint8_t *base = static_cast<const uint8_t *>(src->workspace);
    uint8_t *mine = static_cast<uint8_t *>(workspace);
    uint64_t shift = 0;
    fqj_args a = {};
    a.hdr = reinterpret_cast<const uint64_t *>(base);
    if (src->kind == SK_FQ_REPORT_ORDERED) {
        shift = sk_fq_order_shift(src->batch_capacity);
        a.order_words = a.hdr;
    } else if (src->kind == SK_FQ_REPORT_ORDERED_PIECE) {
        shift = sk_fq_order_piece_shift(src->batch_capacity);
        a.order_words = reinterpret_cast<const uint64_t *>(base + SK_FQOP_EXT_BYTES_AT);
    }
    a.desc = reinterpret_cast<const uint64_t *>(base + shift + L.desc);
    a.cuts = reinterpret_cast<const sk_cut_dev *>(base + shift + L.cuts);
    a.my = reinterpret_cast<uint64_t *>(mine);
    a.blk = reinterpret_cast<uint64_t *>(mine + fqj_blocks_at());
    a.tab = reinterpret_cast<uint64_t *>(mine + fqj_table_at(src->text_bytes));
    a.kind = (int32_t)src->kind;
    a.mode = mode;
    a.split = fqj_framing_mode(mode) == SK_TRIM_PE_SPLIT;
    a.pairs = (flags & SK_FQ_REJECTS_PAIRS) != 0;
    a.flags = flags;
    a.n_bound = fqj_reads_bound(src->text_bytes);
    a.n_blocks = fqj_blocks(src->text_bytes);
    a.slot_bound = (L.offsets - L.desc) / 40;
    const int n_in = a.split ? 2 : 1;
    for (int i = 0; i < n_in; ++i) {
        a.text[i] = static_cast<const uint8_t *>(in->text[i]);
        a.bytes[i] = in->text[i] ? in->bytes[i] : 0;
    }
    a.slots0 = sk_fq_slots(in->bytes[0]);
    if (out && out->text) {
        a.out = out->text;
        a.cap = out->capacity;
        a.index = out->record_index;
        a.rec_cap = out->record_capacity;
    }
    const dim3 threads(FQJ_THREADS);
    hipLaunchKernelGGL(sk_fq_rejects_count_kernel, dim3((unsigned)a.n_blocks), threads, 0, stream, a);
    hipLaunchKernelGGL(sk_fq_rejects_scan_kernel, dim3(1), threads, 0, stream, a);
    if (a.out) {
        hipLaunchKernelGGL(sk_fq_rejects_place_kernel, dim3((unsigned)a.n_blocks), threads, 0, stream, a);
        // the output is fqj_bound(text_bytes) at most; a persistent grid with no second round, as the emission's gather
        uint64_t grid = (fqj_bound(src->text_bytes) + FQJ_GCHUNK - 1) / FQJ_GCHUNK;
        const uint64_t full = (uint64_t)cu_count * SK_TRIM_GATHER_WG_PER_CU;
        if (grid > full) grid = full;
        hipLaunchKernelGGL(sk_fq_rejects_gather_kernel, dim3((unsigned)grid), threads, 0, stream, a);
    }
    return hipGetLastError();
}
