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
//             granule from aligned 16-byte loads funnel-shifted by v_alignbyte (sk_load_window, sk_device_prims.h)
//             and stores it with one aligned 16-byte store; only the output's last granule is stored by
//             bytes, so nothing beyond `bytes` is written.  No 16-byte block without a wanted byte is loaded; a record's
//             closing '\n' is an immediate.  A record's length is off(k + 1) - off(k): the gather loads one descriptor
//             word per staged record, the name start.
// The grids are sized from text_bytes on the host.  A source that names the wrong layout or the wrong texts gives a wrong
// text, no load outside the workspace and the texts: the bounds and the record's clamps are the source view's
// (sk_fastq_source.h), and a text byte is held to in->bytes[i] once more at the load.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_device_prims.h"
#include "sk_fastq_order.h"
#include "sk_fastq_rejects.h"
#include "sk_fastq_source.h"

namespace {

#define FQJ_THREADS 256
#define FQJ_PER_THREAD (FQJ_BLOCK_READS / FQJ_THREADS) // consecutive reads of one lane (even: pairs stay whole)
#define FQJ_GPL 2                                      // 16-byte granules per lane and chunk
#define FQJ_GCHUNK (FQJ_THREADS * 16u * FQJ_GPL)
#define FQJ_WIN 128 // records of a gather chunk staged in LDS

static_assert(FQJ_BLOCK_READS == SK_FQ_BLOCK_READS, "the blocks are the emission's");
static_assert(FQJ_PER_THREAD % 2 == 0, "a lane must hold whole pairs");

struct fqj_args {
    fqs_view s;    // the call behind
    uint64_t *my;  // FQJ_HDR_WORDS
    uint64_t *blk; // FQJ_BLOCK_WORDS per block
    uint64_t *tab; // 2 words per selected record: output offset, read
    uint64_t n_blocks;
    uint8_t *out;
    uint64_t cap;
    uint64_t *index;
    uint64_t rec_cap;
    int32_t pairs; // SK_FQ_REJECTS_PAIRS
    int32_t flags;
};

// the FQJ_PER_THREAD reads of this lane (first even): bytes of the record of a selected read, 0 for the others
__device__ __forceinline__ void fqj_lane_reads(const fqj_args &a, uint64_t first, uint64_t R, uint64_t (&bytes)[FQJ_PER_THREAD])
{
    bool is_read[FQJ_PER_THREAD], kept[FQJ_PER_THREAD];
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        is_read[j] = first + j < R;
        kept[j] = true;
        if (is_read[j]) kept[j] = fqj_kept(a.s.cuts[first + j].three);
    }
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        bytes[j] = 0;
        const bool mate_kept = !is_read[j ^ 1] || kept[j ^ 1];
        if (is_read[j] && fqj_selected(kept[j], mate_kept, a.pairs != 0)) {
            uint64_t at, len;
            fqs_record(a.s, first + j, &at, &len);
            bytes[j] = fqj_record_bytes(len);
        }
    }
}

// ------------------------------------------------------------------------------------------
// 1 count
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQJ_THREADS) sk_fq_rejects_count_kernel(fqj_args a)
{
    __shared__ uint64_t lds[8];
    uint64_t *blk = a.blk + (uint64_t)blockIdx.x * FQJ_BLOCK_WORDS;
    const bool valid = fqs_valid(a.s); // uniform
    const uint64_t R = valid ? fqs_reads(a.s) : 0;
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
    sk_block_scan<2, FQJ_THREADS>(v, tot, lds);
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
    const bool valid = fqs_valid(a.s); // uniform
    uint64_t run[2] = {0, 0};
    if (valid) {
        for (uint64_t b0 = 0; b0 < a.n_blocks; b0 += FQJ_THREADS) {
            const uint64_t b = b0 + threadIdx.x;
            uint64_t v[2], tot[2];
            v[0] = b < a.n_blocks ? a.blk[b * FQJ_BLOCK_WORDS] : 0;
            v[1] = b < a.n_blocks ? a.blk[b * FQJ_BLOCK_WORDS + 1] : 0;
            sk_block_scan<2, FQJ_THREADS>(v, tot, lds);
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
        case FQJ_H_READS: x = valid ? fqs_reads(a.s) : 0; break;
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
    const uint64_t R = fqs_reads(a.s);
    if ((uint64_t)blockIdx.x * FQJ_BLOCK_READS >= R) return; // uniform
    const uint64_t n_rec = min(a.my[FQJ_H_RECORDS], a.s.n_bound);
    const uint64_t first = (uint64_t)blockIdx.x * FQJ_BLOCK_READS + threadIdx.x * FQJ_PER_THREAD;
    uint64_t bytes[FQJ_PER_THREAD];
    fqj_lane_reads(a, first, R, bytes);
    uint64_t v[2] = {0, 0}, tot[2];
#pragma unroll
    for (int j = 0; j < FQJ_PER_THREAD; ++j) {
        v[0] += bytes[j] != 0;
        v[1] += bytes[j];
    }
    sk_block_scan<2, FQJ_THREADS>(v, tot, lds);
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
__device__ __forceinline__ void fqj_store_granule(uint8_t *dst, uint64_t g, sk_u128 x, int n)
{
    if (n == 16) {
        __builtin_nontemporal_store(sk_from_u128(x), reinterpret_cast<sk_u4 *>(dst + g));
    } else {
        for (int i = 0; i < n; ++i) dst[g + i] = (uint8_t)(x >> (8 * i));
    }
}

// where record k's span starts: its text (bit 63) and the offset in it
#define FQJ_SRC_INPUT (1ull << 63)
__device__ __forceinline__ uint64_t fqj_source(const fqj_args &a, uint64_t read)
{
    uint64_t at, len;
    const int i = fqs_record(a.s, min(read, a.s.n_bound), &at, &len);
    return at | (i ? FQJ_SRC_INPUT : 0);
}

// bytes [rel, rel + n) of a record of `rec` bytes whose span starts at src to bytes [d, d + n) of acc: the table of
// fqj_pieces, a span of rec - 1 bytes and the immediate
__device__ __forceinline__ void fqj_fill(const fqj_args &a, uint64_t src, uint64_t rec, uint64_t rel, int d, int n, sk_u128 &acc)
{
    const int i = (src & FQJ_SRC_INPUT) ? 1 : 0;
    fqj_piece pc[2];
    fqj_pieces(src & ~FQJ_SRC_INPUT, rec - 1, pc);
    if (rel < pc[0].len) {
        const uint64_t p = pc[0].at + rel;
        int t = (int)min((uint64_t)n, pc[0].len - rel);
        const uint64_t room = a.s.bytes[i] - min(a.s.bytes[i], p); // == the span's rest, or more, wherever place saw this descriptor
        if ((uint64_t)t <= room) sk_put(acc, sk_to_u128(sk_load_window(a.s.text[i] + p, t)), d, t);
        rel += t;
        d += t;
        n -= t;
    }
    if (n > 0 && rel == pc[0].len) sk_put(acc, (sk_u128)pc[1].imm, d, 1);
}

__global__ void __launch_bounds__(FQJ_THREADS) sk_fq_rejects_gather_kernel(fqj_args a)
{
    __shared__ uint64_t s_off[FQJ_WIN + 1];
    __shared__ uint64_t s_src[FQJ_WIN];
    __shared__ uint64_t s_cur;
    const int t = threadIdx.x, lane = t & 63;
    if (!a.my[FQJ_H_WRITTEN]) return; // uniform
    const uint64_t total = min(a.my[FQJ_H_BYTES], a.cap), R = min(a.my[FQJ_H_RECORDS], a.s.n_bound);
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
            sk_u128 acc = 0;
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
    uint8_t *mine = static_cast<uint8_t *>(workspace);
    fqj_args a = {};
    fqs_fill(src, in, mode, &a.s);
    a.my = reinterpret_cast<uint64_t *>(mine);
    a.blk = reinterpret_cast<uint64_t *>(mine + fqj_blocks_at());
    a.tab = reinterpret_cast<uint64_t *>(mine + fqj_table_at(src->text_bytes));
    a.pairs = (flags & SK_FQ_REJECTS_PAIRS) != 0;
    a.flags = flags;
    a.n_blocks = fqj_blocks(src->text_bytes);
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
