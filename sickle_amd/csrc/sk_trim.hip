// sk_trim.hip -- device-side trimming (sk_trim_device_async): the cuts of a scan applied to the batch on the device, the
// kept records packed back to back into up to three outputs.  What reference src/trim_single.cpp:374-428 (output_single:
// substr + filter) and src/trim_paired.cpp:506-567 (output_paired: the pair routing) do on the host, minus the FASTQ text.
//
// Reduce-then-scan, four launches on one stream, no inter-workgroup waiting (workgroup dispatch order is undefined):
//   1 count   per block of SK_TRIM_BLOCK_READS reads: kept records and bytes of each output, lowest invalid cut
//   2 scan    one workgroup: block totals -> exclusive block bases (in place), the totals, the verdict of every output
//   3 place   per block again: a record's output offset, read index and source delta (input position - output position)
//   4 gather  the hot path: every workgroup owns a contiguous span of OUTPUT bytes, each lane builds aligned 16-byte
//             granules from aligned 16-byte loads funnel-shifted by v_alignbyte (any input alignment), so the stores are
//             coalesced and the balance does not depend on read length
// The workspace (caller's, device) holds the header, the block table and one 8-byte delta per record: sk_device.h.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_device_prims.h"

#define SK_TRIM_THREADS 256
#define SK_TRIM_PER_THREAD (SK_TRIM_BLOCK_READS / SK_TRIM_THREADS) // consecutive reads of one lane (even: pairs stay whole)
#ifndef SK_TRIM_GPL
#define SK_TRIM_GPL 2 // 16-byte granules per lane and chunk of the gather (a chunk = 256 * 16 * GPL output bytes)
#endif
#define SK_TRIM_CHUNK (SK_TRIM_THREADS * 16u * SK_TRIM_GPL)
#define SK_TRIM_WIN 128 // records of a chunk staged in LDS (further ones are searched in global memory)

static_assert(SK_TRIM_PER_THREAD % 2 == 0, "a lane must hold whole pairs");

struct sk_trim_dev_out {
    uint8_t *qual, *seq;
    uint64_t *offsets, *read_index;
    uint64_t byte_cap, rec_cap;
};

struct sk_trim_args {
    const uint8_t *qual, *seq;
    const uint64_t *in_off;   // offsets layout, or NULL
    const uint32_t *lengths;  // fixed stride with per-read lengths, or NULL
    uint64_t stride;
    uint32_t read_len;
    int32_t mode;
    uint64_t n_reads;
    const sk_cut_dev *cuts;
    uint64_t *ws;
    uint64_t n_blocks;
    sk_trim_dev_out out[3];
};

// which output read r goes to (-1: dropped), the pair rule of sk_pair_count_kernel (src/trim_paired.cpp:543-567)
__device__ __forceinline__ int trim_dest(int mode, bool kept, bool mate_kept, bool second)
{
    if (!kept) return -1;
    if (mode == SK_TRIM_SE) return 0;
    if (!mate_kept) return 2;
    return (mode == SK_TRIM_PE_SPLIT && second) ? 1 : 0;
}

struct trim_read {
    uint64_t start; // of the read in qual / seq
    int32_t five, three;
    int dest;
    bool bad;
};

// the SK_TRIM_PER_THREAD reads of this lane: first = an even read number
__device__ __forceinline__ void trim_load(const sk_trim_args &a, uint64_t first, trim_read (&rd)[SK_TRIM_PER_THREAD])
{
    bool kept[SK_TRIM_PER_THREAD];
#pragma unroll
    for (int i = 0; i < SK_TRIM_PER_THREAD; ++i) {
        const uint64_t r = first + i;
        sk_cut_dev c = {-1, -1};
        uint64_t start = 0, len = 0;
        if (r < a.n_reads) {
            c = a.cuts[r];
            if (a.in_off) {
                start = a.in_off[r];
                len = a.in_off[r + 1] - start;
            } else {
                start = r * a.stride;
                len = a.lengths ? a.lengths[r] : a.read_len;
            }
        }
        kept[i] = c.three >= 0; // src/trim_single.cpp:368, src/trim_paired.cpp:500,502
        rd[i].start = start;
        rd[i].five = c.five;
        rd[i].three = c.three;
        rd[i].bad = kept[i] && (c.five < 0 || c.five > c.three || (uint64_t)c.three > len);
    }
#pragma unroll
    for (int i = 0; i < SK_TRIM_PER_THREAD; ++i) rd[i].dest = trim_dest(a.mode, kept[i], kept[i ^ 1], i & 1);
}

// bytes of a kept record (0 for an invalid cut: the counts are then not used)
__device__ __forceinline__ uint64_t trim_bytes(const trim_read &r) { return r.bad ? 0 : (uint64_t)(r.three - r.five); }

// ------------------------------------------------------------------------------------------
// 1 count
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_TRIM_THREADS) sk_trim_count_kernel(sk_trim_args a)
{
    __shared__ uint64_t lds[4 * 6];
    __shared__ unsigned long long bad_min;
    if (threadIdx.x == 0) bad_min = ~0ull; // ordered before the atomics by sk_block_scan's barriers
    const uint64_t first = (uint64_t)blockIdx.x * SK_TRIM_BLOCK_READS + threadIdx.x * SK_TRIM_PER_THREAD;
    trim_read rd[SK_TRIM_PER_THREAD];
    trim_load(a, first, rd);
    uint64_t v[6] = {0, 0, 0, 0, 0, 0}, tot[6];
    uint64_t bad = ~0ull;
#pragma unroll
    for (int i = 0; i < SK_TRIM_PER_THREAD; ++i) {
        if (rd[i].bad && bad == ~0ull) bad = first + i;
#pragma unroll
        for (int o = 0; o < 3; ++o)
            if (rd[i].dest == o) {
                v[o] += 1;
                v[3 + o] += trim_bytes(rd[i]);
            }
    }
    sk_block_scan<6, SK_TRIM_THREADS>(v, tot, lds);
    if (bad != ~0ull) atomicMin(&bad_min, (unsigned long long)bad);
    __syncthreads();
    if (threadIdx.x < 7) {
        uint64_t x = bad_min; // word 6
#pragma unroll
        for (int i = 0; i < 6; ++i) x = threadIdx.x == i ? tot[i] : x; // no runtime index into tot[]: it stays in registers
        a.ws[SK_TRIM_HDR_WORDS + blockIdx.x * SK_TRIM_BLOCK_WORDS + threadIdx.x] = x;
    }
}

// ------------------------------------------------------------------------------------------
// 2 scan of the block totals (one workgroup), header and verdicts
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_TRIM_THREADS) sk_trim_scan_kernel(sk_trim_args a)
{
    __shared__ uint64_t lds[4 * 6];
    __shared__ unsigned long long bad_min;
    if (threadIdx.x == 0) bad_min = ~0ull;
    __syncthreads();
    uint64_t run[6] = {0, 0, 0, 0, 0, 0};
    uint64_t bad = ~0ull;
    uint64_t *blk = a.ws + SK_TRIM_HDR_WORDS;
    for (uint64_t b0 = 0; b0 < a.n_blocks; b0 += SK_TRIM_THREADS) {
        const uint64_t b = b0 + threadIdx.x;
        uint64_t v[6], tot[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i] = b < a.n_blocks ? blk[b * SK_TRIM_BLOCK_WORDS + i] : 0;
        if (b < a.n_blocks) bad = min(bad, blk[b * SK_TRIM_BLOCK_WORDS + 6]);
        sk_block_scan<6, SK_TRIM_THREADS>(v, tot, lds);
        if (b < a.n_blocks)
#pragma unroll
            for (int i = 0; i < 6; ++i) blk[b * SK_TRIM_BLOCK_WORDS + i] = run[i] + v[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) run[i] += tot[i];
    }
    if (bad != ~0ull) atomicMin(&bad_min, (unsigned long long)bad);
    __syncthreads();
    if (threadIdx.x < 3) {
        const int o = threadIdx.x;
        const sk_trim_dev_out &out = a.out[o];
        const bool used = o == 0 || (a.mode == SK_TRIM_PE_SPLIT && o == 1) || (a.mode != SK_TRIM_SE && o == 2);
        const bool produced = used && out.offsets;
        const bool data = out.qual || out.seq;
        const uint64_t recs = o == 0 ? run[0] : o == 1 ? run[1] : run[2], bytes = o == 0 ? run[3] : o == 1 ? run[4] : run[5];
        const bool fit = produced && bad_min == ~0ull && recs <= out.rec_cap && (!data || bytes <= out.byte_cap);
        a.ws[SK_TRIM_H_RECORDS + o] = recs;
        a.ws[SK_TRIM_H_BYTES + o] = bytes;
        a.ws[SK_TRIM_H_PRODUCED + o] = produced;
        a.ws[SK_TRIM_H_FIT + o] = fit;
        if (fit) out.offsets[recs] = bytes; // offsets[records]: also offsets[0] = 0 of an empty output
        if (o == 0) a.ws[SK_TRIM_H_BAD] = bad_min;
    }
}

// ------------------------------------------------------------------------------------------
// 3 place: offsets[], read_index[] and the source deltas of every record of a fitting output
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SK_TRIM_THREADS) sk_trim_place_kernel(sk_trim_args a)
{
    __shared__ uint64_t lds[4 * 6];
    const uint64_t *hdr = a.ws;
    const bool fit[3] = {hdr[SK_TRIM_H_FIT] != 0, hdr[SK_TRIM_H_FIT + 1] != 0, hdr[SK_TRIM_H_FIT + 2] != 0};
    if (!fit[0] && !fit[1] && !fit[2]) return; // uniform
    const uint64_t first = (uint64_t)blockIdx.x * SK_TRIM_BLOCK_READS + threadIdx.x * SK_TRIM_PER_THREAD;
    trim_read rd[SK_TRIM_PER_THREAD];
    trim_load(a, first, rd);
    uint64_t v[6] = {0, 0, 0, 0, 0, 0}, tot[6];
#pragma unroll
    for (int i = 0; i < SK_TRIM_PER_THREAD; ++i)
#pragma unroll
        for (int o = 0; o < 3; ++o)
            if (rd[i].dest == o) {
                v[o] += 1;
                v[3 + o] += trim_bytes(rd[i]);
            }
    sk_block_scan<6, SK_TRIM_THREADS>(v, tot, lds);
    const uint64_t *blk = a.ws + SK_TRIM_HDR_WORDS + blockIdx.x * SK_TRIM_BLOCK_WORDS;
#pragma unroll
    for (int i = 0; i < 6; ++i) v[i] += blk[i];
    uint64_t *delta = a.ws + SK_TRIM_HDR_WORDS + a.n_blocks * SK_TRIM_BLOCK_WORDS;
    const uint64_t dbase[3] = {0, hdr[SK_TRIM_H_RECORDS], hdr[SK_TRIM_H_RECORDS] + hdr[SK_TRIM_H_RECORDS + 1]};
#pragma unroll
    for (int i = 0; i < SK_TRIM_PER_THREAD; ++i)
#pragma unroll
        for (int o = 0; o < 3; ++o)
            if (rd[i].dest == o) {
                const uint64_t j = v[o], b = v[3 + o];
                v[o] += 1;
                v[3 + o] += trim_bytes(rd[i]);
                if (!fit[o]) continue;
                a.out[o].offsets[j] = b;
                if (a.out[o].read_index) a.out[o].read_index[j] = first + i;
                delta[dbase[o] + j] = rd[i].start + (uint64_t)rd[i].five - b; // input byte of output byte p: p + delta
            }
}

// ------------------------------------------------------------------------------------------
// 4 gather
// ------------------------------------------------------------------------------------------
// bytes [0, n) of v to bytes [d, d + n) of acc (d + n <= 16)
__device__ __forceinline__ void place(sk_u128 &acc, sk_u4 v, int d, int n)
{
    const sk_u128 x = sk_to_u128(v);
    const sk_u128 m = n >= 16 ? ~(sk_u128)0 : (((sk_u128)1 << (8 * n)) - 1);
    acc |= (x & m) << (8 * d);
}

__device__ __forceinline__ void store_granule(uint8_t *dst, uint64_t g, sk_u4 v, int n)
{
    if (n == 16) {
        __builtin_nontemporal_store(v, reinterpret_cast<sk_u4 *>(dst + g));
    } else {
        const sk_u128 x = sk_to_u128(v);
        for (int i = 0; i < n; ++i) dst[g + i] = (uint8_t)(x >> (8 * i));
    }
}

__global__ void __launch_bounds__(SK_TRIM_THREADS) sk_trim_gather_kernel(sk_trim_args a)
{
    __shared__ uint64_t s_off[SK_TRIM_WIN + 1];
    __shared__ uint64_t s_delta[SK_TRIM_WIN];
    __shared__ uint64_t s_cur;
    const uint64_t *hdr = a.ws;
    const int t = threadIdx.x, lane = t & 63;
    const uint64_t *delta_all = a.ws + SK_TRIM_HDR_WORDS + a.n_blocks * SK_TRIM_BLOCK_WORDS;
    uint64_t dbase = 0;
    for (int o = 0; o < 3; ++o) {
        const uint64_t R = hdr[SK_TRIM_H_RECORDS + o], total = hdr[SK_TRIM_H_BYTES + o];
        const uint64_t *delta = delta_all + dbase;
        dbase += R;
        const sk_trim_dev_out out = a.out[o];
        if (!hdr[SK_TRIM_H_FIT + o] || (!out.qual && !out.seq) || total == 0) continue; // uniform
        const uint64_t n_chunks = (total + SK_TRIM_CHUNK - 1) / SK_TRIM_CHUNK;
        const uint64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
        const uint64_t c0 = (uint64_t)blockIdx.x * per, c1 = min(c0 + per, n_chunks);
        if (c0 >= c1) continue;
        const uint64_t *off = out.offsets; // R + 1 entries, off[R] == total
        const uint8_t *qual = out.qual ? a.qual : nullptr, *seq = out.seq ? a.seq : nullptr;
        // the record holding the span's first byte: a 64-ary search by wave 0 (the last k < R with off[k] <= x)
        if (t < 64) {
            const uint64_t x = c0 * SK_TRIM_CHUNK;
            uint64_t lo = 0, hi = R;
            while (hi - lo > 1) {
                const uint64_t step = (hi - lo + 63) / 64, p = lo + lane * step;
                const uint64_t m = __builtin_amdgcn_ballot_w64(p < hi && off[p] <= x); // lane 0's probe always holds
                lo += (uint64_t)(63 - __builtin_clzll(m)) * step;
                hi = min(hi, lo + step);
            }
            if (t == 0) s_cur = lo;
        }
        __syncthreads();
        uint64_t cur = s_cur;
        for (uint64_t c = c0; c < c1; ++c) {
            // stage the chunk's first records: off[cur .. cur + WIN] and their deltas
            if (t <= SK_TRIM_WIN) s_off[t] = cur + t <= R ? off[cur + t] : ~0ull;
            if (t < SK_TRIM_WIN && cur + t < R) s_delta[t] = delta[cur + t];
            __syncthreads();
            const uint64_t win_end = s_off[SK_TRIM_WIN];
            uint64_t k_last = cur;
#pragma unroll
            for (int u = 0; u < SK_TRIM_GPL; ++u) {
                const uint64_t g = c * SK_TRIM_CHUNK + (uint64_t)u * (SK_TRIM_THREADS * 16) + 16u * t;
                if (g >= total) break;
                // the record holding byte g: in the staged window, or beyond it in global memory
                uint64_t k;
                if (g < win_end) {
                    int lo = 0, hi = SK_TRIM_WIN; // s_off[lo] <= g < s_off[hi]
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (s_off[mid] <= g) lo = mid; else hi = mid;
                    }
                    k = cur + lo;
                } else {
                    uint64_t lo = cur + SK_TRIM_WIN, hi = R; // off[lo] <= g < off[hi]
                    while (hi - lo > 1) {
                        const uint64_t mid = lo + ((hi - lo) >> 1);
                        if (off[mid] <= g) lo = mid; else hi = mid;
                    }
                    k = lo;
                }
                k_last = k;
                const uint64_t end = min(g + 16, total);
                sk_u128 aq = 0, as = 0;
                sk_u4 vq = {0, 0, 0, 0}, vs = {0, 0, 0, 0};
                uint64_t pos = g;
                bool whole = false;
                while (pos < end) {
                    const uint64_t i = k - cur;
                    const uint64_t e = i < SK_TRIM_WIN ? s_off[i + 1] : off[k + 1];
                    if (e <= pos) { // the record ended (or is empty)
                        ++k;
                        continue;
                    }
                    const uint64_t pe = min(e, end), src = pos + (i < SK_TRIM_WIN ? s_delta[i] : delta[k]);
                    const int d = (int)(pos - g), n = (int)(pe - pos);
                    if (n == 16) { // the granule lies inside one record: the fast path
                        if (qual) vq = sk_load_window(qual + src, 16);
                        if (seq) vs = sk_load_window(seq + src, 16);
                        whole = true;
                    } else {
                        if (qual) place(aq, sk_load_window(qual + src, n), d, n);
                        if (seq) place(as, sk_load_window(seq + src, n), d, n);
                    }
                    pos = pe;
                }
                if (!whole) {
                    vq = sk_from_u128(aq);
                    vs = sk_from_u128(as);
                }
                const int n = (int)(end - g);
                if (qual) store_granule(out.qual, g, vq, n);
                if (seq) store_granule(out.seq, g, vs, n);
            }
            // the next chunk starts at or after the record of the last lane's last granule
            if (t == SK_TRIM_THREADS - 1) s_cur = k_last;
            __syncthreads();
            cur = s_cur;
        }
        __syncthreads(); // s_cur / s_off are reused by the next output
    }
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_trim(const sk_batch *b, const sk_cut_dev *cuts, int mode,
                                                                           const sk_trim_output *out, void *workspace,
                                                                           int cu_count, hipStream_t stream)
{
    sk_trim_args a;
    a.qual = b->qual;
    a.seq = b->seq;
    a.in_off = b->offsets;
    a.lengths = b->offsets ? nullptr : b->lengths;
    a.stride = b->stride;
    a.read_len = b->read_len;
    a.mode = mode;
    a.n_reads = b->n_reads;
    a.cuts = cuts;
    a.ws = static_cast<uint64_t *>(workspace);
    a.n_blocks = (b->n_reads + SK_TRIM_BLOCK_READS - 1) / SK_TRIM_BLOCK_READS;
    for (int o = 0; o < 3; ++o)
        a.out[o] = {out[o].qual, out[o].seq, out[o].offsets, out[o].read_index, out[o].byte_capacity, out[o].record_capacity};
    if (mode == SK_TRIM_SE) a.out[1] = a.out[2] = {};
    if (mode == SK_TRIM_PE_INTERLEAVED) a.out[1] = {};
    if (a.n_blocks) hipLaunchKernelGGL(sk_trim_count_kernel, dim3((unsigned)a.n_blocks), dim3(SK_TRIM_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_trim_scan_kernel, dim3(1), dim3(SK_TRIM_THREADS), 0, stream, a);
    if (a.n_blocks) hipLaunchKernelGGL(sk_trim_place_kernel, dim3((unsigned)a.n_blocks), dim3(SK_TRIM_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_trim_gather_kernel, dim3((unsigned)cu_count * SK_TRIM_GATHER_WG_PER_CU), dim3(SK_TRIM_THREADS), 0, stream, a);
    return hipGetLastError();
}
