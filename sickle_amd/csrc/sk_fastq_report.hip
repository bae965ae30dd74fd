// sk_fastq_report.hip -- the trim report over a finished text call's workspace (sk_trim_fastq_report_device_async): the
// rule of sk_fastq_report.h summed on the device into a sk_fastq_report and the caller's histograms.
//
// Launches on the text call's stream, behind its emission; no inter-workgroup waiting, and the result does not depend on
// the order of workgroups: every global write is an integer atomic add (or max), but for the reset kernel's stores.
//   0 reset  (SK_FQ_REPORT_RESET only) zeroes the report and the given arrays
//   1 reads  per block of SK_FQ_BLOCK_READS reads, as the emission's count kernel: a lane owns FQP_PER_THREAD consecutive
//            reads (whole pairs), loads their offsets and cuts, the scalar words are reduced in the wave and then in the
//            workgroup, the length histograms are 32-bit LDS counters (2 048 reads a block: no overflow); one 64-bit
//            global atomic per non-zero word.  Block 0 counts the call (calls / calls_failed).
//   2 qual   only with a position array: a workgroup takes FQP_CHUNK_BYTES of the packed qual in steps of 256 aligned
//            16-byte loads, finds its first read by a 64-ary search in offsets, stages the next FQP_WIN reads' bounds and
//            cuts in LDS per step (as the gathers' FQ_WIN), walks each lane's granule against them and adds
//            (1 << 32 | byte) to the 64-bit LDS word of the byte's position bin: the count in the high half, the sum in the
//            low half, which cannot overflow (sk_fastq_report.h).  The last bin, which takes every position from
//            pos_bins - 1 on, is summed in registers and added once per lane.  Non-zero halves go out as global atomics.
// Every workgroup takes the call's validity from the header (fqs_valid) and leaves at once when the call does not add.
// Blocks at or beyond SK_FQ_H_NREAL load nothing; no offset or cut at or beyond the count is read but offsets[NREAL],
// and no granule of the packed qual without a byte below offsets[NREAL].  A source that names the wrong layout gives wrong
// numbers, no load outside the workspace: the bounds are the source view's (sk_fastq_source.h).
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_fastq_order.h"
#include "sk_fastq_report.h"
#include "sk_fastq_source.h"

namespace {

typedef unsigned fqp_u4 __attribute__((ext_vector_type(4)));
typedef unsigned long long fqp_ull;

#define FQP_THREADS 256
#define FQP_PER_THREAD (SK_FQ_BLOCK_READS / FQP_THREADS) // consecutive reads of one lane (even: pairs stay whole)
#define FQP_STEP (FQP_THREADS * 16u)                     // packed bytes of one step of a quality workgroup
#define FQP_WIN 128 // reads of a step staged in LDS (further ones are searched in global memory)

static_assert(FQP_PER_THREAD % 2 == 0, "a lane must hold whole pairs");
static_assert(FQP_CHUNK_BYTES % FQP_STEP == 0, "a chunk is whole steps");
static_assert(2 * 4 * SK_FQ_REPORT_MAX_LEN_BINS + 2 * 8 * SK_FQ_REPORT_MAX_POS_BINS <= 64 * 1024, "the LDS tables fit beside each other");
static_assert(SK_FQ_REPORT_MAX_POS_BINS % 32 == 0, "the largest table is whole groups of fqp_slot");

struct fqp_args {
    fqs_view s;    // the call behind; no mode: the report does not compare it
    uint64_t *rep; // sk_fastq_report as FQP_WORDS words
    uint64_t *len_in, *len_out;
    uint64_t *qsum_in, *qcnt_in, *qsum_out, *qcnt_out;
    uint32_t len_bins, pos_bins;
};

__device__ __forceinline__ void fqp_add(uint64_t *p, uint64_t v)
{
    if (v) atomicAdd(reinterpret_cast<fqp_ull *>(p), (fqp_ull)v);
}

// ------------------------------------------------------------------------------------------
// 0 reset
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQP_THREADS) sk_fq_report_reset_kernel(fqp_args a)
{
    const uint32_t i = blockIdx.x * FQP_THREADS + threadIdx.x;
    if (i < FQP_WORDS) a.rep[i] = 0;
    if (i < a.len_bins) {
        if (a.len_in) a.len_in[i] = 0;
        if (a.len_out) a.len_out[i] = 0;
    }
    if (i < a.pos_bins) {
        if (a.qsum_in) a.qsum_in[i] = 0;
        if (a.qcnt_in) a.qcnt_in[i] = 0;
        if (a.qsum_out) a.qsum_out[i] = 0;
        if (a.qcnt_out) a.qcnt_out[i] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// 1 per read
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQP_THREADS) sk_fq_report_reads_kernel(fqp_args a)
{
    extern __shared__ uint32_t s_len[]; // len_in[len_bins], len_out[len_bins] (only with a length array)
    __shared__ uint64_t s_red[FQP_THREADS / 64][FQP_WORDS];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const bool valid = fqs_valid(a.s); // uniform
    if (blockIdx.x == 0 && t == 0) atomicAdd(reinterpret_cast<fqp_ull *>(a.rep + (valid ? FQP_W_CALLS : FQP_W_CALLS_FAILED)), 1ull);
    if (!valid) return;
    const uint64_t n_real = fqs_reads(a.s);
    if ((uint64_t)blockIdx.x * SK_FQ_BLOCK_READS >= n_real) return; // uniform: nothing at or beyond the count is loaded
    const int64_t mode = (int64_t)a.s.hdr[SK_FQ_H_MODE];
    const bool hist = a.len_in || a.len_out;
    if (hist) {
        for (uint32_t i = t; i < 2 * a.len_bins; i += FQP_THREADS) s_len[i] = 0;
        __syncthreads();
    }
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + (uint64_t)t * FQP_PER_THREAD;
    uint64_t w[FQP_WORDS];
#pragma unroll
    for (int k = 0; k < FQP_WORDS; ++k) w[k] = 0;
    uint64_t max_in = 0, max_out = 0;
    if (first < n_real) {
        uint64_t b = a.s.offsets[first];
        int32_t three_even = -1;
#pragma unroll
        for (int j = 0; j < FQP_PER_THREAD; ++j) {
            const uint64_t r = first + j;
            if (r < n_real) {
                const uint64_t e = a.s.offsets[r + 1], len = e - b;
                const sk_cut_dev c = a.s.cuts[r];
                fqp_add_read(len, c.five, c.three, w, &max_in, &max_out);
                if (hist) {
                    atomicAdd(&s_len[fqp_bin(len, a.len_bins)], 1u);
                    if (fqp_kept(c.three)) atomicAdd(&s_len[a.len_bins + fqp_bin((uint64_t)(c.three - c.five), a.len_bins)], 1u);
                }
                if ((j & 1) == 0) three_even = c.three;
                else if (fqp_pair_at(mode, r - 1, n_real)) fqp_add_pair(three_even, c.three, w);
                b = e;
            }
        }
    }
    w[FQP_W_MAX_LEN_IN] = max_in;
    w[FQP_W_MAX_LEN_OUT] = max_out;
    // the wave, then the workgroup: sums, and the two maxima
#pragma unroll
    for (int k = 0; k < FQP_WORDS; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t o = __shfl_xor(w[k], d);
            w[k] = k < FQP_SUM_WORDS ? w[k] + o : max(w[k], o);
        }
        if (lane == 0) s_red[wv][k] = w[k];
    }
    __syncthreads();
    if (t < FQP_WORDS && t != FQP_W_CALLS && t != FQP_W_CALLS_FAILED) {
        uint64_t v = s_red[0][t];
#pragma unroll
        for (int ww = 1; ww < FQP_THREADS / 64; ++ww) v = t < FQP_SUM_WORDS ? v + s_red[ww][t] : max(v, s_red[ww][t]);
        if (v) {
            if (t < FQP_SUM_WORDS) atomicAdd(reinterpret_cast<fqp_ull *>(a.rep + t), (fqp_ull)v);
            else atomicMax(reinterpret_cast<fqp_ull *>(a.rep + t), (fqp_ull)v);
        }
    }
    if (hist) { // (the LDS atomics are done: the barrier above)
        for (uint32_t i = t; i < a.len_bins; i += FQP_THREADS) {
            if (a.len_in) fqp_add(a.len_in + i, s_len[i]);
            if (a.len_out) fqp_add(a.len_out + i, s_len[a.len_bins + i]);
        }
    }
}

// ------------------------------------------------------------------------------------------
// 2 the quality pass
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQP_THREADS) sk_fq_report_qual_kernel(fqp_args a)
{
    extern __shared__ uint64_t s_pos[]; // in[PS], out[PS], PS = fqp_slots(pos_bins): count << 32 | sum of bin p at fqp_slot(p)
    __shared__ uint64_t s_off[FQP_WIN + 1];
    __shared__ sk_cut_dev s_cut[FQP_WIN];
    __shared__ uint64_t s_cur;
    const int t = threadIdx.x, lane = t & 63;
    if (!fqs_valid(a.s)) return; // uniform
    const uint64_t R = fqs_reads(a.s);
    if (R == 0) return;
    // == SK_FQ_H_PACKED: the reads behind the count are empty.  (Never beyond the section, and the walks below never leave
    // offsets[0 .. R]: a source that names the wrong layout gives wrong numbers, not loads outside the workspace.)
    const uint64_t total = min(a.s.offsets[R], a.s.q_bound);
    const uint64_t c0 = (uint64_t)blockIdx.x * FQP_CHUNK_BYTES;
    if (c0 >= total) return; // uniform
    const uint64_t c1 = min(c0 + FQP_CHUNK_BYTES, total);
    const uint32_t PB = a.pos_bins, last = PB - 1, PS = fqp_slots(PB);
    uint64_t *s_in = s_pos, *s_out = s_pos + PS;
    for (uint32_t i = t; i < 2 * PS; i += FQP_THREADS) s_pos[i] = 0;
    auto off = [&](uint64_t k) { return a.s.offsets[k]; }; // k <= R
    // the read holding the chunk's first byte: a 64-ary search by wave 0 (the last k < R with off(k) <= c0)
    if (t < 64) {
        uint64_t lo = 0, hi = R;
        while (hi - lo > 1) {
            const uint64_t step = (hi - lo + 63) / 64, p = lo + lane * step;
            const uint64_t mk = __builtin_amdgcn_ballot_w64(p < hi && off(p) <= c0); // lane 0's probe always holds
            lo += (uint64_t)(63 - __builtin_clzll(mk)) * step;
            hi = min(hi, lo + step);
        }
        if (t == 0) s_cur = lo;
    }
    __syncthreads();
    uint64_t cur = s_cur;
    uint64_t tail_in = 0, tail_out = 0; // the last bin, count << 32 | sum, over the lane's granules of the whole chunk
    for (uint64_t s0 = c0; s0 < c1; s0 += FQP_STEP) {
        if (t <= FQP_WIN) s_off[t] = cur + t <= R ? off(cur + t) : ~0ull;
        if (t < FQP_WIN && cur + t < R) s_cut[t] = a.s.cuts[cur + t];
        __syncthreads();
        const uint64_t g = s0 + 16u * t;
        uint64_t k = cur;
        if (g < c1) {
            if (g < s_off[FQP_WIN]) {
                int lo = 0, hi = FQP_WIN; // s_off[lo] <= g < s_off[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_off[mid] <= g) lo = mid; else hi = mid;
                }
                k = cur + lo;
            } else if (cur + FQP_WIN < R) {
                uint64_t lo = cur + FQP_WIN, hi = R; // off(lo) <= g < off(hi)
                while (hi - lo > 1) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (off(mid) <= g) lo = mid; else hi = mid;
                }
                k = lo;
            } else {
                k = R - 1;
            }
            const fqp_u4 v = __builtin_nontemporal_load(reinterpret_cast<const fqp_u4 *>(a.s.pq + g));
            const uint32_t word[4] = {v.x, v.y, v.z, v.w};
            const int n = (int)min((uint64_t)16, c1 - g);
            // read k's bounds and cut; the reads that end at or before g (empty ones) are stepped over
            uint64_t b, e;
            sk_cut_dev c;
            auto load = [&]() {
                const uint64_t i = k - cur;
                b = i < FQP_WIN ? s_off[i] : off(k);
                e = i < FQP_WIN ? s_off[i + 1] : off(k + 1);
                c = i < FQP_WIN ? s_cut[i] : a.s.cuts[k];
            };
            load();
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < n) {
                    const uint64_t at = g + i;
                    while (at >= e && k + 1 < R) { // at < total = off(R): the bound on k never ends the walk of a batch
                        ++k;
                        load();
                    }
                    const uint32_t q = (word[i >> 2] >> (8 * (i & 3))) & 0xffu;
                    const uint64_t p = at - b, x = fqp_qword(q);
                    if (p >= last) tail_in += x;
                    else atomicAdd(reinterpret_cast<fqp_ull *>(s_in + fqp_slot((uint32_t)p)), (fqp_ull)x);
                    if (fqp_out_byte(p, c.five, c.three)) {
                        const uint64_t po = p - (uint64_t)c.five;
                        if (po >= last) tail_out += x;
                        else atomicAdd(reinterpret_cast<fqp_ull *>(s_out + fqp_slot((uint32_t)po)), (fqp_ull)x);
                    }
                }
            }
        }
        // the next step starts at or after the read of the last lane's last byte
        if (t == FQP_THREADS - 1) s_cur = k;
        __syncthreads();
        cur = s_cur;
    }
    if (tail_in) atomicAdd(reinterpret_cast<fqp_ull *>(s_in + fqp_slot(last)), (fqp_ull)tail_in);
    if (tail_out) atomicAdd(reinterpret_cast<fqp_ull *>(s_out + fqp_slot(last)), (fqp_ull)tail_out);
    __syncthreads();
    for (uint32_t i = t; i < PB; i += FQP_THREADS) {
        const uint64_t x = s_in[fqp_slot(i)], y = s_out[fqp_slot(i)];
        if (a.qsum_in) fqp_add(a.qsum_in + i, x & 0xffffffffull);
        if (a.qcnt_in) fqp_add(a.qcnt_in + i, x >> 32);
        if (a.qsum_out) fqp_add(a.qsum_out + i, y & 0xffffffffull);
        if (a.qcnt_out) fqp_add(a.qcnt_out + i, y >> 32);
    }
}

} // namespace

// src and hists have passed the checks of sk_trim_fastq_report_device_async (sk_capi.hip)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_report(const sk_fastq_report_source *src,
                                                                                   sk_fastq_report *report_dev,
                                                                                   const sk_fastq_report_hists *hists, int flags,
                                                                                   hipStream_t stream)
{
    fqp_args a = {};
    fqs_fill(src, nullptr, FQS_NO_MODE, &a.s);
    a.rep = reinterpret_cast<uint64_t *>(report_dev);
    if (hists) {
        const bool has_len = hists->len_in || hists->len_out;
        const bool has_pos = hists->qsum_in || hists->qcnt_in || hists->qsum_out || hists->qcnt_out;
        a.len_in = hists->len_in;
        a.len_out = hists->len_out;
        a.len_bins = has_len ? (uint32_t)hists->len_bins : 0;
        a.qsum_in = hists->qsum_in;
        a.qcnt_in = hists->qcnt_in;
        a.qsum_out = hists->qsum_out;
        a.qcnt_out = hists->qcnt_out;
        a.pos_bins = has_pos ? (uint32_t)hists->pos_bins : 0;
    }
    const dim3 threads(FQP_THREADS);
    if (flags & SK_FQ_REPORT_RESET) {
        uint32_t words = FQP_WORDS;
        if (a.len_bins > words) words = a.len_bins;
        if (a.pos_bins > words) words = a.pos_bins;
        hipLaunchKernelGGL(sk_fq_report_reset_kernel, dim3((words + FQP_THREADS - 1) / FQP_THREADS), threads, 0, stream, a);
    }
    const uint64_t n_blocks = (a.s.n_bound + SK_FQ_BLOCK_READS - 1) / SK_FQ_BLOCK_READS;
    hipLaunchKernelGGL(sk_fq_report_reads_kernel, dim3((unsigned)n_blocks), threads, 2 * 4 * a.len_bins, stream, a);
    if (a.pos_bins) {
        // the packed qual is at most half the text
        const uint64_t n_chunks = (src->text_bytes / 2 + FQP_CHUNK_BYTES - 1) / FQP_CHUNK_BYTES;
        if (n_chunks)
            hipLaunchKernelGGL(sk_fq_report_qual_kernel, dim3((unsigned)n_chunks), threads, 2 * 8 * fqp_slots(a.pos_bins), stream, a);
    }
    return hipGetLastError();
}
