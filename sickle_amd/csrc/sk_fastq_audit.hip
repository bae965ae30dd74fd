// sk_fastq_audit.hip -- the audit over a finished text call's workspace and texts (sk_trim_fastq_audit_device_async): the
// rule of sk_fastq_audit.h summed on the device into a sk_fastq_audit and the caller's histogram.
//
// Launches on the text call's stream, behind its emission; no inter-workgroup waiting, and the result does not depend on
// the order of workgroups: every global write of the two passes is an integer atomic add, min or max.
//   0 reset  (SK_FQ_AUDIT_RESET only) the struct's start values and a zeroed histogram
//   1 names  (pair modes with texts only) per block of SK_FQ_BLOCK_READS reads, the grid of the report's reads kernel: a
//            lane owns FQA_PER_THREAD / 2 whole pairs, one in each turn of the workgroup over 2 * FQA_THREADS neighbouring
//            reads, finds each mate's descriptor as the text call's kernels do
//            (split texts have their slots one behind the other), and walks the two name lines side by side, 8 bytes a
//            step (fqa_pair).  Counts are reduced in the wave and the workgroup; one global atomic per non-zero word.
//            The call's lowest mismatching pair goes by atomicMin, its pair count by atomicAdd, into two reserved words.
//   2 qual   a workgroup takes FQA_CHUNK_BYTES of the packed qual in steps of 256 aligned 16-byte loads: the minimum and
//            the maximum in packed 16-bit halves, and, with a histogram, runs of equal bytes of a granule added once to one
//            of FQA_TABLES private LDS tables.
//   3 fold   one lane: counts the call (calls / calls_failed) and folds the two reserved words into first_mismatch and
//            pairs (fqa_fold).  It runs behind this call's passes and in front of the next call's, by the stream's order.
// Every workgroup takes the call's validity from the header (fqs_valid) and leaves at once when the call does not add.
// Blocks at or beyond SK_FQ_H_NREAL load nothing.  A source that names the wrong layout or the wrong texts gives wrong
// numbers, no load outside the workspace and the texts, and no unbounded walk: the bounds and the name line's clamps are
// the source view's (sk_fastq_source.h).
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_fastq_audit.h"
#include "sk_fastq_order.h"
#include "sk_fastq_report.h"
#include "sk_fastq_source.h"

namespace {

typedef unsigned fqa_u4 __attribute__((ext_vector_type(4)));
typedef unsigned short fqa_h2 __attribute__((ext_vector_type(2)));
typedef unsigned long long fqa_ull;

#define FQA_THREADS 256
#define FQA_PER_THREAD (SK_FQ_BLOCK_READS / FQA_THREADS) // reads of one lane (even: pairs stay whole)
#define FQA_STEP (FQA_THREADS * 16u)                     // packed bytes of one step of a quality workgroup

static_assert(FQA_PER_THREAD % 2 == 0, "a lane must hold whole pairs");
static_assert(FQA_CHUNK_BYTES % FQA_STEP == 0, "a chunk is whole steps");
static_assert(FQA_THREADS % FQA_TABLES == 0, "every table has the same number of lanes");

struct fqa_args {
    fqs_view s;     // the call behind
    uint64_t *aud;  // sk_fastq_audit as FQA_WORDS words
    uint64_t *hist; // [256] or NULL
};

// ------------------------------------------------------------------------------------------
// 0 reset
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQA_THREADS) sk_fq_audit_reset_kernel(fqa_args a)
{
    const uint32_t i = threadIdx.x;
    if (i < FQA_WORDS) a.aud[i] = fqa_reset_word(i);
    if (a.hist) a.hist[i] = 0; // 256 lanes, 256 bins
}

// ------------------------------------------------------------------------------------------
// 1 the names pass
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQA_THREADS) sk_fq_audit_names_kernel(fqa_args a)
{
    __shared__ uint64_t s_red[FQA_THREADS / 64][4];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (!fqs_valid(a.s)) return; // uniform
    const uint64_t n_real = fqs_reads(a.s);
    if ((uint64_t)blockIdx.x * SK_FQ_BLOCK_READS >= n_real) return; // uniform: nothing at or beyond the count is loaded
    // the lanes of a turn take neighbouring pairs, so that their descriptors and their name lines are neighbours too
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + 2u * (uint64_t)t;
    uint64_t pairs = 0, mism = 0, swapped = 0, low = FQA_NONE;
#pragma unroll 1
    for (int j = 0; j < FQA_PER_THREAD / 2; ++j) {
        const uint64_t r = first + (uint64_t)j * (2u * FQA_THREADS);
        if (!fqp_pair_at(a.s.mode, r, n_real)) break;
        const uint8_t *n1 = nullptr, *n2 = nullptr;
        uint64_t len1 = 0, len2 = 0;
        if (!fqs_name_line(a.s, r, n1, len1) || !fqs_name_line(a.s, r + 1, n2, len2)) break;
        const uint32_t f = fqa_pair(n1, len1, n2, len2);
        ++pairs;
        if (f & FQA_MISMATCH) {
            ++mism;
            low = min(low, r >> 1);
        }
        if (f & FQA_SWAPPED) ++swapped;
    }
    // the wave, then the workgroup: three sums and a minimum
    uint64_t w[4] = {pairs, mism, swapped, low};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t o = __shfl_xor(w[k], d);
            w[k] = k < 3 ? w[k] + o : min(w[k], o);
        }
        if (lane == 0) s_red[wv][k] = w[k];
    }
    __syncthreads();
    if (t < 4) {
        uint64_t v = s_red[0][t];
#pragma unroll
        for (int ww = 1; ww < FQA_THREADS / 64; ++ww) v = t < 3 ? v + s_red[ww][t] : min(v, s_red[ww][t]);
        if (t == 0 && v) atomicAdd(reinterpret_cast<fqa_ull *>(a.aud + FQA_W_CALL_PAIRS), (fqa_ull)v);
        if (t == 1 && v) atomicAdd(reinterpret_cast<fqa_ull *>(a.aud + FQA_W_NAME_MISMATCH), (fqa_ull)v);
        if (t == 2 && v) atomicAdd(reinterpret_cast<fqa_ull *>(a.aud + FQA_W_TAGS_SWAPPED), (fqa_ull)v);
        if (t == 3 && v != FQA_NONE) atomicMin(reinterpret_cast<fqa_ull *>(a.aud + FQA_W_CALL_FIRST), (fqa_ull)v);
    }
}

// ------------------------------------------------------------------------------------------
// 2 the quality pass
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ fqa_h2 fqa_halves(uint32_t x)
{
    return __builtin_bit_cast(fqa_h2, x);
}

template <bool HIST>
__global__ void __launch_bounds__(FQA_THREADS) sk_fq_audit_qual_kernel(fqa_args a)
{
    __shared__ uint32_t s_tab[HIST ? FQA_TABLES * FQA_TABLE_STRIDE : 1];
    __shared__ uint32_t s_lo[FQA_THREADS / 64], s_hi[FQA_THREADS / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (!fqs_valid(a.s)) return; // uniform
    const uint64_t R = fqs_reads(a.s);
    if (R == 0) return;
    const uint64_t total = min(a.s.offsets[R], a.s.q_bound); // never beyond the section
    const uint64_t c0 = (uint64_t)blockIdx.x * FQA_CHUNK_BYTES;
    if (c0 >= total) return; // uniform
    const uint64_t c1 = min(c0 + FQA_CHUNK_BYTES, total);
    if (HIST) {
        for (uint32_t i = t; i < FQA_TABLES * FQA_TABLE_STRIDE; i += FQA_THREADS) s_tab[i] = 0;
        __syncthreads();
    }
    uint32_t *tab = s_tab + (HIST ? fqa_table_slot(t, 0) : 0);
    // minimum and maximum of the even and of the odd bytes, as two 16-bit halves each
    fqa_h2 lo = {0xff, 0xff}, hi = {0, 0};
    for (uint64_t g = c0 + 16u * t; g < c1; g += FQA_STEP) { // a granule with a byte below c1 <= offsets[NREAL]
        const fqa_u4 v = __builtin_nontemporal_load(reinterpret_cast<const fqa_u4 *>(a.s.pq + g));
        uint32_t word[4] = {v.x, v.y, v.z, v.w};
        const uint32_t n = (uint32_t)min((uint64_t)16, c1 - g);
        if (n < 16) fqa_fill_tail(word, n); // the batch's last granule
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const fqa_h2 ev = fqa_halves(word[k] & 0x00ff00ffu), od = fqa_halves((word[k] >> 8) & 0x00ff00ffu);
            lo = __builtin_elementwise_min(lo, __builtin_elementwise_min(ev, od));
            hi = __builtin_elementwise_max(hi, __builtin_elementwise_max(ev, od));
        }
        if (HIST) { // runs of equal bytes are added once
            uint32_t cur = word[0] & 0xffu, run = 0;
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t q = fqa_byte(word, i);
                if (i < n) {
                    if (q != cur) {
                        atomicAdd(tab + cur, run);
                        cur = q;
                        run = 0;
                    }
                    ++run;
                }
            }
            atomicAdd(tab + cur, run);
        }
    }
    uint32_t mn = min((uint32_t)lo.x, (uint32_t)lo.y), mx = max((uint32_t)hi.x, (uint32_t)hi.y);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mn = min(mn, (uint32_t)__shfl_xor(mn, d));
        mx = max(mx, (uint32_t)__shfl_xor(mx, d));
    }
    if (lane == 0) {
        s_lo[wv] = mn;
        s_hi[wv] = mx;
    }
    __syncthreads(); // (the LDS atomics are done too)
    if (t == 0) {
#pragma unroll
        for (int ww = 1; ww < FQA_THREADS / 64; ++ww) {
            mn = min(mn, s_lo[ww]);
            mx = max(mx, s_hi[ww]);
        }
        // the chunk holds a byte (c0 < c1), so a lane of the workgroup has loaded one
        atomicAdd(reinterpret_cast<fqa_ull *>(a.aud + FQA_W_QUAL_BYTES), (fqa_ull)(c1 - c0));
        atomicMin(reinterpret_cast<fqa_ull *>(a.aud + FQA_W_QUAL_MIN), (fqa_ull)mn);
        atomicMax(reinterpret_cast<fqa_ull *>(a.aud + FQA_W_QUAL_MAX), (fqa_ull)mx);
    }
    if (HIST) {
        uint32_t sum = 0; // lane t: value t
#pragma unroll
        for (uint32_t k = 0; k < FQA_TABLES; ++k) sum += s_tab[k * FQA_TABLE_STRIDE + t];
        if (sum) atomicAdd(reinterpret_cast<fqa_ull *>(a.hist + t), (fqa_ull)sum);
    }
}

// ------------------------------------------------------------------------------------------
// 3 the fold
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) sk_fq_audit_fold_kernel(fqa_args a, int names)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool valid = fqs_valid(a.s);
    a.aud[valid ? FQA_W_CALLS : FQA_W_CALLS_FAILED] += 1;
    if (valid && names) fqa_fold(a.aud);
}

} // namespace

// the arguments have passed the checks of sk_trim_fastq_audit_device_async (sk_capi.hip)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_audit(const sk_fastq_report_source *src,
                                                                                  const sk_fastq_input *in, int mode,
                                                                                  sk_fastq_audit *audit_dev,
                                                                                  uint64_t *qual_hist_dev, int flags,
                                                                                  hipStream_t stream)
{
    fqa_args a = {};
    fqs_fill(src, in, mode, &a.s);
    a.aud = reinterpret_cast<uint64_t *>(audit_dev);
    a.hist = qual_hist_dev;
    const bool names = in && a.s.mode != SK_TRIM_SE; // (an SE call's texts are in the view and nothing looks at them)
    const dim3 threads(FQA_THREADS);
    if (flags & SK_FQ_AUDIT_RESET) hipLaunchKernelGGL(sk_fq_audit_reset_kernel, dim3(1), threads, 0, stream, a);
    if (names) {
        uint64_t n_pack = sk_fq_pack_reads(a.s.bytes[0], a.s.bytes[1], a.s.mode);
        if (n_pack > a.s.n_bound) n_pack = a.s.n_bound;
        const uint64_t n_blocks = (n_pack + SK_FQ_BLOCK_READS - 1) / SK_FQ_BLOCK_READS;
        if (n_blocks) hipLaunchKernelGGL(sk_fq_audit_names_kernel, dim3((unsigned)n_blocks), threads, 0, stream, a);
    }
    // the packed qual is at most half the text
    const uint64_t n_chunks = (src->text_bytes / 2 + FQA_CHUNK_BYTES - 1) / FQA_CHUNK_BYTES;
    if (n_chunks) {
        if (a.hist) hipLaunchKernelGGL(sk_fq_audit_qual_kernel<true>, dim3((unsigned)n_chunks), threads, 0, stream, a);
        else hipLaunchKernelGGL(sk_fq_audit_qual_kernel<false>, dim3((unsigned)n_chunks), threads, 0, stream, a);
    }
    hipLaunchKernelGGL(sk_fq_audit_fold_kernel, dim3(1), dim3(64), 0, stream, a, names ? 1 : 0);
    return hipGetLastError();
}
