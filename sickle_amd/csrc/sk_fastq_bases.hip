// sk_fastq_bases.hip -- the bases over a finished text call's workspace and texts (sk_trim_fastq_bases_device_async): the
// rule of sk_fastq_bases.h summed on the device into a sk_fastq_bases and the caller's arrays.
//
// Launches on the text call's stream, behind its emission; no inter-workgroup waiting, and the result does not depend on
// the order of workgroups: every global write is an integer atomic add, but for the reset kernel's stores.
//   0 reset  (SK_FQ_BASES_RESET only) zeroes the struct and the given arrays
//   1 bases  a workgroup takes FQB_CHUNK_BYTES of the packed batch's positions, which number the seq bytes as they number
//            the quality bytes, in steps of 256 granules of 16 positions.  It finds its first read by a 64-ary search in
//            offsets and stages the next FQB_WIN reads' bounds, cuts and seq starts in LDS per step, as the report's
//            quality pass does.  A lane cuts its granule into segments, one per read in it, loads a segment's sixteen text
//            bytes with one bounded load (the text is not aligned to the granule) and classifies them with packed byte
//            operations (fqb_segment): a mask per class.  Everything that is a sum over bytes comes from popcounts of
//            those masks into registers: the class totals, the LOWER bytes, and every position at or beyond the last bin.
//            Only the position bins below the last take LDS atomics: one 64-bit word per class and bin, the count over all
//            reads in its low half and the count over output bytes in its high half, so that a byte of a read with
//            five == 0 adds both with ONE atomic.
//            A read's own figures (an N at all, GC) need the whole line.  A read inside one granule is finished in
//            registers.  A read that lanes share gets a pair of LDS words for the step (fqb_read_part: acgt, C + G and
//            the N flag in one word, for the line and for the output), numbered by the lane its first byte of the step
//            lies in, or the carry slot when it began before the step; behind the step's barrier the lane that holds its
//            first byte finishes it, or carries it into the next step.  The workgroup that holds a read's first byte owns
//            its figures: it walks the part of the read beyond its chunk once more, all lanes, adding to nothing but that
//            pair of words; at most one read per chunk is read twice, and the read's length bounds the walk.
// Every workgroup takes the call's validity from the header (fqs_valid) and leaves at once when the call does not add.
// Workgroups at or beyond offsets[NREAL] load nothing else.  A source that names the wrong layout or the wrong texts gives
// wrong numbers, no load outside the workspace and the texts, and no unbounded walk: the bounds and the seq line's clamps
// are the source view's (sk_fastq_source.h), and fqb_load16 holds every seq byte to in->bytes[i].
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_fastq_audit.h"
#include "sk_fastq_bases.h"
#include "sk_fastq_order.h"
#include "sk_fastq_report.h"
#include "sk_fastq_source.h"

namespace {

typedef unsigned long long fqb_ull;

#define FQB_THREADS 256
#define FQB_STEP (FQB_THREADS * 16u) // packed positions of one step of a workgroup
#define FQB_WIN 128                  // reads of a step staged in LDS (further ones are searched in global memory)
#define FQB_CARRY FQB_THREADS        // the two carry slots of s_rd, taken in turn: the read that began before the step
#define FQB_SCALARS 20               // the struct's words from FQB_W_READS to FQB_W_GC_NONE_OUT, a register each
#define FQB_REGS (FQB_SCALARS + 2 * FQB_CLASSES) // and the last position bin of either table

static_assert(FQB_CHUNK_BYTES % FQB_STEP == 0, "a chunk is whole steps");
static_assert(FQB_W_GC_NONE_OUT - FQB_W_READS + 1 == FQB_SCALARS, "the scalar registers are the struct's words in order");
static_assert(SK_FQ_BASES_GC_BINS <= FQB_THREADS && FQB_REGS <= FQB_THREADS, "one lane flushes one word");

struct fqb_args {
    fqs_view s;    // the call behind
    uint64_t *bas; // sk_fastq_bases as FQB_WORDS words
    uint64_t *pos_in, *pos_out, *gc_in, *gc_out;
    uint32_t pos_bins;
};

__device__ __forceinline__ void fqb_add(uint64_t *p, uint64_t v)
{
    if (v) atomicAdd(reinterpret_cast<fqb_ull *>(p), (fqb_ull)v);
}

// a shared read's pair of words: the sums are added, the flag is OR-ed (fqb_read_add, on LDS)
__device__ __forceinline__ void fqb_lds_read_add(uint64_t *word, uint64_t part)
{
    if (part & ~FQB_R_N) atomicAdd(reinterpret_cast<fqb_ull *>(word), (fqb_ull)(part & ~FQB_R_N));
    if (part & FQB_R_N) atomicOr(reinterpret_cast<fqb_ull *>(word), (fqb_ull)FQB_R_N);
}

// ------------------------------------------------------------------------------------------
// 0 reset
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQB_THREADS) sk_fq_bases_reset_kernel(fqb_args a)
{
    const uint32_t i = blockIdx.x * FQB_THREADS + threadIdx.x;
    if (i < FQB_WORDS) a.bas[i] = 0;
    if (i < FQB_CLASSES * a.pos_bins) {
        if (a.pos_in) a.pos_in[i] = 0;
        if (a.pos_out) a.pos_out[i] = 0;
    }
    if (i < SK_FQ_BASES_GC_BINS) {
        if (a.gc_in) a.gc_in[i] = 0;
        if (a.gc_out) a.gc_out[i] = 0;
    }
}

// ------------------------------------------------------------------------------------------
// 1 the pass
// ------------------------------------------------------------------------------------------
template <bool POS>
__global__ void __launch_bounds__(FQB_THREADS) sk_fq_bases_kernel(fqb_args a)
{
    extern __shared__ uint64_t s_tab[]; // POS: [class][PS], PS = fqp_slots(pos_bins): bin p at fqp_slot(p), out << 32 | in
    __shared__ uint64_t s_off[FQB_WIN + 1];
    __shared__ uint64_t s_seq[FQB_WIN];
    __shared__ sk_cut_dev s_cut[FQB_WIN];
    __shared__ uint64_t s_rd[2][FQB_THREADS + 2]; // [line, output][the lane a shared read starts in; the two carry slots]
    __shared__ uint64_t s_cur, s_tail;            // the step's first read; the read carried out of the step, ~0: none
    __shared__ uint32_t s_gc[2][SK_FQ_BASES_GC_BINS];
    __shared__ uint32_t s_reg[FQB_REGS];
    __shared__ uint64_t *s_dst[5]; // where the flush adds: held in scalar registers across the loop they would cost spills
    const int t = threadIdx.x, lane = t & 63;
    const bool valid = fqs_valid(a.s); // uniform
    if (blockIdx.x == 0 && t == 0) atomicAdd(reinterpret_cast<fqb_ull *>(a.bas + (valid ? FQB_W_CALLS : FQB_W_CALLS_FAILED)), 1ull);
    if (!valid) return;
    const uint64_t R = fqs_reads(a.s);
    if (R == 0) return;
    // The pass below walks packed positions and meets a read at its bytes, so a read of no bases is met nowhere.  No text
    // that passes the checks holds one, but a clipped call (sk_trim_fastq_clipped_device_async) packs one for every read
    // with its hit at 0: a read that came in, that the scan discarded, and that has no A, C, G or T.  The workgroups share
    // the reads evenly and count them from the offsets: a coalesced load a read, and no atomic where there is none.
    {
        const uint64_t r0 = R / gridDim.x * blockIdx.x + min((uint64_t)blockIdx.x, R % gridDim.x);
        const uint64_t r1 = r0 + R / gridDim.x + (blockIdx.x < R % gridDim.x ? 1 : 0);
        uint32_t empty = 0;
        for (uint64_t k = r0 + t; k < r1; k += FQB_THREADS) empty += a.s.offsets[k] == a.s.offsets[k + 1]; // k + 1 <= R
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) empty += __shfl_xor(empty, d);
        if (lane == 0 && empty) {
            fqb_add(a.bas + FQB_W_READS, empty);
            fqb_add(a.bas + FQB_W_GC_NONE_IN, empty);
        }
    }
    // == SK_FQ_H_PACKED: the reads behind the count are empty.  (Never beyond the section, and the walks below never leave
    // offsets[0 .. R]: a source that names the wrong layout gives wrong numbers, not loads outside the workspace.)
    const uint64_t total = min(a.s.offsets[R], a.s.q_bound);
    const uint64_t c0 = (uint64_t)blockIdx.x * FQB_CHUNK_BYTES;
    if (c0 >= total) return; // uniform
    const uint64_t c1 = min(c0 + FQB_CHUNK_BYTES, total);
    const uint32_t PB = POS ? a.pos_bins : 1u, last = PB - 1, PS = fqp_slots(PB);
    if (POS)
        for (uint32_t i = t; i < FQB_CLASSES * PS; i += FQB_THREADS) s_tab[i] = 0;
    for (uint32_t i = t; i < 2 * (FQB_THREADS + 2); i += FQB_THREADS) (&s_rd[0][0])[i] = 0;
    for (uint32_t i = t; i < 2 * SK_FQ_BASES_GC_BINS; i += FQB_THREADS) (&s_gc[0][0])[i] = 0;
    if (t < FQB_REGS) s_reg[t] = 0;
    if (t == 0) {
        s_dst[0] = a.bas;
        s_dst[1] = a.pos_in;
        s_dst[2] = a.pos_out;
        s_dst[3] = a.gc_in;
        s_dst[4] = a.gc_out;
    }
    auto off = [&](uint64_t k) { return a.s.offsets[k]; }; // k <= R
    // the read holding the chunk's first position: a 64-ary search by wave 0 (the last k < R with off(k) <= c0)
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
    // the lane's sums: FQB_W_READS .. FQB_W_GC_NONE_OUT, and the last bin of either table per class
    uint32_t n_reads = 0, n_kept = 0, tot_in[FQB_CLASSES] = {}, tot_out[FQB_CLASSES] = {}, low_in = 0, low_out = 0;
    uint32_t rn_in = 0, rn_out = 0, none_in = 0, none_out = 0, tail_in[FQB_CLASSES] = {}, tail_out[FQB_CLASSES] = {};
    // a whole read: its line's word, its output's word
    auto finish = [&](uint64_t wi, uint64_t wo, bool kept) {
        ++n_reads;
        rn_in += fqb_has_n(wi);
        const int32_t bi = fqb_gc_bin(wi);
        if (bi < 0) ++none_in;
        else atomicAdd(&s_gc[0][bi], 1u);
        if (kept) {
            ++n_kept;
            rn_out += fqb_has_n(wo);
            const int32_t bo = fqb_gc_bin(wo);
            if (bo < 0) ++none_out;
            else atomicAdd(&s_gc[1][bo], 1u);
        }
    };
    uint32_t step = 0;
    for (uint64_t s0 = c0; s0 < c1; s0 += FQB_STEP, ++step) {
        if (t <= FQB_WIN) s_off[t] = cur + t <= R ? off(cur + t) : ~0ull;
        if (t < FQB_WIN && cur + t < R) {
            s_cut[t] = a.s.cuts[cur + t];
            s_seq[t] = fqs_seq_start(a.s, cur + t);
        }
        if (t == 0) s_tail = ~0ull;
        __syncthreads();
        const uint64_t s1 = min(s0 + FQB_STEP, c1);
        const uint32_t carry_in = FQB_CARRY + (step & 1), carry_out = FQB_CARRY + ((step + 1) & 1);
        const uint64_t g = s0 + 16u * t;
        uint64_t k = cur;
        // what this lane settles behind the barrier: the read that starts in its granule and runs on (`mine`), and, lane 0
        // only, the read that began before the step (`came`)
        bool mine = false, mine_kept = false, came = false, came_kept = false;
        uint64_t mine_e = 0, mine_k = 0, came_b = 0, came_e = 0, came_k = 0;
        if (g < s1) {
            if (g < s_off[FQB_WIN]) {
                int lo = 0, hi = FQB_WIN; // s_off[lo] <= g < s_off[hi]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_off[mid] <= g) lo = mid; else hi = mid;
                }
                k = cur + lo;
            } else if (cur + FQB_WIN < R) {
                uint64_t lo = cur + FQB_WIN, hi = R; // off(lo) <= g < off(hi)
                while (hi - lo > 1) {
                    const uint64_t mid = lo + ((hi - lo) >> 1);
                    if (off(mid) <= g) lo = mid; else hi = mid;
                }
                k = lo;
            } // (no third case: g < off(R), and s_off[FQB_WIN] holds off(R) or ~0 where the window reaches R)
            // read k's bounds, cut and seq start
            uint64_t b, e, sq;
            sk_cut_dev c;
            auto load = [&]() {
                const uint64_t i = k - cur;
                b = i < FQB_WIN ? s_off[i] : off(k);
                e = i < FQB_WIN ? s_off[i + 1] : off(k + 1);
                c = i < FQB_WIN ? s_cut[i] : a.s.cuts[k];
                sq = i < FQB_WIN ? s_seq[i] : fqs_seq_start(a.s, k);
            };
            load();
            const uint64_t g1 = min(g + 16, s1);
            uint64_t at = g;
            while (at < g1) { // a segment a turn: at most 16 turns
                while (at >= e && k + 1 < R) { // at < total = off(R): the bound on k never ends the walk of a batch
                    ++k;
                    load();
                }
                if (at >= e || at < b) break; // only where offsets are no offsets
                const uint64_t z = min(e, g1), p0 = at - b;
                const uint32_t n = (uint32_t)(z - at), all = fqb_range16(0, n);
                const int i = fqs_input(a.s, k);
                const bool kept = fqp_kept(c.three);
                uint64_t w[2];
                fqb_load16(a.s.text[i], a.s.bytes[i], sq + p0, w);
                fqb_seg sg;
                fqb_segment(w, n, p0, c.five, c.three, &sg);
#pragma unroll
                for (int cl = 0; cl < FQB_CLASSES; ++cl) {
                    tot_in[cl] += __builtin_popcount(sg.m[cl]);
                    tot_out[cl] += __builtin_popcount(sg.m[cl] & sg.out);
                }
                low_in += __builtin_popcount(sg.lower);
                low_out += __builtin_popcount(sg.lower & sg.out);
                if (POS) {
                    // the positions at or beyond the last bin, of the line and of the output (p - five there)
                    const uint32_t far_in = fqb_range16((int64_t)last - (int64_t)p0, 16) & all;
                    const uint32_t far_out = fqb_range16((int64_t)last + (int64_t)c.five - (int64_t)p0, 16) & sg.out;
#pragma unroll
                    for (int cl = 0; cl < FQB_CLASSES; ++cl) {
                        tail_in[cl] += __builtin_popcount(sg.m[cl] & far_in);
                        tail_out[cl] += __builtin_popcount(sg.m[cl] & far_out);
                    }
                    const uint32_t near_in = all & ~far_in, near_out = sg.out & ~far_out;
                    if (near_in | near_out) {
#pragma unroll
                        for (uint32_t j = 0; j < 16; ++j) {
                            const uint32_t bit = 1u << j;
                            if ((near_in | near_out) & bit) {
                                uint64_t *row = s_tab + fqb_code_at(&sg, j) * PS;
                                const uint32_t p = (uint32_t)p0 + j; // below `last` wherever it is used as a bin
                                const bool in = near_in & bit, out = near_out & bit;
                                if (in && out && c.five == 0) {
                                    atomicAdd(reinterpret_cast<fqb_ull *>(row + fqp_slot(p)), (fqb_ull)((1ull << 32) | 1ull));
                                } else {
                                    if (in) atomicAdd(reinterpret_cast<fqb_ull *>(row + fqp_slot(p)), (fqb_ull)1);
                                    if (out) atomicAdd(reinterpret_cast<fqb_ull *>(row + fqp_slot(p - (uint32_t)c.five)), (fqb_ull)(1ull << 32));
                                }
                            }
                        }
                    }
                }
                const uint64_t wi = fqb_read_part(&sg, all), wo = fqb_read_part(&sg, sg.out);
                if (at == b && z == e) {
                    finish(wi, wo, kept); // the whole read lies in this granule
                } else {
                    const uint32_t slot = b < s0 ? carry_in : (uint32_t)((b - s0) >> 4);
                    fqb_lds_read_add(&s_rd[0][slot], wi);
                    fqb_lds_read_add(&s_rd[1][slot], wo);
                    if (at == b) { // it starts here and runs on
                        mine = true;
                        mine_kept = kept;
                        mine_e = e;
                        mine_k = k;
                    } else if (t == 0 && b < s0) {
                        came = true;
                        came_kept = kept;
                        came_b = b;
                        came_e = e;
                        came_k = k;
                    }
                }
                at = z;
            }
        }
        // the next step starts at or after the read of the last lane's last position
        if (t == FQB_THREADS - 1) s_cur = k;
        __syncthreads(); // (the LDS atomics of the step are done)
        // A read that has ended is finished; the one that has not goes to the other carry slot.  At most one read leaves a
        // step, and where the read that came in leaves it too, no other read has a byte in the step: one writer.
        if (came) {
            const uint64_t wi = s_rd[0][carry_in], wo = s_rd[1][carry_in];
            s_rd[0][carry_in] = s_rd[1][carry_in] = 0;
            if (came_e <= s1) {
                if (came_b >= c0) finish(wi, wo, came_kept); // else its first byte is another workgroup's
            } else {
                s_rd[0][carry_out] = wi;
                s_rd[1][carry_out] = wo;
                s_tail = came_k;
            }
        }
        if (mine) {
            const uint64_t wi = s_rd[0][t], wo = s_rd[1][t];
            s_rd[0][t] = s_rd[1][t] = 0;
            if (mine_e <= s1) {
                finish(wi, wo, mine_kept);
            } else {
                s_rd[0][carry_out] = wi;
                s_rd[1][carry_out] = wo;
                s_tail = mine_k;
            }
        }
        __syncthreads();
        cur = s_cur;
    }
    // The read that runs beyond the chunk, if its first byte is this workgroup's: the rest of it, for its own two words only.
    const uint64_t tail = s_tail;                      // uniform
    const uint32_t carry = FQB_CARRY + (step & 1);     // where the last step left it
    if (tail < R) {
        const uint64_t b = off(tail), e = min(off(tail + 1), total);
        if (b >= c0 && b < c1) { // uniform
            const sk_cut_dev c = a.s.cuts[tail];
            const uint64_t sq = fqs_seq_start(a.s, tail);
            const int i = fqs_input(a.s, tail);
            uint64_t wi = 0, wo = 0;
            for (uint64_t q = c1 + 16u * t; q < e; q += FQB_STEP) { // bounded by the read's length
                const uint32_t n = (uint32_t)min((uint64_t)16, e - q);
                uint64_t w[2];
                fqb_load16(a.s.text[i], a.s.bytes[i], sq + (q - b), w);
                fqb_seg sg;
                fqb_segment(w, n, q - b, c.five, c.three, &sg);
                wi = fqb_read_add(wi, fqb_read_part(&sg, fqb_range16(0, n)));
                wo = fqb_read_add(wo, fqb_read_part(&sg, sg.out));
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                wi = fqb_read_add(wi, __shfl_xor(wi, d));
                wo = fqb_read_add(wo, __shfl_xor(wo, d));
            }
            if (lane == 0) {
                fqb_lds_read_add(&s_rd[0][carry], wi);
                fqb_lds_read_add(&s_rd[1][carry], wo);
            }
            __syncthreads();
            if (t == 0) finish(s_rd[0][carry], s_rd[1][carry], fqp_kept(c.three));
        }
    }
    // the wave, then the workgroup, then one global atomic per non-zero word
    uint32_t v[FQB_REGS];
    v[0] = n_reads;
    v[1] = n_kept;
#pragma unroll
    for (int cl = 0; cl < FQB_CLASSES; ++cl) {
        v[2 + cl] = tot_in[cl];
        v[2 + FQB_CLASSES + cl] = tot_out[cl];
        v[FQB_SCALARS + cl] = tail_in[cl];
        v[FQB_SCALARS + FQB_CLASSES + cl] = tail_out[cl];
    }
    v[14] = low_in;
    v[15] = low_out;
    v[16] = rn_in;
    v[17] = rn_out;
    v[18] = none_in;
    v[19] = none_out;
#pragma unroll
    for (int j = 0; j < FQB_REGS; ++j) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v[j] += __shfl_xor(v[j], d);
        if (lane == 0 && v[j]) atomicAdd(&s_reg[j], v[j]);
    }
    __syncthreads(); // (the GC counters are done too)
    uint64_t *const bas = s_dst[0], *const pos_in = s_dst[1], *const pos_out = s_dst[2], *const gc_in = s_dst[3], *const gc_out = s_dst[4];
    if (t < FQB_SCALARS) fqb_add(bas + FQB_W_READS + t, s_reg[t]);
    if (t < (int)SK_FQ_BASES_GC_BINS) {
        if (gc_in) fqb_add(gc_in + t, s_gc[0][t]);
        if (gc_out) fqb_add(gc_out + t, s_gc[1][t]);
    }
    if (POS) {
        for (uint32_t i = t; i < PB; i += FQB_THREADS) {
#pragma unroll
            for (uint32_t cl = 0; cl < FQB_CLASSES; ++cl) {
                const uint64_t x = s_tab[cl * PS + fqp_slot(i)];
                uint64_t in = x & 0xffffffffull, out = x >> 32;
                if (i == last) {
                    in += s_reg[FQB_SCALARS + cl];
                    out += s_reg[FQB_SCALARS + FQB_CLASSES + cl];
                }
                if (pos_in) fqb_add(pos_in + (uint64_t)cl * PB + i, in);
                if (pos_out) fqb_add(pos_out + (uint64_t)cl * PB + i, out);
            }
        }
    }
}

} // namespace

// the arguments have passed the checks of sk_trim_fastq_bases_device_async (sk_capi.hip)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_bases(const sk_fastq_report_source *src,
                                                                                  const sk_fastq_input *in, int mode,
                                                                                  sk_fastq_bases *bases_dev,
                                                                                  const sk_fastq_bases_hists *hists, int flags,
                                                                                  hipStream_t stream)
{
    fqb_args a = {};
    fqs_fill(src, in, mode, &a.s);
    a.bas = reinterpret_cast<uint64_t *>(bases_dev);
    if (hists) {
        a.pos_in = hists->pos_in;
        a.pos_out = hists->pos_out;
        a.pos_bins = hists->pos_in || hists->pos_out ? (uint32_t)hists->pos_bins : 0;
        a.gc_in = hists->gc_in;
        a.gc_out = hists->gc_out;
    }
    const dim3 threads(FQB_THREADS);
    if (flags & SK_FQ_BASES_RESET) {
        uint32_t words = FQB_CLASSES * a.pos_bins;
        if (words < SK_FQ_BASES_GC_BINS) words = SK_FQ_BASES_GC_BINS;
        hipLaunchKernelGGL(sk_fq_bases_reset_kernel, dim3((words + FQB_THREADS - 1) / FQB_THREADS), threads, 0, stream, a);
    }
    // the packed seq is at most half the text; block 0 counts the call
    uint64_t n_chunks = (src->text_bytes / 2 + FQB_CHUNK_BYTES - 1) / FQB_CHUNK_BYTES;
    if (n_chunks == 0) n_chunks = 1;
    if (a.pos_bins)
        hipLaunchKernelGGL(sk_fq_bases_kernel<true>, dim3((unsigned)n_chunks), threads, 8 * FQB_CLASSES * fqp_slots(a.pos_bins), stream, a);
    else
        hipLaunchKernelGGL(sk_fq_bases_kernel<false>, dim3((unsigned)n_chunks), threads, 0, stream, a);
    return hipGetLastError();
}
