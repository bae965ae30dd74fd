// sk_fastq_adapters.hip -- the adapter search over a finished text call's workspace and texts
// (sk_trim_fastq_adapters_device_async): the rule of sk_fastq_adapters.h on the device, summed into a sk_fastq_adapters and
// the caller's arrays.
//
// Launches on the text call's stream, behind its emission; no inter-workgroup waiting, and the result does not depend on
// the order of workgroups: every global write is an integer atomic add, but for the reset kernel's stores and the clip
// words, of which each has one writer.
//   0 reset   (SK_FQ_ADAPTERS_RESET only) zeroes the struct, pos and overlap
//   1 search  The pass is bound by instructions, (line length x adapter bases) base comparisons a read, not by bytes, so
//             it is laid out by reads and not, like the report's and the bases' passes, by packed positions.  A wave takes
//             64 consecutive reads (whole pairs) a turn: lane j loads read j's bounds, cut and seq start, coalesced, and the
//             wave then searches the 64 lines one after the other, every lane on the same line, the line's figures
//             broadcast from lane j.  A line is walked in tiles of 64 starts, lane j the start t0 + j.  Lane j loads ONE
//             byte a tile, base t + j, and three wave ballots over its code turn the 64 bytes into one 64-bit word per
//             plane (fqd_planes) in scalar registers: the line is never staged in LDS, and a base is loaded and encoded
//             once.  The bytes are loaded three tiles ahead of their use, the next line's first three tiles while this
//             line is searched, so that no compare waits for memory.  The tile's window words are a tile's word and the
//             next one's; a lane forms its own 64-base window by a funnel shift by its lane number and compares it with
//             every adapter, whose planes are kernel arguments (fqd_start: two XORs, an OR with the invalid bits, a mask
//             to the overlap and one popcount per adapter; the kernel is a template on the number of adapters, so that
//             the loop over them unrolls and their planes stay in scalar registers).  The lowest set bit of the ballot
//             over the lanes' hits is the lowest start, and that lane names the adapter; the walk of a line ends at its
//             first tile with a hit.
//             What a read adds to the struct is summed a word a lane (lane w holds word w: fqd_read_word, fqd_pair_word) in
//             registers over the wave's reads, then over the workgroup's waves in LDS, then one global atomic per non-zero
//             word.  pos and overlap take one global atomic per hit, by lane 0; the clip words of a wave's 64 reads leave
//             in one coalesced store, lane j's the word of read j.
// Every workgroup takes the call's validity from the header (fqs_valid) and leaves at once when the call does not add.
// A source that names the wrong layout or the wrong texts gives wrong numbers, no load outside the workspace and the
// texts, and no unbounded walk: the bounds and the seq line's clamps are the source view's (sk_fastq_source.h), fqd_raw
// holds every seq byte to in->bytes[i], and a line's length is SK_MAX_READ_LEN at most.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_fastq_adapters.h"
#include "sk_fastq_audit.h"
#include "sk_fastq_clip.h"
#include "sk_fastq_order.h"
#include "sk_fastq_report.h"
#include "sk_fastq_source.h"

namespace {

typedef unsigned long long fqd_ull;

#define FQD_THREADS 256
#define FQD_WAVES (FQD_THREADS / 64)
#define FQD_MAX_BLOCKS 4096u // the groups of reads beyond them are taken in strides of the grid

static_assert(FQD_WORDS <= 64, "a lane holds a word of the struct");

struct fqd_args {
    fqs_view s;    // the call behind
    uint64_t *res; // sk_fastq_adapters as FQD_WORDS words
    uint64_t *pos, *overlap;
    uint32_t *clip;
    uint64_t clip_capacity;
    uint32_t pos_bins;
    fqd_codes codes;
};

// a seq line as the wave sees it: wave-uniform
struct fqd_line {
    const uint8_t *text;
    uint64_t bytes, sq, L; // the text's length, where the line starts in it, its length
};

// lane j's byte of bases [t, t + 64) of a line: base t + j as the text has it; 0, which is no letter, for a base at or
// beyond L and for a byte at or beyond the text's end
__device__ __forceinline__ uint32_t fqd_raw(const fqd_line &ln, uint64_t t, int lane)
{
    const uint64_t i = t + (uint64_t)lane;
    const bool in = i < ln.L && ln.sq + i < ln.bytes;
    if (ln.bytes == 0) return 0u; // uniform: no text, no load
    // (a lane without a byte of its own loads the line's first, or the text's last where the line starts at its end: one
    // unconditional load instead of a branch over one, and from the cache lines the other lanes load)
    const uint32_t b = ln.text[in ? ln.sq + i : min(ln.sq, ln.bytes - 1)];
    return in ? b : 0u;
}

// the wave's 64 bytes as a word per plane: three ballots over the lanes' codes
__device__ __forceinline__ fqd_planes fqd_ballot_planes(uint32_t raw)
{
    const uint32_t code = fqd_code((uint8_t)raw);
    fqd_planes w;
    w.lo = __builtin_amdgcn_ballot_w64((code & 1u) != 0);
    w.hi = __builtin_amdgcn_ballot_w64((code & 2u) != 0);
    w.valid = __builtin_amdgcn_ballot_w64(code < 4u);
    return w;
}

__device__ __forceinline__ uint64_t fqd_uniform(uint64_t x)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x), hi = __builtin_amdgcn_readfirstlane((uint32_t)(x >> 32));
    return (uint64_t)hi << 32 | lo;
}

// ------------------------------------------------------------------------------------------
// 0 reset
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQD_THREADS) sk_fq_adapters_reset_kernel(fqd_args a)
{
    const uint32_t i = blockIdx.x * FQD_THREADS + threadIdx.x;
    if (i < FQD_WORDS) a.res[i] = 0;
    if (a.pos && i < 8u * a.pos_bins) a.pos[i] = 0;
    if (a.overlap && i < 8u * SK_FQ_ADAPTERS_OVERLAP_BINS) a.overlap[i] = 0;
}

// ------------------------------------------------------------------------------------------
// 1 the search
// ------------------------------------------------------------------------------------------
// lane j's word of x (j wave-uniform), in every lane
__device__ __forceinline__ uint32_t fqd_lane32(uint32_t x, int j) { return (uint32_t)__builtin_amdgcn_readlane((int)x, j); }
__device__ __forceinline__ uint64_t fqd_lane64(uint64_t x, int j)
{
    return (uint64_t)fqd_lane32((uint32_t)(x >> 32), j) << 32 | fqd_lane32((uint32_t)x, j);
}

// The hit of a line (wave-uniform in and out; every lane returns the same fqd_read, whose L is the line's).  c0, c1, c2: the
// lanes' bytes of the line's first three tiles (fqd_raw), loaded by the caller ahead of time.  Further tiles are loaded
// three tiles ahead of their use, so that a load's latency is other tiles' compares.
template <uint32_t N>
__device__ __forceinline__ fqd_read fqd_search_line(const fqd_codes &codes, const fqd_line &ln, uint32_t c0, uint32_t c1, uint32_t c2, int lane)
{
    fqd_read rd = {};
    rd.L = ln.L;
    const uint64_t L = ln.L, mo = codes.min_overlap;
    if (L < mo) return rd;
    const uint64_t last = L - mo; // the last start
    fqd_planes w0 = fqd_ballot_planes(c0);
    for (uint64_t t0 = 0; t0 <= last; t0 += 64) { // at most 2^18 tiles
        const uint32_t c3 = t0 + 192 < L ? fqd_raw(ln, t0 + 192, lane) : 0u;
        const fqd_planes w1 = fqd_ballot_planes(c1);
        const uint64_t p = t0 + (uint64_t)lane;
        uint32_t ad = FQD_NO_ADAPTER;
        if (p <= last) {
            const uint64_t lo = fqd_funnel(w0.lo, w1.lo, (uint32_t)lane), hi = fqd_funnel(w0.hi, w1.hi, (uint32_t)lane);
            const uint64_t valid = fqd_funnel(w0.valid, w1.valid, (uint32_t)lane);
            ad = fqd_start(&codes, N, lo, hi, valid, L, p); // N == codes.n
        }
        const uint64_t hits = __builtin_amdgcn_ballot_w64(ad != FQD_NO_ADAPTER);
        if (hits) { // uniform: the lowest lane with a hit holds the lowest start; its overlap and mismatches once more
            const uint32_t src = (uint32_t)__builtin_ctzll(hits);
            rd.hit = 1;
            rd.a = fqd_lane32(ad, (int)src);
            rd.p = t0 + (uint64_t)src;
            uint32_t A = 0;
            uint64_t ad_lo = 0, ad_hi = 0;
#pragma unroll
            for (uint32_t j = 0; j < 8; ++j) { // (no runtime index into the kernel's arguments)
                A = rd.a == j ? codes.len[j] : A;
                ad_lo = rd.a == j ? codes.lo[j] : ad_lo;
                ad_hi = rd.a == j ? codes.hi[j] : ad_hi;
            }
            rd.A = A;
            rd.v = fqd_overlap(A, L, rd.p);
            rd.m = fqd_mismatches(fqd_funnel(w0.lo, w1.lo, src), fqd_funnel(w0.hi, w1.hi, src), fqd_funnel(w0.valid, w1.valid, src),
                                  ad_lo, ad_hi, rd.v);
            return rd;
        }
        w0 = w1;
        c1 = c2;
        c2 = c3;
    }
    return rd;
}

// N: the set's adapters, so that the loop over them unrolls and their planes stay in scalar registers
template <uint32_t N>
__global__ void __launch_bounds__(FQD_THREADS) sk_fq_adapters_kernel(fqd_args a)
{
    __shared__ fqd_ull s_sum[FQD_WORDS];
    const int t = threadIdx.x, lane = t & 63;
    const bool valid = fqs_valid(a.s); // uniform
    if (blockIdx.x == 0 && t == 0) atomicAdd(reinterpret_cast<fqd_ull *>(a.res + (valid ? FQD_W_CALLS : FQD_W_CALLS_FAILED)), 1ull);
    if (!valid) return;
    const uint64_t R = fqs_reads(a.s);
    if (R == 0) return;
    if (t < FQD_WORDS) s_sum[t] = 0;
    __syncthreads();
    const bool pairs = a.s.mode != SK_TRIM_SE, split = a.s.mode == SK_TRIM_PE_SPLIT;
    const uint64_t groups = (R + 63) / 64; // 64 consecutive reads, whole pairs, a wave's turn
    const uint64_t wave = fqd_uniform((uint64_t)blockIdx.x * FQD_WAVES + (uint64_t)(t >> 6)), n_waves = (uint64_t)gridDim.x * FQD_WAVES;
    uint64_t acc = 0; // lane w: what the wave's reads add to word w
    for (uint64_t g = wave; g < groups; g += n_waves) {
        // lane j: where read 64 g + j lies and how it was cut, by coalesced loads
        const uint64_t base = 64 * g, mine = base + (uint64_t)lane;
        const int n = (int)min((uint64_t)64, R - base); // uniform
        uint64_t my_L = 0, my_sq = 0;
        sk_cut_dev my_cut = {0, -1};
        if (mine < R) {
            const uint64_t b = a.s.offsets[mine], e = a.s.offsets[mine + 1]; // mine < R <= n_bound
            my_L = e > b ? min(e - b, (uint64_t)SK_MAX_READ_LEN_DEV) : 0;
            my_sq = fqs_seq_start(a.s, mine);
            my_cut = a.s.cuts[mine];
        }
        auto line = [&](int j) {
            const int i = split ? j & 1 : 0; // base is even: read base + j lies in input j & 1
            fqd_line ln;
            ln.text = a.s.text[i];
            ln.bytes = a.s.bytes[i];
            ln.sq = fqd_lane64(my_sq, j);
            ln.L = fqd_lane64(my_L, j);
            return ln;
        };
        uint32_t my_clip = SK_FQ_CLIP_NONE;
        fqd_read prev = {};
        // read j + 1's first three tiles are loaded while read j is searched
        fqd_line cur = line(0);
        uint32_t c0 = fqd_raw(cur, 0, lane), c1 = fqd_raw(cur, 64, lane), c2 = fqd_raw(cur, 128, lane);
        for (int j = 0; j < n; ++j) {
            fqd_line nxt = cur;
            uint32_t n0 = 0, n1 = 0, n2 = 0;
            if (j + 1 < n) {
                nxt = line(j + 1);
                n0 = fqd_raw(nxt, 0, lane);
                n1 = fqd_raw(nxt, 64, lane);
                n2 = fqd_raw(nxt, 128, lane);
            }
            fqd_read rd = fqd_search_line<N>(a.codes, cur, c0, c1, c2, lane);
            rd.five = (int32_t)fqd_lane32((uint32_t)my_cut.five, j);
            rd.three = (int32_t)fqd_lane32((uint32_t)my_cut.three, j);
            if (!rd.hit) { // uniform, and most reads
                acc += fqd_miss_word((uint32_t)lane, &rd);
            } else if (lane >= FQD_W_READS && lane <= FQD_W_BASES_HIT_OUT) {
                acc += fqd_read_word((uint32_t)lane, &rd);
            }
            if (pairs && (j & 1) && lane >= FQD_W_PAIRS_BOTH && lane <= FQD_W_PAIRS_SAME_CLIP)
                acc += fqd_pair_word((uint32_t)lane, &prev, &rd); // reads base + j - 1 and base + j are a pair, both below R
            if (lane == j) my_clip = fqd_clip_word(&rd);
            if (lane == 0 && rd.hit) {
                if (a.pos) atomicAdd(reinterpret_cast<fqd_ull *>(a.pos + (uint64_t)rd.a * a.pos_bins + fqp_bin(rd.p, a.pos_bins)), 1ull);
                if (a.overlap) atomicAdd(reinterpret_cast<fqd_ull *>(a.overlap + rd.a * SK_FQ_ADAPTERS_OVERLAP_BINS + rd.v), 1ull);
            }
            prev = rd;
            cur = nxt;
            c0 = n0;
            c1 = n1;
            c2 = n2;
        }
        if (a.clip && mine < R && mine < a.clip_capacity) a.clip[mine] = my_clip; // the group's words in one store
    }
    if (lane < FQD_WORDS && acc) atomicAdd(&s_sum[lane], (fqd_ull)acc);
    __syncthreads();
    if (t >= FQD_W_READS && t < FQD_W_RESERVED && s_sum[t]) atomicAdd(reinterpret_cast<fqd_ull *>(a.res + t), s_sum[t]);
}

// ------------------------------------------------------------------------------------------
// the clip of a clipped text call (sk_trim_fastq_clipped_device_async, sk_fastq_clip.h)
// ------------------------------------------------------------------------------------------
// The search again, inside the front of a text call, between its check and its pack: the same wave of 64 reads and the same
// walk of a line (fqd_search_line), with a line's length from its record descriptor (fqc_line), since the packed batch
// does not exist yet.  No cuts, no pair words, no histograms.  It writes the clip word of every read, which the pack then
// reads, and this call's own sums into the head of the clip section, which sk_fq_clip_reset_kernel has zeroed.
struct fqc_args {
    sk_fq_clip_src s;
    uint64_t *stats; // the call-local block, FQC_WORDS words
    uint32_t *clip;  // s.n_pack words at least
    fqd_codes codes;
};

// zeroes FQC_WORDS words: the call-local block in front of every search, a caller's struct with SK_FQ_CLIP_RESET
__global__ void __launch_bounds__(64) sk_fq_clip_reset_kernel(uint64_t *words)
{
    if (threadIdx.x < FQC_WORDS) words[threadIdx.x] = 0;
}

// text i's length: never beyond the bound the workspace was sized by (== fq_length of sk_fastq.hip)
__device__ __forceinline__ uint64_t fqc_length(const sk_fq_clip_src &s, int i)
{
    uint64_t n = s.bytes[i];
    if (s.bytes_dev[i]) n = min(n, *s.bytes_dev[i]);
    if (s.valid_dev[i] && *s.valid_dev[i] == 0) n = 0;
    return n;
}

template <uint32_t N>
__global__ void __launch_bounds__(FQD_THREADS) sk_fq_clip_kernel(fqc_args a)
{
    __shared__ fqd_ull s_sum[FQC_WORDS];
    const int t = threadIdx.x, lane = t & 63;
    // a malformed text: its descriptors are not to be trusted, and the pack packs nothing either
    if (a.s.hdr[SK_FQ_H_FMT] != ~0ull) return; // uniform
    const uint64_t R = min(a.s.hdr[SK_FQ_H_NREAL], a.s.n_pack);
    if (R == 0) return;
    if (t < FQC_WORDS) s_sum[t] = 0;
    __syncthreads();
    const bool split = a.s.mode == SK_TRIM_PE_SPLIT;
    const uint64_t bytes[2] = {fqc_length(a.s, 0), split ? fqc_length(a.s, 1) : 0};
    const uint64_t groups = (R + 63) / 64; // 64 consecutive reads a wave's turn
    const uint64_t wave = fqd_uniform((uint64_t)blockIdx.x * FQD_WAVES + (uint64_t)(t >> 6)), n_waves = (uint64_t)gridDim.x * FQD_WAVES;
    uint64_t acc = 0; // lane w: what the wave's reads add to word w
    for (uint64_t g = wave; g < groups; g += n_waves) {
        // lane j: where the seq line of read 64 g + j lies, from its descriptor's two words, by coalesced loads
        const uint64_t base = 64 * g, mine = base + (uint64_t)lane;
        const int n = (int)min((uint64_t)64, R - base); // uniform
        uint64_t my_L = 0, my_sq = 0;
        if (mine < R) {
            const int i = split ? (int)(mine & 1) : 0;
            const uint64_t k = split ? mine >> 1 : mine;
            if (k < a.s.slots[i]) { // (always: every record with a line has a slot)
                const uint64_t *d = a.s.desc[i] + 5 * k;
                const fqc_span sp = fqc_line(d[1], d[2], i ? bytes[1] : bytes[0]);
                my_L = sp.L;
                my_sq = sp.sq;
            }
        }
        auto line = [&](int j) {
            const int i = split ? j & 1 : 0; // base is even: read base + j lies in input j & 1
            fqd_line ln;
            ln.text = a.s.text[i];
            ln.bytes = i ? bytes[1] : bytes[0];
            ln.sq = fqd_lane64(my_sq, j);
            ln.L = fqd_lane64(my_L, j);
            return ln;
        };
        uint32_t my_clip = SK_FQ_CLIP_NONE;
        // read j + 1's first three tiles are loaded while read j is searched
        fqd_line cur = line(0);
        uint32_t c0 = fqd_raw(cur, 0, lane), c1 = fqd_raw(cur, 64, lane), c2 = fqd_raw(cur, 128, lane);
        for (int j = 0; j < n; ++j) {
            fqd_line nxt = cur;
            uint32_t n0 = 0, n1 = 0, n2 = 0;
            if (j + 1 < n) {
                nxt = line(j + 1);
                n0 = fqd_raw(nxt, 0, lane);
                n1 = fqd_raw(nxt, 64, lane);
                n2 = fqd_raw(nxt, 128, lane);
            }
            const fqd_read rd = fqd_search_line<N>(a.codes, cur, c0, c1, c2, lane);
            if (!rd.hit) { // uniform, and most reads
                acc += lane == FQC_W_READS;
            } else {
                if (lane >= FQC_W_READS && lane < FQC_W_RESERVED) acc += fqc_read_word((uint32_t)lane, &rd);
                if (lane == j) my_clip = fqd_clip_word(&rd);
            }
            cur = nxt;
            c0 = n0;
            c1 = n1;
            c2 = n2;
        }
        if (mine < R) a.clip[mine] = my_clip; // the group's words in one store; mine < R <= n_pack
    }
    if (lane < FQC_WORDS && acc) atomicAdd(&s_sum[lane], (fqd_ull)acc);
    __syncthreads();
    if (t >= FQC_W_READS && t < FQC_W_RESERVED && s_sum[t]) atomicAdd(reinterpret_cast<fqd_ull *>(a.stats + t), s_sum[t]);
}

// behind the emission, one workgroup: the call-local sums into the caller's struct iff the call adds (fqs_valid; s: the
// words the validity reads)
__global__ void __launch_bounds__(64) sk_fq_clip_commit_kernel(fqs_view s, const uint64_t *local, uint64_t *stats)
{
    const uint32_t w = threadIdx.x;
    if (w >= FQC_W_RESERVED) return;
    const bool valid = fqs_valid(s); // uniform
    uint64_t add = 0;
    if (valid) add = w == FQC_W_CALLS ? 1 : w >= FQC_W_READS ? local[w] : 0;
    else add = w == FQC_W_CALLS_FAILED;
    if (add) atomicAdd(reinterpret_cast<fqd_ull *>(stats + w), (fqd_ull)add);
}

} // namespace

// the arguments have passed the checks of sk_trim_fastq_adapters_device_async (sk_capi.hip)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_adapters(const sk_fastq_report_source *src,
                                                                                     const sk_fastq_input *in, int mode,
                                                                                     const sk_fastq_adapter_set *set,
                                                                                     sk_fastq_adapters *adapters_dev,
                                                                                     const sk_fastq_adapters_out *out, int flags,
                                                                                     int cu_count, hipStream_t stream)
{
    fqd_args a = {};
    fqs_fill(src, in, mode, &a.s);
    a.res = reinterpret_cast<uint64_t *>(adapters_dev);
    if (out) {
        a.pos = out->pos;
        a.pos_bins = out->pos ? (uint32_t)out->pos_bins : 0;
        a.overlap = out->overlap;
        a.clip = out->clip;
        a.clip_capacity = out->clip ? out->clip_capacity : 0;
    }
    fqd_encode_set(set, &a.codes);
    const dim3 threads(FQD_THREADS);
    if (flags & SK_FQ_ADAPTERS_RESET) {
        uint32_t words = 8u * a.pos_bins;
        if (words < 8u * SK_FQ_ADAPTERS_OVERLAP_BINS) words = 8u * SK_FQ_ADAPTERS_OVERLAP_BINS;
        hipLaunchKernelGGL(sk_fq_adapters_reset_kernel, dim3((words + FQD_THREADS - 1) / FQD_THREADS), threads, 0, stream, a);
    }
    // a wave a group of 64 reads, at most a few workgroups a CU: the rest of the groups in strides of the grid; block 0 counts
    // the call
    uint64_t blocks = ((a.s.n_bound + 63) / 64 + FQD_WAVES - 1) / FQD_WAVES;
    const uint64_t cap = cu_count > 0 ? min((uint64_t)cu_count * 16u, (uint64_t)FQD_MAX_BLOCKS) : FQD_MAX_BLOCKS;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    const dim3 grid((unsigned)blocks);
    switch (a.codes.n) {
    case 1: hipLaunchKernelGGL(sk_fq_adapters_kernel<1>, grid, threads, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(sk_fq_adapters_kernel<2>, grid, threads, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(sk_fq_adapters_kernel<3>, grid, threads, 0, stream, a); break;
    case 4: hipLaunchKernelGGL(sk_fq_adapters_kernel<4>, grid, threads, 0, stream, a); break;
    case 5: hipLaunchKernelGGL(sk_fq_adapters_kernel<5>, grid, threads, 0, stream, a); break;
    case 6: hipLaunchKernelGGL(sk_fq_adapters_kernel<6>, grid, threads, 0, stream, a); break;
    case 7: hipLaunchKernelGGL(sk_fq_adapters_kernel<7>, grid, threads, 0, stream, a); break;
    default: hipLaunchKernelGGL(sk_fq_adapters_kernel<8>, grid, threads, 0, stream, a); break;
    }
    return hipGetLastError();
}

// the set has passed fqd_set_error (sk_trim_fastq_clipped_device_async, sk_capi.hip)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_clip(const sk_fq_clip_src *src,
                                                                                 const sk_fq_clip_front *clip, int cu_count,
                                                                                 hipStream_t stream)
{
    fqc_args a = {};
    a.s = *src;
    a.stats = static_cast<uint64_t *>(clip->section);
    a.clip = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(clip->section) + FQC_STATS_BYTES);
    fqd_encode_set(clip->set, &a.codes);
    hipLaunchKernelGGL(sk_fq_clip_reset_kernel, dim3(1), dim3(64), 0, stream, a.stats);
    // the adapters' grid: a wave a group of 64 reads, the rest of the groups in strides of the grid
    uint64_t blocks = ((src->n_pack + 63) / 64 + FQD_WAVES - 1) / FQD_WAVES;
    const uint64_t cap = cu_count > 0 ? min((uint64_t)cu_count * 16u, (uint64_t)FQD_MAX_BLOCKS) : FQD_MAX_BLOCKS;
    if (blocks > cap) blocks = cap;
    if (blocks == 0) blocks = 1;
    const dim3 grid((unsigned)blocks), threads(FQD_THREADS);
    switch (a.codes.n) {
    case 1: hipLaunchKernelGGL(sk_fq_clip_kernel<1>, grid, threads, 0, stream, a); break;
    case 2: hipLaunchKernelGGL(sk_fq_clip_kernel<2>, grid, threads, 0, stream, a); break;
    case 3: hipLaunchKernelGGL(sk_fq_clip_kernel<3>, grid, threads, 0, stream, a); break;
    case 4: hipLaunchKernelGGL(sk_fq_clip_kernel<4>, grid, threads, 0, stream, a); break;
    case 5: hipLaunchKernelGGL(sk_fq_clip_kernel<5>, grid, threads, 0, stream, a); break;
    case 6: hipLaunchKernelGGL(sk_fq_clip_kernel<6>, grid, threads, 0, stream, a); break;
    case 7: hipLaunchKernelGGL(sk_fq_clip_kernel<7>, grid, threads, 0, stream, a); break;
    default: hipLaunchKernelGGL(sk_fq_clip_kernel<8>, grid, threads, 0, stream, a); break;
    }
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_clip_reset(sk_fastq_clip_stats *stats_dev,
                                                                                       hipStream_t stream)
{
    hipLaunchKernelGGL(sk_fq_clip_reset_kernel, dim3(1), dim3(64), 0, stream, reinterpret_cast<uint64_t *>(stats_dev));
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_clip_commit(const void *workspace, uint32_t kind,
                                                                                        int mode, const void *section,
                                                                                        sk_fastq_clip_stats *stats_dev,
                                                                                        hipStream_t stream)
{
    fqs_view s = {};
    fqs_fill_validity(workspace, kind, mode, &s);
    hipLaunchKernelGGL(sk_fq_clip_commit_kernel, dim3(1), dim3(64), 0, stream, s, static_cast<const uint64_t *>(section),
                       reinterpret_cast<uint64_t *>(stats_dev));
    return hipGetLastError();
}
