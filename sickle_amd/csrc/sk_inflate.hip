// sk_inflate.hip -- BGZF read on the device (sk_bgzf_inflate_device_async): a BGZF byte image in device memory -> its text
// in device memory, every member's CRC-32 and ISIZE checked.
//
// Launches on one stream, no inter-workgroup waiting:
//   1 count    every byte position is tested for 1f 8b 08 04 (a CANDIDATE); matches per tile of 4096 positions
//   2 tiles    one workgroup: exclusive scan of the tile counts, the header words
//   3 list     the candidates' positions, compacted in order
//   4 parse    per candidate: the header test (ski_parse_member), then its successor pos + BSIZE + 1 among the candidates
//              by binary search; candidate 0 gets rank 0 if it sits at position 0
//   5 jump     R rounds of pointer doubling: in round k a ranked candidate i ranks next[i] with rank[i] + 2^k, and next
//              becomes next o next (ping-pong).  After round k the ranked ones are the first 2^(k+1) of the chain from
//              position 0; R is fixed by the image size (the chain has n / 26 + 1 links at most).  A candidate inside a
//              compressed body is never ranked: nothing on the chain leads to it.
//   6 gather   a ranked candidate is member `rank`: its table entry; the one whose successor is no candidate ends the
//              chain: at the image's end, or with the framing error of what lies there
//   7 scan     one workgroup: exclusive 64-bit sum of ISIZE, the counts, the lowest framing-level error, the verdict on
//              the capacity
//   8 inflate  one wavefront per member on a fixed persistent grid: ski_inflate_member (sk_inflate_block.h) straight
//              into the member's span of `out`, its verdict to the table and, by atomicMin, to the error word
//   9 written  one lane: the word sk_bgzf_inflate_output_words hands out.  A launch of its own, because any workgroup
//              of 8 may be the last to lower the error word and none of them knows that it is
// Count-only calls (out == NULL) stop behind 7, which has cleared the written word.
// The workspace (caller's, device) holds the header, the tile counts, the candidate arrays and the table: sk_device.h.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_inflate_block.h"

#define SI_THREADS 256
#define SI_NIL 0xffffffffu

static_assert(SK_GZ_HEADER == SKI_HEADER && SK_GZ_TRUNCATED == SKI_TRUNCATED && SK_GZ_DEFLATE == SKI_DEFLATE &&
                  SK_GZ_LENGTH == SKI_LENGTH && SK_GZ_CRC == SKI_CRC && SK_INFLATE_MIN_MEMBER == SKI_MIN_MEMBER,
              "the reasons of the C ABI are those of sk_inflate_block.h");

struct si_args {
    const uint8_t *image;
    uint64_t n;
    uint8_t *out;
    uint64_t capacity;
    uint64_t *hdr;
    uint32_t *tiles, *next_a, *next_b, *rank;
    uint64_t *cand;
    sk_inflate_entry *table;
    uint64_t cand_cap, table_cap, n_tiles;
};

// exclusive prefix sum of v over the workgroup, total = the sum.  lds: SI_THREADS / 64 words.
__device__ __forceinline__ uint64_t si_block_scan(uint64_t v, uint64_t &total, uint64_t *lds)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    uint64_t base = 0, tot = 0;
#pragma unroll
    for (int ww = 0; ww < SI_THREADS / 64; ++ww) {
        const uint64_t x = lds[ww];
        base += ww < w ? x : 0;
        tot += x;
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// bit k: a candidate begins at base + k, k = 0..15.  Reads image[base, min(n, base + 19)) only.
__device__ __forceinline__ uint32_t si_matches(const uint8_t *image, uint64_t n, uint64_t base)
{
    if (base >= n) return 0;
    uint8_t b[19];
#pragma unroll
    for (int k = 0; k < 19; ++k) b[k] = base + k < n ? image[base + k] : 0;
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (base + k + 4 <= n && b[k] == 0x1f && b[k + 1] == 0x8b && b[k + 2] == 8 && b[k + 3] == 4) m |= 1u << k;
    return m;
}

__global__ void __launch_bounds__(SI_THREADS) sk_inflate_count_kernel(si_args a)
{
    __shared__ uint32_t sum;
    for (uint64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        if (threadIdx.x == 0) sum = 0;
        __syncthreads();
        const uint32_t c = __popc(si_matches(a.image, a.n, t * SK_INFLATE_TILE + 16u * threadIdx.x));
        if (c) atomicAdd(&sum, c);
        __syncthreads();
        if (threadIdx.x == 0) a.tiles[t] = sum;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(SI_THREADS) sk_inflate_tiles_kernel(si_args a)
{
    __shared__ uint64_t lds[SI_THREADS / 64];
    uint64_t run = 0;
    for (uint64_t t0 = 0; t0 < a.n_tiles; t0 += SI_THREADS) {
        const uint64_t t = t0 + threadIdx.x;
        uint64_t tot;
        const uint64_t ex = si_block_scan(t < a.n_tiles ? a.tiles[t] : 0, tot, lds);
        if (t < a.n_tiles) a.tiles[t] = (uint32_t)(run + ex);
        run += tot;
    }
    if (threadIdx.x == 0) {
        a.hdr[SK_INFLATE_H_BYTES_IN] = a.n;
        a.hdr[SK_INFLATE_H_CANDIDATES] = run < a.cand_cap ? run : a.cand_cap; // run <= n / 4: matches do not overlap
        a.hdr[SK_INFLATE_H_MEMBERS] = 0;
        a.hdr[SK_INFLATE_H_FRAME_KEY] = ~0ull;
        a.hdr[SK_INFLATE_H_FRAME_OFFSET] = 0;
    }
}

__global__ void __launch_bounds__(SI_THREADS) sk_inflate_list_kernel(si_args a)
{
    __shared__ uint64_t lds[SI_THREADS / 64];
    for (uint64_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const uint64_t base = t * SK_INFLATE_TILE + 16u * threadIdx.x;
        uint32_t m = si_matches(a.image, a.n, base);
        uint64_t tot;
        uint64_t at = a.tiles[t] + si_block_scan(__popc(m), tot, lds);
        while (m) {
            const int k = __ffs(m) - 1;
            m &= m - 1;
            if (at < a.cand_cap) a.cand[at] = base + k;
            ++at;
        }
    }
}

// the candidate at position s, or SI_NIL
__device__ __forceinline__ uint32_t si_find(const uint64_t *cand, uint32_t nc, uint64_t s)
{
    uint32_t lo = 0, hi = nc;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cand[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    return lo < nc && cand[lo] == s ? lo : SI_NIL;
}

__global__ void __launch_bounds__(SI_THREADS) sk_inflate_parse_kernel(si_args a)
{
    const uint32_t nc = (uint32_t)a.hdr[SK_INFLATE_H_CANDIDATES];
    for (uint64_t i = (uint64_t)blockIdx.x * SI_THREADS + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * SI_THREADS) {
        const uint64_t pos = a.cand[i];
        ski_member m;
        uint32_t nx = SI_NIL;
        if (ski_parse_member(a.image, a.n, pos, &m) == SKI_OK && pos + m.size < a.n) nx = si_find(a.cand, nc, pos + m.size);
        a.next_a[i] = nx;
        a.rank[i] = pos == 0 ? 0u : SI_NIL;
    }
}

__global__ void __launch_bounds__(SI_THREADS) sk_inflate_jump_kernel(si_args a, uint32_t step, const uint32_t *from, uint32_t *to)
{
    const uint32_t nc = (uint32_t)a.hdr[SK_INFLATE_H_CANDIDATES];
    for (uint64_t i = (uint64_t)blockIdx.x * SI_THREADS + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * SI_THREADS) {
        const uint32_t p = from[i], r = a.rank[i];
        // a candidate ranked earlier in this very round may or may not be seen as ranked here: what it would write is
        // the true rank of its target either way, and the rounds to come cover that target regardless
        if (p < nc && r != SI_NIL) a.rank[p] = r + step;
        to[i] = p < nc ? from[p] : SI_NIL;
    }
}

__device__ __forceinline__ void si_frame_end(const si_args &a, uint64_t members, uint64_t pos)
{
    a.hdr[SK_INFLATE_H_MEMBERS] = members;
    if (pos >= a.n) return; // the chain ends with the image
    ski_member m;
    uint32_t why = ski_parse_member(a.image, a.n, pos, &m);
    if (why == SKI_OK) why = SKI_HEADER; // unreachable: a position that parses is a candidate
    a.hdr[SK_INFLATE_H_FRAME_KEY] = (members << 3) | why;
    a.hdr[SK_INFLATE_H_FRAME_OFFSET] = pos;
}

__global__ void __launch_bounds__(SI_THREADS) sk_inflate_gather_kernel(si_args a)
{
    const uint32_t nc = (uint32_t)a.hdr[SK_INFLATE_H_CANDIDATES];
    if (blockIdx.x == 0 && threadIdx.x == 0 && (nc == 0 || a.cand[0] != 0)) si_frame_end(a, 0, 0); // no chain at all
    for (uint64_t i = (uint64_t)blockIdx.x * SI_THREADS + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * SI_THREADS) {
        const uint64_t r = a.rank[i];
        if (r == SI_NIL) continue;
        const uint64_t pos = a.cand[i];
        ski_member m;
        if (ski_parse_member(a.image, a.n, pos, &m) != SKI_OK || r >= a.table_cap) {
            si_frame_end(a, r, pos);
            continue;
        }
        sk_inflate_entry e;
        e.image_off = pos;
        e.out_off = 0;
        e.body_off = m.body_off;
        e.body_len = m.body_len;
        e.isize = m.isize;
        e.crc = m.crc;
        e.verdict = m.isize > SKI_MAX_ISIZE ? SKI_LENGTH : SKI_OK;
        e.reserved = 0;
        a.table[r] = e;
        const uint64_t s = pos + m.size;
        if (s >= a.n || si_find(a.cand, nc, s) == SI_NIL) si_frame_end(a, r + 1, s);
    }
}

__global__ void __launch_bounds__(SI_THREADS) sk_inflate_scan_kernel(si_args a)
{
    __shared__ uint64_t lds[SI_THREADS / 64];
    __shared__ unsigned long long worst;
    const uint64_t nm = a.hdr[SK_INFLATE_H_MEMBERS];
    if (threadIdx.x == 0) worst = a.hdr[SK_INFLATE_H_FRAME_KEY];
    __syncthreads();
    uint64_t run = 0;
    for (uint64_t m0 = 0; m0 < nm; m0 += SI_THREADS) {
        const uint64_t m = m0 + threadIdx.x;
        uint64_t v = 0, tot;
        if (m < nm) {
            if (a.table[m].verdict == SKI_OK) v = a.table[m].isize;
            else atomicMin(&worst, (unsigned long long)((m << 3) | a.table[m].verdict));
        }
        const uint64_t ex = si_block_scan(v, tot, lds);
        if (m < nm) a.table[m].out_off = run + ex;
        run += tot;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.hdr[SK_INFLATE_H_BYTES_OUT] = run;
        a.hdr[SK_INFLATE_H_FIT] = a.out == nullptr || run <= a.capacity;
        a.hdr[SK_INFLATE_H_ERROR_KEY] = worst;
        a.hdr[SK_INFLATE_H_WRITTEN] = 0;
    }
}

__global__ void __launch_bounds__(SKI_LANES) sk_inflate_member_kernel(si_args a)
{
    __shared__ ski_shared sh;
    __shared__ skb_shared cs;
    if (!a.hdr[SK_INFLATE_H_FIT]) return; // uniform: a text beyond the capacity leaves `out` untouched
    const int lane = (int)threadIdx.x;
    const uint64_t nm = a.hdr[SK_INFLATE_H_MEMBERS];
    skb_phase_crc_tables(&cs, lane);
    ski_fixed_lengths(&sh, lane);
    __syncthreads();
    {
        const ski_build lit = ski_build_lit(&sh.fixed, 288);
        SKI_BUILD(&sh, lit);
        const ski_build dist = ski_build_dist(&sh.fixed, 288, 32);
        SKI_BUILD(&sh, dist);
    }
    for (uint64_t m = blockIdx.x; m < nm; m += gridDim.x) {
        const sk_inflate_entry e = a.table[m];
        if (e.verdict != SKI_OK) continue; // an ISIZE no member can have: the scan has reported it
        const uint32_t why = ski_inflate_member(&sh, &cs, a.image + e.image_off + e.body_off, e.body_len, a.out + e.out_off,
                                                e.isize, e.crc, lane);
        if (why != SKI_OK && lane == 0) {
            a.table[m].verdict = why;
            atomicMin(reinterpret_cast<unsigned long long *>(a.hdr + SK_INFLATE_H_ERROR_KEY), (unsigned long long)((m << 3) | why));
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64) sk_inflate_written_kernel(si_args a)
{
    if (threadIdx.x == 0) a.hdr[SK_INFLATE_H_WRITTEN] = a.hdr[SK_INFLATE_H_FIT] && a.hdr[SK_INFLATE_H_ERROR_KEY] == ~0ull;
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_bgzf_inflate(const uint8_t *image, uint64_t image_bytes,
                                                                                   uint8_t *out, uint64_t capacity,
                                                                                   void *workspace, hipStream_t stream)
{
    sk_inflate_layout L;
    sk_inflate_layout_of(image_bytes, &L);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    si_args a;
    a.image = image;
    a.n = image_bytes;
    a.out = out;
    a.capacity = capacity;
    a.hdr = reinterpret_cast<uint64_t *>(ws);
    a.tiles = reinterpret_cast<uint32_t *>(ws + L.tiles);
    a.cand = reinterpret_cast<uint64_t *>(ws + L.cand);
    a.next_a = reinterpret_cast<uint32_t *>(ws + L.next_a);
    a.next_b = reinterpret_cast<uint32_t *>(ws + L.next_b);
    a.rank = reinterpret_cast<uint32_t *>(ws + L.rank);
    a.table = reinterpret_cast<sk_inflate_entry *>(ws + L.table);
    a.cand_cap = L.n_cand;
    a.table_cap = L.n_table;
    a.n_tiles = L.n_tiles;
    const unsigned tile_grid = (unsigned)(L.n_tiles < SK_INFLATE_FRAME_GRID ? L.n_tiles : SK_INFLATE_FRAME_GRID);
    const uint64_t cand_wgs = (L.n_cand + SI_THREADS - 1) / SI_THREADS;
    const unsigned cand_grid = (unsigned)(cand_wgs < SK_INFLATE_FRAME_GRID ? cand_wgs : SK_INFLATE_FRAME_GRID);
    hipLaunchKernelGGL(sk_inflate_count_kernel, dim3(tile_grid), dim3(SI_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_inflate_tiles_kernel, dim3(1), dim3(SI_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_inflate_list_kernel, dim3(tile_grid), dim3(SI_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_inflate_parse_kernel, dim3(cand_grid), dim3(SI_THREADS), 0, stream, a);
    uint32_t *from = a.next_a, *to = a.next_b;
    for (uint32_t k = 0; k < L.rounds; ++k) {
        hipLaunchKernelGGL(sk_inflate_jump_kernel, dim3(cand_grid), dim3(SI_THREADS), 0, stream, a, 1u << k, from, to);
        uint32_t *t = from;
        from = to;
        to = t;
    }
    hipLaunchKernelGGL(sk_inflate_gather_kernel, dim3(cand_grid), dim3(SI_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_inflate_scan_kernel, dim3(1), dim3(SI_THREADS), 0, stream, a);
    if (out) {
        const unsigned grid = (unsigned)(L.n_table < SK_INFLATE_GRID ? L.n_table : SK_INFLATE_GRID);
        hipLaunchKernelGGL(sk_inflate_member_kernel, dim3(grid), dim3(SKI_LANES), 0, stream, a);
        hipLaunchKernelGGL(sk_inflate_written_kernel, dim3(1), dim3(64), 0, stream, a);
    }
    return hipGetLastError();
}
