// sk_gunzip.hip -- plain gzip read on the device (sk_gzip_inflate_device_async): a gzip byte image in device memory -> its
// text in device memory, every member's CRC-32 and ISIZE checked.  The stages are the functions of sk_gunzip_block.h.
//
// Launches on one stream, no inter-workgroup waiting:
//   1 search   one wavefront per chunk: the guessed block start; chunk 0: the header words, member 0's gzip header
//   2 count    one wavefront per guessed start: lengths only, to the boundary that is a later guess
//   3 chain    one lane: the stretches the chain from bit 0 goes through, their text offsets, the counts, the verdict on
//              the capacity, the failure that stopped the chain
//   4 decode   one wavefront per used stretch: 16-bit symbols at its text offset, the member table
//   5 windows  one workgroup, used stretch after used stretch: the last 32 Ki symbols of each made literal
//   6 resolve  the grid: symbols -> bytes of `out`, 16 per lane
//   7 crc      one wavefront per 32 KiB piece of `out`: its spans' CRC terms, XORed into their members
//   8 check    one lane per member: ISIZE, CRC-32
//   9 final    one lane: the offset of the lowest failure, and the word sk_gzip_inflate_output_words hands out
// Count-only calls (out == NULL) stop behind 3.  The workspace is the caller's: sk_device.h.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_gunzip_block.h"

#define SG_THREADS 256
#define SG_WINDOW_THREADS 1024

static_assert(sizeof(skg_stretch) == SK_GUNZIP_STRETCH_BYTES && sizeof(skg_member) == SK_GUNZIP_MEMBER_BYTES &&
                  SKG_HDR_WORDS == SK_GUNZIP_HDR_WORDS && SKG_MIN_GAP == 18 && SKG_H_BYTES_OUT == SK_GUNZIP_H_BYTES_OUT &&
                  SKG_H_WRITTEN == SK_GUNZIP_H_WRITTEN,
              "the workspace sections of sk_device.h are those of sk_gunzip_block.h");

// the fixed code's tables, once per workgroup
__device__ __forceinline__ void sg_fixed_tables(ski_shared *sh, int lane)
{
    ski_fixed_lengths(sh, lane);
    __syncthreads();
    const ski_build lit = ski_build_lit(&sh->fixed, 288);
    SKI_BUILD(sh, lit);
    const ski_build dist = ski_build_dist(&sh->fixed, 288, 32);
    SKI_BUILD(sh, dist);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_search_kernel(skg_args a)
{
    __shared__ ski_shared sh;
    const int lane = (int)threadIdx.x;
    if (blockIdx.x == 0 && lane == 0) skg_search_first(a);
    sg_fixed_tables(&sh, lane);
    for (uint64_t c = blockIdx.x; c < a.S; c += gridDim.x)
        if (c) skg_search_chunk(&sh, a, c, lane);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_count_kernel(skg_args a)
{
    __shared__ ski_shared sh;
    __shared__ skg_walk w; // every lane writes the same values
    const int lane = (int)threadIdx.x;
    sg_fixed_tables(&sh, lane);
    for (uint64_t k = blockIdx.x; k < a.S; k += gridDim.x)
        if (a.st[k].start != SKG_NONE) skg_count_stretch(&sh, &w, a, k, lane); // uniform
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_chain_kernel(skg_args a)
{
    if (threadIdx.x == 0) skg_chain(a);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_decode_kernel(skg_args a)
{
    __shared__ ski_shared sh;
    __shared__ skg_walk w;
    if (!a.hdr[SKG_H_FIT]) return; // uniform: a text beyond the capacity leaves `out` and the symbols untouched
    const int lane = (int)threadIdx.x;
    sg_fixed_tables(&sh, lane);
    // the grid stride waits in vector registers: the walk's uniform state fills the scalar ones
    uint64_t next = blockIdx.x;
    uint32_t step = gridDim.x;
    SKG_PER_LANE(step);
    for (;;) {
        SKG_PER_LANE(next);
        const uint64_t u = skg_uniform(next);
        if (u >= a.hdr[SKG_H_USED]) break;
        skg_decode_stretch(&sh, &w, a, u, lane);
        next += step;
    }
}

__global__ void __launch_bounds__(SG_WINDOW_THREADS) sk_gunzip_windows_kernel(skg_args a)
{
    if (!a.hdr[SKG_H_FIT]) return;
    const uint64_t used = a.hdr[SKG_H_USED];
    for (uint64_t u = 1; u < used; ++u) {
        for (uint32_t i = threadIdx.x; i < SKG_WINDOW; i += SG_WINDOW_THREADS) skg_window_elem(a, u, i);
        __syncthreads(); // what this step made literal is the next step's window
    }
}

__global__ void __launch_bounds__(SG_THREADS) sk_gunzip_resolve_kernel(skg_args a)
{
    if (!a.hdr[SKG_H_FIT]) return;
    const uint64_t granules = (a.hdr[SKG_H_BYTES_OUT] + 15) / 16;
    for (uint64_t g = (uint64_t)blockIdx.x * SG_THREADS + threadIdx.x; g < granules; g += (uint64_t)gridDim.x * SG_THREADS)
        skg_resolve_granule(a, g);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_crc_kernel(skg_args a)
{
    __shared__ skg_crc_shared cs;
    if (!a.hdr[SKG_H_FIT]) return;
    const int lane = (int)threadIdx.x;
    skg_crc_tables(&cs, lane);
    __syncthreads();
    const uint64_t pieces = (a.hdr[SKG_H_BYTES_OUT] + SKG_PIECE - 1) / SKG_PIECE;
    for (uint64_t q = blockIdx.x; q < pieces; q += gridDim.x) skg_crc_piece(&cs, a, q, lane);
}

__global__ void __launch_bounds__(SG_THREADS) sk_gunzip_check_kernel(skg_args a)
{
    __shared__ uint32_t power[SKG_POWERS];
    if (!a.hdr[SKG_H_FIT]) return;
    if (threadIdx.x < SKG_POWERS) {
        uint32_t e = 0x00800000u;
        for (uint32_t j = 0; j < threadIdx.x; ++j) e = skb_mul(e, e);
        power[threadIdx.x] = e;
    }
    __syncthreads();
    const uint64_t members = a.hdr[SKG_H_MEMBERS];
    for (uint64_t m = (uint64_t)blockIdx.x * SG_THREADS + threadIdx.x; m < members; m += (uint64_t)gridDim.x * SG_THREADS)
        skg_check_member(power, a, m);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_final_kernel(skg_args a)
{
    if (threadIdx.x == 0 && a.hdr[SKG_H_FIT]) skg_final(a);
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_gunzip(const uint8_t *image, uint64_t image_bytes, uint8_t *out,
                                                                             uint64_t capacity, uint64_t forced_chunk,
                                                                             void *workspace, hipStream_t stream)
{
    sk_gunzip_layout L;
    sk_gunzip_layout_of(image_bytes, capacity, forced_chunk, &L);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    skg_args a;
    a.image = image;
    a.n = image_bytes;
    a.out = out;
    a.capacity = capacity;
    a.hdr = reinterpret_cast<uint64_t *>(ws);
    a.st = reinterpret_cast<skg_stretch *>(ws + L.stretches);
    a.u_off = reinterpret_cast<uint64_t *>(ws + L.u_off);
    a.u_id = reinterpret_cast<uint32_t *>(ws + L.u_id);
    a.mem = reinterpret_cast<skg_member *>(ws + L.members);
    a.sym = reinterpret_cast<uint16_t *>(ws + L.sym);
    a.S = L.S;
    a.chunk_bits = L.chunk * 8;
    a.chunk_shift = (uint32_t)__builtin_ctzll(a.chunk_bits);
    a.pad = 0;
    a.mem_cap = L.n_members;
    const auto grid_of = [](uint64_t units, uint64_t cap) { return dim3((unsigned)(units < 1 ? 1 : units < cap ? units : cap)); };
    const dim3 waves = grid_of(L.S, SK_GUNZIP_GRID);
    hipLaunchKernelGGL(sk_gunzip_search_kernel, waves, dim3(SKI_LANES), 0, stream, a);
    hipLaunchKernelGGL(sk_gunzip_count_kernel, waves, dim3(SKI_LANES), 0, stream, a);
    hipLaunchKernelGGL(sk_gunzip_chain_kernel, dim3(1), dim3(SKI_LANES), 0, stream, a);
    if (out) {
        hipLaunchKernelGGL(sk_gunzip_decode_kernel, waves, dim3(SKI_LANES), 0, stream, a);
        hipLaunchKernelGGL(sk_gunzip_windows_kernel, dim3(1), dim3(SG_WINDOW_THREADS), 0, stream, a);
        hipLaunchKernelGGL(sk_gunzip_resolve_kernel, grid_of((capacity / 16 + SG_THREADS) / SG_THREADS, 2048), dim3(SG_THREADS), 0,
                           stream, a);
        hipLaunchKernelGGL(sk_gunzip_crc_kernel, grid_of(capacity / SKG_PIECE + 1, SK_GUNZIP_GRID), dim3(SKI_LANES), 0, stream, a);
        hipLaunchKernelGGL(sk_gunzip_check_kernel, grid_of(L.n_members / SG_THREADS + 1, 1024), dim3(SG_THREADS), 0, stream, a);
        hipLaunchKernelGGL(sk_gunzip_final_kernel, dim3(1), dim3(SKI_LANES), 0, stream, a);
    }
    return hipGetLastError();
}
