// sk_gunzip_piece.hip -- plain gzip read on the device in pieces (sk_gzip_inflate_piece_device_async): the reader of
// sk_gunzip.hip, started at a device-resident state (a block boundary or a member start, the 32 KiB of text before it, the
// open member's CRC-32 and length) and publishing the next one.  The stages are those of sk_gunzip_block.h, run on the
// window the state and the piece define; what a piece changes in them is said there ("Pieces").
//
// Launches on one stream, no inter-workgroup waiting.  Every workgroup derives the window from the state once:
//    1 search   as sk_gunzip.hip; chunk 0: the header words, stretch 0's start from the state; the grid also writes the
//               state's history as the literals in front of the symbols
//    2 count    lengths only, and each stretch's last resume point
//    3 chain    one lane: from the state's position; cut at a deferred failure or at the capacity, with a stop bit
//    4 decode   honours the stop bit
//    5 windows  from used stretch 0 on: the history is its window
//    6 resolve  symbols -> bytes of `out`
//    7 crc      the open member at the end has an entry too
//    8 check    member 0 continues the state's CRC-32 and length
//    9 final
//   10 state    one workgroup: the next history, then the next state and the words finish and the next calls read
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_gunzip_block.h"

#define SG_THREADS 256
#define SG_WINDOW_THREADS 1024

static_assert(sizeof(skg_piece_state) == SK_GZIP_PIECE_STATE_BYTES && sizeof(skg_piece_state) == sizeof(sk_gzip_piece_state) &&
                  sizeof(skg_resume) == SK_GUNZIP_RESUME_BYTES && SKG_WINDOW == SK_GUNZIP_PIECE_SHIFT &&
                  SKG_H_P_LIMITED == SK_GUNZIP_H_P_LIMITED && SKG_H_P_DONE == SK_GUNZIP_H_P_DONE &&
                  SKG_H_P_STATUS == SK_GUNZIP_H_P_STATUS && SKG_H_P_ERROR == SK_GUNZIP_H_P_ERROR &&
                  SKG_H_P_ERROR_MEMBER == SK_GUNZIP_H_P_ERROR_MEMBER && SKG_H_P_ERROR_OFFSET == SK_GUNZIP_H_P_ERROR_OFFSET &&
                  SKG_H_P_INHERITED == SK_GUNZIP_H_P_INHERITED && SKG_H_P_POS_BIT == SK_GUNZIP_H_P_POS_BIT &&
                  SKG_H_P_IN_MEMBER == SK_GUNZIP_H_P_IN_MEMBER && SKG_H_P_IMAGE_OFFSET == SK_GUNZIP_H_P_IMAGE_OFFSET,
              "the piece's state and workspace sections are those of sk_gunzip_block.h");

__device__ __forceinline__ void sgp_fixed_tables(ski_shared *sh, int lane)
{
    ski_fixed_lengths(sh, lane);
    __syncthreads();
    const ski_build lit = ski_build_lit(&sh->fixed, 288);
    SKI_BUILD(sh, lit);
    const ski_build dist = ski_build_dist(&sh->fixed, 288, 32);
    SKI_BUILD(sh, dist);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_piece_search_kernel(skg_args a, skg_piece_args p)
{
    __shared__ ski_shared sh;
    const int lane = (int)threadIdx.x;
    bool closing;
    const uint32_t kind = skg_piece_window(p, &a, &closing);
    if (blockIdx.x == 0 && lane == 0) skg_piece_first(a, p, kind, closing);
    if (kind != SKG_P_RUN) return; // uniform
    for (uint32_t i = blockIdx.x * SKI_LANES + threadIdx.x; i < SKG_WINDOW; i += gridDim.x * SKI_LANES) a.sym[i] = p.in->history[i];
    sgp_fixed_tables(&sh, lane);
    for (uint64_t c = blockIdx.x; c < a.S; c += gridDim.x)
        if (c) skg_search_chunk(&sh, a, c, lane);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_piece_count_kernel(skg_args a, skg_piece_args p)
{
    __shared__ ski_shared sh;
    __shared__ skg_walk w;
    __shared__ skg_piece_walk pw;
    const int lane = (int)threadIdx.x;
    bool closing;
    if (skg_piece_window(p, &a, &closing) != SKG_P_RUN) return;
    sgp_fixed_tables(&sh, lane);
    for (uint64_t k = blockIdx.x; k < a.S; k += gridDim.x)
        if (a.st[k].start != SKG_NONE) skg_count_stretch_piece(&sh, &w, &pw, a, p, k, lane);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_piece_chain_kernel(skg_args a, skg_piece_args p)
{
    bool closing;
    if (skg_piece_window(p, &a, &closing) != SKG_P_RUN) return;
    if (threadIdx.x == 0) skg_chain_piece(a, p, closing);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_piece_decode_kernel(skg_args a, skg_piece_args p)
{
    __shared__ ski_shared sh;
    __shared__ skg_walk w;
    __shared__ skg_piece_walk pw;
    bool closing;
    if (skg_piece_window(p, &a, &closing) != SKG_P_RUN || !a.hdr[SKG_H_FIT]) return;
    const int lane = (int)threadIdx.x;
    sgp_fixed_tables(&sh, lane);
    uint64_t next = blockIdx.x;
    uint32_t step = gridDim.x;
    SKG_PER_LANE(step);
    for (;;) {
        SKG_PER_LANE(next);
        const uint64_t u = skg_uniform(next);
        if (u >= a.hdr[SKG_H_USED]) break;
        skg_decode_stretch_piece(&sh, &w, &pw, a, p, u, lane);
        next += step;
    }
}

// the stages behind the decode read no image: the window is not derived again, the header says what the call is
__global__ void __launch_bounds__(SG_WINDOW_THREADS) sk_gunzip_piece_windows_kernel(skg_args a)
{
    if (a.hdr[SKG_H_P_KIND] != SKG_P_RUN || !a.hdr[SKG_H_FIT]) return;
    const uint64_t used = a.hdr[SKG_H_USED];
    for (uint64_t u = 0; u < used; ++u) {
        for (uint32_t i = threadIdx.x; i < SKG_WINDOW; i += SG_WINDOW_THREADS) skg_window_elem(a, u, i);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(SG_THREADS) sk_gunzip_piece_resolve_kernel(skg_args a)
{
    if (a.hdr[SKG_H_P_KIND] != SKG_P_RUN || !a.hdr[SKG_H_FIT]) return;
    const uint64_t granules = (a.hdr[SKG_H_BYTES_OUT] + 15) / 16;
    for (uint64_t g = SKG_WINDOW / 16 + (uint64_t)blockIdx.x * SG_THREADS + threadIdx.x; g < granules; g += (uint64_t)gridDim.x * SG_THREADS)
        skg_resolve_granule(a, g);
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_piece_crc_kernel(skg_args a)
{
    __shared__ skg_crc_shared cs;
    if (a.hdr[SKG_H_P_KIND] != SKG_P_RUN || !a.hdr[SKG_H_FIT]) return;
    const int lane = (int)threadIdx.x;
    skg_crc_tables(&cs, lane);
    __syncthreads();
    const uint64_t pieces = (a.hdr[SKG_H_BYTES_OUT] + SKG_PIECE - 1) / SKG_PIECE;
    for (uint64_t q = SKG_WINDOW / SKG_PIECE + blockIdx.x; q < pieces; q += gridDim.x) skg_crc_piece(&cs, a, q, lane);
}

__device__ __forceinline__ void sgp_powers(uint32_t *power)
{
    if (threadIdx.x < SKG_POWERS) {
        uint32_t e = 0x00800000u;
        for (uint32_t j = 0; j < threadIdx.x; ++j) e = skb_mul(e, e);
        power[threadIdx.x] = e;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(SG_THREADS) sk_gunzip_piece_check_kernel(skg_args a, skg_piece_args p)
{
    __shared__ uint32_t power[SKG_POWERS];
    if (a.hdr[SKG_H_P_KIND] != SKG_P_RUN || !a.hdr[SKG_H_FIT]) return;
    sgp_powers(power);
    const uint64_t members = a.hdr[SKG_H_MEMBERS] - 1; // the last entry is the open member's
    for (uint64_t m = (uint64_t)blockIdx.x * SG_THREADS + threadIdx.x; m < members; m += (uint64_t)gridDim.x * SG_THREADS) {
        if (m) skg_check_member(power, a, m);
        else skg_check_first_piece(power, a, p);
    }
}

__global__ void __launch_bounds__(SKI_LANES) sk_gunzip_piece_final_kernel(skg_args a)
{
    if (threadIdx.x == 0 && a.hdr[SKG_H_P_KIND] == SKG_P_RUN && a.hdr[SKG_H_FIT]) skg_final(a);
}

__global__ void __launch_bounds__(SG_WINDOW_THREADS) sk_gunzip_piece_state_kernel(skg_args a, skg_piece_args p)
{
    __shared__ uint32_t power[SKG_POWERS];
    sgp_powers(power);
    for (uint32_t i = threadIdx.x; i < SKG_WINDOW; i += SG_WINDOW_THREADS) skg_piece_history(a, p, i);
    __syncthreads(); // the history reads the header words that the next step rewrites
    if (threadIdx.x == 0) skg_piece_publish(a, p, power);
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_gunzip_piece(const uint8_t *image, uint64_t image_bytes,
                                                                                   const sk_gzip_piece *piece, const void *state_in,
                                                                                   void *state_out, uint8_t *out, uint64_t capacity,
                                                                                   uint64_t forced_chunk, void *workspace,
                                                                                   hipStream_t stream)
{
    sk_gunzip_piece_layout L;
    sk_gunzip_piece_layout_of(piece->window_bytes, capacity, forced_chunk, &L);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    skg_args a;
    a.image = nullptr; // the window's: every workgroup derives them from the state
    a.n = 0;
    a.out = out - SKG_WINDOW; // text offsets are shifted by the history in front of the symbols
    a.capacity = capacity;
    a.hdr = reinterpret_cast<uint64_t *>(ws);
    a.st = reinterpret_cast<skg_stretch *>(ws + L.g.stretches);
    a.u_off = reinterpret_cast<uint64_t *>(ws + L.g.u_off);
    a.u_id = reinterpret_cast<uint32_t *>(ws + L.g.u_id);
    a.mem = reinterpret_cast<skg_member *>(ws + L.g.members);
    a.sym = reinterpret_cast<uint16_t *>(ws + L.g.sym);
    a.S = L.g.S;
    a.chunk_bits = L.g.chunk * 8;
    a.chunk_shift = (uint32_t)__builtin_ctzll(a.chunk_bits);
    a.pad = 0;
    a.mem_cap = L.g.n_members;
    skg_piece_args p;
    p.in = static_cast<const skg_piece_state *>(state_in);
    p.out = static_cast<skg_piece_state *>(state_out);
    p.image = image;
    p.image_bytes = image_bytes;
    p.image_offset = piece->image_offset;
    p.window_bytes = piece->window_bytes;
    p.text = out;
    p.capacity = capacity;
    p.res = reinterpret_cast<skg_resume *>(ws + L.resume);
    p.last = piece->last;
    p.pad = 0;
    const auto grid_of = [](uint64_t units, uint64_t cap) { return dim3((unsigned)(units < 1 ? 1 : units < cap ? units : cap)); };
    const dim3 waves = grid_of(L.g.S, SK_GUNZIP_GRID);
    hipLaunchKernelGGL(sk_gunzip_piece_search_kernel, waves, dim3(SKI_LANES), 0, stream, a, p);
    hipLaunchKernelGGL(sk_gunzip_piece_count_kernel, waves, dim3(SKI_LANES), 0, stream, a, p);
    hipLaunchKernelGGL(sk_gunzip_piece_chain_kernel, dim3(1), dim3(SKI_LANES), 0, stream, a, p);
    hipLaunchKernelGGL(sk_gunzip_piece_decode_kernel, waves, dim3(SKI_LANES), 0, stream, a, p);
    hipLaunchKernelGGL(sk_gunzip_piece_windows_kernel, dim3(1), dim3(SG_WINDOW_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_gunzip_piece_resolve_kernel, grid_of((capacity / 16 + SG_THREADS) / SG_THREADS, 2048), dim3(SG_THREADS), 0,
                       stream, a);
    hipLaunchKernelGGL(sk_gunzip_piece_crc_kernel, grid_of(capacity / SKG_PIECE + 1, SK_GUNZIP_GRID), dim3(SKI_LANES), 0, stream, a);
    hipLaunchKernelGGL(sk_gunzip_piece_check_kernel, grid_of(L.g.n_members / SG_THREADS + 1, 1024), dim3(SG_THREADS), 0, stream, a, p);
    hipLaunchKernelGGL(sk_gunzip_piece_final_kernel, dim3(1), dim3(SKI_LANES), 0, stream, a);
    hipLaunchKernelGGL(sk_gunzip_piece_state_kernel, dim3(1), dim3(SG_WINDOW_THREADS), 0, stream, a, p);
    return hipGetLastError();
}
