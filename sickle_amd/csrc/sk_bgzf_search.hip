// sk_bgzf_search.hip -- the block kernel of the device's BGZF writer with SK_BGZF_SEARCH: sk_bgzf_block_kernel
// (sk_bgzf.hip) with the candidate phases of sk_bgzf_search.h in front of its tokenizer and that header's tokenizer in
// place of skd_phase_tokenize.  Everything behind the tokens, and the scan and pack kernels, are shared as they stand.
// One wavefront per block, a persistent grid; the hash table (16 KiB) lies in LDS next to the encoder's state.
#include <hip/hip_runtime.h>

#include "sk_bgzf_args.h"
#include "sk_bgzf_block.h"
#include "sk_bgzf_search.h"

static_assert(sizeof(skd_shared) + sizeof(skb_shared) + sizeof(sks_shared) <= 65536, "the static LDS limit");
static_assert(SK_BGZF_BLOCK < 65536, "a position + 1 fits 16 bits");
static_assert(SKS_WAYS % 2 == 0 && SKS_CHUNK % SKD_LANES == 0, "two ways to a word; whole rounds of the lanes to a chunk");

// cand_all: one word per text byte of the block in flight, per workgroup (SK_BGZF_TOK_WORDS words each)
__global__ void __launch_bounds__(SKD_LANES) sk_bgzf_search_block_kernel(bz_args a, uint32_t *cand_all)
{
    __shared__ skd_shared sh;
    __shared__ skb_shared cs;
    __shared__ sks_shared ss;
    const int lane = (int)threadIdx.x;
    const uint64_t total = bz_length(a), nb = bz_blocks(total);
    uint32_t *tok = a.tokens + (size_t)blockIdx.x * SK_BGZF_TOK_WORDS;
    uint32_t *cand = cand_all + (size_t)blockIdx.x * SK_BGZF_TOK_WORDS;
    skb_phase_crc_tables(&cs, lane);
    __syncthreads();
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint8_t *p = a.text + b * SK_BGZF_BLOCK;
        const uint32_t n = (uint32_t)min((uint64_t)SK_BGZF_BLOCK, total - b * SK_BGZF_BLOCK); // >= 1
        uint32_t *out = a.slots + b * SKD_OUT_WORDS;
        skd_phase_clear(&sh, out, lane);
        sks_phase_clear(&ss, lane);
        skd_phase_count_newlines(&sh, p, n, lane);
        __syncthreads();
        if (lane == 0) skd_phase_scan_segments(&sh, n);
        __syncthreads();
        skd_phase_line_starts(&sh, p, n, lane);
        __syncthreads();
        if (lane == 0) skd_phase_close_lines(&sh, p, n);
        __syncthreads();
        for (uint32_t c = 0; c * SKS_CHUNK < n; ++c) { // n is uniform: every lane meets every barrier
            sks_phase_candidates(&sh, &ss, p, n, c, cand, lane);
            __syncthreads();
            sks_phase_insert(&ss, p, n, c, lane);
            __syncthreads();
        }
        sks_phase_tokenize(&sh, p, cand, tok, lane); // a lane reads candidates other lanes wrote: the barrier above
        __syncthreads();
        if (lane == 0) skd_phase_codes_and_header(&sh, out);
        skb_phase_crc_lanes(&cs, p, n, lane);
        __syncthreads();
        skd_phase_size_lines(&sh, tok, lane);
        __syncthreads();
        if (lane == 0) skd_phase_place_lines(&sh, out);
        __syncthreads();
        skd_phase_emit(&sh, tok, out, lane);
        __syncthreads();
        if (lane == 0) {
            skb_phase_crc_close(&cs, n);
            const uint32_t clen = skb_stream_bytes(sh.total_bits);
            sk_bgzf_entry e;
            e.body = skb_body_bytes(clen, n) | (skb_is_stored(clen, n) ? SKB_STORED_FLAG : 0u);
            e.crc = cs.crc;
            e.off = 0;
            a.table[b] = e;
        }
        __syncthreads();
    }
}

extern "C" __attribute__((visibility("hidden"))) void sk_launch_bgzf_search_block(const bz_args *a, uint32_t *cand, unsigned grid,
                                                                                 hipStream_t stream)
{
    hipLaunchKernelGGL(sk_bgzf_search_block_kernel, dim3(grid), dim3(SKD_LANES), 0, stream, *a, cand);
}
