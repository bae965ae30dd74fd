// sk_bgzf.hip -- BGZF on the device (sk_bgzf_device_async): text in device memory -> a complete .gz image in device memory.
//
// Three launches on one stream, no inter-workgroup waiting (workgroup dispatch order is undefined):
//   1 block   one wavefront per block of 65 280 text bytes, a persistent grid: the phases of sk_deflate_block.h into the
//             block's 64 KiB slot, the CRC-32 phases of sk_bgzf_block.h on the same text, then lane 0's verdict (deflate or
//             stored) and the block's table entry.  The text's length is read from the device, so the launch is sized by
//             its bound and blocks past the length do nothing.
//   2 scan    one workgroup: member sizes -> exclusive offsets, the counts, the capacity verdict
//   3 pack    a workgroup per member: header, body (from the slot, or straight from the text for a stored block) and
//             trailer to the member's offset.  The offsets have any byte alignment, so the body goes out as aligned 16-byte
//             stores built from aligned 16-byte loads funnel-shifted by v_alignbyte; the few granules at a member's ends,
//             which it shares with its neighbours, are written byte by byte.
// With SK_BGZF_SEARCH launch 1 is sk_bgzf_search_block_kernel instead (sk_bgzf_search.hip: a file of its own, so that the
// code of the kernel here does not depend on it): the same phases around the tokenizer of sk_bgzf_search.h, which also
// takes matches that a hash table in LDS finds.
// The workspace (caller's, device) holds the header, the table, the token scratch and the slots, and behind them the
// search's candidate scratch: sk_device.h.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_device_prims.h"
#include "sk_bgzf_args.h"
#include "sk_bgzf_block.h"

#define BZ_THREADS 256
#define BZ_PACK_WG_PER_CU 8u

static_assert(SK_BGZF_BLOCK == SKD_BLOCK_MAX && SK_BGZF_SLOT == 4 * SKD_OUT_WORDS && SK_BGZF_TOK_WORDS == SKD_BLOCK_MAX + 8,
              "the workspace layout follows sk_deflate_block.h");
static_assert(SK_BGZF_MEMBER_EXTRA == SKB_HEADER_BYTES + SKB_STORED_BYTES + SKB_TRAILER_BYTES && SK_BGZF_EOF_BYTES == SKB_EOF_BYTES,
              "sk_bgzf_bound follows sk_bgzf_block.h");

// ------------------------------------------------------------------------------------------
// 1 block: deflate, CRC-32, verdict
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SKD_LANES) sk_bgzf_block_kernel(bz_args a)
{
    __shared__ skd_shared sh;
    __shared__ skb_shared cs;
    const int lane = (int)threadIdx.x;
    const uint64_t total = bz_length(a), nb = bz_blocks(total);
    uint32_t *tok = a.tokens + (size_t)blockIdx.x * SK_BGZF_TOK_WORDS;
    skb_phase_crc_tables(&cs, lane);
    __syncthreads();
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint8_t *p = a.text + b * SK_BGZF_BLOCK;
        const uint32_t n = (uint32_t)min((uint64_t)SK_BGZF_BLOCK, total - b * SK_BGZF_BLOCK); // >= 1
        uint32_t *out = a.slots + b * SKD_OUT_WORDS;
        skd_phase_clear(&sh, out, lane);
        skd_phase_count_newlines(&sh, p, n, lane);
        __syncthreads();
        if (lane == 0) skd_phase_scan_segments(&sh, n);
        __syncthreads();
        skd_phase_line_starts(&sh, p, n, lane);
        __syncthreads();
        if (lane == 0) skd_phase_close_lines(&sh, p, n);
        __syncthreads();
        skd_phase_tokenize(&sh, p, tok, lane);
        __syncthreads();
        if (lane == 0) skd_phase_codes_and_header(&sh, out);
        skb_phase_crc_lanes(&cs, p, n, lane); // the tokenizer has just pulled the text through the caches
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

// ------------------------------------------------------------------------------------------
// 2 scan of the member sizes (one workgroup), counts and verdict
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BZ_THREADS) sk_bgzf_scan_kernel(bz_args a)
{
    __shared__ uint64_t lds[2 * BZ_THREADS / 64];
    const uint64_t total = bz_length(a), nb = bz_blocks(total);
    uint64_t run[2] = {0, 0};
    for (uint64_t b0 = 0; b0 < nb; b0 += BZ_THREADS) {
        const uint64_t b = b0 + threadIdx.x;
        uint64_t v[2] = {0, 0}, tot[2];
        if (b < nb) {
            const uint32_t body = a.table[b].body;
            v[0] = skb_member_bytes(body & ~SKB_STORED_FLAG);
            v[1] = body >> 31;
        }
        sk_block_scan<2, BZ_THREADS>(v, tot, lds);
        if (b < nb) a.table[b].off = run[0] + v[0];
        run[0] += tot[0];
        run[1] += tot[1];
    }
    if (threadIdx.x == 0) {
        const uint64_t need = run[0] + ((a.flags & SK_BGZF_EOF) ? SKB_EOF_BYTES : 0);
        a.hdr[SK_BGZF_H_BYTES_IN] = total;
        a.hdr[SK_BGZF_H_BLOCKS] = nb;
        a.hdr[SK_BGZF_H_STORED] = run[1];
        a.hdr[SK_BGZF_H_BYTES_OUT] = need;
        a.hdr[SK_BGZF_H_FIT] = need <= a.capacity;
    }
}

// ------------------------------------------------------------------------------------------
// 3 pack
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BZ_THREADS) sk_bgzf_pack_kernel(bz_args a)
{
    if (!a.hdr[SK_BGZF_H_FIT]) return; // uniform: an image beyond the capacity leaves `out` untouched
    const uint64_t total = a.hdr[SK_BGZF_H_BYTES_IN], nb = a.hdr[SK_BGZF_H_BLOCKS];
    if (blockIdx.x == 0 && (a.flags & SK_BGZF_EOF) && threadIdx.x < SKB_EOF_BYTES)
        a.out[a.hdr[SK_BGZF_H_BYTES_OUT] - SKB_EOF_BYTES + threadIdx.x] = skb_eof_byte(threadIdx.x);
    for (uint64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const sk_bgzf_entry e = a.table[b];
        const bool stored = e.body >> 31;
        const uint32_t body = e.body & ~SKB_STORED_FLAG, m = skb_member_bytes(body);
        const uint32_t n = (uint32_t)min((uint64_t)SK_BGZF_BLOCK, total - b * SK_BGZF_BLOCK);
        // member bytes [0, head) are synthesized, [head, tail) come from src, [tail, m) are the trailer
        const uint32_t head = SKB_HEADER_BYTES + (stored ? SKB_STORED_BYTES : 0), tail = SKB_HEADER_BYTES + body;
        const uint8_t *src = stored ? a.text + b * SK_BGZF_BLOCK : reinterpret_cast<const uint8_t *>(a.slots + b * SKD_OUT_WORDS);
        const uint64_t off = e.off, end = off + m;
        for (uint64_t g = (off & ~15ull) + 16u * threadIdx.x; g < end; g += 16u * BZ_THREADS) {
            if (g >= off + head && g + 16 <= off + tail) { // the granule lies inside the body: the fast path
                __builtin_nontemporal_store(sk_load_window(src + (g - off - head), 16), reinterpret_cast<sk_u4 *>(a.out + g));
                continue;
            }
            const uint64_t lo = max(g, off), hi = min(g + 16, end);
            for (uint64_t pos = lo; pos < hi; ++pos) {
                const uint32_t q = (uint32_t)(pos - off);
                a.out[pos] = q < head ? skb_head_byte(q, m, n) : q < tail ? src[q - head] : skb_tail_byte(q - tail, e.crc, n);
            }
        }
    }
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_bgzf(const sk_bgzf_input *in, uint8_t *out, uint64_t capacity,
                                                                           int flags, void *workspace, int cu_count,
                                                                           hipStream_t stream)
{
    sk_bgzf_layout L;
    sk_bgzf_layout_of(in->bytes, &L);
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    bz_args a;
    a.text = in->text;
    a.bytes = in->bytes;
    a.bytes_dev = in->bytes_dev;
    a.valid_dev = in->valid_dev;
    a.out = out;
    a.capacity = capacity;
    a.flags = flags;
    a.hdr = reinterpret_cast<uint64_t *>(ws);
    a.table = reinterpret_cast<sk_bgzf_entry *>(ws + L.table);
    a.tokens = reinterpret_cast<uint32_t *>(ws + L.tokens);
    a.slots = reinterpret_cast<uint32_t *>(ws + L.slots);
    if (L.grid && (flags & SK_BGZF_SEARCH))
        sk_launch_bgzf_search_block(&a, reinterpret_cast<uint32_t *>(ws + L.total), (unsigned)L.grid, stream);
    else if (L.grid)
        hipLaunchKernelGGL(sk_bgzf_block_kernel, dim3((unsigned)L.grid), dim3(SKD_LANES), 0, stream, a);
    hipLaunchKernelGGL(sk_bgzf_scan_kernel, dim3(1), dim3(BZ_THREADS), 0, stream, a);
    const uint64_t pack_grid = L.n_blocks < (uint64_t)cu_count * BZ_PACK_WG_PER_CU ? L.n_blocks : (uint64_t)cu_count * BZ_PACK_WG_PER_CU;
    hipLaunchKernelGGL(sk_bgzf_pack_kernel, dim3((unsigned)(pack_grid ? pack_grid : 1)), dim3(BZ_THREADS), 0, stream, a);
    return hipGetLastError();
}
