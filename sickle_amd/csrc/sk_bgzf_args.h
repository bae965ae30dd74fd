// sk_bgzf_args.h -- what the kernels of the device's BGZF writer take (sk_bgzf.hip, sk_bgzf_search.hip)
#ifndef SK_BGZF_ARGS_H
#define SK_BGZF_ARGS_H

#include <hip/hip_runtime.h>

#include "sk_device.h"

struct bz_args {
    const uint8_t *text;
    uint64_t bytes; // the length, or its bound
    const uint64_t *bytes_dev, *valid_dev;
    uint8_t *out;
    uint64_t capacity;
    int32_t flags;
    uint64_t *hdr;
    sk_bgzf_entry *table;
    uint32_t *tokens, *slots;
};

// the text's length: never beyond the bound the launches and the workspace were sized by
__device__ __forceinline__ uint64_t bz_length(const bz_args &a)
{
    uint64_t n = a.bytes;
    if (a.bytes_dev) n = min(n, *a.bytes_dev);
    if (a.valid_dev && *a.valid_dev == 0) n = 0;
    return n;
}

__device__ __forceinline__ uint64_t bz_blocks(uint64_t n) { return (n + SK_BGZF_BLOCK - 1) / SK_BGZF_BLOCK; }

// launch 1 with SK_BGZF_SEARCH (sk_bgzf_search.hip).  cand: 4 * SK_BGZF_TOK_WORDS bytes per workgroup
extern "C" __attribute__((visibility("hidden"))) void sk_launch_bgzf_search_block(const bz_args *a, uint32_t *cand, unsigned grid,
                                                                                 hipStream_t stream);

#endif
