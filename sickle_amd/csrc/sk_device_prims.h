// sk_device_prims.h -- the device primitives that more than one kernel file uses as they are: the workgroup scan of the
// reduce-then-scan calls (sk_trim.hip, sk_fastq.hip, sk_fastq_rejects.hip, sk_bgzf.hip) and the unaligned 16-byte window
// of their gathers.  Device only; everything is inlined into its caller.
#ifndef SK_DEVICE_PRIMS_H
#define SK_DEVICE_PRIMS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned sk_u4 __attribute__((ext_vector_type(4)));
typedef unsigned __int128 sk_u128;

// exclusive prefix sums of N values over a workgroup of THREADS lanes; total[] = the sums over it.  lds: N * THREADS / 64
// words.  Every lane of the workgroup calls it: two barriers.
template <int N, int THREADS>
__device__ __forceinline__ void sk_block_scan(uint64_t (&v)[N], uint64_t (&total)[N], uint64_t *lds)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t inc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) inc[i] = v[i];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const uint64_t t = __shfl_up(inc[i], d);
            if (lane >= d) inc[i] += t;
        }
    }
    if (lane == 63)
#pragma unroll
        for (int i = 0; i < N; ++i) lds[w * N + i] = inc[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        uint64_t base = 0, tot = 0;
#pragma unroll
        for (int ww = 0; ww < THREADS / 64; ++ww) {
            const uint64_t x = lds[ww * N + i];
            base += ww < w ? x : 0;
            tot += x;
        }
        v[i] = base + inc[i] - v[i];
        total[i] = tot;
    }
    __syncthreads();
}

// the n (1..16) bytes at p as the first bytes of a granule, from aligned 16-byte loads only: both blocks touched hold a
// byte of [p, p + n), so nothing beyond the buffer that holds them is read, whatever p's alignment.  (With a constant
// n = 16 the test for the second block folds away: it is reached with sh != 0 only.)
__device__ __forceinline__ sk_u4 sk_load_window(const uint8_t *p, int n)
{
    const uintptr_t ad = reinterpret_cast<uintptr_t>(p);
    const sk_u4 *blk = reinterpret_cast<const sk_u4 *>(ad & ~(uintptr_t)15);
    const int sh = (int)(ad & 15);
    const sk_u4 lo = blk[0];
    if (sh == 0) return lo;
    const sk_u4 hi = sh + n > 16 ? blk[1] : lo;
    const int s4 = sh >> 2, sb = sh & 3;
    // words s4 .. s4 + 4 of {lo, hi}, then the byte shift
    const uint32_t x0 = lo.x, x1 = lo.y, x2 = lo.z, x3 = lo.w, x4 = hi.x, x5 = hi.y, x6 = hi.z, x7 = hi.w;
    const uint32_t y0 = s4 == 0 ? x0 : s4 == 1 ? x1 : s4 == 2 ? x2 : x3;
    const uint32_t y1 = s4 == 0 ? x1 : s4 == 1 ? x2 : s4 == 2 ? x3 : x4;
    const uint32_t y2 = s4 == 0 ? x2 : s4 == 1 ? x3 : s4 == 2 ? x4 : x5;
    const uint32_t y3 = s4 == 0 ? x3 : s4 == 1 ? x4 : s4 == 2 ? x5 : x6;
    const uint32_t y4 = s4 == 0 ? x4 : s4 == 1 ? x5 : s4 == 2 ? x6 : x7;
    sk_u4 r;
    r.x = __builtin_amdgcn_alignbyte(y1, y0, sb);
    r.y = __builtin_amdgcn_alignbyte(y2, y1, sb);
    r.z = __builtin_amdgcn_alignbyte(y3, y2, sb);
    r.w = __builtin_amdgcn_alignbyte(y4, y3, sb);
    return r;
}

__device__ __forceinline__ sk_u128 sk_to_u128(sk_u4 v)
{
    return (sk_u128)v.x | ((sk_u128)v.y << 32) | ((sk_u128)v.z << 64) | ((sk_u128)v.w << 96);
}

__device__ __forceinline__ sk_u4 sk_from_u128(sk_u128 v)
{
    sk_u4 r;
    r.x = (uint32_t)v;
    r.y = (uint32_t)(v >> 32);
    r.z = (uint32_t)(v >> 64);
    r.w = (uint32_t)(v >> 96);
    return r;
}

// bytes [0, n) of x to bytes [d, d + n) of acc (d + n <= 16)
__device__ __forceinline__ void sk_put(sk_u128 &acc, sk_u128 x, int d, int n)
{
    const sk_u128 m = n >= 16 ? ~(sk_u128)0 : (((sk_u128)1 << (8 * n)) - 1);
    acc |= (x & m) << (8 * d);
}

#endif
