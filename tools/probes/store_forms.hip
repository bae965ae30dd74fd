// probe: what does the headline kernel's cut-pair store cost, by store form?  The traffic shape of
// sk_scan_tile_staged_kernel<10> without its arithmetic (read_bw.hip's read_tiles: one wave per workgroup, 12 per
// CU, ten nt 16-byte loads per lane and 9728-byte tile), with the 512 bytes of cut pairs per tile written
//   0  not at all                         4  16 bytes x 32 lanes, write-through (sc1)
//   1  8 bytes per lane, plain (the kernel's form before this probe)
//   2  8 bytes per lane, nt               5  16 bytes x 32 lanes, write-through (sc0 sc1)
//   3  16 bytes x 32 lanes, plain         6  8 bytes per lane, write-through (sc1)
//   7  16 bytes x 32 lanes, nt
// Each case runs as bench.py runs the headline: 150 launches to settle, then 300 queued back to back with one
// event pair each.  Reported: the mean of the 300 event times, and the time from the first event to the last over
// 300 -- the difference is what a launch boundary costs beyond the kernel's own run.  ROUNDS rounds, the cases
// interleaved, so that a case's spread across its own repetitions stands beside the differences between cases.
// Usage: store_forms [rounds] [only-case]     (only-case: one form, 450 launches, nothing else: for a kernel trace)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1); } } while (0)

typedef unsigned int v4u __attribute__((ext_vector_type(4)));
typedef unsigned int v2u __attribute__((ext_vector_type(2)));

template <int FORM>
__global__ __launch_bounds__(64) void store_tiles(const unsigned char *__restrict__ src, size_t n_tiles, uint2 *out)
{
    v4u acc = {0, 0, 0, 0};
    const unsigned lane = threadIdx.x;
    for (size_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const unsigned char *g = src + t * 9728;
        v4u v[10];
#pragma unroll
        for (int p = 0; p < 10; ++p) {
            unsigned off = p * 1024 + lane * 16;
            if (p == 9 && off > 9728 - 16) off = 9728 - 16;
            v[p] = __builtin_nontemporal_load((const v4u *)(g + off));
        }
#pragma unroll
        for (int p = 0; p < 10; ++p) { acc.x ^= v[p].x; acc.y ^= v[p].y; acc.z ^= v[p].z; acc.w ^= v[p].w; }
        uint2 *dst = out + t * 64; // the tile's 512 bytes of cut pairs (wave-uniform)
        if (FORM == 1) dst[lane] = make_uint2(acc.x, acc.y);
        if (FORM == 2) { v2u c = {acc.x, acc.y}; __builtin_nontemporal_store(c, (v2u *)dst + lane); }
        if (FORM == 3 && lane < 32) ((v4u *)dst)[lane] = acc;
        if (FORM == 7 && lane < 32) __builtin_nontemporal_store(acc, (v4u *)dst + lane);
        if (FORM >= 4 && FORM <= 6) {
            // the write-through forms through a buffer descriptor of the tile's 512 bytes: the cache policy is the
            // store builtin's aux operand (16 = sc1, 17 = sc0 sc1), so the compiler counts the store like any other
            const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(dst, 0, 512, 0x00020000);
            if (FORM == 4 && lane < 32) __builtin_amdgcn_raw_buffer_store_b128(acc, rsrc, (int)(lane * 16), 0, 16);
            if (FORM == 5 && lane < 32) __builtin_amdgcn_raw_buffer_store_b128(acc, rsrc, (int)(lane * 16), 0, 17);
            if (FORM == 6) { v2u c = {acc.x, acc.y}; __builtin_amdgcn_raw_buffer_store_b64(c, rsrc, (int)(lane * 8), 0, 16); }
        }
    }
    if (!FORM && (acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345678u) out[lane] = make_uint2(1, 1);
}

static const char *const NAMES[8] = {"no store (read only)", "8 B/lane plain (parent)", "8 B/lane nt", "16 B x 32 lanes plain",
                                     "16 B x 32 lanes sc1", "16 B x 32 lanes sc0 sc1", "8 B/lane sc1", "16 B x 32 lanes nt"};

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 5;
    const int only = argc > 2 ? atoi(argv[2]) : -1;
    const size_t bytes = 1520000000ull / 9728 * 9728, n_tiles = bytes / 9728;
    const int SETTLE = 150, REPS = 300, GRID = 256 * 12;
    unsigned char *d;
    uint2 *cuts;
    CK(hipMalloc(&d, bytes + 4096));
    CK(hipMalloc(&cuts, n_tiles * 64 * 8));
    CK(hipMemset(d, 1, bytes));
    hipStream_t s;
    CK(hipStreamCreate(&s));
    auto launch = [&](int form) {
        switch (form) {
#define F(N) case N: hipLaunchKernelGGL((store_tiles<N>), dim3(GRID), dim3(64), 0, s, d, n_tiles, cuts); break
            F(0); F(1); F(2); F(3); F(4); F(5); F(6); F(7);
#undef F
        }
    };
    if (only >= 0) {
        for (int i = 0; i < SETTLE + REPS; ++i) launch(only);
        CK(hipStreamSynchronize(s));
        printf("form %d (%s): %d launches queued back to back\n", only, NAMES[only], SETTLE + REPS);
        return 0;
    }
    std::vector<hipEvent_t> e0(REPS), e1(REPS);
    for (int i = 0; i < REPS; ++i) { CK(hipEventCreate(&e0[i])); CK(hipEventCreate(&e1[i])); }
    std::vector<double> ev[8], wall[8];
    for (int r = 0; r < rounds; ++r)
        for (int form = 0; form < 8; ++form) {
            for (int i = 0; i < SETTLE; ++i) launch(form);
            CK(hipStreamSynchronize(s));
            for (int i = 0; i < REPS; ++i) { CK(hipEventRecord(e0[i], s)); launch(form); CK(hipEventRecord(e1[i], s)); }
            CK(hipStreamSynchronize(s));
            CK(hipGetLastError());
            double sum = 0;
            for (int i = 0; i < REPS; ++i) { float ms; CK(hipEventElapsedTime(&ms, e0[i], e1[i])); sum += ms; }
            float span;
            CK(hipEventElapsedTime(&span, e0[0], e1[REPS - 1]));
            ev[form].push_back(sum / REPS);
            wall[form].push_back(span / REPS);
            printf("round %d form %d %-26s events %.4f ms  wall/launch %.4f ms  boundary %.2f us\n", r, form, NAMES[form],
                   sum / REPS, span / REPS, (span / REPS - sum / REPS) * 1e3);
            fflush(stdout);
        }
    printf("\n%-28s %-30s %-30s\n", "form", "events: mean [min .. max] ms", "wall/launch: mean [min .. max] ms");
    for (int form = 0; form < 8; ++form) {
        auto stat = [](const std::vector<double> &v, double &mean, double &lo, double &hi) {
            mean = 0;
            for (double x : v) mean += x;
            mean /= v.size();
            lo = *std::min_element(v.begin(), v.end());
            hi = *std::max_element(v.begin(), v.end());
        };
        double m, lo, hi, wm, wlo, whi;
        stat(ev[form], m, lo, hi);
        stat(wall[form], wm, wlo, whi);
        printf("%d %-26s %.4f [%.4f .. %.4f]      %.4f [%.4f .. %.4f]\n", form, NAMES[form], m, lo, hi, wm, wlo, whi);
    }
    return 0;
}
