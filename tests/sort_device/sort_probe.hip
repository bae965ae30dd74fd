// TEST ONLY (tests/test_gpu_sorted.py): the regrouping kernels of sickle_amd/csrc/sk_sort.hip run on their own, so that what they
// write -- tile lists, perm, counts -- can be compared with tests/sort_model.py.  The file is included, not linked: the
// launcher is hidden inside libsickle_amd.so.
//
// usage: sort_probe IN OUT
//   IN:  uint64 cases; per case uint64 n, uint64 max_len, uint64 offsets[n + 1]
//   OUT: per case uint64 cap, uint32 counts[16], uint64 lists[8 * cap * 4], uint64 perm[8 * cap * 64]
// Per case the scratch is sized as ensure_sort (sk_capi.hip) sizes it, counts (both sets) zeroed, lists and perm pre-filled
// with a sentinel, and sk_launch_sort called once.
#include "sk_sort.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "sort_probe: %s: %s (line %d)\n", #call, hipGetErrorString(e_), __LINE__); \
            return 2;                                                                                 \
        }                                                                                             \
    } while (0)

static const unsigned long long kSentinel = 0xA5A5A5A5A5A5A5A5ull;

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: sort_probe IN OUT\n");
        return 2;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) {
        fprintf(stderr, "sort_probe: cannot open %s / %s\n", argv[1], argv[2]);
        return 2;
    }
    uint64_t cases = 0;
    if (fread(&cases, 8, 1, in) != 1) return 2;
    for (uint64_t c = 0; c < cases; ++c) {
        uint64_t hdr[2];
        if (fread(hdr, 8, 2, in) != 2) return 2;
        const uint64_t n = hdr[0];
        const uint32_t max_len = (uint32_t)hdr[1];
        if (n == 0 || n >= (1ull << 32)) return 2;
        std::vector<uint64_t> offsets(n + 1);
        if (fread(offsets.data(), 8, n + 1, in) != n + 1) return 2;
        // == ensure_sort
        const size_t windows = (size_t)((n + SK_SORT_WINDOW - 1) / SK_SORT_WINDOW);
        const size_t per_list = ((windows + 7) / 8) * (SK_SORT_WINDOW / 64 + 64) + 8;
        const uint64_t cap = per_list + (per_list >> 3);
        const size_t list_words = 8 * cap * 4, perm_words = 8 * cap * 64;
        uint64_t *d_offsets = nullptr, *d_perm = nullptr;
        unsigned long long *d_lists = nullptr;
        uint32_t *d_counts = nullptr;
        CHECK(hipMalloc(&d_offsets, (n + 1) * 8));
        CHECK(hipMalloc(&d_lists, list_words * 8));
        CHECK(hipMalloc(&d_perm, perm_words * 8));
        CHECK(hipMalloc(&d_counts, 32 * sizeof(uint32_t)));
        std::vector<unsigned long long> fill(perm_words, kSentinel);
        CHECK(hipMemcpy(d_offsets, offsets.data(), (n + 1) * 8, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_lists, fill.data(), list_words * 8, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_perm, fill.data(), perm_words * 8, hipMemcpyHostToDevice));
        CHECK(hipMemset(d_counts, 0, 32 * sizeof(uint32_t)));
        CHECK(sk_launch_sort(d_offsets, n, max_len, d_perm, d_lists, (uint32_t)cap, d_counts, d_counts + 16, nullptr));
        CHECK(hipDeviceSynchronize());
        uint32_t counts[16];
        std::vector<unsigned long long> lists(list_words);
        CHECK(hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(lists.data(), d_lists, list_words * 8, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(fill.data(), d_perm, perm_words * 8, hipMemcpyDeviceToHost));
        if (fwrite(&cap, 8, 1, out) != 1 || fwrite(counts, 4, 16, out) != 16 || fwrite(lists.data(), 8, list_words, out) != list_words ||
            fwrite(fill.data(), 8, perm_words, out) != perm_words)
            return 2;
        CHECK(hipFree(d_offsets));
        CHECK(hipFree(d_lists));
        CHECK(hipFree(d_perm));
        CHECK(hipFree(d_counts));
    }
    if (fclose(out) != 0) return 2;
    printf("sort_probe ok: %llu cases\n", (unsigned long long)cases);
    return 0;
}
