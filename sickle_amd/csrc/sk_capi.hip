// sk_capi.hip -- the C ABI of include/sickle_amd.h over the kernels of sk_kernels.hip.
// HIP only: there is no CPU path behind these entry points.

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "sickle_amd.h"
#include "sk_device.h"
#include "sk_fastq_adapters.h"
#include "sk_fastq_clip.h"
#include "sk_fastq_rejects.h"
#include "sk_fastq_verdict.h"
#include "sk_gunzip_block.h"

static_assert(sizeof(sk_tile) == sizeof(sk_tile_dev) && sizeof(sk_tile) == 24, "sk_tile layout");

namespace {

// reference src/sickle.h:85-91
const int32_t kQualityConstants[4][3] = {
    {0, 4, 60},    // PHRED
    {33, 33, 126}, // SANGER
    {64, 58, 112}, // SOLEXA
    {64, 64, 110}, // ILLUMINA
};
// reference src/sickle.h:68-73
const char *const kTypeNames[4] = {"Phred", "Sanger", "Solexa", "Illumina"};

constexpr unsigned long long kNoError = ~0ull;
constexpr uint32_t SK_SEG_MAX_CLASSES = 16;

// device scratch of the regrouping of mixed-length ragged batches (sk_sort.hip): one per stream of scans
struct SortScratch {
    uint64_t *perm = nullptr;            // 8 lists x cap_list tiles x 64 entries
    unsigned long long *lists = nullptr; // 8 lists x cap_list descriptors of 32 bytes
    uint32_t *counts = nullptr;          // 2 x 16 words: tiles per list [8], flags [2] -- one set per scan, in turns: a scan's
                                         // first kernel clears the set of the scan after it (no memset on the launch path)
    uint32_t turn = 0;
    size_t cap_list = 0;
    void release_lists()
    {
        if (perm) (void)hipFree(perm);
        if (lists) (void)hipFree(lists);
        perm = nullptr, lists = nullptr, cap_list = 0;
    }
    void release()
    {
        release_lists();
        if (counts) (void)hipFree(counts);
        counts = nullptr;
    }
};

struct Slot {
    bool busy = false;
    SortScratch sort;
    uint8_t *d_qual = nullptr, *d_seq = nullptr;
    size_t cap_bytes = 0;
    uint64_t *d_offsets = nullptr;
    uint32_t *d_lengths = nullptr;
    size_t cap_reads = 0;
    sk_tile_dev *d_tiles = nullptr;
    uint32_t *d_out_index = nullptr;
    size_t cap_tiles = 0, cap_index = 0;
    sk_cut_dev *d_out = nullptr;
    std::vector<sk_seg_class> classes;   // segmented batches without a class table: cut here
    unsigned long long *d_err = nullptr; // device error word of this slot
    unsigned long long *h_err = nullptr; // pinned copy
    hipEvent_t copied = nullptr;         // H2D done (copy stream)
    hipEvent_t finished = nullptr;       // D2H of cuts + error word done (compute stream)
};

} // namespace

struct sk_ctx {
    int device = 0;
    int cu_count = 256;
    hipStream_t compute = nullptr, copy = nullptr;
    uint32_t *d_band = nullptr;          // the band matrices of every window width the tile kernels take (sk_device.h)
    unsigned long long *d_err = nullptr; // error word of the device-resident path on the NULL stream
    unsigned long long *h_err = nullptr;
    // ... and one per other stream the caller scans on: errors of scans enqueued on different streams do
    // not meet in one word (each sk_scan_device_finish reports what ITS stream's scans found)
    struct ErrWord {
        unsigned long long *d = nullptr, *h = nullptr; // d: error word, hand-over word, four pair counters (6 x 8 bytes)
        SortScratch sort;
    };
    SortScratch sort0; // ... of the NULL stream
    std::map<hipStream_t, ErrWord> stream_err;
    std::mutex stream_err_lock;
    std::vector<Slot> slots;
    unsigned long long scan_counter = 0;
    char last_error[512] = {0};
};

namespace {

// the error word (device, pinned host copy) of the device-resident scans on `stream`
int err_word_of(sk_ctx *ctx, hipStream_t stream, unsigned long long **d, unsigned long long **h, SortScratch **sort = nullptr);

void set_error(sk_ctx *ctx, const char *fmt, ...)
{
    if (!ctx) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->last_error, sizeof ctx->last_error, fmt, ap);
    va_end(ap);
}

#define SK_HIP(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            set_error((ctx), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return SK_EHIP;                                                                    \
        }                                                                                      \
    } while (0)

// the message and SK_EINVAL: a bad argument (nothing is enqueued behind it), or a finish that found one on the device
#define SK_BAD(ctx, ...)               \
    do {                               \
        set_error((ctx), __VA_ARGS__); \
        return SK_EINVAL;              \
    } while (0)

               // how the finishes that take everything from a workspace's header begin: its first `words` words, waited for
               int read_header(sk_ctx *ctx, const void *workspace, uint64_t *h, size_t words, hipStream_t stream)
               {
               SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, hipMemcpyAsync(h, workspace, words * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    SK_HIP(ctx, hipStreamSynchronize(stream));
    return SK_OK;
}

bool tile_eligible(const sk_batch *b);

int make_args(sk_ctx *ctx, const sk_params *p, const sk_batch *b, sk_scan_args *a)
{
    if (!p || !b) return SK_EINVAL;
    if (p->qualtype < 0 || p->qualtype > 3) {
        set_error(ctx, "invalid qualtype %d", p->qualtype);
        return SK_EINVAL;
    }
    if (p->qual_threshold < 0 || p->length_threshold < 0) {
        set_error(ctx, "thresholds must be >= 0"); // reference src/trim_single.cpp:124,132
        return SK_EINVAL;
    }
    if (b->n_reads > 0 && !b->qual) {
        set_error(ctx, "qual is NULL");
        return SK_EINVAL;
    }
    if (p->trunc_n && b->n_reads > 0 && !b->seq) {
        set_error(ctx, "trunc_n needs seq");
        return SK_EINVAL;
    }
    if (b->tiles) {
        if (b->offsets || b->lengths || !b->out_index || b->n_tiles == 0 || b->stride % 8 != 0 ||
            b->stride > SK_TILE_MAX_STRIDE || b->stride == 0) {
            set_error(ctx, "segmented batch: need tiles, out_index, n_tiles and the largest stride (multiple of 8, <= %u)",
                      SK_TILE_MAX_STRIDE);
            return SK_EINVAL;
        }
    } else if (!b->offsets) {
        if (b->stride == 0 || (!b->lengths && b->read_len > b->stride)) {
            set_error(ctx, "fixed-stride batch: need stride >= read_len > 0");
            return SK_EINVAL;
        }
        if (b->read_len > SK_MAX_READ_LEN) return SK_EINVAL;
    }
    if (b->n_reads >= (1ull << 32)) {
        set_error(ctx, "more than 2^32-1 reads in one batch");
        return SK_EINVAL;
    }
    const int32_t *k = kQualityConstants[p->qualtype];
    // Every threshold above the largest representable quality (max - offset <= 93) behaves the
    // same: no window and no char can reach it.  Clamping keeps the device integers small.
    const int32_t qthr = p->qual_threshold > 127 ? 127 : p->qual_threshold;
    a->n_reads = b->n_reads;
    a->stride = b->stride;
    a->read_len = b->read_len;
    a->qmin = k[1];
    a->qmax = k[2];
    a->craw = qthr + k[0];
    a->cthr = a->craw > 128 ? 128 : a->craw;
    a->cthr_raw = a->craw;
    a->lthr = p->length_threshold;
    a->no5 = p->no_fiveprime ? 1 : 0;
    a->truncn = p->trunc_n ? 1 : 0;
    a->n_tiles = b->tiles ? b->n_tiles : 0;
    static const int order = [] { const char *e = getenv("SK_TILE_ORDER"); return e ? atoi(e) : 0; }();
    a->tile_order = order;
    a->buf_bytes = 0;
    a->slot_order = (b->tiles && b->cuts_in_slot_order) ? 1 : 0;
    a->scan_id = 0;
    a->team_rbuf = 0;
    a->team_maxlen = 0;
    a->stream_nb = 0;
    a->stream_read_cost = 0;
    a->stream_tbl = 0;
    static const uint32_t seg_shift = [] { const char *e = getenv("SK_SEG_CHUNK_SHIFT"); return e ? (uint32_t)atoi(e) : 0u; }();
    a->seg_chunk_shift = seg_shift > 6u ? 6u : seg_shift;
    a->sort_flags = nullptr;
    a->n_reads_dev = nullptr;
    a->band_table = ctx ? ctx->d_band : nullptr;
    return SK_OK;
}

// LDS bytes per wave for the tiles of a ragged batch whose reads are at most `max_len` bytes
// (0 = unknown): 64 reads + what a lane may read past its row, so that uniform 150 bp gets 10 KiB
// (16 waves per CU); tiles that do not fit go to the general kernel.
uint32_t rag_buf_bytes(uint64_t max_len, bool uniform)
{
    if (max_len == 0) return SK_RAG_BUF_DEFAULT;
    // == rag_pitch<UNIFORM>() of the kernels
    (void)uniform;
    const uint64_t pitch = 16 * (((max_len + 15) >> 4) | 1);
    uint64_t need = (64 * pitch + SK_TILE_SLACK + 15) & ~(uint64_t)15;
    if (need < 4096) need = 4096;
    if (need > SK_RAG_BUF_MAX) need = SK_RAG_BUF_MAX;
    return (uint32_t)need;
}

// which path a batch takes: 3 segmented, 1 tiled (aligned rows), 5 tiled (rows at any address),
// 2 general kernel only
// The general kernels, by the caller's longest-read hint: teams of 16 lanes per read (sk_team.hip) up to SK_STREAM_MIN
// bytes, the streaming wave-per-read kernel (sk_stream.hip) beyond and when there is no hint.  SK_GENERAL=band|team|stream
// forces one (diagnostics, tests; band = round 3's wave-per-read kernel with matrix-pipe window sums, sk_band.hip:
// parity-green, not faster than the teams, selected by nothing).  Uniform medium reads do not come here: wide_takes().
constexpr uint64_t SK_STREAM_MIN_DEFAULT = 4096;
hipError_t launch_general(const uint8_t *qual, const uint8_t *seq, const uint64_t *offsets, const uint32_t *lengths, sk_cut_dev *out,
                          unsigned long long *errword, const sk_scan_args *a, uint64_t max_len, int cu_count, hipStream_t stream)
{
    const char *force = getenv("SK_GENERAL");
    static const uint64_t stream_min = [] { const char *e = getenv("SK_STREAM_MIN"); return e ? (uint64_t)atoll(e) : SK_STREAM_MIN_DEFAULT; }();
    const bool use_stream = force ? force[0] == 's' : (max_len == 0 || max_len > stream_min);
    if (!use_stream && !(force && force[0] == 'b')) return sk_launch_team(qual, seq, offsets, lengths, out, errword, a, max_len, cu_count, stream);
    return use_stream ? sk_launch_stream(qual, seq, offsets, lengths, out, errword, a, max_len, cu_count, stream)
                      : sk_launch_band(qual, seq, offsets, lengths, out, errword, a, max_len, cu_count, stream);
}

// uniform medium reads (rows beyond the 64-read tiles, windows of 32 and more, two waves' images to a CU): the tile kernel
// with 32-read tiles (sk_kernels.hip, WIDE).  SK_GENERAL=team|band|stream sends them to a general kernel instead (A/B runs,
// tests), SK_WIDE_MAX bounds the lengths it takes.
bool wide_takes(const sk_batch *b)
{
    if (b->offsets || b->lengths || b->tiles || getenv("SK_GENERAL")) return false;
    static const uint32_t wide_max = [] { const char *e = getenv("SK_WIDE_MAX"); return e ? (uint32_t)atoi(e) : 2200u; }();
    return b->read_len <= wide_max && b->stride < (1u << 24) && sk_wide_lds_bytes(b->read_len) != 0; // (the loader's 24-bit row offsets)
}

int path_of(const sk_batch *b)
{
    if (b->tiles) return 3;
    if (tile_eligible(b)) return 1;
    if (!b->offsets && !b->lengths) return (b->stride <= SK_TILE_MAX_STRIDE) ? 5 : 2;
    return 5; // ragged: tiles that fit a wave's LDS buffer by the tile kernel, the others by the general one
}

bool tile_eligible(const sk_batch *b)
{
    return !b->offsets && !b->tiles && b->stride % 8 == 0 && b->stride >= 8 && b->stride <= SK_TILE_MAX_STRIDE &&
           (reinterpret_cast<uintptr_t>(b->qual) & 15) == 0 && (!b->seq || (reinterpret_cast<uintptr_t>(b->seq) & 15) == 0);
}

// enqueue the kernel.  All pointers are device pointers.  The error word is "no error" on
// entry: it is reset when the context is created and again by whoever reads it
// (reset_error_word), so nothing but the kernel sits on the launch path.
// rag_fit (batches with `offsets` or `lengths`): does any 64-read tile fit the tile kernel's LDS buffer?  1 yes, 0 no
// (the general kernel takes the whole batch in spans of equal cost), -1 not known: sk_submit counts on the host,
// a device-resident batch is taken for a long-read batch when the caller's longest-read hint is beyond
// SK_LONG_BATCH_HINT -- 64 CONSECUTIVE reads of at most 2 040 bases do not occur in one.
#define SK_LONG_BATCH_HINT 4096u
// the longest read whose 64-row image fits a wave buffer of `buf` bytes (== rag_tile_fits of the kernels)
uint32_t rag_fit_len(uint32_t buf)
{
    uint32_t best = 0;
    for (uint32_t L = 16; L <= SK_RAG_MAX_LEN; L += 16)
        if (64u * 16u * ((L >> 4) | 1u) + SK_TILE_SLACK <= buf) best = L;
    return best;
}

// scratch for a regrouping of n reads; false (and no sorting) if it cannot be had
bool ensure_sort(sk_ctx *ctx, SortScratch &s, uint64_t n)
{
    // per list: the tiles of every eighth window, at most SK_SORT_WINDOW / 64 full ones + one partial one per class each;
    // 32 bytes of descriptor and 64 x 8 bytes of entries per tile (~9 bytes per read as the lists fill, 13 at worst)
    const size_t windows = (size_t)((n + SK_SORT_WINDOW - 1) / SK_SORT_WINDOW);
    const size_t per_list = ((windows + 7) / 8) * (SK_SORT_WINDOW / 64 + 64) + 8;
    if (hipSetDevice(ctx->device) != hipSuccess) return false;
    if (!s.counts) {
        if (hipMalloc(&s.counts, 32 * sizeof(uint32_t)) != hipSuccess) return false;
        if (hipMemset(s.counts, 0, 32 * sizeof(uint32_t)) != hipSuccess) return false; // synchronous: done before any scan is enqueued
        s.turn = 0;
    }
    if (per_list > s.cap_list) {
        s.release_lists();
        const size_t cap = per_list + (per_list >> 3);
        if (hipMalloc(&s.lists, 8 * cap * 4 * sizeof(unsigned long long)) != hipSuccess) return false;
        if (hipMalloc(&s.perm, 8 * cap * 64 * sizeof(uint64_t)) != hipSuccess) {
            s.release_lists();
            return false;
        }
        s.cap_list = cap;
    }
    return true;
}

int enqueue_scan(sk_ctx *ctx, const sk_scan_args *a, const sk_batch *b, sk_cut_dev *out, unsigned long long *d_err,
                 hipStream_t stream, int rag_fit = -1, SortScratch *sort = nullptr)
{
    if (a->n_reads == 0) return SK_OK;
    const uint8_t *seq = a->truncn ? b->seq : nullptr;
    const int path = path_of(b);
    if (path == 3) {
        SK_HIP(ctx, sk_launch_seg(b->qual, seq, reinterpret_cast<const sk_tile_dev *>(b->tiles), b->out_index, out, d_err, a,
                                  b->classes, b->n_classes, ctx->cu_count, stream));
    } else if (path == 1) {
        SK_HIP(ctx, sk_launch_tile(b->qual, seq, b->lengths, out, d_err, a, ctx->cu_count, stream));
    } else if (path == 5) {
        sk_scan_args ar = *a;
        const bool ragged = b->offsets || b->lengths;
        if (ragged && (rag_fit == 0 || (rag_fit < 0 && b->offsets && b->stride > SK_LONG_BATCH_HINT))) {
            SK_HIP(ctx, launch_general(b->qual, seq, b->offsets, b->lengths, out, d_err, a, b->stride, ctx->cu_count, stream));
            return SK_OK;
        }
        // the scans of a context are numbered upwards: the tile kernel leaves the number in the word after
        // the error word when it skips a tile, the general kernel returns at once if it does not find it
        ar.scan_id = ++ctx->scan_counter;
        // b->stride of an `offsets` batch is the caller's hint of the longest read (0 = unknown); with
        // stride + lengths it bounds the reads; packed uniform batches: the read length is known
        ar.buf_bytes = rag_buf_bytes(ragged ? b->stride : b->read_len, !ragged);
        // A big `offsets` batch is regrouped first (sk_sort.hip: windows of 8192 reads counting-sorted by window width,
        // 8 bytes of scratch per read).  If that finds reads of different lengths -- and none too long for the tiles --
        // the sorted scan below takes the batch on the matrix path and the two kernels after it return at once; a
        // batch of one length (or with long reads) is theirs as before and the sorted scan returns.  SK_SORT=0: never.
        static const bool sort_on = [] { const char *e = getenv("SK_SORT"); return !(e && *e == '0'); }();
        static const uint64_t sort_min = [] { const char *e = getenv("SK_SORT_MIN"); return e ? (uint64_t)atoll(e) : (uint64_t)SK_SORT_MIN_READS; }(); // (tests lower it)
        uint32_t *sort_counts = nullptr;
        const bool sorted = sort_on && sort && b->offsets && a->n_reads >= sort_min && ensure_sort(ctx, *sort, a->n_reads);
        if (sorted) {
            uint32_t fit = rag_fit_len(ar.buf_bytes);
            if (b->stride && b->stride < fit) fit = b->stride;
            sort_counts = sort->counts + 16u * (sort->turn & 1u);
            SK_HIP(ctx, sk_launch_sort_counted(b->offsets, a->n_reads, a->n_reads_dev, fit, sort->perm, sort->lists, (uint32_t)sort->cap_list,
                                               sort_counts, sort->counts + 16u * (~sort->turn & 1u), stream));
            ++sort->turn;
            ar.sort_flags = sort_counts + 8;
        }
        SK_HIP(ctx, sk_launch_any(b->qual, seq, b->offsets, b->lengths, out, d_err, &ar, ctx->cu_count, stream));
        if (sorted) {
            sk_scan_args as = ar;
            as.n_tiles = (uint32_t)sort->cap_list;
            SK_HIP(ctx, sk_launch_sorted(b->qual, seq, b->offsets, sort->perm, sort->lists, sort_counts, out, d_err, &as, ctx->cu_count, stream));
        }
        // the tiles that kernel leaves: those whose reads are too long for a wave's buffer (none in a
        // packed uniform batch)
        if (ragged) SK_HIP(ctx, launch_general(b->qual, seq, b->offsets, b->lengths, out, d_err, &ar, b->stride, ctx->cu_count, stream));
    } else if (wide_takes(b)) {
        SK_HIP(ctx, sk_launch_wide(b->qual, seq, out, d_err, a, ctx->cu_count, stream));
    } else {
        SK_HIP(ctx, launch_general(b->qual, seq, b->offsets, b->lengths, out, d_err, a, b->read_len, ctx->cu_count, stream));
    }
    return SK_OK;
}

int err_word_of(sk_ctx *ctx, hipStream_t stream, unsigned long long **d, unsigned long long **h, SortScratch **sort)
{
    if (stream == nullptr) {
        *d = ctx->d_err;
        *h = ctx->h_err;
        if (sort) *sort = &ctx->sort0;
        return SK_OK;
    }
    std::lock_guard<std::mutex> lock(ctx->stream_err_lock);
    sk_ctx::ErrWord &w = ctx->stream_err[stream];
    if (!w.d) {
        SK_HIP(ctx, hipSetDevice(ctx->device));
        SK_HIP(ctx, hipMalloc(&w.d, 8 * sizeof(unsigned long long)));
        SK_HIP(ctx, hipMemset(w.d, 0xff, sizeof(unsigned long long))); // synchronous: done before any scan is enqueued
        SK_HIP(ctx, hipMemset(w.d + 1, 0, 7 * sizeof(unsigned long long)));
        SK_HIP(ctx, hipHostMalloc(&w.h, 6 * sizeof(unsigned long long), hipHostMallocDefault));
        *w.h = kNoError;
    }
    *d = w.d;
    *h = w.h;
    if (sort) *sort = &w.sort;
    return SK_OK;
}

int reset_error_word(sk_ctx *ctx, unsigned long long *d_err, hipStream_t stream)
{
    SK_HIP(ctx, hipMemsetAsync(d_err, 0xff, sizeof(unsigned long long), stream));
    return SK_OK;
}

size_t batch_bytes(const sk_batch *b)
{
    // bytes of qual (and seq) the batch spans on the host
    if (b->n_reads == 0) return 0;
    if (b->tiles) {
        const sk_tile &last = b->tiles[b->n_tiles - 1];
        return (size_t)last.byte_off + (size_t)last.rows * last.stride;
    }
    if (b->offsets) return (size_t)b->offsets[b->n_reads];
    return (size_t)b->n_reads * b->stride;
}

int grow_slot(sk_ctx *ctx, Slot &s, size_t bytes, size_t reads, bool need_seq, bool need_off, bool need_len)
{
    const size_t pad = 256; // the tiled kernel's last 16-byte chunk never crosses this
    if (bytes + pad > s.cap_bytes || (need_seq && !s.d_seq)) {
        size_t cap = bytes + pad > s.cap_bytes ? (bytes + pad) + (bytes >> 3) : s.cap_bytes;
        if (s.d_qual) (void)hipFree(s.d_qual);
        if (s.d_seq) (void)hipFree(s.d_seq);
        s.d_qual = s.d_seq = nullptr;
        s.cap_bytes = 0;
        SK_HIP(ctx, hipMalloc(&s.d_qual, cap));
        if (need_seq) SK_HIP(ctx, hipMalloc(&s.d_seq, cap));
        s.cap_bytes = cap;
    }
    if (reads + 1 > s.cap_reads || (need_off && !s.d_offsets) || (need_len && !s.d_lengths)) {
        size_t cap = reads + 1 > s.cap_reads ? (reads + 1) + (reads >> 3) : s.cap_reads;
        if (s.d_out) (void)hipFree(s.d_out);
        if (s.d_offsets) (void)hipFree(s.d_offsets);
        if (s.d_lengths) (void)hipFree(s.d_lengths);
        s.d_out = nullptr;
        s.d_offsets = nullptr;
        s.d_lengths = nullptr;
        s.cap_reads = 0;
        SK_HIP(ctx, hipMalloc(&s.d_out, cap * sizeof(sk_cut_dev)));
        if (need_off) SK_HIP(ctx, hipMalloc(&s.d_offsets, cap * sizeof(uint64_t)));
        if (need_len) SK_HIP(ctx, hipMalloc(&s.d_lengths, cap * sizeof(uint32_t)));
        s.cap_reads = cap;
    }
    return SK_OK;
}

} // namespace

extern "C" {

const int32_t *sk_quality_constants(int32_t qualtype)
{
    return (qualtype < 0 || qualtype > 3) ? nullptr : kQualityConstants[qualtype];
}

const char *sk_typename(int32_t qualtype) { return (qualtype < 0 || qualtype > 3) ? nullptr : kTypeNames[qualtype]; }

int sk_abi_version(void) { return SK_ABI_VERSION; }

int sk_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sk_create(int device, int slots, sk_ctx **out)
{
    if (!out) return SK_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SK_ENODEV;
    if (device < 0) {
        if (hipGetDevice(&device) != hipSuccess) return SK_ENODEV;
    }
    if (device >= n) return SK_ENODEV;
    if (slots < 1) slots = 1;
    if (slots > 16) slots = 16;
    sk_ctx *ctx = new (std::nothrow) sk_ctx();
    if (!ctx) return SK_EINVAL;
    ctx->device = device;
    auto fail = [&](int rc) {
        fprintf(stderr, "sickle_amd: sk_create failed: %s\n", ctx->last_error);
        sk_destroy(ctx);
        return rc;
    };
#define SK_TRY(call)                                                                    \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            set_error(ctx, "%s failed: %s", #call, hipGetErrorString(e_));              \
            return fail(SK_EHIP);                                                       \
        }                                                                               \
    } while (0)
    SK_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    SK_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(ctx, "device %d is %s, this library is built for gfx950 only", device, prop.gcnArchName);
        return fail(SK_ENODEV);
    }
    ctx->cu_count = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    SK_TRY(hipStreamCreateWithFlags(&ctx->compute, hipStreamNonBlocking));
    SK_TRY(hipStreamCreateWithFlags(&ctx->copy, hipStreamNonBlocking));
    {
        std::vector<uint32_t> band(SK_BAND_TABLE_DWORDS);
        for (uint32_t w = 0; w < SK_BAND_WIDTHS; ++w)
            for (int b = 0; b < 3; ++b)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j)
                        band[((w * 3u + (uint32_t)b) * 64u + (uint32_t)lane) * 4u + (uint32_t)j] = sk_band_dword(lane, (int)w, 16 * (lane >> 5) + 4 * j + 32 * b);
        SK_TRY(hipMalloc(&ctx->d_band, band.size() * sizeof(uint32_t)));
        SK_TRY(hipMemcpy(ctx->d_band, band.data(), band.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    SK_TRY(hipMalloc(&ctx->d_err, 8 * sizeof(unsigned long long)));
    SK_TRY(hipMemset(ctx->d_err, 0xff, sizeof(unsigned long long)));
    SK_TRY(hipMemset(ctx->d_err + 1, 0, 7 * sizeof(unsigned long long))); // the hand-over word (see enqueue_scan), four pair counters, tiles left by the tile kernel
    SK_TRY(hipHostMalloc(&ctx->h_err, 6 * sizeof(unsigned long long), hipHostMallocDefault));
    *ctx->h_err = kNoError;
    ctx->slots.resize((size_t)slots);
    for (Slot &s : ctx->slots) {
        SK_TRY(hipMalloc(&s.d_err, 8 * sizeof(unsigned long long))); // the same block as the context's (words 2..5 unused)
        SK_TRY(hipMemset(s.d_err, 0xff, sizeof(unsigned long long)));
        SK_TRY(hipMemset(s.d_err + 1, 0, 7 * sizeof(unsigned long long)));
        SK_TRY(hipHostMalloc(&s.h_err, sizeof(unsigned long long), hipHostMallocDefault));
        SK_TRY(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
        SK_TRY(hipEventCreateWithFlags(&s.finished, hipEventDisableTiming));
    }
#undef SK_TRY
    *out = ctx;
    return SK_OK;
}

void sk_destroy(sk_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->compute) (void)hipStreamSynchronize(ctx->compute);
    if (ctx->copy) (void)hipStreamSynchronize(ctx->copy);
    for (Slot &s : ctx->slots) {
        if (s.d_qual) (void)hipFree(s.d_qual);
        if (s.d_seq) (void)hipFree(s.d_seq);
        if (s.d_offsets) (void)hipFree(s.d_offsets);
        if (s.d_lengths) (void)hipFree(s.d_lengths);
        if (s.d_tiles) (void)hipFree(s.d_tiles);
        if (s.d_out_index) (void)hipFree(s.d_out_index);
        if (s.d_out) (void)hipFree(s.d_out);
        if (s.d_err) (void)hipFree(s.d_err);
        if (s.h_err) (void)hipHostFree(s.h_err);
        s.sort.release();
        if (s.copied) (void)hipEventDestroy(s.copied);
        if (s.finished) (void)hipEventDestroy(s.finished);
    }
    if (ctx->d_band) (void)hipFree(ctx->d_band);
    if (ctx->d_err) (void)hipFree(ctx->d_err);
    if (ctx->h_err) (void)hipHostFree(ctx->h_err);
    for (auto &kv : ctx->stream_err) {
        if (kv.second.d) (void)hipFree(kv.second.d);
        if (kv.second.h) (void)hipHostFree(kv.second.h);
        kv.second.sort.release();
    }
    ctx->sort0.release();
    if (ctx->compute) (void)hipStreamDestroy(ctx->compute);
    if (ctx->copy) (void)hipStreamDestroy(ctx->copy);
    delete ctx;
}

const char *sk_last_error(const sk_ctx *ctx) { return ctx ? ctx->last_error : "no context"; }
int sk_device(const sk_ctx *ctx) { return ctx ? ctx->device : -1; }

void *sk_host_alloc(sk_ctx *ctx, size_t bytes)
{
    if (!ctx) return nullptr;
    void *p = nullptr;
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
        set_error(ctx, "hipHostMalloc(%zu) failed", bytes);
        return nullptr;
    }
    return p;
}

void sk_host_free(sk_ctx *ctx, void *p)
{
    (void)ctx;
    if (p) (void)hipHostFree(p);
}

int sk_kernel_for(const sk_batch *batch)
{
    if (!batch) return 0;
    if (batch->tiles) return 3;
    if (!tile_eligible(batch)) {
        const int path = path_of(batch);
        const bool ragged = batch->offsets || batch->lengths;
        const uint64_t longest = ragged ? batch->stride : batch->read_len;
        const bool general_only = path == 2 || (path == 5 && batch->offsets && batch->stride > SK_LONG_BATCH_HINT);
        if (path == 2 && wide_takes(batch)) return 8;
        return general_only ? ((longest == 0 || longest > SK_STREAM_MIN_DEFAULT) ? 6 : 2) : path;
    }
    // uniform batches without a sequence buffer (no -n) and rows of 72..160 bytes: the tile comes in
    // through the wave's registers instead of LDS-DMA
    if (!batch->lengths && !batch->seq && sk_tile_is_staged(batch->stride, batch->read_len, 0)) return 4;
    return 1;
}

uint32_t sk_seg_classes(const sk_tile *tiles, uint32_t n_tiles, sk_seg_class *out, uint32_t max_classes)
{
    if (!tiles || !out || n_tiles == 0 || max_classes == 0) return 0;
    // occupancy class of a tile = single-wave workgroups per CU its LDS buffer allows (16 down to 4)
    auto per_cu = [](uint32_t stride) {
        const uint32_t lds = 64u * stride + SK_TILE_SLACK;
        const uint32_t n = lds ? SK_LDS_PER_CU / lds : 16u;
        return n > 16u ? 16u : n;
    };
    auto wide = [](const sk_tile &t) -> uint32_t { return (uint32_t)(t.read_len / 10) > 33u; };
    // pass 1: maximal runs of equal (occupancy, wide)
    std::vector<sk_seg_class> runs;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t pc = per_cu(tiles[t].stride), w = wide(tiles[t]);
        if (!runs.empty() && per_cu(runs.back().max_stride) == pc && runs.back().wide == w) {
            runs.back().n_tiles++;
            if (tiles[t].stride > runs.back().max_stride) runs.back().max_stride = tiles[t].stride;
        } else {
            if (runs.size() >= 4096) return 0; // not a sorted batch
            runs.push_back(sk_seg_class{t, 1u, tiles[t].stride, w});
        }
    }
    // pass 2: runs are gathered into a class until it can fill the device a few times over; then the
    // next run of a different kind opens a new class (a class takes the widest stride and the wide
    // loop of its runs); a short last class joins the one before it
    static const uint32_t min_tiles = [] { const char *e = getenv("SK_SEG_MIN_TILES"); return e ? (uint32_t)atoi(e) : 65536u; }();
    std::vector<sk_seg_class> merged;
    auto join = [](sk_seg_class &m, const sk_seg_class &r) {
        m.n_tiles += r.n_tiles;
        if (r.max_stride > m.max_stride) m.max_stride = r.max_stride;
        m.wide |= r.wide;
    };
    for (const sk_seg_class &r : runs) {
        if (!merged.empty() && merged.back().n_tiles < min_tiles) join(merged.back(), r);
        else merged.push_back(r);
    }
    if (merged.size() > 1 && merged.back().n_tiles < min_tiles) {
        const sk_seg_class last = merged.back();
        merged.pop_back();
        join(merged.back(), last);
    }
    if (merged.size() > max_classes) return 0;
    for (size_t i = 0; i < merged.size(); ++i) out[i] = merged[i];
    return (uint32_t)merged.size();
}

const char *sk_kernel_name(int which)
{
    switch (which) {
    case 1: return "sk_scan_tile_kernel";
    case 2: return "sk_scan_team_kernel";
    case 3: return "sk_scan_tile_kernel";
    case 4: return "sk_scan_tile_staged_kernel";
    case 5: return "sk_scan_tile_any_kernel";
    case 6: return "sk_scan_stream_kernel";
    case 7: return "sk_scan_band_kernel";
    case 8: return "sk_scan_tile_wide_kernel";
    default: return "";
    }
}

int sk_count_pairs_device_async(sk_ctx *ctx, const sk_cut *cuts, uint64_t n_pairs, uint8_t *classes, void *hip_stream)
{
    if (!ctx || (!cuts && n_pairs) || (reinterpret_cast<uintptr_t>(cuts) & 15)) return SK_EINVAL;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    unsigned long long *d, *h;
    int rc = err_word_of(ctx, stream, &d, &h);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, sk_launch_pair_count(reinterpret_cast<const sk_cut_dev *>(cuts), n_pairs, classes, d + 2, ctx->cu_count, stream));
    return SK_OK;
}

int sk_count_pairs_device_finish(sk_ctx *ctx, void *hip_stream, sk_pair_counts *counts)
{
    if (!ctx || !counts) return SK_EINVAL;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    unsigned long long *d, *h;
    int rc = err_word_of(ctx, stream, &d, &h);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, hipMemcpyAsync(h + 2, d + 2, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    SK_HIP(ctx, hipMemsetAsync(d + 2, 0, 4 * sizeof(unsigned long long), stream));
    SK_HIP(ctx, hipStreamSynchronize(stream));
    counts->both = h[2];
    counts->only_first = h[3];
    counts->only_second = h[4];
    counts->none = h[5];
    return SK_OK;
}

size_t sk_trim_workspace_bytes(uint64_t n_reads)
{
    const uint64_t blocks = (n_reads + SK_TRIM_BLOCK_READS - 1) / SK_TRIM_BLOCK_READS;
    return (size_t)(8 * (SK_TRIM_HDR_WORDS + SK_TRIM_BLOCK_WORDS * blocks + n_reads));
}

int sk_trim_device_async(sk_ctx *ctx, const sk_batch *batch, const sk_cut *cuts, int mode, const sk_trim_output out[3],
                         void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!batch || !out) SK_BAD(ctx, "sk_trim_device_async: batch and out are required");
    // (packed reads have no name line to keep: the N records of SK_TRIM_PE_COMBO_ALL are the FASTQ text calls')
    if (mode == SK_TRIM_PE_COMBO_ALL) SK_BAD(ctx, "trim: SK_TRIM_PE_COMBO_ALL is a mode of the FASTQ text calls only");
    if (mode != SK_TRIM_SE && mode != SK_TRIM_PE_SPLIT && mode != SK_TRIM_PE_INTERLEAVED) SK_BAD(ctx, "trim mode %d is unknown", mode);
    const uint64_t n = batch->n_reads;
    if (batch->tiles) SK_BAD(ctx, "trim: segmented batches are not supported");
    if (mode != SK_TRIM_SE && (n & 1)) SK_BAD(ctx, "trim: a paired mode needs an even number of reads, not %llu", (unsigned long long)n);
    if (n && (!batch->qual || !cuts)) SK_BAD(ctx, "trim: qual and cuts are required");
    if (reinterpret_cast<uintptr_t>(cuts) & 7) SK_BAD(ctx, "trim: cuts must be 8-byte aligned");
    if (!batch->offsets) {
        if (batch->stride == 0 || (!batch->lengths && (batch->read_len > batch->stride || batch->read_len > SK_MAX_READ_LEN)))
            SK_BAD(ctx, "trim: fixed-stride batch: need stride >= read_len (<= %u), or lengths", SK_MAX_READ_LEN);
    }
    for (int o = 0; o < 3; ++o) {
        const bool used = o == 0 || (mode == SK_TRIM_PE_SPLIT && o == 1) || (mode != SK_TRIM_SE && o == 2);
        if (!used || !out[o].offsets) continue;
        if ((reinterpret_cast<uintptr_t>(out[o].qual) | reinterpret_cast<uintptr_t>(out[o].seq)) & 15)
            SK_BAD(ctx, "trim: out[%d].qual and out[%d].seq must be 16-byte aligned", o, o);
        if ((reinterpret_cast<uintptr_t>(out[o].offsets) | reinterpret_cast<uintptr_t>(out[o].read_index)) & 7)
            SK_BAD(ctx, "trim: out[%d].offsets and out[%d].read_index must be 8-byte aligned", o, o);
        if (n && out[o].seq && !batch->seq) SK_BAD(ctx, "trim: out[%d].seq needs batch->seq", o);
    }
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < sk_trim_workspace_bytes(n))
        SK_BAD(ctx, "trim: workspace must be 16-byte aligned and hold sk_trim_workspace_bytes(%llu) = %zu bytes",
               (unsigned long long)n, sk_trim_workspace_bytes(n));
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_trim(batch, reinterpret_cast<const sk_cut_dev *>(cuts), mode, out, workspace, ctx->cu_count,
                               static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

int sk_trim_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_trim_counts *counts)
{
    if (!ctx || !workspace || !counts) return SK_EINVAL;
    uint64_t h[SK_TRIM_HDR_WORDS];
    int rc = read_header(ctx, workspace, h, SK_TRIM_HDR_WORDS, static_cast<hipStream_t>(hip_stream));
    if (rc != SK_OK) return rc;
    for (int o = 0; o < 3; ++o) {
        counts->records[o] = h[SK_TRIM_H_RECORDS + o];
        counts->bytes[o] = h[SK_TRIM_H_BYTES + o];
        if (h[SK_TRIM_H_PRODUCED + o] && !h[SK_TRIM_H_FIT + o]) rc = SK_ESPACE;
    }
    counts->bad_read = h[SK_TRIM_H_BAD];
    if (counts->bad_read != UINT64_MAX) SK_BAD(ctx, "trim: read %llu has an invalid kept cut", (unsigned long long)counts->bad_read);
    if (rc == SK_ESPACE) set_error(ctx, "trim: an output's buffers are too small for what it needs");
    return rc;
}

size_t sk_trim_fastq_workspace_bytes(uint64_t text_bytes, int32_t trunc_n)
{
    sk_fq_layout L;
    sk_fq_layout_of(text_bytes, trunc_n, &L);
    return (size_t)L.total;
}

namespace {
// the argument checks of every FASTQ text call; extra = what an ordered call's batch table (and an ordered piece's block)
// adds to the workspace; clipped: the clip section follows (*kind_bytes: where)
int fastq_check_args(sk_ctx *ctx, const char *who, const sk_params *params, const sk_fastq_input *in, int mode,
                     const sk_fastq_output out[3], void *workspace, size_t workspace_bytes, size_t extra, bool clipped = false,
                     size_t *kind_bytes = nullptr)
{
    if (!ctx) return SK_EINVAL;
    if (!params || !in || !out) SK_BAD(ctx, "%s: params, in and out are required", who);
    if (mode != SK_TRIM_SE && mode != SK_TRIM_PE_SPLIT && mode != SK_TRIM_PE_INTERLEAVED && mode != SK_TRIM_PE_COMBO_ALL)
        SK_BAD(ctx, "trim mode %d is unknown", mode);
    const bool split = mode == SK_TRIM_PE_SPLIT;
    if (split && !in->text[1]) SK_BAD(ctx, "fastq: SK_TRIM_PE_SPLIT needs text[1]");
    if (!split && (in->text[1] || in->bytes[1])) SK_BAD(ctx, "fastq: text[1] is only for SK_TRIM_PE_SPLIT");
    for (int i = 0; i < (split ? 2 : 1); ++i)
        if (!in->text[i] && in->bytes[i]) SK_BAD(ctx, "fastq: text[%d] is NULL with %llu bytes", i, (unsigned long long)in->bytes[i]);
    for (int o = 0; o < 3; ++o) {
        if (reinterpret_cast<uintptr_t>(out[o].text) & 15) SK_BAD(ctx, "fastq: out[%d].text must be 16-byte aligned", o);
        if (reinterpret_cast<uintptr_t>(out[o].record_index) & 7) SK_BAD(ctx, "fastq: out[%d].record_index must be 8-byte aligned", o);
    }
    const uint64_t T = in->bytes[0] + (split ? in->bytes[1] : 0);
    if (sk_fq_pack_reads(in->bytes[0], split ? in->bytes[1] : 0, mode) >= (1ull << 32))
        SK_BAD(ctx, "fastq: %llu bytes of text is beyond what one call takes", (unsigned long long)T);
    // a clipped call: the clip section is the last bytes of the requirement, behind everything the kind lays out
    const size_t kind_need = sk_trim_fastq_workspace_bytes(T, params->trunc_n) + extra;
    const size_t need = kind_need + (clipped ? sk_trim_fastq_clip_extra_bytes(T) : 0);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < need)
        SK_BAD(ctx, "fastq: workspace must be 16-byte aligned and hold sk_trim_fastq%s_workspace_bytes(%llu, %d%s)%s = %zu bytes",
               extra ? "_ordered" : "", (unsigned long long)T, params->trunc_n, extra ? ", batch_capacity" : "",
               clipped ? " + sk_trim_fastq_clip_extra_bytes" : "", need);
    if (kind_bytes) *kind_bytes = kind_need;
    return SK_OK;
}

// Q of an N record of SK_TRIM_PE_COMBO_ALL: the quality type's lowest quality byte (reference src/sickle.h:85-91).  (The
// parameter checks of the scan have passed by the time this is called, so the type is known.)
int fastq_fail_qual(const sk_params *params)
{
    const int32_t *k = sk_quality_constants(params->qualtype);
    return k ? k[1] : 0;
}

// the device words of the chained and the piece calls
int fastq_check_words(sk_ctx *ctx, const sk_fastq_lengths *lengths, const sk_fastq_piece *piece, int mode)
{
    if (lengths) {
        uintptr_t words = 0;
        for (int i = 0; i < 2; ++i)
            words |= reinterpret_cast<uintptr_t>(lengths->bytes_dev[i]) | reinterpret_cast<uintptr_t>(lengths->valid_dev[i]);
        if (words & 7) SK_BAD(ctx, "fastq: bytes_dev and valid_dev must be 8-byte aligned");
        if (mode != SK_TRIM_PE_SPLIT && (lengths->bytes_dev[1] || lengths->valid_dev[1]))
            SK_BAD(ctx, "fastq: bytes_dev[1] and valid_dev[1] are only for SK_TRIM_PE_SPLIT");
    }
    if (piece) {
        if (piece->reserved != 0) SK_BAD(ctx, "fastq: piece->reserved must be 0");
        if ((reinterpret_cast<uintptr_t>(piece->start_dev[0]) | reinterpret_cast<uintptr_t>(piece->start_dev[1])) & 7)
            SK_BAD(ctx, "fastq: start_dev must be 8-byte aligned");
        if (mode != SK_TRIM_PE_SPLIT && piece->start_dev[1]) SK_BAD(ctx, "fastq: start_dev[1] is only for SK_TRIM_PE_SPLIT");
    }
    return SK_OK;
}

// the order of both ordered calls
int check_order(sk_ctx *ctx, const sk_fastq_order *order)
{
    if (!order || order->threads == 0 || order->reserved != 0 || order->batch_len < SK_FQO_MIN_BATCH_LEN ||
        order->batch_capacity == 0 || order->batch_capacity > (1ull << 40))
        SK_BAD(ctx, "fastq: order needs threads >= 1, reserved 0, batch_len >= 20 and 1 <= batch_capacity <= 2^40");
    return SK_OK;
}

// Every FASTQ text call: the checks, then the front, the counted scan and the emission.  lengths: NULL = in->bytes are the
// lengths; order: NULL = read order; piece: NULL = the whole text; state_out: not NULL = an ordered piece (piece and order
// given), whose launchers take the states.  clip: not NULL = the clipped call (its own checks have passed): the search in
// the front, the clip section behind the kind's workspace, the commit of its sums behind the emission.
int fastq_async(sk_ctx *ctx, const char *who, const sk_params *params, const sk_fastq_input *in,
                const sk_fastq_lengths *lengths, int mode, const sk_fastq_order *order, const sk_fastq_output out[3],
                void *workspace, size_t workspace_bytes, void *hip_stream, const sk_fastq_piece *piece = nullptr,
                const sk_fastq_order_state *state_in = nullptr, sk_fastq_order_state *state_out = nullptr,
                const sk_fastq_clip *clip = nullptr)
{
    const uint64_t extra = !order ? 0 : state_out ? sk_fq_order_piece_shift(order->batch_capacity) : sk_fq_order_shift(order->batch_capacity);
    size_t kind_bytes = 0;
    int rc = fastq_check_args(ctx, who, params, in, mode, out, workspace, workspace_bytes, (size_t)extra, clip != nullptr, &kind_bytes);
    if (rc != SK_OK) return rc;
    rc = fastq_check_words(ctx, lengths, piece, mode);
    if (rc != SK_OK) return rc;
    sk_scan_args chk;
    const uint64_t no_reads = 0;
    sk_batch probe = {};
    probe.offsets = &no_reads; // an empty `offsets` batch: only params is checked
    rc = make_args(ctx, params, &probe, &chk); // the parameter checks of the scan, before anything is enqueued
    if (rc != SK_OK) return rc;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    unsigned long long *d_err, *h_err;
    rc = err_word_of(ctx, stream, &d_err, &h_err);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, hipSetDevice(ctx->device));
    sk_batch packed;
    sk_cut_dev *cuts;
    // SK_FQ_COUNTED=0: the scan and the per-read steps walk the bound (the most records the text could hold) instead of
    // stopping at the records the framing found.  Read on every call, so that a probe can alternate the two in one process.
    const char *counted_env = getenv("SK_FQ_COUNTED");
    const int counted = !(counted_env && *counted_env == '0');
    const uint64_t *n_reads_dev = nullptr;
    sk_fq_clip_front clip_front = {};
    const sk_fq_clip_front *cf = nullptr;
    if (clip) {
        clip_front.set = clip->set;
        clip_front.section = static_cast<uint8_t *>(workspace) + kind_bytes;
        cf = &clip_front;
        if (clip->clip_words_dev)
            *clip->clip_words_dev = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(clip_front.section) + FQC_STATS_BYTES);
        if (clip->stats_dev && (clip->flags & SK_FQ_CLIP_RESET)) SK_HIP(ctx, sk_launch_fastq_clip_reset(clip->stats_dev, stream));
    }
    if (state_out)
        SK_HIP(ctx, sk_launch_fastq_order_piece_front(in, lengths, mode, params->trunc_n, counted, order, piece, state_in, state_out,
                                                      d_err, workspace, ctx->cu_count, stream, &packed, &cuts, &n_reads_dev, cf));
    else
        SK_HIP(ctx, sk_launch_fastq_front(in, lengths, mode, params->trunc_n, counted, order, piece, d_err, workspace, ctx->cu_count,
                                          stream, &packed, &cuts, &n_reads_dev, cf));
    rc = sk_scan_counted_device_async(ctx, params, &packed, n_reads_dev, reinterpret_cast<sk_cut *>(cuts), hip_stream);
    if (rc != SK_OK) return rc;
    if (state_out)
        SK_HIP(ctx, sk_launch_fastq_order_piece_emit(in, mode, params->trunc_n, counted, order, state_in, state_out,
                                                     fastq_fail_qual(params), out, workspace, d_err, ctx->cu_count, stream));
    else
        SK_HIP(ctx, sk_launch_fastq_emit(in, mode, params->trunc_n, counted, order, piece != nullptr, fastq_fail_qual(params), out,
                                         workspace, d_err, ctx->cu_count, stream));
    if (clip && clip->stats_dev) {
        const uint32_t kind = state_out ? SK_FQ_REPORT_ORDERED_PIECE : order ? SK_FQ_REPORT_ORDERED : piece ? SK_FQ_REPORT_PIECE : SK_FQ_REPORT_PLAIN;
        SK_HIP(ctx, sk_launch_fastq_clip_commit(workspace, kind, mode, clip_front.section, clip->stats_dev, stream));
    }
    return SK_OK;
}

// The finish of every FASTQ text call: the header back (with the block of the order words behind it for an ordered piece),
// the stream's live range-error word for the whole-text kinds, which judge it, the word cleared, one wait; then the
// verdict, a function of those words alone (sk_fastq_verdict.h).
int fastq_finish(sk_ctx *ctx, int kind, void *workspace, void *hip_stream, sk_fastq_counts *counts, sk_fastq_order_counts *oc,
                 sk_fastq_piece_counts *pc, sk_fastq_order_piece_counts *opc)
{
    if (!ctx || !workspace || !counts) return SK_EINVAL;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    unsigned long long *d_err, *h_err;
    int rc = err_word_of(ctx, stream, &d_err, &h_err);
    if (rc != SK_OK) return rc;
    uint64_t h[SK_FQ_HDR_WORDS + SK_FQOP_EXT_BYTES / 8];
    static_assert(SK_FQOP_EXT_BYTES_AT == 8 * SK_FQ_HDR_WORDS, "the block follows the header");
    const bool block = kind == SK_FQV_ORDERED_PIECE;
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, hipMemcpyAsync(h, workspace, block ? sizeof h : 8 * SK_FQ_HDR_WORDS, hipMemcpyDeviceToHost, stream));
    if (!fqv_is_piece(kind)) SK_HIP(ctx, hipMemcpyAsync(h_err, d_err, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    rc = reset_error_word(ctx, d_err, stream);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, hipStreamSynchronize(stream));
    return fqv_verdict(kind, h, block ? h + SK_FQ_HDR_WORDS : h, fqv_range_word(kind, h, *h_err), counts, oc, pc, opc,
                       ctx->last_error, sizeof ctx->last_error);
}
} // namespace

int sk_trim_fastq_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in, int mode,
                               const sk_fastq_output out[3], void *workspace, size_t workspace_bytes, void *hip_stream)
{
    return fastq_async(ctx, "sk_trim_fastq_device_async", params, in, nullptr, mode, nullptr, out, workspace, workspace_bytes,
                       hip_stream);
}

int sk_trim_fastq_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts)
{
    return fastq_finish(ctx, SK_FQV_PLAIN, workspace, hip_stream, counts, nullptr, nullptr, nullptr);
}

size_t sk_trim_fastq_ordered_workspace_bytes(uint64_t text_bytes, int32_t trunc_n, uint64_t batch_capacity)
{
    return sk_trim_fastq_workspace_bytes(text_bytes, trunc_n) + (size_t)sk_fq_order_shift(batch_capacity);
}

int sk_trim_fastq_ordered_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in, int mode,
                                       const sk_fastq_order *order, const sk_fastq_output out[3], void *workspace,
                                       size_t workspace_bytes, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (int rc = check_order(ctx, order)) return rc;
    return fastq_async(ctx, "sk_trim_fastq_ordered_device_async", params, in, nullptr, mode, order, out, workspace, workspace_bytes,
                       hip_stream);
}

// order: NULL = read order, else the ordered call with the lengths on the device
int sk_trim_fastq_chained_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in,
                                       const sk_fastq_lengths *lengths, int mode, const sk_fastq_order *order,
                                       const sk_fastq_output out[3], void *workspace, size_t workspace_bytes,
                                       void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (order)
        if (int rc = check_order(ctx, order)) return rc;
    return fastq_async(ctx, order ? "sk_trim_fastq_ordered_device_async" : "sk_trim_fastq_chained_device_async", params, in, lengths,
                       mode, order, out, workspace, workspace_bytes, hip_stream);
}

int sk_trim_fastq_piece_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in,
                                     const sk_fastq_lengths *lengths, const sk_fastq_piece *piece, int mode,
                                     const sk_fastq_output out[3], void *workspace, size_t workspace_bytes,
                                     void *hip_stream)
{
    return fastq_async(ctx, piece ? "sk_trim_fastq_piece_device_async" : "sk_trim_fastq_chained_device_async", params, in, lengths,
                       mode, nullptr, out, workspace, workspace_bytes, hip_stream, piece);
}

int sk_trim_fastq_piece_words(void *workspace, int input, const uint64_t **consumed_dev, const uint64_t **end_dev,
                              const uint64_t **ok_dev)
{
    if (!workspace || input < 0 || input > 1 || !consumed_dev || !end_dev || !ok_dev) return SK_EINVAL;
    const uint64_t *hdr = static_cast<const uint64_t *>(workspace);
    *consumed_dev = hdr + SK_FQP_H_CONSUMED + input;
    *end_dev = hdr + SK_FQP_H_END + input;
    *ok_dev = hdr + SK_FQP_H_OK;
    return SK_OK;
}

int sk_trim_fastq_piece_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts,
                                      sk_fastq_piece_counts *pc)
{
    return fastq_finish(ctx, SK_FQV_PIECE, workspace, hip_stream, counts, nullptr, pc, nullptr);
}

int sk_fastq_carry_device_async(sk_ctx *ctx, const void *prev_workspace, int input, const uint8_t *prev_text,
                                uint64_t prev_bytes, uint8_t *next_text, uint64_t room, const uint64_t *chunk_bytes_dev,
                                uint64_t chunk_bytes, const uint64_t *chunk_valid_dev,
                                const sk_fastq_carry_words *prev_words, const sk_fastq_carry_words *other_prev_words,
                                sk_fastq_carry_words *words, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!next_text || !words) SK_BAD(ctx, "carry: next_text and words are required");
    if (input < 0 || input > 1) SK_BAD(ctx, "carry: input is 0 or 1");
    if (prev_workspace && !prev_text) SK_BAD(ctx, "carry: prev_text is required with prev_workspace");
    if (room & 15) SK_BAD(ctx, "carry: room must be a multiple of 16");
    uintptr_t w = reinterpret_cast<uintptr_t>(chunk_bytes_dev) | reinterpret_cast<uintptr_t>(chunk_valid_dev) |
                  reinterpret_cast<uintptr_t>(prev_words) | reinterpret_cast<uintptr_t>(other_prev_words) |
                  reinterpret_cast<uintptr_t>(words) | reinterpret_cast<uintptr_t>(prev_workspace);
    if (w & 7) SK_BAD(ctx, "carry: the device words and prev_workspace must be 8-byte aligned");
    if (words == prev_words || words == other_prev_words) SK_BAD(ctx, "carry: words must not be one of the previous words");
    if (prev_workspace) {
        const uintptr_t p0 = reinterpret_cast<uintptr_t>(prev_text), p1 = p0 + prev_bytes;
        const uintptr_t n0 = reinterpret_cast<uintptr_t>(next_text), n1 = n0 + room;
        if (p0 < n1 && n0 < p1) SK_BAD(ctx, "carry: [next_text, next_text + room) overlaps the previous text");
    }
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_fastq_carry(static_cast<const uint64_t *>(prev_workspace), input, prev_text, next_text, room,
                                      chunk_bytes_dev, chunk_bytes, chunk_valid_dev, prev_words, other_prev_words, words,
                                      static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

int sk_trim_fastq_ordered_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts,
                                        sk_fastq_order_counts *order_counts)
{
    return fastq_finish(ctx, SK_FQV_ORDERED, workspace, hip_stream, counts, order_counts, nullptr, nullptr);
}

int sk_trim_fastq_ordered_batches(void *workspace, const uint64_t **first_unit_dev)
{
    if (!workspace || !first_unit_dev) return SK_EINVAL;
    *first_unit_dev = reinterpret_cast<const uint64_t *>(static_cast<const uint8_t *>(workspace) + SK_FQO_TABLE_BYTES_AT);
    return SK_OK;
}

// ---- ordered pieces ----
size_t sk_trim_fastq_ordered_piece_workspace_bytes(uint64_t text_bytes, int32_t trunc_n, uint64_t batch_capacity)
{
    return sk_trim_fastq_ordered_workspace_bytes(text_bytes, trunc_n, batch_capacity) + SK_FQOP_EXT_BYTES;
}

int sk_trim_fastq_ordered_piece_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in,
                                             const sk_fastq_lengths *lengths, const sk_fastq_piece *piece,
                                             const sk_fastq_order *order, const sk_fastq_order_state *state_in,
                                             sk_fastq_order_state *state_out, int mode, const sk_fastq_output out[3],
                                             void *workspace, size_t workspace_bytes, void *hip_stream)
{
    static_assert(sizeof(sk_fastq_order_state) == 64, "the kernels read the state as 8 words");
    if (!ctx) return SK_EINVAL;
    if (!piece || !order || !state_out) SK_BAD(ctx, "fastq: an ordered piece needs piece, order and state_out");
    if (int rc = check_order(ctx, order)) return rc;
    if (state_in == state_out || ((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 7))
        SK_BAD(ctx, "fastq: state_in and state_out must be 8-byte aligned and differ");
    return fastq_async(ctx, "sk_trim_fastq_ordered_piece_device_async", params, in, lengths, mode, order, out, workspace,
                       workspace_bytes, hip_stream, piece, state_in, state_out);
}

int sk_trim_fastq_ordered_piece_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts,
                                              sk_fastq_order_counts *oc, sk_fastq_piece_counts *pc,
                                              sk_fastq_order_piece_counts *opc)
{
    return fastq_finish(ctx, SK_FQV_ORDERED_PIECE, workspace, hip_stream, counts, oc, pc, opc);
}

// ---- the clipped call: every kind through the one front ----
size_t sk_trim_fastq_clip_extra_bytes(uint64_t text_bytes) { return (size_t)fqc_extra_bytes(text_bytes); }

int sk_trim_fastq_clipped_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in, const sk_fastq_clip *clip,
                                       int mode, const sk_fastq_output out[3], void *workspace, size_t workspace_bytes,
                                       void *hip_stream)
{
    static_assert(sizeof(sk_fastq_clip_stats) == 128, "the kernels add the stats as 16 words");
    if (!ctx) return SK_EINVAL;
    if (!clip || !clip->set) SK_BAD(ctx, "clip: clip and clip->set are required");
    if (const char *why = fqd_set_error(clip->set)) SK_BAD(ctx, "clip: set: %s", why);
    if (clip->reserved != 0) SK_BAD(ctx, "clip: reserved must be 0");
    if (clip->flags & ~SK_FQ_CLIP_RESET) SK_BAD(ctx, "clip: flags %u are unknown", clip->flags);
    if (reinterpret_cast<uintptr_t>(clip->stats_dev) & 7) SK_BAD(ctx, "clip: stats_dev must be 8-byte aligned");
    const char *who = "sk_trim_fastq_clipped_device_async";
    if (clip->state_out || clip->state_in) { // the ordered piece's own checks
        if (!clip->piece || !clip->order || !clip->state_out) SK_BAD(ctx, "fastq: an ordered piece needs piece, order and state_out");
        if (clip->state_in == clip->state_out ||
            ((reinterpret_cast<uintptr_t>(clip->state_in) | reinterpret_cast<uintptr_t>(clip->state_out)) & 7))
            SK_BAD(ctx, "fastq: state_in and state_out must be 8-byte aligned and differ");
    } else if (clip->piece && clip->order) {
        SK_BAD(ctx, "fastq: an ordered piece needs piece, order and state_out");
    }
    if (clip->order)
        if (int rc = check_order(ctx, clip->order)) return rc;
    return fastq_async(ctx, who, params, in, clip->lengths, mode, clip->order, out, workspace, workspace_bytes, hip_stream, clip->piece,
                       clip->state_in, clip->state_out, clip);
}

int sk_bgzf_inflate_output_words(void *workspace, const uint64_t **bytes_dev, const uint64_t **written_dev)
{
    if (!workspace || !bytes_dev || !written_dev) return SK_EINVAL;
    const uint64_t *hdr = static_cast<const uint64_t *>(workspace);
    *bytes_dev = hdr + SK_INFLATE_H_BYTES_OUT;
    *written_dev = hdr + SK_INFLATE_H_WRITTEN;
    return SK_OK;
}

int sk_gzip_inflate_output_words(void *workspace, const uint64_t **bytes_dev, const uint64_t **written_dev)
{
    if (!workspace || !bytes_dev || !written_dev) return SK_EINVAL;
    const uint64_t *hdr = static_cast<const uint64_t *>(workspace);
    *bytes_dev = hdr + SK_GUNZIP_H_BYTES_OUT;
    *written_dev = hdr + SK_GUNZIP_H_WRITTEN;
    return SK_OK;
}

int sk_trim_fastq_output_words(void *fastq_workspace, int output, const uint64_t **bytes_dev, const uint64_t **written_dev)
{
    if (!fastq_workspace || output < 0 || output > 2 || !bytes_dev || !written_dev) return SK_EINVAL;
    const uint64_t *hdr = static_cast<const uint64_t *>(fastq_workspace);
    *bytes_dev = hdr + SK_FQ_H_OUT_BYTES + output;
    *written_dev = hdr + SK_FQ_H_FIT + output;
    return SK_OK;
}

namespace {
// The calls that go behind a text call (report, audit, bases, rejects; who: "report:" ..) check every argument before the
// first HIP call: bad arguments enqueue nothing and need no device.
// the source, once the caller has seen that src and src->workspace are there
int check_source(sk_ctx *ctx, const char *who, const sk_fastq_report_source *src)
{
    if (reinterpret_cast<uintptr_t>(src->workspace) & 15) SK_BAD(ctx, "%s src->workspace must be 16-byte aligned", who);
    if (src->kind > SK_FQ_REPORT_ORDERED_PIECE) SK_BAD(ctx, "%s source kind %u is unknown", who, src->kind);
    if (src->reserved != 0) SK_BAD(ctx, "%s src->reserved must be 0", who);
    return SK_OK;
}

// the mode, and the texts against it (in: NULL = no texts, where the caller allows that).  text0_in_se: an SE call reads
// text[0] too (the audit looks at the names of pairs alone)
int check_texts(sk_ctx *ctx, const char *who, const sk_fastq_input *in, int mode, bool text0_in_se)
{
    if (mode < SK_TRIM_SE || mode > SK_TRIM_PE_COMBO_ALL) SK_BAD(ctx, "%s mode %d is unknown", who, mode);
    if (!in) return SK_OK;
    if (mode == SK_TRIM_PE_SPLIT && !in->text[1]) SK_BAD(ctx, "%s SK_TRIM_PE_SPLIT needs text[1]", who);
    if (mode != SK_TRIM_PE_SPLIT && in->text[1]) SK_BAD(ctx, "%s text[1] is for SK_TRIM_PE_SPLIT only", who);
    if ((text0_in_se || mode != SK_TRIM_SE) && !in->text[0] && in->bytes[0]) SK_BAD(ctx, "%s text[0] is NULL with bytes[0] != 0", who);
    return SK_OK;
}
} // namespace

int sk_trim_fastq_report_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, sk_fastq_report *report_dev,
                                      const sk_fastq_report_hists *hists, int flags, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!src || !src->workspace || !report_dev) SK_BAD(ctx, "report: src, src->workspace and report_dev are required");
    if (int rc = check_source(ctx, "report:", src)) return rc;
    if (reinterpret_cast<uintptr_t>(report_dev) & 7) SK_BAD(ctx, "report: report_dev must be 8-byte aligned");
    if (flags & ~SK_FQ_REPORT_RESET) SK_BAD(ctx, "report: flags %d are unknown", flags);
    if (hists) {
        const uintptr_t len = reinterpret_cast<uintptr_t>(hists->len_in) | reinterpret_cast<uintptr_t>(hists->len_out);
        const uintptr_t pos = reinterpret_cast<uintptr_t>(hists->qsum_in) | reinterpret_cast<uintptr_t>(hists->qcnt_in) |
                              reinterpret_cast<uintptr_t>(hists->qsum_out) | reinterpret_cast<uintptr_t>(hists->qcnt_out);
        if ((len | pos) & 7) SK_BAD(ctx, "report: the histogram arrays must be 8-byte aligned");
        if (len && hists->len_bins == 0) SK_BAD(ctx, "report: len_bins is 0 with a length array given");
        if (pos && hists->pos_bins == 0) SK_BAD(ctx, "report: pos_bins is 0 with a position array given");
        if (hists->len_bins > SK_FQ_REPORT_MAX_LEN_BINS)
            SK_BAD(ctx, "report: len_bins %llu is above SK_FQ_REPORT_MAX_LEN_BINS = %u", (unsigned long long)hists->len_bins,
                   SK_FQ_REPORT_MAX_LEN_BINS);
        if (hists->pos_bins > SK_FQ_REPORT_MAX_POS_BINS)
            SK_BAD(ctx, "report: pos_bins %llu is above SK_FQ_REPORT_MAX_POS_BINS = %u", (unsigned long long)hists->pos_bins,
                   SK_FQ_REPORT_MAX_POS_BINS);
    }
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_fastq_report(src, report_dev, hists, flags, static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

// in: NULL = the names are not looked at
int sk_trim_fastq_audit_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                     sk_fastq_audit *audit_dev, uint64_t *qual_hist_dev, int flags, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!src || !src->workspace || !audit_dev) SK_BAD(ctx, "audit: src, src->workspace and audit_dev are required");
    if (int rc = check_source(ctx, "audit:", src)) return rc;
    if (reinterpret_cast<uintptr_t>(audit_dev) & 7) SK_BAD(ctx, "audit: audit_dev must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(qual_hist_dev) & 7) SK_BAD(ctx, "audit: qual_hist_dev must be 8-byte aligned");
    if (flags & ~SK_FQ_AUDIT_RESET) SK_BAD(ctx, "audit: flags %d are unknown", flags);
    if (int rc = check_texts(ctx, "audit:", in, mode, false)) return rc;
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_fastq_audit(src, in, mode, audit_dev, qual_hist_dev, flags, static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

// the texts are the data: in is required
int sk_trim_fastq_bases_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                     sk_fastq_bases *bases_dev, const sk_fastq_bases_hists *hists, int flags, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!src || !src->workspace || !bases_dev || !in) SK_BAD(ctx, "bases: src, src->workspace, bases_dev and in are required");
    if (int rc = check_source(ctx, "bases:", src)) return rc;
    if (reinterpret_cast<uintptr_t>(bases_dev) & 7) SK_BAD(ctx, "bases: bases_dev must be 8-byte aligned");
    if (flags & ~SK_FQ_BASES_RESET) SK_BAD(ctx, "bases: flags %d are unknown", flags);
    if (int rc = check_texts(ctx, "bases:", in, mode, true)) return rc;
    if (hists) {
        const uintptr_t pos = reinterpret_cast<uintptr_t>(hists->pos_in) | reinterpret_cast<uintptr_t>(hists->pos_out);
        const uintptr_t gc = reinterpret_cast<uintptr_t>(hists->gc_in) | reinterpret_cast<uintptr_t>(hists->gc_out);
        if ((pos | gc) & 7) SK_BAD(ctx, "bases: the arrays must be 8-byte aligned");
        if (pos && hists->pos_bins == 0) SK_BAD(ctx, "bases: pos_bins is 0 with a position array given");
        if (hists->pos_bins > SK_FQ_BASES_MAX_POS_BINS)
            SK_BAD(ctx, "bases: pos_bins %llu is above SK_FQ_BASES_MAX_POS_BINS = %u", (unsigned long long)hists->pos_bins,
                   SK_FQ_BASES_MAX_POS_BINS);
    }
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_fastq_bases(src, in, mode, bases_dev, hists, flags, static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

// the texts are the data: in is required; the set is read here, on the host
int sk_trim_fastq_adapters_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                        const sk_fastq_adapter_set *set, sk_fastq_adapters *adapters_dev,
                                        const sk_fastq_adapters_out *out, int flags, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!src || !src->workspace || !adapters_dev || !in || !set)
        SK_BAD(ctx, "adapters: src, src->workspace, adapters_dev, in and set are required");
    if (int rc = check_source(ctx, "adapters:", src)) return rc;
    if (reinterpret_cast<uintptr_t>(adapters_dev) & 7) SK_BAD(ctx, "adapters: adapters_dev must be 8-byte aligned");
    if (flags & ~SK_FQ_ADAPTERS_RESET) SK_BAD(ctx, "adapters: flags %d are unknown", flags);
    if (int rc = check_texts(ctx, "adapters:", in, mode, true)) return rc;
    if (const char *why = fqd_set_error(set)) SK_BAD(ctx, "adapters: set: %s", why);
    if (out) {
        if ((reinterpret_cast<uintptr_t>(out->pos) | reinterpret_cast<uintptr_t>(out->overlap)) & 7)
            SK_BAD(ctx, "adapters: pos and overlap must be 8-byte aligned");
        if (out->pos && out->pos_bins == 0) SK_BAD(ctx, "adapters: pos_bins is 0 with pos given");
        if (out->pos_bins > SK_FQ_ADAPTERS_MAX_POS_BINS)
            SK_BAD(ctx, "adapters: pos_bins %llu is above SK_FQ_ADAPTERS_MAX_POS_BINS = %u", (unsigned long long)out->pos_bins,
                   SK_FQ_ADAPTERS_MAX_POS_BINS);
        if (reinterpret_cast<uintptr_t>(out->clip) & 3) SK_BAD(ctx, "adapters: clip must be 4-byte aligned");
        if (out->clip && out->clip_capacity == 0) SK_BAD(ctx, "adapters: clip_capacity is 0 with clip given");
    }
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_fastq_adapters(src, in, mode, set, adapters_dev, out, flags, ctx->cu_count,
                                         static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

size_t sk_trim_fastq_rejects_workspace_bytes(uint64_t text_bytes) { return (size_t)fqj_workspace_bytes(text_bytes); }

uint64_t sk_trim_fastq_rejects_bound(uint64_t text_bytes) { return fqj_bound(text_bytes); }

int sk_trim_fastq_rejects_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                       const sk_fastq_output *out, int flags, void *workspace, size_t workspace_bytes,
                                       void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!src || !src->workspace || !in || !workspace) SK_BAD(ctx, "rejects: src, src->workspace, in and workspace are required");
    if (int rc = check_source(ctx, "rejects:", src)) return rc;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) SK_BAD(ctx, "rejects: workspace must be 16-byte aligned");
    if (out && (reinterpret_cast<uintptr_t>(out->text) & 15)) SK_BAD(ctx, "rejects: out->text must be 16-byte aligned");
    if (out && (reinterpret_cast<uintptr_t>(out->record_index) & 7)) SK_BAD(ctx, "rejects: out->record_index must be 8-byte aligned");
    if (int rc = check_texts(ctx, "rejects:", in, mode, true)) return rc;
    if (flags & ~SK_FQ_REJECTS_PAIRS) SK_BAD(ctx, "rejects: flags %d are unknown", flags);
    if ((flags & SK_FQ_REJECTS_PAIRS) && mode == SK_TRIM_SE) SK_BAD(ctx, "rejects: SK_FQ_REJECTS_PAIRS needs a pair mode");
    if (!in->text[1] && in->bytes[1]) SK_BAD(ctx, "rejects: text[1] is NULL with bytes[1] != 0"); // (in every mode)
    if (src->text_bytes > (1ull << 35)) SK_BAD(ctx, "rejects: %llu bytes of text is beyond what a text call takes", (unsigned long long)src->text_bytes);
    const size_t need = sk_trim_fastq_rejects_workspace_bytes(src->text_bytes);
    if (workspace_bytes < need)
        SK_BAD(ctx, "rejects: workspace must hold sk_trim_fastq_rejects_workspace_bytes(%llu) = %zu bytes",
               (unsigned long long)src->text_bytes, need);
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_fastq_rejects(src, in, mode, out, flags, workspace, ctx->cu_count, static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

int sk_trim_fastq_rejects_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_rejects_counts *counts)
{
    if (!ctx || !workspace || !counts) return SK_EINVAL;
    uint64_t h[FQJ_HDR_WORDS];
    if (int rc = read_header(ctx, workspace, h, FQJ_HDR_WORDS, static_cast<hipStream_t>(hip_stream))) return rc;
    counts->records = h[FQJ_H_RECORDS];
    counts->bytes = h[FQJ_H_BYTES];
    counts->reads = h[FQJ_H_READS];
    counts->valid = (uint32_t)h[FQJ_H_VALID];
    counts->flags = (uint32_t)h[FQJ_H_FLAGS];
    if (h[FQJ_H_VALID] && h[FQJ_H_PRODUCED] && !h[FQJ_H_WRITTEN]) {
        set_error(ctx, "rejects: the text needs %llu bytes and %llu records, more than a capacity",
                  (unsigned long long)counts->bytes, (unsigned long long)counts->records);
        return SK_ESPACE;
    }
    return SK_OK;
}

int sk_trim_fastq_rejects_output_words(void *rejects_workspace, const uint64_t **bytes_dev, const uint64_t **written_dev)
{
    if (!rejects_workspace || !bytes_dev || !written_dev) return SK_EINVAL;
    const uint64_t *hdr = static_cast<const uint64_t *>(rejects_workspace);
    *bytes_dev = hdr + FQJ_H_OUT_BYTES;
    *written_dev = hdr + FQJ_H_WRITTEN;
    return SK_OK;
}

uint64_t sk_bgzf_bound(uint64_t text_bytes, int flags)
{
    sk_bgzf_layout L;
    sk_bgzf_layout_of(text_bytes, &L);
    return text_bytes + SK_BGZF_MEMBER_EXTRA * L.n_blocks + ((flags & SK_BGZF_EOF) ? SK_BGZF_EOF_BYTES : 0);
}

size_t sk_bgzf_workspace_bytes(uint64_t text_bytes)
{
    sk_bgzf_layout L;
    sk_bgzf_layout_of(text_bytes, &L);
    return (size_t)L.total;
}

size_t sk_bgzf_workspace_bytes_flags(uint64_t text_bytes, int flags)
{
    sk_bgzf_layout L;
    sk_bgzf_layout_of(text_bytes, &L);
    return (size_t)(L.total + ((flags & SK_BGZF_SEARCH) ? sk_bgzf_search_bytes(&L) : 0));
}

int sk_bgzf_device_async(sk_ctx *ctx, const sk_bgzf_input *in, uint8_t *out, uint64_t capacity, int flags, void *workspace,
                         size_t workspace_bytes, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!in) SK_BAD(ctx, "sk_bgzf_device_async: in is required");
    if (flags & ~(SK_BGZF_EOF | SK_BGZF_SEARCH)) SK_BAD(ctx, "bgzf: flags %d are unknown", flags);
    if (!in->text && in->bytes) SK_BAD(ctx, "bgzf: text is NULL with %llu bytes", (unsigned long long)in->bytes);
    if ((reinterpret_cast<uintptr_t>(in->bytes_dev) | reinterpret_cast<uintptr_t>(in->valid_dev)) & 7)
        SK_BAD(ctx, "bgzf: bytes_dev and valid_dev must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & 15) SK_BAD(ctx, "bgzf: out must be 16-byte aligned");
    if (!out && capacity) SK_BAD(ctx, "bgzf: out is NULL with a capacity of %llu bytes", (unsigned long long)capacity);
    if (in->bytes > (1ull << 60)) SK_BAD(ctx, "bgzf: %llu bytes of text is beyond what one call takes", (unsigned long long)in->bytes);
    const size_t need = sk_bgzf_workspace_bytes_flags(in->bytes, flags);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < need)
        SK_BAD(ctx, "bgzf: workspace must be 16-byte aligned and hold sk_bgzf_workspace_bytes_flags(%llu, %d) = %zu bytes",
               (unsigned long long)in->bytes, flags, need);
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_bgzf(in, out, capacity, flags, workspace, ctx->cu_count, static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

int sk_bgzf_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_bgzf_counts *counts)
{
    if (!ctx || !workspace || !counts) return SK_EINVAL;
    uint64_t h[SK_BGZF_HDR_WORDS];
    if (int rc = read_header(ctx, workspace, h, SK_BGZF_HDR_WORDS, static_cast<hipStream_t>(hip_stream))) return rc;
    counts->bytes_in = h[SK_BGZF_H_BYTES_IN];
    counts->blocks = h[SK_BGZF_H_BLOCKS];
    counts->stored_blocks = h[SK_BGZF_H_STORED];
    counts->bytes_out = h[SK_BGZF_H_BYTES_OUT];
    if (!h[SK_BGZF_H_FIT]) {
        set_error(ctx, "bgzf: the image needs %llu bytes, more than the capacity", (unsigned long long)counts->bytes_out);
        return SK_ESPACE;
    }
    return SK_OK;
}

size_t sk_bgzf_inflate_workspace_bytes(uint64_t image_bytes)
{
    sk_inflate_layout L;
    sk_inflate_layout_of(image_bytes, &L);
    return (size_t)L.total;
}

int sk_bgzf_inflate_device_async(sk_ctx *ctx, const uint8_t *image, uint64_t image_bytes, uint8_t *out, uint64_t capacity,
                                 void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!image && image_bytes) SK_BAD(ctx, "bgzf inflate: image is NULL with %llu bytes", (unsigned long long)image_bytes);
    if (image_bytes > SK_INFLATE_MAX_IMAGE)
        SK_BAD(ctx, "bgzf inflate: an image of %llu bytes is beyond what one call takes (8 GiB)", (unsigned long long)image_bytes);
    if (reinterpret_cast<uintptr_t>(out) & 15) SK_BAD(ctx, "bgzf inflate: out must be 16-byte aligned");
    if (!out && capacity) SK_BAD(ctx, "bgzf inflate: out is NULL with a capacity of %llu bytes", (unsigned long long)capacity);
    const size_t need = sk_bgzf_inflate_workspace_bytes(image_bytes);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < need)
        SK_BAD(ctx, "bgzf inflate: workspace must be 16-byte aligned and hold sk_bgzf_inflate_workspace_bytes(%llu) = %zu bytes",
               (unsigned long long)image_bytes, need);
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_bgzf_inflate(image, image_bytes, out, capacity, workspace, static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

int sk_bgzf_inflate_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_bgzf_inflate_counts *counts)
{
    if (!ctx || !workspace || !counts) return SK_EINVAL;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    uint64_t h[SK_INFLATE_HDR_WORDS];
    if (int rc = read_header(ctx, workspace, h, SK_INFLATE_HDR_WORDS, stream)) return rc;
    memset(counts, 0, sizeof *counts);
    counts->bytes_in = h[SK_INFLATE_H_BYTES_IN];
    counts->members = h[SK_INFLATE_H_MEMBERS];
    counts->bytes_out = h[SK_INFLATE_H_BYTES_OUT];
    const uint64_t key = h[SK_INFLATE_H_ERROR_KEY];
    if (key != ~0ull) {
        counts->error = (int32_t)(key & 7);
        counts->error_member = key >> 3;
        if (key == h[SK_INFLATE_H_FRAME_KEY]) {
            counts->error_offset = h[SK_INFLATE_H_FRAME_OFFSET];
        } else { // a member that framed: its offset is in the table
            sk_inflate_layout L;
            sk_inflate_layout_of(counts->bytes_in, &L);
            const uint8_t *entry = static_cast<const uint8_t *>(workspace) + L.table + sizeof(sk_inflate_entry) * counts->error_member;
            SK_HIP(ctx, hipMemcpyAsync(&counts->error_offset, entry, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
            SK_HIP(ctx, hipStreamSynchronize(stream));
        }
        set_error(ctx, "bgzf inflate: member %llu at byte %llu is not valid BGZF (reason %d)",
                  (unsigned long long)counts->error_member, (unsigned long long)counts->error_offset, counts->error);
        return SK_EDATA;
    }
    if (!h[SK_INFLATE_H_FIT]) {
        set_error(ctx, "bgzf inflate: the text needs %llu bytes, more than the capacity", (unsigned long long)counts->bytes_out);
        return SK_ESPACE;
    }
    return SK_OK;
}

// SK_GZIP_CHUNK: a power of two of 256 or more, else 0 (the chunk follows the image's size)
static uint64_t gzip_forced_chunk()
{
    const char *e = getenv("SK_GZIP_CHUNK");
    if (!e || !*e) return 0;
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 10);
    if (*end || v < 256 || v > (1ull << 40) || (v & (v - 1))) return 0;
    return v;
}

size_t sk_gzip_inflate_workspace_bytes(uint64_t image_bytes, uint64_t capacity)
{
    sk_gunzip_layout L;
    sk_gunzip_layout_of(image_bytes, capacity, gzip_forced_chunk(), &L);
    return (size_t)L.total;
}

int sk_gzip_inflate_device_async(sk_ctx *ctx, const uint8_t *image, uint64_t image_bytes, uint8_t *out, uint64_t capacity,
                                 void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!image && image_bytes) SK_BAD(ctx, "gzip inflate: image is NULL with %llu bytes", (unsigned long long)image_bytes);
    if (image_bytes > SK_GUNZIP_MAX_IMAGE)
        SK_BAD(ctx, "gzip inflate: an image of %llu bytes is beyond what one call takes (8 GiB)", (unsigned long long)image_bytes);
    if (reinterpret_cast<uintptr_t>(out) & 15) SK_BAD(ctx, "gzip inflate: out must be 16-byte aligned");
    if (!out && capacity) SK_BAD(ctx, "gzip inflate: out is NULL with a capacity of %llu bytes", (unsigned long long)capacity);
    if (capacity > (1ull << 60)) SK_BAD(ctx, "gzip inflate: a capacity of %llu bytes", (unsigned long long)capacity);
    const uint64_t forced = gzip_forced_chunk();
    sk_gunzip_layout L;
    sk_gunzip_layout_of(image_bytes, capacity, forced, &L);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < L.total)
        SK_BAD(ctx, "gzip inflate: workspace must be 16-byte aligned and hold sk_gzip_inflate_workspace_bytes(%llu, %llu) = %llu bytes",
               (unsigned long long)image_bytes, (unsigned long long)capacity, (unsigned long long)L.total);
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_gunzip(image, image_bytes, out, capacity, forced, workspace, static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

// how both gzip finishes begin: the header (words: SKG_H_* of sk_gunzip_block.h) and the counts every call has
static int gzip_finish_head(sk_ctx *ctx, void *workspace, void *hip_stream, uint64_t h[SK_GUNZIP_HDR_WORDS],
                            sk_gzip_inflate_counts *counts)
{
    int rc = read_header(ctx, workspace, h, SK_GUNZIP_HDR_WORDS, static_cast<hipStream_t>(hip_stream));
    if (rc != SK_OK) return rc;
    memset(counts, 0, sizeof *counts);
    counts->bytes_in = h[SKG_H_BYTES_IN];
    counts->members = h[SKG_H_MEMBERS];
    counts->bytes_out = h[SKG_H_BYTES_OUT];
    counts->stretches = h[SKG_H_STRETCHES];
    counts->stretches_used = h[SKG_H_USED];
    return SK_OK;
}

int sk_gzip_inflate_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_gzip_inflate_counts *counts)
{
    if (!ctx || !workspace || !counts) return SK_EINVAL;
    uint64_t h[SK_GUNZIP_HDR_WORDS];
    if (int rc = gzip_finish_head(ctx, workspace, hip_stream, h, counts)) return rc;
    const uint64_t key = h[SKG_H_ERROR_KEY];
    if (key != ~0ull) {
        counts->error = (int32_t)(key & 7);
        counts->error_member = key >> 3;
        counts->error_offset = h[SKG_H_ERROR_OFFSET];
        set_error(ctx, "gzip inflate: member %llu is not valid gzip at byte %llu (reason %d)",
                  (unsigned long long)counts->error_member, (unsigned long long)counts->error_offset, counts->error);
        return SK_EDATA;
    }
    if (!h[SKG_H_FIT]) {
        set_error(ctx, "gzip inflate: the text needs %llu bytes, more than the capacity", (unsigned long long)counts->bytes_out);
        return SK_ESPACE;
    }
    return SK_OK;
}

size_t sk_gzip_inflate_piece_workspace_bytes(uint64_t window_bytes, uint64_t capacity)
{
    sk_gunzip_piece_layout L;
    sk_gunzip_piece_layout_of(window_bytes, capacity, gzip_forced_chunk(), &L);
    return (size_t)L.total;
}

int sk_gzip_inflate_piece_device_async(sk_ctx *ctx, const uint8_t *image, uint64_t image_bytes, const sk_gzip_piece *piece,
                                       const sk_gzip_piece_state *state_in, sk_gzip_piece_state *state_out, uint8_t *out,
                                       uint64_t capacity, void *workspace, size_t workspace_bytes, void *hip_stream)
{
    if (!ctx) return SK_EINVAL;
    if (!piece || !state_in || !state_out) SK_BAD(ctx, "gzip piece: piece, state_in or state_out is NULL");
    if (!image && image_bytes) SK_BAD(ctx, "gzip piece: image is NULL with %llu bytes", (unsigned long long)image_bytes);
    if (static_cast<const void *>(state_in) == static_cast<const void *>(state_out))
        SK_BAD(ctx, "gzip piece: state_out is state_in (pieces alternate two states)");
    if ((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out)) & 15)
        SK_BAD(ctx, "gzip piece: the states must be 16-byte aligned");
    if (piece->reserved) SK_BAD(ctx, "gzip piece: reserved must be 0");
    if (piece->window_bytes == 0 || piece->window_bytes > SK_GUNZIP_MAX_WINDOW)
        SK_BAD(ctx, "gzip piece: a window of %llu bytes (1 .. 8 GiB)", (unsigned long long)piece->window_bytes);
    if (!out || (reinterpret_cast<uintptr_t>(out) & 15)) SK_BAD(ctx, "gzip piece: out must be 16-byte aligned and not NULL");
    if (capacity > (1ull << 60)) SK_BAD(ctx, "gzip piece: a capacity of %llu bytes", (unsigned long long)capacity);
    const uint64_t forced = gzip_forced_chunk();
    sk_gunzip_piece_layout L;
    sk_gunzip_piece_layout_of(piece->window_bytes, capacity, forced, &L);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < L.total)
        SK_BAD(ctx, "gzip piece: workspace must be 16-byte aligned and hold sk_gzip_inflate_piece_workspace_bytes(%llu, %llu) = %llu bytes",
               (unsigned long long)piece->window_bytes, (unsigned long long)capacity, (unsigned long long)L.total);
    SK_HIP(ctx, hipSetDevice(ctx->device));
    SK_HIP(ctx, sk_launch_gunzip_piece(image, image_bytes, piece, state_in, state_out, out, capacity, forced, workspace,
                                       static_cast<hipStream_t>(hip_stream)));
    return SK_OK;
}

int sk_gzip_inflate_piece_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_gzip_inflate_counts *counts,
                                        sk_gzip_piece_counts *piece_counts)
{
    if (!ctx || !workspace || !counts || !piece_counts) return SK_EINVAL;
    uint64_t h[SK_GUNZIP_HDR_WORDS];
    if (int rc = gzip_finish_head(ctx, workspace, hip_stream, h, counts)) return rc;
    memset(piece_counts, 0, sizeof *piece_counts);
    piece_counts->pos_bit = h[SK_GUNZIP_H_P_POS_BIT];
    piece_counts->in_member = h[SK_GUNZIP_H_P_IN_MEMBER];
    if ((h[SK_GUNZIP_H_P_POS_BIT] >> 3) >= h[SK_GUNZIP_H_P_IMAGE_OFFSET])
        piece_counts->image_bytes_consumed = (h[SK_GUNZIP_H_P_POS_BIT] >> 3) - h[SK_GUNZIP_H_P_IMAGE_OFFSET];
    piece_counts->inherited = (uint32_t)h[SK_GUNZIP_H_P_INHERITED];
    piece_counts->done = (uint32_t)h[SK_GUNZIP_H_P_DONE];
    const uint64_t status = h[SK_GUNZIP_H_P_STATUS];
    if (status == 1) {
        counts->error = (int32_t)h[SK_GUNZIP_H_P_ERROR];
        counts->error_member = h[SK_GUNZIP_H_P_ERROR_MEMBER];
        counts->error_offset = h[SK_GUNZIP_H_P_ERROR_OFFSET];
        piece_counts->window_limited = (uint32_t)(h[SK_GUNZIP_H_P_LIMITED] && !piece_counts->inherited);
        set_error(ctx, "gzip piece: member %llu is not valid gzip at byte %llu (reason %d)%s",
                  (unsigned long long)counts->error_member, (unsigned long long)counts->error_offset, counts->error,
                  piece_counts->window_limited ? ", or the window ends inside its first block" : "");
        return SK_EDATA;
    }
    if (status == 2) {
        set_error(ctx, piece_counts->inherited ? "gzip piece: an earlier piece's text was beyond its capacity"
                                               : "gzip piece: the first stretch needs %llu bytes, more than the capacity",
                  (unsigned long long)counts->bytes_out);
        return SK_ESPACE;
    }
    if (status) SK_BAD(ctx, "gzip piece: the state's position is outside the image handed in");
    return SK_OK;
}

int sk_probe_read_bandwidth(sk_ctx *ctx, const void *dev_buf, size_t bytes, int launches, void *hip_stream, double *gb_per_s)
{
    if (!ctx || !dev_buf || !gb_per_s || launches < 1 || bytes < (1u << 20) || (reinterpret_cast<uintptr_t>(dev_buf) & 15)) return SK_EINVAL;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    SK_HIP(ctx, hipSetDevice(ctx->device));
    hipEvent_t e0, e1;
    SK_HIP(ctx, hipEventCreate(&e0));
    SK_HIP(ctx, hipEventCreate(&e1));
    uint32_t *sink = reinterpret_cast<uint32_t *>(ctx->d_err); // never written: the kernel's store is unreachable for real data
    for (int i = 0; i < 3; ++i) SK_HIP(ctx, sk_launch_read_probe(dev_buf, bytes, sink, ctx->cu_count, stream));
    SK_HIP(ctx, hipEventRecord(e0, stream));
    for (int i = 0; i < launches; ++i) SK_HIP(ctx, sk_launch_read_probe(dev_buf, bytes, sink, ctx->cu_count, stream));
    SK_HIP(ctx, hipEventRecord(e1, stream));
    SK_HIP(ctx, hipEventSynchronize(e1));
    float ms = 0;
    SK_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *gb_per_s = ms > 0 ? (double)bytes * launches / (ms * 1e-3) / 1e9 : 0.0;
    return SK_OK;
}

namespace {
// both device-resident scans; n_reads_dev: NULL = batch->n_reads reads (sk_scan_device_async)
int scan_device_async(sk_ctx *ctx, const sk_params *params, const sk_batch *batch, const uint64_t *n_reads_dev, sk_cut *out,
                      void *hip_stream)
{
    if (!ctx || !out) return SK_EINVAL;
    sk_scan_args a;
    int rc = make_args(ctx, params, batch, &a);
    if (rc != SK_OK) return rc;
    if (n_reads_dev) {
        // everything sized on the host -- grids, the regrouping's scratch and whether it runs, LDS -- stays a function
        // of the bound; the kernels an `offsets` batch reaches lower their n_reads to the word (sk_counted_reads)
        if (!batch->offsets || batch->tiles || batch->lengths) {
            set_error(ctx, "sk_scan_counted_device_async: a device read count needs an `offsets` batch (no tiles, no lengths)");
            return SK_EINVAL;
        }
        if (reinterpret_cast<uintptr_t>(n_reads_dev) & 7) {
            set_error(ctx, "sk_scan_counted_device_async: n_reads_dev must be 8-byte aligned");
            return SK_EINVAL;
        }
        a.n_reads_dev = n_reads_dev;
    }
    // NULL is HIP's default (null) stream, like everywhere else in HIP: ordered after whatever the
    // caller queued there (e.g. the kernels that produced the batch)
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    unsigned long long *d_err, *h_err;
    SortScratch *sort = nullptr;
    rc = err_word_of(ctx, stream, &d_err, &h_err, &sort);
    if (rc != SK_OK) return rc;
    return enqueue_scan(ctx, &a, batch, reinterpret_cast<sk_cut_dev *>(out), d_err, stream, -1, sort);
}
} // namespace

int sk_scan_device_async(sk_ctx *ctx, const sk_params *params, const sk_batch *batch, sk_cut *out, void *hip_stream)
{
    return scan_device_async(ctx, params, batch, nullptr, out, hip_stream);
}

int sk_scan_counted_device_async(sk_ctx *ctx, const sk_params *params, const sk_batch *batch, const uint64_t *n_reads_dev,
                                 sk_cut *out, void *hip_stream)
{
    return scan_device_async(ctx, params, batch, n_reads_dev, out, hip_stream);
}

int sk_scan_device_finish(sk_ctx *ctx, void *hip_stream, sk_err *err)
{
    if (!ctx) return SK_EINVAL;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    unsigned long long *d_err, *h_err;
    int rc = err_word_of(ctx, stream, &d_err, &h_err);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, hipMemcpyAsync(h_err, d_err, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    rc = reset_error_word(ctx, d_err, stream);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, hipStreamSynchronize(stream));
    return decode_error(*h_err, err);
}

int sk_submit(sk_ctx *ctx, int slot, const sk_params *params, const sk_batch *batch, sk_cut *out)
{
    if (!ctx || slot < 0 || (size_t)slot >= ctx->slots.size() || !batch || (!out && batch->n_reads)) return SK_EINVAL;
    Slot &s = ctx->slots[(size_t)slot];
    if (s.busy) return SK_EBUSY;
    sk_scan_args a;
    int rc = make_args(ctx, params, batch, &a);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = batch_bytes(batch);
    const size_t n = (size_t)batch->n_reads;
    if (!batch->offsets && batch->lengths) {
        for (size_t r = 0; r < n; ++r)
            if (batch->lengths[r] > batch->stride) {
                set_error(ctx, "lengths[%zu] = %u exceeds stride %u", r, batch->lengths[r], batch->stride);
                return SK_EINVAL;
            }
    }
    uint64_t rag_max_len = 0;
    int rag_fit = -1;
    if (batch->offsets) {
        // host offsets are checked here (ascending, reads within SK_MAX_READ_LEN: the error word keeps
        // 24 bits of position) and give the exact longest read, which sizes the tile kernel's buffers
        for (size_t r = 0; r < n; ++r) {
            const uint64_t o = batch->offsets[r], e = batch->offsets[r + 1];
            if (e < o || e - o > SK_MAX_READ_LEN) {
                set_error(ctx, "offsets[%zu..%zu] = %llu, %llu: not ascending, or a read longer than %u", r, r + 1,
                          (unsigned long long)o, (unsigned long long)e, SK_MAX_READ_LEN);
                return SK_EINVAL;
            }
            if (e - o > rag_max_len) rag_max_len = e - o;
        }
        // does any tile of 64 consecutive reads fit the tile kernel's buffer (rag_tile_fits of the kernels)?
        const uint32_t buf = rag_buf_bytes(rag_max_len, false);
        rag_fit = 0;
        for (size_t t = 0; t < n && !rag_fit; t += 64) {
            uint64_t lmax = 0;
            for (size_t r = t; r < n && r < t + 64; ++r) lmax = std::max<uint64_t>(lmax, batch->offsets[r + 1] - batch->offsets[r]);
            if (lmax <= SK_RAG_MAX_LEN && 64 * 16 * (((lmax + 15) >> 4) | 1) + SK_TILE_SLACK <= buf) rag_fit = 1;
        }
    }
    rc = grow_slot(ctx, s, bytes, n, a.truncn != 0, batch->offsets != nullptr, batch->lengths != nullptr);
    if (rc != SK_OK) return rc;
    if (batch->tiles) {
        // descriptors are checked here, on the host, before any of them reaches a kernel
        uint64_t reads = 0;
        for (uint32_t t = 0; t < batch->n_tiles; ++t) {
            const sk_tile &d = batch->tiles[t];
            if (d.rows == 0 || d.rows > 64 || d.stride % 8 != 0 || d.stride > batch->stride || d.read_len > d.stride ||
                d.byte_off % 16 != 0 || (size_t)d.byte_off + (size_t)d.rows * d.stride > bytes ||
                (uint64_t)d.slot0 + d.rows > batch->n_reads) {
                set_error(ctx, "segmented batch: tile %u is malformed", t);
                return SK_EINVAL;
            }
            reads += d.rows;
        }
        if (reads != batch->n_reads) {
            set_error(ctx, "segmented batch: tiles hold %llu reads, n_reads is %llu", (unsigned long long)reads,
                      (unsigned long long)batch->n_reads);
            return SK_EINVAL;
        }
        for (size_t i = 0; i < n; ++i)
            if (batch->out_index[i] >= batch->n_reads) {
                set_error(ctx, "segmented batch: out_index[%zu] out of range", i);
                return SK_EINVAL;
            }
        if (batch->n_tiles > s.cap_tiles) {
            if (s.d_tiles) (void)hipFree(s.d_tiles);
            s.d_tiles = nullptr;
            s.cap_tiles = 0;
            const size_t cap = batch->n_tiles + (batch->n_tiles >> 3) + 16;
            SK_HIP(ctx, hipMalloc(&s.d_tiles, cap * sizeof(sk_tile_dev)));
            s.cap_tiles = cap;
        }
        if (n > s.cap_index) {
            if (s.d_out_index) (void)hipFree(s.d_out_index);
            s.d_out_index = nullptr;
            s.cap_index = 0;
            const size_t cap = n + (n >> 3) + 16;
            SK_HIP(ctx, hipMalloc(&s.d_out_index, cap * sizeof(uint32_t)));
            s.cap_index = cap;
        }
        if (!batch->classes) {
            s.classes.resize(SK_SEG_MAX_CLASSES);
            s.classes.resize(sk_seg_classes(batch->tiles, batch->n_tiles, s.classes.data(), SK_SEG_MAX_CLASSES));
        }
        SK_HIP(ctx, hipMemcpyAsync(s.d_tiles, batch->tiles, batch->n_tiles * sizeof(sk_tile), hipMemcpyHostToDevice, ctx->copy));
        SK_HIP(ctx, hipMemcpyAsync(s.d_out_index, batch->out_index, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->copy));
    }

    // H2D on the copy stream (overlaps the previous slot's kernel on the compute stream)
    if (bytes) {
        SK_HIP(ctx, hipMemcpyAsync(s.d_qual, batch->qual, bytes, hipMemcpyHostToDevice, ctx->copy));
        if (a.truncn) SK_HIP(ctx, hipMemcpyAsync(s.d_seq, batch->seq, bytes, hipMemcpyHostToDevice, ctx->copy));
    }
    if (batch->offsets)
        SK_HIP(ctx, hipMemcpyAsync(s.d_offsets, batch->offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->copy));
    if (!batch->offsets && batch->lengths && n)
        SK_HIP(ctx, hipMemcpyAsync(s.d_lengths, batch->lengths, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->copy));
    SK_HIP(ctx, hipEventRecord(s.copied, ctx->copy));
    SK_HIP(ctx, hipStreamWaitEvent(ctx->compute, s.copied, 0));

    sk_batch dev = *batch;
    dev.qual = s.d_qual;
    dev.seq = a.truncn ? s.d_seq : nullptr;
    dev.offsets = batch->offsets ? s.d_offsets : nullptr;
    if (batch->offsets) dev.stride = (uint32_t)rag_max_len;
    dev.lengths = (!batch->offsets && batch->lengths) ? s.d_lengths : nullptr;
    dev.tiles = batch->tiles ? reinterpret_cast<const sk_tile *>(s.d_tiles) : nullptr;
    dev.out_index = batch->tiles ? s.d_out_index : nullptr;
    if (batch->tiles && !batch->classes && !s.classes.empty()) {
        dev.classes = s.classes.data();
        dev.n_classes = (uint32_t)s.classes.size();
    }
    rc = enqueue_scan(ctx, &a, &dev, s.d_out, s.d_err, ctx->compute, rag_fit, &s.sort);
    if (rc != SK_OK) return rc;
    if (n) SK_HIP(ctx, hipMemcpyAsync(out, s.d_out, n * sizeof(sk_cut_dev), hipMemcpyDeviceToHost, ctx->compute));
    SK_HIP(ctx, hipMemcpyAsync(s.h_err, s.d_err, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->compute));
    rc = reset_error_word(ctx, s.d_err, ctx->compute);
    if (rc != SK_OK) return rc;
    SK_HIP(ctx, hipEventRecord(s.finished, ctx->compute));
    s.busy = true;
    return SK_OK;
}

int sk_wait(sk_ctx *ctx, int slot, sk_err *err)
{
    if (!ctx || slot < 0 || (size_t)slot >= ctx->slots.size()) return SK_EINVAL;
    Slot &s = ctx->slots[(size_t)slot];
    if (!s.busy) return SK_EINVAL;
    SK_HIP(ctx, hipEventSynchronize(s.finished));
    s.busy = false;
    return decode_error(*s.h_err, err);
}

int sk_trim_batch(sk_ctx *ctx, const sk_params *params, const sk_batch *batch, sk_cut *out, sk_err *err)
{
    int rc = sk_submit(ctx, 0, params, batch, out);
    if (rc != SK_OK) return rc;
    return sk_wait(ctx, 0, err);
}

} // extern "C"
