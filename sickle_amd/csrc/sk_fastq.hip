// sk_fastq.hip -- FASTQ text on the device (sk_trim_fastq_device_async): frame the text into records, check them the way
// reference src/FQEntry.cpp:53-97 does, pack qual (and seq) into an `offsets` batch for the scan, and write the kept
// records back as FASTQ text in the record format of src/trim_single.cpp:393-396, routed by the pair rule.
//
// Launches on one stream, no inter-workgroup waiting (workgroup dispatch order is undefined):
//   frame   1 count  per 64 KiB chunk of text: '\n' count and the last '\n'
//           2 scan   one workgroup: chunk bases (first line number, last '\n' before the chunk), the unterminated last
//                    line, line / record totals, the pair-count verdict
//           3 lines  per chunk again: every '\n' gives the end of line ln and the start of line ln + 1; the line ends of
//                    record ln / 4 go to its descriptor slot
//           4 check  the checks of every framed record, the lowest failing (read, reason) by a global atomicMin
//   pack    5 count / 6 scan / 7 place   qual lengths -> offsets[] of the packed batch (reduce-then-scan over blocks)
//           8 gather qual (and seq) of every record into the workspace: output-partitioned, aligned 16-byte stores
//   (the scan: sk_scan_device_async on the packed batch, launched by sk_capi.hip)
//   emit    9 count / 10 scan / 11 place  the pair rule over the cuts: output offset and read of every kept record
//           12 gather the records' bytes: name line, seq[five:three], '\n', '+' line, qual[five:three], '\n'
// SK_TRIM_PE_COMBO_ALL (sickle's -M) is SK_TRIM_PE_INTERLEAVED everywhere but in the emission: fq_route sends every read of
// the call to out[0], a read that is not kept as an N record (sk_fastq_record.h), and step 12 runs as
// sk_fq_gather_combo_kernel, the same gather instantiated with the N record's piece table.
// Piece calls (sk_trim_fastq_piece_device_async): the three frame kernels start the text at a device word (fq_start), the
// frame scan takes whole records (pairs) only when more text follows, and the emission's scan publishes what was consumed
// and the ok word for the carry kernel of sk_fastq_piece.hip; everything else runs as it does for a whole text.
// The workspace layout and the header words are in sk_device.h.  The gathers build aligned 16-byte granules from aligned
// 16-byte loads funnel-shifted by v_alignbyte (sk_load_window, sk_device_prims.h), so the text may
// have any alignment and no load touches a 16-byte block without a wanted byte.
#include <hip/hip_runtime.h>

#include "sk_device.h"
#include "sk_device_prims.h"
#include "sk_fastq_clip.h"
#include "sk_fastq_order.h"
#include "sk_fastq_record.h"

namespace {


#define FQ_THREADS 256
#define FQ_SUB (FQ_THREADS * 16u)                        // text bytes of one pass of a framing workgroup
#define FQ_PER_THREAD (SK_FQ_BLOCK_READS / FQ_THREADS)  // consecutive reads of one lane (even: pairs stay whole)
#define FQ_GPL 2                                         // 16-byte granules per lane and chunk of a gather
#define FQ_GCHUNK (FQ_THREADS * 16u * FQ_GPL)
#define FQ_WIN 128 // records of a gather chunk staged in LDS (further ones are searched in global memory)

static_assert(SK_FQ_CHUNK_BYTES % FQ_SUB == 0, "a framing chunk is whole passes");
static_assert(FQ_PER_THREAD % 2 == 0, "a lane must hold whole pairs");

struct fq_out {
    uint8_t *text;
    uint64_t cap;
    uint64_t *index;
    uint64_t rec_cap;
};

struct fq_args {
    const uint8_t *text[2];
    uint64_t bytes[2]; // the lengths, or their bounds
    const uint64_t *bytes_dev[2], *valid_dev[2];
    uint64_t n_chunks[2];
    uint64_t slots[2];
    int32_t mode;      // the framing mode: SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED, with combo_all set
    int32_t combo_all; // the routing of SK_TRIM_PE_COMBO_ALL: every read below NREAL to out[0], the not kept ones as N records
    uint32_t fail_qual; // Q of an N record
    int32_t trunc_n;
    int32_t counted; // the per-read steps stop at SK_FQ_H_NREAL (fq_block_empty) and the scan takes its read count from it
    uint64_t n_pack, n_blocks;
    uint64_t *hdr;
    uint64_t *chunks; // 2 words per chunk, input 0's chunks first
    uint64_t *desc[2]; // 5 words per slot: name start, then the end ('\n' or end of text) of each of the four lines
    uint64_t *offsets; // n_pack + 1
    sk_cut_dev *cuts;
    uint64_t *blk;  // SK_FQ_BLOCK_WORDS per block of SK_FQ_BLOCK_READS packed reads (pack, then emit)
    uint64_t *emit; // 2 words per kept record: output offset, read
    uint8_t *pq, *ps;
    const unsigned long long *errword;
    fq_out out[3];
    // piece calls (sk_trim_fastq_piece_device_async with a piece): text i is [*start_dev[i], n_i) of text[i]; the frame
    // scan captures *errword
    const uint64_t *start_dev[2];
    int32_t piece; // 0: no piece (the words 21.. of the header are not touched), 1: a piece, more == 0, 2: more != 0
    // clipped calls (sk_trim_fastq_clipped_device_async): read r's clip word, written by sk_fq_clip_kernel in front of the
    // pack; NULL: no clip
    const uint32_t *clip;
};

// ------------------------------------------------------------------------------------------
// shared pieces
// ------------------------------------------------------------------------------------------
// text i's length: never beyond the bound the launches and the workspace were sized by
__device__ __forceinline__ uint64_t fq_length(const fq_args &a, int i)
{
    uint64_t n = a.bytes[i];
    if (a.bytes_dev[i]) n = min(n, *a.bytes_dev[i]);
    if (a.valid_dev[i] && *a.valid_dev[i] == 0) n = 0;
    return n;
}

// text i's first byte (a piece's window start; 0 without one): never beyond the length n
__device__ __forceinline__ uint64_t fq_start(const fq_args &a, int i, uint64_t n)
{
    return a.start_dev[i] ? min(*a.start_dev[i], n) : 0;
}

// the '\n' bytes of the aligned 16-byte block at q (offset from the aligned base of text i) that lie inside the text
// [s, n) (fq_start, fq_length, loaded once per workgroup): bit b = byte q + b.  A block without a byte of the text is not
// loaded.  sh = the alignment shift + s: the text's first byte, from the aligned base.
__device__ __forceinline__ uint32_t fq_nl_mask(const fq_args &a, int i, uint64_t sh, uint64_t n, uint64_t q)
{
    const uint64_t span = (reinterpret_cast<uintptr_t>(a.text[i]) & 15) + n;
    if (q + 16 <= sh || q >= span) return 0;
    const sk_u4 *blk = reinterpret_cast<const sk_u4 *>((reinterpret_cast<uintptr_t>(a.text[i]) & ~(uintptr_t)15) + q);
    const sk_u4 v = __builtin_nontemporal_load(blk);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = w[j] ^ 0x0a0a0a0au;                              // '\n' -> 0
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu); // exact: 0x80 in every zero byte
        const uint32_t b = z >> 7;                                            // bits 0, 8, 16, 24
        m |= ((b | (b >> 7) | (b >> 14) | (b >> 21)) & 0xfu) << (4 * j);
    }
    const uint32_t lo = q < sh ? (uint32_t)(sh - q) : 0u, hi = span - q < 16 ? (uint32_t)(span - q) : 16u;
    return m & (((1u << hi) - 1u) & ~((1u << lo) - 1u));
}

// A block of SK_FQ_BLOCK_READS reads (or emission ranks) that lies wholly at or beyond the packed batch's records: it
// contributes zeros to its block table entry and loads no descriptor, offset or cut (wave-uniform).  Only when the scan
// behind the pack is the counted one (a.counted): then nothing beyond the records is scanned either.
__device__ __forceinline__ bool fq_block_empty(const fq_args &a, uint64_t n_real)
{
    return a.counted && (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS >= n_real;
}

// exclusive prefix sum of s and exclusive prefix max of m over the workgroup, and both totals.  lds: 8 words.
__device__ __forceinline__ void fq_scan2(uint64_t s, uint64_t m, uint64_t &s_ex, uint64_t &m_ex, uint64_t &s_tot,
                                         uint64_t &m_tot, uint64_t *lds)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t is = s, im = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t ts = __shfl_up(is, d), tm = __shfl_up(im, d);
        if (lane >= d) {
            is += ts;
            im = max(im, tm);
        }
    }
    uint64_t pm = __shfl_up(im, 1);
    if (lane == 0) pm = 0;
    if (lane == 63) {
        lds[2 * w] = is;
        lds[2 * w + 1] = im;
    }
    __syncthreads();
    uint64_t bs = 0, bm = 0, ts = 0, tm = 0;
#pragma unroll
    for (int ww = 0; ww < FQ_THREADS / 64; ++ww) {
        const uint64_t x = lds[2 * ww], y = lds[2 * ww + 1];
        if (ww < w) {
            bs += x;
            bm = max(bm, y);
        }
        ts += x;
        tm = max(tm, y);
    }
    s_ex = bs + is - s;
    m_ex = max(bm, pm);
    s_tot = ts;
    m_tot = tm;
    __syncthreads();
}

// line ln of text i spans [start, end): its end goes to the slot of record ln / 4 (the name line's start too)
__device__ __forceinline__ void fq_put_line(const fq_args &a, int i, uint64_t ln, uint64_t start, uint64_t end)
{
    const uint64_t r = ln >> 2;
    if (r >= a.slots[i]) return; // never: b bytes hold at most b lines (sk_device.h)
    uint64_t *d = a.desc[i] + 5 * r;
    if ((ln & 3) == 0) d[0] = start;
    d[1 + (ln & 3)] = end;
}

// read number -> (input, record of that input)
__device__ __forceinline__ int fq_input_of(const fq_args &a, uint64_t read, uint64_t &rec)
{
    if (a.mode == SK_TRIM_PE_SPLIT) {
        rec = read >> 1;
        return (int)(read & 1);
    }
    rec = read;
    return 0;
}

struct fq_rec {
    const uint8_t *text;
    uint64_t s0, e0, e1, e2, e3; // name start, line ends
};

__device__ __forceinline__ fq_rec fq_record(const fq_args &a, uint64_t read)
{
    uint64_t k;
    const int i = fq_input_of(a, read, k);
    const uint64_t *d = a.desc[i] + 5 * k;
    return {a.text[i], d[0], d[1], d[2], d[3], d[4]};
}

// ------------------------------------------------------------------------------------------
// 1 frame: count
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQ_THREADS) sk_fq_frame_count_kernel(fq_args a)
{
    __shared__ uint64_t lds[8];
    const int i = blockIdx.x < a.n_chunks[0] ? 0 : 1;
    const uint64_t c = blockIdx.x - (i ? a.n_chunks[0] : 0);
    const uint64_t sh = reinterpret_cast<uintptr_t>(a.text[i]) & 15, n = fq_length(a, i), s = fq_start(a, i, n);
    uint64_t cnt = 0, last = 0; // last: position + 1 of the lane's last '\n', 0 = none
    for (uint32_t u = 0; u < SK_FQ_CHUNK_BYTES / FQ_SUB; ++u) {
        const uint64_t q = c * SK_FQ_CHUNK_BYTES + u * FQ_SUB + 16u * threadIdx.x;
        const uint32_t m = fq_nl_mask(a, i, sh + s, n, q);
        cnt += __builtin_popcount(m);
        if (m) last = q + (31 - __builtin_clz(m)) - sh + 1;
    }
    uint64_t s_ex, m_ex, s_tot, m_tot;
    fq_scan2(cnt, last, s_ex, m_ex, s_tot, m_tot, lds);
    if (threadIdx.x == 0) {
        a.chunks[2 * blockIdx.x] = s_tot;
        a.chunks[2 * blockIdx.x + 1] = m_tot;
    }
}

// ------------------------------------------------------------------------------------------
// 2 frame: scan of the chunk table (one workgroup), the unterminated last line, totals
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQ_THREADS) sk_fq_frame_scan_kernel(fq_args a)
{
    __shared__ uint64_t lds[8];
    uint64_t lines[2] = {0, 0};
    for (int i = 0; i < 2; ++i) {
        const uint64_t nc = a.n_chunks[i];
        uint64_t *tab = a.chunks + 2 * (i ? a.n_chunks[0] : 0);
        const uint64_t per = (nc + FQ_THREADS - 1) / FQ_THREADS, c0 = min(nc, per * threadIdx.x), c1 = min(nc, c0 + per);
        uint64_t s = 0, m = 0;
        for (uint64_t c = c0; c < c1; ++c) {
            s += tab[2 * c];
            m = max(m, tab[2 * c + 1]);
        }
        uint64_t s_ex, m_ex, s_tot, m_tot;
        fq_scan2(s, m, s_ex, m_ex, s_tot, m_tot, lds);
        for (uint64_t c = c0; c < c1; ++c) {
            const uint64_t x = tab[2 * c], y = tab[2 * c + 1];
            tab[2 * c] = s_ex;
            tab[2 * c + 1] = m_ex;
            s_ex += x;
            m_ex = max(m_ex, y);
        }
        lines[i] = s_tot;
        // a last line without '\n' ends at the end of the text; behind a piece with more text to come it is no line
        const uint64_t n = fq_length(a, i), first = fq_start(a, i, n);
        if (threadIdx.x == 0 && a.piece != 2 && n > first && a.text[i][n - 1] != '\n') {
            fq_put_line(a, i, s_tot, max(m_tot, first), n);
            lines[i] += 1;
        }
        if (threadIdx.x == 0 && a.piece) {
            a.hdr[SK_FQP_H_START + i] = first;
            a.hdr[SK_FQP_H_END + i] = n;
        }
        __syncthreads(); // lds reuse
    }
    if (threadIdx.x == 0) {
        uint64_t *h = a.hdr;
        uint64_t r0 = lines[0] >> 2, r1 = lines[1] >> 2;
        h[SK_FQ_H_LINES] = lines[0];
        h[SK_FQ_H_LINES + 1] = lines[1];
        if (a.piece) {
            // an earlier call's range error on the stream: the piece takes no record, so that its scan leaves the word alone
            const unsigned long long range0 = *a.errword;
            h[SK_FQP_H_RANGE0] = range0;
            h[SK_FQP_H_MORE] = a.piece == 2;
            if (a.piece == 2) { // whole records (pairs) only: the rest is the carry, no record of the piece
                if (a.mode == SK_TRIM_PE_SPLIT) r0 = r1 = min(r0, r1);
                else if (a.mode == SK_TRIM_PE_INTERLEAVED) r0 &= ~1ull;
            }
            if (range0 != ~0ull) r0 = r1 = 0;
        }
        h[SK_FQ_H_RECORDS] = r0;
        h[SK_FQ_H_RECORDS + 1] = r1;
        uint64_t fmt = ~0ull, real;
        if (a.mode == SK_TRIM_PE_SPLIT) {
            // the first record without a mate: the CLI's "Batch2 and Batch1 have different lengths"
            if (r0 != r1) fmt = ((r0 < r1 ? 2 * r0 + 1 : 2 * r1) << 3) | SK_FQ_PAIR_COUNT;
            real = 2 * min(r0, r1);
        } else {
            real = a.mode == SK_TRIM_PE_INTERLEAVED ? (r0 & ~1ull) : r0;
        }
        h[SK_FQ_H_FMT] = fmt;
        h[SK_FQ_H_MODE] = (uint64_t)a.mode;
        h[SK_FQ_H_NREAL] = min(real, a.n_pack); // more only in a text with a malformed record (sk_device.h)
    }
}

// ------------------------------------------------------------------------------------------
// 3 frame: every line's end into its record's slot
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQ_THREADS) sk_fq_frame_lines_kernel(fq_args a)
{
    __shared__ uint64_t lds[8];
    const int i = blockIdx.x < a.n_chunks[0] ? 0 : 1;
    const uint64_t c = blockIdx.x - (i ? a.n_chunks[0] : 0);
    const uint64_t sh = reinterpret_cast<uintptr_t>(a.text[i]) & 15, n = fq_length(a, i), s = fq_start(a, i, n);
    uint64_t ln0 = a.chunks[2 * blockIdx.x], prev = max(a.chunks[2 * blockIdx.x + 1], s); // prev: start of the chunk's first line
    for (uint32_t u = 0; u < SK_FQ_CHUNK_BYTES / FQ_SUB; ++u) {
        const uint64_t q = c * SK_FQ_CHUNK_BYTES + u * FQ_SUB + 16u * threadIdx.x;
        uint32_t m = fq_nl_mask(a, i, sh + s, n, q);
        const uint64_t last = m ? q + (31 - __builtin_clz(m)) - sh + 1 : 0;
        uint64_t s_ex, m_ex, s_tot, m_tot;
        fq_scan2(__builtin_popcount(m), last, s_ex, m_ex, s_tot, m_tot, lds);
        uint64_t ln = ln0 + s_ex, start = max(prev, m_ex);
        while (m) {
            const int b = __builtin_ctz(m);
            m &= m - 1;
            const uint64_t p = q + b - sh;
            fq_put_line(a, i, ln, start, p);
            ++ln;
            start = p + 1;
        }
        ln0 += s_tot;
        prev = max(prev, m_tot);
    }
}

// ------------------------------------------------------------------------------------------
// 4 check: reference src/FQEntry.cpp:53-97, in its order; the first failing check of a record is its lowest reason
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FQ_THREADS) sk_fq_check_kernel(fq_args a)
{
    const uint64_t *h = a.hdr;
    // the clamps never bite: every record with a line has a slot (sk_device.h)
    const uint64_t n0 = min(h[SK_FQ_H_RECORDS], a.slots[0]), n1 = min(h[SK_FQ_H_RECORDS + 1], a.slots[1]);
    uint64_t best = ~0ull;
    for (uint64_t g = (uint64_t)blockIdx.x * FQ_THREADS + threadIdx.x; g < n0 + n1; g += (uint64_t)gridDim.x * FQ_THREADS) {
        const int i = g < n0 ? 0 : 1;
        const uint64_t r = g - (i ? n0 : 0);
        const uint64_t *d = a.desc[i] + 5 * r;
        const uint64_t s0 = d[0], e0 = d[1], e1 = d[2], e2 = d[3], e3 = d[4];
        const uint64_t name = e0 - s0, seq = e1 - e0 - 1, qual = e3 - e2 - 1;
        uint64_t why = SK_FQ_OK;
        if (name <= 1) why = SK_FQ_ID_SHORT;
        else if (a.text[i][s0] != '@') why = SK_FQ_ID_NO_AT;
        else if (seq == 0) why = SK_FQ_SEQ_EMPTY;
        else if (qual == 0) why = SK_FQ_QUAL_EMPTY;
        else if (qual != seq) why = SK_FQ_LENGTHS;
        else if (qual > SK_MAX_READ_LEN_DEV) why = SK_FQ_TOO_LONG;
        if (why != SK_FQ_OK) {
            const uint64_t read = a.mode == SK_TRIM_PE_SPLIT ? 2 * r + i : r;
            best = min(best, (read << 3) | why);
        }
    }
    if (best != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(a.hdr + SK_FQ_H_FMT), (unsigned long long)best);
}

// ------------------------------------------------------------------------------------------
// 5-7 pack: the packed batch's offsets
// ------------------------------------------------------------------------------------------
// qual length of packed read r (0 beyond the framed records and for every read of a malformed text); of a clipped call the
// bases in front of the read's clip point (sk_fastq_clip.h)
__device__ __forceinline__ uint64_t fq_pack_len(const fq_args &a, uint64_t r, uint64_t n_real, bool bad)
{
    if (bad || r >= n_real) return 0;
    const fq_rec x = fq_record(a, r);
    const uint64_t len = x.e3 - x.e2 - 1;
    return a.clip ? fqc_packed_len(len, a.clip[r]) : len; // uniform
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_pack_count_kernel(fq_args a)
{
    __shared__ uint64_t lds[4];
    const uint64_t n_real = a.hdr[SK_FQ_H_NREAL];
    if (fq_block_empty(a, n_real)) {
        if (threadIdx.x == 0) a.blk[blockIdx.x * SK_FQ_BLOCK_WORDS] = 0;
        return;
    }
    const bool bad = a.hdr[SK_FQ_H_FMT] != ~0ull;
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + threadIdx.x * FQ_PER_THREAD;
    uint64_t v[1] = {0}, tot[1];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j) v[0] += fq_pack_len(a, first + j, n_real, bad);
    sk_block_scan<1, FQ_THREADS>(v, tot, lds);
    if (threadIdx.x == 0) a.blk[blockIdx.x * SK_FQ_BLOCK_WORDS] = tot[0];
}

// one workgroup: the block table's first `nv` words -> exclusive bases in place; the totals
template <int N>
__device__ __forceinline__ void fq_scan_blocks(const fq_args &a, uint64_t (&run)[N], uint64_t *lds)
{
#pragma unroll
    for (int i = 0; i < N; ++i) run[i] = 0;
    for (uint64_t b0 = 0; b0 < a.n_blocks; b0 += FQ_THREADS) {
        const uint64_t b = b0 + threadIdx.x;
        uint64_t v[N], tot[N];
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = b < a.n_blocks ? a.blk[b * SK_FQ_BLOCK_WORDS + i] : 0;
        sk_block_scan<N, FQ_THREADS>(v, tot, lds);
        if (b < a.n_blocks)
#pragma unroll
            for (int i = 0; i < N; ++i) a.blk[b * SK_FQ_BLOCK_WORDS + i] = run[i] + v[i];
#pragma unroll
        for (int i = 0; i < N; ++i) run[i] += tot[i];
    }
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_pack_scan_kernel(fq_args a)
{
    __shared__ uint64_t lds[4];
    uint64_t run[1];
    fq_scan_blocks<1>(a, run, lds);
    if (threadIdx.x == 0) {
        a.hdr[SK_FQ_H_PACKED] = run[0];
        a.offsets[a.n_pack] = run[0];
        // the counted scan's batch ends at offsets[NREAL], and the place kernel's blocks beyond the records write nothing
        if (a.counted) a.offsets[min(a.hdr[SK_FQ_H_NREAL], a.n_pack)] = run[0];
    }
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_pack_place_kernel(fq_args a)
{
    __shared__ uint64_t lds[4];
    const uint64_t n_real = a.hdr[SK_FQ_H_NREAL];
    if (fq_block_empty(a, n_real)) return; // (offsets[NREAL] is the scan kernel's; nobody reads the offsets behind it)
    const bool bad = a.hdr[SK_FQ_H_FMT] != ~0ull;
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + threadIdx.x * FQ_PER_THREAD;
    uint64_t len[FQ_PER_THREAD];
    uint64_t v[1] = {0}, tot[1];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j) {
        len[j] = fq_pack_len(a, first + j, n_real, bad);
        v[0] += len[j];
    }
    sk_block_scan<1, FQ_THREADS>(v, tot, lds);
    uint64_t b = v[0] + a.blk[blockIdx.x * SK_FQ_BLOCK_WORDS];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j) {
        if (first + j < a.n_pack) a.offsets[first + j] = b;
        b += len[j];
    }
}

// ------------------------------------------------------------------------------------------
// 9-11 emit: the pair rule over the cuts
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int fq_dest(int mode, bool kept, bool mate_kept, bool second)
{
    if (!kept) return -1;
    if (mode == SK_TRIM_SE) return 0;
    if (!mate_kept) return 2;
    return (mode == SK_TRIM_PE_SPLIT && second) ? 1 : 0;
}

struct fq_emit_read {
    int dest;
    uint64_t bytes;
};

// Destination and bytes of the FQ_PER_THREAD records of a lane from their cuts.  is_read: the rank holds a read of the call
// (below NREAL, below the cuts, no verdict); only such a one is ever emitted, and its cut is {-1, -1} otherwise.  The pair
// rule cannot tell "not kept" from "no read" and need not.  SK_TRIM_PE_COMBO_ALL must: the first is an N record in out[0],
// the second nothing.  The flag is uniform and is looked at once, outside the loops, so that the other modes run the loop
// they always ran.  record(j): the fq_rec of the lane's j-th read.
template <class F>
__device__ __forceinline__ void fq_route(const fq_args &a, const bool (&is_read)[FQ_PER_THREAD], const sk_cut_dev (&c)[FQ_PER_THREAD],
                                         F record, fq_emit_read (&rd)[FQ_PER_THREAD])
{
    if (a.combo_all) {
#pragma unroll
        for (int j = 0; j < FQ_PER_THREAD; ++j) {
            rd[j].dest = is_read[j] ? 0 : -1;
            rd[j].bytes = 0;
            if (is_read[j]) {
                const fq_rec x = record(j);
                rd[j].bytes = fqr_bytes({x.s0, x.e0, x.e1, x.e2, x.e3}, c[j].five, c[j].three);
            }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j) {
        rd[j].dest = fq_dest(a.mode, fqr_kept(c[j].three), fqr_kept(c[j ^ 1].three), j & 1);
        rd[j].bytes = 0;
        if (rd[j].dest >= 0) {
            const fq_rec x = record(j);
            rd[j].bytes = fqr_kept_bytes({x.s0, x.e0, x.e1, x.e2, x.e3}, c[j].five, c[j].three);
        }
    }
}

// the FQ_PER_THREAD reads of this lane (first even): destination and bytes of the emitted record
__device__ __forceinline__ void fq_emit_load(const fq_args &a, uint64_t first, uint64_t n_real, bool bad,
                                             fq_emit_read (&rd)[FQ_PER_THREAD])
{
    bool is_read[FQ_PER_THREAD];
    sk_cut_dev c[FQ_PER_THREAD];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j) {
        const uint64_t r = first + j;
        c[j] = {-1, -1};
        is_read[j] = !bad && r < n_real;
        if (is_read[j]) c[j] = a.cuts[r];
    }
    fq_route(a, is_read, c, [&](int j) { return fq_record(a, first + j); }, rd);
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_emit_count_kernel(fq_args a)
{
    __shared__ uint64_t lds[4 * 6];
    const uint64_t n_real = a.hdr[SK_FQ_H_NREAL];
    if (fq_block_empty(a, n_real)) {
        if (threadIdx.x < 6) a.blk[blockIdx.x * SK_FQ_BLOCK_WORDS + threadIdx.x] = 0;
        return;
    }
    const bool bad = a.hdr[SK_FQ_H_FMT] != ~0ull;
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + threadIdx.x * FQ_PER_THREAD;
    fq_emit_read rd[FQ_PER_THREAD];
    fq_emit_load(a, first, n_real, bad, rd);
    uint64_t v[6] = {0, 0, 0, 0, 0, 0}, tot[6];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j)
#pragma unroll
        for (int o = 0; o < 3; ++o)
            if (rd[j].dest == o) {
                v[o] += 1;
                v[3 + o] += rd[j].bytes;
            }
    sk_block_scan<6, FQ_THREADS>(v, tot, lds);
    if (threadIdx.x < 6) {
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) x = threadIdx.x == k ? tot[k] : x; // no runtime index into tot[]
        a.blk[blockIdx.x * SK_FQ_BLOCK_WORDS + threadIdx.x] = x;
    }
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_emit_scan_kernel(fq_args a)
{
    __shared__ uint64_t lds[4 * 6];
    uint64_t run[6];
    fq_scan_blocks<6>(a, run, lds);
    if (threadIdx.x < 3) {
        const int o = threadIdx.x;
        const fq_out &out = a.out[o];
        const unsigned long long range = *a.errword;
        const bool ok = a.hdr[SK_FQ_H_FMT] == ~0ull && range == ~0ull;
        const uint64_t recs = o == 0 ? run[0] : o == 1 ? run[1] : run[2], bytes = o == 0 ? run[3] : o == 1 ? run[4] : run[5];
        const bool produced = out.text != nullptr;
        const bool fit = produced && ok && bytes <= out.cap && (!out.index || recs <= out.rec_cap);
        a.hdr[SK_FQ_H_OUT_RECORDS + o] = recs;
        a.hdr[SK_FQ_H_OUT_BYTES + o] = bytes;
        a.hdr[SK_FQ_H_PRODUCED + o] = produced;
        a.hdr[SK_FQ_H_FIT + o] = fit;
        if (o == 0) a.hdr[SK_FQ_H_RANGE] = range;
    }
    if (a.piece && threadIdx.x == 3) { // the word a carry behind this piece goes by
        bool ok = a.hdr[SK_FQ_H_FMT] == ~0ull && *a.errword == ~0ull && a.hdr[SK_FQP_H_RANGE0] == ~0ull;
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            const fq_out &out = a.out[o];
            const uint64_t recs = o == 0 ? run[0] : o == 1 ? run[1] : run[2], bytes = o == 0 ? run[3] : o == 1 ? run[4] : run[5];
            if (out.text && (bytes > out.cap || (out.index && recs > out.rec_cap))) ok = false;
        }
        a.hdr[SK_FQP_H_OK] = ok;
    }
    if (a.piece && (threadIdx.x == 4 || threadIdx.x == 5)) { // the first byte of text i the piece did not consume
        const int i = threadIdx.x - 4;
        const uint64_t u = a.hdr[SK_FQ_H_RECORDS + i], end = a.hdr[SK_FQP_H_END + i];
        uint64_t consumed = a.hdr[SK_FQP_H_START + i];
        if (!a.hdr[SK_FQP_H_MORE] || i >= (a.mode == SK_TRIM_PE_SPLIT ? 2 : 1)) consumed = end; // the stream ends here
        else if (u > a.slots[i]) consumed = end; // never: every record with a line has a slot (sk_device.h)
        else if (u) consumed = a.desc[i][5 * (u - 1) + 4] + 1;
        a.hdr[SK_FQP_H_CONSUMED + i] = consumed;
    }
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_emit_place_kernel(fq_args a)
{
    __shared__ uint64_t lds[4 * 6];
    const uint64_t *h = a.hdr;
    const bool fit[3] = {h[SK_FQ_H_FIT] != 0, h[SK_FQ_H_FIT + 1] != 0, h[SK_FQ_H_FIT + 2] != 0};
    if (!fit[0] && !fit[1] && !fit[2]) return; // uniform
    const uint64_t n_real = h[SK_FQ_H_NREAL];
    if (fq_block_empty(a, n_real)) return;
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + threadIdx.x * FQ_PER_THREAD;
    fq_emit_read rd[FQ_PER_THREAD];
    fq_emit_load(a, first, n_real, false, rd);
    uint64_t v[6] = {0, 0, 0, 0, 0, 0}, tot[6];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j)
#pragma unroll
        for (int o = 0; o < 3; ++o)
            if (rd[j].dest == o) {
                v[o] += 1;
                v[3 + o] += rd[j].bytes;
            }
    sk_block_scan<6, FQ_THREADS>(v, tot, lds);
    const uint64_t *blk = a.blk + blockIdx.x * SK_FQ_BLOCK_WORDS;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += blk[k];
    const uint64_t dbase[3] = {0, h[SK_FQ_H_OUT_RECORDS], h[SK_FQ_H_OUT_RECORDS] + h[SK_FQ_H_OUT_RECORDS + 1]};
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j)
#pragma unroll
        for (int o = 0; o < 3; ++o)
            if (rd[j].dest == o) {
                const uint64_t k = v[o], b = v[3 + o];
                v[o] += 1;
                v[3 + o] += rd[j].bytes;
                if (!fit[o]) continue;
                a.emit[2 * (dbase[o] + k)] = b;
                a.emit[2 * (dbase[o] + k) + 1] = first + j;
                if (a.out[o].index) a.out[o].index[k] = first + j;
            }
}

// ------------------------------------------------------------------------------------------
// 8, 12 gathers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void fq_store_granule(uint8_t *dst, uint64_t g, sk_u128 x, int n)
{
    if (n == 16) {
        __builtin_nontemporal_store(sk_from_u128(x), reinterpret_cast<sk_u4 *>(dst + g));
    } else {
        for (int i = 0; i < n; ++i) dst[g + i] = (uint8_t)(x >> (8 * i));
    }
}

// one piece of a record: bytes [0, len) at src, or (src == nullptr) the low len bytes of imm, for which nothing is loaded
struct fq_piece {
    const uint8_t *src;
    uint64_t len, imm;
};

// the table of sk_fastq_record.h over `text`
template <int NP>
__device__ __forceinline__ void fq_pieces_at(const uint8_t *text, const fqr_piece (&in)[NP], fq_piece (&pc)[NP])
{
#pragma unroll
    for (int j = 0; j < NP; ++j) pc[j] = {in[j].at != FQR_IMM ? text + in[j].at : nullptr, in[j].len, in[j].imm};
}

// bytes [rel, rel + n) of a record made of NP pieces to bytes [d, d + n) of acc.  WIDE: an immediate may have more than one
// byte (the N record's); else every immediate is one byte, a '\n'.
template <int NP, bool WIDE>
__device__ __forceinline__ void fq_fill(const fq_piece (&pc)[NP], uint64_t rel, int d, int n, sk_u128 &acc)
{
    uint64_t ps = 0;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const uint64_t pe = ps + pc[j].len;
        if (n > 0 && rel < pe && rel >= ps) {
            const int t = (int)min((uint64_t)n, pe - rel);
            if (pc[j].src)
                sk_put(acc, sk_to_u128(sk_load_window(pc[j].src + (rel - ps), t)), d, t);
            else if (WIDE)
                sk_put(acc, (sk_u128)(pc[j].imm >> (8 * (rel - ps))), d, t);
            else
                sk_put(acc, (sk_u128)pc[j].imm, d, 1);
            rel += t;
            d += t;
            n -= t;
        }
        ps = pe;
    }
}

// kind 0: packed qual, 1: packed seq, 2..4: emitted output kind - 2
struct fq_job {
    uint8_t *dst;
    uint64_t total, R;
    const uint64_t *off; // record k starts at off[k * ostride]
    uint32_t ostride;
    int kind;
};

// bytes [rel, rel + n) of record k of the job to bytes [d, d + n) of acc.  COMBO: the emission of SK_TRIM_PE_COMBO_ALL, whose
// table also lists reads that are not kept (their N records); without it every listed read is kept and the table of
// fqr_pieces has constant kinds, lengths and immediates where it always had them.
template <bool COMBO>
__device__ __forceinline__ void fq_record_bytes(const fq_args &a, const fq_job &j, uint64_t k, uint64_t rel, int d, int n,
                                                sk_u128 &acc)
{
    if (j.kind < 2) {
        const fq_rec x = fq_record(a, k);
        const fq_piece pc[1] = {{x.text + (j.kind == 0 ? x.e2 : x.e0) + 1, x.e3 - x.e2 - 1, 0}};
        fq_fill<1, false>(pc, rel, d, n, acc);
        return;
    }
    const uint64_t read = j.off[k * 2 + 1];
    const fq_rec x = fq_record(a, read);
    const sk_cut_dev c = a.cuts[read];
    fqr_piece rule[6];
    fq_piece pc[6];
    fqr_pieces({x.s0, x.e0, x.e1, x.e2, x.e3}, c.five, c.three, COMBO, a.fail_qual, rule);
    fq_pieces_at<6>(x.text, rule, pc);
    fq_fill<6, COMBO>(pc, rel, d, n, acc);
}

template <bool COMBO>
__device__ __forceinline__ void fq_gather(const fq_args &a, int emit)
{
    __shared__ uint64_t s_off[FQ_WIN + 1];
    __shared__ uint64_t s_cur;
    const int t = threadIdx.x, lane = t & 63;
    const uint64_t *h = a.hdr;
    const int n_jobs = emit ? 3 : (a.trunc_n ? 2 : 1);
    uint64_t dbase = 0;
    for (int jb = 0; jb < n_jobs; ++jb) {
        fq_job j;
        if (emit) {
            const uint64_t R = h[SK_FQ_H_OUT_RECORDS + jb];
            j = {a.out[jb].text, h[SK_FQ_H_OUT_BYTES + jb], R, a.emit + 2 * dbase, 2, 2 + jb};
            dbase += R;
            if (!h[SK_FQ_H_FIT + jb]) continue; // uniform
        } else {
            // (counted: the offsets end at offsets[NREAL] = the total; the reads behind are empty either way)
            j = {jb ? a.ps : a.pq, h[SK_FQ_H_PACKED], a.counted ? min(h[SK_FQ_H_NREAL], a.n_pack) : a.n_pack, a.offsets, 1, jb};
        }
        if (j.total == 0) continue;
        const uint64_t n_chunks = (j.total + FQ_GCHUNK - 1) / FQ_GCHUNK;
        const uint64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
        const uint64_t c0 = (uint64_t)blockIdx.x * per, c1 = min(c0 + per, n_chunks);
        if (c0 >= c1) continue;
        // offset of record k (k <= R; off(R) = total)
        auto off = [&](uint64_t k) { return k < j.R ? j.off[k * j.ostride] : j.total; };
        // the record holding the span's first byte: a 64-ary search by wave 0 (the last k < R with off(k) <= x)
        if (t < 64) {
            const uint64_t x = c0 * FQ_GCHUNK;
            uint64_t lo = 0, hi = j.R;
            while (hi - lo > 1) {
                const uint64_t step = (hi - lo + 63) / 64, p = lo + lane * step;
                const uint64_t mk = __builtin_amdgcn_ballot_w64(p < hi && off(p) <= x); // lane 0's probe always holds
                lo += (uint64_t)(63 - __builtin_clzll(mk)) * step;
                hi = min(hi, lo + step);
            }
            if (t == 0) s_cur = lo;
        }
        __syncthreads();
        uint64_t cur = s_cur;
        for (uint64_t c = c0; c < c1; ++c) {
            if (t <= FQ_WIN) s_off[t] = cur + t <= j.R ? off(cur + t) : ~0ull;
            __syncthreads();
            const uint64_t win_end = s_off[FQ_WIN];
            uint64_t k_last = cur;
#pragma unroll
            for (int u = 0; u < FQ_GPL; ++u) {
                const uint64_t g = c * FQ_GCHUNK + (uint64_t)u * (FQ_THREADS * 16) + 16u * t;
                if (g >= j.total) break;
                uint64_t k;
                if (g < win_end) {
                    int lo = 0, hi = FQ_WIN; // s_off[lo] <= g < s_off[hi]
                    while (hi - lo > 1) {
                        const int mid = (lo + hi) >> 1;
                        if (s_off[mid] <= g) lo = mid; else hi = mid;
                    }
                    k = cur + lo;
                } else {
                    uint64_t lo = cur + FQ_WIN, hi = j.R; // off(lo) <= g < off(hi)
                    while (hi - lo > 1) {
                        const uint64_t mid = lo + ((hi - lo) >> 1);
                        if (off(mid) <= g) lo = mid; else hi = mid;
                    }
                    k = lo;
                }
                k_last = k;
                const uint64_t end = min(g + 16, j.total);
                sk_u128 acc = 0;
                uint64_t pos = g;
                while (pos < end) {
                    const uint64_t i = k - cur;
                    const uint64_t b = i < FQ_WIN ? s_off[i] : off(k);
                    const uint64_t e = i < FQ_WIN ? s_off[i + 1] : off(k + 1);
                    if (e <= pos) { // the record ended (or is empty)
                        ++k;
                        continue;
                    }
                    const uint64_t pe = min(e, end);
                    fq_record_bytes<COMBO>(a, j, k, pos - b, (int)(pos - g), (int)(pe - pos), acc);
                    pos = pe;
                }
                fq_store_granule(j.dst, g, acc, (int)(end - g));
            }
            // the next chunk starts at or after the record of the last lane's last granule
            if (t == FQ_THREADS - 1) s_cur = k_last;
            __syncthreads();
            cur = s_cur;
        }
        __syncthreads(); // s_cur / s_off are reused by the next job
    }
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_gather_kernel(fq_args a, int emit) { fq_gather<false>(a, emit); }

// the emission's gather of SK_TRIM_PE_COMBO_ALL: a kernel of its own, so that the N record's variable immediate costs the
// other modes' gather no register
__global__ void __launch_bounds__(FQ_THREADS) sk_fq_gather_combo_kernel(fq_args a) { fq_gather<true>(a, 1); }

void fq_launch_emit_gather(const fq_args &a, int cu_count, hipStream_t stream)
{
    const dim3 grid((unsigned)cu_count * SK_TRIM_GATHER_WG_PER_CU), threads(FQ_THREADS);
    if (a.combo_all) hipLaunchKernelGGL(sk_fq_gather_combo_kernel, grid, threads, 0, stream, a);
    else hipLaunchKernelGGL(sk_fq_gather_kernel, grid, threads, 0, stream, a, 1);
}

// ------------------------------------------------------------------------------------------
// ordered calls (sk_trim_fastq_ordered_device_async): the reference's batches and -a T order, sk_fastq_order.h
//   frame 1-3 as above, then  O1 chain  one lane walks the batches: the table of first units, the counts, NREAL
//                             O2 check  the records inside the batches; every line of every text against batch_len - 1
//   pack 5-8 and the scan as above (reads stay in read order), then
//   emit  O3 count / O4 scan / O5 place  as 9-11, but over emission ranks: a lane owns FQ_PER_THREAD consecutive ranks
//         and maps each to its read; 12 gather as above (a.emit holds (output offset, read) in rank order)
// ------------------------------------------------------------------------------------------
struct fq_order {
    uint64_t *tab; // capacity + 1 first units
    uint64_t capacity, batch_len, limit;
    uint32_t threads;
};

// lines of text i the descriptor table holds: all of them (sk_device.h: a slot for every four lines of any text)
__device__ __forceinline__ uint64_t fq_order_lines(const fq_args &a, int i)
{
    return min(a.hdr[SK_FQ_H_LINES + i], 4 * a.slots[i]);
}

__global__ void __launch_bounds__(64) sk_fq_order_chain_kernel(fq_args a, fq_order o)
{
    if (threadIdx.x != 0) return;
    uint64_t *h = a.hdr;
    const int n_in = a.mode == SK_TRIM_PE_SPLIT ? 2 : 1;
    const uint64_t *const desc[2] = {a.desc[0], a.desc[1]};
    const uint64_t nl[2] = {fq_order_lines(a, 0), n_in == 2 ? fq_order_lines(a, 1) : 0};
    fqo_chain_result r;
    fqo_chain(desc, nl, n_in, a.mode == SK_TRIM_PE_INTERLEAVED ? 8u : 4u, o.batch_len, o.capacity, o.limit, o.tab, &r);
    h[SK_FQO_H_BATCHES] = r.overflow ? o.capacity + 1 : r.batches;
    h[SK_FQO_H_UNITS] = r.units;
    h[SK_FQO_H_LAST_UNITS] = r.last_units;
    h[SK_FQO_H_UNBATCHED] = h[SK_FQ_H_RECORDS] - r.batched_lines[0] / 4;
    h[SK_FQO_H_UNBATCHED + 1] = n_in == 2 ? h[SK_FQ_H_RECORDS + 1] - r.batched_lines[1] / 4 : 0;
    h[SK_FQO_H_MISMATCH] = r.mismatch;
    h[SK_FQO_H_OVERFLOW] = r.overflow;
    h[SK_FQO_H_LONG] = ~0ull;
    h[SK_FQO_H_ERROR_BATCH] = ~0ull;
    h[SK_FQ_H_FMT] = ~0ull; // records without a mate are behind the last batch: no verdict
    // a table that was too small trims nothing; more reads than the packed batch holds only with a malformed record
    // inside the batches (sk_device.h)
    h[SK_FQ_H_NREAL] = r.overflow ? 0 : min(r.units * (a.mode == SK_TRIM_SE ? 1u : 2u), a.n_pack);
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_check_kernel(fq_args a, fq_order o)
{
    const uint64_t *h = a.hdr;
    const uint64_t nl[2] = {fq_order_lines(a, 0), a.mode == SK_TRIM_PE_SPLIT ? fq_order_lines(a, 1) : 0};
    const uint64_t n0 = (nl[0] + 3) / 4, n1 = (nl[1] + 3) / 4; // records with a line, the last one maybe incomplete
    const uint64_t inside = h[SK_FQO_H_UNITS] * (a.mode == SK_TRIM_PE_INTERLEAVED ? 2u : 1u); // records per input
    uint64_t best = ~0ull, longest = ~0ull;
    for (uint64_t g = (uint64_t)blockIdx.x * FQ_THREADS + threadIdx.x; g < n0 + n1; g += (uint64_t)gridDim.x * FQ_THREADS) {
        const int i = g < n0 ? 0 : 1;
        const uint64_t r = g - (i ? n0 : 0);
        const uint64_t *d = a.desc[i] + 5 * r;
        const uint64_t have = min(nl[i] - 4 * r, (uint64_t)4);
        uint64_t start = d[0], e[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((uint64_t)k < have) {
                e[k] = d[1 + k];
                if (e[k] - start + 1 >= o.batch_len) longest = min(longest, ((uint64_t)i << 63) | (4 * r + k));
                start = e[k] + 1;
            }
        if (r >= inside) continue;
        const uint64_t s0 = d[0], name = e[0] - s0, seq = e[1] - e[0] - 1, qual = e[3] - e[2] - 1;
        uint64_t why = SK_FQ_OK;
        if (name <= 1) why = SK_FQ_ID_SHORT;
        else if (a.text[i][s0] != '@') why = SK_FQ_ID_NO_AT;
        else if (seq == 0) why = SK_FQ_SEQ_EMPTY;
        else if (qual == 0) why = SK_FQ_QUAL_EMPTY;
        else if (qual != seq) why = SK_FQ_LENGTHS;
        else if (qual > SK_MAX_READ_LEN_DEV) why = SK_FQ_TOO_LONG;
        if (why != SK_FQ_OK) {
            const uint64_t read = a.mode == SK_TRIM_PE_SPLIT ? 2 * r + i : r;
            best = min(best, (read << 3) | why);
        }
    }
    if (best != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(a.hdr + SK_FQ_H_FMT), (unsigned long long)best);
    if (longest != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(a.hdr + SK_FQO_H_LONG), (unsigned long long)longest);
}

// The same check for an ordered piece, whose order words (SK_FQO_H_*) live at oh, its extension block.  (A copy: routing
// the kernel above through it changes that kernel's register allocation.)
__device__ __forceinline__ void fq_order_check(const fq_args &a, const fq_order &o, uint64_t *oh)
{
    const uint64_t nl[2] = {fq_order_lines(a, 0), a.mode == SK_TRIM_PE_SPLIT ? fq_order_lines(a, 1) : 0};
    const uint64_t n0 = (nl[0] + 3) / 4, n1 = (nl[1] + 3) / 4; // records with a line, the last one maybe incomplete
    const uint64_t inside = oh[SK_FQO_H_UNITS] * (a.mode == SK_TRIM_PE_INTERLEAVED ? 2u : 1u); // records per input
    uint64_t best = ~0ull, longest = ~0ull;
    for (uint64_t g = (uint64_t)blockIdx.x * FQ_THREADS + threadIdx.x; g < n0 + n1; g += (uint64_t)gridDim.x * FQ_THREADS) {
        const int i = g < n0 ? 0 : 1;
        const uint64_t r = g - (i ? n0 : 0);
        const uint64_t *d = a.desc[i] + 5 * r;
        const uint64_t have = min(nl[i] - 4 * r, (uint64_t)4);
        uint64_t start = d[0], e[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((uint64_t)k < have) {
                e[k] = d[1 + k];
                if (e[k] - start + 1 >= o.batch_len) longest = min(longest, ((uint64_t)i << 63) | (4 * r + k));
                start = e[k] + 1;
            }
        if (r >= inside) continue;
        const uint64_t s0 = d[0], name = e[0] - s0, seq = e[1] - e[0] - 1, qual = e[3] - e[2] - 1;
        uint64_t why = SK_FQ_OK;
        if (name <= 1) why = SK_FQ_ID_SHORT;
        else if (a.text[i][s0] != '@') why = SK_FQ_ID_NO_AT;
        else if (seq == 0) why = SK_FQ_SEQ_EMPTY;
        else if (qual == 0) why = SK_FQ_QUAL_EMPTY;
        else if (qual != seq) why = SK_FQ_LENGTHS;
        else if (qual > SK_MAX_READ_LEN_DEV) why = SK_FQ_TOO_LONG;
        if (why != SK_FQ_OK) {
            const uint64_t read = a.mode == SK_TRIM_PE_SPLIT ? 2 * r + i : r;
            best = min(best, (read << 3) | why);
        }
    }
    if (best != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(a.hdr + SK_FQ_H_FMT), (unsigned long long)best);
    if (longest != ~0ull) atomicMin(reinterpret_cast<unsigned long long *>(oh + SK_FQO_H_LONG), (unsigned long long)longest);
}


// the reads at the lane's FQ_PER_THREAD consecutive ranks from `first` (even): mates share a pair rank, so they stay
// neighbours.  Ranks at or beyond n_real get ~0.
__device__ __forceinline__ void fq_order_reads(const fq_args &a, const fq_order &o, const uint64_t *oh, uint64_t first,
                                               uint64_t n_real, uint64_t (&reads)[FQ_PER_THREAD])
{
    const uint64_t batches = oh[SK_FQO_H_BATCHES];
    if (a.mode == SK_TRIM_SE) {
        fqo_lane_units<FQ_PER_THREAD>(o.tab, batches, o.threads, true, first, n_real, reads);
    } else {
        uint64_t pairs[FQ_PER_THREAD / 2];
        fqo_lane_units<FQ_PER_THREAD / 2>(o.tab, batches, o.threads, false, first >> 1, n_real >> 1, pairs);
#pragma unroll
        for (int j = 0; j < FQ_PER_THREAD; ++j) reads[j] = pairs[j >> 1] == ~0ull ? ~0ull : 2 * pairs[j >> 1] + (j & 1);
    }
}

// fq_emit_load at the mapped reads
// (cuts exist below n_cuts: n_pack, or NREAL behind the counted scan -- a read in between is empty, its cut {-1, -1})
__device__ __forceinline__ void fq_order_emit_load(const fq_args &a, const uint64_t (&reads)[FQ_PER_THREAD], bool bad,
                                                   uint64_t n_cuts, fq_emit_read (&rd)[FQ_PER_THREAD])
{
    bool is_read[FQ_PER_THREAD];
    sk_cut_dev c[FQ_PER_THREAD];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j) {
        c[j] = {-1, -1};
        is_read[j] = !bad && reads[j] < n_cuts; // (a rank at or beyond NREAL has reads[j] = ~0)
        if (is_read[j]) c[j] = a.cuts[reads[j]];
    }
    fq_route(a, is_read, c, [&](int j) { return fq_record(a, reads[j]); }, rd);
}

// nothing is trimmed after a format error, a line gzgets would split or a table that was too small
__device__ __forceinline__ bool fq_order_bad(const uint64_t *h, const uint64_t *oh)
{
    return h[SK_FQ_H_FMT] != ~0ull || oh[SK_FQO_H_LONG] != ~0ull || oh[SK_FQO_H_OVERFLOW] != 0;
}

__device__ __forceinline__ void fq_order_emit_count(const fq_args &a, const fq_order &o, const uint64_t *oh)
{
    __shared__ uint64_t lds[4 * 6];
    const uint64_t n_real = a.hdr[SK_FQ_H_NREAL];
    if (fq_block_empty(a, n_real)) { // ranks at or beyond NREAL map to no read
        if (threadIdx.x < 6) a.blk[blockIdx.x * SK_FQ_BLOCK_WORDS + threadIdx.x] = 0;
        return;
    }
    const bool bad = fq_order_bad(a.hdr, oh);
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + threadIdx.x * FQ_PER_THREAD;
    uint64_t reads[FQ_PER_THREAD];
    fq_emit_read rd[FQ_PER_THREAD];
    fq_order_reads(a, o, oh, first, bad ? 0 : n_real, reads);
    fq_order_emit_load(a, reads, bad, a.counted ? n_real : a.n_pack, rd);
    uint64_t v[6] = {0, 0, 0, 0, 0, 0}, tot[6];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (rd[j].dest == k) {
                v[k] += 1;
                v[3 + k] += rd[j].bytes;
            }
    sk_block_scan<6, FQ_THREADS>(v, tot, lds);
    if (threadIdx.x < 6) {
        uint64_t x = 0;
#pragma unroll
        for (int k = 0; k < 6; ++k) x = threadIdx.x == k ? tot[k] : x; // no runtime index into tot[]
        a.blk[blockIdx.x * SK_FQ_BLOCK_WORDS + threadIdx.x] = x;
    }
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_emit_count_kernel(fq_args a, fq_order o)
{
    fq_order_emit_count(a, o, a.hdr);
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_emit_scan_kernel(fq_args a, fq_order o)
{
    __shared__ uint64_t lds[4 * 6];
    uint64_t run[6];
    fq_scan_blocks<6>(a, run, lds);
    const unsigned long long range = *a.errword;
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const fq_out &out = a.out[k];
        const bool ok = !fq_order_bad(a.hdr, a.hdr) && range == ~0ull;
        const uint64_t recs = k == 0 ? run[0] : k == 1 ? run[1] : run[2], bytes = k == 0 ? run[3] : k == 1 ? run[4] : run[5];
        const bool produced = out.text != nullptr;
        const bool fit = produced && ok && bytes <= out.cap && (!out.index || recs <= out.rec_cap);
        a.hdr[SK_FQ_H_OUT_RECORDS + k] = recs;
        a.hdr[SK_FQ_H_OUT_BYTES + k] = bytes;
        a.hdr[SK_FQ_H_PRODUCED + k] = produced;
        a.hdr[SK_FQ_H_FIT + k] = fit;
        if (k == 0) a.hdr[SK_FQ_H_RANGE] = range;
    }
    if (threadIdx.x == 3) { // the batch of the record behind the error finish will report
        const uint64_t fmt = a.hdr[SK_FQ_H_FMT], units = a.hdr[SK_FQO_H_UNITS];
        uint64_t read = ~0ull;
        if (fmt != ~0ull) read = fmt >> 3;
        else if (range != ~0ull) read = range >> 32;
        const uint64_t unit = a.mode == SK_TRIM_SE ? read : read >> 1;
        if (read != ~0ull && unit < units && !a.hdr[SK_FQO_H_OVERFLOW])
            a.hdr[SK_FQO_H_ERROR_BATCH] = fqo_batch_of(o.tab, a.hdr[SK_FQO_H_BATCHES], unit);
    }
}

__device__ __forceinline__ void fq_order_emit_place(const fq_args &a, const fq_order &o, const uint64_t *oh)
{
    __shared__ uint64_t lds[4 * 6];
    const uint64_t *h = a.hdr;
    const bool fit[3] = {h[SK_FQ_H_FIT] != 0, h[SK_FQ_H_FIT + 1] != 0, h[SK_FQ_H_FIT + 2] != 0};
    if (!fit[0] && !fit[1] && !fit[2]) return; // uniform
    const uint64_t n_real = h[SK_FQ_H_NREAL];
    const uint64_t first = (uint64_t)blockIdx.x * SK_FQ_BLOCK_READS + threadIdx.x * FQ_PER_THREAD;
    uint64_t reads[FQ_PER_THREAD];
    fq_emit_read rd[FQ_PER_THREAD];
    if (fq_block_empty(a, n_real)) return;
    fq_order_reads(a, o, oh, first, n_real, reads);
    fq_order_emit_load(a, reads, false, a.counted ? n_real : a.n_pack, rd);
    uint64_t v[6] = {0, 0, 0, 0, 0, 0}, tot[6];
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (rd[j].dest == k) {
                v[k] += 1;
                v[3 + k] += rd[j].bytes;
            }
    sk_block_scan<6, FQ_THREADS>(v, tot, lds);
    const uint64_t *blk = a.blk + blockIdx.x * SK_FQ_BLOCK_WORDS;
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += blk[k];
    const uint64_t dbase[3] = {0, h[SK_FQ_H_OUT_RECORDS], h[SK_FQ_H_OUT_RECORDS] + h[SK_FQ_H_OUT_RECORDS + 1]};
#pragma unroll
    for (int j = 0; j < FQ_PER_THREAD; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (rd[j].dest == k) {
                const uint64_t at = v[k], b = v[3 + k];
                v[k] += 1;
                v[3 + k] += rd[j].bytes;
                if (!fit[k]) continue;
                a.emit[2 * (dbase[k] + at)] = b;
                a.emit[2 * (dbase[k] + at) + 1] = reads[j];
                if (a.out[k].index) a.out[k].index[at] = reads[j];
            }
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_emit_place_kernel(fq_args a, fq_order o)
{
    fq_order_emit_place(a, o, a.hdr);
}

// ------------------------------------------------------------------------------------------
// ordered pieces (sk_trim_fastq_ordered_piece_device_async): a piece (the frame kernels with a.piece) whose records are
// the lines of the batches it commits (fqo_chain_piece).  The header keeps the piece's words (SK_FQP_H_*); the order words
// live in the extension block p.oh (sk_fastq_order.h).
//   frame 1-3, then  P1 chain  one lane: *state_in, the walk over the window, the table, RECORDS / NREAL lowered to the
//                              committed reads, the consumed offsets
//                    O2 check  as above over p.oh (a void piece checks nothing)
//   pack 5-8, the scan, O3 count as above over p.oh, then
//                    P2 scan   O4, then the piece's words (consumed, ok) and *state_out
//                    O5 place as above over p.oh, 12 gather
// ------------------------------------------------------------------------------------------
struct fq_opiece {
    uint64_t *oh;              // the extension block
    const uint64_t *state_in;  // sk_fastq_order_state as 8 words, or NULL: the start of a stream
    uint64_t *state_out;
};

// sk_fastq_order_state's words
#define FQ_ST_CARRIED 0 // [2]
#define FQ_ST_BATCHES 2
#define FQ_ST_UNITS 3
#define FQ_ST_LAST_UNITS 4
#define FQ_ST_ENDED_MISMATCH 5 // ended | stopped_on_mismatch << 32
#define FQ_ST_FAILED 6         // failed | reserved0 << 32

__global__ void __launch_bounds__(64) sk_fq_order_piece_chain_kernel(fq_args a, fq_order o, fq_opiece p)
{
    if (threadIdx.x != 0) return;
    uint64_t *h = a.hdr, *oh = p.oh;
    const int n_in = a.mode == SK_TRIM_PE_SPLIT ? 2 : 1;
    uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (p.state_in)
#pragma unroll
        for (int j = 0; j < 8; ++j) st[j] = p.state_in[j];
    const bool inherited = (uint32_t)st[FQ_ST_FAILED] != 0;
    // void: a failed stream, or the stream's range-error word set when the piece began (the frame scan's look)
    const bool is_void = inherited || h[SK_FQP_H_RANGE0] != ~0ull;
    const uint64_t *const desc[2] = {a.desc[0], a.desc[1]};
    const uint64_t nl[2] = {is_void ? 0 : fq_order_lines(a, 0), n_in == 2 && !is_void ? fq_order_lines(a, 1) : 0};
    const uint64_t first[2] = {h[SK_FQP_H_START], h[SK_FQP_H_START + 1]};
    const fqo_piece_state ps = {{st[FQ_ST_CARRIED], st[FQ_ST_CARRIED + 1]}, st[FQ_ST_BATCHES],
                                (uint32_t)st[FQ_ST_ENDED_MISMATCH] != 0 || is_void};
    fqo_piece_result r;
    fqo_chain_piece(desc, nl, first, n_in, a.mode == SK_TRIM_PE_INTERLEAVED ? 8u : 4u, o.batch_len, o.capacity, o.limit, &ps,
                    h[SK_FQP_H_MORE] != 0, o.tab, &r);
    oh[SK_FQO_H_BATCHES] = r.batches;
    oh[SK_FQO_H_UNITS] = r.units;
    oh[SK_FQO_H_LAST_UNITS] = r.last_units;
    oh[SK_FQO_H_MISMATCH] = r.mismatch;
    oh[SK_FQO_H_OVERFLOW] = 0; // a full table is no error in a piece
    oh[SK_FQO_H_LONG] = ~0ull;
    oh[SK_FQO_H_ERROR_BATCH] = ~0ull;
    oh[SK_FQOP_X_TABLE_FULL] = r.table_full;
    oh[SK_FQOP_X_UNDETERMINED] = r.undetermined;
    oh[SK_FQOP_X_INHERITED] = inherited;
    oh[SK_FQOP_X_BASE_BATCHES] = st[FQ_ST_BATCHES];
    oh[SK_FQOP_X_LAST_UNITS] = r.batches ? r.last_units : st[FQ_ST_LAST_UNITS];
    oh[SK_FQOP_X_ENDED] = is_void ? (uint32_t)st[FQ_ST_ENDED_MISMATCH] : r.ended;
    oh[SK_FQOP_X_STICKY_MISMATCH] = (st[FQ_ST_ENDED_MISMATCH] >> 32) | r.mismatch;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const bool used = i < n_in;
        // the unterminated last line a closing piece closes ends at the text's end: nothing lies behind it
        oh[SK_FQOP_X_CONSUMED + i] = used ? min(fqo_line_start_from(desc[i], r.batched_lines[i], first[i]), h[SK_FQP_H_END + i])
                                          : h[SK_FQP_H_END + i];
        oh[SK_FQO_H_UNBATCHED + i] = used && !is_void ? h[SK_FQ_H_LINES + i] / 4 - r.batched_lines[i] / 4 : 0;
        oh[SK_FQOP_X_STATE + FQ_ST_CARRIED + i] = is_void ? st[FQ_ST_CARRIED + i] : r.carried[i]; // for P2
        h[SK_FQ_H_RECORDS + i] = used ? r.batched_lines[i] / 4 : 0;
        if (is_void) h[SK_FQ_H_LINES + i] = 0; // all counts of a void piece are 0
    }
    h[SK_FQ_H_FMT] = ~0ull; // records without a mate are behind the last batch: no verdict
    h[SK_FQ_H_NREAL] = min(r.units * (a.mode == SK_TRIM_SE ? 1u : 2u), a.n_pack);
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_piece_check_kernel(fq_args a, fq_order o, fq_opiece p)
{
    if (p.oh[SK_FQOP_X_INHERITED] || a.hdr[SK_FQP_H_RANGE0] != ~0ull) return; // void: LINES is 0 anyway
    fq_order_check(a, o, p.oh);
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_piece_emit_count_kernel(fq_args a, fq_order o, fq_opiece p)
{
    fq_order_emit_count(a, o, p.oh);
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_piece_emit_place_kernel(fq_args a, fq_order o, fq_opiece p)
{
    fq_order_emit_place(a, o, p.oh);
}

__global__ void __launch_bounds__(FQ_THREADS) sk_fq_order_piece_emit_scan_kernel(fq_args a, fq_order o, fq_opiece p)
{
    __shared__ uint64_t lds[4 * 6];
    uint64_t run[6];
    fq_scan_blocks<6>(a, run, lds);
    uint64_t *h = a.hdr, *oh = p.oh;
    const unsigned long long range = *a.errword;
    const bool sound = !fq_order_bad(h, oh) && range == ~0ull && h[SK_FQP_H_RANGE0] == ~0ull && !oh[SK_FQOP_X_INHERITED];
    bool fits = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const fq_out &out = a.out[k];
        const uint64_t recs = k == 0 ? run[0] : k == 1 ? run[1] : run[2], bytes = k == 0 ? run[3] : k == 1 ? run[4] : run[5];
        if (out.text && (bytes > out.cap || (out.index && recs > out.rec_cap))) fits = false;
    }
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        const fq_out &out = a.out[k];
        const uint64_t recs = k == 0 ? run[0] : k == 1 ? run[1] : run[2], bytes = k == 0 ? run[3] : k == 1 ? run[4] : run[5];
        const bool produced = out.text != nullptr;
        const bool fit = produced && sound && bytes <= out.cap && (!out.index || recs <= out.rec_cap);
        h[SK_FQ_H_OUT_RECORDS + k] = recs;
        h[SK_FQ_H_OUT_BYTES + k] = bytes;
        h[SK_FQ_H_PRODUCED + k] = produced;
        h[SK_FQ_H_FIT + k] = fit;
        if (k == 0) h[SK_FQ_H_RANGE] = range;
    }
    if (threadIdx.x == 3) { // the (local) batch of the record behind the error finish will report
        const uint64_t fmt = h[SK_FQ_H_FMT], units = oh[SK_FQO_H_UNITS];
        uint64_t read = ~0ull;
        if (fmt != ~0ull) read = fmt >> 3;
        else if (range != ~0ull) read = range >> 32;
        const uint64_t unit = a.mode == SK_TRIM_SE ? read : read >> 1;
        if (read != ~0ull && unit < units) oh[SK_FQO_H_ERROR_BATCH] = fqo_batch_of(o.tab, oh[SK_FQO_H_BATCHES], unit);
    }
    if (threadIdx.x == 4) { // the words a carry behind this piece goes by, and the state the next piece starts from
        const bool ok = sound && fits;
        h[SK_FQP_H_OK] = ok;
        uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (p.state_in)
#pragma unroll
            for (int j = 0; j < 8; ++j) st[j] = p.state_in[j];
        if (ok) { // state_in advanced; a failed piece hands state_in on as it is, with `failed`
            st[FQ_ST_CARRIED] = oh[SK_FQOP_X_STATE + FQ_ST_CARRIED];
            st[FQ_ST_CARRIED + 1] = oh[SK_FQOP_X_STATE + FQ_ST_CARRIED + 1];
            st[FQ_ST_BATCHES] += oh[SK_FQO_H_BATCHES];
            st[FQ_ST_UNITS] += oh[SK_FQO_H_UNITS];
            st[FQ_ST_LAST_UNITS] = oh[SK_FQOP_X_LAST_UNITS];
            st[FQ_ST_ENDED_MISMATCH] = (oh[SK_FQOP_X_ENDED] != 0) | (oh[SK_FQOP_X_STICKY_MISMATCH] << 32);
        }
        st[FQ_ST_FAILED] = ok ? 0 : 1;
        st[7] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            p.state_out[j] = st[j];
            oh[SK_FQOP_X_STATE + j] = st[j];
        }
    }
    if (threadIdx.x == 5 || threadIdx.x == 6) {
        const int i = threadIdx.x - 5;
        h[SK_FQP_H_CONSUMED + i] = oh[SK_FQOP_X_CONSUMED + i];
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
uint64_t fq_chunks_of(const uint8_t *text, uint64_t bytes)
{
    if (!bytes) return 0;
    const uint64_t span = (reinterpret_cast<uintptr_t>(text) & 15) + bytes;
    return (span + SK_FQ_CHUNK_BYTES - 1) / SK_FQ_CHUNK_BYTES;
}

// shift: bytes between the header and the sections (an ordered call's batch table lies there)
// mode: the call's; SK_TRIM_PE_COMBO_ALL becomes the framing mode SK_TRIM_PE_INTERLEAVED with a.combo_all, so that every
// kernel that frames, pairs or orders by a.mode takes it as that.  fail_qual: Q of its N records (emission only).
void fq_make_args(const sk_fastq_input *in, const sk_fastq_lengths *lengths, int mode, int trunc_n, int counted,
                  const sk_fastq_output *out, void *workspace, const unsigned long long *errword, fq_args &a,
                  uint64_t shift = 0, int fail_qual = 0)
{
    const bool combo_all = mode == SK_TRIM_PE_COMBO_ALL;
    if (combo_all) mode = SK_TRIM_PE_INTERLEAVED;
    sk_fq_layout L;
    sk_fq_layout_of(in->bytes[0] + (mode == SK_TRIM_PE_SPLIT ? in->bytes[1] : 0), trunc_n, &L);
    uint8_t *ws = static_cast<uint8_t *>(workspace) + shift;
    const int n_in = mode == SK_TRIM_PE_SPLIT ? 2 : 1;
    for (int i = 0; i < 2; ++i) {
        a.text[i] = i < n_in ? in->text[i] : nullptr;
        a.bytes[i] = i < n_in ? in->bytes[i] : 0;
        a.bytes_dev[i] = i < n_in && lengths ? lengths->bytes_dev[i] : nullptr;
        a.valid_dev[i] = i < n_in && lengths ? lengths->valid_dev[i] : nullptr;
        a.n_chunks[i] = fq_chunks_of(a.text[i], a.bytes[i]);
        a.slots[i] = i < n_in ? sk_fq_slots(a.bytes[i]) : 0;
    }
    a.mode = mode;
    a.combo_all = combo_all ? 1 : 0;
    a.fail_qual = (uint32_t)fail_qual & 0xffu;
    a.trunc_n = trunc_n ? 1 : 0;
    a.counted = counted ? 1 : 0;
    a.n_pack = sk_fq_pack_reads(a.bytes[0], a.bytes[1], mode);
    a.n_blocks = (a.n_pack + SK_FQ_BLOCK_READS - 1) / SK_FQ_BLOCK_READS;
    a.hdr = static_cast<uint64_t *>(workspace);
    a.chunks = reinterpret_cast<uint64_t *>(ws + L.chunks);
    a.desc[0] = reinterpret_cast<uint64_t *>(ws + L.desc);
    a.desc[1] = a.desc[0] + 5 * a.slots[0];
    a.offsets = reinterpret_cast<uint64_t *>(ws + L.offsets);
    a.cuts = reinterpret_cast<sk_cut_dev *>(ws + L.cuts);
    a.blk = reinterpret_cast<uint64_t *>(ws + L.blocks);
    a.emit = reinterpret_cast<uint64_t *>(ws + L.emit);
    a.pq = ws + L.qual;
    a.ps = trunc_n ? ws + L.seq : nullptr;
    a.errword = errword;
    a.start_dev[0] = a.start_dev[1] = nullptr;
    a.piece = 0;
    a.clip = nullptr;
    for (int o = 0; o < 3; ++o) {
        const bool used = o == 0 || (!combo_all && ((mode == SK_TRIM_PE_SPLIT && o == 1) || (mode != SK_TRIM_SE && o == 2)));
        a.out[o] = used && out ? fq_out{out[o].text, out[o].capacity, out[o].record_index, out[o].record_capacity} : fq_out{};
    }
}

// a clipped call's search, between the check and the pack: the clip words are the pack's from here on.  Its launcher ends
// with hipGetLastError, which clears the runtime's error: what it returns stands for every launch of the front so far, and
// the front hands it on
hipError_t fq_launch_clip(fq_args &a, const sk_fq_clip_front *clip, int cu_count, hipStream_t stream)
{
    sk_fq_clip_src src = {};
    src.hdr = a.hdr;
    for (int i = 0; i < 2; ++i) {
        src.desc[i] = a.desc[i];
        src.slots[i] = a.slots[i];
        src.text[i] = a.text[i];
        src.bytes[i] = a.bytes[i];
        src.bytes_dev[i] = a.bytes_dev[i];
        src.valid_dev[i] = a.valid_dev[i];
    }
    src.n_pack = a.n_pack;
    src.mode = a.mode;
    a.clip = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(clip->section) + FQC_STATS_BYTES);
    return sk_launch_fastq_clip(&src, clip, cu_count, stream);
}

} // namespace

namespace {
fq_order fq_make_order(const sk_fastq_order *order, void *workspace)
{
    return {reinterpret_cast<uint64_t *>(static_cast<uint8_t *>(workspace) + SK_FQO_TABLE_BYTES_AT), order->batch_capacity,
            order->batch_len, order->batch_limit, order->threads};
}
} // namespace

// order: NULL = read order; else the batch chain and its check take the place of the check of every record.  lengths:
// NULL = in->bytes are the lengths; else the device words that hold them, in->bytes their bounds.  piece: NULL = the whole
// text; else the window start and the piece rule of sk_trim_fastq_piece_device_async (read order only)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_front(const sk_fastq_input *in,
                                                                                  const sk_fastq_lengths *lengths, int mode,
                                                                                  int trunc_n, int counted,
                                                                                  const sk_fastq_order *order,
                                                                                  const sk_fastq_piece *piece,
                                                                                  const unsigned long long *errword,
                                                                                  void *workspace, int cu_count,
                                                                                  hipStream_t stream, sk_batch *packed,
                                                                                  sk_cut_dev **cuts,
                                                                                  const uint64_t **n_reads_dev,
                                                                                  const sk_fq_clip_front *clip)
{
    fq_args a;
    fq_make_args(in, lengths, mode, trunc_n, counted, nullptr, workspace, piece ? errword : nullptr, a,
                 order ? sk_fq_order_shift(order->batch_capacity) : 0);
    if (piece) {
        for (int i = 0; i < (a.mode == SK_TRIM_PE_SPLIT ? 2 : 1); ++i) a.start_dev[i] = piece->start_dev[i];
        a.piece = piece->more ? 2 : 1;
    }
    const uint64_t nc = a.n_chunks[0] + a.n_chunks[1];
    if (nc) hipLaunchKernelGGL(sk_fq_frame_count_kernel, dim3((unsigned)nc), dim3(FQ_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_fq_frame_scan_kernel, dim3(1), dim3(FQ_THREADS), 0, stream, a);
    if (nc) hipLaunchKernelGGL(sk_fq_frame_lines_kernel, dim3((unsigned)nc), dim3(FQ_THREADS), 0, stream, a);
    if (order) {
        const fq_order o = fq_make_order(order, workspace);
        hipLaunchKernelGGL(sk_fq_order_chain_kernel, dim3(1), dim3(64), 0, stream, a, o);
        hipLaunchKernelGGL(sk_fq_order_check_kernel, dim3((unsigned)cu_count * 4), dim3(FQ_THREADS), 0, stream, a, o);
    } else {
        hipLaunchKernelGGL(sk_fq_check_kernel, dim3((unsigned)cu_count * 4), dim3(FQ_THREADS), 0, stream, a);
    }
    if (clip) {
        const hipError_t e = fq_launch_clip(a, clip, cu_count, stream);
        if (e != hipSuccess) return e; // nothing of the call is waited for: the caller fails it
    }
    if (a.n_blocks) hipLaunchKernelGGL(sk_fq_pack_count_kernel, dim3((unsigned)a.n_blocks), dim3(FQ_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_fq_pack_scan_kernel, dim3(1), dim3(FQ_THREADS), 0, stream, a);
    if (a.n_blocks) hipLaunchKernelGGL(sk_fq_pack_place_kernel, dim3((unsigned)a.n_blocks), dim3(FQ_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_fq_gather_kernel, dim3((unsigned)cu_count * SK_TRIM_GATHER_WG_PER_CU), dim3(FQ_THREADS), 0, stream, a, 0);
    *packed = sk_batch{};
    packed->qual = a.pq;
    packed->seq = a.ps;
    packed->offsets = a.offsets;
    packed->stride = in->max_read_len;
    packed->n_reads = a.n_pack;
    *cuts = a.cuts;
    *n_reads_dev = counted ? a.hdr + SK_FQ_H_NREAL : nullptr; // written by the frame scan / the ordered chain, before the pack
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_emit(const sk_fastq_input *in, int mode, int trunc_n,
                                                                                 int counted, const sk_fastq_order *order,
                                                                                 int piece, int fail_qual,
                                                                                 const sk_fastq_output *out, void *workspace,
                                                                                 const unsigned long long *errword, int cu_count,
                                                                                 hipStream_t stream)
{
    fq_args a;
    // no emission kernel looks at a text's length: lines and records come from the descriptors and the header
    fq_make_args(in, nullptr, mode, trunc_n, counted, out, workspace, errword, a, order ? sk_fq_order_shift(order->batch_capacity) : 0,
                 fail_qual);
    a.piece = piece ? 1 : 0; // the emission takes `more` and the window from the header
    const dim3 blocks((unsigned)a.n_blocks), threads(FQ_THREADS);
    if (order) {
        const fq_order o = fq_make_order(order, workspace);
        if (a.n_blocks) hipLaunchKernelGGL(sk_fq_order_emit_count_kernel, blocks, threads, 0, stream, a, o);
        hipLaunchKernelGGL(sk_fq_order_emit_scan_kernel, dim3(1), threads, 0, stream, a, o);
        if (a.n_blocks) hipLaunchKernelGGL(sk_fq_order_emit_place_kernel, blocks, threads, 0, stream, a, o);
    } else {
        if (a.n_blocks) hipLaunchKernelGGL(sk_fq_emit_count_kernel, blocks, threads, 0, stream, a);
        hipLaunchKernelGGL(sk_fq_emit_scan_kernel, dim3(1), threads, 0, stream, a);
        if (a.n_blocks) hipLaunchKernelGGL(sk_fq_emit_place_kernel, blocks, threads, 0, stream, a);
    }
    fq_launch_emit_gather(a, cu_count, stream);
    return hipGetLastError();
}

// ---- ordered pieces: the two launch functions of sk_trim_fastq_ordered_piece_device_async (sk_device.h) ----
namespace {
void fq_make_opiece(const sk_fastq_order *order, const void *state_in, void *state_out, void *workspace, fq_order &o, fq_opiece &p)
{
    uint8_t *ws = static_cast<uint8_t *>(workspace);
    o = {reinterpret_cast<uint64_t *>(ws + SK_FQOP_TABLE_BYTES_AT), order->batch_capacity, order->batch_len, order->batch_limit,
         order->threads};
    p = {reinterpret_cast<uint64_t *>(ws + SK_FQOP_EXT_BYTES_AT), static_cast<const uint64_t *>(state_in),
         static_cast<uint64_t *>(state_out)};
}
} // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_order_piece_front(
    const sk_fastq_input *in, const sk_fastq_lengths *lengths, int mode, int trunc_n, int counted, const sk_fastq_order *order,
    const sk_fastq_piece *piece, const void *state_in, void *state_out, const unsigned long long *errword, void *workspace,
    int cu_count, hipStream_t stream, sk_batch *packed, sk_cut_dev **cuts, const uint64_t **n_reads_dev,
    const sk_fq_clip_front *clip)
{
    fq_args a;
    fq_make_args(in, lengths, mode, trunc_n, counted, nullptr, workspace, errword, a, sk_fq_order_piece_shift(order->batch_capacity));
    for (int i = 0; i < (a.mode == SK_TRIM_PE_SPLIT ? 2 : 1); ++i) a.start_dev[i] = piece->start_dev[i];
    a.piece = piece->more ? 2 : 1;
    fq_order o;
    fq_opiece p;
    fq_make_opiece(order, state_in, state_out, workspace, o, p);
    const uint64_t nc = a.n_chunks[0] + a.n_chunks[1];
    if (nc) hipLaunchKernelGGL(sk_fq_frame_count_kernel, dim3((unsigned)nc), dim3(FQ_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_fq_frame_scan_kernel, dim3(1), dim3(FQ_THREADS), 0, stream, a);
    if (nc) hipLaunchKernelGGL(sk_fq_frame_lines_kernel, dim3((unsigned)nc), dim3(FQ_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_fq_order_piece_chain_kernel, dim3(1), dim3(64), 0, stream, a, o, p);
    hipLaunchKernelGGL(sk_fq_order_piece_check_kernel, dim3((unsigned)cu_count * 4), dim3(FQ_THREADS), 0, stream, a, o, p);
    if (clip) {
        const hipError_t e = fq_launch_clip(a, clip, cu_count, stream);
        if (e != hipSuccess) return e; // nothing of the call is waited for: the caller fails it
    }
    if (a.n_blocks) hipLaunchKernelGGL(sk_fq_pack_count_kernel, dim3((unsigned)a.n_blocks), dim3(FQ_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_fq_pack_scan_kernel, dim3(1), dim3(FQ_THREADS), 0, stream, a);
    if (a.n_blocks) hipLaunchKernelGGL(sk_fq_pack_place_kernel, dim3((unsigned)a.n_blocks), dim3(FQ_THREADS), 0, stream, a);
    hipLaunchKernelGGL(sk_fq_gather_kernel, dim3((unsigned)cu_count * SK_TRIM_GATHER_WG_PER_CU), dim3(FQ_THREADS), 0, stream, a, 0);
    *packed = sk_batch{};
    packed->qual = a.pq;
    packed->seq = a.ps;
    packed->offsets = a.offsets;
    packed->stride = in->max_read_len;
    packed->n_reads = a.n_pack;
    *cuts = a.cuts;
    *n_reads_dev = counted ? a.hdr + SK_FQ_H_NREAL : nullptr; // written by the piece's chain, before the pack
    return hipGetLastError();
}

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_order_piece_emit(
    const sk_fastq_input *in, int mode, int trunc_n, int counted, const sk_fastq_order *order, const void *state_in,
    void *state_out, int fail_qual, const sk_fastq_output *out, void *workspace, const unsigned long long *errword,
    int cu_count, hipStream_t stream)
{
    fq_args a;
    fq_make_args(in, nullptr, mode, trunc_n, counted, out, workspace, errword, a, sk_fq_order_piece_shift(order->batch_capacity),
                 fail_qual);
    a.piece = 1;
    fq_order o;
    fq_opiece p;
    fq_make_opiece(order, state_in, state_out, workspace, o, p);
    const dim3 blocks((unsigned)a.n_blocks), threads(FQ_THREADS);
    if (a.n_blocks) hipLaunchKernelGGL(sk_fq_order_piece_emit_count_kernel, blocks, threads, 0, stream, a, o, p);
    hipLaunchKernelGGL(sk_fq_order_piece_emit_scan_kernel, dim3(1), threads, 0, stream, a, o, p);
    if (a.n_blocks) hipLaunchKernelGGL(sk_fq_order_piece_emit_place_kernel, blocks, threads, 0, stream, a, o, p);
    fq_launch_emit_gather(a, cu_count, stream);
    return hipGetLastError();
}
