// sk_device.h -- shared between the kernels (sk_kernels.hip) and the C-ABI layer (sk_capi.hip).
#ifndef SK_DEVICE_H
#define SK_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sickle_amd.h"
#include "sk_fastq_words.h"

#define SK_TILE_THREADS 256
#define SK_TILE_WAVES (SK_TILE_THREADS / 64)
#define SK_TILE_SLACK 128u /* bytes a lane may read past its tile (the lead stream runs ahead) */
#define SK_LDS_PER_CU (160u * 1024u)
#define SK_TILE_NBUF_DEFAULT 1 /* LDS buffers per wave for the quality tile (see sk_kernels.hip) */
#define SK_MAX_READ_LEN_DEV (1u << 24) /* == SK_MAX_READ_LEN of the C ABI */
#define SK_RAG_MAX_LEN 2040            /* longest read the lane-per-read kernel takes from a ragged batch */
#define SK_RAG_BUF_DEFAULT (20u * 1024u) /* LDS bytes per wave for ragged tiles when the caller gives no length hint */
#define SK_RAG_BUF_MAX (40u * 1024u)
#ifndef SK_SORT_WINDOW
#define SK_SORT_WINDOW 8192  /* reads per window of the device-side regrouping of mixed-length ragged batches (sk_sort.hip) */
#endif
#define SK_SORT_MIN_READS 65536u /* ragged batches below this keep the plain tile kernel */

struct sk_cut_dev {
    int32_t five, three;
};

// == sk_tile of the C ABI (include/sickle_amd.h)
struct sk_tile_dev {
    uint64_t byte_off;
    uint32_t slot0;
    uint32_t stride;
    uint16_t rows;
    uint16_t read_len;
    uint32_t reserved;
};

// Scalar arguments of one scan, derived on the host from sk_params (+ the batch shape).
struct sk_scan_args {
    uint64_t n_reads;
    uint32_t stride;   // bytes between reads (fixed-stride layouts)
    uint32_t read_len; // uniform read length (fixed-stride, lengths == NULL)
    int32_t qmin, qmax; // legal char range of the encoding (reference src/sickle.h:85-91)
    int32_t craw;      // qual_threshold + offset: the threshold on raw chars (window: craw * w)
    int32_t cthr;      // min(craw, 128), for the byte-parallel compares
    int32_t cthr_raw;  // == craw (scalar compares of the wave kernel)
    int32_t lthr;      // length_threshold
    int32_t no5;       // -x
    int32_t truncn;    // -n
    uint32_t n_tiles;   // segmented batches: number of tile descriptors
    int32_t tile_order; // diagnostic (SK_TILE_ORDER): 0 = tile t on workgroup t mod G, 1 = contiguous tile ranges per XCD
    uint32_t buf_bytes; // LDS bytes per wave (segmented / rows at any address); general kernel: != 0 = only the tiles that do not fit them
    int32_t slot_order;   // segmented batches: cuts written in slot order, out_index only names erroring reads
    uint64_t scan_id;     // number of this scan on its error word (ragged batches: tile kernel -> general kernel hand-over)
    uint32_t team_rbuf;   // general kernels with resident reads (band, team): LDS bytes of one read's buffer
    uint32_t team_maxlen; // ... and the longest read that goes through LDS
    uint32_t stream_nb;   // streaming general kernel: 1 KiB blocks in a wave's ring
    uint32_t stream_read_cost;  // streaming general kernel: what a read costs beyond its bytes when the batch is cut into spans
    uint32_t stream_tbl;  // streaming general kernel: entries of the prefix table (a power of two)
    uint32_t seg_chunk_shift; // segmented batches: a wave takes 1 << this consecutive tiles at a time
    const uint32_t *band_table; // SK_BAND_WIDTHS band matrices, one per window width (sk_band_dword): what a tile kernel loads when a
                                // tile's window width differs from the one before (segmented batches, regrouped ragged batches)
    const uint32_t *sort_flags; // ragged batches behind the device-side regrouping: {windows of mixed lengths, reads too long for the tiles}; the
                                // plain tile kernel (and the general kernel behind it) return at once when the sorted scan runs, and vice versa
    const uint64_t *n_reads_dev; // counted scans (sk_scan_counted_device_async, `offsets` batches): n_reads is a bound and the kernels an
                                 // `offsets` batch reaches scan min(*n_reads_dev, n_reads) reads (sk_counted_reads); NULL: n_reads reads
};

// The band matrix of window width wu, as lane `lane` of a wave holds it for v_mfma_i32_32x32x32_i8 (sk_kernels.hip, MFMA path):
// the dword whose four bytes multiply positions p .. p+3 (relative to a 32-position block), 1 where the lane's window
// covers the position.  The lane supplies row m' = lane & 31 of A; the hardware puts that row into accumulator r of lane
// half hh with m' = (r & 3) + 8 * (r >> 2) + 4 * hh, and that slot is to be window 16 * hh + r.
#if defined(__HIPCC__) || defined(__CUDACC__)
__host__ __device__
#endif
static inline uint32_t sk_band_dword(int lane, int wu, int p)
{
    const int mp = lane & 31;
    const int hh = (mp >> 2) & 1, r = (mp & 3) | ((mp >> 3) << 2);
    const int win = 16 * hh + r;
    const int hi = win + wu - p, lo = win - p; // bytes j with lo <= j < hi
    const uint32_t below_hi = hi >= 4 ? 0x01010101u : (hi <= 0 ? 0u : 0x01010101u & ((1u << (8 * hi)) - 1u));
    const uint32_t below_lo = lo >= 4 ? 0x01010101u : (lo <= 0 ? 0u : 0x01010101u & ((1u << (8 * lo)) - 1u));
    return below_hi & ~below_lo;
}
// the table: [width 0 .. SK_BAND_WIDTHS-1][block 0..2][lane 0..63][4 dwords]: dword j of block b of a lane = positions
// 16 * (lane >> 5) + 4 * j + 32 * b
#define SK_BAND_WIDTHS 66u
#define SK_BAND_TABLE_DWORDS (SK_BAND_WIDTHS * 3u * 64u * 4u)

// internal to libsickle_amd.so (not part of the C ABI)
extern "C" __attribute__((visibility("hidden"))) int sk_tile_is_staged(uint32_t stride, uint32_t read_len, int has_seq);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_tile(const uint8_t *qual, const uint8_t *seq, const uint32_t *lengths,
                                     sk_cut_dev *out, unsigned long long *errword, const sk_scan_args *a,
                                     int cu_count, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_seg(const uint8_t *qual, const uint8_t *seq, const sk_tile_dev *tiles,
                                    const uint32_t *out_index, sk_cut_dev *out, unsigned long long *errword,
                                    const sk_scan_args *a, const sk_seg_class *classes, uint32_t n_classes,
                                    int cu_count, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_team(const uint8_t *qual, const uint8_t *seq, const uint64_t *offsets,
                                     const uint32_t *lengths, sk_cut_dev *out, unsigned long long *errword,
                                     const sk_scan_args *a, uint64_t max_len, int cu_count, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_band(const uint8_t *qual, const uint8_t *seq, const uint64_t *offsets,
                                     const uint32_t *lengths, sk_cut_dev *out, unsigned long long *errword,
                                     const sk_scan_args *a, uint64_t max_len, int cu_count, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_stream(const uint8_t *qual, const uint8_t *seq, const uint64_t *offsets,
                                       const uint32_t *lengths, sk_cut_dev *out, unsigned long long *errword,
                                       const sk_scan_args *a, uint64_t max_len, int cu_count, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_any(const uint8_t *qual, const uint8_t *seq, const uint64_t *offsets,
                                    const uint32_t *lengths, sk_cut_dev *out, unsigned long long *errword,
                                    const sk_scan_args *a, int cu_count, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) uint32_t sk_wide_lds_bytes(uint32_t read_len);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_wide(const uint8_t *qual, const uint8_t *seq, sk_cut_dev *out, unsigned long long *errword,
                                     const sk_scan_args *a, int cu_count, hipStream_t stream);
// mixed-length ragged batches: the per-window regrouping (sk_sort.hip) and the scan of its tiles (sk_kernels.hip)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_sort(const uint64_t *offsets, uint64_t n_reads, uint32_t max_len, uint64_t *perm,
                                     unsigned long long *lists, uint32_t list_cap, uint32_t *counts, uint32_t *counts_of_next_scan,
                                     hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_sort_counted(const uint64_t *offsets, uint64_t n_reads, const uint64_t *n_reads_dev,
                                     uint32_t max_len, uint64_t *perm, unsigned long long *lists, uint32_t list_cap, uint32_t *counts,
                                     uint32_t *counts_of_next_scan, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_sorted(const uint8_t *qual, const uint8_t *seq, const uint64_t *offsets, const uint64_t *perm,
                                       const unsigned long long *lists, const uint32_t *counts, sk_cut_dev *out,
                                       unsigned long long *errword, const sk_scan_args *a, int cu_count, hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_pair_count(const sk_cut_dev *cuts, uint64_t n_pairs, uint8_t *classes,
                                           unsigned long long *counters, int cu_count, hipStream_t stream);
// device-side trimming (sk_trim.hip).  The caller's workspace, in 8-byte words: the header (SK_TRIM_HDR_WORDS), the table of
// the count kernel (SK_TRIM_BLOCK_WORDS per block of SK_TRIM_BLOCK_READS reads: records[3], bytes[3], lowest bad read; the
// scan turns records and bytes into the block's exclusive bases), then one source delta per record of the three outputs.
#define SK_TRIM_BLOCK_READS 2048u
#define SK_TRIM_BLOCK_WORDS 8u
#define SK_TRIM_HDR_WORDS 16u
#define SK_TRIM_H_RECORDS 0  // [3]
#define SK_TRIM_H_BYTES 3    // [3]
#define SK_TRIM_H_BAD 6      // lowest read with an invalid kept cut, or ~0
#define SK_TRIM_H_PRODUCED 7 // [3] offsets != NULL for an output of the mode
#define SK_TRIM_H_FIT 10     // [3] produced, no bad cut, and within its capacities: the place and gather kernels write it
#define SK_TRIM_GATHER_WG_PER_CU 7u // the gather kernel's occupancy (SGPR-bound): a persistent grid with no second round
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_trim(const sk_batch *b, const sk_cut_dev *cuts, int mode,
                                                                           const sk_trim_output *out, void *workspace,
                                                                           int cu_count, hipStream_t stream);
// FASTQ text on the device (sk_fastq.hip).  The caller's workspace (16-byte sections, sizes in bytes, T = text bytes of all
// inputs, H = (T + 2) / 16, G = (T + 7) / 8):
//   header    SK_FQ_HDR_WORDS words
//   chunks    16 per framing chunk of SK_FQ_CHUNK_BYTES (T / 65536 + 3 chunks at most over both inputs): '\n' count, last '\n'
//   desc      40 per record slot, 2G + 2 slots: name start and the end of each of the four lines of record k
//   offsets   8 * (N + 2), N = 2H + 2: the packed batch's offsets (n_pack + 1 of them)
//   cuts      8 * N
//   blocks    64 per block of SK_FQ_BLOCK_READS packed reads (the pack's, then the emission's block table)
//   emit      16 * N: output offset and read of every emitted record
//   qual, seq 16 * ceil(T / 32) each (seq only with trunc_n): the packed batch
// Sizing by the worst case, without a look at the text: a valid record is at least 8 bytes ("@a\nA\n+\nI\n"; 7 for an
// unterminated last one), so text i of b bytes holds at most (b + 1) / 8 valid records and at most b / 2 bytes of qual.
// The packed batch is sized by that; a text with more records than it holds is SK_EFORMAT.  The descriptors are sized by
// the lines of any text, valid or not: b bytes hold at most b lines, so b / 4 + 1 slots take every line of text i, and
// the ordered calls, whose batches and counts are a matter of lines alone, see all of them (with (b + 1) / 8 + 1 slots
// they stopped at the last slot of a text of empty lines).  The clamps at the slot count in the kernels never bite.
// SK_FQ_HDR_WORDS and the header's words, SK_FQ_H_* and the piece calls' SK_FQP_H_*, the sections (sk_fq_layout_of, SK_FQ_CHUNK_BYTES,
// SK_FQ_BLOCK_READS) and the ordered calls' shifts: sk_fastq_words.h (no HIP: the host reads them too)
struct sk_fq_clip_front;
// order: NULL = read order (sk_trim_fastq_device_async).  lengths: NULL = in->bytes are the texts' lengths; else
// (sk_trim_fastq_chained_device_async) in->bytes are bounds and the framing kernels, the only ones that look at a text's
// length, take it from the device words: everything behind them reads lines and records from the header.
// piece: NULL = the whole text; else (sk_trim_fastq_piece_device_async) text i starts at *piece->start_dev[i], with
// piece->more only whole records (pairs) are taken, and errword is the stream's range-error word for the frame scan to
// capture.  The emission takes the piece from the header.
// mode: the call's; SK_TRIM_PE_COMBO_ALL frames, pairs and orders as SK_TRIM_PE_INTERLEAVED and differs in the emission
// alone, which takes fail_qual, the Q of its N records (sk_fastq_record.h).
// counted: the packed batch is for sk_scan_counted_device_async with *n_reads_dev (the header's SK_FQ_H_NREAL) -- packed->n_reads
// stays the bound -- and the per-read steps of the pack and the emission stop at that word too; 0: everything walks the bound.
// clip: NULL = no clip; else (sk_trim_fastq_clipped_device_async) the search of sk_launch_fastq_clip runs behind the check
// and the pack takes a read's length through its clip word (sk_fastq_clip.h).
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
                                                                                  const struct sk_fq_clip_front *clip);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_emit(const sk_fastq_input *in, int mode, int trunc_n,
                                                                                 int counted, const sk_fastq_order *order,
                                                                                 int piece, int fail_qual,
                                                                                 const sk_fastq_output *out, void *workspace,
                                                                                 const unsigned long long *errword, int cu_count,
                                                                                 hipStream_t stream);
// Ordered pieces (sk_trim_fastq_ordered_piece_device_async; the workspace: sk_fq_order_piece_shift, sk_fastq_words.h).
// state_in / state_out: sk_fastq_order_state in device memory (state_in NULL = the start of a stream).
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_order_piece_front(
    const sk_fastq_input *in, const sk_fastq_lengths *lengths, int mode, int trunc_n, int counted, const sk_fastq_order *order,
    const sk_fastq_piece *piece, const void *state_in, void *state_out, const unsigned long long *errword, void *workspace,
    int cu_count, hipStream_t stream, sk_batch *packed, sk_cut_dev **cuts, const uint64_t **n_reads_dev,
    const struct sk_fq_clip_front *clip);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_order_piece_emit(
    const sk_fastq_input *in, int mode, int trunc_n, int counted, const sk_fastq_order *order, const void *state_in,
    void *state_out, int fail_qual, const sk_fastq_output *out, void *workspace, const unsigned long long *errword,
    int cu_count, hipStream_t stream);
// BGZF on the device (sk_bgzf.hip).  The caller's workspace (16-byte sections, sizes in bytes, NB = ceil(text bytes /
// SK_BGZF_BLOCK) blocks, G = min(NB, SK_BGZF_GRID) workgroups of the block kernel):
//   header    SK_BGZF_HDR_WORDS words
//   table     16 per block: body bytes (bit 31: stored), CRC-32, the member's offset in the image
//   tokens    4 * SK_BGZF_TOK_WORDS per workgroup of the block kernel: one token per text byte of the block in flight
//   slots     65536 per block: its deflate stream
//   cand      with SK_BGZF_SEARCH only, behind everything else (at sk_bgzf_layout.total): 4 * SK_BGZF_TOK_WORDS per
//             workgroup of the block kernel, the search's candidate match for each text byte of the block in flight
// The grid is a constant, not the device's CU count: the size must not depend on a device (5 workgroups per CU by LDS on
// the 256 CUs of an MI355X; on fewer CUs the surplus workgroups wait their turn).
#define SK_BGZF_BLOCK 65280u
#define SK_BGZF_SLOT 65536u
#define SK_BGZF_GRID 1280u
#define SK_BGZF_TOK_WORDS (SK_BGZF_BLOCK + 8u)
#define SK_BGZF_MEMBER_EXTRA 31u // a stored member: 18 + 5 + 8 bytes beyond its text
#define SK_BGZF_EOF_BYTES 28u
#define SK_BGZF_HDR_WORDS 16u
#define SK_BGZF_H_BYTES_IN 0
#define SK_BGZF_H_BLOCKS 1
#define SK_BGZF_H_STORED 2
#define SK_BGZF_H_BYTES_OUT 3 // what the image needs
#define SK_BGZF_H_FIT 4       // the image is within the capacity: the pack kernel writes it
struct sk_bgzf_entry {
    uint32_t body, crc;
    uint64_t off;
};
struct sk_bgzf_layout {
    uint64_t n_blocks, grid, table, tokens, slots, total;
};
static inline void sk_bgzf_layout_of(uint64_t text_bytes, sk_bgzf_layout *L)
{
    L->n_blocks = text_bytes / SK_BGZF_BLOCK + (text_bytes % SK_BGZF_BLOCK != 0);
    L->grid = L->n_blocks < SK_BGZF_GRID ? L->n_blocks : SK_BGZF_GRID;
    L->table = 8 * SK_BGZF_HDR_WORDS;
    L->tokens = L->table + 16 * L->n_blocks;
    L->slots = L->tokens + 4ull * SK_BGZF_TOK_WORDS * L->grid;
    L->total = L->slots + (uint64_t)SK_BGZF_SLOT * L->n_blocks;
}
static inline uint64_t sk_bgzf_search_bytes(const sk_bgzf_layout *L) { return 4ull * SK_BGZF_TOK_WORDS * L->grid; }
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_bgzf(const sk_bgzf_input *in, uint8_t *out, uint64_t capacity,
                                                                           int flags, void *workspace, int cu_count,
                                                                           hipStream_t stream);
// BGZF read on the device (sk_inflate.hip).  The caller's workspace (16-byte sections, sizes in bytes, n = image bytes):
//   header    SK_INFLATE_HDR_WORDS words
//   tiles     4 per tile of SK_INFLATE_TILE byte positions (n / 4096 + 1 tiles): candidates in the tile, then their base
//   cand      8 per candidate: its position.  A candidate is a match of 1f 8b 08 04, and matches cannot overlap, so an
//             image holds n / 4 at most, whatever its bytes; + 1
//   next a/b  4 per candidate each: the successor's index, ping-pong for the pointer doubling
//   rank      4 per candidate: its member number if the chain from position 0 reaches it
//   table     40 per member: n / 26 + 1 members at most (SK_INFLATE_MIN_MEMBER bytes each)
// The grids are constants, not the device's CU count: 16 single-wave workgroups per CU on the 256 CUs of an MI355X.
#define SK_INFLATE_TILE 4096u
#define SK_INFLATE_MIN_MEMBER 26u
#define SK_INFLATE_GRID 4096u
#define SK_INFLATE_FRAME_GRID 2048u
#define SK_INFLATE_MAX_IMAGE (1ull << 33) // the candidates' indices are 32-bit
#define SK_INFLATE_HDR_WORDS 16u
#define SK_INFLATE_H_BYTES_IN 0
#define SK_INFLATE_H_MEMBERS 1
#define SK_INFLATE_H_BYTES_OUT 2
#define SK_INFLATE_H_FIT 3          // count-only, or the text is within the capacity: the inflate kernel writes it
#define SK_INFLATE_H_ERROR_KEY 4    // (member << 3) | SK_GZ_* of the lowest bad member, or ~0
#define SK_INFLATE_H_FRAME_KEY 5    // the same for the framing error alone
#define SK_INFLATE_H_FRAME_OFFSET 6 // its byte offset (a member that framed has its offset in the table)
#define SK_INFLATE_H_CANDIDATES 7
#define SK_INFLATE_H_WRITTEN 8      // 1 iff the call decoded, without an error, a text within the capacity (sk_bgzf_inflate_output_words)
struct sk_inflate_entry {
    uint64_t image_off, out_off;
    uint32_t body_off, body_len; // the deflate stream, relative to image_off
    uint32_t isize, crc;
    uint32_t verdict, reserved;  // SK_GZ_*
};
struct sk_inflate_layout {
    uint64_t n_tiles, n_cand, n_table, rounds, tiles, cand, next_a, next_b, rank, table, total;
};
static inline uint64_t sk_inflate_a16(uint64_t x) { return (x + 15) & ~15ull; }
static inline void sk_inflate_layout_of(uint64_t image_bytes, sk_inflate_layout *L)
{
    L->n_tiles = image_bytes / SK_INFLATE_TILE + 1;
    L->n_cand = image_bytes / 4 + 1;
    L->n_table = image_bytes / SK_INFLATE_MIN_MEMBER + 1;
    L->rounds = 0;
    while ((1ull << L->rounds) < L->n_table) ++L->rounds; // ranks are below n_table
    L->tiles = 8 * SK_INFLATE_HDR_WORDS;
    L->cand = L->tiles + sk_inflate_a16(4 * L->n_tiles);
    L->next_a = L->cand + sk_inflate_a16(8 * L->n_cand);
    L->next_b = L->next_a + sk_inflate_a16(4 * L->n_cand);
    L->rank = L->next_b + sk_inflate_a16(4 * L->n_cand);
    L->table = L->rank + sk_inflate_a16(4 * L->n_cand);
    L->total = L->table + sk_inflate_a16(sizeof(sk_inflate_entry) * L->n_table);
}
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_bgzf_inflate(const uint8_t *image, uint64_t image_bytes,
                                                                                   uint8_t *out, uint64_t capacity,
                                                                                   void *workspace, hipStream_t stream);
// Plain gzip read on the device (sk_gunzip.hip, sk_gunzip_block.h).  The caller's workspace (16-byte sections, sizes in
// bytes, n = image bytes, S = ceil(n / chunk) stretches, chunk = sk_gunzip_chunk_of(n)):
//   header    SK_GUNZIP_HDR_WORDS words
//   stretches 128 per stretch, S + 1
//   used      8 * (S + 1) text offsets and 4 * (S + 1) stretch numbers of the chain from bit 0
//   members   32 per member end: n / 18 + 1 (two trailers lie 18 bytes apart at least)
//   symbols   2 * capacity: the text as 16-bit symbols
// The chunk: 32 KiB, doubled until 4096 chunks cover the image (the decode kernels' grids are 4096 single-wave
// workgroups); SK_GZIP_CHUNK (a power of two of 256 or more) replaces it.
#define SK_GUNZIP_HDR_WORDS 32u
#define SK_GUNZIP_H_BYTES_OUT 2 // the header words sk_gzip_inflate_output_words hands out (== SKG_H_* of sk_gunzip_block.h)
#define SK_GUNZIP_H_WRITTEN 11
#define SK_GUNZIP_STRETCH_BYTES 128u
#define SK_GUNZIP_MEMBER_BYTES 32u
#define SK_GUNZIP_MIN_CHUNK 32768u
#define SK_GUNZIP_GRID 4096u
#define SK_GUNZIP_MAX_IMAGE (1ull << 33)
struct sk_gunzip_layout {
    uint64_t chunk, S, n_members, stretches, u_off, u_id, members, sym, total;
};
static inline uint64_t sk_gunzip_chunk_of(uint64_t image_bytes, uint64_t forced)
{
    if (forced) return forced;
    uint64_t c = SK_GUNZIP_MIN_CHUNK;
    while (c * SK_GUNZIP_GRID < image_bytes) c <<= 1;
    return c;
}
static inline void sk_gunzip_layout_of(uint64_t image_bytes, uint64_t capacity, uint64_t forced_chunk, sk_gunzip_layout *L)
{
    L->chunk = sk_gunzip_chunk_of(image_bytes, forced_chunk);
    L->S = image_bytes / L->chunk + (image_bytes % L->chunk != 0);
    L->n_members = image_bytes / 18 + 1;
    L->stretches = 8 * SK_GUNZIP_HDR_WORDS;
    L->u_off = L->stretches + SK_GUNZIP_STRETCH_BYTES * (L->S + 1);
    L->u_id = L->u_off + sk_inflate_a16(8 * (L->S + 1));
    L->members = L->u_id + sk_inflate_a16(4 * (L->S + 1));
    L->sym = L->members + (uint64_t)SK_GUNZIP_MEMBER_BYTES * L->n_members;
    L->total = L->sym + sk_inflate_a16(2 * capacity);
}
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_gunzip(const uint8_t *image, uint64_t image_bytes, uint8_t *out,
                                                                             uint64_t capacity, uint64_t forced_chunk,
                                                                             void *workspace, hipStream_t stream);
// Plain gzip read in pieces (sk_gunzip_piece.hip): the workspace above for an image of window_bytes, with
//   symbols   2 * (32768 + capacity): the state's history as literals in front of the text
//   members   one entry more: the member in progress at the piece's end
//   resume    32 per stretch, S + 1: each stretch's last resume point, and the bit its decode stops at
#define SK_GUNZIP_RESUME_BYTES 32u
#define SK_GUNZIP_H_P_LIMITED 17 // the header words sk_gzip_inflate_piece_device_finish reads (== SKG_H_P_* of sk_gunzip_block.h)
#define SK_GUNZIP_H_P_DONE 18
#define SK_GUNZIP_H_P_STATUS 19
#define SK_GUNZIP_H_P_ERROR 20
#define SK_GUNZIP_H_P_ERROR_MEMBER 21
#define SK_GUNZIP_H_P_ERROR_OFFSET 22
#define SK_GUNZIP_H_P_INHERITED 23
#define SK_GUNZIP_H_P_POS_BIT 24
#define SK_GUNZIP_H_P_IN_MEMBER 25
#define SK_GUNZIP_H_P_IMAGE_OFFSET 27
#define SK_GUNZIP_PIECE_SHIFT 32768u
#define SK_GUNZIP_MAX_WINDOW (1ull << 33)
struct sk_gunzip_piece_layout {
    sk_gunzip_layout g;
    uint64_t resume, total;
};
static inline void sk_gunzip_piece_layout_of(uint64_t window_bytes, uint64_t capacity, uint64_t forced_chunk, sk_gunzip_piece_layout *L)
{
    sk_gunzip_layout *g = &L->g;
    g->chunk = sk_gunzip_chunk_of(window_bytes, forced_chunk);
    g->S = window_bytes / g->chunk + (window_bytes % g->chunk != 0);
    g->n_members = window_bytes / 18 + 2;
    g->stretches = 8 * SK_GUNZIP_HDR_WORDS;
    g->u_off = g->stretches + SK_GUNZIP_STRETCH_BYTES * (g->S + 1);
    g->u_id = g->u_off + sk_inflate_a16(8 * (g->S + 1));
    g->members = g->u_id + sk_inflate_a16(4 * (g->S + 1));
    L->resume = g->members + (uint64_t)SK_GUNZIP_MEMBER_BYTES * g->n_members;
    g->sym = L->resume + SK_GUNZIP_RESUME_BYTES * (g->S + 1);
    g->total = L->total = g->sym + sk_inflate_a16(2 * (SK_GUNZIP_PIECE_SHIFT + capacity));
}
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_gunzip_piece(const uint8_t *image, uint64_t image_bytes,
                                                                                   const sk_gzip_piece *piece, const void *state_in,
                                                                                   void *state_out, uint8_t *out, uint64_t capacity,
                                                                                   uint64_t forced_chunk, void *workspace,
                                                                                   hipStream_t stream);
// the carry between two pieces (sk_fastq_piece.hip): sk_fastq_carry_device_async's arguments as they are, prev_hdr the
// previous piece's header or NULL
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_carry(const uint64_t *prev_hdr, int input,
                                                                                  const uint8_t *prev_text, uint8_t *next_text,
                                                                                  uint64_t room, const uint64_t *chunk_bytes_dev,
                                                                                  uint64_t chunk_bytes,
                                                                                  const uint64_t *chunk_valid_dev,
                                                                                  const sk_fastq_carry_words *prev_words,
                                                                                  const sk_fastq_carry_words *other_prev_words,
                                                                                  sk_fastq_carry_words *words, hipStream_t stream);
// the trim report over a text call's workspace (sk_fastq_report.hip); the arguments have passed the checks of
// sk_trim_fastq_report_device_async
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_report(const sk_fastq_report_source *src,
                                                                                   sk_fastq_report *report_dev,
                                                                                   const sk_fastq_report_hists *hists, int flags,
                                                                                   hipStream_t stream);
// the audit over a text call's workspace and texts (sk_fastq_audit.hip); the arguments have passed the checks of
// sk_trim_fastq_audit_device_async
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_audit(const sk_fastq_report_source *src,
                                                                                  const sk_fastq_input *in, int mode,
                                                                                  sk_fastq_audit *audit_dev,
                                                                                  uint64_t *qual_hist_dev, int flags,
                                                                                  hipStream_t stream);
// the bases over a text call's workspace and texts (sk_fastq_bases.hip); the arguments have passed the checks of
// sk_trim_fastq_bases_device_async
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_bases(const sk_fastq_report_source *src,
                                                                                  const sk_fastq_input *in, int mode,
                                                                                  sk_fastq_bases *bases_dev,
                                                                                  const sk_fastq_bases_hists *hists, int flags,
                                                                                  hipStream_t stream);
// the rejects text over a text call's workspace and texts (sk_fastq_rejects.hip); the arguments have passed the checks of
// sk_trim_fastq_rejects_device_async
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_rejects(const sk_fastq_report_source *src,
                                                                                    const sk_fastq_input *in, int mode,
                                                                                    const sk_fastq_output *out, int flags,
                                                                                    void *workspace, int cu_count,
                                                                                    hipStream_t stream);
// the adapter search over a text call's workspace and texts (sk_fastq_adapters.hip); the arguments have passed the checks
// of sk_trim_fastq_adapters_device_async
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_adapters(const sk_fastq_report_source *src,
                                                                                     const sk_fastq_input *in, int mode,
                                                                                     const sk_fastq_adapter_set *set,
                                                                                     sk_fastq_adapters *adapters_dev,
                                                                                     const sk_fastq_adapters_out *out, int flags,
                                                                                     int cu_count, hipStream_t stream);
// the clip of a clipped text call (sk_trim_fastq_clipped_device_async; sk_fastq_adapters.hip, sk_fastq_clip.h).
// sk_fq_clip_front: what such a call hands its front launcher, which passes a NULL for every other call: the set and the
// clip section of the workspace, the call-local stats block (128 bytes) with the clip words behind it.
struct sk_fq_clip_front {
    const sk_fastq_adapter_set *set;
    void *section;
};
// sk_fq_clip_src: the front's view of the text and the workspace, as the search kernel takes it
struct sk_fq_clip_src {
    const uint64_t *hdr;
    const uint64_t *desc[2]; // 5 words per slot
    uint64_t slots[2];
    const uint8_t *text[2];
    uint64_t bytes[2]; // the lengths, or their bounds
    const uint64_t *bytes_dev[2], *valid_dev[2];
    uint64_t n_pack;
    int32_t mode; // the framing mode
};
// behind the front's check, in front of its pack: zeroes the section's stats block, then searches
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_clip(const sk_fq_clip_src *src,
                                                                                 const sk_fq_clip_front *clip, int cu_count,
                                                                                 hipStream_t stream);
// zeroes a caller's sk_fastq_clip_stats (SK_FQ_CLIP_RESET)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_clip_reset(sk_fastq_clip_stats *stats_dev,
                                                                                       hipStream_t stream);
// behind the emission: the section's sums into stats_dev, by the validity of the call behind `workspace` (kind:
// SK_FQ_REPORT_*; mode: the call's)
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_clip_commit(const void *workspace, uint32_t kind,
                                                                                        int mode, const void *section,
                                                                                        sk_fastq_clip_stats *stats_dev,
                                                                                        hipStream_t stream);
extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_read_probe(const void *buf, size_t bytes, uint32_t *sink, int cu_count,
                                           hipStream_t stream);
#endif
