/*
 * sickle_amd.h -- C ABI of libsickle_amd.so: the MI355X (gfx950) replacement for the
 * per-batch quality scan of pentalpha/sickle.
 *
 * The reference has no FFI; the seam this ABI fills is what its worker threads do for
 * one batch:
 *   Trim_Single::processing_thread   reference src/trim_single.cpp:357-372
 *   Trim_Paired::processing_thread   reference src/trim_paired.cpp:483-504
 * i.e. `saved_cutsites[i] = sliding_window(*queue[i])` for every read of the batch, with
 *   Abstract_Trimmer::sliding_window  reference src/trim.cpp:3-116
 *   Abstract_Trimmer::get_quality_num reference src/trim.cpp:118-140
 * Conventions kept from the reference: the result per read is its `cutsites` pair
 * (src/sickle.h:93-96), a read is kept iff three >= 0 (src/trim_single.cpp:368), and a
 * quality character outside the encoding's range is fatal (src/trim.cpp:129-137).
 * Conventions changed because this is a library: the caller owns every buffer, nothing
 * is malloc'd per read, and the range error is RETURNED (sk_err) instead of exit(1) --
 * the host pipeline prints the reference's message and exits.
 *
 * There is no CPU fallback: every entry point that computes runs the HIP kernels and
 * fails (SK_ENODEV / SK_EHIP) when no gfx950 device is usable.
 *
 * Batch layout (struct-of-arrays, packed by the ingest side):
 *   ragged      : offsets != NULL; read r = bytes [offsets[r], offsets[r+1]) of qual (and seq),
 *                 offsets ascending.  batch->stride is then a HINT: the longest read of the batch
 *                 (0 = unknown), which sizes the kernel's LDS tiles (sk_submit / sk_trim_batch see
 *                 the offsets and work it out themselves).  (ABI 1 ignored `stride` on such batches: a
 *                 caller that leaves a stale value there gets the right cuts from a slower kernel --
 *                 above 4096 the batch goes to the long-read kernel whole.  Set it to 0 or to the truth.)
 *                 A batch of 65 536 reads or more whose reads differ in length is regrouped on the
 *                 device first (windows of 8192 reads counting-sorted by window width, ~9 bytes of
 *                 scratch per read owned by the context, per stream): its tiles then hold reads of one
 *                 window width and take the matrix path; batches of one length and batches with reads
 *                 too long for a tile are scanned as they lie.  Cuts and errors keep the caller's numbering.  Tiles of 64 consecutive reads are
 *                 re-strided on their way into LDS and scanned one lane per read; a tile whose
 *                 reads are too long for that goes to the general kernel (a wave per read, the read
 *                 streamed through LDS: any length).  A hint beyond 4096 declares a long-read batch:
 *                 the general kernel takes all of it, in spans of equal cost per wave.
 *   fixed stride: offsets == NULL; read r = bytes [r*stride, r*stride + len_r) with
 *                 len_r = lengths ? lengths[r] : read_len.  Fastest: stride % 8 == 0, stride <=
 *                 SK_TILE_MAX_STRIDE, base pointers 16-byte aligned, stride/8 ODD (152, 104, 264
 *                 ...: the rows then spread over all LDS banks; stride/8 even still works, slower).
 *                 Any other stride <= SK_TILE_MAX_STRIDE or alignment (e.g. reads packed back to
 *                 back, stride == read_len) is re-strided like a ragged batch; longer rows: one
 *                 length (lengths == NULL) of up to ~2200 bases keeps the tile kernel with 32 or 16
 *                 reads to a tile (round 3), anything else goes through the general kernels.
 *   segmented   : tiles != NULL (offsets and lengths NULL).  The caller has grouped the reads
 *                 by length: tile t holds `rows` (<= 64) reads of `read_len` bytes each at
 *                 qual[byte_off + i*stride] (stride % 8 == 0, byte_off % 16 == 0), and slot
 *                 slot0+i of out_index[] says where read i's cut goes: out[out_index[slot0+i]] (or
 *                 out[slot0+i] with cuts_in_slot_order).
 *                 Every tile is uniform inside, so mixed-length batches keep the fast tiled
 *                 kernel (matrix-pipe window sums) with no padding to the longest read.
 *                 batch->stride = the largest tile stride, n_reads = number of reads.
 * seq is only read when params->trunc_n != 0 (the N rule, src/trim.cpp:86-98) and may be
 * NULL otherwise.
 */
#ifndef SICKLE_AMD_H
#define SICKLE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_ABI_VERSION 2

/* quality_type, reference src/sickle.h:61-66 */
enum { SK_PHRED = 0, SK_SANGER = 1, SK_SOLEXA = 2, SK_ILLUMINA = 3 };

/* return codes */
enum {
    SK_OK = 0,
    SK_ERANGE = 1, /* a quality char outside the encoding's range was read: *err is filled */
    SK_EINVAL = -1,
    SK_ENODEV = -2, /* no usable gfx950 device */
    SK_EHIP = -3,   /* a HIP runtime call failed: see sk_last_error() */
    SK_EBUSY = -4,  /* slot still in flight */
    SK_ESPACE = -5, /* sk_trim_device_finish: an output's buffers are too small (counts say what it needs) */
    SK_EFORMAT = -6 /* sk_trim_fastq_device_finish: a malformed FASTQ record (counts say which and why) */
};

#define SK_TILE_MAX_STRIDE 512u /* two LDS buffers of 64 reads per wave must fit the 160 KiB of a CU */
/* The longest read a batch may hold: 16 Mi bases (sk_err and the device's error word keep 24 bits of position).  The
 * reference has no such limit (it has no limits at all: std::string).  sk_submit / sk_trim_batch return SK_EINVAL for
 * an `offsets` batch with a longer read, and so does a fixed-stride batch with read_len beyond it; the CLI names the
 * record and exits 1. */
#define SK_MAX_READ_LEN (1u << 24)

/* the config ints of Abstract_Trimmer, reference src/trim.h:16-20 */
typedef struct {
    int32_t qualtype;         /* SK_SANGER / SK_SOLEXA / SK_ILLUMINA (SK_PHRED accepted) */
    int32_t qual_threshold;   /* -q, >= 0 */
    int32_t length_threshold; /* -l, >= 0 */
    int32_t no_fiveprime;     /* -x */
    int32_t trunc_n;          /* -n */
} sk_params;

/* == reference `cutsites`, src/sickle.h:93-96; discarded reads are (-1,-1) */
typedef struct {
    int32_t five;
    int32_t three;
} sk_cut;

/* the first out-of-range quality char: what src/trim.cpp:130-135 prints */
typedef struct {
    uint32_t read; /* lowest erroring read index in the batch */
    uint32_t pos;  /* 0-based position in the read (the reference prints pos+1) */
    int32_t ch;    /* (int)(char) value, i.e. bytes >= 0x80 are negative */
} sk_err;

/* one tile of a segmented batch */
typedef struct {
    uint64_t byte_off; /* of the tile's first read in qual (and seq); multiple of 16 */
    uint32_t slot0;    /* index of the tile's first read in out_index[] */
    uint32_t stride;   /* bytes between the tile's reads; multiple of 8, <= SK_TILE_MAX_STRIDE */
    uint16_t rows;     /* reads in this tile, 1..64 */
    uint16_t read_len; /* their common length, <= stride */
    uint32_t reserved; /* 0 */
} sk_tile;

/* a run of tiles of a segmented batch that is launched together (optional, see sk_batch) */
typedef struct {
    uint32_t first_tile; /* index of the run's first tile */
    uint32_t n_tiles;
    uint32_t max_stride; /* the largest tile stride in the run: sizes the LDS buffer of its waves */
    uint32_t wide;       /* != 0 if any tile of the run has read_len / 10 > 33 */
} sk_seg_class;

typedef struct {
    const uint8_t *qual;
    const uint8_t *seq;      /* NULL unless trunc_n */
    const uint64_t *offsets; /* n_reads+1 entries, or NULL */
    uint32_t stride;         /* fixed-stride layout; segmented: the largest tile stride; ragged: longest read or 0 */
    uint32_t read_len;       /* fixed-stride layout with lengths == NULL */
    const uint32_t *lengths; /* fixed-stride layout, per-read lengths, or NULL */
    uint64_t n_reads;
    const sk_tile *tiles;      /* segmented layout: n_tiles descriptors, or NULL */
    uint32_t n_tiles;
    const uint32_t *out_index; /* segmented layout: n_reads entries */
    /* segmented layout, optional: the tile array cut into runs that are launched one after the other,
     * each with LDS sized for its own widest row (a batch sorted by length then gives its short reads
     * full occupancy).  HOST memory, also for device-resident batches; NULL = one run (sk_submit /
     * sk_trim_batch then cut the host tiles themselves).  sk_seg_classes() fills such a table. */
    const sk_seg_class *classes;
    uint32_t n_classes;
    /* segmented layout, optional: != 0 = out[slot] takes the cut of the read in slot `slot` (tile order)
     * instead of out[out_index[slot]].  The device then writes its cuts as one coalesced stream (the
     * scattered 8-byte stores cost 22 % extra HBM traffic on a 75-301 bp mix) and the caller, who has
     * out_index, puts them in order while it consumes them.  Range errors are still reported with the
     * caller's read number (out_index is only consulted for an erroring read). */
    uint32_t cuts_in_slot_order;
} sk_batch;

typedef struct sk_ctx sk_ctx;

/* {offset, min, max} of an encoding, reference src/sickle.h:85-91; NULL if qualtype invalid */
const int32_t *sk_quality_constants(int32_t qualtype);
/* "Phred" / "Sanger" / "Solexa" / "Illumina", reference src/sickle.h:68-73 */
const char *sk_typename(int32_t qualtype);
int sk_abi_version(void);
/* number of visible HIP devices (0 when none / no driver) */
int sk_device_count(void);

/* One context per device and host thread of use; owns two streams (compute, copy) and
 * `slots` staging slots for the asynchronous host path.  device < 0 -> current device. */
int sk_create(int device, int slots, sk_ctx **out);
void sk_destroy(sk_ctx *ctx);
const char *sk_last_error(const sk_ctx *ctx);
int sk_device(const sk_ctx *ctx);

/* pinned host memory for batches and cut arrays (plain malloc'd memory also works with
 * sk_submit, only slower) */
void *sk_host_alloc(sk_ctx *ctx, size_t bytes);
void sk_host_free(sk_ctx *ctx, void *p);

/*
 * Device-resident batch: every pointer in *batch and `out` is a DEVICE pointer.  Enqueues
 * the scan on `hip_stream` (a hipStream_t; NULL = HIP's default stream, so it is ordered after
 * the work the caller queued there) and
 * returns without waiting.  out[r] is written for every read.  Range errors of the scans enqueued
 * on one stream since that stream's last sk_scan_device_finish accumulate in one device word per
 * stream (lowest read index wins), so scans on different streams of one context do not steal each
 * other's errors; nothing but the kernel(s) is enqueued here.  One host thread per context at a time.
 */
int sk_scan_device_async(sk_ctx *ctx, const sk_params *params, const sk_batch *batch,
                         sk_cut *out, void *hip_stream);
/* Waits for the stream and reports (and clears) the range error of the scans enqueued on it
 * since the previous finish: SK_OK, or SK_ERANGE with *err filled.  After SK_ERANGE the cuts of the scan are
 * undefined, and so is what sk_trim_device_async made of them. */
int sk_scan_device_finish(sk_ctx *ctx, void *hip_stream, sk_err *err);

/*
 * Host batch, synchronous: H2D, scan, D2H.  What processing_thread does for one batch.
 * Returns SK_OK, SK_ERANGE (*err filled; `out` then holds the cuts of the reads the device
 * still scanned, the caller is expected to abort like the reference does) or < 0.
 */
int sk_trim_batch(sk_ctx *ctx, const sk_params *params, const sk_batch *batch, sk_cut *out,
                  sk_err *err);

/*
 * Host batch, asynchronous, double-buffered: sk_submit copies the batch to the device on
 * the copy stream, scans it on the compute stream and copies the cuts back into `out`;
 * sk_wait blocks until that slot is done.  The caller keeps *batch's buffers and `out`
 * alive and untouched in between.  With slots >= 2 the H2D copy of one batch overlaps the
 * scan of the previous one.
 */
int sk_submit(sk_ctx *ctx, int slot, const sk_params *params, const sk_batch *batch, sk_cut *out);
int sk_wait(sk_ctx *ctx, int slot, sk_err *err);

/* Cuts the n_tiles HOST tile descriptors into at most max_classes runs of equal occupancy class (and
 * of equal need for the wide-window matrix loop), merging runs too short to fill the device.
 * Returns the number of runs written to out (>= 1 for n_tiles > 0), or 0 when the tiles change class
 * too often for max_classes runs (pass classes = NULL then). */
uint32_t sk_seg_classes(const sk_tile *tiles, uint32_t n_tiles, sk_seg_class *out, uint32_t max_classes);

/* Which kernel a batch of this shape would use: 1 = tiled (lane per read, LDS tile by LDS-DMA),
 * 8 = uniform medium reads (fixed stride, one length of ~505 .. 2200 bases: tiles of 32 or 16 reads, a pair / four lanes
 * per read, windows of any width on the matrix path), 2 = general, medium reads (teams of 16 lanes per read, up to a
 * longest read of 4096: ragged medium reads, uniform ones beyond 8's range), 6 = general, long reads (a
 * wave per read with the read streamed through LDS), 3 = tiled over a segmented batch, 4 = tiled with the tile
 * staged through registers (equal lengths, no sequence buffer, row stride 72..320), 5 = tiled with rows re-strided
 * on the way into LDS (packed / misaligned fixed stride, ragged; a ragged batch of mixed lengths is regrouped on
 * the device first -- the device decides, so the answer stays 5).  7 = round 3's matrix-pipe wave-per-read kernel
 * for medium reads (sk_band.hip): built and parity-tested, no shape selects it (SK_GENERAL=band forces it; it is
 * not faster than 2).  For tests and bench labels. */
int sk_kernel_for(const sk_batch *batch);

/* For bench.py's roofline: name of the dominant kernel as rocprofv3 reports it */
const char *sk_kernel_name(int which);

/*
 * Pair classification on the device: reference src/trim_paired.cpp:543-567.  `cuts` (DEVICE pointer, the
 * output of a scan in read order) holds the mates of pair k at 2k and 2k+1; a mate is kept iff its three >= 0
 * (src/trim_paired.cpp:500,502).  Counts the four classes into the context (per stream, like the error word)
 * and, if classes != NULL (device pointer, n_pairs bytes), writes each pair's class: SK_PAIR_BOTH (both kept:
 * two paired records), SK_PAIR_FIRST / SK_PAIR_SECOND (one single record), SK_PAIR_NONE.  The reference's
 * six counters follow: kept_p = 2*both, kept_s1 = discard_s2 = only_first, kept_s2 = discard_s1 =
 * only_second, discard_p = 2*none.  Enqueued on hip_stream behind the scan that produced `cuts`.
 */
enum { SK_PAIR_BOTH = 0, SK_PAIR_FIRST = 1, SK_PAIR_SECOND = 2, SK_PAIR_NONE = 3 };
typedef struct {
    uint64_t both, only_first, only_second, none; /* pairs */
} sk_pair_counts;
int sk_count_pairs_device_async(sk_ctx *ctx, const sk_cut *cuts, uint64_t n_pairs, uint8_t *classes, void *hip_stream);
/* Waits for the stream, returns and clears the counts accumulated on it since the last finish. */
int sk_count_pairs_device_finish(sk_ctx *ctx, void *hip_stream, sk_pair_counts *counts);

/*
 * Trimming on the device: the cuts of a scan applied to a device-resident batch, the kept records packed back to back.
 * Reference src/trim_single.cpp:374-428 (output_single: substr + filter) and src/trim_paired.cpp:506-567 (output_paired:
 * the pair routing), without the FASTQ text: for reads that go on to more GPU work.  Every pointer is a DEVICE pointer.
 *
 * A read is kept iff its three >= 0 (src/trim_single.cpp:368, src/trim_paired.cpp:500,502); its record is bytes
 * [five, three) of its qual (and seq).  Records stay in read order.  In the PE modes the mates of pair k are reads 2k and
 * 2k+1 (n_reads must be even) and the pair rule of sk_count_pairs_device_async routes them: both kept -> the paired
 * output(s), one kept -> out[2] (singles), none -> dropped.
 *   SK_TRIM_SE              out[0]: every kept read                                       (out[1], out[2] unused)
 *   SK_TRIM_PE_SPLIT        out[0]: mate 1 of the pairs with both kept, out[1]: their mate 2, out[2]: singles
 *   SK_TRIM_PE_INTERLEAVED  out[0]: both mates of such pairs (2k, then 2k+1), out[2]: singles   (out[1] unused)
 * An output is produced iff its `offsets` is not NULL; then offsets[0..records] are its record boundaries (offsets[0] = 0,
 * offsets[records] = bytes), so (qual, seq, offsets) is an `offsets` sk_batch of `records` reads as it stands, and
 * read_index[j] (if not NULL) is the input read of record j.  qual / seq may each be NULL (no bytes written); seq must be
 * NULL when batch->seq is.
 * Capacity: an output whose records exceed record_capacity, or (with qual or seq given) whose bytes exceed
 * byte_capacity, gets NOTHING written, not even offsets; sk_trim_device_finish then returns SK_ESPACE with the counts,
 * so the caller can size its buffers and call again.  With every offsets NULL the call only counts.
 * Batches: `offsets` and fixed-stride layouts (read_len or lengths), reads up to SK_MAX_READ_LEN, input pointers of any
 * alignment.  Segmented batches (tiles != NULL) are SK_EINVAL.  out[].qual / seq must be 16-byte aligned, offsets /
 * read_index 8-byte aligned, cuts 8-byte aligned.
 * Invalid kept cuts (five < 0, five > three or three > the read's length; a scan never writes one, hand-made cuts can
 * hold them) make finish return SK_EINVAL with bad_read = the lowest such read, and nothing is written to any output.
 *
 * sk_trim_device_async only enqueues four kernels on hip_stream (no allocation, no copy, no synchronisation: it may be
 * captured into a graph); every bit of scratch and the counts live in `workspace` (device, 16-byte aligned, at least
 * sk_trim_workspace_bytes(n_reads) bytes: 128 + 64 * ceil(n_reads / 2048) + 8 * n_reads, i.e. below
 * 8.04 bytes per read + 192 bytes).  sk_trim_device_finish is the only call that waits: it reads the counts out of the
 * workspace after the stream's work.  Two trims in flight at once need two workspaces.
 * The workspace's contents on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.
 */
typedef struct {
    uint8_t *qual;            /* device, 16-byte aligned, or NULL (then no bytes are written) */
    uint8_t *seq;             /* device, 16-byte aligned, or NULL; must be NULL if batch->seq is NULL */
    uint64_t *offsets;        /* device, record_capacity + 1 entries (offsets[0] = 0), or NULL = output not produced */
    uint64_t *read_index;     /* device, record_capacity entries: the input read number of each record, or NULL */
    uint64_t byte_capacity;   /* bytes available in qual (and in seq) */
    uint64_t record_capacity; /* entries available in read_index; offsets holds record_capacity + 1 */
} sk_trim_output;

/* SK_TRIM_PE_COMBO_ALL is a mode of the FASTQ text calls only (below): sk_trim_device_async returns SK_EINVAL for it, since
 * a packed read has no name line for an N record to keep. */
enum { SK_TRIM_SE = 0, SK_TRIM_PE_SPLIT = 1, SK_TRIM_PE_INTERLEAVED = 2, SK_TRIM_PE_COMBO_ALL = 3 };

typedef struct {
    uint64_t records[3], bytes[3]; /* what each output needs, also when it was not produced or did not fit */
    uint64_t bad_read;             /* lowest read with an invalid kept cut, or UINT64_MAX */
} sk_trim_counts;

size_t sk_trim_workspace_bytes(uint64_t n_reads);
/* Enqueues the trim of `batch` by `cuts` (n_reads entries, e.g. the output of sk_scan_device_async on the same stream).
 * Returns SK_EINVAL for bad arguments, without enqueueing anything. */
int sk_trim_device_async(sk_ctx *ctx, const sk_batch *batch, const sk_cut *cuts, int mode, const sk_trim_output out[3],
                         void *workspace, size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills *counts from the workspace: SK_OK, SK_ESPACE (a produced output did not fit) or
 * SK_EINVAL (an invalid kept cut, counts->bad_read). */
int sk_trim_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_trim_counts *counts);

/*
 * FASTQ text on the device: the whole of a trim, from FASTQ text in device memory to the trimmed FASTQ text, byte-identical
 * to the files of the reference at -a 1.  Every pointer in the structs below is a DEVICE pointer.
 *
 * Lines end at '\n' only; a '\r' belongs to its line (as in the reference: a CRLF quality line is a range error).  A last
 * line without '\n' ends at the end of the text (the CLI's reader drops its last character instead, DESIGN 1: the library
 * trims the records it is handed).  A record is four consecutive lines counted from the start of the text; lines after
 * the last complete record are counted in tail_lines and not trimmed (the CLI drops lines still carried at EOF).
 * Checks per record, in the order of reference src/FQEntry.cpp:53-97, the first failing one is its reason: the name line
 * has at most 1 byte (SK_FQ_ID_SHORT), it does not start with '@' (SK_FQ_ID_NO_AT), the seq line is empty
 * (SK_FQ_SEQ_EMPTY), the qual line is empty (SK_FQ_QUAL_EMPTY), their lengths differ (SK_FQ_LENGTHS); then a qual line
 * longer than SK_MAX_READ_LEN (SK_FQ_TOO_LONG).  The '+' line is not checked and is copied verbatim.  The lowest
 * malformed record in read order makes finish return SK_EFORMAT.
 * Modes (sk_trim_device_async's): SK_TRIM_SE and SK_TRIM_PE_INTERLEAVED read text[0]; SK_TRIM_PE_SPLIT reads mate 1 from
 * text[0] and mate 2 from text[1], which must frame to the same record count (else SK_EFORMAT with SK_FQ_PAIR_COUNT at the
 * first record without a mate: the CLI's "Batch2 and Batch1 have different lengths").  SK_TRIM_PE_INTERLEAVED with an odd
 * record count drops the last record (dropped_unpaired = 1) after checking it, as the CLI does.
 * Read numbers (range.read, record_index): SE and interleaved: the record number; split: record k of text[0] is read 2k,
 * record k of text[1] is read 2k + 1.
 * The scan is sk_scan_device_async with `params` on the qual (and, with trunc_n, seq) lines packed into an `offsets`
 * batch in the workspace, with in->max_read_len as its length hint (0 = unknown); a range error makes finish return
 * SK_ERANGE with counts->range (what the CLI prints).  A format error beats a range error (the reference frames a whole
 * batch before it scans it).  On either error nothing is written to any output.
 * Emission: every kept record as name '\n' seq[five:three] '\n' plus '\n' qual[five:three] '\n' (reference
 * src/trim_single.cpp:393-396), in read order (the -a 1 order), routed by the pair rule of sk_trim_device_async:
 *   SK_TRIM_SE              out[0]: every kept record
 *   SK_TRIM_PE_SPLIT        out[0]: mate 1 of the pairs with both kept, out[1]: their mate 2, out[2]: singles
 *   SK_TRIM_PE_INTERLEAVED  out[0]: both mates of such pairs, out[2]: singles
 *   SK_TRIM_PE_COMBO_ALL    out[0]: both mates of EVERY pair, a mate that is not kept as an N record   (out[1], out[2] unused)
 * SK_TRIM_PE_COMBO_ALL is sickle's documented -M (reference README.md:116-120; the record layout is upstream sickle 1.33's).
 * Its input and framing are SK_TRIM_PE_INTERLEAVED's in every respect: one text (text[1] NULL), pairs are records 2k and
 * 2k + 1, an odd last record is checked and dropped (dropped_unpaired = 1), and the checks and their precedence are the
 * same.  Every read of every framed pair goes to out[0], mate 1 then mate 2, so records 2k and 2k + 1 of the output are
 * always pair k, also when neither mate is kept.  A kept read (three >= 0) is emitted as above.  A read that is not kept is
 * emitted as an N record: its name line verbatim (the whole first line, a comment and a trailing '\r' included), then the
 * six bytes 'N' '\n' '+' '\n' Q '\n'.  The '+' of an N record is bare: the record is synthetic, its own '+' line is not
 * copied.  Q is the byte sk_quality_constants(params->qualtype)[1], the type's lowest quality (phred 4, sanger 33, solexa
 * 58, illumina 64).  out[1] and out[2] are ignored (never written, whatever they hold) and records[1] = records[2] =
 * bytes[1] = bytes[2] = 0.  record_index gets the read number of every record, N records included.  After an error
 * nothing is written, N records neither.  The N records are not counted on their own (sk_fastq_counts is fixed): their
 * number is records[0] less the records[0] + records[2] of a counting SK_TRIM_PE_INTERLEAVED call on the same text.
 * Output size: for the other modes an output never exceeds its text(s) by more than one '\n' each (the one an
 * unterminated last line gains).  An N record is one byte LONGER than the record it stands for when that is a 1-base read
 * with an empty '+' line (name + 7 bytes against name + 6), so out[0] of SK_TRIM_PE_COMBO_ALL can exceed the text:
 *   bytes[0] <= bytes of text + records_in + 1 <= T + floor((T + 1) / 8) + 1
 * (a valid record has 8 bytes or more, 7 if it is the unterminated last one).  Size out[0] by this, or by a counting call.
 * The workspace formula is the same: its emission table has room for every record of the packed batch.
 * An output is produced iff its text is not NULL (16-byte aligned); record_index (8-byte aligned, or NULL) then gets the
 * read number of each record.  An output whose bytes exceed capacity, or whose records exceed record_capacity while
 * record_index is given, gets nothing written; finish then returns SK_ESPACE with the counts.  With every text NULL the
 * call only counts.  Inputs may have any alignment and any size (64-bit offsets); a text of 32 GiB or more is SK_EINVAL
 * (the packed batch would reach 2^32 reads).
 *
 * sk_trim_fastq_device_async only enqueues kernels on hip_stream: no copy, no synchronisation, no allocation beyond the
 * one sk_scan_device_async makes on its own (the regrouping scratch of a context's first big mixed batch).  All scratch
 * lives in `workspace` (device, 16-byte aligned), sized without a look at the text by the most records and qual bytes a
 * valid text of T = bytes[0] + bytes[1] bytes can hold, and by the most lines any text of T bytes can hold (a descriptor
 * slot for every four lines: the ordered calls count lines of malformed texts too).  With H = floor((T + 2) / 16) and
 * G = floor((T + 7) / 8):
 *   sk_trim_fastq_workspace_bytes(T, trunc_n) = 464 + 80 G + 64 H + 16 floor(T / 65536) + 64 ceil((H + 1) / 1024)
 *                                               + (trunc_n ? 2 : 1) * 16 ceil(T / 32)
 * i.e. about 14.5 bytes per text byte (15 with trunc_n).  It holds for any text, malformed ones included.  finish is the
 * only call that waits: it reads the counts out of the workspace and reads and clears the stream's range-error word (a
 * later sk_scan_device_finish on that stream does not report it again).  Two calls in flight need two workspaces.
 * The workspace's contents on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.
 */
enum { SK_FQ_OK = 0, SK_FQ_ID_SHORT = 1, SK_FQ_ID_NO_AT = 2, SK_FQ_SEQ_EMPTY = 3, SK_FQ_QUAL_EMPTY = 4, SK_FQ_LENGTHS = 5,
       SK_FQ_TOO_LONG = 6, SK_FQ_PAIR_COUNT = 7 };

typedef struct {
    const uint8_t *text[2]; /* device, any alignment; text[1] only (and required) for SK_TRIM_PE_SPLIT */
    uint64_t bytes[2];
    uint32_t max_read_len;  /* optional hint, 0 = unknown: the stride (longest-read hint) of the packed batch */
} sk_fastq_input;

typedef struct {
    uint8_t *text;            /* device, 16-byte aligned, or NULL = output not produced */
    uint64_t capacity;        /* bytes */
    uint64_t *record_index;   /* device, 8-byte aligned, or NULL: the read number of each emitted record */
    uint64_t record_capacity;
} sk_fastq_output;

typedef struct {
    uint64_t records_in[2];        /* complete records framed per input */
    uint64_t tail_lines[2];        /* lines after the last complete record: not trimmed, not an error */
    uint64_t dropped_unpaired;     /* SK_TRIM_PE_INTERLEAVED, SK_TRIM_PE_COMBO_ALL with an odd record count: 1 */
    uint64_t records[3], bytes[3]; /* what each output needs, also when not produced or too small (0 after an error) */
    int32_t format_error;          /* SK_FQ_* of the lowest malformed record, SK_FQ_OK if none */
    uint32_t format_input;         /* 0 / 1 */
    uint64_t format_record;        /* 0-based record number within that input */
    sk_err range;                  /* filled on SK_ERANGE; range.read in the read numbering above */
} sk_fastq_counts;

size_t sk_trim_fastq_workspace_bytes(uint64_t text_bytes, int32_t trunc_n);
/* Enqueues the trim of the FASTQ text(s) of *in.  Returns SK_EINVAL for bad arguments, without enqueueing anything. */
int sk_trim_fastq_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in, int mode,
                               const sk_fastq_output out[3], void *workspace, size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills *counts: SK_OK, SK_EFORMAT, SK_ERANGE or SK_ESPACE (in this order of precedence).
 * The range verdict is the stream's error word as it is when this call reads it: with several text calls in flight on one
 * stream, use sk_trim_fastq_piece_device_async and its finish, which takes every verdict from its own workspace. */
int sk_trim_fastq_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts);

/*
 * The same trim with the records in the order the reference writes them at -a T (its default T is the machine's hardware
 * concurrency), so the outputs are byte-identical to its files for any T, not only -a 1.  Everything said above holds
 * (framing, checks, read numbers, the pair rule, the record format, capacities, "nothing is written on an error"), except
 * for what follows.  This comment is the normative text of the rule.
 *
 * Lines and units.  A line ends at '\n'; len(line) does not count it.  m = 4 lines (SK_TRIM_SE, SK_TRIM_PE_SPLIT) or 8
 * (SK_TRIM_PE_INTERLEAVED, SK_TRIM_PE_COMBO_ALL), L = order->batch_len.  The unit of ordering is a read (SE) or a pair (every
 * PE mode).
 * Batches (the reference's reader, src/GZReader.cpp:59-132), per input text, on line numbers.  Start with a = c = 0, then:
 *   1. if c is already the number of lines the input has ended, and the current set is the carried lines [a, c);
 *   2. else e = the smallest line number > c with sum(len(lines[a:e])) >= L; without one e = the number of lines and the
 *      input has ended;
 *   3. the batch is lines [a, e - (e - a) % m);
 *   4. an empty batch ends the run;
 *   5. else a = the batch's end, c = e; go on unless the input has ended.
 * Lines left over at the end are dropped.  SK_TRIM_PE_SPLIT cuts both texts with the same L and stops before the first
 * batch index at which one text has no batch or the two batches differ in their line count (stopped_on_mismatch; the
 * reference's "Batch2 and Batch1 have different lengths", which exits 0 after writing what came before).  With
 * batch_limit != 0 only the first batch_limit batches exist.  Records behind the last batch do not exist for the call:
 * they are not checked, not scanned, so no format or range error comes from them, and not emitted; they are counted in
 * records_unbatched (the odd record of an interleaved text is one of them: dropped_unpaired is 0 in ordered calls, and
 * SK_FQ_PAIR_COUNT never occurs).
 * Order.  Batches go in input order.  Inside a batch of n units, with T = order->threads and k the unit's number in the
 * batch: SE writes the units with k % T == T - 1 first, then residues 0, 1, .., T - 2 (src/trim_single.cpp:263-298); PE
 * writes residues 0, 1, .., T - 1 (src/trim_paired.cpp:388-403,530-567); k ascends inside a residue.  The pair rule routes
 * the kept reads as above; each output is that order filtered by its destination.  record_index gets the read numbers
 * (as above) in emission order.  T = 1 is read order.
 * Lines gzgets would split.  The reference reads with gzgets(file, buf, L), which splits a line of L - 1 bytes or more;
 * that is not reproduced.  If ANY line of an input is that long -- the lines of records behind the last batch and the
 * lines after the last complete record included, so the rare text whose only such line lies behind the point where the
 * reference stops is refused too -- finish returns SK_ELONGLINE with long_line_input = the lowest input that has one
 * and long_line = its lowest such line (0-based); nothing is written, the order counts are filled, records[] and bytes[]
 * are 0.
 * Unterminated last line.  Parity with the reference is claimed for texts that end in '\n'.  A last line without one
 * ends at the end of the text, as above (the reference's reader drops its last character).
 *
 * The workspace: sk_trim_fastq_ordered_workspace_bytes(text_bytes, trunc_n, batch_capacity), with text_bytes = bytes[0] +
 * bytes[1], is sk_trim_fastq_workspace_bytes(text_bytes, trunc_n) + 8 (batch_capacity + 1) rounded up to 16.  Its contents
 * on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.  The number
 * of batches depends on the text: a batch usually holds about batch_len bytes, fewer when long carried lines use the
 * budget up.  A caller starts at, say, batch_capacity = text_bytes / batch_len + 16 and calls again with a larger table
 * when it was too small: finish then returns SK_ESPACE with batches = batch_capacity + 1 ("more than") and nothing
 * written.  max(bytes[0], bytes[1]) / 4 + 2 always suffices (a batch holds four lines at least).  The walk stops at a full
 * table, so the one serial loop of the call is bounded by batch_capacity + 1 steps of about 32 dependent loads per input.
 * Same discipline as sk_trim_fastq_device_async: only kernels are enqueued, all state lives in the workspace, finish is
 * the only call that waits, nothing is written on any error, and sk_trim_fastq_output_words works on this workspace.
 * finish returns, in this order of precedence: SK_ELONGLINE, SK_ESPACE for the batch table, SK_EFORMAT, SK_ERANGE,
 * SK_ESPACE for the outputs, SK_OK.  Bad arguments (those of sk_trim_fastq_device_async; order NULL, threads 0, reserved
 * != 0, batch_len < 20, batch_capacity 0 or beyond 2^40) return SK_EINVAL and enqueue nothing.
 */
enum { SK_ELONGLINE = -8 }; /* sk_trim_fastq_ordered_device_finish: a line of batch_len - 1 bytes or more (counts say where) */

typedef struct {
    uint32_t threads;        /* -a T, >= 1 */
    uint32_t reserved;       /* 0 */
    uint64_t batch_len;      /* GZReader's byte budget, >= 20 (the caller computes it from the file size) */
    uint64_t batch_capacity; /* entries of the batch table in the workspace, >= 1 */
    uint64_t batch_limit;    /* 0 = none; else only the first batch_limit batches exist for the call */
} sk_fastq_order;

typedef struct {
    uint64_t batches;             /* batches trimmed (after the PE stop and batch_limit) */
    uint64_t units;               /* reads (SE) or pairs in them */
    uint64_t last_batch_units;    /* what the PE summary's "Total input FastQ records" is made from */
    uint64_t records_unbatched[2];/* complete records of each input behind the last batch */
    uint32_t stopped_on_mismatch; /* PE split: the two inputs' batches differed in line count */
    uint32_t long_line_input;     /* with SK_ELONGLINE: which input, and */
    uint64_t long_line;           /*   its lowest line of batch_len - 1 bytes or more */
    uint64_t error_batch;         /* batch of the record behind SK_EFORMAT / SK_ERANGE, else UINT64_MAX */
} sk_fastq_order_counts;

size_t sk_trim_fastq_ordered_workspace_bytes(uint64_t text_bytes, int32_t trunc_n, uint64_t batch_capacity); /* pure */
int sk_trim_fastq_ordered_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in, int mode,
                                       const sk_fastq_order *order, const sk_fastq_output out[3], void *workspace,
                                       size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills both counts (order_counts may be NULL). */
int sk_trim_fastq_ordered_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts,
                                        sk_fastq_order_counts *order_counts);
/* *first_unit_dev = the device table of the call that used `workspace`: batches + 1 entries, batch b holds units
 * [t[b], t[b + 1]), valid once the call's kernels have run.  No device access, no wait. */
int sk_trim_fastq_ordered_batches(void *workspace, const uint64_t **first_unit_dev);

/* Measurement aid (bench.py's second roofline denominator): streams `bytes` of device memory at
 * dev_buf through a read-only kernel (16-byte nt loads, nothing written) `launches` times on
 * hip_stream and returns the average rate in GB/s, timed with HIP events on that stream. */
int sk_probe_read_bandwidth(sk_ctx *ctx, const void *dev_buf, size_t bytes, int launches, void *hip_stream,
                            double *gb_per_s);

/* ---- BGZF block deflate for the -g writer (no counterpart in the reference, whose -g hands the
 * records to gzprintf, src/trim_single.cpp:418).  text: n_blocks blocks at a stride of 65280 bytes,
 * block b holding sizes[b] (<= 65280) bytes (the buffer may end with the last block's bytes); out: n_blocks slots of 65536 bytes; out_sizes[b] = the
 * length of block b's deflate stream in its slot, or 0 when the block does not compress into the
 * slot (the caller then writes it as a stored block).  The caller frames each stream as a gzip
 * member with the BGZF size field, CRC-32 and ISIZE.  Host pointers (pinned ones from
 * sk_bgzf_host_alloc are copied fastest); synchronous; callable from several threads. */
int sk_bgzf_deflate(int device, const uint8_t *text, const uint32_t *sizes, uint32_t n_blocks, uint8_t *out, uint32_t *out_sizes);
void *sk_bgzf_host_alloc(size_t bytes);
void sk_bgzf_host_free(void *p);
const char *sk_bgzf_last_error(void);

/*
 * BGZF on the device: text in device memory -> a complete BGZF byte image in device memory, a valid .gz file as it
 * stands.  Stream-ordered, so it chains behind sk_trim_fastq_device_async without a host wait in between.
 *
 * Blocks: block b is text bytes [65280 b, min(65280 (b + 1), n)), n the text's actual length: in->bytes, or *in->bytes_dev
 * (read on the stream, must be <= in->bytes; a larger value is taken as in->bytes) when that is given; with valid_dev given
 * and *valid_dev == 0 the text counts as empty.  The launches are sized by in->bytes; blocks past n produce nothing, and
 * n == 0 gives no data block.
 * Each data block becomes one gzip member: the 18-byte BGZF header (1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00, then
 * BSIZE = member size - 1, 16 bit LE), the body, then CRC-32 and ISIZE of the block's text (LE).  The body is the deflate
 * stream sk_bgzf_deflate writes for that block, or a stored block (01 LEN NLEN + text) iff that stream does not fit its
 * 64 KiB slot or has text + 5 bytes or more: the rule of the CLI's -g writer.  Members lie back to back from out[0]; with
 * SK_BGZF_EOF the standard 28-byte empty member (1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00
 * 00 00 00) follows.
 * `out` is 16-byte aligned.  If the image exceeds `capacity`, NOTHING is written to out and finish returns SK_ESPACE with
 * bytes_out = the need.  sk_bgzf_bound(bytes, flags) = bytes + 31 ceil(bytes / 65280) + (SK_BGZF_EOF ? 28 : 0) always
 * suffices (a stored member is its text + 5 + 26 bytes).
 *
 * The workspace's contents on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.
 * sk_bgzf_device_async only enqueues three kernels on hip_stream: no allocation, no copy, no synchronisation, no lock.  All
 * scratch and the counts live in `workspace` (device, 16-byte aligned).  With NB = ceil(text_bytes / 65280):
 *   sk_bgzf_workspace_bytes(text_bytes) = 128 + 16 NB + 261152 min(NB, 1280) + 65536 NB
 * (header; table; one token per text byte for each of at most 1280 blocks in flight -- a fixed grid, not the device's CU
 * count, so the size needs no device; a 64 KiB deflate slot per block), i.e. about the text's size plus at most 334 MB.
 * sk_bgzf_device_finish is the only call that waits.  Two calls in flight need two workspaces.  Bad arguments (NULL ctx or
 * in, unknown flags, text NULL with bytes != 0, out NULL with capacity != 0, out or workspace not 16-byte aligned, bytes_dev
 * or valid_dev not 8-byte aligned, a short workspace) return SK_EINVAL and enqueue nothing.
 *
 * SK_BGZF_SEARCH: a data block's body is the deflate stream of the SEARCHING encoder instead: next to the copies from the
 * line four lines up and the runs it takes matches of 5 bytes or more that a hash table over the block finds (4-byte
 * hashes, 2048 buckets of 4 ways, at most 32 768 back, never across a line's end), so the image of real reads is smaller
 * and the call slower.  The image is a function of the text alone, as without the flag.  Everything else above holds as
 * it stands: the stored-block rule, the framing, CRC-32 and ISIZE, sk_bgzf_bound, the counts, bytes_dev / valid_dev, the
 * SK_ESPACE rule.  The workspace is larger by one candidate word per text byte of each block in flight:
 *   sk_bgzf_workspace_bytes_flags(text_bytes, flags) = sk_bgzf_workspace_bytes(text_bytes)
 *                                                      + (flags & SK_BGZF_SEARCH ? 261152 min(NB, 1280) : 0)
 * and a workspace shorter than that, passed with the flag, is SK_EINVAL.  A workspace may serve calls with and without
 * the flag in turn.
 */
enum {
    SK_BGZF_EOF = 1,   /* flags: close the image with the 28-byte empty end-of-file member */
    SK_BGZF_SEARCH = 2 /* encode the data blocks with the match search */
};

typedef struct {
    const uint8_t *text;       /* device, ANY alignment */
    uint64_t bytes;            /* the text's length, or an upper bound on it when bytes_dev is given */
    const uint64_t *bytes_dev; /* device, 8-byte aligned, or NULL: the length, read on the stream; must be <= bytes */
    const uint64_t *valid_dev; /* device, 8-byte aligned, or NULL: if given and *valid_dev == 0 the text counts as empty */
} sk_bgzf_input;

typedef struct {
    uint64_t bytes_in, blocks, stored_blocks; /* data blocks; the EOF member is not counted */
    uint64_t bytes_out;                       /* what the image needs, also when it did not fit */
} sk_bgzf_counts;

uint64_t sk_bgzf_bound(uint64_t text_bytes, int flags); /* worst-case image size; pure, no device */
size_t sk_bgzf_workspace_bytes(uint64_t text_bytes);    /* pure, no device */
size_t sk_bgzf_workspace_bytes_flags(uint64_t text_bytes, int flags); /* pure, no device; what a call with `flags` needs */
int sk_bgzf_device_async(sk_ctx *ctx, const sk_bgzf_input *in, uint8_t *out, uint64_t capacity, int flags, void *workspace,
                         size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills *counts from the workspace: SK_OK, or SK_ESPACE (the image is beyond the capacity). */
int sk_bgzf_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_bgzf_counts *counts);

/*
 * The device words of output `output` (0..2) inside the workspace of a sk_trim_fastq_device_async call, as its kernels write
 * them on the stream: *bytes_dev = the output's byte count, *written_dev = 1 iff the output's text is in its buffer
 * (produced, no format or range error, within its capacities), else 0.  Fed to sk_bgzf_input.bytes_dev / valid_dev (with
 * bytes = the output buffer's capacity) they chain the two calls without a host wait; after an upstream error or an output
 * that did not fit, the image is empty (the EOF member only): whatever the buffer held is never compressed.
 * One-pass sizing: a trimmed text holds, per kept record, its name and '+' lines as they were and its seq and qual lines cut
 * shorter or not at all (sk_fastq.hip's emission: name + 1, plus-line + 1, 2 * (three - five + 1) bytes), so it never
 * exceeds its inputs by more than the one '\n' synthesized after an unterminated last line of each input text: an output
 * buffer of bytes[0] + bytes[1] + 2 bytes always fits.
 */
int sk_trim_fastq_output_words(void *fastq_workspace, int output, const uint64_t **bytes_dev, const uint64_t **written_dev);

/*
 * BGZF read on the device: a BGZF byte image in device memory -> the concatenated text of its members in device memory,
 * with every member's CRC-32 and ISIZE checked.  The inverse of sk_bgzf_device_async, and it reads what bgzip and htslib
 * write.  Plain (non-BGZF) gzip is NOT decoded: it is reported as SK_GZ_HEADER at member 0, and the caller goes on to
 * sk_gzip_inflate_device_async (below), which reads any gzip.
 *
 * Framing.  Members lie back to back from image[0].  A member begins 1f 8b 08, FLG exactly 04, six bytes that are not
 * looked at (MTIME, XFL, OS), XLEN; the extra field is walked subfield by subfield (SI1 SI2 SLEN data) for the first
 * 'B' 'C' 02 00 BSIZE, which need not come first.  The member is BSIZE + 1 bytes, its body lies between the extra field and
 * the 8-byte trailer (CRC-32, ISIZE).  Where a member must begin, in this order: bytes that are not 1f 8b 08 04 (as many
 * of the four as the image still holds) are SK_GZ_HEADER, so trailing garbage is; fewer than 26 bytes left (12 + the
 * 6-byte subfield + an empty body + 8: the shortest member), or an extra field that ends beyond the image, is
 * SK_GZ_TRUNCATED; a subfield that overruns XLEN, no BC subfield, or BSIZE + 1 < 12 + XLEN + 8 is SK_GZ_HEADER; a member that
 * ends beyond the image is SK_GZ_TRUNCATED.  Framing stops there: `members` counts those framed before it, and the error
 * is that of member `members`.  ISIZE above 65 536 is SK_GZ_LENGTH (the member is framed, not decoded, and adds nothing to
 * bytes_out).  An empty image is valid: 0 members.
 *
 * Decoding.  All of RFC 1951: stored, fixed and dynamic blocks, any number per member, empty ones included.  SK_GZ_DEFLATE:
 * block type 3; stored LEN != ~NLEN; HLIT > 29 or HDIST > 29; an over-subscribed code; an incomplete code, except (as in
 * zlib) one whose longest code has one bit; no end-of-block code; a repeat with nothing before it or past HLIT + HDIST; a
 * bit pattern without a symbol; length symbols 286 / 287, distance symbols 30 / 31; a distance reaching before the member's
 * first byte; bits or stored bytes beyond the body.  Body bytes behind the final block are ignored.  Text beyond ISIZE is
 * SK_GZ_LENGTH at the token that would cross it, text short of ISIZE at the end of the stream; then the CRC-32 of the text
 * against the trailer, SK_GZ_CRC.  The first check to fail is the member's reason; across members the lowest index wins.
 *
 * out == NULL with capacity == 0 only counts (framing and sums, no decode, so only framing errors and ISIZE > 65 536 are
 * seen): this is how a caller sizes `out`.  If bytes_out > capacity NOTHING is written to out, nothing is decoded, and
 * finish returns SK_ESPACE with bytes_out = the need.  finish returns, in this order of precedence, SK_EDATA (counts say
 * where and why), SK_ESPACE, SK_OK.  After SK_EDATA out[0, min(bytes_out, capacity)) is undefined; no byte at or beyond
 * capacity is ever written, and a member writes inside its own ISIZE span only.  A corrupt image is never read outside
 * [image, image + image_bytes).  `image` has any alignment, `out` and `workspace` are 16-byte aligned.
 * The workspace's contents on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.
 *
 * sk_bgzf_inflate_device_async only enqueues kernels on hip_stream (with R = ceil(log2(floor(n / 26) + 1)): 6 + R when
 * counting, 8 + R otherwise, the last one a single lane that writes the word of sk_bgzf_inflate_output_words): no allocation,
 * no copy, no synchronisation.  All scratch and the counts live in `workspace`.  With n = image_bytes and
 * A(x) = 16 ceil(x / 16):
 *   sk_bgzf_inflate_workspace_bytes(n) = 128 + A(4 (floor(n / 4096) + 1)) + A(8 C) + 3 A(4 C) + A(40 (floor(n / 26) + 1)),
 *                                        C = floor(n / 4) + 1
 * (header; a count per 4096 positions; position, two successor words and a rank for each of the at most n / 4
 * non-overlapping matches of 1f 8b 08 04; a table entry per member), about 6.6 bytes per image byte.  It holds for any image,
 * adversarial ones included, and needs no device: the grids are constants.  An image above 8 GiB is SK_EINVAL.
 * sk_bgzf_inflate_device_finish is the only call that waits.  Two calls in flight need two workspaces.  Bad arguments (NULL
 * ctx, image NULL with bytes != 0, out NULL with capacity != 0, out or workspace not 16-byte aligned, a short workspace, an
 * image above 8 GiB) return SK_EINVAL and enqueue nothing.
 */
enum { SK_EDATA = -7 }; /* sk_bgzf_inflate_device_finish: the image is not valid BGZF (counts say where and why) */
enum { SK_GZ_OK = 0, SK_GZ_HEADER = 1, SK_GZ_TRUNCATED = 2, SK_GZ_DEFLATE = 3, SK_GZ_LENGTH = 4, SK_GZ_CRC = 5 };

typedef struct {
    uint64_t bytes_in, members;  /* members framed, empty ones (the EOF marker) included */
    uint64_t bytes_out;          /* sum of ISIZE: what `out` needs, also when it did not fit or was NULL */
    int32_t  error;              /* SK_GZ_* of the LOWEST bad member, SK_GZ_OK if none */
    uint32_t reserved;
    uint64_t error_member, error_offset; /* its index, and its byte offset in the image */
} sk_bgzf_inflate_counts;

size_t sk_bgzf_inflate_workspace_bytes(uint64_t image_bytes);   /* pure, no device */
int sk_bgzf_inflate_device_async(sk_ctx *ctx, const uint8_t *image, uint64_t image_bytes, uint8_t *out, uint64_t capacity,
                                 void *workspace, size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills *counts from the workspace: SK_EDATA, SK_ESPACE or SK_OK (in this order of precedence). */
int sk_bgzf_inflate_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_bgzf_inflate_counts *counts);

/*
 * Plain gzip read on the device: any gzip byte image in device memory (what gzip, pigz and zlib write: one long member or a
 * few, no BC subfield) -> the concatenated text of its members in device memory, every member's CRC-32 and ISIZE checked.
 * One deflate stream is decoded in parallel: the image is cut into chunks, a block start is guessed per chunk, every
 * guessed start is decoded as a STRETCH until it arrives exactly on a later guess, and the chain of stretches from the
 * first block is what counts; matches into the unknown 32 KiB before a stretch are filled in afterwards.  No result rests
 * on a guess.  A BGZF image is valid input here, only slow: parallelism comes from non-final dynamic block headers, and
 * an image of stored or fixed blocks alone, or of many one-block members, is decoded by few wavefronts
 * (`stretches_used` tells).
 *
 * Format.  RFC 1952 members lie back to back from image[0].  Where a member must begin, in this order: bytes that are not
 * 1f 8b 08 (as many of the three as the image still holds) are SK_GZ_HEADER, so trailing bytes are; fewer than 10 bytes
 * left is SK_GZ_TRUNCATED; a reserved FLG bit (0xe0) is SK_GZ_HEADER; FEXTRA, FNAME, FCOMMENT and FHCRC are stepped over
 * (the header CRC is not checked), and one that runs past the image is SK_GZ_TRUNCATED.  The deflate stream follows:
 * all of RFC 1951 with the SK_GZ_DEFLATE list of the BGZF reader; bits that run out are SK_GZ_DEFLATE too.  A distance
 * reaching before its member's first byte is SK_GZ_DEFLATE.  The final block ends on a byte boundary with the 8-byte
 * trailer; fewer than 8 bytes left is SK_GZ_TRUNCATED.  A text length that differs from ISIZE mod 2^32 is SK_GZ_LENGTH;
 * then the CRC-32: SK_GZ_CRC.  Within a member the reasons come in the order of their numbers, across members the lowest
 * index wins.  error_offset is the member's first byte for header, truncation, length and CRC errors and the byte that
 * holds the first bit of the failing block for SK_GZ_DEFLATE (image_bytes when the stream ends where a block must begin).
 * A header, truncation or Huffman-level error stops the chain: `members` and `bytes_out` are then those up to it.  An empty
 * image is valid: 0 members.
 *
 * out == NULL with capacity == 0 only counts: the lengths alone are decoded, so header, truncation and Huffman-level
 * errors are seen, distance, length and CRC errors are not.  This is how a caller sizes `out`.  If bytes_out > capacity
 * NOTHING is written to out and finish returns SK_ESPACE with bytes_out = the need.  finish returns, in this order of
 * precedence, SK_EDATA, SK_ESPACE, SK_OK.  After SK_EDATA out[0, min(bytes_out, capacity)) is undefined.  No byte at or
 * beyond capacity is ever written, none outside [image, image + image_bytes) is ever read.  `image` has any alignment,
 * `out` and `workspace` are 16-byte aligned.
 * The workspace's contents on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.
 *
 * sk_gzip_inflate_device_async only enqueues kernels on hip_stream (3 when counting, 9 otherwise): no allocation, no copy,
 * no synchronisation.  All scratch and the counts live in `workspace`.  With n = image_bytes, A(x) = 16 ceil(x / 16),
 * chunk = 32768 doubled until 4096 chunks hold n, and S = ceil(n / chunk):
 *   sk_gzip_inflate_workspace_bytes(n, capacity) = 256 + 128 (S + 1) + A(8 (S + 1)) + A(4 (S + 1))
 *                                                  + 32 (floor(n / 18) + 1) + A(2 capacity)
 * (header; a record per stretch; the chain; an entry per member, whose trailers lie 18 bytes apart at least; the text as
 * 16-bit symbols).  It needs no device.  The environment variable SK_GZIP_CHUNK, a power of two of 256 or more, replaces
 * `chunk` in both calls (read at call time; anything else is ignored); it exists for tests.  Bad arguments (NULL ctx,
 * image NULL with bytes != 0, out NULL with capacity != 0, out or workspace not 16-byte aligned, a short workspace, an
 * image above 8 GiB) return SK_EINVAL and enqueue nothing.  Two calls in flight need two workspaces.
 */
typedef struct {
    uint64_t bytes_in, members;       /* members completed (trailer reached) */
    uint64_t bytes_out;               /* text bytes of the chain: what `out` needs */
    uint64_t stretches, stretches_used; /* chunks the image was cut into; those the chain from bit 0 went through */
    int32_t  error;                   /* SK_GZ_* of the lowest failure on the chain, SK_GZ_OK if none */
    uint32_t reserved;
    uint64_t error_member, error_offset;
} sk_gzip_inflate_counts;

size_t sk_gzip_inflate_workspace_bytes(uint64_t image_bytes, uint64_t capacity);   /* pure, no device */
int sk_gzip_inflate_device_async(sk_ctx *ctx, const uint8_t *image, uint64_t image_bytes, uint8_t *out, uint64_t capacity,
                                 void *workspace, size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills *counts from the workspace: SK_EDATA, SK_ESPACE or SK_OK (in this order of precedence). */
int sk_gzip_inflate_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_gzip_inflate_counts *counts);

/*
 * The device words of a reader's call inside its workspace, as its kernels write them on the stream: *bytes_dev = the
 * call's bytes_out (what the text needs, also when it did not fit), *written_dev = 1 iff the text is in `out`: the call
 * decoded (out != NULL), ended without an error, and its text fitted the capacity; else 0, so a count-only call gives 0.
 * The written word is the last thing a call writes: behind the last kernel that can still lower the error.  Like
 * sk_trim_fastq_output_words: no device access, no wait; SK_EINVAL for a NULL argument.  Fed to sk_fastq_lengths (below)
 * with sk_fastq_input.bytes = the capacity of `out`, they chain a reader and the trim without a host wait in between.
 */
int sk_bgzf_inflate_output_words(void *workspace, const uint64_t **bytes_dev, const uint64_t **written_dev);
int sk_gzip_inflate_output_words(void *workspace, const uint64_t **bytes_dev, const uint64_t **written_dev);

/*
 * Plain gzip read on the device in PIECES: sk_gzip_inflate_device_async resumed at a block boundary, for streams whose
 * text is beyond one call's workspace.  A deflate stream can be taken up again at any block boundary, given the bit
 * position, the 32 KiB of text before it, and the running CRC-32 and length of the member in progress.  That is the
 * STATE, in device memory; a piece call starts at *state_in and publishes *state_out, so pieces chain on a stream
 * without a host wait.  A state of all zeros is the start of a stream.  These calls stand beside the whole-image calls,
 * which are unchanged.
 *
 * Window.  With p = state_in->pos_bit >> 3 the piece's WINDOW is the stream bytes [p, min(p + window_bytes, image_offset +
 * image_bytes)); image[0] is stream byte image_offset.  No image byte outside the window bears on anything, and none
 * outside [image, image + image_bytes) is read.  The piece is CLOSING iff last != 0 and the window reaches the image's
 * end.  From in_member == 0 the piece parses a member header at p (a closing piece whose window is empty ends the stream
 * there); from in_member == 1 it takes a block header at pos_bit.
 *
 * Resume points are every block boundary inside a member (also the one behind a header, with member_text 0) and every
 * member start behind a complete trailer.  A closing piece is sk_gzip_inflate_device_async on the rest of the stream:
 * every failure is real, and on success done = 1.  A piece that is not closing ends in front of the first header, block
 * or trailer that does not parse or decode inside the window, whether bits ran out or the image is damaged; R is the
 * last resume point it reached.  R > pos: the piece succeeds with the text up to R, and nothing behind R is decoded or
 * reported.  R == pos: the failure is reported as what it appears to be, with window_limited = 1; state_in is never
 * written, so the caller may repeat the piece from it with a larger window.  A distance reaching before its member's first
 * byte, SK_GZ_LENGTH and SK_GZ_CRC in the consumed part are always real.
 *
 * Capacity.  The piece also ends in front of the first stretch (sk_gzip_inflate_device_async) whose text would pass
 * `capacity`; a stretch begins at a block boundary, a resume point.  If even the first stretch does not fit, the state's
 * status is 2, finish returns SK_ESPACE with bytes_out = that stretch's need, and nothing is written to out.
 *
 * state_in->status != 0: the piece is void: it writes no text (the written word is 0), *state_out inherits the failure,
 * and finish returns it with inherited = 1.  state_in->done: an empty successful piece.  A position outside the image
 * handed in gives status 3 and SK_EINVAL from finish.  Member numbers and byte offsets in a state and in what finish
 * reports are stream-wide; counts->members, bytes_in (the window) and bytes_out are the piece's own.  finish returns, in
 * this order of precedence, SK_EDATA, SK_ESPACE, SK_OK.  Unlike the whole-image call, the FIRST failing piece reports: a
 * lower-numbered reason for the same member that a later piece would have found (a cut trailer behind a distance that
 * reaches too far) no longer wins.
 *
 * sk_gzip_inflate_output_words works on a piece's workspace: the piece's text length and its written word, which feed
 * sk_fastq_carry_device_async as the BGZF reader's do.
 *
 * The workspace's contents on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.
 * sk_gzip_inflate_piece_device_async only enqueues kernels (10) on hip_stream: no allocation, no copy, no wait.  Two pieces
 * in flight need two workspaces and alternate two states.  With w = window_bytes, chunk and S taken on w as
 * sk_gzip_inflate_workspace_bytes takes them on n (SK_GZIP_CHUNK applies likewise):
 *   sk_gzip_inflate_piece_workspace_bytes(w, capacity) = 256 + 128 (S + 1) + A(8 (S + 1)) + A(4 (S + 1))
 *                                                        + 32 (floor(w / 18) + 2) + 32 (S + 1) + A(2 (32768 + capacity))
 * SK_EINVAL, nothing enqueued: NULL ctx, piece or states; image NULL with image_bytes != 0; state_out == state_in; states
 * not 16-byte aligned; piece->reserved != 0; window_bytes 0 or above 8 GiB; out NULL or not 16-byte aligned; a capacity
 * above 2^60; a workspace that is NULL, not 16-byte aligned or short.
 */
#define SK_GZIP_PIECE_STATE_BYTES (128 + 32768)
typedef struct {            /* device memory, 16-byte aligned */
    uint64_t pos_bit;       /* stream bit of the resume point (bit 0 = first bit of stream byte 0) */
    uint64_t in_member;     /* 0: a member begins at byte pos_bit / 8 (or the stream ends there); 1: a block header begins at pos_bit */
    uint64_t member_text;   /* text bytes of the member in progress so far */
    uint64_t member_crc;    /* zlib's crc32 of that text */
    uint64_t members, text_bytes;  /* completed members / text produced, stream-wide */
    uint64_t status;        /* 0, or sticky: 1 data error, 2 text beyond capacity, 3 pos outside the image handed in */
    uint64_t error, error_member, error_offset;  /* SK_GZ_*, stream-wide member number and byte offset */
    uint64_t done;          /* the stream has ended cleanly */
    uint64_t reserved[5];   /* the reader's own (reserved[0]: first byte of the member in progress); zero at a stream's start */
    uint8_t  history[32768];/* the last 32 KiB of stream text, zeros in front of the stream's start */
} sk_gzip_piece_state;
typedef struct {
    uint64_t image_offset;   /* stream offset of image[0] */
    uint64_t window_bytes;   /* > 0 */
    uint32_t last;           /* image's end is the stream's end */
    uint32_t reserved;
} sk_gzip_piece;
typedef struct {
    uint64_t pos_bit, in_member;   /* the state the piece published */
    uint64_t image_bytes_consumed; /* image bytes in front of the byte that holds pos_bit: pos_bit / 8 - image_offset */
    uint32_t window_limited;       /* SK_EDATA from a piece that is not closing, at its first header, block or trailer */
    uint32_t inherited;            /* the failure is state_in's: the piece was void */
    uint32_t done, reserved;
} sk_gzip_piece_counts;

size_t sk_gzip_inflate_piece_workspace_bytes(uint64_t window_bytes, uint64_t capacity);   /* pure, no device */
int sk_gzip_inflate_piece_device_async(sk_ctx *ctx, const uint8_t *image, uint64_t image_bytes, const sk_gzip_piece *piece,
                                       const sk_gzip_piece_state *state_in, sk_gzip_piece_state *state_out, uint8_t *out,
                                       uint64_t capacity, void *workspace, size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills *counts and *piece_counts from the workspace. */
int sk_gzip_inflate_piece_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_gzip_inflate_counts *counts,
                                        sk_gzip_piece_counts *piece_counts);

/*
 * The FASTQ trim with the texts' lengths taken from the device: sk_trim_fastq_device_async (order == NULL, a workspace of
 * sk_trim_fastq_workspace_bytes, finished by sk_trim_fastq_device_finish) or sk_trim_fastq_ordered_device_async (order !=
 * NULL, sk_trim_fastq_ordered_workspace_bytes, sk_trim_fastq_ordered_device_finish), and everything said there holds, with
 * in->bytes[i] an upper bound on text i's length instead of the length.
 * The length n_i of text i is in->bytes[i], or *lengths->bytes_dev[i] (read on the stream, must be <= in->bytes[i]; a
 * larger value is taken as in->bytes[i]) when that is given; with valid_dev[i] given and *valid_dev[i] == 0 the text counts
 * as empty.  The workspace, the launches and every per-read step are sized by in->bytes (a tight bound is a fast call);
 * chunks past n_i count no line and load nothing.  No 16-byte block of text[i] without a byte of [0, n_i) is loaded, and
 * no byte at or beyond n_i bears on anything: the buffer behind n_i may be uninitialised.  It must be READABLE, though, as
 * for the call without `lengths`: text[i] up to the end of the aligned 16-byte block that holds byte n_i - 1, so at most 15
 * bytes beyond in->bytes[i].  A last line without '\n' ends at n_i.  Every count, verdict and output is what the call without `lengths` gives on the text text[i][0, n_i).
 * lengths == NULL, or all four pointers NULL, is that call bit for bit.  Words that are not 8-byte aligned, or a word for
 * text[1] outside SK_TRIM_PE_SPLIT, are SK_EINVAL and enqueue nothing (as are the bad arguments of the two calls above).
 * Same discipline: only kernels are enqueued (the same ones, no more), finish is the only call that waits, and
 * sk_trim_fastq_output_words works on this workspace: reader -> trim -> BGZF writer chain on one stream with one wait.
 */
typedef struct {
    const uint64_t *bytes_dev[2]; /* device, 8-byte aligned, or NULL: text i's length, read on the stream; must be <= bytes[i] */
    const uint64_t *valid_dev[2]; /* device, 8-byte aligned, or NULL: if given and *valid_dev[i] == 0 text i counts as empty */
} sk_fastq_lengths;

int sk_trim_fastq_chained_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in,
                                       const sk_fastq_lengths *lengths, int mode, const sk_fastq_order *order,
                                       const sk_fastq_output out[3], void *workspace, size_t workspace_bytes,
                                       void *hip_stream);

/*
 * The device-resident scan with the read count taken from the device: sk_scan_device_async, and everything said there
 * holds, with batch->n_reads an upper bound B on the read count instead of the count.
 * The scan covers n = min(*n_reads_dev, B) reads; the word is read on the stream (it may be written by work the caller
 * enqueued there earlier; a value above B is taken as B).  out[r] is written for r < n and not touched for r >= n.
 * offsets[i] is read for i <= n only, and no byte of qual or seq at or beyond offsets[n] bears on a result: the entries
 * and bytes behind them may be uninitialised.  Range errors come from reads below n only.  n == 0 scans nothing.
 * The grids, the regrouping of a big mixed batch (whether it runs, and its scratch), the LDS buffers and what
 * batch->stride hints at are sized by B on the host: the launches are those of sk_scan_device_async on a batch of B
 * reads, so a tight bound is a fast call; windows, tiles, teams and spans at or beyond n return without a load, and the
 * regrouping's verdict (a batch of one length is not regrouped) is taken over the n reads -- empty reads behind them do
 * not make it a mixed batch.
 * Only `offsets` batches: offsets != NULL, tiles == NULL, lengths == NULL; a word with any other layout, or a word that
 * is not 8-byte aligned, is SK_EINVAL and enqueues nothing.  n_reads_dev == NULL is sk_scan_device_async bit for bit: the
 * same launches, nothing more loaded.  Finished by sk_scan_device_finish, which is unchanged.
 */
int sk_scan_counted_device_async(sk_ctx *ctx, const sk_params *params, const sk_batch *batch,
                                 const uint64_t *n_reads_dev, sk_cut *out, void *hip_stream);

/*
 * The FASTQ trim in pieces: a text longer than one call's workspace allows is trimmed as a sequence of calls, each on a
 * PIECE of the stream, and what a piece does not consume (the CARRY: an incomplete record, an unpaired one) becomes the
 * front of the next piece's text -- without the host learning anything in between: the window's start, the lengths and the
 * carry are device words, and a finish is the only call that waits.  This call writes read order; the -a T order in
 * pieces is sk_trim_fastq_ordered_piece_device_async (below).  This comment is the normative text.
 *
 * sk_trim_fastq_piece_device_async is sk_trim_fastq_chained_device_async(.., order = NULL, ..), and everything said there
 * holds (the workspace is sk_trim_fastq_workspace_bytes(bytes[0] + bytes[1], trunc_n), its contents on entry are arbitrary
 * and nothing outside it is written, everything sized on the host is a function of in->bytes), with what follows.  piece == NULL is that call bit for bit: the same launches, nothing more
 * loaded, finished by sk_trim_fastq_device_finish.  A call with a piece is finished by sk_trim_fastq_piece_device_finish.
 * Window.  n_i is text i's length as the chained call defines it (in->bytes, bytes_dev, valid_dev).  s_i = min(*start_dev[i],
 * n_i), or 0 for a NULL word.  Text i of the call is text[i][s_i, n_i): the first line starts at s_i, no 16-byte block
 * without a byte of the window is loaded, and no byte outside it bears on anything.  Offsets the call reports (consumed,
 * end) count from text[i].  A start at or beyond n_i is an empty text.
 * more == 0 (the stream's last piece).  Every count, verdict and output is what sk_trim_fastq_device_async gives on the
 * texts text[i][s_i, n_i): the closed unterminated last line, SK_FQ_PAIR_COUNT and dropped_unpaired included.
 * consumed = n_i.
 * more != 0.  A line exists only if its '\n' lies in the window; the bytes behind the last '\n' are no line and are not
 * closed.  With r_i = lines_i / 4 the piece takes u records from each input: SK_TRIM_SE u = r_0; SK_TRIM_PE_INTERLEAVED
 * and SK_TRIM_PE_COMBO_ALL u = r_0 & ~1; SK_TRIM_PE_SPLIT u = min(r_0, r_1).  Records [0, u) of each input are checked, packed, scanned, routed and
 * emitted exactly as sk_trim_fastq_device_async does on a text made of those records alone (read numbers count from the
 * piece's first record).  Everything behind them is the carry: not checked, not scanned, no format or range error comes
 * from it; SK_FQ_PAIR_COUNT never occurs and dropped_unpaired is 0.  records_in[i] = u; tail_lines[i] = the complete lines
 * carried, lines_i - 4u, which may exceed 3.  consumed_i = s_i when u == 0, else one past the '\n' of line 4u - 1.  A text
 * with more records than the packed batch has reads, (b + 1) / 8, ends in SK_EFORMAT, as in the whole-text call (a
 * malformed record lies among the consumed ones).
 * The stream's range-error word.  The frame scan captures the word as it is when the piece begins.  If it is set -- an
 * earlier call on the stream met a range error that no finish has cleared yet -- the piece is void: it takes no record
 * (u = 0, nothing checked, scanned or emitted, so the earlier error stays as it is), ok = 0, and its finish returns
 * SK_ERANGE with counts->range = that earlier error (its read number is the earlier call's) and inherited_range = 1.
 * Words on the stream.  sk_trim_fastq_piece_words(workspace, input, ..) gives the device addresses, inside the workspace's
 * header, of the words the call's kernels write (no device access, no wait; SK_EINVAL for a NULL argument or an input
 * other than 0 / 1): *consumed_dev and *end_dev (= n_i) of that input, and *ok_dev, one word per call, the same through
 * either input: 1 iff there is no format error, the range-error word was clear when the piece began and as its emission
 * saw it, and every produced output fitted.  They are written by the emission's scan kernel, which takes those verdicts.
 * sk_trim_fastq_piece_device_finish waits for hip_stream, fills *counts as sk_trim_fastq_device_finish does and
 * *piece_counts (may be NULL), and clears the stream's range-error word as that call does -- but takes EVERY verdict
 * from this workspace: the range error is the word this piece's emission captured, never the live word, so that pieces
 * enqueued behind this one neither lend it their errors nor lose theirs to it.  It returns, in this order of precedence:
 * SK_ERANGE with inherited_range = 1 (the piece was void), SK_EFORMAT, SK_ERANGE, SK_ESPACE, SK_OK.
 * Bad arguments (those of the chained call; piece->reserved != 0; a start word that is not 8-byte aligned; a start word for
 * text[1] outside SK_TRIM_PE_SPLIT) return SK_EINVAL and enqueue nothing.
 */
typedef struct {
    const uint64_t *start_dev[2]; /* device, 8-byte aligned, or NULL (= 0): text i is bytes [*start_dev[i], n_i) of text[i] */
    uint32_t more;                /* != 0: more text follows this piece */
    uint32_t reserved;            /* 0 */
} sk_fastq_piece;

typedef struct {
    uint64_t consumed[2];      /* offset in text[i] of the first byte the piece did not consume */
    uint64_t carried_bytes[2]; /* n_i - consumed[i] */
    uint32_t ok;               /* the word a carry behind this piece goes by */
    uint32_t inherited_range;  /* 1: the stream's range-error word was set when the piece began; the piece was void */
} sk_fastq_piece_counts;

int sk_trim_fastq_piece_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in,
                                     const sk_fastq_lengths *lengths, const sk_fastq_piece *piece, int mode,
                                     const sk_fastq_output out[3], void *workspace, size_t workspace_bytes,
                                     void *hip_stream);
int sk_trim_fastq_piece_words(void *workspace, int input, const uint64_t **consumed_dev, const uint64_t **end_dev,
                              const uint64_t **ok_dev);
int sk_trim_fastq_piece_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts,
                                      sk_fastq_piece_counts *piece_counts);

/*
 * The carry between two pieces: enqueued behind the previous piece, it moves what that piece did not consume of input
 * `input` in front of the next chunk of text and writes the words the next piece takes its window from.  The caller (or a
 * reader: room is a multiple of 16, so a reader's `out` can point there) puts the next chunk at next_text + room; its length
 * is min(*chunk_bytes_dev, chunk_bytes), or chunk_bytes for a NULL word.
 * With c = end - consumed of the piece that used prev_workspace, for `input` (prev_workspace == NULL, the first piece:
 * c = 0, ok = 1), the kernel sets status to the first of these that applies:
 *   1. prev_words != NULL and prev_words->status != 0:                    prev_words->status (sticky)
 *   1b. other_prev_words != NULL and other_prev_words->status != 0:       other_prev_words->status
 *   2. the previous piece's ok == 0:                                      1
 *   3. c > room:                                                          2
 *   4. chunk_valid_dev != NULL and *chunk_valid_dev == 0:                 3
 *   5. none of these:                                                     0
 * status == 0: prev_text[consumed, end) is copied to next_text[room - c, room) and *words = {room - c, room + chunk length,
 * 1, 0}.  status != 0: nothing is copied and *words = {room, room, 0, status}: the next piece sees an empty text, and every
 * later carry inherits the status: a stream that has failed never resumes behind the failure.
 * The words feed the next piece: in.text = next_text, in.bytes = room + chunk_bytes, lengths.bytes_dev = &words->end,
 * lengths.valid_dev = &words->valid, piece.start_dev = &words->start.
 * SK_TRIM_PE_SPLIT runs one carry per input, each with the OTHER input's previous words as other_prev_words (NULL
 * elsewhere): a status that only one input meets (its carry beyond room, its chunk invalid) empties that input's text at
 * once -- the piece then takes no record from either input -- and reaches the other input's words at the next carry, from
 * where both are sticky.
 * Source and destination have any alignment.  No byte of next_text outside [room - c, room) is written, none of prev_text
 * outside [consumed, end) is read.  prev_bytes is the previous piece's in->bytes[input]: the buffers must not overlap,
 * and [next_text, next_text + room) meeting [prev_text, prev_text + prev_bytes) is SK_EINVAL, as are a NULL ctx, next_text
 * or words, prev_workspace given without prev_text, an input other than 0 / 1, room not a multiple of 16, words that are not
 * 8-byte aligned, and `words` being one of the two previous words (keep two sets and alternate).  One kernel is enqueued,
 * its grid sized by room: no allocation, no copy, no wait.
 */
typedef struct {
    uint64_t start, end, valid, status;
} sk_fastq_carry_words; /* device memory, 8-byte aligned */

int sk_fastq_carry_device_async(sk_ctx *ctx, const void *prev_workspace, int input, const uint8_t *prev_text,
                                uint64_t prev_bytes, uint8_t *next_text, uint64_t room, const uint64_t *chunk_bytes_dev,
                                uint64_t chunk_bytes, const uint64_t *chunk_valid_dev,
                                const sk_fastq_carry_words *prev_words, const sk_fastq_carry_words *other_prev_words,
                                sk_fastq_carry_words *words, void *hip_stream);

/*
 * The FASTQ trim in pieces in the reference's -a T order: sk_trim_fastq_piece_device_async whose records are the lines of
 * the reader's BATCHES (sk_trim_fastq_ordered_device_async's rule) that the piece can commit, emitted in the -a T order.
 * The reader keeps little between batches: after a batch a is its end and c = e, c - a = (e - a) % m < m, and the next stop
 * depends on lines [a, e) only.  So the k_i = c_i - a_i of every input, in a STATE in device memory, is all a piece needs
 * to go on where the last one stopped; batches go in input order, so the pieces' outputs, one after the other, are the
 * whole file's ordered output.  This comment is the normative text.
 *
 * What holds as sk_trim_fastq_piece_device_async defines it: the window, start_dev, lengths and more; "a line exists only
 * if its '\n' lies in the window" when more != 0, and the closed unterminated last line when more == 0; the captured
 * range-error word and the void piece behind it; read numbers counting from the piece's first record; nothing is written on
 * an error; sk_trim_fastq_piece_words and sk_trim_fastq_output_words on this workspace, and sk_fastq_carry_device_async
 * behind it.  piece, order and state_out are required.
 * The walk.  Line numbers count from the window's first line.  The reader's rule with L = order->batch_len, m and the
 * threads as in the ordered call, from a_i = 0 and c_i = min(state_in->carried_lines[i], lines_i) (state_in == NULL: a
 * state of zeros); unless state_in->ended, batch after batch:
 *   1. state_in->batches + the piece's batches == order->batch_limit != 0: the run has ended.
 *   2. The stop e_i of every input.  more != 0: e_i exists only if the budget is used up on a line of the window (the
 *      smallest e > c_i with sum(len(lines[a_i:e])) >= L); if c_i == lines_i, or the window's lines run out first, the
 *      batch is UNDETERMINED.  more == 0: the text's end is the reader's end of input, exactly as in the ordered call.
 *      The batch of input i is lines [a_i, e_i - (e_i - a_i) % m).
 *   3. In this order: input 0's batch determined and empty: the run has ended.  A batch undetermined: the walk ends here
 *      (undetermined = 1), nothing of this batch is committed.  PE split: input 1's batch empty: the run has ended; the
 *      two batches differ in their line count: the run has ended, stopped_on_mismatch = 1.
 *   4. The piece's table is full (order->batch_capacity batches committed): the walk ends here (table_full = 1).  This is
 *      never an error, in a closing piece neither: the rest is carry and the state stays open; the caller runs further
 *      pieces with more == 0 on the carry until one is not full.
 *   5. The batch is committed: a_i = its end, c_i = e_i.
 * The records of the piece are lines [0, a_i) of each input: they are checked, packed, scanned, routed and emitted as the
 * ordered call does on a text made of them, with the table of the piece's own batches (record_index in emission order).
 * Everything behind them is carry: not checked, not scanned, no format or range error comes from it.  SK_FQ_PAIR_COUNT never
 * occurs, dropped_unpaired is 0.
 * Counts.  consumed_i = the start of line a_i (s_i when nothing was committed; never beyond n_i).  records_in[i] = a_i / 4,
 * tail_lines[i] = lines_i - a_i.  order_counts: batches, units, last_batch_units (0 without a batch), records_unbatched
 * (lines_i / 4 - a_i / 4) and stopped_on_mismatch are the piece's own; error_batch is stream-wide (state_in->batches + the
 * piece's batch).
 * *state_out = *state_in with carried_lines[i] = c_i - a_i, batches and units advanced, last_batch_units replaced if the
 * piece committed a batch, ended and stopped_on_mismatch set where they apply (sticky).  A piece that starts from `ended`
 * commits nothing, ok = 1, and its whole window is carry.
 * Lines gzgets would split.  Every complete line of the window is checked against batch_len - 1, committed or not, whatever
 * the state, so carried lines are checked again in the next piece, and the stream refuses exactly the texts the ordered call
 * refuses: SK_ELONGLINE with long_line counting from the window's first line; the piece writes nothing.  Deviation: the
 * pieces before it have already been emitted.
 * Failures.  Whenever finish returns anything but SK_OK for a piece, its emission has written ok = 0 and *state_out =
 * *state_in with failed = 1, on the stream.  A piece that starts from `failed` is void: it commits nothing, checks
 * nothing, ok = 0, inherited_failure = 1, every count is 0, *state_out = *state_in, and its finish returns SK_OK: the first
 * failing piece is the one that reports.  A piece that finds the stream's range-error word set is void in the same way,
 * and its finish returns SK_ERANGE with inherited_range = 1 (whether or not the state had failed too).
 * finish returns, in this order of precedence: SK_ERANGE with inherited_range = 1, SK_OK with inherited_failure = 1,
 * SK_ELONGLINE, SK_EFORMAT, SK_ERANGE, SK_ESPACE (the outputs only: the table never gives it), SK_OK.  It takes every verdict
 * from this workspace, as sk_trim_fastq_piece_device_finish does.
 *
 * The workspace: the header keeps the piece's words, and the order words get a block of 256 bytes of their own in front of
 * the batch table:
 *   sk_trim_fastq_ordered_piece_workspace_bytes(text_bytes, trunc_n, batch_capacity)
 *       = sk_trim_fastq_ordered_workspace_bytes(text_bytes, trunc_n, batch_capacity) + 256
 * The workspace's contents on entry are arbitrary, and nothing outside [workspace, workspace + bytes) is written.
 * A batch usually holds about batch_len bytes, so batch_capacity = text_bytes / batch_len + 16 is a good guess, and a wrong
 * one costs nothing but shorter pieces.  The walk's serial loop is bounded by batch_capacity + 1 steps.
 * Same discipline: only kernels are enqueued, finish is the only call that waits.  SK_EINVAL, nothing enqueued: the bad
 * arguments of sk_trim_fastq_ordered_device_async and of sk_trim_fastq_piece_device_async; piece, order or state_out NULL;
 * state_in == state_out; a state that is not 8-byte aligned; a short workspace.
 */
typedef struct {                 /* device memory, 8-byte aligned, 64 bytes; all zero = the start of a stream */
    uint64_t carried_lines[2];   /* k_i = c - a of input i: complete lines at the window's start that the reader had
                                    already taken when the last batch was cut; always < m */
    uint64_t batches, units;     /* stream-wide, up to this piece's start */
    uint64_t last_batch_units;
    uint32_t ended;              /* the run is over (empty batch, PE mismatch, batch_limit reached): later pieces take nothing */
    uint32_t stopped_on_mismatch;
    uint32_t failed;             /* a piece before this one failed: later pieces are void */
    uint32_t reserved0;
    uint64_t reserved1;
} sk_fastq_order_state;

typedef struct {
    uint32_t table_full;        /* the walk stopped at a full batch table: call again on the carry */
    uint32_t undetermined;      /* the walk stopped because a stop line is not in the window yet */
    uint32_t inherited_failure; /* state_in->failed: the piece was void */
    uint32_t reserved;
    sk_fastq_order_state state; /* a host copy of *state_out as the piece wrote it */
} sk_fastq_order_piece_counts;

size_t sk_trim_fastq_ordered_piece_workspace_bytes(uint64_t text_bytes, int32_t trunc_n, uint64_t batch_capacity); /* pure */
int sk_trim_fastq_ordered_piece_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in,
                                             const sk_fastq_lengths *lengths, const sk_fastq_piece *piece,
                                             const sk_fastq_order *order, const sk_fastq_order_state *state_in,
                                             sk_fastq_order_state *state_out, int mode, const sk_fastq_output out[3],
                                             void *workspace, size_t workspace_bytes, void *hip_stream);
/* Waits for hip_stream and fills the counts (all but `counts` may be NULL). */
int sk_trim_fastq_ordered_piece_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_counts *counts,
                                              sk_fastq_order_counts *order_counts, sk_fastq_piece_counts *piece_counts,
                                              sk_fastq_order_piece_counts *order_piece_counts);

/*
 * The trim report: what a run cut, on the device, over the workspace of a text call that has been enqueued on the same
 * stream.  It gives sickle's closing summary (the kept / discarded lines), base counts and, optionally, length and
 * per-position quality histograms.  It is exact integer arithmetic and accumulates in device memory, so a stream of pieces
 * yields one report for the file with no host wait in between.  This comment is the normative text; the rule as code is
 * sickle_amd/csrc/sk_fastq_report.h.  The host CLI does not use this call: it counts on the host, as it always did.
 *
 * The rule.  Read r of the call's packed batch has input length len = offsets[r + 1] - offsets[r] (its quality line) and
 * the cut {five, three}; it is kept iff three >= 0, and then its output length is three - five.  Only the reads the call
 * trimmed are reads (an interleaved text's odd last record, dropped_unpaired, and a piece's carry are in no count).  In
 * the pair modes reads 2k and 2k + 1 are pair k.
 *   calls, calls_failed   calls that added / that did not (below)
 *   reads, kept, discarded
 *   pairs[kept1 | kept2 << 1]   pairs by which mates are kept; all zero for SK_TRIM_SE.  The reference's numbers:
 *       kept_p = 2 pairs[3]; kept_s1 = discard_s2 = pairs[1]; kept_s2 = discard_s1 = pairs[2]; discard_p = 2 pairs[0];
 *       the N records of SK_TRIM_PE_COMBO_ALL are 2 pairs[0] + pairs[1] + pairs[2]
 *   bases_in, bases_out   sum of len over all reads; of three - five over kept reads
 *   bases_cut5, bases_cut3   of kept reads: five and len - three;  bases_discarded: len of the reads not kept
 *   reads_cut5, reads_cut3   kept reads with five != 0, with three != len
 *   max_len_in, max_len_out   the longest input; the longest output of a kept read
 * Histograms (sk_fastq_report_hists, may be NULL, as may each array in it; device arrays of uint64_t that the caller owns
 * and sizes): len_in[len_bins] and len_out[len_bins] count reads in bin min(length, len_bins - 1), len_out kept reads
 * only by output length.  qsum_in / qcnt_in [pos_bins]: the sum of the RAW quality bytes and their number at position
 * min(p, pos_bins - 1), p counted from the read's first base, over all reads; qsum_out / qcnt_out: the same over the
 * three - five output bytes of kept reads, p counted from five.  Mean quality at a position is sum / cnt less
 * sk_quality_constants(qualtype)[0]; that is left to the caller.  len_bins <= SK_FQ_REPORT_MAX_LEN_BINS and pos_bins <=
 * SK_FQ_REPORT_MAX_POS_BINS: the tables are summed in LDS, 2 * 4 * 4096 = 32 KiB of 32-bit length counters and 2 * 8 *
 * 2048 = 32 KiB of 64-bit position words, beside each other within the 64 KiB a workgroup may hold.
 * Validity.  A call adds iff it has no format verdict and no range verdict, taken from its own workspace: SK_EFORMAT or
 * SK_ERANGE of its finish (for the piece kinds also a range error inherited from the stream: a void piece adds nothing),
 * and SK_ELONGLINE / a full batch table of sk_trim_fastq_ordered_device_async, after which nothing was written either.
 * SK_ESPACE does not matter: a counting call, with every output NULL, reports in full.  A call that adds increments calls;
 * one that does not increments calls_failed and touches nothing else, neither in the struct nor in the arrays.
 * The source.  src->workspace is the text call's workspace and src->kind says which call wrote it:
 *   SK_FQ_REPORT_PLAIN          sk_trim_fastq_device_async, the chained call without an order, the piece call with piece == NULL
 *   SK_FQ_REPORT_PIECE          sk_trim_fastq_piece_device_async with a piece
 *   SK_FQ_REPORT_ORDERED        sk_trim_fastq_ordered_device_async, the chained call with an order
 *   SK_FQ_REPORT_ORDERED_PIECE  sk_trim_fastq_ordered_piece_device_async
 * text_bytes, trunc_n and (ordered kinds) batch_capacity are what the call's workspace formula was called with: bytes[0] +
 * bytes[1] of its input, params->trunc_n, order->batch_capacity.  They locate the sections; wrong ones read the wrong words.
 * When.  The call must be enqueued on the text call's stream, after that call (its emission writes the range verdict the
 * report goes by) and before the workspace is used again.  It only enqueues kernels: no copy, no allocation, no
 * synchronisation, no host wait, and nothing is read from the texts.  flags: SK_FQ_REPORT_RESET zeroes *report_dev and the
 * given arrays first (a kernel of its own); without it the call adds to what they hold.  report_dev is device memory; the
 * caller copies it back after its own wait.
 * SK_EINVAL, with sk_last_error text and nothing enqueued: ctx, src, src->workspace or report_dev NULL; a workspace that
 * is not 16-byte aligned, a report or an array that is not 8-byte aligned; an unknown kind; flags other than
 * SK_FQ_REPORT_RESET; src->reserved != 0; len_bins (pos_bins) of 0 with a length (position) array given, or above its limit.
 */
#define SK_FQ_REPORT_RESET 1
#define SK_FQ_REPORT_MAX_LEN_BINS 4096u
#define SK_FQ_REPORT_MAX_POS_BINS 2048u
enum { SK_FQ_REPORT_PLAIN = 0, SK_FQ_REPORT_PIECE = 1, SK_FQ_REPORT_ORDERED = 2, SK_FQ_REPORT_ORDERED_PIECE = 3 };

typedef struct {
    uint64_t calls, calls_failed;
    uint64_t reads, kept, discarded;
    uint64_t pairs[4];
    uint64_t bases_in, bases_out;
    uint64_t bases_cut5, bases_cut3;
    uint64_t bases_discarded;
    uint64_t reads_cut5, reads_cut3;
    uint64_t max_len_in, max_len_out;
} sk_fastq_report; /* device memory, 8-byte aligned, 144 bytes */

typedef struct {
    const void *workspace;   /* device: the text call's workspace */
    uint32_t kind;           /* SK_FQ_REPORT_* */
    int32_t trunc_n;
    uint64_t text_bytes;
    uint64_t batch_capacity; /* ordered kinds; ignored by the others */
    uint64_t reserved;       /* 0 */
} sk_fastq_report_source;

typedef struct {
    uint64_t *len_in, *len_out; /* device, 8-byte aligned, or NULL */
    uint64_t len_bins;
    uint64_t *qsum_in, *qcnt_in, *qsum_out, *qcnt_out;
    uint64_t pos_bins;
} sk_fastq_report_hists;

int sk_trim_fastq_report_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, sk_fastq_report *report_dev,
                                      const sk_fastq_report_hists *hists, int flags, void *hip_stream);

/*
 * The audit: whether a paired run made sense, on the device, over the workspace AND the texts of a text call that has been
 * enqueued on the same stream.  It compares the names of the two mates of every pair and gives the range of the quality
 * bytes, the two mistakes (mates that are not mates, the wrong -t) that neither the reference nor a text call notices.
 * Exact integers, accumulated in device memory like the report.  Nothing acts on the verdict: the caller decides.  This
 * comment is the normative text; the rule as code is sickle_amd/csrc/sk_fastq_audit.h.  The host CLI does not use it.
 *
 * Key of a name line.  The name line is the record's first line without its '\n'; byte 0 is '@' in any call that adds.
 * The key is bytes [1, e): e is the index of the first byte at or after index 1 that is ' ' (0x20), '\t' (0x09) or '\r'
 * (0x0d), or the line's length if there is none.  Then, once: if the key has 2 bytes or more, its last but one is '/' and
 * its last is '1' or '2', the tag is that digit and the key loses those two bytes; otherwise the tag is 0.  An empty key
 * is a key.  ("@x/1/1" has the key "x/1" and the tag 1; "@x/3" the key "x/3"; "@/1" the empty key and the tag 1.)
 * Pair k is reads 2k and 2k + 1 of the call's packed batch (SK_TRIM_PE_SPLIT, SK_TRIM_PE_INTERLEAVED and
 * SK_TRIM_PE_COMBO_ALL, which frames as interleaved), only where both lie below the reads the call trimmed: a dropped odd
 * record and a piece's carry are in no count (the report's rule).  The pair MATCHES iff the two keys have the same length
 * and the same bytes; it is TAG-SWAPPED iff it matches, mate 1's tag is 2 and mate 2's tag is 1.  SK_TRIM_SE has no pairs.
 * CASAVA 1.8 names match through the space rule, "/1" "/2" names through the tag rule, names with neither must be equal.
 *   calls, calls_failed   calls that added / that did not (below)
 *   pairs                 pairs whose names were compared
 *   name_mismatch         of them: the keys differ
 *   first_mismatch        the lowest such pair, pairs numbered over all ADDING calls since the reset, in call order; ~0: none.
 *                         Over a stream of pieces that is the pair's number in the file; in the ordered kinds the number in
 *                         read order, not in emission order
 *   tags_swapped          matching pairs with the tags 2, 1
 *   qual_bytes, qual_min, qual_max   number, lowest and highest of ALL bytes of the quality lines of the call's reads, taken
 *                         as unsigned (the bytes of the packed batch; params->trunc_n plays no part, nor do the cuts);
 *                         qual_min = ~0 and qual_max = 0 while qual_bytes == 0
 *   reserved              the kernels' own words: a call's lowest mismatch and pair count before they are folded
 * qual_hist_dev (device, uint64_t[256], 8-byte aligned, or NULL): qual_hist_dev[b] counts the quality bytes of value b.
 * src is the report's source descriptor, with the same four kinds and the same meaning of text_bytes, trunc_n and
 * batch_capacity: text_bytes is what THAT call's workspace formula took (a piece lays its sections out by its own bounds).
 * in and mode are what the text call was given: the text pointers for the names, in->bytes as bounds of every load of a
 * name byte (the descriptors count from text[i], also in a piece).  in == NULL: the names are not looked at and pairs,
 * name_mismatch, first_mismatch and tags_swapped stay as they are; the same holds for SK_TRIM_SE.  The quality part needs no
 * text.
 * Validity is the report's, from the call's own workspace; and a mode whose framing mode (SK_TRIM_PE_COMBO_ALL ->
 * SK_TRIM_PE_INTERLEAVED) differs from the one the text call recorded counts as failed too.  A call that does not add
 * increments calls_failed and touches nothing else, neither in the struct nor in the histogram.
 * When.  On the text call's stream, behind it, before the workspace AND THE TEXTS are reused (a stream driver's text
 * buffers rotate).  It only enqueues kernels: no copy, no allocation, no wait.  A zeroed struct is not a valid start
 * (first_mismatch and qual_min start at ~0): the first call on a struct carries SK_FQ_AUDIT_RESET, which sets the struct and
 * zeroes the histogram by a kernel of its own in front.  Calls that add to one struct must be on one stream; the pair
 * numbering is their order.
 * SK_EINVAL, with sk_last_error text and nothing enqueued: ctx, src, src->workspace or audit_dev NULL; a workspace that is
 * not 16-byte aligned, a struct or a histogram that is not 8-byte aligned; an unknown kind or mode; with in given:
 * SK_TRIM_PE_SPLIT and text[1] NULL, another mode and text[1] not NULL, a pair mode and text[0] NULL with bytes[0] != 0;
 * flags other than SK_FQ_AUDIT_RESET; src->reserved != 0.
 */
#define SK_FQ_AUDIT_RESET 1

typedef struct {
    uint64_t calls, calls_failed;
    uint64_t pairs;
    uint64_t name_mismatch;
    uint64_t first_mismatch;
    uint64_t tags_swapped;
    uint64_t qual_bytes, qual_min, qual_max;
    uint64_t reserved[7];
} sk_fastq_audit; /* device memory, 8-byte aligned, 128 bytes */

int sk_trim_fastq_audit_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                     sk_fastq_audit *audit_dev, uint64_t *qual_hist_dev, int flags, void *hip_stream);

/*
 * The bases: what the reads are made of, on the device, over the workspace AND the texts of a text call that has been
 * enqueued on the same stream: base content and N content per position, the reads that hold an N at all, GC per read,
 * each before and after the cut.  It is what tells whether params->trunc_n (-n) is worth passing and what it will cost.
 * Exact integers, accumulated in device memory like the report and the audit.  Nothing acts on the result.  This comment
 * is the normative text; the rule as code is sickle_amd/csrc/sk_fastq_bases.h.  The host CLI does not use it.
 *
 * Classes of a seq byte b: 0 'A' 'a'; 1 'C' 'c'; 2 'G' 'g'; 3 'T' 't'; 4 'N' 'n'; 5 everything else (IUPAC codes, '.',
 * 'U', '\r', bytes >= 0x80).  A byte is LOWER iff it lies in 'a'..'z', whatever its class.
 * Reads are the report's: read r of the call's packed batch counts only if it lies below the reads the call trimmed; its
 * cut {five, three} is the workspace's; it is kept iff three >= 0, and then its output is bytes [five, three) of its seq
 * line.  A dropped odd record and a piece's carry are in no count; the N records of SK_TRIM_PE_COMBO_ALL are not output
 * bytes, so every `out` figure covers kept reads only.  In the ordered kinds the reads are in read order, which plays no
 * part.
 * The seq line of read r is found as the audit finds its name line: through the call's record descriptors, in text[0],
 * or for SK_TRIM_PE_SPLIT in text[r & 1]; it is the bytes from behind the name line's '\n' to the seq line's '\n', counted
 * from text[i], also in a piece.  In a call that adds its length is offsets[r + 1] - offsets[r], the quality line's.
 * Position p counts from the line's first byte.  The bytes are always the text's, with params->trunc_n or without.
 *   calls, calls_failed   calls that added / that did not (below)
 *   reads, kept           as in the report
 *   bases_in[c]           seq bytes of class c over all reads;  bases_out[c]: over the output bytes of kept reads
 *   lower_in, lower_out   LOWER bytes likewise
 *   reads_n_in            reads with at least one byte of class 4;  reads_n_out: kept reads whose output holds one
 *   gc_none_in            reads with no byte of class 0-3;  gc_none_out: kept reads whose output has none (an empty output
 *                         is one)
 *   reserved              zero
 * Arrays (sk_fastq_bases_hists, may be NULL, as may each array in it; device arrays of uint64_t that the caller owns):
 * pos_in[6 * pos_bins] and pos_out[6 * pos_bins]: entry c * pos_bins + min(p, pos_bins - 1) counts the bytes of class c
 * at position p; for pos_out over output bytes, p counted from five.  pos_bins <= SK_FQ_BASES_MAX_POS_BINS: the tables are
 * summed in LDS, 2 * 6 * 1024 32-bit counters, 48 KiB.  gc_in[101] and gc_out[101]: a read whose bytes of class 0-3 number
 * acgt > 0 counts in bin floor(100 * (C + G) / acgt), C and G its bytes of classes 1 and 2; gc_out: kept reads, over their
 * output.  A read with acgt == 0 counts in gc_none_* instead.
 * src is the report's source descriptor.  in and mode are what the text call was given; the texts are required, they are
 * the data, and in->bytes bound every load of a seq byte.
 * Validity is the audit's: the report's, from the call's own workspace, and a mode whose framing mode differs from the one
 * the text call recorded counts as failed too.  A call that does not add increments calls_failed and touches nothing else,
 * neither in the struct nor in the arrays.  SK_ESPACE does not matter: a counting call reports in full.
 * When.  On the text call's stream, behind it, before the workspace AND THE TEXTS are reused.  It only enqueues kernels: no
 * copy, no allocation, no wait.  SK_FQ_BASES_RESET zeroes the struct and the given arrays first, by a kernel of its own; a
 * zeroed struct is a valid start.  Calls that add to one struct must be on one stream.
 * SK_EINVAL, with sk_last_error text and nothing enqueued: ctx, src, src->workspace, bases_dev or in NULL; a workspace
 * that is not 16-byte aligned, a struct or an array that is not 8-byte aligned; an unknown kind, mode or flags;
 * src->reserved != 0; SK_TRIM_PE_SPLIT and text[1] NULL, another mode and text[1] not NULL; text[0] NULL with bytes[0] != 0;
 * pos_bins of 0 with a position array given, or above its limit.
 */
#define SK_FQ_BASES_RESET 1
#define SK_FQ_BASES_MAX_POS_BINS 1024u
#define SK_FQ_BASES_GC_BINS 101u

typedef struct {
    uint64_t calls, calls_failed;
    uint64_t reads, kept;
    uint64_t bases_in[6], bases_out[6];
    uint64_t lower_in, lower_out;
    uint64_t reads_n_in, reads_n_out;
    uint64_t gc_none_in, gc_none_out;
    uint64_t reserved[2];
} sk_fastq_bases; /* device memory, 8-byte aligned, 192 bytes */

typedef struct {
    uint64_t *pos_in, *pos_out; /* device, 8-byte aligned, [6 * pos_bins], or NULL */
    uint64_t pos_bins;
    uint64_t *gc_in, *gc_out;   /* device, 8-byte aligned, [SK_FQ_BASES_GC_BINS], or NULL */
} sk_fastq_bases_hists;

int sk_trim_fastq_bases_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                     sk_fastq_bases *bases_dev, const sk_fastq_bases_hists *hists, int flags,
                                     void *hip_stream);

/*
 * The rejects: the records of the reads a text call did NOT keep, as FASTQ text in device memory, over the workspace AND
 * the texts of a text call that has been enqueued on the same stream.  It is fastp's --failed_out and cutadapt's
 * --too-short-output: the records to look at, or to trim again with other settings.  The reference has no counterpart (it
 * drops them); what ties this to it is conservation: what the text call wrote plus the rejects is what it read.  This
 * comment is the normative text; the rule as code is sickle_amd/csrc/sk_fastq_rejects.h.  The host CLI does not use it.
 *
 * Reads are the report's: read r of the text call's packed batch with r < the reads the call trimmed (the header's
 * SK_FQ_H_NREAL).  A dropped odd record, a piece's carry and the records behind an ordered call's last batch are not reads.
 * A read is kept iff its cut has three >= 0.  In the pair framings reads 2k and 2k + 1 are pair k.
 * Selection.  flags == 0: every read that is not kept.  SK_FQ_REJECTS_PAIRS: both mates of every pair of which at least one
 * mate is not kept, kept mates included; the rejects text is then a valid interleaved text that can be trimmed again.
 * SK_FQ_REJECTS_PAIRS with SK_TRIM_SE is SK_EINVAL.  SK_TRIM_PE_COMBO_ALL selects as SK_TRIM_PE_INTERLEAVED does; the N
 * records it emitted are no part of this.
 * Record.  A record is the input's own four lines, uncut: bytes [s0, e3) of the record's text (SK_TRIM_PE_SPLIT: text[r & 1]),
 * s0 the name line's first byte and e3 the end of the quality line, then one '\n': e3 - s0 + 1 bytes.  The closing '\n' is
 * always synthesized and never loaded, so an unterminated last line gains it (in the chained forms the byte at e3 lies
 * beyond the text).  A '\r' belongs to its line and is copied.
 * Order.  Read order, in every kind: the ordered kinds do not reorder the rejects (the audit numbers its pairs the same way).
 * Index.  out->record_index gets the read number of each record, in the text call's numbering.
 * Validity is the audit's, taken from the text call's own workspace: no format verdict, no range verdict (for the piece
 * kinds also none inherited: a void piece), not SK_ELONGLINE nor a full batch table; and a mode whose framing mode
 * (SK_TRIM_PE_COMBO_ALL -> SK_TRIM_PE_INTERLEAVED) differs from the one the text call recorded makes the call void too.  A void
 * call writes nothing to `out`; its counts are records = bytes = reads = 0 and valid = 0, its words are *bytes_dev = 0 and
 * *written_dev = 0, and its finish returns SK_OK.  SK_ESPACE of the text call does not matter: a counting text call can be
 * followed by a counting rejects call.
 * Capacity.  out == NULL or out->text == NULL: the call only counts (its words are 0).  Bytes beyond out->capacity, or
 * records beyond out->record_capacity with a record_index given: nothing is written to either buffer, finish returns
 * SK_ESPACE with the needs in counts, and the words are 0.  A text buffer of sk_trim_fastq_rejects_bound(T) = T + 2 bytes
 * always fits, T = the text call's bytes[0] + bytes[1]: the records' spans are disjoint parts of the texts, and every
 * record's '\n' but an unterminated last line's (one per text) is a text byte outside every span.
 * Counts.  records, bytes: the selected records and their bytes, exact: bytes is the sum of e3 - s0 + 1 over them.  reads
 * is the reads the text call trimmed.  valid: 1, or 0 for a void call.  flags: the call's.
 * Words.  sk_trim_fastq_rejects_output_words gives two device words of the workspace with the meaning
 * sk_bgzf_input's bytes_dev and valid_dev take: the bytes written, and 1 iff they were written.  sk_bgzf_device_async chains
 * behind the rejects with no host wait; after a void call, a counting call or one that did not fit, its image is the EOF
 * member alone.
 * Workspace.  sk_trim_fastq_rejects_workspace_bytes(T) is a pure function of src->text_bytes:
 *   128 + 16 ceil(N / 2048) + 16 N,  N = 2 floor((T + 2) / 16) + 2
 * a header, a table of blocks and an output offset and a read number per read the packed batch can hold, the emission's
 * cost.  Its contents on entry are arbitrary.  Nothing outside the workspace, out->text[0, capacity) and
 * out->record_index[0, record_capacity) is ever written.  Every load of a descriptor is bounded by the slots of the text
 * call's section, every load of a text byte by in->bytes[i]: a source that names the wrong layout or the wrong texts
 * gives wrong bytes, never a load outside the workspaces and the texts (but for the rest of an aligned 16-byte block that
 * holds a wanted byte, as in the text call), and never an unbounded walk.
 * When.  On the text call's stream, behind it, before its workspace AND ITS TEXTS are reused.  sk_trim_fastq_rejects_device_async
 * only enqueues kernels: no copy, no allocation, no wait; all scratch and counts live in `workspace`.  finish is the only
 * call that waits.  Two rejects calls in flight need two workspaces.  src is the report's source descriptor; in and mode
 * are what the text call was given.
 * SK_EINVAL, with sk_last_error text and nothing enqueued: ctx, src, src->workspace, in or workspace NULL; src->workspace,
 * workspace or out->text not 16-byte aligned, out->record_index not 8-byte aligned; an unknown kind, mode or flag;
 * SK_FQ_REJECTS_PAIRS with SK_TRIM_SE; src->reserved != 0; SK_TRIM_PE_SPLIT and text[1] NULL, another mode and text[1] not
 * NULL; a text NULL with bytes != 0; workspace_bytes below sk_trim_fastq_rejects_workspace_bytes(src->text_bytes).
 */
#define SK_FQ_REJECTS_PAIRS 1

typedef struct {
    uint64_t records, bytes; /* the selected records and their bytes: what the buffers need */
    uint64_t reads;          /* the reads the text call trimmed */
    uint32_t valid;          /* 0: a void call */
    uint32_t flags;
} sk_fastq_rejects_counts;

size_t sk_trim_fastq_rejects_workspace_bytes(uint64_t text_bytes); /* pure, no device */
uint64_t sk_trim_fastq_rejects_bound(uint64_t text_bytes);         /* pure: a text buffer that always fits */
int sk_trim_fastq_rejects_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                       const sk_fastq_output *out, int flags, void *workspace, size_t workspace_bytes,
                                       void *hip_stream);
/* Waits for hip_stream and fills *counts: SK_OK, or SK_ESPACE with the needs. */
int sk_trim_fastq_rejects_device_finish(sk_ctx *ctx, void *workspace, void *hip_stream, sk_fastq_rejects_counts *counts);
int sk_trim_fastq_rejects_output_words(void *rejects_workspace, const uint64_t **bytes_dev, const uint64_t **written_dev);

/*
 * The adapters: where the reads run into a 3' adapter, on the device, over the workspace AND the texts of a text call that
 * has been enqueued on the same stream: per read the leftmost occurrence of up to eight adapter sequences, summed into
 * exact integer counts (FastQC's adapter content; the adapter bases that sickle's window trim leaves in the output; the
 * mates whose clip points agree) and, optionally, written as one clip point per read.  Nothing acts on the result: the
 * text call's output is what it was.  This comment is the normative text; the rule as code is
 * sickle_amd/csrc/sk_fastq_adapters.h.  The host CLI does not use it.
 *
 * The set (sk_fastq_adapter_set, host memory; the call reads it before it returns): n adapters, 1 .. SK_FQ_ADAPTERS_MAX;
 * len[a] in 1 .. SK_FQ_ADAPTER_MAX_LEN; seq[a][0 .. len[a]) bytes from "ACGTacgt" only, compared without regard to case
 * (the bytes behind len[a] play no part); min_overlap >= 1 and <= every len[a]; max_mismatch_permille in 0 .. 500;
 * reserved 0.
 * Reads are the report's: read r of the call's packed batch with r below the reads the call trimmed.  A dropped odd record,
 * a piece's carry and the records behind an ordered call's last batch are not reads.  In the pair framings reads 2k and
 * 2k + 1 are pair k, where both are reads.
 * The seq line of read r is the bases': found through the call's record descriptors in text[0], or for SK_TRIM_PE_SPLIT in
 * text[r & 1]; its length L is offsets[r + 1] - offsets[r]; its bytes are the text's, with params->trunc_n or without.
 * Matching.  A read byte b matches the adapter base c (upper case) iff (b & 0xDF) == c.  'N', IUPAC codes, '\r' and bytes
 * >= 0x80 match nothing.
 * A hit.  For adapter a of length A and a start p with 0 <= p <= L - min_overlap the overlap is v = min(A, L - p) and m is
 * the number of bytes among read[p .. p + v) that do not match adapter[0 .. v).  (a, p) is a hit iff v >= min_overlap and
 * m <= floor(v * max_mismatch_permille / 1000).  The read's hit is the hit with the lowest p, among the adapters at that p
 * the one with the lowest a; v and m are that hit's.  A read shorter than min_overlap has none.
 *   calls, calls_failed   calls that added / that did not (below)
 *   reads, kept           as in the report
 *   reads_hit             reads with a hit;  reads_hit_kept: kept reads with a hit
 *   hits[a]               reads whose hit is adapter a
 *   hits_full             hits with v == A;  hits_at_0: hits with p == 0 (no insert at all)
 *   mismatches            sum of m over the hits;  bases_behind: sum of L - p over the hits
 *   reads_hit_out         kept reads with a hit and p < three: adapter bases survive the quality trim
 *   bases_hit_out         sum over those reads of three - max(p, five)
 *   pairs_both, pairs_one pairs with a hit in both mates, in exactly one; both 0 for SK_TRIM_SE
 *   pairs_same_clip       pairs with a hit in both mates and equal p, the signature of a read-through
 *   reserved              zero
 * Arrays (sk_fastq_adapters_out, may be NULL, as may each array in it; device memory that the caller owns):
 * pos[8 * pos_bins] (uint64_t): entry a * pos_bins + min(p, pos_bins - 1) counts the hits of adapter a at p; pos_bins <=
 * SK_FQ_ADAPTERS_MAX_POS_BINS; FastQC's cumulative curve is a prefix sum that the caller takes.  overlap[8 * 65]
 * (uint64_t): entry a * 65 + v.  Both accumulate like the struct.  clip[clip_capacity] (uint32_t, 4-byte aligned): one
 * entry per read of THIS call, in the call's read numbering: a << 24 | p for a hit (p < 2^24 by SK_MAX_READ_LEN),
 * SK_FQ_CLIP_NONE for a read without one.  Entries at or beyond clip_capacity, and at or beyond the call's reads, are never
 * written; clip does not accumulate, and SK_FQ_ADAPTERS_RESET does not touch it.
 * src is the report's source descriptor.  in and mode are what the text call was given; the texts are required, and
 * in->bytes bound every load of a seq byte.
 * Validity is the bases': the report's, from the call's own workspace (a format or range verdict, a void piece,
 * SK_ELONGLINE, a full batch table), and a mode whose framing mode differs from the one the text call recorded counts as
 * failed too.  A call that does not add increments calls_failed and touches nothing else, neither in the struct nor in
 * pos, overlap or clip.  SK_ESPACE of the text call does not matter: a counting call is searched in full.
 * When.  On the text call's stream, behind it, before the workspace AND THE TEXTS are reused.  It only enqueues kernels: no
 * copy, no allocation, no wait.  SK_FQ_ADAPTERS_RESET zeroes the struct, pos and overlap first, by a kernel of its own; a
 * zeroed struct is a valid start.  Calls that add to one struct must be on one stream.
 * SK_EINVAL, with sk_last_error text and nothing enqueued: the bases' cases (ctx, src, src->workspace, adapters_dev or in
 * NULL; a workspace that is not 16-byte aligned, a struct or a uint64_t array that is not 8-byte aligned; an unknown kind,
 * mode or flags; src->reserved != 0; SK_TRIM_PE_SPLIT and text[1] NULL, another mode and text[1] not NULL; text[0] NULL with
 * bytes[0] != 0); set NULL or a set outside the bounds above; clip given with clip_capacity 0 or not 4-byte aligned;
 * pos_bins of 0 with pos given, or above its limit.
 */
#define SK_FQ_ADAPTERS_RESET 1
#define SK_FQ_ADAPTERS_MAX 8u
#define SK_FQ_ADAPTER_MAX_LEN 64u
#define SK_FQ_ADAPTERS_MAX_POS_BINS 2048u
#define SK_FQ_ADAPTERS_OVERLAP_BINS 65u
#define SK_FQ_CLIP_NONE 0xFFFFFFFFu

typedef struct {
    uint32_t n;
    uint32_t len[8];
    uint8_t seq[8][64];
    uint32_t min_overlap;
    uint32_t max_mismatch_permille;
    uint32_t reserved; /* 0 */
} sk_fastq_adapter_set; /* host memory, 560 bytes */

typedef struct {
    uint64_t calls, calls_failed;
    uint64_t reads, kept;
    uint64_t reads_hit, reads_hit_kept;
    uint64_t hits[8];
    uint64_t hits_full, hits_at_0;
    uint64_t mismatches, bases_behind;
    uint64_t reads_hit_out, bases_hit_out;
    uint64_t pairs_both, pairs_one, pairs_same_clip;
    uint64_t reserved;
} sk_fastq_adapters; /* device memory, 8-byte aligned, 192 bytes */

typedef struct {
    uint64_t *pos;     /* device, 8-byte aligned, [8 * pos_bins], or NULL */
    uint64_t pos_bins;
    uint64_t *overlap; /* device, 8-byte aligned, [8 * SK_FQ_ADAPTERS_OVERLAP_BINS], or NULL */
    uint32_t *clip;    /* device, 4-byte aligned, [clip_capacity], or NULL */
    uint64_t clip_capacity;
} sk_fastq_adapters_out;

int sk_trim_fastq_adapters_device_async(sk_ctx *ctx, const sk_fastq_report_source *src, const sk_fastq_input *in, int mode,
                                        const sk_fastq_adapter_set *set, sk_fastq_adapters *adapters_dev,
                                        const sk_fastq_adapters_out *out, int flags, void *hip_stream);

/*
 * The clipped text call: a text call of any kind that clips every read at its 3' adapter hit IN FRONT OF the quality trim,
 * on the device, inside the call: the search runs between the format checks and the pack, and the pack takes the first p
 * bases of a read with a hit at p.  This comment is the normative text; the rule as code is sickle_amd/csrc/
 * sk_fastq_clip.h (and, for the hit, sk_fastq_adapters.h).  The host CLI does not use it.
 *
 * The kind.  clip->lengths, piece, order, state_in and state_out are each NULL or what the call of that kind takes, and
 * the members that are not NULL name the kind exactly as the five calls above do: all NULL is sk_trim_fastq_device_async;
 * lengths alone the chained call; piece (with or without lengths) the piece call; order (with or without lengths) the
 * ordered call; state_out, which needs both piece and order, the ordered piece.  The finish is the finish of that kind,
 * and the header words, the output words and the piece words are unchanged.
 * The hit of a read is exactly the adapters' (above), with the seq line's length L taken from the record descriptor, the
 * bytes between the end of the name line and the end of the seq line, instead of the packed batch: the lowest start p,
 * then the lowest adapter a; partial overlaps at the read's end, min_overlap and the permille allowance; either case
 * matches, and 'N', IUPAC codes, '\r' and bytes >= 0x80 match nothing.  Mates are clipped independently.
 * The packed length of read r is min(L, p) when the read has a hit and L otherwise.  Everything behind the clip point
 * does not exist for the scan: a quality byte out of range behind p is no SK_ERANGE, an 'N' behind p does not count for
 * params->trunc_n, and params->length_threshold applies to the clipped length.  A read clipped to 0 bases (p == 0) is an
 * empty read, which the scan discards; the pair rule then routes its mate to the singles, and SK_TRIM_PE_COMBO_ALL
 * writes it as an N record.  No new check refuses it: SK_FQ_SEQ_EMPTY stays a property of the text alone.
 * The output is therefore what the unclipped call writes for a text whose hit reads had seq and qual cut to p bytes
 * before the call saw them (with p >= 1; no valid text holds a p == 0 read's truncation).  Format checks, framing, pair
 * counts, read numbering, ordering, capacities and "nothing is written on an error" are untouched, and a clipped call's
 * outputs never exceed the unclipped call's bounds (sk_trim_fastq_output_bound and the like hold as they are).
 * The workspace is the kind's own (sk_trim_fastq_workspace_bytes, .._ordered_.., .._ordered_piece_..) plus
 * sk_trim_fastq_clip_extra_bytes(text_bytes): a 128-byte block of this call's own sums and 4 * (2H + 2) bytes of clip
 * words, H = (text_bytes + 2) / 16, rounded up to 16.  The clip section is the last `extra` bytes of that requirement, so
 * no section of the kind's layout moves and a sk_fastq_report_source describes the workspace as it always did.
 * *clip->clip_words_dev (where clip_words_dev is not NULL) is set before the call returns to where this call's clip
 * words lie in its workspace: one uint32_t per read, in the call's read numbering, a << 24 | p or SK_FQ_CLIP_NONE,
 * written for the reads of a call without a format verdict and valid until the workspace is reused.
 * clip->stats_dev (device memory that the caller owns, or NULL) accumulates like the side calls' structs: a one-workgroup
 * kernel behind the emission adds this call's sums iff the call's verdict is clean, with the report's validity (above),
 * read from the call's own workspace; otherwise it increments calls_failed and touches nothing else.
 *   calls, calls_failed   calls that added / that did not
 *   reads                 the reads of the call (the report's)
 *   reads_clipped         reads with a hit;  reads_emptied: those with p == 0
 *   bases_clipped         sum of L - p over the hits
 *   hits[a]               reads whose hit is adapter a
 *   reserved              zero
 * SK_FQ_CLIP_RESET zeroes the struct first, by a kernel of its own; a zeroed struct is a valid start.  Calls that add to
 * one struct must be on one stream.
 * What the side calls see behind a clipped call.  The report, the bases, the audit, the adapters and the rejects take a
 * read's length from the packed batch, so they describe the run as if the text had held the clipped reads: the report's
 * bases_in is after the clip, and what is missing is bases_clipped; the adapters search the clipped reads; a read
 * emptied by the clip counts among the bases' reads and gc_none_in, as a read of no bases does by their rule.  The rejects
 * still write a discarded read's own four lines uncut, adapter included, so their identity "output + rejects = input" NO
 * LONGER HOLDS behind a clipped call: the kept reads have lost their clipped bases and no text holds them.
 * SK_EINVAL, with sk_last_error text and nothing enqueued: everything the call of the kind refuses; clip or clip->set
 * NULL; a set outside the adapters' bounds; clip->reserved != 0 or flags other than SK_FQ_CLIP_RESET; state_out without
 * piece and order; stats_dev not 8-byte aligned; a workspace smaller than the kind's size plus the extra.
 */
#define SK_FQ_CLIP_RESET 1u

typedef struct {
    uint64_t calls, calls_failed;
    uint64_t reads, reads_clipped, reads_emptied, bases_clipped;
    uint64_t hits[8];
    uint64_t reserved[2];
} sk_fastq_clip_stats; /* device memory, 8-byte aligned, 128 bytes */

typedef struct {
    const sk_fastq_adapter_set *set; /* required; host memory, read before the call returns */
    const sk_fastq_lengths *lengths;
    const sk_fastq_piece *piece;
    const sk_fastq_order *order;
    const sk_fastq_order_state *state_in;
    sk_fastq_order_state *state_out;     /* each NULL or as in the call of that kind */
    sk_fastq_clip_stats *stats_dev;      /* or NULL */
    const uint32_t **clip_words_dev;     /* out, or NULL: where this call's clip words lie in its workspace */
    uint32_t flags, reserved;            /* SK_FQ_CLIP_RESET; 0 */
} sk_fastq_clip;

size_t sk_trim_fastq_clip_extra_bytes(uint64_t text_bytes); /* pure, no device */
int sk_trim_fastq_clipped_device_async(sk_ctx *ctx, const sk_params *params, const sk_fastq_input *in, const sk_fastq_clip *clip,
                                       int mode, const sk_fastq_output out[3], void *workspace, size_t workspace_bytes,
                                       void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* SICKLE_AMD_H */
