// sk_fastq_report.h -- what one read, one pair and one quality byte of a finished text call add to a trim report
// (sk_trim_fastq_report_device_async, include/sickle_amd.h), as plain functions of integers: the read's
// input length (offsets[r + 1] - offsets[r] of the packed batch), its cut, and the call's header words.  Nothing here
// takes a pointer into device state.
//
// Reads.  Only reads below the header's SK_FQ_H_NREAL are reads.  Read r is kept iff three >= 0 (sk_fastq_record.h's
// fqr_kept), and then its output is bytes [five, three) of its len input bytes.  In the pair framings (SK_FQ_H_MODE other
// than SK_TRIM_SE) reads 2k and 2k + 1 are pair k; SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED, so its N records
// are the reads that are not kept: 2 * pairs[0] + pairs[1] + pairs[2].  An interleaved text's odd last record
// (dropped_unpaired) is checked and dropped by the framing: it is not in the packed batch and is in no count here.
// Calls.  A call adds iff it has no format verdict and no range verdict (fqs_valid, sk_fastq_source.h); one that does not add
// increments calls_failed and touches nothing else.  SK_ESPACE does not matter: the cuts are there either way.
// sk_fastq_report.hip calls these from its two kernels; tests/fastq_report/report_host.cpp runs them on the host.
#ifndef SK_FASTQ_REPORT_H
#define SK_FASTQ_REPORT_H

#include <stdint.h>

#include "sickle_amd.h"

#ifdef __HIPCC__
#define FQP_FN __host__ __device__ static inline
#else
#define FQP_FN static inline
#endif

// sk_fastq_report as 8-byte words, in the order of the struct (the kernels add by word)
enum {
    FQP_W_CALLS = 0,
    FQP_W_CALLS_FAILED,
    FQP_W_READS,
    FQP_W_KEPT,
    FQP_W_DISCARDED,
    FQP_W_PAIRS, // [4], indexed by kept1 | kept2 << 1
    FQP_W_BASES_IN = FQP_W_PAIRS + 4,
    FQP_W_BASES_OUT,
    FQP_W_BASES_CUT5,
    FQP_W_BASES_CUT3,
    FQP_W_BASES_DISCARDED,
    FQP_W_READS_CUT5,
    FQP_W_READS_CUT3,
    FQP_W_MAX_LEN_IN, // the two maxima are the last words: everything below them is a sum
    FQP_W_MAX_LEN_OUT,
    FQP_WORDS
};
#define FQP_SUM_WORDS FQP_W_MAX_LEN_IN
#ifdef __cplusplus
static_assert(sizeof(sk_fastq_report) == 8 * FQP_WORDS, "sk_fastq_report is FQP_WORDS words");
#endif

// The quality pass (sk_fq_report_qual_kernel): a workgroup takes FQP_CHUNK_BYTES of the packed qual, and sums raw quality
// bytes per position bin in 32-bit halves of LDS words before it flushes them: FQP_CHUNK_BYTES * 255 = 66 846 720 < 2^32.
#define FQP_CHUNK_BYTES (256u * 1024u)
#ifdef __cplusplus
static_assert((uint64_t)FQP_CHUNK_BYTES * 255u < (1ull << 32), "a chunk's sums fit 32 bits");
static_assert(FQP_CHUNK_BYTES % 4096u == 0, "a chunk is whole steps of 256 lanes x 16 bytes");
#endif

FQP_FN bool fqp_kept(int32_t three) { return three >= 0; }

// a histogram's bin: the last one takes everything from bins - 1 on (bins >= 1)
FQP_FN uint64_t fqp_bin(uint64_t x, uint64_t bins) { return x < bins - 1 ? x : bins - 1; }

// the class of pair k from its mates: the index into pairs[]
FQP_FN uint32_t fqp_pair_class(bool kept1, bool kept2) { return (kept1 ? 1u : 0u) | (kept2 ? 2u : 0u); }

// whether a read number is the first mate of a pair that lies wholly below n_real, under framing mode `mode`
FQP_FN bool fqp_pair_at(int64_t mode, uint64_t r, uint64_t n_real)
{
    return mode != SK_TRIM_SE && (r & 1) == 0 && r + 1 < n_real;
}

// what one read adds to the sum words (w[FQP_SUM_WORDS]) and the maxima; the pair words are fqp_add_pair's
FQP_FN void fqp_add_read(uint64_t len, int32_t five, int32_t three, uint64_t *w, uint64_t *max_in, uint64_t *max_out)
{
    w[FQP_W_READS] += 1;
    w[FQP_W_BASES_IN] += len;
    if (len > *max_in) *max_in = len;
    if (!fqp_kept(three)) {
        w[FQP_W_DISCARDED] += 1;
        w[FQP_W_BASES_DISCARDED] += len;
        return;
    }
    const uint64_t f = (uint64_t)five, t = (uint64_t)three, out = t - f;
    w[FQP_W_KEPT] += 1;
    w[FQP_W_BASES_OUT] += out;
    w[FQP_W_BASES_CUT5] += f;
    w[FQP_W_BASES_CUT3] += len - t;
    w[FQP_W_READS_CUT5] += f != 0;
    w[FQP_W_READS_CUT3] += len != t;
    if (out > *max_out) *max_out = out;
}

FQP_FN void fqp_add_pair(int32_t three1, int32_t three2, uint64_t *w)
{
    const uint32_t cls = fqp_pair_class(fqp_kept(three1), fqp_kept(three2));
    for (uint32_t k = 0; k < 4; ++k) w[FQP_W_PAIRS + k] += cls == k; // no runtime index: w lives in registers on the device
}

// byte p (from the read's first base) of a read with this cut is one of its output bytes; its output position is p - five
FQP_FN bool fqp_out_byte(uint64_t p, int32_t five, int32_t three)
{
    return fqp_kept(three) && p >= (uint64_t)five && p < (uint64_t)three;
}

// Where position bin p lies in a workgroup's LDS table.  The lanes of a wave hold granules 16 bytes apart, so at any moment
// their positions differ by multiples of 16: with 8-byte words in p's own order that is two banks for the whole wave.
// XOR-ing the low five bits with the five above them sends 64 such positions to 32 different words, the two-way conflict
// that 64 eight-byte words on 64 four-byte banks cannot avoid.  A bijection on every aligned group of 32 bins, so a
// table of fqp_slots(bins) words holds it.
FQP_FN uint32_t fqp_slot(uint32_t p) { return p ^ ((p >> 5) & 31u); }
FQP_FN uint32_t fqp_slots(uint32_t bins) { return (bins + 31u) & ~31u; }

// one position bin's LDS word: the count in the high half, the sum of raw bytes in the low half
FQP_FN uint64_t fqp_qword(uint32_t q) { return (1ull << 32) | (q & 0xffu); }

// Validity of the call behind a workspace: fqs_valid of sk_fastq_source.h.

#endif
