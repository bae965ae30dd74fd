// sk_fastq_record.h -- the bytes of one emitted FASTQ record of the device text path (sk_fastq.hip), as plain functions
// of integers: the record's line ends (the descriptor the framing kernels write), its cut, and the quality type's lowest
// quality byte Q (sk_quality_constants(qualtype)[1]).
//
// Two records (include/sickle_amd.h):
//   a kept read (three >= 0)  name line '\n' seq[five:three] '\n' the record's own '+' line '\n' qual[five:three] '\n'
//                             (reference src/trim_single.cpp:393-396): six pieces, four from the text, two newlines
//   a read that is not kept   SK_TRIM_PE_COMBO_ALL only: name line '\n' then the six bytes N '\n' + '\n' Q '\n' (the record
//                             of upstream sickle 1.33's -M): two pieces, the name line from the text and one immediate,
//                             in the same six-slot table (fqr_pieces)
// A piece is bytes [at, at + len) of the record's text, or the low len (<= 8) bytes of an immediate: no memory stands
// behind an immediate piece, so the gather of sk_fastq.hip never loads for one.
// sk_fastq.hip calls these from its emission and its gather; tests/fastq_combo/combo_host.cpp runs them on the host.
#ifndef SK_FASTQ_RECORD_H
#define SK_FASTQ_RECORD_H

#include <stdint.h>

#ifdef __HIPCC__
#define FQR_FN __host__ __device__ static inline
#else
#define FQR_FN static inline
#endif

#define FQR_IMM (~0ull) // fqr_piece.at of an immediate piece
#define FQR_N_TAIL 6u   // bytes of an N record behind its name line

struct fqr_lines {
    uint64_t s0, e0, e1, e2, e3; // name start, then the end ('\n' or end of text) of each of the four lines
};

struct fqr_piece {
    uint64_t at;  // offset in the record's text, or FQR_IMM
    uint64_t len;
    uint64_t imm; // FQR_IMM: byte k of the piece is imm >> 8k
};

FQR_FN bool fqr_kept(int32_t three) { return three >= 0; } // src/trim_single.cpp:368, src/trim_paired.cpp:500,502

// bytes of a kept read's record
FQR_FN uint64_t fqr_kept_bytes(const fqr_lines &x, int32_t five, int32_t three)
{
    return (x.e0 - x.s0 + 1) + (x.e2 - x.e1) + 2 * (uint64_t)(three - five + 1);
}

// bytes of the emitted record: a kept read's, or (not kept) the N record's
FQR_FN uint64_t fqr_bytes(const fqr_lines &x, int32_t five, int32_t three)
{
    if (!fqr_kept(three)) return (x.e0 - x.s0 + 1) + FQR_N_TAIL;
    return fqr_kept_bytes(x, five, three);
}

// N '\n' + '\n' Q '\n' as an immediate
FQR_FN uint64_t fqr_n_tail(uint32_t q)
{
    return (uint64_t)'N' | ((uint64_t)'\n' << 8) | ((uint64_t)'+' << 16) | ((uint64_t)'\n' << 24) | ((uint64_t)(q & 0xffu) << 32) |
           ((uint64_t)'\n' << 40);
}

// The piece table of a record: six slots whose kinds never change (0, 1, 3, 4 text, 2 and 5 immediates), so that one
// walk serves both records and only lengths and the immediate are chosen per read.  A kept read fills all six: name line,
// seq[five:three], '\n', '+' line, qual[five:three], '\n'.  An N record fills two, the name line (slot 0) and the six
// constant bytes (slot 2); its other slots are empty, and an empty piece is never looked at, let alone loaded.
// The name line's '\n' is the text's own in both: the name line of a complete record never ends at the end of the text,
// so x.e0 is always a byte of the text.
// combo_all: the flag of SK_TRIM_PE_COMBO_ALL; without it only kept reads are emitted, and every read handed in is one.
FQR_FN void fqr_pieces(const fqr_lines &x, int32_t five, int32_t three, bool combo_all, uint32_t q, fqr_piece (&pc)[6])
{
    const bool kept = !combo_all || fqr_kept(three);
    const uint64_t f = kept ? (uint64_t)five : 0, m = kept ? (uint64_t)(three - five) : 0;
    pc[0] = {x.s0, x.e0 - x.s0 + 1, 0};
    pc[1] = {x.e0 + 1 + f, m, 0};
    pc[2] = {FQR_IMM, kept ? 1u : FQR_N_TAIL, kept ? (uint64_t)'\n' : fqr_n_tail(q)};
    pc[3] = {x.e1 + 1, kept ? x.e2 - x.e1 : 0, 0};
    pc[4] = {x.e2 + 1 + f, m, 0};
    pc[5] = {FQR_IMM, kept ? 1u : 0u, '\n'};
}

// The most bytes SK_TRIM_PE_COMBO_ALL writes to out[0] for a text of text_bytes bytes holding `records` complete records:
// a record's output is never longer than its four lines with their newlines, but for an N record, which is one byte
// longer than a 1-base read with an empty '+' line (name + 7 against name + 6); and the last record's last line may lack
// its '\n', which the output has.
FQR_FN uint64_t fqr_combo_all_bound(uint64_t text_bytes, uint64_t records) { return text_bytes + records + 1; }

#endif
