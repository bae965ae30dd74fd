// sk_fastq_words.h -- the words of the header of a FASTQ text call's workspace (sk_device.h describes the workspace).  No
// HIP: sk_device.h includes it for the kernels, sk_fastq_verdict.h for the host.
#ifndef SK_FASTQ_WORDS_H
#define SK_FASTQ_WORDS_H

#define SK_FQ_HDR_WORDS 32u
#define SK_FQ_H_LINES 0        // [2] lines of each input
#define SK_FQ_H_RECORDS 2      // [2] complete records of each input
#define SK_FQ_H_FMT 4          // (read << 3) | SK_FQ_* of the lowest malformed record, or ~0
#define SK_FQ_H_NREAL 5        // reads of the packed batch that are records (the rest are empty)
#define SK_FQ_H_PACKED 6       // bytes of the packed qual (and seq)
#define SK_FQ_H_OUT_RECORDS 7  // [3]
#define SK_FQ_H_OUT_BYTES 10   // [3]
#define SK_FQ_H_FIT 13         // [3] produced, no error, within its capacities: the emission writes it
#define SK_FQ_H_PRODUCED 16    // [3] out[o].text != NULL for an output of the mode
#define SK_FQ_H_RANGE 19       // the stream's range-error word as the emission saw it
#define SK_FQ_H_MODE 20        // the call's framing mode (SK_TRIM_PE_INTERLEAVED for SK_TRIM_PE_COMBO_ALL)
// Piece calls (sk_trim_fastq_piece_device_async with piece != NULL) use words 21..29, which are otherwise the ordered
// calls' (sk_fastq_order.h); an ordered piece keeps these here and its order words in an extension block (sk_device.h).
#define SK_FQP_H_START 21      // [2] s_i: the window's first byte, offset in text[i]
#define SK_FQP_H_END 23        // [2] n_i: the window's end (sk_trim_fastq_piece_words' end)
#define SK_FQP_H_CONSUMED 25   // [2] offset in text[i] of the first byte the piece did not consume
#define SK_FQP_H_OK 27         // 1 iff no format error, the range-error word clear at both looks, every produced output fitted
#define SK_FQP_H_RANGE0 28     // the stream's range-error word as the frame scan saw it, before the piece's own scan
#define SK_FQP_H_MORE 29       // the piece's `more`

#endif
