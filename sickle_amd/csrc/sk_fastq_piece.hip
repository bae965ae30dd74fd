// sk_fastq_piece.hip -- the carry between two pieces of a FASTQ stream (sk_fastq_carry_device_async): what the previous
// piece (sk_trim_fastq_piece_device_async with more != 0) did not consume, prev_text[consumed, end), goes in front of the
// next chunk of text, to next_text[room - c, room), and the words the next piece takes its window from are written.
//
// One launch of one kernel.  Every workgroup derives the status from the same device words (a handful of scalar loads);
// lane 0 of workgroup 0 writes `words`.  The copy is destination-partitioned: one aligned 16-byte granule of next_text per
// lane and step, its source bytes read with one 16-byte load at any alignment (exactly the 16 wanted bytes, so no byte
// outside [consumed, end) is read), stored with one 16-byte store; the head and the tail granule, which hold bytes outside
// [room - c, room), are copied byte by byte.  The carry is a few records, so this is not a hot kernel: for gfx950 it
// compiles to global_load_dwordx4 / global_store_dwordx4 in the loop and global_load_ubyte / global_store_byte for the two
// partial granules, 0 bytes of scratch, no LDS.
#include <hip/hip_runtime.h>

#include "sk_device.h"

namespace {

typedef unsigned fqc_u4 __attribute__((ext_vector_type(4)));
struct __attribute__((packed, aligned(1))) fqc_u4_any {
    fqc_u4 v;
};

#define FQC_THREADS 256
#define FQC_MAX_BLOCKS 1024u

struct fqc_args {
    const uint64_t *prev_hdr; // the previous piece's header, or NULL: the first piece
    const uint8_t *prev_text;
    uint8_t *next_text;
    uint64_t room;
    const uint64_t *chunk_bytes_dev, *chunk_valid_dev;
    uint64_t chunk_bytes;
    const sk_fastq_carry_words *prev_words, *other_prev_words;
    sk_fastq_carry_words *words;
    int32_t input;
};

__global__ void __launch_bounds__(FQC_THREADS) sk_fq_carry_kernel(fqc_args a)
{
    uint64_t consumed = 0, c = 0, status = 0;
    bool ok = true;
    if (a.prev_hdr) {
        consumed = a.prev_hdr[SK_FQP_H_CONSUMED + a.input];
        const uint64_t end = a.prev_hdr[SK_FQP_H_END + a.input];
        c = end > consumed ? end - consumed : 0;
        ok = a.prev_hdr[SK_FQP_H_OK] != 0;
    }
    if (a.prev_words && a.prev_words->status) status = a.prev_words->status;
    else if (a.other_prev_words && a.other_prev_words->status) status = a.other_prev_words->status;
    else if (!ok) status = 1;
    else if (c > a.room) status = 2;
    else if (a.chunk_valid_dev && *a.chunk_valid_dev == 0) status = 3;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint64_t chunk = a.chunk_bytes;
        if (a.chunk_bytes_dev) chunk = min(chunk, *a.chunk_bytes_dev);
        sk_fastq_carry_words w;
        if (status) w = {a.room, a.room, 0, status};
        else w = {a.room - c, a.room + chunk, 1, 0};
        *a.words = w;
    }
    if (status || c == 0) return;
    // destination bytes [d0, d1) of next_text, in aligned 16-byte granules from the one that holds d0
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(a.next_text) + (a.room - c), d1 = d0 + c;
    const uintptr_t g0 = d0 & ~(uintptr_t)15;
    const uint64_t n_gran = (d1 - g0 + 15) / 16;
    const uint8_t *src = a.prev_text + consumed; // the byte that goes to d0
    for (uint64_t g = (uint64_t)blockIdx.x * FQC_THREADS + threadIdx.x; g < n_gran; g += (uint64_t)gridDim.x * FQC_THREADS) {
        const uintptr_t lo = g0 + 16 * g, hi = lo + 16;
        if (lo >= d0 && hi <= d1) {
            const fqc_u4 v = reinterpret_cast<const fqc_u4_any *>(src + (lo - d0))->v;
            *reinterpret_cast<fqc_u4 *>(lo) = v;
        } else {
            const uintptr_t b0 = lo < d0 ? d0 : lo, b1 = hi > d1 ? d1 : hi;
            for (uintptr_t b = b0; b < b1; ++b) *reinterpret_cast<uint8_t *>(b) = src[b - d0];
        }
    }
}

} // namespace

extern "C" __attribute__((visibility("hidden"))) hipError_t sk_launch_fastq_carry(const uint64_t *prev_hdr, int input,
                                                                                  const uint8_t *prev_text, uint8_t *next_text,
                                                                                  uint64_t room, const uint64_t *chunk_bytes_dev,
                                                                                  uint64_t chunk_bytes,
                                                                                  const uint64_t *chunk_valid_dev,
                                                                                  const sk_fastq_carry_words *prev_words,
                                                                                  const sk_fastq_carry_words *other_prev_words,
                                                                                  sk_fastq_carry_words *words, hipStream_t stream)
{
    fqc_args a;
    a.prev_hdr = prev_hdr;
    a.prev_text = prev_text;
    a.next_text = next_text;
    a.room = room;
    a.chunk_bytes_dev = chunk_bytes_dev;
    a.chunk_valid_dev = chunk_valid_dev;
    a.chunk_bytes = chunk_bytes;
    a.prev_words = prev_words;
    a.other_prev_words = other_prev_words;
    a.words = words;
    a.input = input;
    // sized by room, the most the carry can be: a granule per lane, FQC_MAX_BLOCKS workgroups at most (then lanes stride)
    const uint64_t gran = room / 16 + 2, blocks = (gran + FQC_THREADS - 1) / FQC_THREADS;
    hipLaunchKernelGGL(sk_fq_carry_kernel, dim3((unsigned)(blocks < FQC_MAX_BLOCKS ? blocks : FQC_MAX_BLOCKS)), dim3(FQC_THREADS), 0,
                       stream, a);
    return hipGetLastError();
}
