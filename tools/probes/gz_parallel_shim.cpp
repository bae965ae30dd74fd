// probe helper: host/GzParallel.cpp behind one C function, so that tools/probes/gunzip_rate.py can time the host decoder in
// its own process.  Built by the probe (g++ -O3 -shared), not part of the product.
#include <cstddef>
#include <cstdint>

#include "GzParallel.h"

// data[0, n): a gzip image.  The text goes to out[0, cap) -> its length, -1: the decoder failed, -2: cap is too small.
// *stretches_used: the decoder's own count.  Threads: SICKLE_HOST_THREADS, read when the pool is first used.
extern "C" long long skp_gz_parallel(const unsigned char *data, size_t n, char *out, size_t cap, unsigned long long *stretches_used)
{
    GzParallel z(data, n);
    size_t at = 0;
    while (!z.finished()) {
        if (at == cap) return -2;
        const size_t got = z.read(out + at, cap - at);
        if (z.error()) return -1;
        if (got == 0 && !z.finished()) return -1;
        at += got;
    }
    if (z.error()) return -1;
    if (stretches_used) *stretches_used = z.stretches_used;
    return (long long)at;
}
