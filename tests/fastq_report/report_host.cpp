// TEST INFRASTRUCTURE ONLY: the report rule of sickle_amd/csrc/sk_fastq_report.h executed on the host in the shape the
// two kernels of sk_fastq_report.hip give it -- blocks of 2 048 reads whose lanes own 8 consecutive reads, and chunks of
// FQP_CHUNK_BYTES of packed qual walked in steps of 256 lanes x 16 bytes, each lane's granule against the read bounds, the
// last position bin summed apart -- and checked against a second, naive computation, read by read and byte by byte.
// Batches: drawn ones, and the shapes the GPU test lists (block edges, granule edges, 1-base reads, a read longer than a
// chunk, a read that straddles a chunk boundary with its two cuts on either side, every bin limit).
// `report_host` prints "ok <cases>" and returns 0; `report_host --corrupt` leaves the last bin's register sum out of the
// walk and must return 1 (the comparison sees it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "sk_fastq_report.h"

namespace {

const uint32_t BLOCK_READS = 2048, THREADS = 256, PER_THREAD = BLOCK_READS / THREADS, STEP = THREADS * 16;

struct Batch {
    int64_t mode;
    std::vector<uint64_t> off; // reads + 1
    std::vector<int32_t> five, three;
    std::vector<uint8_t> qual;
    uint64_t reads() const { return off.size() - 1; }
};

struct Report {
    uint64_t w[FQP_WORDS];
    std::vector<uint64_t> len_in, len_out, qsum_in, qcnt_in, qsum_out, qcnt_out;
    Report(uint64_t lb, uint64_t pb) : len_in(lb), len_out(lb), qsum_in(pb), qcnt_in(pb), qsum_out(pb), qcnt_out(pb)
    {
        std::memset(w, 0, sizeof w);
    }
    bool operator==(const Report &o) const
    {
        return std::memcmp(w, o.w, sizeof w) == 0 && len_in == o.len_in && len_out == o.len_out && qsum_in == o.qsum_in &&
               qcnt_in == o.qcnt_in && qsum_out == o.qsum_out && qcnt_out == o.qcnt_out;
    }
};

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
uint64_t below(uint64_t n) { return rnd() % n; }

// the naive side: the rule as include/sickle_amd.h words it, nothing taken from sk_fastq_report.h
Report naive(const Batch &b, uint64_t lb, uint64_t pb)
{
    Report r(lb, pb);
    r.w[0] = 1; // calls
    uint64_t *reads = r.w + 2, *kept = r.w + 3, *discarded = r.w + 4, *pairs = r.w + 5, *bases_in = r.w + 9, *bases_out = r.w + 10,
             *cut5 = r.w + 11, *cut3 = r.w + 12, *bases_disc = r.w + 13, *reads5 = r.w + 14, *reads3 = r.w + 15, *max_in = r.w + 16,
             *max_out = r.w + 17;
    for (uint64_t i = 0; i < b.reads(); ++i) {
        const uint64_t len = b.off[i + 1] - b.off[i];
        const bool k = b.three[i] >= 0;
        ++*reads;
        *bases_in += len;
        *max_in = std::max(*max_in, len);
        if (lb) ++r.len_in[std::min(len, lb - 1)];
        for (uint64_t p = 0; p < len && pb; ++p) {
            r.qsum_in[std::min(p, pb - 1)] += b.qual[b.off[i] + p];
            ++r.qcnt_in[std::min(p, pb - 1)];
        }
        if (!k) {
            ++*discarded;
            *bases_disc += len;
            continue;
        }
        const uint64_t f = (uint64_t)b.five[i], t = (uint64_t)b.three[i];
        ++*kept;
        *bases_out += t - f;
        *cut5 += f;
        *cut3 += len - t;
        *reads5 += f != 0;
        *reads3 += t != len;
        *max_out = std::max(*max_out, t - f);
        if (lb) ++r.len_out[std::min(t - f, lb - 1)];
        for (uint64_t p = f; p < t && pb; ++p) {
            r.qsum_out[std::min(p - f, pb - 1)] += b.qual[b.off[i] + p];
            ++r.qcnt_out[std::min(p - f, pb - 1)];
        }
    }
    if (b.mode != SK_TRIM_SE)
        for (uint64_t k = 0; 2 * k + 1 < b.reads(); ++k) ++pairs[(b.three[2 * k] >= 0 ? 1 : 0) | (b.three[2 * k + 1] >= 0 ? 2 : 0)];
    return r;
}

// the kernels' side: sk_fastq_report.h's functions, block after block, lane after lane
bool kernel_shape(const Batch &b, uint64_t lb, uint64_t pb, bool corrupt, Report &r)
{
    const uint64_t n_real = b.reads();
    r.w[FQP_W_CALLS] = 1;
    for (uint64_t blk = 0; blk * BLOCK_READS < n_real; ++blk) {
        std::vector<uint32_t> s_len(2 * lb, 0);
        uint64_t tot[FQP_WORDS] = {0};
        for (uint32_t t = 0; t < THREADS; ++t) {
            const uint64_t first = blk * BLOCK_READS + (uint64_t)t * PER_THREAD;
            uint64_t w[FQP_WORDS] = {0}, max_in = 0, max_out = 0;
            int32_t three_even = -1;
            for (uint32_t j = 0; j < PER_THREAD && first + j < n_real; ++j) {
                const uint64_t i = first + j, len = b.off[i + 1] - b.off[i];
                fqp_add_read(len, b.five[i], b.three[i], w, &max_in, &max_out);
                if (lb) {
                    ++s_len[fqp_bin(len, lb)];
                    if (fqp_kept(b.three[i])) ++s_len[lb + fqp_bin((uint64_t)(b.three[i] - b.five[i]), lb)];
                }
                if ((j & 1) == 0) three_even = b.three[i];
                else if (fqp_pair_at(b.mode, i - 1, n_real)) fqp_add_pair(three_even, b.three[i], w);
            }
            for (int k = 0; k < FQP_SUM_WORDS; ++k) tot[k] += w[k];
            tot[FQP_W_MAX_LEN_IN] = std::max(tot[FQP_W_MAX_LEN_IN], max_in);
            tot[FQP_W_MAX_LEN_OUT] = std::max(tot[FQP_W_MAX_LEN_OUT], max_out);
        }
        for (int k = 0; k < FQP_SUM_WORDS; ++k) r.w[k] += tot[k];
        for (int k = FQP_SUM_WORDS; k < FQP_WORDS; ++k) r.w[k] = std::max(r.w[k], tot[k]);
        for (uint64_t i = 0; i < lb; ++i) {
            r.len_in[i] += s_len[i];
            r.len_out[i] += s_len[lb + i];
        }
    }
    if (!pb || !n_real) return true;
    const uint64_t total = b.off[n_real], last = pb - 1;
    for (uint64_t c0 = 0; c0 < total; c0 += FQP_CHUNK_BYTES) {
        const uint64_t c1 = std::min(c0 + FQP_CHUNK_BYTES, total);
        std::vector<uint64_t> s_in(fqp_slots((uint32_t)pb), 0), s_out(fqp_slots((uint32_t)pb), 0), tail_in(THREADS, 0), tail_out(THREADS, 0);
        auto slot = [&](uint64_t p) { return (size_t)fqp_slot((uint32_t)p); }; // .at() below: a slot outside the table throws
        for (uint64_t s0 = c0; s0 < c1; s0 += STEP)
            for (uint32_t t = 0; t < THREADS; ++t) {
                const uint64_t g = s0 + 16ull * t;
                if (g >= c1) break;
                // the last read that starts at or before g
                uint64_t k = (uint64_t)(std::upper_bound(b.off.begin(), b.off.begin() + n_real, g) - b.off.begin()) - 1;
                const int n = (int)std::min<uint64_t>(16, c1 - g);
                for (int i = 0; i < n; ++i) {
                    const uint64_t at = g + i;
                    while (at >= b.off[k + 1]) ++k;
                    if (k >= n_real) return false;
                    const uint64_t p = at - b.off[k], x = fqp_qword(b.qual[at]);
                    if (p >= last) tail_in[t] += x;
                    else s_in.at(slot(p)) += x;
                    if (fqp_out_byte(p, b.five[k], b.three[k])) {
                        const uint64_t po = p - (uint64_t)b.five[k];
                        if (po >= last) tail_out[t] += x;
                        else s_out.at(slot(po)) += x;
                    }
                }
            }
        for (uint32_t t = 0; t < THREADS && !corrupt; ++t) {
            s_in.at(slot(last)) += tail_in[t];
            s_out.at(slot(last)) += tail_out[t];
        }
        for (uint64_t i = 0; i < pb; ++i) {
            // the halves: a chunk's sum of bytes stays below 2^32, so the low half never reached the count
            const uint64_t x = s_in.at(slot(i)), y = s_out.at(slot(i));
            if ((x & 0xffffffffull) > 255ull * (x >> 32) || (y & 0xffffffffull) > 255ull * (y >> 32)) return false;
            r.qsum_in[i] += x & 0xffffffffull;
            r.qcnt_in[i] += x >> 32;
            r.qsum_out[i] += y & 0xffffffffull;
            r.qcnt_out[i] += y >> 32;
        }
    }
    return true;
}

// lens: the reads' lengths; keep: 0 none kept, 1 all kept (whole), 2 drawn cuts
Batch make(int64_t mode, const std::vector<uint64_t> &lens, int keep)
{
    Batch b;
    b.mode = mode;
    b.off.push_back(0);
    for (uint64_t len : lens) {
        b.off.push_back(b.off.back() + len);
        int32_t f = -1, t = -1;
        if (keep == 1) {
            f = 0;
            t = (int32_t)len;
        } else if (keep == 2 && below(4) != 0) {
            f = (int32_t)below(len + 1);
            t = f + (int32_t)below(len - f + 1);
            if (below(3) == 0) f = 0;
            if (below(3) == 0) t = (int32_t)len;
        }
        b.five.push_back(f);
        b.three.push_back(t);
    }
    b.qual.resize(b.off.back());
    for (auto &q : b.qual) q = (uint8_t)(below(8) == 0 ? 255 : 33 + below(42));
    return b;
}

int failures = 0, cases = 0;

void check(const Batch &b, uint64_t lb, uint64_t pb, bool corrupt, const char *what)
{
    ++cases;
    const Report want = naive(b, lb, pb);
    Report got(lb, pb);
    if (!kernel_shape(b, lb, pb, corrupt, got) || !(got == want)) {
        ++failures;
        std::fprintf(stderr, "differs: %s (mode %lld, %llu reads, len_bins %llu, pos_bins %llu)\n", what, (long long)b.mode,
                     (unsigned long long)b.reads(), (unsigned long long)lb, (unsigned long long)pb);
    }
}

} // namespace

int main(int argc, char **argv)
{
    const bool corrupt = argc > 1 && std::strcmp(argv[1], "--corrupt") == 0;
    const int64_t modes[3] = {SK_TRIM_SE, SK_TRIM_PE_SPLIT, SK_TRIM_PE_INTERLEAVED};
    // read counts at a block's edge and over several blocks: every read kept, then none, then drawn
    for (uint64_t n : {1ull, 2ull, 2047ull, 2048ull, 2049ull, 3ull * 2048 + 1})
        for (int keep = 0; keep < 3; ++keep)
            for (int64_t mode : modes) {
                if (mode != SK_TRIM_SE && (n & 1)) continue; // the pair framings hold whole pairs
                std::vector<uint64_t> lens(n);
                for (auto &l : lens) l = 1 + below(40);
                check(make(mode, lens, keep), 48, 48, corrupt, "read counts");
            }
    // the granule's edges
    for (uint64_t len : {1ull, 15ull, 16ull, 17ull, 31ull, 32ull, 33ull})
        for (int keep = 1; keep < 3; ++keep) {
            check(make(SK_TRIM_SE, std::vector<uint64_t>(300, len), keep), len + 1, len + 1, corrupt, "granule edges");
            check(make(SK_TRIM_PE_INTERLEAVED, std::vector<uint64_t>(300, len), keep), len, len, corrupt, "granule edges, exact bins");
        }
    // 1-base reads only: thousands of reads in a step
    check(make(SK_TRIM_SE, std::vector<uint64_t>(3 * STEP + 5, 1), 2), 4, 4, corrupt, "1-base reads");
    // one read longer than a chunk among short ones
    {
        std::vector<uint64_t> lens(40, 20);
        lens[17] = FQP_CHUNK_BYTES + 1000;
        for (uint64_t pb : {1ull, 2ull, 64ull, (unsigned long long)SK_FQ_REPORT_MAX_POS_BINS})
            check(make(SK_TRIM_PE_SPLIT, lens, 2), 64, pb, corrupt, "a read longer than a chunk");
    }
    // a read that straddles a chunk boundary, five on one side and three on the other
    {
        std::vector<uint64_t> lens;
        uint64_t at = 0;
        while (at + 150 < FQP_CHUNK_BYTES - 40) {
            lens.push_back(150);
            at += 150;
        }
        lens.push_back(100); // starts below the boundary, ends above it
        const uint64_t straddler = lens.size() - 1, before = FQP_CHUNK_BYTES - at;
        lens.push_back(150);
        Batch b = make(SK_TRIM_SE, lens, 1);
        b.five[straddler] = (int32_t)(before - 3);
        b.three[straddler] = (int32_t)(before + 5);
        check(b, 256, 256, corrupt, "a read across a chunk boundary");
        check(b, 256, 7, corrupt, "a read across a chunk boundary, a small last bin");
    }
    // the bin limits: 1, 2, the exact longest length, that + 1, the limits
    {
        std::vector<uint64_t> lens(500);
        for (auto &l : lens) l = 1 + below(90);
        lens[3] = 90;
        const Batch b = make(SK_TRIM_PE_INTERLEAVED, lens, 2);
        for (uint64_t bins : {1ull, 2ull, 90ull, 91ull}) check(b, bins, bins, corrupt, "bin limits");
        check(b, SK_FQ_REPORT_MAX_LEN_BINS, SK_FQ_REPORT_MAX_POS_BINS, corrupt, "the largest tables");
        check(b, 0, 16, corrupt, "no length arrays");
        check(b, 16, 0, corrupt, "no position arrays");
    }
    // drawn batches
    for (int it = 0; it < 60; ++it) {
        const int64_t mode = modes[below(3)];
        uint64_t n = 1 + below(it % 10 == 0 ? 6000 : 400);
        if (mode != SK_TRIM_SE) n += n & 1;
        std::vector<uint64_t> lens(n);
        const uint64_t top = below(4) == 0 ? 3000 : 160;
        for (auto &l : lens) l = 1 + below(top);
        check(make(mode, lens, 2), 1 + below(300), 1 + below(300), corrupt, "drawn");
    }
    if (failures) {
        std::fprintf(stderr, "%d of %d cases differ\n", failures, cases);
        return 1;
    }
    std::printf("ok %d\n", cases);
    return 0;
}
