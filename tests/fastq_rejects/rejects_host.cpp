// TEST INFRASTRUCTURE ONLY: the rule of sickle_amd/csrc/sk_fastq_rejects.h executed on the host in the shape the four
// kernels of sk_fastq_rejects.hip give it -- count per block of FQJ_BLOCK_READS reads with eight consecutive reads a lane,
// one scan over the blocks with the fit verdict, place into a table of (output offset, read), and a gather partitioned
// by output bytes: chunks of 256 lanes x 2 granules of 16 bytes, a window of 128 records with a binary search in it and
// one beyond it, every granule filled record by record through the piece table (one text span, one immediate) -- and
// checked against a naive copy.  Every record's text lies in a heap block of exactly its span's length, so that the
// address sanitizer sees any load beyond a span: the closing '\n' above all, which has no byte behind it.  A load here
// copies exactly the wanted bytes; that the device widens it to the aligned 16-byte blocks that hold them is no part
// of the rule.
// Batches: drawn ones, and the shapes the GPU test lists (read counts around a block, outputs of one chunk and a byte more
// or fewer, a record longer than a chunk, more records in a chunk than the window holds, record lengths that put the
// granule boundaries at every offset).
// `rejects_host` prints "ok <cases> chunk <bytes> window <records> block <reads>" and returns 0; `rejects_host --corrupt`
// forgets the mate in the selection on the walk's side and must return 1 (the comparison sees it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "sk_fastq_rejects.h"

namespace {

const uint32_t THREADS = 256, PER_THREAD = FQJ_BLOCK_READS / THREADS, GPL = 2, GCHUNK = THREADS * 16 * GPL, WIN = 128;
bool corrupt = false;

struct Read {
    std::unique_ptr<uint8_t[]> text; // exactly `bytes` bytes: the record's text
    uint64_t bytes, s0, e3;          // the descriptor's two words, as the text call wrote them (or did not)
    int32_t three;
};

struct Result {
    std::vector<uint8_t> text;
    std::vector<uint64_t> index;
    uint64_t records = 0, bytes = 0;
    bool written = false;
    bool operator==(const Result &o) const
    {
        return text == o.text && index == o.index && records == o.records && bytes == o.bytes && written == o.written;
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

// ---- the naive side: the rule as include/sickle_amd.h words it, nothing taken from sk_fastq_rejects.h --------------------
void naive(const std::vector<Read> &reads, bool pairs, uint64_t cap, bool index, uint64_t rec_cap, Result &r)
{
    std::vector<uint8_t> text;
    std::vector<uint64_t> idx;
    for (size_t k = 0; k < reads.size(); ++k) {
        bool chosen = reads[k].three < 0;
        if (pairs && (k ^ 1) < reads.size() && reads[k ^ 1].three < 0) chosen = true;
        if (!chosen) continue;
        const Read &rd = reads[k];
        const uint64_t s = std::min(rd.s0, rd.bytes), e = std::max(s, std::min(rd.e3, rd.bytes));
        for (uint64_t i = s; i < e; ++i) text.push_back(rd.text[i]);
        text.push_back('\n');
        idx.push_back(k);
    }
    r.records = idx.size();
    r.bytes = text.size();
    r.written = text.size() <= cap && (!index || idx.size() <= rec_cap);
    if (r.written) {
        r.text = text;
        if (index) r.index = idx;
    }
}

// ---- the walk: the kernels' shape --------------------------------------------------------------------------------------------
// fqj_lane_reads: the bytes of the record of each selected read of a lane, 0 for the others
void lane_reads(const std::vector<Read> &reads, uint64_t first, bool pairs, uint64_t *bytes)
{
    const uint64_t R = reads.size();
    bool is_read[PER_THREAD], kept[PER_THREAD];
    for (uint32_t j = 0; j < PER_THREAD; ++j) {
        is_read[j] = first + j < R;
        kept[j] = is_read[j] ? fqj_kept(reads[first + j].three) : true;
    }
    for (uint32_t j = 0; j < PER_THREAD; ++j) {
        bytes[j] = 0;
        const bool mate_kept = !is_read[j ^ 1] || kept[j ^ 1];
        if (is_read[j] && fqj_selected(kept[j], mate_kept, pairs && !corrupt)) {
            uint64_t at, len;
            fqj_span(reads[first + j].s0, reads[first + j].e3, reads[first + j].bytes, &at, &len);
            bytes[j] = fqj_record_bytes(len);
        }
    }
}

// bytes [rel, rel + n) of a record of `rec` bytes to out[0, n): the table of fqj_pieces
void fill(const Read &rd, uint64_t rec, uint64_t rel, uint32_t n, uint8_t *out)
{
    uint64_t at, len;
    fqj_span(rd.s0, rd.e3, rd.bytes, &at, &len);
    fqj_piece pc[2];
    fqj_pieces(at, rec - 1, pc);
    if (rel < pc[0].len) {
        const uint32_t t = (uint32_t)std::min<uint64_t>(n, pc[0].len - rel);
        const uint64_t p = pc[0].at + rel, room = rd.bytes - std::min(rd.bytes, p);
        if (t <= room) std::memcpy(out, rd.text.get() + p, t); // exactly the wanted bytes
        rel += t;
        out += t;
        n -= t;
    }
    if (n > 0 && rel == pc[0].len) *out = (uint8_t)pc[1].imm;
}

void walk(const std::vector<Read> &reads, bool pairs, uint64_t cap, bool index, uint64_t rec_cap, uint32_t grid, Result &r)
{
    const uint64_t R = reads.size(), n_blocks = (R + FQJ_BLOCK_READS - 1) / FQJ_BLOCK_READS + 1; // one block beyond the reads
    std::vector<uint64_t> blk(FQJ_BLOCK_WORDS * n_blocks, 0xdeadbeefull), tab(2 * (R + 1), ~0ull);
    // 1 count
    for (uint64_t b = 0; b < n_blocks; ++b) {
        uint64_t recs = 0, bytes = 0;
        if (b * FQJ_BLOCK_READS < R)
            for (uint32_t t = 0; t < THREADS; ++t) {
                uint64_t len[PER_THREAD];
                lane_reads(reads, b * FQJ_BLOCK_READS + t * PER_THREAD, pairs, len);
                for (uint32_t j = 0; j < PER_THREAD; ++j) {
                    recs += len[j] != 0;
                    bytes += len[j];
                }
            }
        blk[FQJ_BLOCK_WORDS * b] = recs;
        blk[FQJ_BLOCK_WORDS * b + 1] = bytes;
    }
    // 2 scan
    uint64_t run[2] = {0, 0};
    for (uint64_t b = 0; b < n_blocks; ++b)
        for (int i = 0; i < 2; ++i) {
            const uint64_t v = blk[FQJ_BLOCK_WORDS * b + i];
            blk[FQJ_BLOCK_WORDS * b + i] = run[i];
            run[i] += v;
        }
    r.records = run[0];
    r.bytes = run[1];
    r.written = fqj_fits(true, true, run[1], cap, index, run[0], rec_cap);
    if (!r.written) return;
    r.text.assign(run[1], 0xee);
    if (index) r.index.assign(run[0], ~0ull);
    // 3 place
    for (uint64_t b = 0; b < n_blocks && b * FQJ_BLOCK_READS < R; ++b) {
        uint64_t k = blk[FQJ_BLOCK_WORDS * b], at = blk[FQJ_BLOCK_WORDS * b + 1];
        for (uint32_t t = 0; t < THREADS; ++t) {
            const uint64_t first = b * FQJ_BLOCK_READS + t * PER_THREAD;
            uint64_t len[PER_THREAD];
            lane_reads(reads, first, pairs, len);
            for (uint32_t j = 0; j < PER_THREAD; ++j) {
                if (!len[j]) continue;
                tab[2 * k] = at;
                tab[2 * k + 1] = first + j;
                if (index) r.index[k] = first + j;
                ++k;
                at += len[j];
            }
        }
    }
    // 4 gather
    const uint64_t total = run[1], Rn = run[0];
    if (total == 0) return;
    auto off = [&](uint64_t k) { return k < Rn ? tab[2 * k] : total; };
    const uint64_t n_chunks = (total + GCHUNK - 1) / GCHUNK, per = (n_chunks + grid - 1) / grid;
    for (uint32_t wg = 0; wg < grid; ++wg) {
        const uint64_t c0 = wg * per, c1 = std::min(c0 + per, n_chunks);
        if (c0 >= c1) continue;
        uint64_t lo = 0, hi = Rn; // the last k < Rn with off(k) <= the chunk's first byte
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (off(mid) <= c0 * GCHUNK) lo = mid; else hi = mid;
        }
        uint64_t cur = lo;
        for (uint64_t c = c0; c < c1; ++c) {
            uint64_t s_off[WIN + 1];
            for (uint32_t t = 0; t <= WIN; ++t) s_off[t] = cur + t <= Rn ? off(cur + t) : ~0ull;
            uint64_t k_last = cur;
            for (uint32_t t = 0; t < THREADS; ++t)
                for (uint32_t u = 0; u < GPL; ++u) {
                    const uint64_t g = c * GCHUNK + (uint64_t)u * (THREADS * 16) + 16u * t;
                    if (g >= total) break;
                    uint64_t k;
                    if (g < s_off[WIN]) {
                        int l = 0, h = WIN;
                        while (h - l > 1) {
                            const int mid = (l + h) >> 1;
                            if (s_off[mid] <= g) l = mid; else h = mid;
                        }
                        k = cur + l;
                    } else {
                        uint64_t l = cur + WIN, h = Rn;
                        while (h - l > 1) {
                            const uint64_t mid = l + ((h - l) >> 1);
                            if (off(mid) <= g) l = mid; else h = mid;
                        }
                        k = l;
                    }
                    if (t == THREADS - 1) k_last = k; // the last lane's last granule
                    const uint64_t end = std::min(g + 16, total);
                    uint8_t acc[16] = {0};
                    uint64_t pos = g;
                    while (pos < end && k < Rn) {
                        const uint64_t i = k - cur;
                        const uint64_t b = i < WIN ? s_off[i] : off(k), e = i < WIN ? s_off[i + 1] : off(k + 1);
                        if (e <= pos) {
                            ++k;
                            continue;
                        }
                        const uint64_t pe = std::min(e, end);
                        fill(reads[tab[2 * k + 1]], e - b, pos - b, (uint32_t)(pe - pos), acc + (pos - g));
                        pos = pe;
                    }
                    std::memcpy(r.text.data() + g, acc, end - g); // the last granule stops at `bytes`
                }
            cur = std::min(k_last, Rn - 1);
        }
    }
}

// ---- batches -----------------------------------------------------------------------------------------------------------------
Read make(uint64_t len, bool kept)
{
    Read rd;
    rd.text.reset(new uint8_t[len ? len : 1]);
    for (uint64_t i = 0; i < len; ++i) rd.text[i] = (uint8_t)(33 + below(90));
    if (len) rd.text[0] = '@';
    rd.bytes = len;
    rd.s0 = 0;
    rd.e3 = len;
    rd.three = kept ? (int32_t)below(100) : -1;
    return rd;
}

int cases = 0;
bool check(const std::vector<Read> &reads, const char *what)
{
    uint64_t need = 0, recs = 0;
    {
        Result r;
        naive(reads, true, ~0ull, false, 0, r);
        need = r.bytes;
        recs = r.records;
    }
    for (int pairs = 0; pairs < 2; ++pairs)
        for (int v = 0; v < 4; ++v) {
            // all it needs; one byte short; an index; an index one record short
            const uint64_t cap = v == 1 && need ? need - 1 : need;
            const bool index = v >= 2;
            const uint64_t rec_cap = v == 3 && recs ? recs - 1 : recs;
            Result a, b;
            naive(reads, pairs != 0, cap, index, rec_cap, a);
            walk(reads, pairs != 0, cap, index, rec_cap, v == 0 ? 1 : 1 + (uint32_t)below(9), b);
            ++cases;
            if (!(a == b)) {
                std::fprintf(stderr, "%s: pairs %d variant %d: the walk and the naive copy differ (%llu / %llu bytes, %llu / %llu records)\n",
                             what, pairs, v, (unsigned long long)b.bytes, (unsigned long long)a.bytes,
                             (unsigned long long)b.records, (unsigned long long)a.records);
                return false;
            }
        }
    return true;
}

std::vector<Read> uniform(uint64_t n, uint64_t len, int pattern)
{
    // pattern 0: none rejected, 1: all, 2: exactly the first, 3: exactly the last
    std::vector<Read> reads;
    for (uint64_t k = 0; k < n; ++k)
        reads.push_back(make(len, !(pattern == 1 || (pattern == 2 && k == 0) || (pattern == 3 && k + 1 == n))));
    return reads;
}

} // namespace

int main(int argc, char **argv)
{
    corrupt = argc > 1 && std::strcmp(argv[1], "--corrupt") == 0;
    bool ok = true;
    // drawn batches: lengths from a byte to beyond a chunk, a third of the reads rejected
    for (int it = 0; it < 60 && ok; ++it) {
        std::vector<Read> reads;
        const uint64_t n = 1 + below(it < 50 ? 400 : 5000);
        const uint64_t top = it % 10 == 0 ? 3 * GCHUNK : (it % 3 == 0 ? 40 : 400);
        for (uint64_t k = 0; k < n; ++k) reads.push_back(make(below(20) == 0 ? below(top) : below(std::min<uint64_t>(top, 400)), below(3) != 0));
        // descriptors that are no descriptors: a start or an end beyond the text, an end before the start
        if (it % 7 == 0)
            for (int j = 0; j < 5; ++j) {
                Read &rd = reads[below(n)];
                rd.s0 = below(2 * rd.bytes + 2);
                rd.e3 = below(2 * rd.bytes + 2);
            }
        ok = check(reads, "drawn");
    }
    // the read counts around a block, with none, all, the first and the last rejected
    const uint64_t counts[] = {1, 2, 2047, 2048, 2049, 4097};
    for (uint64_t n : counts)
        for (int pattern = 0; pattern < 4 && ok; ++pattern) ok = check(uniform(n, 30, pattern), "counts");
    // record lengths that put the output's granule boundaries at every offset
    for (uint64_t len = 0; len < 34 && ok; ++len) ok = check(uniform(70, len, 1), "granules");
    // an output of exactly one chunk, and of one byte more and one fewer: 128 records of 64 bytes, the last one varied
    for (int d = -1; d <= 1 && ok; ++d) {
        std::vector<Read> reads = uniform(GCHUNK / 64, 63, 1);
        reads.back() = make(63 + d, false);
        ok = check(reads, "one chunk");
    }
    // a record longer than a chunk, among short ones
    if (ok) {
        std::vector<Read> reads = uniform(10, 30, 1);
        reads[4] = make(70000, false);
        reads[7] = make(2 * 20000 + 40, false);
        ok = check(reads, "long records");
    }
    // more rejected records overlapping one chunk than the window holds
    if (ok) ok = check(uniform(9001, 7, 1), "beyond the window");
    if (!ok) return 1;
    std::printf("ok %d chunk %u window %u block %u\n", cases, GCHUNK, WIN, FQJ_BLOCK_READS);
    return 0;
}
