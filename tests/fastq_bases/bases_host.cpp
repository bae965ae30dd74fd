// TEST INFRASTRUCTURE ONLY: the rule of sickle_amd/csrc/sk_fastq_bases.h executed on the host in the shape the kernel of
// sk_fastq_bases.hip gives it -- chunks of packed positions walked in steps of 256 lanes x 16 positions, a lane's granule
// cut into one segment per read, sixteen bytes loaded with fqb_load16 and classified with fqb_segment, sums from
// popcounts, the position bins below the last added one byte at a time with the two counts in one word, a read that lanes
// share summed in a pair of words numbered by the lane it starts in or in a carry slot, the owner of a read's first byte
// walking the rest of it beyond its chunk -- and checked against a second, naive computation, byte by byte.  Every seq
// line lies in a heap block of exactly its length, so that the address sanitizer sees a load beyond a line.
// Batches: drawn ones at small chunks, and the shapes the GPU test lists at the header's chunk (a read of chunk + 1 000
// bases among 20-base ones, a 200-base read across the chunk boundary with its N on either side, read lengths around the
// granule, 9 001 one-base reads).
// `bases_host` prints "ok <cases> chunk <FQB_CHUNK_BYTES>" and returns 0; `bases_host --corrupt` stops folding lower case
// into the classes on the walk's side and must return 1 (the comparison sees it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "sk_fastq_bases.h"
#include "sk_fastq_report.h"

namespace {

const uint32_t THREADS = 256, STEP = THREADS * 16, CARRY = THREADS;
bool corrupt = false;

struct Read {
    std::unique_ptr<uint8_t[]> seq; // exactly len bytes
    uint64_t len;
    int32_t five, three;
};

struct Result {
    uint64_t w[FQB_WORDS];
    std::vector<uint64_t> pos_in, pos_out, gc_in, gc_out;
    explicit Result(uint32_t bins) : pos_in(6 * bins), pos_out(6 * bins), gc_in(SK_FQ_BASES_GC_BINS), gc_out(SK_FQ_BASES_GC_BINS)
    {
        std::memset(w, 0, sizeof w);
    }
    bool operator==(const Result &o) const
    {
        return std::memcmp(w, o.w, sizeof w) == 0 && pos_in == o.pos_in && pos_out == o.pos_out && gc_in == o.gc_in && gc_out == o.gc_out;
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

// ---- the naive side: the rule as include/sickle_amd.h words it, nothing taken from sk_fastq_bases.h ----------------------
int naive_class(uint8_t b)
{
    const char *letters = "AaCcGgTtNn";
    for (int i = 0; i < 10; ++i)
        if (b == (uint8_t)letters[i]) return i / 2;
    return 5;
}

void naive_line(const uint8_t *p, uint64_t n, uint32_t bins, uint64_t *classes, uint64_t *lower, uint64_t *reads_n, uint64_t *none,
                std::vector<uint64_t> &pos, std::vector<uint64_t> &gc)
{
    uint64_t cnt[6] = {0, 0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < n; ++i) {
        const int c = naive_class(p[i]);
        ++cnt[c];
        ++classes[c];
        if (p[i] >= 'a' && p[i] <= 'z') ++*lower;
        ++pos[(uint64_t)c * bins + std::min<uint64_t>(i, bins - 1)];
    }
    if (cnt[4]) ++*reads_n;
    const uint64_t acgt = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    if (acgt) ++gc[100 * (cnt[1] + cnt[2]) / acgt];
    else ++*none;
}

void naive(const std::vector<Read> &reads, uint32_t bins, Result &r)
{
    r.w[FQB_W_CALLS] += 1;
    for (const Read &rd : reads) {
        r.w[FQB_W_READS] += 1;
        naive_line(rd.seq.get(), rd.len, bins, r.w + FQB_W_BASES_IN, r.w + FQB_W_LOWER_IN, r.w + FQB_W_READS_N_IN,
                   r.w + FQB_W_GC_NONE_IN, r.pos_in, r.gc_in);
        if (rd.three < 0) continue;
        r.w[FQB_W_KEPT] += 1;
        naive_line(rd.seq.get() + rd.five, (uint64_t)(rd.three - rd.five), bins, r.w + FQB_W_BASES_OUT, r.w + FQB_W_LOWER_OUT,
                   r.w + FQB_W_READS_N_OUT, r.w + FQB_W_GC_NONE_OUT, r.pos_out, r.gc_out);
    }
}

// ---- the walk: the kernel's shape ------------------------------------------------------------------------------------------
void load(const Read &rd, uint64_t at, uint64_t *w)
{
    fqb_load16(rd.seq.get(), rd.len, at, w);
    if (corrupt)
        for (int j = 0; j < 16; ++j) {
            const uint8_t b = (uint8_t)(w[j >> 3] >> (8 * (j & 7)));
            if (b >= 'a' && b <= 'z') w[j >> 3] ^= (uint64_t)(b ^ '.') << (8 * (j & 7)); // lower case is not folded
        }
}

void finish(uint64_t wi, uint64_t wo, bool kept, Result &r)
{
    r.w[FQB_W_READS] += 1;
    r.w[FQB_W_READS_N_IN] += fqb_has_n(wi);
    const int32_t bi = fqb_gc_bin(wi);
    if (bi < 0) r.w[FQB_W_GC_NONE_IN] += 1;
    else r.gc_in[bi] += 1;
    if (!kept) return;
    r.w[FQB_W_KEPT] += 1;
    r.w[FQB_W_READS_N_OUT] += fqb_has_n(wo);
    const int32_t bo = fqb_gc_bin(wo);
    if (bo < 0) r.w[FQB_W_GC_NONE_OUT] += 1;
    else r.gc_out[bo] += 1;
}

void walk_chunk(const std::vector<Read> &reads, const std::vector<uint64_t> &off, uint64_t c0, uint64_t c1, uint32_t bins, Result &r)
{
    const uint64_t R = reads.size(), total = off[R];
    const uint32_t last = bins - 1, PS = fqp_slots(bins);
    std::vector<uint64_t> tab(6 * PS, 0), tail_in(6, 0), tail_out(6, 0);
    uint64_t rd_words[2][THREADS + 2];
    std::memset(rd_words, 0, sizeof rd_words);
    uint64_t cur = (uint64_t)(std::upper_bound(off.begin(), off.begin() + R, c0) - off.begin()) - 1;
    uint64_t tail = ~0ull;
    uint32_t step = 0;
    for (uint64_t s0 = c0; s0 < c1; s0 += STEP, ++step) {
        const uint64_t s1 = std::min<uint64_t>(s0 + STEP, c1);
        const uint32_t carry_in = CARRY + (step & 1), carry_out = CARRY + ((step + 1) & 1);
        tail = ~0ull;
        struct Settle {
            bool mine = false, mine_kept = false, came = false, came_kept = false;
            uint64_t mine_e = 0, mine_k = 0, came_b = 0, came_e = 0, came_k = 0;
        };
        std::vector<Settle> settle(THREADS);
        uint64_t k_last = cur;
        for (uint32_t t = 0; t < THREADS; ++t) {
            const uint64_t g = s0 + 16u * t;
            if (g >= s1) continue;
            uint64_t k = (uint64_t)(std::upper_bound(off.begin() + cur, off.begin() + R, g) - off.begin()) - 1;
            const uint64_t g1 = std::min<uint64_t>(g + 16, s1);
            uint64_t at = g;
            Settle &st = settle[t];
            while (at < g1) {
                while (at >= off[k + 1] && k + 1 < R) ++k;
                const uint64_t b = off[k], e = off[k + 1];
                if (at >= e || at < b) break;
                const Read &rd = reads[k];
                const uint64_t z = std::min(e, g1), p0 = at - b;
                const uint32_t n = (uint32_t)(z - at), all = fqb_range16(0, n);
                const bool kept = fqp_kept(rd.three);
                uint64_t w[2];
                load(rd, p0, w);
                fqb_seg sg;
                fqb_segment(w, n, p0, rd.five, rd.three, &sg);
                for (int cl = 0; cl < FQB_CLASSES; ++cl) {
                    r.w[FQB_W_BASES_IN + cl] += __builtin_popcount(sg.m[cl]);
                    r.w[FQB_W_BASES_OUT + cl] += __builtin_popcount(sg.m[cl] & sg.out);
                }
                r.w[FQB_W_LOWER_IN] += __builtin_popcount(sg.lower);
                r.w[FQB_W_LOWER_OUT] += __builtin_popcount(sg.lower & sg.out);
                const uint32_t far_in = fqb_range16((int64_t)last - (int64_t)p0, 16) & all;
                const uint32_t far_out = fqb_range16((int64_t)last + (int64_t)rd.five - (int64_t)p0, 16) & sg.out;
                for (int cl = 0; cl < FQB_CLASSES; ++cl) {
                    tail_in[cl] += __builtin_popcount(sg.m[cl] & far_in);
                    tail_out[cl] += __builtin_popcount(sg.m[cl] & far_out);
                }
                const uint32_t near_in = all & ~far_in, near_out = sg.out & ~far_out;
                for (uint32_t j = 0; j < 16; ++j) {
                    const uint32_t bit = 1u << j;
                    if (!((near_in | near_out) & bit)) continue;
                    uint64_t *row = tab.data() + fqb_code_at(&sg, j) * PS;
                    const uint32_t p = (uint32_t)p0 + j;
                    const bool in = near_in & bit, out = near_out & bit;
                    if (in && out && rd.five == 0) {
                        row[fqp_slot(p)] += (1ull << 32) | 1ull;
                    } else {
                        if (in) row[fqp_slot(p)] += 1;
                        if (out) row[fqp_slot(p - (uint32_t)rd.five)] += 1ull << 32;
                    }
                }
                const uint64_t wi = fqb_read_part(&sg, all), wo = fqb_read_part(&sg, sg.out);
                if (at == b && z == e) {
                    finish(wi, wo, kept, r);
                } else {
                    const uint32_t slot = b < s0 ? carry_in : (uint32_t)((b - s0) >> 4);
                    rd_words[0][slot] = fqb_read_add(rd_words[0][slot], wi);
                    rd_words[1][slot] = fqb_read_add(rd_words[1][slot], wo);
                    if (at == b) {
                        st.mine = true;
                        st.mine_kept = kept;
                        st.mine_e = e;
                        st.mine_k = k;
                    } else if (t == 0 && b < s0) {
                        st.came = true;
                        st.came_kept = kept;
                        st.came_b = b;
                        st.came_e = e;
                        st.came_k = k;
                    }
                }
                at = z;
            }
            k_last = k;
        }
        for (uint32_t t = 0; t < THREADS; ++t) { // behind the barrier
            const Settle &st = settle[t];
            if (st.came) {
                const uint64_t wi = rd_words[0][carry_in], wo = rd_words[1][carry_in];
                rd_words[0][carry_in] = rd_words[1][carry_in] = 0;
                if (st.came_e <= s1) {
                    if (st.came_b >= c0) finish(wi, wo, st.came_kept, r);
                } else {
                    rd_words[0][carry_out] = wi;
                    rd_words[1][carry_out] = wo;
                    tail = st.came_k;
                }
            }
            if (st.mine) {
                const uint64_t wi = rd_words[0][t], wo = rd_words[1][t];
                rd_words[0][t] = rd_words[1][t] = 0;
                if (st.mine_e <= s1) {
                    finish(wi, wo, st.mine_kept, r);
                } else {
                    rd_words[0][carry_out] = wi;
                    rd_words[1][carry_out] = wo;
                    tail = st.mine_k;
                }
            }
        }
        cur = k_last;
    }
    const uint32_t carry = CARRY + (step & 1);
    if (tail < R) {
        const uint64_t b = off[tail], e = std::min(off[tail + 1], total);
        if (b >= c0 && b < c1) {
            const Read &rd = reads[tail];
            uint64_t wi = rd_words[0][carry], wo = rd_words[1][carry];
            for (uint64_t q = c1; q < e; q += 16) {
                const uint32_t n = (uint32_t)std::min<uint64_t>(16, e - q);
                uint64_t w[2];
                load(rd, q - b, w);
                fqb_seg sg;
                fqb_segment(w, n, q - b, rd.five, rd.three, &sg);
                wi = fqb_read_add(wi, fqb_read_part(&sg, fqb_range16(0, n)));
                wo = fqb_read_add(wo, fqb_read_part(&sg, sg.out));
            }
            finish(wi, wo, fqp_kept(rd.three), r);
        }
    }
    for (uint32_t i = 0; i < bins; ++i)
        for (uint32_t cl = 0; cl < FQB_CLASSES; ++cl) {
            const uint64_t x = tab[cl * PS + fqp_slot(i)];
            r.pos_in[(uint64_t)cl * bins + i] += (x & 0xffffffffull) + (i == last ? tail_in[cl] : 0);
            r.pos_out[(uint64_t)cl * bins + i] += (x >> 32) + (i == last ? tail_out[cl] : 0);
        }
}

void walk(const std::vector<Read> &reads, uint64_t chunk, uint32_t bins, Result &r)
{
    r.w[FQB_W_CALLS] += 1;
    std::vector<uint64_t> off(reads.size() + 1, 0);
    for (size_t i = 0; i < reads.size(); ++i) off[i + 1] = off[i] + reads[i].len;
    for (uint64_t c0 = 0; c0 < off.back(); c0 += chunk) walk_chunk(reads, off, c0, std::min(c0 + chunk, off.back()), bins, r);
}

// ---- batches ---------------------------------------------------------------------------------------------------------------
uint8_t draw_byte(int flavour)
{
    static const char *plain = "ACGT", *mixed = "ACGTNacgtn", *wild = "ACGTNacgtnRYKMSWBDHVU.-*\r";
    switch (flavour) {
    case 0: return (uint8_t)plain[below(4)];
    case 1: return below(50) ? (uint8_t)plain[below(4)] : (uint8_t)'N';
    case 2: return (uint8_t)mixed[below(10)];
    case 3: return below(4) ? (uint8_t)wild[below(25)] : (uint8_t)below(256);
    default: return (uint8_t)'N';
    }
}

Read make_read(uint64_t len, int flavour, int cut)
{
    Read r;
    r.len = len;
    r.seq.reset(new uint8_t[len]);
    for (uint64_t i = 0; i < len; ++i) r.seq[i] = draw_byte(flavour);
    // cut: 0 whole, 1 not kept, 2 drawn, 3 empty output
    if (cut == 1) {
        r.five = r.three = -1;
    } else if (cut == 0) {
        r.five = 0;
        r.three = (int32_t)len;
    } else if (cut == 3) {
        r.five = r.three = (int32_t)below(len + 1);
    } else {
        r.five = (int32_t)below(len);
        r.three = r.five + 1 + (int32_t)below(len - r.five);
    }
    return r;
}

int cases = 0;

bool check(const std::vector<Read> &reads, uint64_t chunk, uint32_t bins, const char *what)
{
    Result a(bins), b(bins);
    naive(reads, bins, a);
    walk(reads, chunk, bins, b);
    ++cases;
    if (a == b) return true;
    std::fprintf(stderr, "the walk and the naive computation differ: %s (%zu reads, chunk %llu, %u bins)\n", what, reads.size(),
                 (unsigned long long)chunk, bins);
    for (int i = 0; i < FQB_WORDS; ++i)
        if (a.w[i] != b.w[i]) std::fprintf(stderr, "  word %d: naive %llu, walk %llu\n", i, (unsigned long long)a.w[i], (unsigned long long)b.w[i]);
    return false;
}

bool drawn()
{
    const uint32_t bin_choices[] = {1, 2, 5, 16, 31, 32, 33, 150, 151, 1024};
    for (int it = 0; it < 300; ++it) {
        std::vector<Read> reads;
        const uint64_t n = 1 + below(it % 10 == 0 ? 3000 : 200);
        const int shape = (int)below(4);
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t len = shape == 0 ? 1 + below(40) : shape == 1 ? 1 + below(5) : shape == 2 ? 100 + below(100) : 1 + below(20);
            if (shape == 3 && below(40) == 0) len = 3000 + below(12000); // a long read among short ones
            reads.push_back(make_read(len, (int)below(5), (int)below(4)));
        }
        const uint64_t chunk = 4096u << below(3);
        if (!check(reads, chunk, bin_choices[below(10)], "drawn")) return false;
    }
    return true;
}

bool shapes()
{
    const uint64_t C = FQB_CHUNK_BYTES;
    // a read of chunk + 1 000 bases among 20-base ones
    for (uint32_t bins : {1u, 64u, 1024u}) {
        std::vector<Read> reads;
        for (int i = 0; i < 50; ++i) reads.push_back(make_read(20, 2, 2));
        reads.push_back(make_read(C + 1000, 2, 2));
        for (int i = 0; i < 50; ++i) reads.push_back(make_read(20, 2, 2));
        if (!check(reads, C, bins, "a read longer than a chunk")) return false;
    }
    // a 200-base read across the chunk boundary, five below it and three above, its only N on either side
    for (int side = 0; side < 2; ++side) {
        std::vector<Read> reads;
        uint64_t have = 0;
        while (have + 150 <= C - 100) {
            reads.push_back(make_read(150, 0, 2));
            have += 150;
        }
        reads.push_back(make_read(C - 100 - have, 0, 0)); // the next read starts 100 below the boundary
        Read r = make_read(200, 0, 0);
        r.five = 40;
        r.three = 160;
        r.seq[side ? 130 : 70] = 'N';
        reads.push_back(std::move(r));
        for (int i = 0; i < 30; ++i) reads.push_back(make_read(150, 0, 2));
        if (!check(reads, C, 151, "a read across the chunk boundary")) return false;
    }
    // the only N the last byte, the only N the first
    for (uint64_t len : {1u, 15u, 16u, 17u, 31u, 32u, 33u, 150u}) {
        std::vector<Read> reads;
        for (int i = 0; i < 300; ++i) {
            Read r = make_read(len, 0, i % 3 ? 2 : 0);
            r.seq[i & 1 ? len - 1 : 0] = i & 2 ? 'N' : 'n';
            reads.push_back(std::move(r));
        }
        if (!check(reads, 4096, 33, "read lengths around the granule")) return false;
    }
    std::vector<Read> ones;
    for (int i = 0; i < 9001; ++i) ones.push_back(make_read(1, 2, i % 4 == 0 ? 1 : 0));
    return check(ones, 4096, 2, "one-base reads") && check(ones, C, 1, "one-base reads");
}

} // namespace

int main(int argc, char **argv)
{
    corrupt = argc > 1 && std::strcmp(argv[1], "--corrupt") == 0;
    if (!drawn() || !shapes()) return 1;
    std::printf("ok %d chunk %u\n", cases, (unsigned)FQB_CHUNK_BYTES);
    return 0;
}
