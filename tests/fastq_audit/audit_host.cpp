// TEST INFRASTRUCTURE ONLY: the audit rule of sickle_amd/csrc/sk_fastq_audit.h executed on the host in the shape the
// kernels of sk_fastq_audit.hip give it -- blocks of 2 048 reads whose lanes own four whole pairs, one a turn, each
// pair's two name lines walked side by side 8 bytes a step; chunks of FQA_CHUNK_BYTES of packed qual walked in steps of
// 256 lanes x 16 bytes, runs of equal bytes added once to one of FQA_TABLES tables; the fold -- and checked against a
// second, naive computation, byte by byte.  Every name line lies in a heap block of exactly its length, so that the
// address sanitizer sees a load beyond a line.
// Batches: drawn ones, and the shapes the GPU test lists (names of 2 to 40 bytes with every key end at every position of
// the 8-byte step, pair counts around a block, a name line of 70 000 bytes, the extremes at the first and the last byte
// and at either side of a chunk boundary, one value only, 1-base reads).
// `audit_host` prints "ok <cases>" and returns 0; `audit_host --corrupt` takes the tag rule out of the walk's side and
// must return 1 (the comparison sees it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "sk_fastq_audit.h"

namespace {

const uint32_t BLOCK_READS = 2048, THREADS = 256, PER_THREAD = BLOCK_READS / THREADS, STEP = THREADS * 16;
bool corrupt = false;

struct Batch {
    int64_t mode;
    std::vector<std::string> names; // one per read, without the '\n'
    std::vector<uint8_t> qual;      // the packed qual
};

struct Audit {
    uint64_t w[FQA_WORDS];
    std::vector<uint64_t> hist;
    Audit() : hist(256)
    {
        for (uint32_t i = 0; i < FQA_WORDS; ++i) w[i] = fqa_reset_word(i);
    }
    bool operator==(const Audit &o) const { return std::memcmp(w, o.w, sizeof w) == 0 && hist == o.hist; }
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

// the naive side: the rule as include/sickle_amd.h words it, nothing taken from sk_fastq_audit.h
void naive_key(const std::string &line, std::string &key, int &tag)
{
    size_t e = line.size();
    for (size_t i = 1; i < line.size(); ++i)
        if (line[i] == ' ' || line[i] == '\t' || line[i] == '\r') {
            e = i;
            break;
        }
    key = line.size() > 1 ? line.substr(1, e - 1) : std::string();
    tag = 0;
    if (key.size() >= 2 && key[key.size() - 2] == '/' && (key.back() == '1' || key.back() == '2')) {
        tag = key.back() - '0';
        key.resize(key.size() - 2);
    }
}

void naive(const Batch &b, Audit &r)
{
    r.w[0] += 1;
    uint64_t pairs = 0;
    if (b.mode != SK_TRIM_SE)
        for (uint64_t k = 0; 2 * k + 1 < b.names.size(); ++k) {
            std::string k1, k2;
            int t1, t2;
            naive_key(b.names[2 * k], k1, t1);
            naive_key(b.names[2 * k + 1], k2, t2);
            ++pairs;
            if (k1 != k2) {
                ++r.w[3];
                r.w[4] = std::min(r.w[4], r.w[2] + k);
            } else if (t1 == 2 && t2 == 1) {
                ++r.w[5];
            }
        }
    r.w[2] += pairs;
    for (uint8_t q : b.qual) {
        ++r.w[6];
        r.w[7] = std::min<uint64_t>(r.w[7], q);
        r.w[8] = std::max<uint64_t>(r.w[8], q);
        ++r.hist[q];
    }
}

uint32_t pair_of(const uint8_t *n1, uint64_t l1, const uint8_t *n2, uint64_t l2)
{
    uint32_t f = fqa_pair(n1, l1, n2, l2);
    if (corrupt && !(f & FQA_MISMATCH)) { // the walk without the tag rule: equal lines up to the key's end
        std::string a(reinterpret_cast<const char *>(n1), l1), b(reinterpret_cast<const char *>(n2), l2);
        auto cut = [](std::string &s) {
            const size_t e = s.find_first_of(" \t\r", 1);
            if (e != std::string::npos) s.resize(e);
        };
        cut(a);
        cut(b);
        if (a != b) f = FQA_MISMATCH;
    }
    return f;
}

// the kernels' side
void walk(const Batch &b, Audit &r)
{
    const uint64_t n_real = b.names.size();
    // exact heap blocks
    std::vector<std::unique_ptr<uint8_t[]>> line(n_real);
    for (uint64_t i = 0; i < n_real; ++i) {
        line[i].reset(new uint8_t[b.names[i].size()]);
        std::memcpy(line[i].get(), b.names[i].data(), b.names[i].size());
    }
    r.w[FQA_W_CALLS] += 1;
    // 1 the names pass
    if (b.mode != SK_TRIM_SE) {
        const uint64_t blocks = (n_real + BLOCK_READS - 1) / BLOCK_READS;
        for (uint64_t blk = 0; blk < blocks; ++blk)
            for (uint32_t t = 0; t < THREADS; ++t) {
                const uint64_t first = blk * BLOCK_READS + 2u * (uint64_t)t;
                for (uint32_t j = 0; j < PER_THREAD / 2; ++j) {
                    const uint64_t rd = first + (uint64_t)j * (2u * THREADS);
                    if (!(rd + 1 < n_real)) break;
                    const uint32_t f = pair_of(line[rd].get(), b.names[rd].size(), line[rd + 1].get(), b.names[rd + 1].size());
                    r.w[FQA_W_CALL_PAIRS] += 1;
                    if (f & FQA_MISMATCH) {
                        r.w[FQA_W_NAME_MISMATCH] += 1;
                        r.w[FQA_W_CALL_FIRST] = std::min(r.w[FQA_W_CALL_FIRST], rd >> 1);
                    }
                    if (f & FQA_SWAPPED) r.w[FQA_W_TAGS_SWAPPED] += 1;
                }
            }
    }
    // 2 the quality pass: the section is whole granules; the bytes behind the total are junk the walk must not count
    const uint64_t total = b.qual.size();
    std::vector<uint8_t> pq((total + 15) / 16 * 16, 0xa5);
    std::memcpy(pq.data(), b.qual.data(), total);
    for (uint64_t c0 = 0; c0 < total; c0 += FQA_CHUNK_BYTES) {
        const uint64_t c1 = std::min<uint64_t>(c0 + FQA_CHUNK_BYTES, total);
        std::vector<uint32_t> tab(FQA_TABLES * FQA_TABLE_STRIDE, 0);
        uint32_t lo = 0xff, hi = 0;
        for (uint32_t t = 0; t < THREADS; ++t)
            for (uint64_t g = c0 + 16u * t; g < c1; g += STEP) {
                uint32_t word[4];
                std::memcpy(word, pq.data() + g, 16);
                const uint32_t n = (uint32_t)std::min<uint64_t>(16, c1 - g);
                if (n < 16) fqa_fill_tail(word, n);
                for (int k = 0; k < 4; ++k) fqa_minmax4(word[k], &lo, &hi);
                uint32_t cur = fqa_byte(word, 0), run = 0;
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint32_t q = fqa_byte(word, i);
                    if (i < n) {
                        if (q != cur) {
                            tab[fqa_table_slot(t, cur)] += run;
                            cur = q;
                            run = 0;
                        }
                        ++run;
                    }
                }
                tab[fqa_table_slot(t, cur)] += run;
            }
        r.w[FQA_W_QUAL_BYTES] += c1 - c0;
        r.w[FQA_W_QUAL_MIN] = std::min<uint64_t>(r.w[FQA_W_QUAL_MIN], lo);
        r.w[FQA_W_QUAL_MAX] = std::max<uint64_t>(r.w[FQA_W_QUAL_MAX], hi);
        for (uint32_t q = 0; q < 256; ++q)
            for (uint32_t k = 0; k < FQA_TABLES; ++k) r.hist[q] += tab[k * FQA_TABLE_STRIDE + q];
    }
    // 3 the fold
    if (b.mode != SK_TRIM_SE) fqa_fold(r.w);
}

uint64_t cases = 0;
bool check(const std::vector<Batch> &calls, const char *what)
{
    Audit a, n;
    for (const Batch &b : calls) {
        walk(b, a);
        naive(b, n);
    }
    ++cases;
    if (a == n) return true;
    std::fprintf(stderr, "audits differ: %s (case %llu)\n", what, (unsigned long long)cases);
    for (uint32_t i = 0; i < FQA_WORDS; ++i)
        if (a.w[i] != n.w[i])
            std::fprintf(stderr, "  word %u: walk %llu naive %llu\n", i, (unsigned long long)a.w[i], (unsigned long long)n.w[i]);
    return false;
}

std::string drawn_name(uint32_t len)
{
    static const char alphabet[] = "ab:/12 \t\r3_";
    std::string s = "@";
    for (uint32_t i = 1; i < len; ++i) s += alphabet[below(sizeof alphabet - 1)];
    return s;
}

std::vector<uint8_t> drawn_qual(uint64_t n, uint32_t lo, uint32_t span)
{
    std::vector<uint8_t> q(n);
    for (auto &x : q) x = (uint8_t)(lo + below(span));
    return q;
}

Batch pairs_batch(uint64_t pairs, int how, uint64_t at)
{
    // how 0: none mismatching, 1: all, 2: exactly one, at pair `at`
    Batch b{SK_TRIM_PE_INTERLEAVED, {}, drawn_qual(pairs * 2 * 3, 33, 41)};
    for (uint64_t k = 0; k < pairs; ++k) {
        const std::string base = "@r" + std::to_string(k);
        const bool mis = how == 1 || (how == 2 && k == at);
        b.names.push_back(base + "/1");
        b.names.push_back((mis ? base + "x" : base) + "/2");
    }
    return b;
}

} // namespace

int main(int argc, char **argv)
{
    corrupt = argc > 1 && std::strcmp(argv[1], "--corrupt") == 0;
    bool ok = true;
    // every key length and end at every position of the step: names of 2 to 40 bytes, the mate equal, one byte off at the
    // key's last byte, one byte longer, with a comment behind each kind of end, with each tag
    for (uint32_t len = 2; len <= 40; ++len) {
        Batch b{SK_TRIM_PE_SPLIT, {}, drawn_qual(len, 33, 60)};
        const std::string base = "@" + std::string(len - 1, 'k');
        std::string off = base;
        off.back() = 'j';
        const char ends[] = {' ', '\t', '\r'};
        const std::pair<std::string, std::string> table[] = {
            {base, base}, {base, off}, {base, base + "k"}, {base + "/1", base + "/2"}, {base + "/2", base + "/1"},
            {base + "/2", off + "/1"}, {base + "/3", base + "/3"}, {base + "/1/1", base + "/1/2"}, {base, base + "/1"}};
        for (const auto &p : table) {
            b.names.push_back(p.first);
            b.names.push_back(p.second);
            for (char e : ends) {
                b.names.push_back(p.first + e + "1:N:0:ACGT");
                b.names.push_back(p.second + e + "2:N");
            }
        }
        ok &= check({b}, "key lengths");
    }
    {
        Batch b{SK_TRIM_PE_INTERLEAVED, {"@/1", "@/2", "@/2", "@/1", "@ a", "@ b", "@x", "@x", "@odd"}, drawn_qual(9, 0x80, 0x80)};
        ok &= check({b}, "short keys and an odd read");
        b.mode = SK_TRIM_SE;
        ok &= check({b}, "SE");
    }
    // pair counts around a block of 2 048 reads
    for (uint64_t pairs : {1ull, 1023ull, 1024ull, 1025ull, 3073ull})
        for (int how = 0; how < 3; ++how)
            for (uint64_t at : {(uint64_t)0, pairs / 2, pairs - 1}) {
                ok &= check({pairs_batch(pairs, how, at)}, "pair counts");
                if (how != 2) break;
            }
    // long name lines
    for (int differ = 0; differ < 2; ++differ) {
        std::string a = "@" + std::string(69999, 'n'), c = a;
        if (differ) c.back() = 'm';
        Batch b{SK_TRIM_PE_SPLIT, {"@p/1", "@p/2", a, c, a + " x", c + "\ty"}, drawn_qual(17, 40, 3)};
        ok &= check({b}, "long names");
    }
    // quality: the extremes at the first and the last byte and at either side of a chunk boundary; one value; sizes
    // around the granule and the chunk
    for (uint64_t total : {(uint64_t)1, (uint64_t)15, (uint64_t)16, (uint64_t)17, (uint64_t)4095, (uint64_t)4097, (uint64_t)9001,
                           (uint64_t)FQA_CHUNK_BYTES - 1, (uint64_t)FQA_CHUNK_BYTES, (uint64_t)FQA_CHUNK_BYTES + 1,
                           (uint64_t)2 * FQA_CHUNK_BYTES + 5}) {
        const uint64_t spots[] = {0, total - 1, total / 2, FQA_CHUNK_BYTES - 1, FQA_CHUNK_BYTES};
        for (uint64_t lo_at : spots)
            for (uint64_t hi_at : spots) {
                if (lo_at >= total || hi_at >= total || lo_at == hi_at) continue;
                Batch b{SK_TRIM_SE, {"@a"}, std::vector<uint8_t>(total, 70)};
                b.qual[lo_at] = 35;
                b.qual[hi_at] = 200;
                ok &= check({b}, "planted extremes");
            }
        ok &= check({Batch{SK_TRIM_SE, {"@a"}, std::vector<uint8_t>(total, 73)}}, "one value");
        ok &= check({Batch{SK_TRIM_SE, {"@a"}, drawn_qual(total, 33, 94)}}, "printable values");
    }
    // drawn batches, and accumulation over several calls (the fold's numbering)
    for (int it = 0; it < 60; ++it) {
        std::vector<Batch> calls;
        for (uint64_t c = 0, nc = 1 + below(3); c < nc; ++c) {
            Batch b{below(4) ? SK_TRIM_PE_INTERLEAVED : SK_TRIM_SE, {}, drawn_qual(below(5000), 33 + below(40), 1 + below(60))};
            for (uint64_t k = 0, n = below(300); k < n; ++k) {
                const std::string a = drawn_name(2 + below(24));
                b.names.push_back(a);
                b.names.push_back(below(3) ? a : drawn_name(2 + below(24)));
            }
            calls.push_back(b);
        }
        ok &= check(calls, "drawn");
    }
    if (!ok) return 1;
    std::printf("ok %llu chunk %llu\n", (unsigned long long)cases, (unsigned long long)FQA_CHUNK_BYTES);
    return 0;
}
