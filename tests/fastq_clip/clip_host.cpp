// TEST INFRASTRUCTURE ONLY: the rule of sickle_amd/csrc/sk_fastq_clip.h executed on the host in the shape sk_fq_clip_kernel
// gives it -- a read's line from its descriptor's two words (fqc_line), the search of sk_fastq_adapters.h on ballot bit
// planes in tiles of 64 starts, the clip word (fqd_clip_word), the packed length through it (fqc_packed_len) and the stats
// by word (fqc_read_word) -- and checked against a second, naive computation, byte by byte, that takes nothing from either
// header.  Every seq line lies in a heap block of exactly its length, so that the address sanitizer sees a load beyond a
// line.
// Cases: adapters of 1, 13, 33 and 64 bases; lines of 1 .. 130 bases with the adapter planted at EVERY start (the tile
// edges of 64 starts among them), and of 4 095 .. 4 097 bases with it around every tile edge and at the line's two ends;
// sets of one to eight adapters with drawn rules; descriptors that no framing writes (ends in front of starts, beyond the
// text, lines beyond SK_MAX_READ_LEN), which fqc_line must hold to the text; sk_trim_fastq_clip_extra_bytes' formula.
// `clip_host` prints "ok <cases>" and returns 0; `clip_host --corrupt` lets the walk's pack ignore the clip word and must
// return 1 (the comparison sees it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "sk_fastq_clip.h"

namespace {

bool corrupt = false;

struct Read {
    std::unique_ptr<uint8_t[]> seq; // exactly len bytes
    uint64_t len;
    uint64_t e0, e1; // its descriptor's words in a text of `bytes` bytes
};

uint64_t rng_state = 0x2545f4914f6cdd1dull;
uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
uint64_t below(uint64_t n) { return rnd() % n; }

// ---- the naive side: the rule as include/sickle_amd.h words it -------------------------------------------------------------
struct Hit {
    bool hit;
    uint32_t a;
    uint64_t p;
};

Hit naive_hit(const uint8_t *line, uint64_t L, const sk_fastq_adapter_set &s)
{
    if (L < s.min_overlap) return Hit{false, 0, 0};
    for (uint64_t p = 0; p + s.min_overlap <= L; ++p)
        for (uint32_t a = 0; a < s.n; ++a) {
            const uint64_t v = std::min<uint64_t>(s.len[a], L - p);
            if (v < s.min_overlap) continue;
            const uint64_t allow = v * s.max_mismatch_permille / 1000;
            uint64_t m = 0;
            for (uint64_t j = 0; j < v && m <= allow; ++j) m += (uint8_t)(line[p + j] & 0xDF) != (uint8_t)(s.seq[a][j] & 0xDF);
            if (m <= allow) return Hit{true, a, p};
        }
    return Hit{false, 0, 0};
}

// ---- the walk: the kernel's shape --------------------------------------------------------------------------------------
fqd_planes load_planes(const uint8_t *line, uint64_t L, uint64_t t)
{
    fqd_planes w = {0, 0, 0};
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = t + lane;
        uint32_t code = 4;
        if (i < L) code = fqd_code(line[i]); // the line's own block: a load at or beyond L is the sanitizer's
        w.lo |= (uint64_t)((code & 1u) != 0) << lane;
        w.hi |= (uint64_t)((code & 2u) != 0) << lane;
        w.valid |= (uint64_t)(code < 4u) << lane;
    }
    return w;
}

fqd_read walk_line(const uint8_t *line, uint64_t L, const fqd_codes &c)
{
    fqd_read rd;
    std::memset(&rd, 0, sizeof rd);
    rd.L = L;
    const uint64_t mo = c.min_overlap;
    if (L < mo) return rd;
    const uint64_t last = L - mo;
    fqd_planes w0 = load_planes(line, L, 0);
    for (uint64_t t0 = 0; t0 <= last; t0 += 64) {
        fqd_planes w1 = {0, 0, 0};
        if (t0 + 64 < L) w1 = load_planes(line, L, t0 + 64);
        uint32_t ad[64];
        uint64_t hits = 0;
        for (uint32_t lane = 0; lane < 64; ++lane) {
            const uint64_t p = t0 + lane;
            ad[lane] = FQD_NO_ADAPTER;
            if (p <= last)
                ad[lane] = fqd_start(&c, c.n, fqd_funnel(w0.lo, w1.lo, lane), fqd_funnel(w0.hi, w1.hi, lane),
                                     fqd_funnel(w0.valid, w1.valid, lane), L, p);
            hits |= (uint64_t)(ad[lane] != FQD_NO_ADAPTER) << lane;
        }
        if (hits) {
            const uint32_t src = (uint32_t)__builtin_ctzll(hits);
            rd.hit = 1;
            rd.a = ad[src];
            rd.p = t0 + (uint64_t)src;
            return rd;
        }
        w0 = w1;
    }
    return rd;
}

// ---- cases -------------------------------------------------------------------------------------------------------------------
const char BASES[] = "ACGT";

sk_fastq_adapter_set make_set(const std::vector<uint32_t> &lens, uint32_t min_overlap, uint32_t permille)
{
    sk_fastq_adapter_set s;
    std::memset(&s, 0, sizeof s);
    s.n = (uint32_t)lens.size();
    s.min_overlap = min_overlap;
    s.max_mismatch_permille = permille;
    for (uint32_t a = 0; a < s.n; ++a) {
        s.len[a] = lens[a];
        for (uint32_t j = 0; j < lens[a]; ++j) s.seq[a][j] = (uint8_t)(BASES[below(4)] | (below(8) == 0 ? 0x20 : 0));
    }
    return s;
}

// a line of L drawn bases with adapter a planted at p (cut at the line's end), `mut` drawn bytes of the copy replaced
Read make_read(uint64_t L, const sk_fastq_adapter_set *s, uint32_t a, uint64_t p, uint32_t mut)
{
    Read r;
    r.len = L;
    r.seq.reset(new uint8_t[L ? L : 1]);
    for (uint64_t i = 0; i < L; ++i) r.seq[i] = (uint8_t)BASES[below(4)];
    if (s && p < L) {
        const uint64_t v = std::min<uint64_t>(s->len[a], L - p);
        for (uint64_t j = 0; j < v; ++j) r.seq[p + j] = (uint8_t)(s->seq[a][j] ^ (below(5) == 0 ? 0x20 : 0));
        const char others[] = "ACGTNn\r.R\x80";
        for (uint32_t k = 0; k < mut; ++k) r.seq[p + below(v)] = (uint8_t)others[below(10)];
    }
    r.e0 = r.e1 = 0;
    return r;
}

uint64_t cases = 0;

// the reads as the records of one text: name lines of drawn lengths in front, '+' and qual lines behind
bool run_batch(std::vector<Read> &reads, const sk_fastq_adapter_set &s, const char *what)
{
    if (fqd_set_error(&s)) {
        std::fprintf(stderr, "%s: the set is refused: %s\n", what, fqd_set_error(&s));
        return false;
    }
    uint64_t at = 0;
    for (Read &r : reads) {
        r.e0 = at + 1 + below(40);          // the name line's '\n'
        r.e1 = r.e0 + 1 + r.len;            // the seq line's
        at = r.e1 + 1 + 1 + 1 + r.len + 1;  // "+\n", the qual line and its '\n'
    }
    const uint64_t bytes = at;
    fqd_codes c;
    fqd_encode_set(&s, &c);
    uint64_t naive[FQC_WORDS], walk[FQC_WORDS];
    std::memset(naive, 0, sizeof naive);
    std::memset(walk, 0, sizeof walk);
    for (size_t i = 0; i < reads.size(); ++i) {
        const Read &r = reads[i];
        // naive: the line is the block, the packed length min(L, p)
        const Hit hn = naive_hit(r.seq.get(), r.len, s);
        const uint64_t want_len = hn.hit ? std::min<uint64_t>(r.len, hn.p) : r.len;
        naive[2] += 1;
        if (hn.hit) {
            naive[3] += 1;
            naive[4] += hn.p == 0;
            naive[5] += r.len - hn.p;
            naive[6 + hn.a] += 1;
        }
        // the walk: L from the descriptor, the search, the word, the pack's min, the stats by word
        const fqc_span sp = fqc_line(r.e0, r.e1, bytes);
        if (sp.sq != r.e0 + 1 || sp.L != r.len) {
            std::fprintf(stderr, "%s: read %zu: the line differs: sq %llu L %llu\n", what, i, (unsigned long long)sp.sq,
                         (unsigned long long)sp.L);
            return false;
        }
        const fqd_read rd = walk_line(r.seq.get(), sp.L, c);
        const uint32_t word = fqd_clip_word(&rd);
        const uint32_t want_word = hn.hit ? (hn.a << 24 | (uint32_t)hn.p) : 0xFFFFFFFFu;
        if (word != want_word) {
            std::fprintf(stderr, "%s: read %zu of %llu bases: the clip words differ: naive %08x, walk %08x\n", what, i,
                         (unsigned long long)r.len, want_word, word);
            return false;
        }
        const uint64_t got_len = corrupt ? r.len : fqc_packed_len(r.len, word); // (the qual line is as long as the seq line)
        if (got_len != want_len) {
            std::fprintf(stderr, "%s: read %zu: the packed lengths differ: naive %llu, walk %llu\n", what, i,
                         (unsigned long long)want_len, (unsigned long long)got_len);
            return false;
        }
        for (uint32_t w = FQC_W_READS; w < FQC_W_RESERVED; ++w) walk[w] += fqc_read_word(w, &rd);
        ++cases;
    }
    if (std::memcmp(naive, walk, sizeof naive) != 0) {
        for (uint32_t w = 0; w < FQC_WORDS; ++w)
            if (naive[w] != walk[w])
                std::fprintf(stderr, "%s: word %u differ: naive %llu, walk %llu\n", what, w, (unsigned long long)naive[w],
                             (unsigned long long)walk[w]);
        return false;
    }
    return true;
}

// descriptors no framing writes: the line is held to the text and to SK_MAX_READ_LEN whatever the words are
bool wild_descriptors()
{
    const uint64_t edge[] = {0, 1, 2, 99, 100, 101, 1ull << 24, (1ull << 24) + 1, (1ull << 24) + 2, 1ull << 40, ~0ull - 1, ~0ull};
    for (uint64_t bytes : {0ull, 1ull, 100ull, (1ull << 24) + 50, 1ull << 33})
        for (uint64_t e0 : edge)
            for (uint64_t e1 : edge) {
                const fqc_span sp = fqc_line(e0, e1, bytes);
                if (sp.sq > bytes || sp.L > bytes - sp.sq || sp.L > SK_MAX_READ_LEN) {
                    std::fprintf(stderr, "wild descriptors: e0 %llu e1 %llu in %llu bytes: sq %llu L %llu\n", (unsigned long long)e0,
                                 (unsigned long long)e1, (unsigned long long)bytes, (unsigned long long)sp.sq, (unsigned long long)sp.L);
                    return false;
                }
                ++cases;
            }
    // a clip word beyond the line (no search writes one) packs the line as it is
    if (fqc_packed_len(10, 11) != 10 || fqc_packed_len(10, 10) != 10 || fqc_packed_len(10, 7u << 24 | 9) != 9 ||
        fqc_packed_len(10, 0) != 0 || fqc_packed_len(10, SK_FQ_CLIP_NONE) != 10)
        return false;
    return true;
}

bool extra_bytes()
{
    for (uint64_t T : {0ull, 1ull, 13ull, 14ull, 29ull, 30ull, 1000ull, 65536ull, (1ull << 32) - 1}) {
        const uint64_t H = (T + 2) / 16, want = (128 + 4 * (2 * H + 2) + 15) / 16 * 16;
        if (fqc_extra_bytes(T) != want || fqc_words_bound(T) != 2 * H + 2) return false;
        ++cases;
    }
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    corrupt = argc > 1 && std::strcmp(argv[1], "--corrupt") == 0;
    bool ok = true;
    const uint32_t LENS[] = {1, 13, 33, 64};
    // every adapter length alone, lines of 1 .. 130 bases, the adapter at every start
    for (uint32_t A : LENS) {
        const uint32_t mo = std::min<uint32_t>(A, 1 + (uint32_t)below(5));
        for (uint32_t permille : {0u, 100u}) {
            const sk_fastq_adapter_set s = make_set({A}, mo, permille);
            std::vector<Read> reads;
            for (uint64_t L = 1; L <= 130; ++L)
                for (uint64_t p = 0; p < L; ++p) reads.push_back(make_read(L, &s, 0, p, (uint32_t)below(A / 8 + 2)));
            ok = run_batch(reads, s, "short lines") && ok;
        }
    }
    // lines of 4 095 .. 4 097 bases: around every tile edge, and at the two ends
    for (uint32_t A : LENS) {
        const uint32_t mo = std::min<uint32_t>(A, 12);
        const sk_fastq_adapter_set s = make_set({A}, mo, A >= 31 ? 100 : 0);
        std::vector<Read> reads;
        for (uint64_t L = 4095; L <= 4097; ++L) {
            for (uint64_t p = 0; p < L; ++p) {
                const uint64_t in_tile = p & 63;
                if (p < 70 || p + 140 >= L || in_tile <= 1 || in_tile >= 62) reads.push_back(make_read(L, &s, 0, p, (uint32_t)below(3)));
            }
            reads.push_back(make_read(L, nullptr, 0, 0, 0));
        }
        ok = run_batch(reads, s, "long lines") && ok;
    }
    // sets of one to eight adapters of drawn lengths, with drawn rules
    for (int it = 0; it < 40; ++it) {
        std::vector<uint32_t> lens;
        const uint32_t n = 1 + (uint32_t)below(8);
        uint32_t shortest = 64;
        for (uint32_t a = 0; a < n; ++a) {
            lens.push_back(below(3) ? LENS[below(4)] : 1 + (uint32_t)below(64));
            shortest = std::min(shortest, lens.back());
        }
        const sk_fastq_adapter_set s = make_set(lens, 1 + (uint32_t)below(shortest), (uint32_t)below(501));
        std::vector<Read> reads;
        for (int k = 0; k < 300; ++k) {
            const uint64_t L = 1 + below(300);
            reads.push_back(below(4) ? make_read(L, &s, (uint32_t)below(n), below(L), (uint32_t)below(6)) : make_read(L, nullptr, 0, 0, 0));
        }
        ok = run_batch(reads, s, "drawn sets") && ok;
    }
    ok = wild_descriptors() && ok;
    ok = extra_bytes() && ok;
    if (!ok) return 1;
    std::printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
