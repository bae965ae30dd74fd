// TEST INFRASTRUCTURE ONLY: the rule of sickle_amd/csrc/sk_fastq_adapters.h executed on the host in the shape the kernel of
// sk_fastq_adapters.hip gives it -- a wave of 64 lanes a read, tiles of 64 starts, a lane encoding ONE byte a tile
// (fqd_code) and the wave's three ballots making a word per plane, a lane's window a funnel shift of two words by its lane
// number (fqd_funnel), every adapter compared with one popcount (fqd_start), the lowest lane with a hit ending the walk,
// and a read's words summed with fqd_read_word and fqd_pair_word -- and checked against a second, naive computation, byte
// by byte, that takes nothing from that header.  Every seq line lies in a heap block of exactly its length, so that the
// address sanitizer sees a load beyond a line.
// Cases: adapters of 1, 31, 32, 33, 63 and 64 bases; lines of 1 .. 130 bases with the adapter planted at EVERY start, and of
// 4 095 .. 4 097 bases with it planted around every tile edge and at the line's two ends; drawn mismatches, lower case, N
// and '\r' in the planted copy; sets of one to eight adapters with drawn min_overlap and permille.
// `adapters_host` prints "ok <cases>" and returns 0; `adapters_host --corrupt` drops the VALID plane on the walk's side (an
// N then reads as an A) and must return 1 (the comparison sees it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "sk_fastq_adapters.h"

namespace {

bool corrupt = false;

struct Read {
    std::unique_ptr<uint8_t[]> seq; // exactly len bytes
    uint64_t len;
    int32_t five, three;
};

struct Hit {
    bool hit;
    uint32_t a, v, m;
    uint64_t p;
    bool operator==(const Hit &o) const { return hit == o.hit && (!hit || (a == o.a && v == o.v && m == o.m && p == o.p)); }
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

// ---- the naive side: the rule as include/sickle_amd.h words it, nothing taken from sk_fastq_adapters.h ---------------------
bool naive_match(uint8_t b, uint8_t c) { return (uint8_t)(b & 0xDF) == (uint8_t)(c & 0xDF); } // c is a letter of the set

Hit naive_hit(const uint8_t *line, uint64_t L, const sk_fastq_adapter_set &s)
{
    Hit none = {false, 0, 0, 0, 0};
    if (L < s.min_overlap) return none;
    for (uint64_t p = 0; p + s.min_overlap <= L; ++p)
        for (uint32_t a = 0; a < s.n; ++a) {
            const uint64_t v = std::min<uint64_t>(s.len[a], L - p);
            if (v < s.min_overlap) continue;
            const uint64_t allow = v * s.max_mismatch_permille / 1000;
            uint64_t m = 0;
            for (uint64_t j = 0; j < v && m <= allow; ++j) m += !naive_match(line[p + j], s.seq[a][j]); // (stops once it is no hit)
            if (m <= allow) return Hit{true, a, (uint32_t)v, (uint32_t)m, p};
        }
    return none;
}

void naive_add(uint64_t *w, const Read &r, const Hit &h, const sk_fastq_adapter_set &s)
{
    const bool kept = r.three >= 0;
    w[2] += 1;
    w[3] += kept;
    if (!h.hit) return;
    w[4] += 1;
    w[5] += kept;
    w[6 + h.a] += 1;
    w[14] += h.v == s.len[h.a];
    w[15] += h.p == 0;
    w[16] += h.m;
    w[17] += r.len - h.p;
    if (kept && h.p < (uint64_t)r.three) {
        w[18] += 1;
        w[19] += (uint64_t)r.three - std::max<uint64_t>(h.p, (uint64_t)r.five);
    }
}

void naive_pair(uint64_t *w, const Hit &h1, const Hit &h2)
{
    w[20] += h1.hit && h2.hit;
    w[21] += h1.hit != h2.hit;
    w[22] += h1.hit && h2.hit && h1.p == h2.p;
}

// ---- the walk: the kernel's shape --------------------------------------------------------------------------------------
// the wave's three ballots over the lanes' codes of bases [t, t + 64): every byte is loaded from the line's own block
fqd_planes load_planes(const uint8_t *line, uint64_t L, uint64_t t)
{
    fqd_planes w = {0, 0, 0};
    for (uint32_t lane = 0; lane < 64; ++lane) {
        const uint64_t i = t + lane;
        uint32_t code = 4;
        if (i < L) code = fqd_code(line[i]);
        w.lo |= (uint64_t)((code & 1u) != 0) << lane;
        w.hi |= (uint64_t)((code & 2u) != 0) << lane;
        w.valid |= (uint64_t)(code < 4u || (corrupt && i < L)) << lane;
    }
    return w;
}

fqd_read walk_read(const Read &r, const fqd_codes &c)
{
    fqd_read rd;
    std::memset(&rd, 0, sizeof rd);
    rd.L = r.len;
    rd.five = r.five;
    rd.three = r.three;
    const uint64_t L = r.len, mo = c.min_overlap;
    if (L < mo) return rd;
    const uint64_t last = L - mo;
    fqd_planes w0 = load_planes(r.seq.get(), L, 0);
    for (uint64_t t0 = 0; t0 <= last; t0 += 64) {
        fqd_planes w1 = {0, 0, 0};
        if (t0 + 64 < L) w1 = load_planes(r.seq.get(), L, t0 + 64);
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
        if (hits) { // the winner's overlap and mismatches are worked out once more, for it alone
            const uint32_t src = (uint32_t)__builtin_ctzll(hits);
            rd.hit = 1;
            rd.a = ad[src];
            rd.p = t0 + (uint64_t)src;
            rd.A = c.len[rd.a];
            rd.v = fqd_overlap(rd.A, L, rd.p);
            rd.m = fqd_mismatches(fqd_funnel(w0.lo, w1.lo, src), fqd_funnel(w0.hi, w1.hi, src), fqd_funnel(w0.valid, w1.valid, src),
                                  c.lo[rd.a], c.hi[rd.a], rd.v);
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
    // a drawn cut: not kept, or 0 <= five <= three <= L
    if (below(5) == 0 || L == 0) {
        r.five = r.three = -1;
    } else {
        r.three = (int32_t)below(L + 1);
        r.five = (int32_t)below((uint64_t)r.three + 1);
    }
    return r;
}

uint64_t cases = 0;

bool run_batch(const std::vector<Read> &reads, const sk_fastq_adapter_set &s, const char *what)
{
    if (fqd_set_error(&s)) {
        std::fprintf(stderr, "%s: the set is refused: %s\n", what, fqd_set_error(&s));
        return false;
    }
    fqd_codes c;
    fqd_encode_set(&s, &c);
    uint64_t naive[FQD_WORDS], walk[FQD_WORDS];
    std::memset(naive, 0, sizeof naive);
    std::memset(walk, 0, sizeof walk);
    Hit prev_n = {false, 0, 0, 0, 0};
    fqd_read prev_w;
    std::memset(&prev_w, 0, sizeof prev_w);
    for (size_t i = 0; i < reads.size(); ++i) {
        const Read &r = reads[i];
        const Hit hn = naive_hit(r.seq.get(), r.len, s);
        const fqd_read rd = walk_read(r, c);
        const Hit hw = {rd.hit != 0, rd.a, rd.v, rd.m, rd.p};
        if (!(hn == hw)) {
            std::fprintf(stderr, "%s: read %zu of %llu bases: the hits differ: naive %d a %u p %llu v %u m %u, walk %d a %u p %llu v %u m %u\n",
                         what, i, (unsigned long long)r.len, hn.hit, hn.a, (unsigned long long)hn.p, hn.v, hn.m, hw.hit, hw.a,
                         (unsigned long long)hw.p, hw.v, hw.m);
            return false;
        }
        const uint32_t want_clip = hn.hit ? (hn.a << 24 | (uint32_t)hn.p) : 0xFFFFFFFFu;
        if (fqd_clip_word(&rd) != want_clip) {
            std::fprintf(stderr, "%s: read %zu: the clip words differ\n", what, i);
            return false;
        }
        naive_add(naive, r, hn, s);
        for (uint32_t w = FQD_W_READS; w <= FQD_W_BASES_HIT_OUT; ++w) walk[w] += fqd_read_word(w, &rd);
        if (i & 1) {
            naive_pair(naive, prev_n, hn);
            for (uint32_t w = FQD_W_PAIRS_BOTH; w <= FQD_W_PAIRS_SAME_CLIP; ++w) walk[w] += fqd_pair_word(w, &prev_w, &rd);
        }
        prev_n = hn;
        prev_w = rd;
        ++cases;
    }
    if (std::memcmp(naive, walk, sizeof naive) != 0) {
        for (uint32_t w = 0; w < FQD_WORDS; ++w)
            if (naive[w] != walk[w])
                std::fprintf(stderr, "%s: word %u differ: naive %llu, walk %llu\n", what, w, (unsigned long long)naive[w],
                             (unsigned long long)walk[w]);
        return false;
    }
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    corrupt = argc > 1 && std::strcmp(argv[1], "--corrupt") == 0;
    bool ok = true;
    const uint32_t LENS[] = {1, 31, 32, 33, 63, 64};
    // every adapter length alone, lines of 1 .. 130 bases, the adapter at every start
    for (uint32_t A : LENS) {
        const uint32_t mo = std::min<uint32_t>(A, 1 + (uint32_t)below(5));
        for (uint32_t permille : {0u, 100u, 500u}) {
            const sk_fastq_adapter_set s = make_set({A}, mo, permille);
            std::vector<Read> reads;
            for (uint64_t L = 1; L <= 130; ++L)
                for (uint64_t p = 0; p < L; ++p) reads.push_back(make_read(L, &s, 0, p, (uint32_t)below(A / 8 + 2)));
            ok = run_batch(reads, s, "short lines") && ok;
        }
    }
    // lines of 4 095 .. 4 097 bases: around every tile edge, and at the two ends; min_overlap high enough that the drawn
    // bases hold no hit of their own in front of the planted one too often
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
    for (int it = 0; it < 60; ++it) {
        std::vector<uint32_t> lens;
        const uint32_t n = 1 + (uint32_t)below(8);
        uint32_t shortest = 64;
        for (uint32_t a = 0; a < n; ++a) {
            lens.push_back(below(3) ? LENS[below(6)] : 1 + (uint32_t)below(64));
            shortest = std::min(shortest, lens.back());
        }
        const sk_fastq_adapter_set s = make_set(lens, 1 + (uint32_t)below(shortest), (uint32_t)below(501));
        std::vector<Read> reads;
        for (int k = 0; k < 300; ++k) {
            const uint64_t L = below(20) ? 1 + below(300) : below(3);
            reads.push_back(below(4) && L ? make_read(L, &s, (uint32_t)below(n), below(L), (uint32_t)below(6)) : make_read(L, nullptr, 0, 0, 0));
        }
        ok = run_batch(reads, s, "drawn sets") && ok;
    }
    // an N where the adapter has an A, at 0 permille: no hit (what --corrupt turns into one)
    {
        sk_fastq_adapter_set s = make_set({8}, 8, 0);
        std::memcpy(s.seq[0], "ACGTACGT", 8);
        std::vector<Read> reads;
        reads.push_back(make_read(20, nullptr, 0, 0, 0));
        std::memcpy(reads[0].seq.get(), "TTTTTTNCGTACGTTTTTTT", 20);
        reads.push_back(make_read(20, nullptr, 0, 0, 0));
        std::memcpy(reads[1].seq.get(), "TTTTTTacgtACGTTTTTTT", 20);
        ok = run_batch(reads, s, "an N is no A") && ok;
    }
    if (!ok) return 1;
    std::printf("ok %llu\n", (unsigned long long)cases);
    return 0;
}
