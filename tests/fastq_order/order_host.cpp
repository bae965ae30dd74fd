// TEST INFRASTRUCTURE ONLY: sk_fastq_order.h on the host.  Reads cases from a file of little-endian 64-bit words and writes
// its results as such words (tests/test_fastq_order_host.py has both formats):
//   case "chain" (1): n_in, m, batch_len, capacity, limit, T, se, then per input: its line count
//       and the length of every line.  The descriptor table is built the way the framing kernels build it (5 words per
//       record: name start, line ends), in a buffer of exactly the size the lines need, so that the sanitizer sees a read
//       beyond it.  -> batches, units, last_units, mismatch, overflow, batched_lines[2], tab[0 .. batches], then the units
//       in emission order as the lanes of the emission kernels find them (fqo_lane_units), lane after lane.
//   case "walk" (2): T, se, batches, tab[0 .. batches] -> the units in emission order, lane after lane.
// Every result is preceded by its word count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sk_fastq_order.h"

typedef std::vector<uint64_t> words;

static void walk(const uint64_t *tab, uint64_t batches, uint64_t T, bool se, words &out)
{
    const uint64_t ranks = tab[batches];
    if (se) {
        for (uint64_t first = 0; first < ranks + 8; first += 8) { // one idle lane behind the last rank
            uint64_t u[8];
            fqo_lane_units<8>(tab, batches, T, true, first, ranks, u);
            for (int j = 0; j < 8; ++j)
                if (u[j] != ~0ull) out.push_back(u[j]);
        }
    } else {
        for (uint64_t first = 0; first < ranks + 4; first += 4) {
            uint64_t u[4];
            fqo_lane_units<4>(tab, batches, T, false, first, ranks, u);
            for (int j = 0; j < 4; ++j)
                if (u[j] != ~0ull) out.push_back(u[j]);
        }
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    words in;
    uint64_t w;
    while (fread(&w, 8, 1, f) == 1) in.push_back(w);
    fclose(f);
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    size_t at = 0;
    auto next = [&]() -> uint64_t {
        if (at >= in.size()) {
            fprintf(stderr, "short case file\n");
            exit(2);
        }
        return in[at++];
    };
    while (at < in.size()) {
        const uint64_t kind = next();
        words out;
        if (kind == 1) {
            const uint64_t n_in = next(), m = next(), L = next(), cap = next(), limit = next(), T = next(), se = next();
            std::vector<words> desc(2);
            uint64_t nl[2] = {0, 0};
            for (uint64_t i = 0; i < n_in; ++i) {
                nl[i] = next();
                desc[i].assign(5 * ((nl[i] + 3) / 4), 0);
                uint64_t start = 0;
                for (uint64_t l = 0; l < nl[i]; ++l) {
                    const uint64_t len = next();
                    if ((l & 3) == 0) desc[i][5 * (l >> 2)] = start;
                    desc[i][5 * (l >> 2) + 1 + (l & 3)] = start + len;
                    start += len + 1;
                }
                desc[i].shrink_to_fit();
            }
            const uint64_t *const d[2] = {desc[0].data(), desc[1].data()};
            words tab(cap + 1);
            fqo_chain_result r;
            fqo_chain(d, nl, (int)n_in, (uint32_t)m, L, cap, limit, tab.data(), &r);
            out = {r.batches, r.units, r.last_units, r.mismatch, r.overflow, r.batched_lines[0], r.batched_lines[1]};
            for (uint64_t b = 0; b <= r.batches; ++b) out.push_back(tab[b]);
            walk(tab.data(), r.batches, T, se != 0, out);
        } else if (kind == 2) {
            const uint64_t T = next(), se = next(), batches = next();
            words tab(batches + 1);
            for (uint64_t b = 0; b <= batches; ++b) tab[b] = next();
            walk(tab.data(), batches, T, se != 0, out);
        } else {
            fprintf(stderr, "unknown case kind\n");
            return 2;
        }
        const uint64_t n = out.size();
        fwrite(&n, 8, 1, g);
        if (n) fwrite(out.data(), 8, n, g);
    }
    fclose(g);
    return 0;
}
