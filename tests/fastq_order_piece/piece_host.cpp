// TEST INFRASTRUCTURE ONLY: fqo_chain_piece of sk_fastq_order.h on the host.  Reads cases from a file of little-endian
// 64-bit words and writes its results as such words (tests/test_fastq_order_piece_host.py has both formats):
//   case: n_in, m, batch_len, capacity, limit, more, then the state (carried[2], batches, ended), then per input: the
//       window's first byte, its line count and the length of every line.  The descriptor table is built the way the
//       framing kernels build it for a window that starts at that byte (5 words per record: name start, line ends, as
//       offsets in the text), in a buffer of exactly the size the lines need, and the batch table has capacity + 1 entries,
//       so that the sanitizer sees an access beyond either.
//       -> batches, units, last_units, mismatch, ended, table_full, undetermined, batched_lines[2], carried[2],
//          tab[0 .. batches]
// Every result is preceded by its word count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sk_fastq_order.h"

typedef std::vector<uint64_t> words;

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
        const uint64_t n_in = next(), m = next(), L = next(), cap = next(), limit = next(), more = next();
        fqo_piece_state st;
        st.carried[0] = next();
        st.carried[1] = next();
        st.batches = next();
        st.ended = (uint32_t)next();
        std::vector<words> desc(2);
        uint64_t nl[2] = {0, 0}, first[2] = {0, 0};
        for (uint64_t i = 0; i < n_in && i < 2; ++i) {
            first[i] = next();
            nl[i] = next();
            desc[i].assign(5 * ((nl[i] + 3) / 4), 0);
            uint64_t start = first[i];
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
        tab.shrink_to_fit();
        fqo_piece_result r;
        fqo_chain_piece(d, nl, first, (int)n_in, (uint32_t)m, L, cap, limit, &st, more != 0, tab.data(), &r);
        words out = {r.batches, r.units, r.last_units, r.mismatch, r.ended, r.table_full, r.undetermined,
                     r.batched_lines[0], r.batched_lines[1], r.carried[0], r.carried[1]};
        for (uint64_t b = 0; b <= r.batches; ++b) out.push_back(tab[b]);
        const uint64_t n = out.size();
        fwrite(&n, 8, 1, g);
        fwrite(out.data(), 8, n, g);
    }
    fclose(g);
    return 0;
}
