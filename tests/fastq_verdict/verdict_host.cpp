// TEST INFRASTRUCTURE ONLY: fqv_verdict of sk_fastq_verdict.h on the host.  Reads cases from a file of little-endian
// 64-bit words and writes its results as such words (tests/test_fastq_verdict_host.py has both formats):
//   case: kind, the stream's live range-error word, the header's 32 words, the 32 words of an ordered piece's block
//       (read for that kind alone).  The header and the block are buffers of exactly their size, the order words are the
//       header for the ordered call, the block for the ordered piece and NULL for the other kinds, so that the sanitizer
//       sees a word read that is not there.
//       -> rc, sk_fastq_counts (17 words), sk_fastq_order_counts (9), sk_fastq_piece_counts (6), the three flags of
//          sk_fastq_order_piece_counts and its state (8 words as they lie), then the message: its bytes, one per word.
//       A struct the kind does not fill keeps the byte 0x5a, a message not written is "untouched".
// The verdict runs a second time without the optional structs and must give the same code, counts and message (exit 3).
// Every result is preceded by its word count.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sk_fastq_verdict.h"

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
    const size_t per_case = 2 + SK_FQ_HDR_WORDS + SK_FQOP_EXT_BYTES / 8;
    if (in.size() % per_case) {
        fprintf(stderr, "short case file\n");
        return 2;
    }
    for (size_t at = 0; at < in.size(); at += per_case) {
        const int kind = (int)in[at];
        const uint64_t live = in[at + 1];
        words h(in.begin() + at + 2, in.begin() + at + 2 + SK_FQ_HDR_WORDS);
        words block(in.begin() + at + 2 + SK_FQ_HDR_WORDS, in.begin() + at + per_case);
        h.shrink_to_fit();
        block.shrink_to_fit();
        const uint64_t *x = kind == SK_FQV_ORDERED ? h.data() : kind == SK_FQV_ORDERED_PIECE ? block.data() : nullptr;
        sk_fastq_counts c, c2;
        sk_fastq_order_counts oc;
        sk_fastq_piece_counts pc;
        sk_fastq_order_piece_counts opc;
        char msg[512] = "untouched", msg2[512] = "untouched";
        memset(&c, 0x5a, sizeof c);
        memset(&c2, 0x5a, sizeof c2);
        memset(&oc, 0x5a, sizeof oc);
        memset(&pc, 0x5a, sizeof pc);
        memset(&opc, 0x5a, sizeof opc);
        const uint64_t range = fqv_range_word(kind, h.data(), live);
        const int rc = fqv_verdict(kind, h.data(), x, range, &c, &oc, &pc, &opc, msg, sizeof msg);
        const int rc2 = fqv_verdict(kind, h.data(), x, range, &c2, nullptr, nullptr, nullptr, msg2, sizeof msg2);
        if (rc != rc2 || memcmp(&c, &c2, sizeof c) || strcmp(msg, msg2)) {
            fprintf(stderr, "case %zu: the optional structs change the verdict\n", at / per_case);
            return 3;
        }
        words out = {(uint64_t)(int64_t)rc, c.records_in[0], c.records_in[1], c.tail_lines[0], c.tail_lines[1], c.dropped_unpaired};
        for (int o = 0; o < 3; ++o) out.push_back(c.records[o]);
        for (int o = 0; o < 3; ++o) out.push_back(c.bytes[o]);
        for (uint64_t v : {(uint64_t)(int64_t)c.format_error, (uint64_t)c.format_input, c.format_record, (uint64_t)c.range.read,
                           (uint64_t)c.range.pos, (uint64_t)(int64_t)c.range.ch})
            out.push_back(v);
        for (uint64_t v : {oc.batches, oc.units, oc.last_batch_units, oc.records_unbatched[0], oc.records_unbatched[1],
                           (uint64_t)oc.stopped_on_mismatch, (uint64_t)oc.long_line_input, oc.long_line, oc.error_batch})
            out.push_back(v);
        for (uint64_t v : {pc.consumed[0], pc.consumed[1], pc.carried_bytes[0], pc.carried_bytes[1], (uint64_t)pc.ok,
                           (uint64_t)pc.inherited_range})
            out.push_back(v);
        for (uint64_t v : {(uint64_t)opc.table_full, (uint64_t)opc.undetermined, (uint64_t)opc.inherited_failure}) out.push_back(v);
        uint64_t state[8];
        static_assert(sizeof opc.state == sizeof state, "the state is 8 words");
        memcpy(state, &opc.state, sizeof state);
        for (uint64_t v : state) out.push_back(v);
        for (const char *p = msg; *p; ++p) out.push_back((uint64_t)(unsigned char)*p);
        const uint64_t n = out.size();
        fwrite(&n, 8, 1, g);
        fwrite(out.data(), 8, n, g);
    }
    fclose(g);
    return 0;
}
