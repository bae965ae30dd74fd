// TEST INFRASTRUCTURE ONLY: the source view of sk_fastq_source.h on the host.  Reads cases from a file of little-endian
// 64-bit words and writes its results as such words, every result preceded by its word count
// (tests/test_fastq_source_host.py has both formats).  A case is the count of the words that follow, its tag, and then:
//   1 layout:   text_bytes, trunc_n, kind, batch_capacity, mode (~0: FQS_NO_MODE), in given, text[0] given, text[1]
//               given, bytes[0], bytes[1].  No memory is touched: the workspace and the texts are made-up addresses.
//       -> hdr, order_words, desc, offsets, cuts, pq as offsets from the workspace (~0: NULL); text[0], text[1] as offsets
//          from their made-up addresses (~0: NULL); bytes[2], slots0, slot_bound, n_bound, q_bound, kind, mode
//   2 validity: kind, mode (~0: FQS_NO_MODE), the header's 32 words, the 32 words of an ordered piece's block.  The
//               workspace is a buffer of exactly the header, and the block behind it for the ordered piece alone, so that
//               the sanitizer sees a word read that is not there.
//       -> fqs_valid
//   3 lookups:  framing mode, bytes[0], bytes[1], slots0, slot_bound, the 5 * slot_bound descriptor words, the number of
//               reads asked for, the reads.  The table and the texts are buffers of exactly their sizes, and every byte
//               of every span that comes back is read.
//       -> per read: fqs_input; fqs_name_line (ok, offset, length); fqs_seq_start; fqs_record (input, offset, length)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sk_fastq_source.h"

typedef std::vector<uint64_t> words;

static const uintptr_t WS = (uintptr_t)1 << 40, TEXT[2] = {(uintptr_t)3 << 40, (uintptr_t)5 << 40};
static const uint64_t NONE = ~0ull;
static volatile uint64_t g_sink; // the bytes read

static uint64_t off_of(const void *p, uintptr_t base) { return p ? (uint64_t)((uintptr_t)p - base) : NONE; }

static void touch(const uint8_t *p, uint64_t len)
{
    uint64_t s = 0;
    for (uint64_t i = 0; i < len; ++i) s += p[i];
    g_sink = g_sink + s;
}

static size_t layout_case(const uint64_t *c, words &out)
{
    sk_fastq_report_source src = {};
    src.workspace = reinterpret_cast<const void *>(WS);
    src.text_bytes = c[0];
    src.trunc_n = (int32_t)c[1];
    src.kind = (uint32_t)c[2];
    src.batch_capacity = c[3];
    const int mode = c[4] == NONE ? FQS_NO_MODE : (int)c[4];
    sk_fastq_input in = {};
    for (int i = 0; i < 2; ++i) {
        in.text[i] = c[6 + i] ? reinterpret_cast<const uint8_t *>(TEXT[i]) : nullptr;
        in.bytes[i] = c[8 + i];
    }
    fqs_view v;
    memset(&v, 0x5a, sizeof v);
    fqs_fill(&src, c[5] ? &in : nullptr, mode, &v);
    out = {off_of(v.hdr, WS), off_of(v.order_words, WS), off_of(v.desc, WS), off_of(v.offsets, WS), off_of(v.cuts, WS),
           off_of(v.pq, WS), off_of(v.text[0], TEXT[0]), off_of(v.text[1], TEXT[1]), v.bytes[0], v.bytes[1], v.slots0,
           v.slot_bound, v.n_bound, v.q_bound, (uint64_t)(int64_t)v.kind, (uint64_t)(int64_t)v.mode};
    return 10;
}

static size_t validity_case(const uint64_t *c, words &out)
{
    const uint32_t kind = (uint32_t)c[0];
    const int mode = c[1] == NONE ? FQS_NO_MODE : (int)c[1];
    static_assert(SK_FQOP_EXT_BYTES_AT == 8 * SK_FQ_HDR_WORDS, "the block lies behind the header");
    const size_t n = SK_FQ_HDR_WORDS + (kind == SK_FQ_REPORT_ORDERED_PIECE ? SK_FQOP_EXT_BYTES / 8 : 0);
    uint64_t *ws = static_cast<uint64_t *>(malloc(8 * n)); // exactly the words the kind has
    memcpy(ws, c + 2, 8 * n);
    fqs_view v;
    memset(&v, 0x5a, sizeof v);
    fqs_fill_validity(ws, kind, mode, &v);
    out = {(uint64_t)fqs_valid(v)};
    free(ws);
    return 2 + SK_FQ_HDR_WORDS + SK_FQOP_EXT_BYTES / 8;
}

static size_t lookup_case(const uint64_t *c, words &out)
{
    fqs_view v = {};
    v.mode = (int32_t)c[0];
    v.bytes[0] = c[1];
    v.bytes[1] = c[2];
    v.slots0 = c[3];
    v.slot_bound = c[4];
    const size_t nd = 5 * (size_t)v.slot_bound;
    uint64_t *desc = static_cast<uint64_t *>(malloc(nd ? 8 * nd : 1)); // exactly slot_bound slots
    memcpy(desc, c + 5, 8 * nd);
    v.desc = desc;
    uint8_t *text[2];
    for (int i = 0; i < 2; ++i) {
        text[i] = static_cast<uint8_t *>(malloc(v.bytes[i] ? v.bytes[i] : 1));
        memset(text[i], 'A' + i, v.bytes[i] ? v.bytes[i] : 1);
        v.text[i] = text[i];
    }
    const size_t nq = (size_t)c[5 + nd];
    out.clear();
    for (size_t q = 0; q < nq; ++q) {
        const uint64_t r = c[6 + nd + q];
        out.push_back((uint64_t)fqs_input(v, r));
        const uint8_t *p = nullptr;
        uint64_t len = 0;
        const bool ok = fqs_name_line(v, r, p, len);
        out.push_back(ok);
        out.push_back(ok ? (uint64_t)(p - text[fqs_input(v, r)]) : NONE);
        out.push_back(ok ? len : NONE);
        if (ok) touch(p, len);
        out.push_back(fqs_seq_start(v, r));
        uint64_t at = 0, rl = 0;
        const int i = fqs_record(v, r, &at, &rl);
        out.push_back((uint64_t)i);
        out.push_back(at);
        out.push_back(rl);
        touch(text[i] + at, rl);
    }
    free(desc);
    free(text[0]);
    free(text[1]);
    return 6 + nd + nq;
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
    // every case carries its own length in front, so that a short file is seen
    for (size_t at = 0; at < in.size();) {
        const uint64_t len = in[at], tag = at + 1 < in.size() ? in[at + 1] : 0;
        if (len < 1 || at + 1 + len > in.size()) {
            fprintf(stderr, "short case file\n");
            return 2;
        }
        words c(in.begin() + at + 2, in.begin() + at + 1 + len), out;
        c.shrink_to_fit();
        size_t used = 0;
        if (tag == 1) used = layout_case(c.data(), out);
        else if (tag == 2) used = validity_case(c.data(), out);
        else if (tag == 3) used = lookup_case(c.data(), out);
        if (used != c.size()) {
            fprintf(stderr, "case at word %zu: tag %llu takes %zu words, has %zu\n", at, (unsigned long long)tag, used, c.size());
            return 2;
        }
        const uint64_t n = out.size();
        fwrite(&n, 8, 1, g);
        fwrite(out.data(), 8, n, g);
        at += 1 + len;
    }
    fclose(g);
    return 0;
}
