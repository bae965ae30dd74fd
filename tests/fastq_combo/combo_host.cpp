// TEST INFRASTRUCTURE ONLY: the record rule of the device's FASTQ emission (sickle_amd/csrc/sk_fastq_record.h) executed on
// the host: for every read of every case the bytes of its record and every one of them through the piece table, the way
// the gather of sk_fastq.hip walks it, against the text the Python model wrote (tests/test_fastq_combo_model.py).
//
//   combo_host CASES
// CASES, little-endian 64-bit words: the number of cases, then per case
//   text bytes, the text (padded with zeros to 8 bytes), reads, Q, combo_all,
//   per read: s0 e0 e1 e2 e3 five three (the cut's as two's complement),
//   expected bytes, the expected text (padded likewise)
// With combo_all = 0 the reads that are not kept emit nothing (the caller lists the reads of one output in its order).
// Prints "ok <cases> <records> <bytes>" and exits 0, or says what differs and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "sk_fastq_record.h"

namespace {

struct reader {
    std::vector<uint8_t> data;
    size_t at = 0;
    bool ok = true;
    uint64_t word()
    {
        if (at + 8 > data.size()) {
            ok = false;
            return 0;
        }
        uint64_t v;
        memcpy(&v, data.data() + at, 8);
        at += 8;
        return v;
    }
    std::vector<uint8_t> bytes(uint64_t n)
    {
        const uint64_t padded = (n + 7) & ~7ull;
        if (padded > data.size() - at) {
            ok = false;
            return {};
        }
        std::vector<uint8_t> v(data.begin() + at, data.begin() + at + n);
        at += padded;
        return v;
    }
};

// byte rel of a record made of np pieces, as fq_fill of sk_fastq.hip finds it; every text piece must lie inside the text
template <int NP>
bool piece_byte(const std::vector<uint8_t> &text, const fqr_piece (&pc)[NP], uint64_t rel, uint8_t *out, std::string *why)
{
    uint64_t ps = 0;
    for (int j = 0; j < NP; ++j) {
        const uint64_t pe = ps + pc[j].len;
        if (rel >= ps && rel < pe) {
            if (pc[j].at == FQR_IMM) {
                if (pc[j].len > 8) {
                    *why = "an immediate piece of more than 8 bytes";
                    return false;
                }
                *out = (uint8_t)(pc[j].imm >> (8 * (rel - ps)));
                return true;
            }
            const uint64_t p = pc[j].at + (rel - ps);
            if (p >= text.size()) {
                *why = "a text piece reaches beyond the text";
                return false;
            }
            *out = text[p];
            return true;
        }
        ps = pe;
    }
    *why = "a byte beyond the pieces";
    return false;
}

template <int NP>
uint64_t pieces_total(const fqr_piece (&pc)[NP])
{
    uint64_t n = 0;
    for (int j = 0; j < NP; ++j) n += pc[j].len;
    return n;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: combo_host CASES\n");
        return 2;
    }
    reader in;
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    uint8_t chunk[1 << 16];
    for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) in.data.insert(in.data.end(), chunk, chunk + n);
    fclose(f);
    const uint64_t cases = in.word();
    uint64_t total_records = 0, total_bytes = 0;
    for (uint64_t c = 0; c < cases && in.ok; ++c) {
        const uint64_t text_bytes = in.word();
        const std::vector<uint8_t> text = in.bytes(text_bytes);
        const uint64_t reads = in.word();
        const uint32_t q = (uint32_t)in.word();
        const bool combo_all = in.word() != 0;
        std::vector<uint8_t> got;
        uint64_t emitted = 0;
        for (uint64_t r = 0; r < reads && in.ok; ++r) {
            fqr_lines x;
            x.s0 = in.word();
            x.e0 = in.word();
            x.e1 = in.word();
            x.e2 = in.word();
            x.e3 = in.word();
            const int32_t five = (int32_t)(int64_t)in.word(), three = (int32_t)(int64_t)in.word();
            if (!in.ok) break;
            if (!fqr_kept(three) && !combo_all) continue;
            const uint64_t n = fqr_bytes(x, five, three);
            std::string why;
            uint64_t total;
            bool fine = true;
            fqr_piece pc[6];
            fqr_pieces(x, five, three, combo_all, q, pc);
            total = pieces_total(pc);
            // the slots' kinds are fixed, and an N record has no byte from the text behind its name line
            if (pc[2].at != FQR_IMM || pc[5].at != FQR_IMM || pc[0].at == FQR_IMM || pc[1].at == FQR_IMM || pc[3].at == FQR_IMM ||
                pc[4].at == FQR_IMM || (!fqr_kept(three) && pc[1].len + pc[3].len + pc[4].len + pc[5].len != 0)) {
                fine = false;
                why = "the piece table's slots are not what the gather takes them for";
            }
            for (uint64_t b = 0; b < n && fine; ++b) {
                uint8_t v = 0;
                fine = piece_byte(text, pc, b, &v, &why);
                got.push_back(v);
            }
            if (!fine || total != n) {
                fprintf(stderr, "case %llu, read %llu: %s (bytes %llu, pieces %llu)\n", (unsigned long long)c, (unsigned long long)r,
                        fine ? "the pieces do not add up to the record's bytes" : why.c_str(), (unsigned long long)n,
                        (unsigned long long)total);
                return 1;
            }
            ++emitted;
        }
        const uint64_t want_bytes = in.word();
        const std::vector<uint8_t> want = in.bytes(want_bytes);
        if (!in.ok) break;
        if (got != want) {
            size_t d = 0;
            while (d < got.size() && d < want.size() && got[d] == want[d]) ++d;
            fprintf(stderr, "case %llu: %zu bytes against the model's %zu, first difference at byte %zu\n", (unsigned long long)c,
                    got.size(), want.size(), d);
            return 1;
        }
        if (combo_all && got.size() > fqr_combo_all_bound(text_bytes, reads)) {
            fprintf(stderr, "case %llu: %zu bytes are beyond the bound %llu\n", (unsigned long long)c, got.size(),
                    (unsigned long long)fqr_combo_all_bound(text_bytes, reads));
            return 1;
        }
        total_records += emitted;
        total_bytes += got.size();
    }
    if (!in.ok || in.at != in.data.size()) {
        fprintf(stderr, "the case file is cut short or has bytes left over\n");
        return 2;
    }
    printf("ok %llu %llu %llu\n", (unsigned long long)cases, (unsigned long long)total_records, (unsigned long long)total_bytes);
    return 0;
}
