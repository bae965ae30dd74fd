// TEST INFRASTRUCTURE ONLY: sk_gunzip_block.h on the host.  Usage: gunzip_host <batch> <results> <texts>
//                                                                 gunzip_host --shift <numbers> <results>
//                                                                 gunzip_host --crc <buffer> <cut> <results>
//   batch    records of: uint32 LE chunk bytes, uint32 LE length, then that many bytes of a gzip image
//   results  one line per image: error member offset members bytes_out stretches stretches_used   (error: SK_GZ_*)
//   texts    the texts of the images without an error, back to back
// The stages run in the order of sk_gunzip.hip's launches, every unit of work in turn, lanes one after the other.  Every
// image, `out` and every section of the workspace is an allocation of exactly its size, so a read or a write outside
// them is a sanitizer report.  The capacity is what a counting pass reports, as Context.gunzip does it.
// --shift: one decimal k per line of <numbers> -> one line each: skg_shift_of(power, k) after skg_crc_tables.
// --crc: the CRC-32 of <buffer> as skg_crc_piece and skg_check_member assemble it from the spans [0, cut) and [cut, end).
// The same source with -DSKG_REBASE_AT=64u is gunzip_host_rebase: the bit reader re-bases at every block and batch.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sk_gunzip_block.h"

static ski_shared sh;
static skg_crc_shared cs;
static skg_walk walk;

static int shift_mode(const char *numbers, const char *results)
{
    FILE *in = fopen(numbers, "r"), *res = fopen(results, "w");
    if (!in || !res) return 2;
    unsigned long long k;
    while (fscanf(in, "%llu", &k) == 1) fprintf(res, "%u\n", skg_shift_of(cs.power, k));
    fclose(in);
    fclose(res);
    return 0;
}

static int crc_mode(const char *buffer, const char *cut_text, const char *results)
{
    FILE *in = fopen(buffer, "rb"), *res = fopen(results, "w");
    if (!in || !res) return 2;
    std::vector<uint8_t> data;
    uint8_t block[65536];
    for (size_t got; (got = fread(block, 1, sizeof block, in)) > 0;) data.insert(data.end(), block, block + got);
    const uint64_t len = data.size(), cut = strtoull(cut_text, nullptr, 10);
    if (cut > len || len > 0xffffffffull) return 2;
    uint32_t acc = 0;
    if (cut) {
        SKI_ALL(skg_crc_span_lane(&cs, data.data(), (uint32_t)cut, len - cut, lane));
        skg_crc_span_close(&cs, &acc);
    }
    if (len > cut) {
        SKI_ALL(skg_crc_span_lane(&cs, data.data() + cut, (uint32_t)(len - cut), 0, lane));
        skg_crc_span_close(&cs, &acc);
    }
    fprintf(res, "%u\n", ~(skb_mul(0xffffffffu, skg_shift_of(cs.power, len)) ^ acc));
    fclose(in);
    fclose(res);
    return 0;
}

int main(int argc, char **argv)
{
    SKI_ALL(skg_crc_tables(&cs, lane));
    if (argc == 4 && !strcmp(argv[1], "--shift")) return shift_mode(argv[2], argv[3]);
    if (argc == 5 && !strcmp(argv[1], "--crc")) return crc_mode(argv[2], argv[3], argv[4]);
    if (argc != 4) return 2;
    FILE *in = fopen(argv[1], "rb"), *res = fopen(argv[2], "w"), *txt = fopen(argv[3], "wb");
    if (!in || !res || !txt) return 2;
    SKI_ALL(ski_fixed_lengths(&sh, lane));
    const ski_build lit = ski_build_lit(&sh.fixed, 288), dist = ski_build_dist(&sh.fixed, 288, 32);
    SKI_BUILD(&sh, lit);
    SKI_BUILD(&sh, dist);
    uint8_t lenb[8];
    while (fread(lenb, 1, 8, in) == 8) {
        const uint64_t chunk = ski_le32(lenb), n = ski_le32(lenb + 4);
        uint8_t *image = n ? static_cast<uint8_t *>(malloc(n)) : nullptr;
        if (n && fread(image, 1, n, in) != n) return 2;
        skg_args a;
        a.image = image;
        a.n = n;
        a.S = n / chunk + (n % chunk != 0);
        a.chunk_bits = chunk * 8;
        a.chunk_shift = (uint32_t)__builtin_ctzll(a.chunk_bits);
        a.pad = 0;
        a.mem_cap = n / SKG_MIN_GAP + 1;
        std::vector<uint64_t> hdr(SKG_HDR_WORDS), u_off(a.S + 1);
        std::vector<uint32_t> u_id(a.S + 1);
        std::vector<skg_stretch> st(a.S + 1);
        std::vector<skg_member> mem(a.mem_cap);
        a.hdr = hdr.data();
        a.st = st.data();
        a.u_off = u_off.data();
        a.u_id = u_id.data();
        a.mem = mem.data();
        a.out = nullptr;
        a.capacity = 0;
        a.sym = nullptr;
        uint64_t need = 0;
        std::vector<uint8_t> out;
        std::vector<uint16_t> sym;
        for (int pass = 0; pass < 2; ++pass) { // counting, then decoding into exactly what the count asked for
            skg_search_first(a);
            for (uint64_t c = 1; c < a.S; ++c) skg_search_chunk(&sh, a, c, 0);
            for (uint64_t k = 0; k < a.S; ++k)
                if (a.st[k].start != SKG_NONE) skg_count_stretch(&sh, &walk, a, k, 0);
            skg_chain(a);
            if (pass == 0) {
                need = hdr[SKG_H_BYTES_OUT];
                out.assign(need ? need : 1, 0xa5);
                sym.assign(need ? need : 1, 0xa5a5);
                a.out = out.data();
                a.capacity = need;
                a.sym = sym.data();
                if (need == 0) { // nothing of an empty text may be touched
                    out = std::vector<uint8_t>();
                    sym = std::vector<uint16_t>();
                    a.out = reinterpret_cast<uint8_t *>(16);
                    a.sym = nullptr;
                }
                continue;
            }
            const uint64_t used = hdr[SKG_H_USED], total = hdr[SKG_H_BYTES_OUT], members = hdr[SKG_H_MEMBERS];
            if (!hdr[SKG_H_FIT]) return 3;
            for (uint64_t u = 0; u < used; ++u) skg_decode_stretch(&sh, &walk, a, u, 0);
            for (uint64_t u = 1; u < used; ++u)
                for (uint32_t i = 0; i < SKG_WINDOW; ++i) skg_window_elem(a, u, i);
            for (uint64_t g = 0; g < (total + 15) / 16; ++g) skg_resolve_granule(a, g);
            for (uint64_t q = 0; q < (total + SKG_PIECE - 1) / SKG_PIECE; ++q) skg_crc_piece(&cs, a, q, 0);
            for (uint64_t m = 0; m < members; ++m) skg_check_member(cs.power, a, m);
            skg_final(a);
        }
        const uint64_t key = hdr[SKG_H_ERROR_KEY];
        const bool bad = key != SKG_NONE;
        fprintf(res, "%llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)(bad ? key & 7 : 0),
                (unsigned long long)(bad ? key >> 3 : 0), (unsigned long long)(bad ? hdr[SKG_H_ERROR_OFFSET] : 0),
                (unsigned long long)hdr[SKG_H_MEMBERS], (unsigned long long)hdr[SKG_H_BYTES_OUT],
                (unsigned long long)hdr[SKG_H_STRETCHES], (unsigned long long)hdr[SKG_H_USED]);
        if (!bad && need) fwrite(out.data(), 1, need, txt);
        free(image);
    }
    fclose(res);
    fclose(txt);
    return 0;
}
