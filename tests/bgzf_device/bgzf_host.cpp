// test-only: the per-block work of the device's BGZF writer (sk_bgzf.hip) on the host: the phases of sk_deflate_block.h
// and sk_bgzf_block.h with the 64 lanes run one after the other and the barriers where the kernel has them, the member
// assembled byte by byte the way the pack kernel does it.
//   bgzf_host crc FILE           the CRC-32 of each 65280-byte block of FILE, one hex word per line
//   bgzf_host crclen FILE L...   the CRC-32 of the first L bytes of FILE taken as one block, for each L
//   bgzf_host image FILE [eof]   the BGZF image of FILE on stdout (no member for an empty file), "blocks stored" on stderr
#include "sk_bgzf_block.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#define ALL_LANES(call) for (int lane = 0; lane < SKD_LANES; ++lane) { call; }

static uint32_t crc_of(skb_shared *cs, const uint8_t *p, uint32_t n)
{
    ALL_LANES(skb_phase_crc_lanes(cs, p, n, lane));
    skb_phase_crc_close(cs, n);
    return cs->crc;
}

static uint32_t deflate_block(const uint8_t *p, uint32_t n, uint32_t *out_words, skd_shared *sh, uint32_t *tok)
{
    ALL_LANES(skd_phase_clear(sh, out_words, lane));
    ALL_LANES(skd_phase_count_newlines(sh, p, n, lane));
    skd_phase_scan_segments(sh, n);
    ALL_LANES(skd_phase_line_starts(sh, p, n, lane));
    skd_phase_close_lines(sh, p, n);
    ALL_LANES(skd_phase_tokenize(sh, p, tok, lane));
    skd_phase_codes_and_header(sh, out_words);
    ALL_LANES(skd_phase_size_lines(sh, tok, lane));
    skd_phase_place_lines(sh, out_words);
    ALL_LANES(skd_phase_emit(sh, tok, out_words, lane));
    return skb_stream_bytes(sh->total_bits);
}

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    const std::string mode = argv[1];
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 1;
    std::string data;
    std::vector<char> buf(1 << 20);
    for (size_t n; (n = fread(buf.data(), 1, buf.size(), f)) > 0;) data.append(buf.data(), n);
    fclose(f);
    const uint8_t *text = (const uint8_t *)data.data();
    skb_shared *cs = new skb_shared;
    ALL_LANES(skb_phase_crc_tables(cs, lane));
    if (mode == "crclen") {
        for (int i = 3; i < argc; ++i) {
            const unsigned long n = strtoul(argv[i], nullptr, 10);
            if (n > data.size() || n > SKD_BLOCK_MAX) return 1;
            printf("%08x\n", crc_of(cs, text, (uint32_t)n));
        }
        return 0;
    }
    if (mode == "crc") {
        for (size_t at = 0; at < data.size(); at += SKD_BLOCK_MAX)
            printf("%08x\n", crc_of(cs, text + at, (uint32_t)std::min<size_t>(SKD_BLOCK_MAX, data.size() - at)));
        return 0;
    }
    if (mode != "image") return 1;
    const bool eof = argc > 3 && std::string(argv[3]) == "eof";
    std::vector<uint32_t> out_words(SKD_OUT_WORDS), tok(SKD_BLOCK_MAX + 8);
    skd_shared *sh = new skd_shared;
    std::string out;
    size_t blocks = 0, stored_blocks = 0;
    for (size_t at = 0; at < data.size(); at += SKD_BLOCK_MAX) {
        const uint32_t n = (uint32_t)std::min<size_t>(SKD_BLOCK_MAX, data.size() - at);
        const uint8_t *p = text + at;
        const uint32_t clen = deflate_block(p, n, out_words.data(), sh, tok.data());
        const uint32_t crc = crc_of(cs, p, n);
        const bool stored = skb_is_stored(clen, n);
        const uint32_t body = skb_body_bytes(clen, n), m = skb_member_bytes(body);
        const uint32_t head = SKB_HEADER_BYTES + (stored ? SKB_STORED_BYTES : 0), tail = SKB_HEADER_BYTES + body;
        const uint8_t *src = stored ? p : (const uint8_t *)out_words.data();
        for (uint32_t q = 0; q < m; ++q)
            out.push_back((char)(q < head ? skb_head_byte(q, m, n) : q < tail ? src[q - head] : skb_tail_byte(q - tail, crc, n)));
        ++blocks;
        stored_blocks += stored;
    }
    if (eof)
        for (uint32_t i = 0; i < SKB_EOF_BYTES; ++i) out.push_back((char)skb_eof_byte(i));
    fwrite(out.data(), 1, out.size(), stdout);
    fprintf(stderr, "%zu %zu\n", blocks, stored_blocks);
    return 0;
}
