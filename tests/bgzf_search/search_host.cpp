// test-only: the per-block work of the device's BGZF writer with SK_BGZF_SEARCH (sk_bgzf.hip, sk_bgzf_search_block_kernel)
// on the host: the phases of sk_bgzf_search.h, sk_deflate_block.h and sk_bgzf_block.h with the 64 lanes run one after
// the other and the barriers where the kernel has them, the member assembled byte by byte the way the pack kernel does it.
//   search_host image FILE [eof] [rev]   the BGZF image of FILE on stdout (no member for an empty file), "blocks stored"
//                                        on stderr
//   search_host tokens FILE [rev]        every match token, one per line: block, position in the block, length, distance,
//                                        end of the position's line
// rev: the lanes run in the order 63..0 instead of 0..63.
#include "sk_bgzf_block.h"
#include "sk_bgzf_search.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <thread>
#include <vector>

static bool g_rev = false;
#define ALL_LANES(call) for (int k_ = 0; k_ < SKD_LANES; ++k_) { const int lane = g_rev ? SKD_LANES - 1 - k_ : k_; call; }

struct state {
    skb_shared cs;
    skd_shared sh;
    sks_shared ss;
};

static uint32_t crc_of(skb_shared *cs, const uint8_t *p, uint32_t n)
{
    ALL_LANES(skb_phase_crc_lanes(cs, p, n, lane));
    skb_phase_crc_close(cs, n);
    return cs->crc;
}

static uint32_t deflate_block(const uint8_t *p, uint32_t n, uint32_t *out_words, skd_shared *sh, sks_shared *ss, uint32_t *cand,
                              uint32_t *tok)
{
    ALL_LANES(skd_phase_clear(sh, out_words, lane));
    ALL_LANES(sks_phase_clear(ss, lane));
    ALL_LANES(skd_phase_count_newlines(sh, p, n, lane));
    skd_phase_scan_segments(sh, n);
    ALL_LANES(skd_phase_line_starts(sh, p, n, lane));
    skd_phase_close_lines(sh, p, n);
    for (uint32_t c = 0; c * SKS_CHUNK < n; ++c) {
        ALL_LANES(sks_phase_candidates(sh, ss, p, n, c, cand, lane));
        ALL_LANES(sks_phase_insert(ss, p, n, c, lane));
    }
    ALL_LANES(sks_phase_tokenize(sh, p, cand, tok, lane));
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
    bool eof = false;
    for (int i = 3; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "eof") eof = true;
        else if (a == "rev") g_rev = true;
        else return 1;
    }
    if (mode != "image" && mode != "tokens") return 1;
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 1;
    std::string data;
    std::vector<char> buf(1 << 20);
    for (size_t n; (n = fread(buf.data(), 1, buf.size(), f)) > 0;) data.append(buf.data(), n);
    fclose(f);
    const uint8_t *text = (const uint8_t *)data.data();
    // the blocks are independent: worker w of W takes blocks w, w + W, ... with a state of its own, which it does not clean
    // between them, and the pieces are put together in block order afterwards
    const size_t n_blocks = (data.size() + SKD_BLOCK_MAX - 1) / SKD_BLOCK_MAX;
    const unsigned workers = (unsigned)std::max<size_t>(1, std::min<size_t>({8, std::thread::hardware_concurrency(), n_blocks}));
    std::vector<std::string> piece(n_blocks);
    std::vector<char> is_stored(n_blocks, 0);
    std::atomic<bool> bad(false);
    auto work = [&](unsigned first) {
        std::unique_ptr<state> st(new state);
        skb_shared *cs = &st->cs;
        skd_shared *sh = &st->sh;
        sks_shared *ss = &st->ss;
        std::vector<uint32_t> out_words(SKD_OUT_WORDS), tok(SKD_BLOCK_MAX + 8), cand(SKD_BLOCK_MAX + 8);
        ALL_LANES(skb_phase_crc_tables(cs, lane));
        // what a block leaves behind must not reach the next one: start from a table and candidates that are all wrong
        std::fill(ss->way2, ss->way2 + SKS_BUCKETS * SKS_WAYS / 2, 0x00010001u);
        std::fill(cand.begin(), cand.end(), skd_match(258, 1));
        for (size_t b = first; b < n_blocks; b += workers) {
            const size_t at = b * SKD_BLOCK_MAX;
            const uint32_t n = (uint32_t)std::min<size_t>(SKD_BLOCK_MAX, data.size() - at);
            const uint8_t *p = text + at;
            const uint32_t clen = deflate_block(p, n, out_words.data(), sh, ss, cand.data(), tok.data());
            std::string &out = piece[b];
            if (mode == "tokens") {
                char line[96];
                for (uint32_t l = 0; l < sh->n_lines; ++l) {
                    uint32_t j = sh->line_start[l];
                    for (uint32_t k = 0; k < sh->line_tokens[l]; ++k) {
                        const uint32_t t = tok[sh->line_start[l] + k];
                        if (t >> 31) {
                            const uint32_t len = ((t >> 15) & 0xffffu) + 3, // bits 23..30 are zero in a sound token
                                           dist = (t & 0x7fff) + 1;
                            snprintf(line, sizeof line, "%zu %u %u %u %u\n", b, j, len, dist, sh->line_start[l + 1]);
                            out += line;
                            j += len;
                        } else {
                            ++j;
                        }
                    }
                    if (j != sh->line_start[l + 1]) bad = true; // the tokens of a line cover it exactly
                }
                continue;
            }
            const uint32_t crc = crc_of(cs, p, n);
            const bool stored = skb_is_stored(clen, n);
            const uint32_t body = skb_body_bytes(clen, n), m = skb_member_bytes(body);
            const uint32_t head = SKB_HEADER_BYTES + (stored ? SKB_STORED_BYTES : 0), tail = SKB_HEADER_BYTES + body;
            const uint8_t *src = stored ? p : (const uint8_t *)out_words.data();
            for (uint32_t q = 0; q < m; ++q)
                out.push_back((char)(q < head ? skb_head_byte(q, m, n) : q < tail ? src[q - head] : skb_tail_byte(q - tail, crc, n)));
            is_stored[b] = stored;
        }
    };
    std::vector<std::thread> pool;
    for (unsigned w = 1; w < workers; ++w) pool.emplace_back(work, w);
    work(0);
    for (auto &t : pool) t.join();
    if (bad) return 2;
    size_t stored_blocks = 0;
    for (size_t b = 0; b < n_blocks; ++b) {
        fwrite(piece[b].data(), 1, piece[b].size(), stdout);
        stored_blocks += is_stored[b];
    }
    if (mode == "tokens") return 0;
    if (eof)
        for (uint32_t i = 0; i < SKB_EOF_BYTES; ++i) fputc(skb_eof_byte(i), stdout);
    fprintf(stderr, "%zu %zu\n", n_blocks, stored_blocks);
    return 0;
}
