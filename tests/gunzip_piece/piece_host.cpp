// TEST INFRASTRUCTURE ONLY: the piece stages of sk_gunzip_block.h on the host.  Usage: piece_host <batch> <results> <texts>
//   batch    records of: uint32 LE chunk bytes, uint32 LE image length, uint64 LE window bytes, uint64 LE capacity,
//            uint64 LE the window a window-limited piece is repeated with (0: it ends the stream), then the image
//   results  per image a line "image <pieces>", then one line per piece:
//            status error error_member error_offset pos_bit in_member member_text member_crc members text_bytes done
//            window_limited inherited bytes_out written stretches_used max_stretch_text
//   texts    the texts of the pieces that wrote, back to back
// The image is streamed from the all-zero state with `last` set, two states alternating, until a piece is done or fails;
// a piece whose first stretch is beyond the capacity (status 2) is repeated with its need.  The stages run in the order
// of sk_gunzip_piece.hip's launches, every unit of work in turn, lanes one after the other.  Every buffer is an
// allocation of exactly its size, so a read or a write outside it is a sanitizer report.
// The same source with -DSKG_REBASE_AT=64u is piece_host_rebase.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "sk_gunzip_block.h"

static ski_shared sh;
static skg_crc_shared cs;
static skg_walk walk;
static skg_piece_walk pwalk;

static uint64_t le64(const uint8_t *p)
{
    return (uint64_t)ski_le32(p) | ((uint64_t)ski_le32(p + 4) << 32);
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[1], "rb"), *res = fopen(argv[2], "w"), *txt = fopen(argv[3], "wb");
    if (!in || !res || !txt) return 2;
    SKI_ALL(skg_crc_tables(&cs, lane));
    SKI_ALL(ski_fixed_lengths(&sh, lane));
    const ski_build lit = ski_build_lit(&sh.fixed, 288), dist = ski_build_dist(&sh.fixed, 288, 32);
    SKI_BUILD(&sh, lit);
    SKI_BUILD(&sh, dist);
    uint8_t rec[32];
    while (fread(rec, 1, 32, in) == 32) {
        const uint64_t chunk = ski_le32(rec), n = ski_le32(rec + 4), window0 = le64(rec + 8), grow = le64(rec + 24);
        uint64_t capacity = le64(rec + 16);
        std::vector<uint8_t> image(n);
        if (n && fread(image.data(), 1, n, in) != n) return 2;
        std::unique_ptr<skg_piece_state> state[2] = {std::make_unique<skg_piece_state>(), std::make_unique<skg_piece_state>()};
        memset(state[0].get(), 0, sizeof(skg_piece_state));
        std::vector<std::vector<uint64_t>> lines;
        int cur = 0;
        uint64_t window = window0;
        for (;;) {
            skg_args a;
            a.image = nullptr;
            a.n = 0;
            a.S = window / chunk + (window % chunk != 0);
            a.chunk_bits = chunk * 8;
            a.chunk_shift = (uint32_t)__builtin_ctzll(a.chunk_bits);
            a.pad = 0;
            a.mem_cap = window / SKG_MIN_GAP + 2;
            std::vector<uint64_t> hdr(SKG_HDR_WORDS), u_off(a.S + 1);
            std::vector<uint32_t> u_id(a.S + 1);
            std::vector<skg_stretch> st(a.S + 1);
            std::vector<skg_resume> rs(a.S + 1);
            std::vector<skg_member> mem(a.mem_cap);
            std::vector<uint8_t> out(capacity ? capacity : 1, 0xa5);
            std::vector<uint16_t> sym(SKG_WINDOW + capacity, 0xa5a5);
            a.hdr = hdr.data();
            a.st = st.data();
            a.u_off = u_off.data();
            a.u_id = u_id.data();
            a.mem = mem.data();
            a.sym = sym.data();
            a.out = reinterpret_cast<uint8_t *>(reinterpret_cast<uintptr_t>(out.data()) - SKG_WINDOW);
            a.capacity = capacity;
            skg_piece_args p;
            p.in = state[cur].get();
            p.out = state[cur ^ 1].get();
            p.image = image.data();
            p.image_bytes = n;
            p.image_offset = 0;
            p.window_bytes = window;
            p.text = out.data();
            p.capacity = capacity;
            p.res = rs.data();
            p.last = 1;
            p.pad = 0;
            bool closing;
            const uint32_t kind = skg_piece_window(p, &a, &closing);
            skg_piece_first(a, p, kind, closing);
            uint64_t longest = 0;
            if (kind == SKG_P_RUN) {
                for (uint32_t i = 0; i < SKG_WINDOW; ++i) a.sym[i] = p.in->history[i];
                for (uint64_t c = 1; c < a.S; ++c) skg_search_chunk(&sh, a, c, 0);
                for (uint64_t k = 0; k < a.S; ++k)
                    if (a.st[k].start != SKG_NONE) skg_count_stretch_piece(&sh, &walk, &pwalk, a, p, k, 0);
                skg_chain_piece(a, p, closing);
                if (hdr[SKG_H_FIT]) {
                    const uint64_t used = hdr[SKG_H_USED], total = hdr[SKG_H_BYTES_OUT], members = hdr[SKG_H_MEMBERS] - 1;
                    for (uint64_t u = 0; u < used; ++u) {
                        skg_decode_stretch_piece(&sh, &walk, &pwalk, a, p, u, 0);
                        if (u_off[u + 1] - u_off[u] > longest) longest = u_off[u + 1] - u_off[u];
                    }
                    for (uint64_t u = 0; u < used; ++u)
                        for (uint32_t i = 0; i < SKG_WINDOW; ++i) skg_window_elem(a, u, i);
                    for (uint64_t g = SKG_WINDOW / 16; g < (total + 15) / 16; ++g) skg_resolve_granule(a, g);
                    for (uint64_t q = SKG_WINDOW / SKG_PIECE; q < (total + SKG_PIECE - 1) / SKG_PIECE; ++q) skg_crc_piece(&cs, a, q, 0);
                    for (uint64_t m = 0; m < members; ++m) {
                        if (m) skg_check_member(cs.power, a, m);
                        else skg_check_first_piece(cs.power, a, p);
                    }
                    skg_final(a);
                }
            }
            for (uint32_t i = 0; i < SKG_WINDOW; ++i) skg_piece_history(a, p, i);
            skg_piece_publish(a, p, cs.power);
            const skg_piece_words &w = p.out->w;
            const uint64_t limited = w.status == 1 && hdr[SKG_H_P_LIMITED] && !hdr[SKG_H_P_INHERITED];
            lines.push_back({w.status, w.error, w.error_member, w.error_offset, w.pos_bit, w.in_member, w.member_text, w.member_crc,
                             w.members, w.text_bytes, w.done, limited, hdr[SKG_H_P_INHERITED], hdr[SKG_H_BYTES_OUT],
                             hdr[SKG_H_WRITTEN], hdr[SKG_H_USED], longest});
            if (hdr[SKG_H_WRITTEN] && hdr[SKG_H_BYTES_OUT]) fwrite(out.data(), 1, hdr[SKG_H_BYTES_OUT], txt);
            if (w.status == 2 && hdr[SKG_H_BYTES_OUT] > capacity) { // repeated from the same state with the need
                capacity = hdr[SKG_H_BYTES_OUT];
                continue;
            }
            if (limited && grow && window != grow) {
                window = grow;
                continue;
            }
            if (w.status || w.done || lines.size() > 100000) break;
            window = window0;
            cur ^= 1;
        }
        fprintf(res, "image %zu\n", lines.size());
        for (const auto &l : lines) {
            for (size_t i = 0; i < l.size(); ++i) fprintf(res, "%llu%c", (unsigned long long)l[i], i + 1 < l.size() ? ' ' : '\n');
        }
    }
    fclose(res);
    fclose(txt);
    return 0;
}
