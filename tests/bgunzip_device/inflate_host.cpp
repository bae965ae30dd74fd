// TEST INFRASTRUCTURE ONLY: sk_inflate_block.h on the host.  Usage: inflate_host <batch> <results> <texts>
//   batch    records of: uint32 LE length, then that many bytes of a BGZF image
//   results  one line per image: error member offset members bytes_out   (error: SK_GZ_*, 0 = none)
//   texts    the texts of the images without an error, back to back
// Every image sits in an allocation of exactly its size and every text in one of exactly the sum of ISIZE, so a read or a
// write outside them is a sanitizer report.  The chain of members is walked here (the device frames in parallel, with the
// same ski_parse_member); members are decoded with the device's own ski_inflate_member, lanes one after the other.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sk_inflate_block.h"

static ski_shared sh;
static skb_shared cs;

struct entry {
    uint64_t off, out_off;
    ski_member m;
};

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *in = fopen(argv[1], "rb"), *res = fopen(argv[2], "w"), *txt = fopen(argv[3], "wb");
    if (!in || !res || !txt) return 2;
    SKI_ALL(skb_phase_crc_tables(&cs, lane));
    SKI_ALL(ski_fixed_lengths(&sh, lane));
    const ski_build lit = ski_build_lit(&sh.fixed, 288), dist = ski_build_dist(&sh.fixed, 288, 32);
    SKI_BUILD(&sh, lit);
    SKI_BUILD(&sh, dist);
    uint8_t lenb[4];
    while (fread(lenb, 1, 4, in) == 4) {
        const uint64_t n = ski_le32(lenb);
        uint8_t *image = static_cast<uint8_t *>(malloc(n ? n : 1));
        if (n && fread(image, 1, n, in) != n) return 2;
        if (n == 0) { // nothing of an empty image may be read
            free(image);
            image = nullptr;
        }
        std::vector<entry> table;
        uint64_t pos = 0, need = 0, err = 0, err_member = 0, err_off = 0;
        while (pos < n) {
            entry e;
            const uint32_t why = ski_parse_member(image, n, pos, &e.m);
            if (why != SKI_OK) {
                err = why, err_member = table.size(), err_off = pos;
                break;
            }
            e.off = pos;
            e.out_off = need;
            if (e.m.isize <= SKI_MAX_ISIZE) need += e.m.isize;
            table.push_back(e);
            pos += e.m.size;
        }
        uint8_t *out = static_cast<uint8_t *>(malloc(need ? need : 1));
        for (uint64_t k = 0; k < table.size(); ++k) {
            const entry &e = table[k];
            const uint32_t why = e.m.isize > SKI_MAX_ISIZE
                                     ? SKI_LENGTH
                                     : ski_inflate_member(&sh, &cs, image + e.off + e.m.body_off, e.m.body_len, out + e.out_off,
                                                          e.m.isize, e.m.crc, 0);
            if (why != SKI_OK) { // members come in order: the first bad one is the lowest
                err = why, err_member = k, err_off = e.off;
                break;
            }
        }
        fprintf(res, "%llu %llu %llu %llu %llu\n", (unsigned long long)err, (unsigned long long)err_member,
                (unsigned long long)err_off, (unsigned long long)table.size(), (unsigned long long)need);
        if (!err && need) fwrite(out, 1, need, txt);
        free(out);
        free(image);
    }
    fclose(res);
    fclose(txt);
    return 0;
}
