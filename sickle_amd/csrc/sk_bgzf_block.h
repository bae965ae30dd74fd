// sk_bgzf_block.h -- what turns one block's deflate stream (sk_deflate_block.h) into a BGZF member: the CRC-32 of the
// block's text, written as PHASES that the 64 lanes of one wavefront run in step, and the member's framing bytes.
//
// CRC-32 (the gzip polynomial, reflected: 0xEDB88320) without a carry-less multiply: every lane runs the byte-wise table
// CRC (the table in LDS) over its contiguous share of the block from a zero register, which is linear in the text; the
// register of lane l then has to pass over the bytes behind its share, i.e. be multiplied by x^(8 * bytes behind) mod P
// (zlib's crc32_combine idea).  That multiply is a 32-step shift/xor, the power comes from the squares x^(8 * 2^j) kept
// in LDS, and every lane does it for itself, so the shares combine with one XOR over the lanes:
//   crc = ~( 0xffffffff * x^(8 n)  ^  XOR_l  raw_l * x^(8 (n - end_l)) )
//
// The same source compiles for the device (sk_bgzf.hip) and for the host, where a test harness runs the lanes one after
// the other (tests/bgzf_device/bgzf_host.cpp).
#ifndef SK_BGZF_BLOCK_H
#define SK_BGZF_BLOCK_H

#include "sk_deflate_block.h"

#define SKB_POLY 0xedb88320u
#define SKB_POWERS 17       /* x^(8 * 2^j), j = 0..16: shifts of up to 2^17 - 1 bytes */
#define SKB_HEADER_BYTES 18 /* gzip header with the BGZF extra field */
#define SKB_TRAILER_BYTES 8 /* CRC-32, ISIZE */
#define SKB_STORED_BYTES 5  /* 01 LEN NLEN of a stored block */
#define SKB_EOF_BYTES 28    /* the empty member that ends a BGZF file */
#define SKB_STORED_FLAG 0x80000000u

struct skb_shared {
    uint32_t table[256];        // of the byte-wise CRC
    uint32_t power[SKB_POWERS]; // x^(8 * 2^j) mod P
    uint32_t lane_crc[SKD_LANES];
    uint32_t crc;
};

// a * b mod P, polynomials over GF(2) in the reflected representation (bit 31 = x^0): 32 shift/xor steps
SKD_FN uint32_t skb_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= (a >> i) & 1u ? b : 0u;
        b = (b >> 1) ^ (b & 1u ? SKB_POLY : 0u);
    }
    return p;
}

// x^(8 k) mod P from the squares in sh->power; k < 2^SKB_POWERS
SKD_FN uint32_t skb_shift_of(const skb_shared *sh, uint32_t k)
{
    uint32_t r = 0x80000000u; // x^0
    for (int j = 0; j < SKB_POWERS; ++j)
        if ((k >> j) & 1u) r = skb_mul(r, sh->power[j]);
    return r;
}

// ---- phase A, once per workgroup: the byte table (4 entries per lane) and the powers (lane j squares j times)
SKD_FN void skb_phase_crc_tables(skb_shared *sh, int lane)
{
    for (int i = lane; i < 256; i += SKD_LANES) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (c & 1u ? SKB_POLY : 0u);
        sh->table[i] = c;
    }
    if (lane < SKB_POWERS) {
        uint32_t e = 0x00800000u; // x^8
        for (int j = 0; j < lane; ++j) e = skb_mul(e, e);
        sh->power[lane] = e;
    }
}

// ---- phase B: each lane's share (the segments of skd_phase_count_newlines), shifted to the end of the block
SKD_FN void skb_phase_crc_lanes(skb_shared *sh, const uint8_t *p, uint32_t n, int lane)
{
    const uint32_t seg = (n + SKD_LANES - 1) / SKD_LANES;
    uint32_t lo = (uint32_t)lane * seg, hi = lo + seg < n ? lo + seg : n;
    if (lo > n) lo = n;
    uint32_t c = 0;
    for (uint32_t i = lo; i < hi; ++i) c = sh->table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    sh->lane_crc[lane] = hi > lo ? skb_mul(c, skb_shift_of(sh, n - hi)) : 0u;
}

// ---- phase C (lane 0): the initial register shifted over the whole block, the lanes' terms, the final inversion
SKD_FN void skb_phase_crc_close(skb_shared *sh, uint32_t n)
{
    uint32_t c = skb_mul(0xffffffffu, skb_shift_of(sh, n));
    for (int l = 0; l < SKD_LANES; ++l) c ^= sh->lane_crc[l];
    sh->crc = ~c;
}

// ---- framing.  clen: bytes of the block's deflate stream, 0 when it did not fit its slot (sh.total_bits beyond the slot)
SKD_FN uint32_t skb_stream_bytes(uint32_t total_bits)
{
    return total_bits > (SKD_OUT_WORDS - 2) * 32u ? 0u : (total_bits + 7) / 8;
}
// stored iff the stream did not fit or does not pay: the rule of the CLI's writer and of tests/cpu_shim/gpu_deflate_sim.cpp
SKD_FN bool skb_is_stored(uint32_t clen, uint32_t n) { return clen == 0 || clen >= n + SKB_STORED_BYTES; }
SKD_FN uint32_t skb_body_bytes(uint32_t clen, uint32_t n) { return skb_is_stored(clen, n) ? n + SKB_STORED_BYTES : clen; }
SKD_FN uint32_t skb_member_bytes(uint32_t body) { return SKB_HEADER_BYTES + body + SKB_TRAILER_BYTES; }

// byte q of a member's head: the 18 header bytes, then for a stored block of n bytes its 01 LEN NLEN
SKD_FN uint8_t skb_head_byte(uint32_t q, uint32_t member_bytes, uint32_t n)
{
    const uint32_t bsize = member_bytes - 1;
    switch (q) {
    case 0: return 0x1f;
    case 1: return 0x8b;
    case 2: return 8;
    case 3: return 4;
    case 9: return 0xff;
    case 10: return 6;
    case 12: return 'B';
    case 13: return 'C';
    case 14: return 2;
    case 16: return (uint8_t)bsize;
    case 17: return (uint8_t)(bsize >> 8);
    case 18: return 1;
    case 19: return (uint8_t)n;
    case 20: return (uint8_t)(n >> 8);
    case 21: return (uint8_t)~n;
    case 22: return (uint8_t)(~n >> 8);
    default: return 0;
    }
}
// byte k (0..7) of the trailer: CRC-32, ISIZE, little endian
SKD_FN uint8_t skb_tail_byte(uint32_t k, uint32_t crc, uint32_t n) { return (uint8_t)((k < 4 ? crc : n) >> (8 * (k & 3))); }
// byte i (0..27) of the end-of-file member: an empty fixed-Huffman block (03 00), CRC 0, ISIZE 0
SKD_FN uint8_t skb_eof_byte(uint32_t i) { return i < 18 ? skb_head_byte(i, SKB_EOF_BYTES, 0) : i == 18 ? 3 : 0; }

#endif
