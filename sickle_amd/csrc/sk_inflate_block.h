// sk_inflate_block.h -- one BGZF member back to its text: the header test, the Huffman tables, the symbol decoder, the
// token resolve and the verdict, written as functions of (lane, shared state) that the 64 lanes of one wavefront run in step.
//
// The split: reading symbols off a deflate stream is serial, so that part (ski_block_header, ski_read_lengths,
// ski_decode_batch) is UNIFORM: every lane runs it on its own copy of the state and gets the same answer; what it leaves
// in shared memory (code lengths, tokens) is the same value from every lane.  Everything else is spread over the lanes:
// the table builds (histogram, codes per length, the fill per symbol), stored blocks (a strided copy), the tokens of a
// batch (lane t owns token t) and the CRC-32 (the phases of sk_bgzf_block.h).
//
// Decoding a symbol: the low ROOT bits of the bit buffer index a primary table (entry = symbol << 4 | length); codes
// longer than ROOT, and the bit patterns an incomplete code leaves unassigned, have a zero entry and go through the
// canonical bit-by-bit search over count[] and sorted[] (bounded by 15 steps).  Codes are accepted and refused exactly as
// zlib does: over-subscribed never, incomplete only when the longest code has one bit, no codes at all only for
// distances (a block of literals).
//
// Safety: the bit buffer never reads outside [body, body + body_len), a token is queued only once its bytes are known to
// lie inside [0, isize), the copies check the span again, and every loop consumes input bits or is counted.
//
// The same source compiles for the device (sk_inflate.hip) and for the host, where SKI_ALL runs the lanes one after the
// other (tests/bgunzip_device/inflate_host.cpp).
#ifndef SK_INFLATE_BLOCK_H
#define SK_INFLATE_BLOCK_H

#include "sk_bgzf_block.h"

#define SKI_LANES 64
#define SKI_BATCH 64
#define SKI_MAX_ISIZE 65536u
#define SKI_MIN_MEMBER 26u /* 12 fixed header bytes, the 6-byte BC subfield, an empty body, the trailer */
#define SKI_LIT_ROOT 10
#define SKI_DIST_ROOT 8
#define SKI_CL_ROOT 7

// == SK_GZ_* of the C ABI
#define SKI_OK 0u
#define SKI_HEADER 1u
#define SKI_TRUNCATED 2u
#define SKI_DEFLATE 3u
#define SKI_LENGTH 4u
#define SKI_CRC 5u

#ifdef __HIPCC__
#define SKI_SYNC() __syncthreads()
#define SKI_FENCE() __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup")
#define SKI_ALL(stmt) \
    do {              \
        stmt;         \
        SKI_SYNC();   \
    } while (0)
#define SKI_BALLOT(mask, expr) (mask) = __ballot(expr)
#else
#define SKI_SYNC() ((void)0)
#define SKI_FENCE() ((void)0)
#define SKI_ALL(stmt) \
    for (int lane = 0; lane < SKI_LANES; ++lane) { stmt; }
#define SKI_BALLOT(mask, expr)                         \
    do {                                               \
        (mask) = 0;                                    \
        for (int lane = 0; lane < SKI_LANES; ++lane)   \
            if (expr) (mask) |= 1ull << lane;          \
    } while (0)
#endif

// ------------------------------------------------------------------------------------------
// framing: the member that begins at image[pos], pos < n
// ------------------------------------------------------------------------------------------
struct ski_member {
    uint32_t size;     // BSIZE + 1
    uint32_t body_off; // behind the extra field
    uint32_t body_len;
    uint32_t isize, crc;
};

SKD_FN uint8_t ski_magic(uint32_t k) { return k == 0 ? 0x1f : k == 1 ? 0x8b : k == 2 ? 8 : 4; }

SKD_FN uint32_t ski_le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
SKD_FN uint32_t ski_le32(const uint8_t *p) { return ski_le16(p) | (ski_le16(p + 2) << 16); }

// SKI_OK and *m, or why no member begins here.  What is there of 1f 8b 08 04 is compared first, so garbage is a header
// error and a cut-off file a truncation.  Reads image[pos, min(n, pos + member size)) only.
SKD_FN uint32_t ski_parse_member(const uint8_t *image, uint64_t n, uint64_t pos, ski_member *m)
{
    const uint64_t rem = n - pos;
    const uint8_t *p = image + pos;
    for (uint32_t k = 0; k < 4 && k < rem; ++k)
        if (p[k] != ski_magic(k)) return SKI_HEADER;
    if (rem < SKI_MIN_MEMBER) return SKI_TRUNCATED;
    const uint32_t end = 12 + ski_le16(p + 10);
    if (end > rem) return SKI_TRUNCATED;
    uint32_t at = 12, bsize = 0;
    bool found = false;
    while (at < end) { // at grows by 4 or more, end <= 65547
        if (at + 4 > end) return SKI_HEADER;
        const uint32_t slen = ski_le16(p + at + 2);
        if (at + 4 + slen > end) return SKI_HEADER;
        if (!found && p[at] == 'B' && p[at + 1] == 'C' && slen == 2) {
            bsize = ski_le16(p + at + 4);
            found = true;
        }
        at += 4 + slen;
    }
    if (!found) return SKI_HEADER;
    const uint32_t size = bsize + 1;
    if (size < end + SKB_TRAILER_BYTES) return SKI_HEADER;
    if (size > rem) return SKI_TRUNCATED;
    m->size = size;
    m->body_off = end;
    m->body_len = size - end - SKB_TRAILER_BYTES;
    m->crc = ski_le32(p + size - 8);
    m->isize = ski_le32(p + size - 4);
    return SKI_OK;
}

// ------------------------------------------------------------------------------------------
// shared state
// ------------------------------------------------------------------------------------------
struct ski_tables {
    uint16_t lit[1 << SKI_LIT_ROOT];
    uint16_t dist[1 << SKI_DIST_ROOT];
    uint16_t lit_sorted[288], dist_sorted[32]; // symbols by (length, symbol)
    uint16_t lit_count[16], dist_count[16];    // codes of each length
};

struct ski_shared {
    ski_tables fixed, dyn;
    uint16_t cl[1 << SKI_CL_ROOT];
    uint16_t cl_sorted[20], cl_count[16];
    uint16_t code[320]; // a build's canonical codes
    uint8_t lens[320];  // the code lengths being built from: 19, then HLIT + HDIST
    uint32_t hist[16];
    uint32_t bad; // the build's verdict
    uint32_t tok_pos[SKI_BATCH], tok_len[SKI_BATCH], tok_arg[SKI_BATCH]; // len 0: literal arg; else a copy from arg back
};

// modes of ski_state
#define SKI_M_HEADER 0u
#define SKI_M_HUFF 1u
#define SKI_M_STORED 2u
#define SKI_M_DYNAMIC 3u
#define SKI_M_DONE 4u
#define SKI_M_ERROR 5u

struct ski_state {
    const uint8_t *body;
    uint64_t buf;
    uint32_t nbits, in, end; // valid bits of buf, next byte, body_len
    uint32_t pos, isize;     // text produced, text stated
    uint32_t mode, reason, final, fixed;
    uint32_t stored_src, stored_len;
    uint32_t nlen, ndist;
};

// ------------------------------------------------------------------------------------------
// the bit buffer
// ------------------------------------------------------------------------------------------
SKD_FN void ski_refill(ski_state *s)
{
    if (s->nbits > 48) return;
    if (s->in + 8 <= s->end) {
        uint64_t w;
        memcpy(&w, s->body + s->in, 8);
        s->buf |= w << s->nbits; // the bits above nbits + 8 adv are those of the bytes that come next: the same again later
        const uint32_t adv = (63 - s->nbits) >> 3;
        s->in += adv;
        s->nbits += adv << 3;
        return;
    }
    while (s->nbits <= 56 && s->in < s->end) {
        s->buf |= (uint64_t)s->body[s->in++] << s->nbits;
        s->nbits += 8;
    }
}

SKD_FN void ski_fail(ski_state *s, uint32_t reason)
{
    s->mode = SKI_M_ERROR;
    s->reason = reason;
}

// k <= 32 bits off the buffer; false (and the state failed) when the body has no more
SKD_FN bool ski_take(ski_state *s, uint32_t k, uint32_t *v)
{
    if (k > s->nbits) {
        ski_fail(s, SKI_DEFLATE);
        return false;
    }
    *v = (uint32_t)(s->buf & ((1ull << k) - 1));
    s->buf >>= k;
    s->nbits -= k;
    return true;
}

// one symbol, or -1: a bit pattern without a code, or bits beyond the body
SKD_FN int ski_symbol(ski_state *s, const uint16_t *primary, uint32_t root, const uint16_t *sorted, const uint16_t *count)
{
    const uint32_t e = primary[s->buf & ((1u << root) - 1)], l = e & 15u;
    if (l) {
        if (l > s->nbits) return -1;
        s->buf >>= l;
        s->nbits -= l;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= 15; ++len) {
        if (len > s->nbits) return -1;
        code |= (int)((s->buf >> (len - 1)) & 1u);
        const int cnt = count[len];
        if (code - cnt < first) {
            s->buf >>= len;
            s->nbits -= len;
            return sorted[index + (code - first)];
        }
        index += cnt;
        first = (first + cnt) << 1;
        code <<= 1;
    }
    return -1;
}

// ------------------------------------------------------------------------------------------
// table build: four phases over sh->lens + lens_at, a barrier after each
// ------------------------------------------------------------------------------------------
struct ski_build {
    uint32_t lens_at, nsym, root, is_cl;
    uint16_t *primary, *sorted, *count;
};

SKD_FN void ski_build_clear(ski_shared *sh, const ski_build &b, int lane)
{
    if (lane < 16) sh->hist[lane] = 0;
    for (uint32_t i = (uint32_t)lane; i < (1u << b.root); i += SKI_LANES) b.primary[i] = 0;
}

SKD_FN void ski_build_histogram(ski_shared *sh, const ski_build &b, int lane)
{
    for (uint32_t s = (uint32_t)lane; s < b.nsym; s += SKI_LANES) SKD_ATOMIC_ADD(&sh->hist[sh->lens[b.lens_at + s] & 15u], 1u);
}

// lane L = 1..15: where the codes of length L start and which symbols get them; lane 0: is this a code zlib takes
SKD_FN void ski_build_codes(ski_shared *sh, const ski_build &b, int lane)
{
    if (lane == 0) {
        int left = 1, max = 0;
        bool over = false;
        for (int l = 1; l <= 15; ++l) {
            left = (left << 1) - (int)sh->hist[l];
            if (left < 0) {
                over = true;
                break;
            }
            if (sh->hist[l]) max = l;
        }
        sh->bad = over || (max != 0 && left > 0 && (b.is_cl || max != 1));
        b.count[0] = 0;
    } else if (lane < 16) {
        uint32_t code = 0, off = 0;
        for (int l = 1; l < lane; ++l) {
            code = (code + sh->hist[l]) << 1;
            off += sh->hist[l];
        }
        b.count[lane] = (uint16_t)sh->hist[lane];
        if (sh->hist[lane])
            for (uint32_t s = 0; s < b.nsym; ++s)
                if (sh->lens[b.lens_at + s] == (uint32_t)lane) {
                    b.sorted[off++] = (uint16_t)s; // off stays below nsym: it counts symbols
                    sh->code[s] = (uint16_t)code++;
                }
    }
}

SKD_FN void ski_build_fill(ski_shared *sh, const ski_build &b, int lane)
{
    for (uint32_t s = (uint32_t)lane; s < b.nsym; s += SKI_LANES) {
        const uint32_t l = sh->lens[b.lens_at + s];
        if (l == 0 || l > b.root) continue;
        uint32_t c = sh->code[s], r = 0;
        for (uint32_t k = 0; k < l; ++k) r |= ((c >> k) & 1u) << (l - 1 - k); // the code leaves its first bit first
        for (uint32_t i = r; i < (1u << b.root); i += 1u << l) b.primary[i] = (uint16_t)((s << 4) | l);
    }
}

#define SKI_BUILD(sh, b)                                  \
    do {                                                  \
        SKI_ALL(ski_build_clear((sh), (b), lane));        \
        SKI_ALL(ski_build_histogram((sh), (b), lane));    \
        SKI_ALL(ski_build_codes((sh), (b), lane));        \
        SKI_ALL(ski_build_fill((sh), (b), lane));         \
    } while (0)

SKD_FN ski_build ski_build_lit(ski_tables *t, uint32_t nsym)
{
    ski_build b = {0, nsym, SKI_LIT_ROOT, 0, t->lit, t->lit_sorted, t->lit_count};
    return b;
}
SKD_FN ski_build ski_build_dist(ski_tables *t, uint32_t at, uint32_t nsym)
{
    ski_build b = {at, nsym, SKI_DIST_ROOT, 0, t->dist, t->dist_sorted, t->dist_count};
    return b;
}

// the fixed code's lengths (RFC 1951 3.2.6): 288 literal/length symbols, then 32 distance symbols
SKD_FN void ski_fixed_lengths(ski_shared *sh, int lane)
{
    for (uint32_t s = (uint32_t)lane; s < 320; s += SKI_LANES)
        sh->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
}

// ------------------------------------------------------------------------------------------
// the uniform part
// ------------------------------------------------------------------------------------------
SKD_FN void ski_begin(ski_state *s, const uint8_t *body, uint32_t body_len, uint32_t isize)
{
    s->body = body;
    s->buf = 0;
    s->nbits = 0;
    s->in = 0;
    s->end = body_len;
    s->pos = 0;
    s->isize = isize;
    s->mode = SKI_M_HEADER;
    s->reason = SKI_OK;
    s->final = s->fixed = 0;
    s->stored_src = s->stored_len = 0;
    s->nlen = s->ndist = 0;
}

SKD_FN uint8_t ski_cl_order(uint32_t i) { return (uint8_t)"\x10\x11\x12\x00\x08\x07\x09\x06\x0a\x05\x0b\x04\x0c\x03\x0d\x02\x0e\x01\x0f"[i]; }

// BFINAL, BTYPE and what belongs to the type: a stored block's lengths, or the code-length code's lengths into sh->lens
SKD_FN void ski_block_header(ski_shared *sh, ski_state *s)
{
    uint32_t v;
    ski_refill(s);
    if (!ski_take(s, 3, &v)) return;
    s->final = v & 1u;
    const uint32_t type = v >> 1;
    if (type == 0) {
        if (!ski_take(s, s->nbits & 7u, &v)) return; // the buffer holds whole bytes beyond the cursor
        ski_refill(s);
        if (!ski_take(s, 32, &v)) return;
        if ((v & 0xffffu) != (~v >> 16)) return ski_fail(s, SKI_DEFLATE);
        s->stored_len = v & 0xffffu;
        s->stored_src = s->in - (s->nbits >> 3);
        if (s->stored_src + s->stored_len > s->end) return ski_fail(s, SKI_DEFLATE);
        if (s->pos + s->stored_len > s->isize) return ski_fail(s, SKI_LENGTH);
        s->mode = SKI_M_STORED;
    } else if (type == 1) {
        s->fixed = 1;
        s->mode = SKI_M_HUFF;
    } else if (type == 2) {
        if (!ski_take(s, 14, &v)) return;
        s->nlen = 257 + (v & 31u);
        s->ndist = 1 + ((v >> 5) & 31u);
        const uint32_t ncl = 4 + (v >> 10);
        if (s->nlen > 286 || s->ndist > 30) return ski_fail(s, SKI_DEFLATE);
        for (uint32_t i = 0; i < 19; ++i) {
            uint32_t l = 0;
            if (i < ncl) {
                ski_refill(s);
                if (!ski_take(s, 3, &l)) return;
            }
            sh->lens[ski_cl_order(i)] = (uint8_t)l;
        }
        s->fixed = 0;
        s->mode = SKI_M_DYNAMIC;
    } else {
        ski_fail(s, SKI_DEFLATE);
    }
}

// the HLIT + HDIST code lengths, through the code-length code, into sh->lens
SKD_FN void ski_read_lengths(ski_shared *sh, ski_state *s)
{
    const uint32_t total = s->nlen + s->ndist;
    uint32_t at = 0;
    while (at < total) { // a symbol of 1 bit or more each time round
        ski_refill(s);
        const int sym = ski_symbol(s, sh->cl, SKI_CL_ROOT, sh->cl_sorted, sh->cl_count);
        if (sym < 0) return ski_fail(s, SKI_DEFLATE);
        if (sym < 16) {
            sh->lens[at++] = (uint8_t)sym;
            continue;
        }
        uint32_t rep, len = 0;
        if (sym == 16) {
            if (at == 0) return ski_fail(s, SKI_DEFLATE);
            len = sh->lens[at - 1];
            if (!ski_take(s, 2, &rep)) return;
            rep += 3;
        } else if (sym == 17) {
            if (!ski_take(s, 3, &rep)) return;
            rep += 3;
        } else {
            if (!ski_take(s, 7, &rep)) return;
            rep += 11;
        }
        if (at + rep > total) return ski_fail(s, SKI_DEFLATE);
        while (rep--) sh->lens[at++] = (uint8_t)len;
    }
    if (sh->lens[256] == 0) return ski_fail(s, SKI_DEFLATE); // no end-of-block code
    s->mode = SKI_M_HUFF;
}

// symbols of the current block into tokens until the batch is full, the block ends or the stream fails -> tokens queued
SKD_FN uint32_t ski_decode_batch(ski_shared *sh, ski_state *s, const ski_tables *t)
{
    uint32_t n = 0;
    while (n < SKI_BATCH) {
        ski_refill(s); // 56 bits or all there is: a length, its extra, a distance and its extra are 48 at most
        int sym = ski_symbol(s, t->lit, SKI_LIT_ROOT, t->lit_sorted, t->lit_count);
        if (sym < 0) {
            ski_fail(s, SKI_DEFLATE);
            break;
        }
        if (sym < 256) {
            if (s->pos >= s->isize) {
                ski_fail(s, SKI_LENGTH);
                break;
            }
            sh->tok_pos[n] = s->pos++;
            sh->tok_len[n] = 0;
            sh->tok_arg[n++] = (uint32_t)sym;
            continue;
        }
        if (sym == 256) {
            s->mode = s->final ? SKI_M_DONE : SKI_M_HEADER;
            break;
        }
        sym -= 257;
        if (sym >= 29) {
            ski_fail(s, SKI_DEFLATE);
            break;
        }
        uint32_t len, dist, x = 0;
        if (sym < 8) {
            len = 3 + (uint32_t)sym;
        } else if (sym == 28) {
            len = 258;
        } else {
            const uint32_t eb = ((uint32_t)sym >> 2) - 1;
            if (!ski_take(s, eb, &x)) break;
            len = 3 + ((4 + ((uint32_t)sym & 3u)) << eb) + x;
        }
        const int ds = ski_symbol(s, t->dist, SKI_DIST_ROOT, t->dist_sorted, t->dist_count);
        if (ds < 0 || ds >= 30) {
            ski_fail(s, SKI_DEFLATE);
            break;
        }
        if (ds < 4) {
            dist = 1 + (uint32_t)ds;
        } else {
            const uint32_t eb = ((uint32_t)ds >> 1) - 1;
            if (!ski_take(s, eb, &x)) break;
            dist = 1 + ((2 + ((uint32_t)ds & 1u)) << eb) + x;
        }
        if (dist > s->pos) {
            ski_fail(s, SKI_DEFLATE);
            break;
        }
        if (s->pos + len > s->isize) {
            ski_fail(s, SKI_LENGTH);
            break;
        }
        sh->tok_pos[n] = s->pos;
        sh->tok_len[n] = len;
        sh->tok_arg[n++] = dist;
        s->pos += len;
    }
    return n;
}

// ------------------------------------------------------------------------------------------
// the lanes' part
// ------------------------------------------------------------------------------------------
// a stored block: out[pos + i] = body[src + i], strided over the lanes
SKD_FN void ski_copy_stored(const ski_state *s, uint8_t *out, int lane)
{
    for (uint32_t i = (uint32_t)lane; i < s->stored_len; i += SKI_LANES)
        if (s->pos + i < s->isize && s->stored_src + i < s->end) out[s->pos + i] = s->body[s->stored_src + i];
}

// one round of a batch for token `lane`: it goes iff it is not done and its source ends at or below the finished prefix,
// i.e. the start of the first token not done (that token itself always qualifies; a copy that overlaps itself can only be
// that one, and goes byte by byte like every copy here).  -> done in this round
SKD_FN bool ski_resolve_lane(const ski_shared *sh, uint8_t *out, uint32_t isize, uint32_t n, uint64_t done, int lane)
{
    if ((uint32_t)lane >= n || ((done >> lane) & 1u)) return false;
    const uint32_t first = (uint32_t)__builtin_ctzll(~done); // < n: the caller stops when all are done
    const uint32_t finished = sh->tok_pos[first];
    const uint32_t pos = sh->tok_pos[lane], len = sh->tok_len[lane], arg = sh->tok_arg[lane];
    if (len == 0) {
        if (pos < isize) out[pos] = (uint8_t)arg;
        return true;
    }
    if (pos - arg + (len < arg ? len : arg) > finished) return false;
    if (arg > pos || pos + len > isize) return true; // never queued (ski_decode_batch): nothing is copied
    for (uint32_t k = 0; k < len; ++k) out[pos + k] = out[pos - arg + k];
    return true;
}

// ------------------------------------------------------------------------------------------
// a member: body -> out[0, isize), -> SKI_OK or why not.  cs: its tables built (skb_phase_crc_tables); sh->fixed built.
// ------------------------------------------------------------------------------------------
SKD_FN uint32_t ski_inflate_member(ski_shared *sh, skb_shared *cs, const uint8_t *body, uint32_t body_len, uint8_t *out,
                                   uint32_t isize, uint32_t crc, int lane)
{
    ski_state s;
    ski_begin(&s, body, body_len, isize);
    (void)lane;
    while (s.mode != SKI_M_DONE && s.mode != SKI_M_ERROR) { // every turn takes bits off the body
        if (s.mode == SKI_M_HEADER) {
            SKI_SYNC(); // the lengths of the block before are no longer read
            ski_block_header(sh, &s);
            SKI_SYNC();
            if (s.mode == SKI_M_DYNAMIC) {
                const ski_build cl = {0, 19, SKI_CL_ROOT, 1, sh->cl, sh->cl_sorted, sh->cl_count};
                SKI_BUILD(sh, cl);
                if (sh->bad) {
                    ski_fail(&s, SKI_DEFLATE);
                    break;
                }
                SKI_SYNC();
                ski_read_lengths(sh, &s);
                SKI_SYNC();
                if (s.mode == SKI_M_ERROR) break;
                const ski_build lit = ski_build_lit(&sh->dyn, s.nlen);
                SKI_BUILD(sh, lit);
                uint32_t bad = sh->bad;
                SKI_SYNC();
                const ski_build dist = ski_build_dist(&sh->dyn, s.nlen, s.ndist);
                SKI_BUILD(sh, dist);
                bad |= sh->bad;
                if (bad) {
                    ski_fail(&s, SKI_DEFLATE);
                    break;
                }
            }
        }
        if (s.mode == SKI_M_STORED) {
            SKI_ALL(ski_copy_stored(&s, out, lane));
            SKI_FENCE();
            s.pos += s.stored_len;
            s.in = s.stored_src + s.stored_len;
            s.buf = 0;
            s.nbits = 0;
            s.mode = s.final ? SKI_M_DONE : SKI_M_HEADER;
        } else if (s.mode == SKI_M_HUFF) {
            SKI_SYNC(); // the batch before has been read
            const uint32_t n = ski_decode_batch(sh, &s, s.fixed ? &sh->fixed : &sh->dyn);
            SKI_SYNC();
            const uint64_t all = n == 64 ? ~0ull : (1ull << n) - 1;
            uint64_t done = 0;
            while (done != all) { // the first token not done goes in every round: n rounds at most
                uint64_t got;
                SKI_BALLOT(got, ski_resolve_lane(sh, out, isize, n, done, lane));
                done |= got;
                SKI_FENCE(); // what this round wrote is what the next round's lanes read
            }
        }
    }
    if (s.mode == SKI_M_ERROR) return s.reason;
    if (s.pos != isize) return SKI_LENGTH;
    SKI_FENCE();
    SKI_ALL(skb_phase_crc_lanes(cs, out, isize, lane));
    SKI_ALL(if (lane == 0) skb_phase_crc_close(cs, isize));
    return cs->crc == crc ? SKI_OK : SKI_CRC;
}

#endif
