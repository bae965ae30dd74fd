// sk_gunzip_block.h -- plain gzip (RFC 1952 members of any size) back to its text, in parallel over one deflate stream
// (Kerbiriou & Chikhi 2019; the host version is host/GzParallel.cpp).  The image is cut into chunks; per chunk a block
// start is GUESSED (skg_search_chunk), every guessed start is decoded for its lengths until it arrives exactly at a later
// guess (skg_walk, count), the chain of stretches from bit 0 is walked (skg_chain), its stretches are decoded into 16-bit
// symbols -- a literal, or 256 + j = "byte j of the 32 KiB before my start" -- (skg_walk, decode), the placeholders are
// filled in (skg_window_elem, skg_resolve_granule), and every member's CRC-32 and ISIZE are checked (skg_crc_piece,
// skg_check_member, skg_final).  Correctness never rests on a guess: a wrong one is never arrived at, or fails unused.
//
// The stages are functions of (unit of work, lane, shared state): sk_gunzip.hip launches them as kernels, and
// tests/gunzip_device/gunzip_host.cpp runs them on the host, lanes one after the other.  Huffman tables, the symbol
// reader and the table builds are those of sk_inflate_block.h; its ski_state addresses 32 bits, so the reader is re-based
// on the image as it goes (skg_rebase).
#ifndef SK_GUNZIP_BLOCK_H
#define SK_GUNZIP_BLOCK_H

#include "sk_inflate_block.h"

#define SKG_NONE (~0ull)
#define SKG_WINDOW 32768
#define SKG_UNKNOWN 256u             /* symbol 256 + j: byte j of the window before the stretch */
#define SKG_POWERS 34                /* x^(8 * 2^j), j = 0..33: shifts of up to 2^34 - 1 bytes */
#define SKG_PIECE 32768u             /* text bytes per CRC piece */
#define SKG_MIN_GAP 18u              /* two members' trailers lie this far apart at least */
#define SKG_TRY_CAP (4u << 20)       /* a guessed block that decodes more text than this is taken for nonsense */
#ifndef SKG_REBASE_AT
#define SKG_REBASE_AT (1u << 24)     /* skg_rebase moves the reader's base once s.in reaches this (a test harness lowers it) */
#endif
#define SKG_HDR_WORDS 32u
#define SKG_H_BYTES_IN 0
#define SKG_H_MEMBERS 1
#define SKG_H_BYTES_OUT 2
#define SKG_H_STRETCHES 3
#define SKG_H_USED 4
#define SKG_H_FIT 5          // count-only, or the text is within the capacity: the later stages write
#define SKG_H_ERROR_KEY 6    // (member << 3) | SK_GZ_* of the lowest failure, or ~0 (atomicMin)
#define SKG_H_ERROR_OFFSET 7 // skg_final: its byte offset
#define SKG_H_CHAIN_KEY 8    // the failure that stopped the chain, or ~0
#define SKG_H_CHAIN_OFFSET 9
#define SKG_H_DECODED 10     // the call decodes (out != NULL)
#define SKG_H_WRITTEN 11     // skg_final: 1 iff the call decoded, without an error, a text within the capacity

#define SKG_S_JOIN 0u  // ended exactly on a later stretch's start
#define SKG_S_END 1u   // ended with the image, behind a trailer
#define SKG_S_ERROR 2u

#ifdef __HIPCC__
// a value kept out of the scalar registers, which the walk's uniform state fills: one the lanes alone use, or a cold one
#define SKG_PER_LANE(x) asm volatile("" : "+v"(x))
#define SKG_ATOMIC_MIN64(p, v) atomicMin(reinterpret_cast<unsigned long long *>(p), (unsigned long long)(v))
#define SKG_ATOMIC_XOR(p, v) atomicXor((p), (v))
#else
#define SKG_PER_LANE(x) ((void)0)
#define SKG_ATOMIC_MIN64(p, v) (*(p) = *(p) < (uint64_t)(v) ? *(p) : (uint64_t)(v))
#define SKG_ATOMIC_XOR(p, v) (*(p) ^= (v))
#endif

struct skg_stretch { // 128 bytes
    // search
    uint64_t start; // bit, or SKG_NONE
    // count
    uint64_t end, len, tail; // bit it stopped at; text bytes; those behind its last member end (== len without one)
    uint64_t err_off;        // SKG_S_ERROR: byte offset, SKG_NONE = the start of the member in progress at `start`
    uint64_t last_mstart;    // header offset of the member in progress at `end`, SKG_NONE = the one in progress at `start`
    uint32_t nmem, status, reason, err_nmem; // member ends; SKG_S_*; SK_GZ_*; member ends ahead of the error (+1: the next's header)
    // chain
    uint64_t off, mtext, mstart, mbase; // text offset; text offset and header offset of the member in progress; its index
    uint32_t used, derr;                // decode: a distance reached before its member's first byte
    uint64_t derr_off, derr_nmem;
    uint64_t reserved;
};

struct skg_member { // 32 bytes, one per member end on the chain
    uint64_t text_end, next_start; // text offset behind its last byte; byte offset behind its trailer
    uint32_t crc, isize, acc, reserved; // acc: XOR of its pieces' CRC terms
};

struct skg_args {
    const uint8_t *image;
    uint64_t n;
    uint8_t *out;
    uint64_t capacity;
    uint64_t *hdr;
    skg_stretch *st;
    uint64_t *u_off; // text offsets of the used stretches, then the total
    uint32_t *u_id;
    skg_member *mem;
    uint16_t *sym;
    uint64_t S, chunk_bits, mem_cap; // chunk_bits is a power of two
    uint32_t chunk_shift, pad;       // log2 of it
};

// ------------------------------------------------------------------------------------------
// the gzip header at image[pos], pos < n -> SKI_OK and the offset of the deflate stream
// ------------------------------------------------------------------------------------------
SKD_FN uint32_t skg_parse_header(const uint8_t *image, uint64_t n, uint64_t pos, uint64_t *after)
{
    const uint64_t rem = n - pos;
    const uint8_t *p = image + pos;
    for (uint32_t k = 0; k < 3 && k < rem; ++k)
        if (p[k] != ski_magic(k)) return SKI_HEADER;
    if (rem < 10) return SKI_TRUNCATED;
    const uint32_t flg = p[3];
    if (flg & 0xe0u) return SKI_HEADER;
    uint64_t at = 10;
    if (flg & 4u) { // FEXTRA
        if (at + 2 > rem) return SKI_TRUNCATED;
        at += 2 + ski_le16(p + at);
        if (at > rem) return SKI_TRUNCATED;
    }
    for (uint32_t bit = 8; bit <= 16; bit <<= 1) // FNAME, FCOMMENT: zero-terminated
        if (flg & bit) {
            while (at < rem && p[at]) ++at;
            if (at >= rem) return SKI_TRUNCATED;
            ++at;
        }
    if (flg & 2u) at += 2; // FHCRC, not checked
    if (at > rem) return SKI_TRUNCATED;
    *after = pos + at;
    return SKI_OK;
}

// ------------------------------------------------------------------------------------------
// the bit reader on an image of up to 2^33 bytes
// ------------------------------------------------------------------------------------------
struct skg_reader {
    ski_state s; // s.body moves along the image
};

SKD_FN void skg_window_of(skg_reader *r, const uint8_t *image, uint64_t n, uint64_t byte)
{
    r->s.body = image + byte;
    const uint64_t rem = n - byte;
    r->s.end = rem < (1u << 30) ? (uint32_t)rem : (1u << 30);
}

SKD_FN void skg_seek(skg_reader *r, const uint8_t *image, uint64_t n, uint64_t bit)
{
    ski_begin(&r->s, image, 0, 0xffffffffu);
    skg_window_of(r, image, n, bit >> 3); // bit <= 8 n
    if (bit & 7u) {
        uint32_t v;
        ski_refill(&r->s);
        if (r->s.nbits >= 8) ski_take(&r->s, (uint32_t)(bit & 7u), &v);
    }
}

SKD_FN uint64_t skg_bitpos(const skg_reader *r, const uint8_t *image) { return ((uint64_t)(r->s.body - image) + r->s.in) * 8 - r->s.nbits; }

// keeps s.in small; 8 bytes stay below it: the buffer's bytes, which a stored block's start is counted back over
SKD_FN void skg_rebase(skg_reader *r, const uint8_t *image, uint64_t n)
{
    if (r->s.in < SKG_REBASE_AT) return;
    const uint32_t in = r->s.in;
    skg_window_of(r, image, n, (uint64_t)(r->s.body - image) + in - 8);
    r->s.in = 8;
}

// ------------------------------------------------------------------------------------------
// a block's header and tables (the code of ski_inflate_member) -> false: the state has failed
// ------------------------------------------------------------------------------------------
SKD_FN bool skg_block_begin(ski_shared *sh, ski_state *s, int lane)
{
    (void)lane;
    SKI_SYNC();
    ski_block_header(sh, s);
    SKI_SYNC();
    if (s->mode == SKI_M_DYNAMIC) {
        const ski_build cl = {0, 19, SKI_CL_ROOT, 1, sh->cl, sh->cl_sorted, sh->cl_count};
        SKI_BUILD(sh, cl);
        if (sh->bad) {
            ski_fail(s, SKI_DEFLATE);
            return false;
        }
        SKI_SYNC();
        ski_read_lengths(sh, s);
        SKI_SYNC();
        if (s->mode == SKI_M_ERROR) return false;
        const ski_build lit = ski_build_lit(&sh->dyn, s->nlen);
        SKI_BUILD(sh, lit);
        uint32_t bad = sh->bad;
        SKI_SYNC();
        const ski_build dist = ski_build_dist(&sh->dyn, s->nlen, s->ndist);
        SKI_BUILD(sh, dist);
        bad |= sh->bad;
        if (bad) {
            ski_fail(s, SKI_DEFLATE);
            return false;
        }
    }
    return s->mode != SKI_M_ERROR;
}

// ------------------------------------------------------------------------------------------
// symbols of the current block: ski_decode_batch on a 64-bit text position, the window unknown.  EMIT: tokens are queued
// (positions relative to *pos at entry); a distance that reaches before `floor` (the member's first byte, relative to the
// stretch) queues a zero fill (arg 0) and is reported in *far.
// ------------------------------------------------------------------------------------------
template <bool EMIT>
SKD_FN uint32_t skg_decode_batch(ski_shared *sh, ski_state *s, const ski_tables *t, uint64_t *pos, int64_t floor, bool *far)
{
    uint32_t n = 0, rel = 0;
    while (n < SKI_BATCH) {
        ski_refill(s);
        int sym = ski_symbol(s, t->lit, SKI_LIT_ROOT, t->lit_sorted, t->lit_count);
        if (sym < 0) {
            ski_fail(s, SKI_DEFLATE);
            break;
        }
        if (sym < 256) {
            if (EMIT) {
                sh->tok_pos[n] = rel;
                sh->tok_len[n] = 0;
                sh->tok_arg[n] = (uint32_t)sym;
            }
            ++n;
            ++rel;
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
        if (EMIT) {
            if ((int64_t)dist > (int64_t)(*pos + rel) - floor) {
                *far = true;
                dist = 0;
            }
            sh->tok_pos[n] = rel;
            sh->tok_len[n] = len;
            sh->tok_arg[n] = dist;
        }
        ++n;
        rel += len;
    }
    *pos += rel;
    return n;
}

// ski_resolve_lane on 16-bit symbols: sym is the stretch's first symbol, at the batch's first, lim the stretch's length;
// what lies before the stretch reads as its placeholder
SKD_FN bool skg_resolve_lane(const ski_shared *sh, uint16_t *sym, uint64_t at, uint64_t lim, uint32_t n, uint64_t todo, int lane)
{
    if ((uint32_t)lane >= n || !((todo >> lane) & 1u)) return false;
    const uint32_t first = (uint32_t)__builtin_ctzll(todo); // the caller stops when none is left
    const uint32_t finished = sh->tok_pos[first];
    const uint32_t pos = sh->tok_pos[lane], len = sh->tok_len[lane], arg = sh->tok_arg[lane];
    const uint64_t to = at + pos;
    if (len == 0) {
        if (to < lim) sym[to] = (uint16_t)arg;
        return true;
    }
    if (arg == 0) {
        for (uint32_t k = 0; k < len; ++k)
            if (to + k < lim) sym[to + k] = 0;
        return true;
    }
    if ((int64_t)pos - (int64_t)arg + (int64_t)(len < arg ? len : arg) > (int64_t)finished) return false;
    for (uint32_t k = 0; k < len; ++k) {
        const int64_t from = (int64_t)to - (int64_t)arg + k;
        const uint16_t v = from >= 0 ? sym[from] : from >= -SKG_WINDOW ? (uint16_t)(SKG_UNKNOWN + SKG_WINDOW + from) : (uint16_t)0;
        if (to + k < lim) sym[to + k] = v;
    }
    return true;
}

// ------------------------------------------------------------------------------------------
// one stretch, from its start to where it ends: block after block, member after member.  A boundary that is the guessed
// start of a later chunk ends it.  EMIT: symbols to sym[0, w->len of the count), member ends to mem[].
// ------------------------------------------------------------------------------------------
struct skg_walk { // shared (LDS on the device): every lane writes the same values, so the walk's rarely used state costs no registers
    // in (decode)
    skg_member *mem;   // entries of the member ends in this stretch
    uint64_t text_off; // text offset of the stretch
    // state
    uint64_t self, block_bit, tail_from;
    // out
    uint64_t end, len, tail, err_off, last_mstart;
    uint32_t nmem, status, reason, err_nmem;
    uint32_t derr, pad;
    uint64_t derr_off, derr_nmem;
};

// a piece's walk (skg_walk_stretch<EMIT, true>) keeps more, shared in the same way: the last resume point it reached -- a
// block boundary (in = 1) or a member start behind a complete trailer (in = 0) -- and the bit the decode stops at
struct skg_piece_walk {
    uint64_t stop;       // in (decode): a resume point of the count, or SKG_NONE
    uint64_t r_bit, r_len; // out: the resume point, the stretch's text in front of it
    uint32_t r_in, pad;
};

#ifdef __HIPCC__
// a value every lane holds alike, read back from shared memory: told to the compiler
SKD_FN uint64_t skg_uniform(uint64_t v)
{
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}
#else
SKD_FN uint64_t skg_uniform(uint64_t v) { return v; }
#endif

// the member's end behind a final block: the trailer, then the next member's header or the image's end.  -> true: the
// walk goes on at the next member's first block; false: it ends here (w->status, w->reason say how)
template <bool EMIT, bool PIECE>
SKD_FN bool skg_member_end(const skg_args &a, skg_reader *r, skg_walk *w, skg_piece_walk *pw, uint64_t pos, int lane)
{
    (void)lane;
    (void)pw;
    const uint64_t at = (skg_bitpos(r, a.image) + 7) >> 3;
    w->end = at * 8;
    if (a.n - at < 8) {
        w->reason = SKI_TRUNCATED;
        w->err_off = w->last_mstart;
        w->err_nmem = w->nmem;
        return false;
    }
    if (EMIT) {
        skg_member m;
        m.text_end = w->text_off + pos;
        m.next_start = at + 8;
        m.crc = ski_le32(a.image + at);
        m.isize = ski_le32(a.image + at + 4);
        m.acc = m.reserved = 0;
        SKI_ALL(if (lane == 0) w->mem[w->nmem] = m);
    }
    w->nmem = w->nmem + 1;
    w->tail_from = pos;
    w->end = (at + 8) * 8;
    if (PIECE) {
        pw->r_bit = (at + 8) * 8;
        pw->r_len = pos;
        pw->r_in = 0;
        if (EMIT && pw->stop == (at + 8) * 8) {
            w->status = SKG_S_END;
            return false;
        }
    }
    if (at + 8 == a.n) {
        w->status = SKG_S_END;
        return false;
    }
    uint64_t after = 0;
    const uint64_t next = skg_uniform(at + 8); // opaque: image + 8 is not to become a loop invariant of the whole walk
    const uint32_t why = skg_parse_header(a.image, a.n, next, &after);
    if (why != SKI_OK) {
        w->reason = why;
        w->err_off = next;
        w->err_nmem = w->nmem;
        return false;
    }
    w->last_mstart = next;
    skg_seek(r, a.image, a.n, skg_uniform(after * 8));
    return true;
}

template <bool EMIT, bool PIECE = false>
SKD_FN void skg_walk_stretch(ski_shared *sh, const skg_args &a, uint64_t self, uint16_t *sym, uint64_t lim, int64_t floor,
                             skg_walk *w, int lane, skg_piece_walk *pw = nullptr)
{
    (void)lane;
    (void)pw;
    SKG_PER_LANE(sym);
    SKG_PER_LANE(lim);
    SKG_PER_LANE(floor);
    skg_reader r;
    skg_seek(&r, a.image, a.n, a.st[self].start);
    uint64_t pos = 0;
    w->self = self;
    w->tail_from = 0;
    w->nmem = 0;
    w->status = SKG_S_ERROR;
    w->reason = SKI_DEFLATE;
    w->err_off = w->last_mstart = SKG_NONE;
    w->err_nmem = 0;
    w->derr = 0;
    w->derr_off = w->derr_nmem = 0;
    for (;;) {
        {
            const uint64_t b = skg_bitpos(&r, a.image);
            const uint64_t c = b >> a.chunk_shift;
            w->block_bit = b;
            if (PIECE) {
                pw->r_bit = b;
                pw->r_len = pos;
                pw->r_in = 1;
                if (EMIT && pw->stop == b) {
                    w->status = SKG_S_JOIN;
                    w->end = b;
                    break;
                }
            }
            if (c > skg_uniform(w->self) && c < a.S && a.st[c].start == b) {
                w->status = SKG_S_JOIN;
                w->end = b;
                break;
            }
        }
        skg_rebase(&r, a.image, a.n);
        r.s.mode = SKI_M_HEADER;
        bool ok = skg_block_begin(sh, &r.s, lane);
        if (ok && r.s.mode == SKI_M_STORED) {
            if (EMIT) {
                SKI_ALL(for (uint32_t i = (uint32_t)lane; i < r.s.stored_len; i += SKI_LANES) if (pos + i < lim)
                            sym[pos + i] = r.s.body[r.s.stored_src + i]);
                SKI_FENCE();
            }
            pos += r.s.stored_len;
            r.s.in = r.s.stored_src + r.s.stored_len;
            r.s.buf = 0;
            r.s.nbits = 0;
            r.s.mode = r.s.final ? SKI_M_DONE : SKI_M_HEADER;
        }
        while (ok && r.s.mode == SKI_M_HUFF) {
            skg_rebase(&r, a.image, a.n);
            SKI_SYNC();
            uint64_t at = pos;
            SKG_PER_LANE(at);
            bool far = false;
            const uint32_t n = skg_decode_batch<EMIT>(sh, &r.s, r.s.fixed ? &sh->fixed : &sh->dyn, &pos, floor, &far);
            if (EMIT) {
                if (far && !w->derr) {
                    w->derr = 1;
                    w->derr_off = w->block_bit >> 3;
                    w->derr_nmem = w->nmem;
                }
                SKI_SYNC();
                uint64_t todo = n == 64 ? ~0ull : (1ull << n) - 1;
                while (todo) { // the first token left goes in every round
                    uint64_t got;
                    SKI_BALLOT(got, skg_resolve_lane(sh, sym, at, lim, n, todo, lane));
                    todo &= ~got;
                    SKI_FENCE();
                }
            }
            ok = r.s.mode != SKI_M_ERROR;
        }
        if (!ok) { // a block that does not decode: the byte of its first bit
            w->end = w->block_bit;
            w->err_off = w->block_bit >> 3;
            w->err_nmem = w->nmem;
            break;
        }
        if (r.s.mode != SKI_M_DONE) continue;
        if (!skg_member_end<EMIT, PIECE>(a, &r, w, pw, pos, lane)) break;
        floor = (int64_t)pos;
        SKG_PER_LANE(floor);
    }
    w->len = pos;
    w->tail = pos - w->tail_from;
}

// ------------------------------------------------------------------------------------------
// stage 1, search: chunk c >= 1.  Lane L tests bit base + L for the fixed part of a non-final dynamic block header and a
// complete code-length code; the wave then tries the hits in order: the codes build, the block decodes, a header follows.
// ------------------------------------------------------------------------------------------
SKD_FN bool skg_plausible(const uint8_t *image, uint64_t n, uint64_t p)
{
    if (p + 128 > n * 8) return false;
    const uint8_t *q = image + (p >> 3);
    const uint32_t bit = (uint32_t)(p & 7u);
    uint64_t v, w;
    memcpy(&v, q, 8);
    memcpy(&w, q + 4, 8);
    v >>= bit;
    w >>= bit;
    if ((v & 7u) != 4u) return false; // BFINAL 0, BTYPE 2
    if (((v >> 3) & 31u) > 29u || ((v >> 8) & 31u) > 29u) return false;
    const uint32_t hclen = (uint32_t)((v >> 13) & 15u) + 4;
    uint32_t kraft = 0, codes = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        const uint32_t at = 17 + 3 * i;
        const uint32_t len = (uint32_t)((at + 3 <= 56 ? v >> at : w >> (at - 32)) & 7u);
        if (len) {
            kraft += 128u >> len;
            ++codes;
        }
    }
    return kraft == 128 || (codes == 1 && kraft == 64);
}

SKD_FN bool skg_try_start(ski_shared *sh, const skg_args &a, uint64_t p, int lane)
{
    skg_reader r;
    skg_seek(&r, a.image, a.n, p);
    if (!skg_block_begin(sh, &r.s, lane) || r.s.fixed || r.s.final || r.s.mode != SKI_M_HUFF) return false;
    uint64_t pos = 0;
    bool far;
    while (r.s.mode == SKI_M_HUFF && pos < SKG_TRY_CAP) {
        skg_rebase(&r, a.image, a.n);
        skg_decode_batch<false>(sh, &r.s, &sh->dyn, &pos, 0, &far);
    }
    if (r.s.mode != SKI_M_HEADER) return false;
    SKI_SYNC();
    ski_block_header(sh, &r.s); // what follows must parse too
    SKI_SYNC();
    return r.s.mode != SKI_M_ERROR;
}

SKD_FN void skg_search_chunk(ski_shared *sh, const skg_args &a, uint64_t c, int lane)
{
    (void)lane;
    const uint64_t lo = c * a.chunk_bits, hi = lo + a.chunk_bits < a.n * 8 ? lo + a.chunk_bits : a.n * 8;
    for (uint64_t base = lo; base < hi; base += SKI_LANES) {
        uint64_t hits;
        SKI_BALLOT(hits, base + (uint64_t)lane < hi && skg_plausible(a.image, a.n, base + (uint64_t)lane));
        while (hits) {
            const uint64_t p = base + (uint64_t)__builtin_ctzll(hits);
            hits &= hits - 1;
            SKI_ALL(if (lane == 0) a.st[c].start = p); // stays if p passes
            if (skg_try_start(sh, a, p, lane)) return;
        }
    }
    SKI_ALL(if (lane == 0) a.st[c].start = SKG_NONE);
}

// chunk 0 and the header: stretch 0 starts behind member 0's header
SKD_FN void skg_search_first(const skg_args &a)
{
    for (uint32_t i = 0; i < SKG_HDR_WORDS; ++i) a.hdr[i] = 0;
    a.hdr[SKG_H_BYTES_IN] = a.n;
    a.hdr[SKG_H_STRETCHES] = a.S;
    a.hdr[SKG_H_FIT] = 1;
    a.hdr[SKG_H_DECODED] = a.out != nullptr;
    a.hdr[SKG_H_ERROR_KEY] = a.hdr[SKG_H_CHAIN_KEY] = SKG_NONE;
    if (a.S == 0) return;
    uint64_t after = 0;
    const uint32_t why = skg_parse_header(a.image, a.n, 0, &after);
    a.st[0].start = why == SKI_OK ? after * 8 : SKG_NONE;
    if (why != SKI_OK) a.hdr[SKG_H_CHAIN_KEY] = why; // member 0
}

// ------------------------------------------------------------------------------------------
// stage 2, count: stretch k (with a start): lengths only
// ------------------------------------------------------------------------------------------
SKD_FN void skg_count_stretch(ski_shared *sh, skg_walk *w, const skg_args &a, uint64_t k, int lane)
{
    skg_walk_stretch<false>(sh, a, k, nullptr, 0, 0, w, lane);
    SKI_ALL(if (lane == 0) {
        skg_stretch *s = &a.st[k];
        s->end = w->end;
        s->len = w->len;
        s->tail = w->tail;
        s->err_off = w->err_off;
        s->last_mstart = w->last_mstart;
        s->nmem = w->nmem;
        s->status = w->status;
        s->reason = w->reason;
        s->err_nmem = w->err_nmem;
        s->used = 0;
        s->derr = 0;
    });
}

// ------------------------------------------------------------------------------------------
// stage 3, chain (one lane): from stretch 0, a stretch is used iff the one before ended exactly on its start
// ------------------------------------------------------------------------------------------
SKD_FN void skg_chain(const skg_args &a)
{
    uint64_t used = 0, off = 0, members = 0, mtext = 0, mstart = 0;
    if (a.S && a.st[0].start != SKG_NONE) {
        uint64_t k = 0;
        for (;;) { // k grows
            skg_stretch *s = &a.st[k];
            s->used = 1;
            s->off = off;
            s->mtext = mtext;
            s->mstart = mstart;
            s->mbase = members;
            a.u_off[used] = off;
            a.u_id[used++] = (uint32_t)k;
            if (s->status == SKG_S_ERROR) {
                a.hdr[SKG_H_CHAIN_KEY] = ((members + s->err_nmem) << 3) | s->reason;
                a.hdr[SKG_H_CHAIN_OFFSET] = s->err_off != SKG_NONE ? s->err_off : mstart;
            }
            if (s->nmem) mtext = off + s->len - s->tail;
            if (s->last_mstart != SKG_NONE) mstart = s->last_mstart;
            off += s->len;
            members += s->nmem < a.mem_cap - members ? s->nmem : a.mem_cap - members; // nmem <= n / 18 on a chain: never cut
            if (s->status != SKG_S_JOIN) break;
            k = s->end >> a.chunk_shift;
        }
    }
    a.u_off[used] = off;
    a.hdr[SKG_H_USED] = used;
    a.hdr[SKG_H_MEMBERS] = members;
    a.hdr[SKG_H_BYTES_OUT] = off;
    a.hdr[SKG_H_FIT] = a.out == nullptr || off <= a.capacity;
    a.hdr[SKG_H_ERROR_KEY] = a.hdr[SKG_H_CHAIN_KEY];
    a.hdr[SKG_H_ERROR_OFFSET] = a.hdr[SKG_H_CHAIN_OFFSET];
}

// ------------------------------------------------------------------------------------------
// stage 4, decode: used stretch number u, into symbols at its text offset
// ------------------------------------------------------------------------------------------
// a distance that reached before its member's first byte, to the stretch's record and the call's key
SKD_FN void skg_decode_publish(skg_walk *w, const skg_args &a, int lane)
{
    (void)lane;
    // the lane is compared here, on an opaque copy: "lane == 0" as a mask would live in a scalar pair through the walk
    SKI_ALL(int who = lane; SKG_PER_LANE(who); if (who == 0 && w->derr) {
        skg_stretch *t = &a.st[w->self];
        t->derr = 1;
        t->derr_off = w->derr_off;
        t->derr_nmem = w->derr_nmem;
        SKG_ATOMIC_MIN64(&a.hdr[SKG_H_ERROR_KEY], ((t->mbase + w->derr_nmem) << 3) | SKI_DEFLATE);
    });
}

SKD_FN void skg_decode_stretch(ski_shared *sh, skg_walk *w, const skg_args &a, uint64_t u, int lane)
{
    const uint64_t k = a.u_id[u];
    const skg_stretch *s = &a.st[k];
    const uint64_t off = s->off, before = off - s->mtext; // text of the member in progress ahead of the stretch
    const int64_t floor = before > (1ull << 40) ? -(int64_t)(1ull << 40) : -(int64_t)before;
    w->mem = a.mem + s->mbase;
    w->text_off = off;
    skg_walk_stretch<true>(sh, a, k, a.sym + off, s->len, floor, w, lane);
    skg_decode_publish(w, a, lane);
}

// ------------------------------------------------------------------------------------------
// stage 5, windows: element i of the last min(len, 32 Ki) symbols of used stretch u >= 1, from the 32 Ki symbols before
// the stretch, which the steps before have made literal
// ------------------------------------------------------------------------------------------
SKD_FN uint16_t skg_fill(const uint16_t *sym, uint64_t off, uint16_t v)
{
    if (v < SKG_UNKNOWN) return v;
    const uint64_t j = v - SKG_UNKNOWN;
    if (j >= SKG_WINDOW || off + j < SKG_WINDOW) return 0; // before the text: reported by the decode
    return sym[off - SKG_WINDOW + j];
}

SKD_FN void skg_window_elem(const skg_args &a, uint64_t u, uint32_t i)
{
    const uint64_t off = a.u_off[u], len = a.u_off[u + 1] - off;
    const uint64_t r = len < SKG_WINDOW ? len : SKG_WINDOW;
    if (i >= r) return;
    uint16_t *p = a.sym + off + len - r + i;
    *p = skg_fill(a.sym, off, *p);
}

// ------------------------------------------------------------------------------------------
// stage 6, resolve: granule g of out, 16 bytes stored once
// ------------------------------------------------------------------------------------------
SKD_FN void skg_resolve_granule(const skg_args &a, uint64_t g)
{
    const uint64_t total = a.hdr[SKG_H_BYTES_OUT], used = a.hdr[SKG_H_USED];
    const uint64_t t0 = g * 16;
    if (t0 >= total) return;
    uint64_t lo = 0, hi = used; // the last used stretch that starts at or before t0
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (a.u_off[mid] <= t0) lo = mid;
        else hi = mid;
    }
    uint64_t u = lo;
    uint8_t b[16];
    const uint32_t cnt = total - t0 < 16 ? (uint32_t)(total - t0) : 16u;
    for (uint32_t i = 0; i < 16; ++i) {
        b[i] = 0;
        if (i >= cnt) continue;
        while (u + 1 < used && a.u_off[u + 1] <= t0 + i) ++u;
        b[i] = (uint8_t)skg_fill(a.sym, a.u_off[u], a.sym[t0 + i]);
    }
    if (cnt == 16) {
        memcpy(a.out + t0, b, 16); // out is 16-byte aligned
    } else {
        for (uint32_t i = 0; i < cnt; ++i) a.out[t0 + i] = b[i];
    }
}

// ------------------------------------------------------------------------------------------
// stage 7, CRC: piece q of out, cut at member ends; each span's term goes to its member by XOR (the CRC is linear)
// ------------------------------------------------------------------------------------------
struct skg_crc_shared {
    uint32_t table[256];
    uint32_t power[SKG_POWERS];
    uint32_t lane_crc[SKI_LANES];
};

SKD_FN void skg_crc_tables(skg_crc_shared *cs, int lane)
{
    for (int i = lane; i < 256; i += SKI_LANES) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (c & 1u ? SKB_POLY : 0u);
        cs->table[i] = c;
    }
    if (lane < SKG_POWERS) {
        uint32_t e = 0x00800000u; // x^8
        for (int j = 0; j < lane; ++j) e = skb_mul(e, e);
        cs->power[lane] = e;
    }
}

SKD_FN uint32_t skg_shift_of(const uint32_t *power, uint64_t k)
{
    uint32_t r = 0x80000000u;
    for (int j = 0; j < SKG_POWERS; ++j)
        if ((k >> j) & 1u) r = skb_mul(r, power[j]);
    return r;
}

// the member whose text holds byte t < total: the first whose text_end is beyond t
SKD_FN uint64_t skg_member_of(const skg_member *mem, uint64_t members, uint64_t t)
{
    uint64_t lo = 0, hi = members;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (mem[mid].text_end <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// a span p[0, n) of a member that goes on for `behind` bytes after it: each lane's share, shifted to the member's end
SKD_FN void skg_crc_span_lane(skg_crc_shared *cs, const uint8_t *p, uint32_t n, uint64_t behind, int lane)
{
    const uint32_t seg = (n + SKI_LANES - 1) / SKI_LANES;
    uint32_t from = (uint32_t)lane * seg;
    const uint32_t to = from + seg < n ? from + seg : n;
    if (from > n) from = n;
    uint32_t c = 0;
    for (uint32_t i = from; i < to; ++i) c = cs->table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    cs->lane_crc[lane] = to > from ? skb_mul(c, skg_shift_of(cs->power, behind + (n - to))) : 0u;
}

SKD_FN void skg_crc_span_close(skg_crc_shared *cs, uint32_t *acc)
{
    uint32_t x = 0;
    for (int l = 0; l < SKI_LANES; ++l) x ^= cs->lane_crc[l];
    SKG_ATOMIC_XOR(acc, x);
}

SKD_FN void skg_crc_piece(skg_crc_shared *cs, const skg_args &a, uint64_t q, int lane)
{
    (void)lane;
    const uint64_t members = a.hdr[SKG_H_MEMBERS];
    const uint64_t last = members ? a.mem[members - 1].text_end : 0; // text behind it belongs to no finished member
    uint64_t lo = q * SKG_PIECE, end = lo + SKG_PIECE < last ? lo + SKG_PIECE : last;
    if (lo >= end) return;
    uint64_t m = skg_member_of(a.mem, members, lo);
    while (lo < end && m < members) {
        const uint64_t mend = a.mem[m].text_end, hi = mend < end ? mend : end;
        if (hi > lo) {
            SKI_ALL(skg_crc_span_lane(cs, a.out + lo, (uint32_t)(hi - lo), mend - hi, lane));
            SKI_ALL(if (lane == 0) skg_crc_span_close(cs, &a.mem[m].acc));
        }
        lo = hi;
        ++m;
    }
}

// ------------------------------------------------------------------------------------------
// stage 8, check: member m's length against ISIZE, then its CRC-32
// ------------------------------------------------------------------------------------------
SKD_FN void skg_check_member(const uint32_t *power, const skg_args &a, uint64_t m)
{
    const skg_member e = a.mem[m];
    const uint64_t len = e.text_end - (m ? a.mem[m - 1].text_end : 0);
    uint32_t why = SKI_OK;
    if ((uint32_t)len != e.isize) why = SKI_LENGTH;
    else if (~(skb_mul(0xffffffffu, skg_shift_of(power, len)) ^ e.acc) != e.crc) why = SKI_CRC;
    if (why != SKI_OK) SKG_ATOMIC_MIN64(&a.hdr[SKG_H_ERROR_KEY], (m << 3) | why);
}

// ------------------------------------------------------------------------------------------
// stage 9, final (one lane): the written word, and the offset that goes with the lowest failure
// ------------------------------------------------------------------------------------------
SKD_FN void skg_final(const skg_args &a)
{
    const uint64_t key = a.hdr[SKG_H_ERROR_KEY];
    // nothing behind this stage lowers the key, and the stage runs in decoding calls whose text fitted only: in every
    // other call the word keeps the 0 skg_search_first gave it
    a.hdr[SKG_H_WRITTEN] = a.out != nullptr && key == SKG_NONE;
    if (key == SKG_NONE) return;
    const uint32_t why = (uint32_t)(key & 7u);
    const uint64_t m = key >> 3;
    uint64_t off = SKG_NONE;
    if (key == a.hdr[SKG_H_CHAIN_KEY]) off = a.hdr[SKG_H_CHAIN_OFFSET];
    if (why == SKI_DEFLATE) {
        const uint64_t used = a.hdr[SKG_H_USED];
        for (uint64_t u = 0; u < used; ++u) { // in stream order: the first is the lowest
            const skg_stretch *s = &a.st[a.u_id[u]];
            if (s->derr && (((s->mbase + s->derr_nmem) << 3) | SKI_DEFLATE) == key) {
                if (s->derr_off < off) off = s->derr_off;
                break;
            }
        }
    } else if (why == SKI_LENGTH || why == SKI_CRC) {
        off = m ? a.mem[m - 1].next_start : 0;
    }
    a.hdr[SKG_H_ERROR_OFFSET] = off;
}

// ==========================================================================================
// Pieces (sk_gzip_inflate_piece_device_async, sk_gunzip_piece.hip): the call starts at a device-resident state and
// publishes the next one.  The stages above run on the WINDOW: an skg_args whose image begins at the byte that holds the
// state's position, so every bit and byte offset below is relative to it.  The symbols get a prefix of SKG_WINDOW
// literals, the state's history, and every text offset is shifted by as much: stretch 0's placeholders then resolve as
// every other stretch's do.  `out` is shifted the other way, and one more member entry, the open member's, ends the
// table, so that its text has a CRC term too.
// ==========================================================================================
struct skg_piece_words {
    uint64_t pos_bit, in_member, member_text, member_crc, members, text_bytes, status, error, error_member, error_offset, done;
    uint64_t mstart; // reserved[0]: the header offset of the member in progress (of the member that begins, in_member 0)
    uint64_t reserved[4];
};
struct skg_piece_state { // sk_gzip_piece_state of sickle_amd.h
    skg_piece_words w;
    uint8_t history[SKG_WINDOW];
};

struct skg_resume { // 32 bytes per stretch
    uint64_t bit, len; // count: the last resume point of the stretch's walk, its text in front of it
    uint64_t in;       // 1: a block boundary, 0: a member start
    uint64_t stop;     // chain: the bit the decode stops at, or SKG_NONE
};

struct skg_piece_args {
    const skg_piece_state *in;
    skg_piece_state *out;
    const uint8_t *image;
    uint64_t image_bytes, image_offset, window_bytes;
    uint8_t *text; // the caller's out
    uint64_t capacity;
    skg_resume *res;
    uint32_t last, pad;
};

#define SKG_P_RUN 0u     // what the state asks of the call
#define SKG_P_VOID 1u    // a failed state: nothing is done, the failure is handed on
#define SKG_P_DONE 2u    // the stream has ended: an empty piece
#define SKG_P_OUTSIDE 3u // the position is not in the image handed in
// header words of a piece, behind those of the whole call
#define SKG_H_P_KIND 12
#define SKG_H_P_BASE 13    // stream offset of the window's first byte
#define SKG_H_P_END_BIT 14 // chain: the resume point the piece ends at (window-relative), what it is, the header of its member
#define SKG_H_P_END_IN 15
#define SKG_H_P_END_MSTART 16
#define SKG_H_P_LIMITED 17 // the failure is the first thing in the window of a piece that is not closing
#define SKG_H_P_DONE 18
#define SKG_H_P_STATUS 19  // state: what finish reports: the state's status, failure, position
#define SKG_H_P_ERROR 20
#define SKG_H_P_ERROR_MEMBER 21
#define SKG_H_P_ERROR_OFFSET 22
#define SKG_H_P_INHERITED 23
#define SKG_H_P_POS_BIT 24
#define SKG_H_P_IN_MEMBER 25
#define SKG_H_P_CLOSING 26
#define SKG_H_P_IMAGE_OFFSET 27

// the window, from the state: a->image and a->n.  Once per workgroup; the state is never written
SKD_FN uint32_t skg_piece_window(const skg_piece_args &p, skg_args *a, bool *closing)
{
    *closing = false;
    if (p.in->w.status) return SKG_P_VOID;
    if (p.in->w.done) return SKG_P_DONE;
    const uint64_t pos = p.in->w.pos_bit >> 3, image_end = p.image_offset + p.image_bytes;
    if (pos < p.image_offset || pos > image_end) return SKG_P_OUTSIDE;
    const uint64_t end = image_end - pos < p.window_bytes ? image_end : pos + p.window_bytes;
    a->image = p.image + (pos - p.image_offset);
    a->n = end - pos;
    *closing = p.last && end == image_end;
    return SKG_P_RUN;
}

// stage 1, chunk 0 (one lane): the header words, and stretch 0's start: behind the header of the member that begins at
// the position, or the position itself
SKD_FN void skg_piece_first(const skg_args &a, const skg_piece_args &p, uint32_t kind, bool closing)
{
    for (uint32_t i = 0; i < SKG_HDR_WORDS; ++i) a.hdr[i] = 0;
    a.hdr[SKG_H_STRETCHES] = a.S;
    a.hdr[SKG_H_FIT] = 1;
    a.hdr[SKG_H_DECODED] = 1;
    a.hdr[SKG_H_ERROR_KEY] = a.hdr[SKG_H_CHAIN_KEY] = SKG_NONE;
    a.hdr[SKG_H_P_KIND] = kind;
    a.hdr[SKG_H_P_IMAGE_OFFSET] = p.image_offset;
    if (kind != SKG_P_RUN) return;
    a.hdr[SKG_H_BYTES_IN] = a.n;
    a.hdr[SKG_H_P_BASE] = p.in->w.pos_bit >> 3;
    a.hdr[SKG_H_P_CLOSING] = closing;
    if (p.in->w.in_member) {
        a.st[0].start = p.in->w.pos_bit & 7u;
        return;
    }
    a.st[0].start = SKG_NONE;
    if (a.n == 0 && closing) return; // the stream ends where a member may begin
    uint64_t after = 0;
    const uint32_t why = skg_parse_header(a.image, a.n, 0, &after);
    if (why == SKI_OK) a.st[0].start = after * 8;
    else a.hdr[SKG_H_CHAIN_KEY] = why; // member 0 of the piece
}

// stage 2
SKD_FN void skg_count_stretch_piece(ski_shared *sh, skg_walk *w, skg_piece_walk *pw, const skg_args &a, const skg_piece_args &p,
                                    uint64_t k, int lane)
{
    (void)lane;
    pw->stop = SKG_NONE;
    skg_walk_stretch<false, true>(sh, a, k, nullptr, 0, 0, w, lane, pw);
    SKI_ALL(if (lane == 0) {
        skg_stretch *s = &a.st[k];
        s->end = w->end;
        s->len = w->len;
        s->tail = w->tail;
        s->err_off = w->err_off;
        s->last_mstart = w->last_mstart;
        s->nmem = w->nmem;
        s->status = w->status;
        s->reason = w->reason;
        s->err_nmem = w->err_nmem;
        s->used = 0;
        s->derr = 0;
        skg_resume *r = &p.res[k];
        r->bit = pw->r_bit;
        r->len = pw->r_len;
        r->in = pw->r_in;
        r->stop = SKG_NONE;
    });
}

// stage 3 (one lane): skg_chain from the state.  A piece that is not closing takes a stretch that failed up to its last
// resume point and ends there; every piece ends in front of the first stretch whose text would pass the capacity.
SKD_FN void skg_chain_piece(const skg_args &a, const skg_piece_args &p, bool closing)
{
    const skg_piece_state *in = p.in;
    const uint64_t base = in->w.pos_bit >> 3;
    uint64_t used = 0, off = SKG_WINDOW, members = 0;
    uint64_t mtext = SKG_WINDOW - in->w.member_text, mstart = in->w.in_member ? in->w.mstart - base : 0; // both may wrap: they are only subtracted
    uint64_t end_bit = in->w.pos_bit & 7u, end_in = in->w.in_member, need = 0;
    bool fit = true, limited = false, ended = a.n == 0 && closing && !in->w.in_member;
    if (a.st[0].start == SKG_NONE) {
        limited = !closing && a.hdr[SKG_H_CHAIN_KEY] != SKG_NONE;
        a.hdr[SKG_H_CHAIN_OFFSET] = 0;
    } else {
        uint64_t k = 0;
        for (;;) { // k grows
            skg_stretch *s = &a.st[k];
            skg_resume *r = &p.res[k];
            const bool failed = s->status == SKG_S_ERROR, first = used == 0;
            bool cut = false;
            uint64_t len = s->len;
            if (failed && !closing) {
                const bool progress = r->bit != s->start || (first && !in->w.in_member); // behind a header is a resume point
                if (!progress && !first) break;
                if (progress) {
                    cut = true;
                    len = r->len;
                } else { // the failure is the first thing in the window: reported, and none of its text
                    limited = true;
                    len = 0;
                }
            }
            if (off - SKG_WINDOW + len > p.capacity) {
                if (first) {
                    fit = false;
                    need = len;
                }
                break;
            }
            s->used = 1;
            s->off = off;
            s->mtext = mtext;
            s->mstart = mstart;
            s->mbase = members;
            a.u_off[used] = off;
            a.u_id[used++] = (uint32_t)k;
            r->stop = cut ? r->bit : SKG_NONE;
            if (failed && !cut) {
                a.hdr[SKG_H_CHAIN_KEY] = ((members + s->err_nmem) << 3) | s->reason;
                a.hdr[SKG_H_CHAIN_OFFSET] = s->err_off != SKG_NONE ? s->err_off : mstart;
            }
            if (s->nmem) mtext = off + s->len - s->tail;
            if (s->last_mstart != SKG_NONE) mstart = s->last_mstart;
            s->len = len;
            off += len;
            members += s->nmem < a.mem_cap - 1 - members ? s->nmem : a.mem_cap - 1 - members; // never cut: skg_chain
            end_bit = cut ? r->bit : s->end;
            end_in = cut ? r->in : s->status != SKG_S_END;
            if (!end_in) mstart = end_bit >> 3;
            ended = closing && !cut && s->status == SKG_S_END;
            if (cut || s->status != SKG_S_JOIN) break;
            k = s->end >> a.chunk_shift;
        }
    }
    skg_member open; // the member in progress at the end: its text is what lies behind the last member end
    open.text_end = off;
    open.next_start = 0;
    open.crc = open.isize = open.acc = open.reserved = 0;
    a.mem[members] = open;
    a.u_off[used] = off;
    a.hdr[SKG_H_USED] = used;
    a.hdr[SKG_H_MEMBERS] = members + 1; // with the open member's entry, until skg_piece_publish
    a.hdr[SKG_H_BYTES_OUT] = fit ? off : SKG_WINDOW + need;
    a.hdr[SKG_H_FIT] = fit;
    a.hdr[SKG_H_ERROR_KEY] = a.hdr[SKG_H_CHAIN_KEY];
    a.hdr[SKG_H_ERROR_OFFSET] = a.hdr[SKG_H_CHAIN_OFFSET];
    a.hdr[SKG_H_P_END_BIT] = end_bit;
    a.hdr[SKG_H_P_END_IN] = end_in;
    a.hdr[SKG_H_P_END_MSTART] = mstart;
    a.hdr[SKG_H_P_LIMITED] = limited;
    a.hdr[SKG_H_P_DONE] = ended;
}

// stage 4: skg_decode_stretch with the chain's stop bit
SKD_FN void skg_decode_stretch_piece(ski_shared *sh, skg_walk *w, skg_piece_walk *pw, const skg_args &a, const skg_piece_args &p,
                                     uint64_t u, int lane)
{
    const uint64_t k = a.u_id[u];
    const skg_stretch *s = &a.st[k];
    const uint64_t off = s->off, before = off - s->mtext;
    const int64_t floor = before > (1ull << 40) ? -(int64_t)(1ull << 40) : -(int64_t)before;
    w->mem = a.mem + s->mbase;
    w->text_off = off;
    pw->stop = p.res[k].stop;
    skg_walk_stretch<true, true>(sh, a, k, a.sym + off, s->len, floor, w, lane, pw);
    skg_decode_publish(w, a, lane);
}

// stage 8, member 0 of a piece: the state's length and CRC-32 go in front of the piece's
SKD_FN void skg_check_first_piece(const uint32_t *power, const skg_args &a, const skg_piece_args &p)
{
    const skg_member e = a.mem[0];
    const uint64_t len = e.text_end - SKG_WINDOW;
    uint32_t why = SKI_OK;
    if ((uint32_t)(p.in->w.member_text + len) != e.isize) why = SKI_LENGTH;
    else if (~(skb_mul(~(uint32_t)p.in->w.member_crc, skg_shift_of(power, len)) ^ e.acc) != e.crc) why = SKI_CRC;
    if (why != SKI_OK) SKG_ATOMIC_MIN64(&a.hdr[SKG_H_ERROR_KEY], (uint64_t)why);
}

// the last stage, behind skg_final.  Byte i of the next history: the last SKG_WINDOW bytes of history ++ text
SKD_FN void skg_piece_history(const skg_args &a, const skg_piece_args &p, uint32_t i)
{
    const bool wrote = a.hdr[SKG_H_P_KIND] == SKG_P_RUN && a.hdr[SKG_H_FIT] && a.hdr[SKG_H_ERROR_KEY] == SKG_NONE;
    const uint64_t text = wrote ? a.hdr[SKG_H_BYTES_OUT] - SKG_WINDOW : 0, at = text + i;
    p.out->history[i] = at < SKG_WINDOW ? p.in->history[at] : p.text[at - SKG_WINDOW];
}

// (one lane) the next state, and the header words as the call's callers read them: counts of the piece, stream-wide
// member numbers and offsets
SKD_FN void skg_piece_publish(const skg_args &a, const skg_piece_args &p, const uint32_t *power)
{
    const skg_piece_words in = p.in->w;
    skg_piece_words n = in;
    uint64_t *h = a.hdr;
    const uint64_t kind = h[SKG_H_P_KIND];
    if (kind == SKG_P_VOID) {
        h[SKG_H_P_INHERITED] = 1;
    } else if (kind == SKG_P_DONE) {
        h[SKG_H_WRITTEN] = 1;
    } else if (kind == SKG_P_OUTSIDE) {
        n.status = 3;
    } else {
        const uint64_t members = h[SKG_H_MEMBERS] - 1, base = h[SKG_H_P_BASE], key = h[SKG_H_ERROR_KEY];
        h[SKG_H_MEMBERS] = members;
        h[SKG_H_BYTES_OUT] -= SKG_WINDOW;
        n.members = in.members + members;
        if (key != SKG_NONE) {
            const uint32_t why = (uint32_t)(key & 7u);
            const uint64_t m = key >> 3;
            n.status = 1;
            n.error = why;
            n.error_member = in.members + m;
            // member 0's first byte lies before the window when the piece began inside it
            n.error_offset = m == 0 && (why == SKI_LENGTH || why == SKI_CRC) && in.in_member ? in.mstart : base + h[SKG_H_ERROR_OFFSET];
            n.text_bytes = in.text_bytes + h[SKG_H_BYTES_OUT];
        } else if (!h[SKG_H_FIT]) {
            n.status = 2;
            n.members = in.members;
        } else {
            const skg_member open = a.mem[members];
            const uint64_t tail = open.text_end - (members ? a.mem[members - 1].text_end : (uint64_t)SKG_WINDOW);
            n.pos_bit = base * 8 + h[SKG_H_P_END_BIT];
            n.in_member = h[SKG_H_P_END_IN];
            n.member_text = n.member_crc = 0;
            if (n.in_member) {
                const uint32_t before = members ? 0u : (uint32_t)in.member_crc;
                n.member_text = (members ? 0 : in.member_text) + tail;
                n.member_crc = (uint32_t)~(skb_mul(~before, skg_shift_of(power, tail)) ^ open.acc);
            }
            n.mstart = base + h[SKG_H_P_END_MSTART];
            n.text_bytes = in.text_bytes + h[SKG_H_BYTES_OUT];
            n.done = h[SKG_H_P_DONE];
        }
    }
    p.out->w = n;
    h[SKG_H_P_STATUS] = n.status;
    h[SKG_H_P_ERROR] = n.error;
    h[SKG_H_P_ERROR_MEMBER] = n.error_member;
    h[SKG_H_P_ERROR_OFFSET] = n.error_offset;
    h[SKG_H_P_POS_BIT] = n.pos_bit;
    h[SKG_H_P_IN_MEMBER] = n.in_member;
    h[SKG_H_P_DONE] = n.done;
    if (n.status) h[SKG_H_WRITTEN] = 0;
}

#endif
