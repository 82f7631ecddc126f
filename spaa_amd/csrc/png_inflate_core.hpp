// png_inflate_core.hpp — one inflate (RFC 1951) for the device and the host: the bit reader, the Huffman table construction with its
// checks, the symbol loop and every bound.  png_decode.hip instantiates it with one wave per image (a 32 KiB history ring in LDS);
// tests/host/png_inflate_host.cpp instantiates it with one "lane" and a flat output array, under ASan + UBSan.
//
// Control flow is UNIFORM: every lane holds the same bit buffer, decodes the same symbol and takes the same branch.  Lanes differ only
// inside the loops marked "lanes": clearing and filling tables, copying a match, copying a stored block.  A value that all lanes store
// to one address (a literal, a code length) is the same value, and each lane later reads back what it stored itself; data that
// ONE lane stores for the others is followed by P::sync().
//
// The policy P supplies:
//   int  lane(), lanes()                       this lane and the number of lanes (host: 0 and 1)
//   void sync()                                orders the lanes' table / history accesses (host: nothing)
//   uint8_t in(uint32_t pos)                   input byte pos, pos < in_len
//   uint8_t& hist(uint32_t p)                  the byte of output position p; positions older than 32768 need not be kept
//   void stored(uint32_t out, uint32_t pos, uint32_t n)   output[out .. out + n) = input[pos .. pos + n), n <= STORED_PIECE
//   void produced(uint32_t out)                called after every symbol with the output length so far (device: flushes the ring)
// Bounds: input is read only at pos < in_len, output is written only at p < expect, a match reads only p < out.  Every turn of
// every loop consumes at least one input bit or ends the block, so the work is bounded by 8 in_len + expect.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PNGI_FN __device__ __forceinline__
#else
#define PNGI_FN inline
#endif

#ifndef SPAA_PNG_OK   // (include/spaa_hip.h names the same values for callers)
#define SPAA_PNG_OK 0
#define SPAA_PNG_BAD_BLOCK_TYPE 1
#define SPAA_PNG_STORED_LEN 2
#define SPAA_PNG_OVERSUBSCRIBED 3
#define SPAA_PNG_INCOMPLETE 4
#define SPAA_PNG_BAD_REPEAT 5
#define SPAA_PNG_BAD_SYMBOL 6
#define SPAA_PNG_DIST_TOO_FAR 7
#define SPAA_PNG_OUTPUT_LONG 8
#define SPAA_PNG_INPUT_END 9
#define SPAA_PNG_OUTPUT_SHORT 10
#define SPAA_PNG_BAD_FILTER 11
#define SPAA_PNG_BAD_DESC 12
#endif

namespace pngi {

constexpr int LIT_FAST = 10, DIST_FAST = 8;      // bits of the one-load tables; longer codes walk the canonical counts
constexpr uint32_t STORED_PIECE = 4096;
constexpr int INVALID = -1;

template <int NSYM, int FB>
struct Huff {
    uint16_t count[16];          // codes per length
    uint16_t symbol[NSYM];       // symbols in canonical order
    uint16_t fast[1 << FB];      // next FB bits -> length << 9 | symbol; 0: a longer or an unused code
};

struct Tables {
    Huff<288, LIT_FAST> lit;     // also the code-length code while a dynamic header is read
    Huff<32, DIST_FAST> dist;
    uint8_t lens[320];
    uint8_t fixed_built;
};

struct Bits {
    uint64_t hold;
    uint32_t n, pos, in_len;
};

template <class P>
PNGI_FN void refill(P& p, Bits& b) {
    if (b.n <= 32 && b.pos + 4 <= b.in_len) {
        const uint32_t w = (uint32_t)p.in(b.pos) | (uint32_t)p.in(b.pos + 1) << 8 | (uint32_t)p.in(b.pos + 2) << 16 |
                           (uint32_t)p.in(b.pos + 3) << 24;
        b.hold |= (uint64_t)w << b.n;
        b.n += 32;
        b.pos += 4;
    }
    while (b.n <= 56 && b.pos < b.in_len) {
        b.hold |= (uint64_t)p.in(b.pos++) << b.n;
        b.n += 8;
    }
}

PNGI_FN uint32_t take(Bits& b, uint32_t k) {      // k <= 16 bits the caller knows to be there
    const uint32_t v = (uint32_t)b.hold & ((1u << k) - 1u);
    b.hold >>= k;
    b.n -= k;
    return v;
}

PNGI_FN uint32_t rev16(uint32_t v) {
    v = (v >> 1 & 0x5555u) | (v & 0x5555u) << 1;
    v = (v >> 2 & 0x3333u) | (v & 0x3333u) << 2;
    v = (v >> 4 & 0x0f0fu) | (v & 0x0f0fu) << 4;
    return (v >> 8 & 0x00ffu) | (v & 0x00ffu) << 8;
}

// The canonical code of lens[0 .. n): counts, symbols in code order, the fast table.  `single_ok`: a code set of ONE code of length 1 is
// accepted although it is incomplete (zlib accepts it for the literal and the distance code).  An empty set is accepted (a symbol
// decoded with it is SPAA_PNG_BAD_SYMBOL).
template <class P, int NSYM, int FB>
PNGI_FN int build(P& p, Huff<NSYM, FB>& h, const uint8_t* lens, int n, bool single_ok) {
    p.sync();                                                     // (lens and the previous table's readers are done)
    for (int i = p.lane(); i < (1 << FB); i += p.lanes()) h.fast[i] = 0;        // lanes
    for (int l = p.lane(); l < 16; l += p.lanes()) {                          // lanes: one code length each
        int c = 0;
        for (int i = 0; i < n; ++i) c += lens[i] == l;
        h.count[l] = (uint16_t)c;
    }
    p.sync();
    int left = 1, total = 0;
    for (int l = 1; l <= 15; ++l) {
        left = (left << 1) - (int)h.count[l];
        total += h.count[l];
        if (left < 0) return SPAA_PNG_OVERSUBSCRIBED;
    }
    if (left > 0 && total > 0 && !(single_ok && total == 1 && h.count[1] == 1)) return SPAA_PNG_INCOMPLETE;
    for (int l = 1 + p.lane(); l < 16; l += p.lanes()) {                      // lanes: the symbols of one length, in order
        uint32_t code = 0, at = 0;
        for (int k = 1; k < l; ++k) {
            code = (code + h.count[k]) << 1;
            at += h.count[k];
        }
        for (int i = 0; i < n; ++i)
            if (lens[i] == l) {
                h.symbol[at++] = (uint16_t)i;
                if (l <= FB)
                    for (uint32_t k = rev16(code) >> (16 - l); k < (1u << FB); k += 1u << l) h.fast[k] = (uint16_t)(l << 9 | i);
                ++code;
            }
    }
    p.sync();
    return SPAA_PNG_OK;
}

// One symbol from the bits at hand (missing bits read as 0; the caller compares the length with what it has): INVALID for a bit
// pattern that no code of the set begins.
template <int NSYM, int FB>
PNGI_FN int decode(const Huff<NSYM, FB>& h, uint32_t bits, uint32_t& len) {
    const uint32_t e = h.fast[bits & ((1u << FB) - 1u)];
    if (e) {
        len = e >> 9;
        return (int)(e & 511u);
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = h.count[l];
        if (code - c < first) {
            len = (uint32_t)l;
            return h.symbol[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return INVALID;
}

template <class P>
PNGI_FN int fixed_tables(P& p, Tables& t) {
    if (t.fixed_built) return SPAA_PNG_OK;
    p.sync();
    for (int i = p.lane(); i < 320; i += p.lanes())                             // lanes
        t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
    int rc = build(p, t.lit, t.lens, 288, false);
    if (rc == SPAA_PNG_OK) rc = build(p, t.dist, t.lens + 288, 32, false);
    p.sync();
    t.fixed_built = 1;          // (every lane stores the same value and reads its own store)
    return rc;
}

template <class P>
PNGI_FN int dynamic_tables(P& p, Tables& t, Bits& b) {
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    t.fixed_built = 0;
    refill(p, b);
    if (b.n < 14) return SPAA_PNG_INPUT_END;
    const int nlen = (int)take(b, 5) + 257, ndist = (int)take(b, 5) + 1, ncode = (int)take(b, 4) + 4;
    if (nlen > 286 || ndist > 30) return SPAA_PNG_BAD_SYMBOL;
    p.sync();
    for (int i = 0; i < 19; ++i) {
        uint32_t v = 0;
        if (i < ncode) {
            refill(p, b);
            if (b.n < 3) return SPAA_PNG_INPUT_END;
            v = take(b, 3);
        }
        t.lens[order[i]] = (uint8_t)v;
    }
    int rc = build(p, t.lit, t.lens, 19, false);
    if (rc != SPAA_PNG_OK) return rc;
    p.sync();
    int i = 0;
    while (i < nlen + ndist) {
        refill(p, b);
        uint32_t l = 0;
        const int sym = decode(t.lit, (uint32_t)b.hold, l);
        if (sym == INVALID) return b.n < 15 ? SPAA_PNG_INPUT_END : SPAA_PNG_BAD_SYMBOL;
        if (l > b.n) return SPAA_PNG_INPUT_END;
        take(b, l);
        if (sym < 16) {
            t.lens[i++] = (uint8_t)sym;
            continue;
        }
        const uint32_t extra = sym == 16 ? 2 : sym == 17 ? 3 : 7;      // (a refill leaves >= 57 bits unless the input ends)
        if (extra > b.n) return SPAA_PNG_INPUT_END;
        uint32_t v = 0;
        if (sym == 16) {
            if (i == 0) return SPAA_PNG_BAD_REPEAT;
            v = t.lens[i - 1];
        }
        uint32_t rep = (sym == 18 ? 11 : 3) + take(b, extra);
        if (i + (int)rep > nlen + ndist) return SPAA_PNG_BAD_REPEAT;
        while (rep--) t.lens[i++] = (uint8_t)v;
    }
    if (t.lens[256] == 0) return SPAA_PNG_INCOMPLETE;              // no end-of-block code
    // the distance lengths move out of the way before the literal table is rebuilt over the code-length code
    p.sync();
    for (int k = ndist - 1; k >= 0; --k) t.lens[288 + k] = t.lens[nlen + k];      // (nlen <= 286: the ranges do not cross going down)
    rc = build(p, t.lit, t.lens, nlen, true);
    if (rc == SPAA_PNG_OK) rc = build(p, t.dist, t.lens + 288, ndist, true);
    return rc;
}

// in_len bytes of raw deflate -> exactly `expect` bytes.  Returns a SPAA_PNG_* status; on SPAA_PNG_OK `out_len` == expect.
template <class P>
PNGI_FN int inflate(P& p, Tables& t, uint32_t in_len, uint32_t expect, uint32_t& out_len) {
    const uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    const uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    const uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    Bits b = {0, 0, 0, in_len};
    uint32_t out = 0;
    out_len = 0;
    t.fixed_built = 0;
    uint32_t last;
    do {
        refill(p, b);
        if (b.n < 3) return SPAA_PNG_INPUT_END;
        last = take(b, 1);
        const uint32_t type = take(b, 2);
        if (type == 3) return SPAA_PNG_BAD_BLOCK_TYPE;
        if (type == 0) {
            take(b, b.n & 7);
            refill(p, b);
            if (b.n < 32) return SPAA_PNG_INPUT_END;
            const uint32_t len = take(b, 16), nlen = take(b, 16);
            if (len != (~nlen & 0xffffu)) return SPAA_PNG_STORED_LEN;
            b.pos -= b.n >> 3;                                    // whole bytes still in the buffer go back
            b.hold = 0;
            b.n = 0;
            if (len > in_len - b.pos) return SPAA_PNG_INPUT_END;
            if (len > expect - out) return SPAA_PNG_OUTPUT_LONG;
            for (uint32_t done = 0; done < len;) {
                const uint32_t piece = len - done < STORED_PIECE ? len - done : STORED_PIECE;
                p.stored(out, b.pos, piece);
                done += piece;
                out += piece;
                b.pos += piece;
                p.produced(out);
            }
            continue;
        }
        const int rc = type == 1 ? fixed_tables(p, t) : dynamic_tables(p, t, b);
        if (rc != SPAA_PNG_OK) return rc;
        for (;;) {
            refill(p, b);
            uint32_t l = 0;
            int sym = decode(t.lit, (uint32_t)b.hold, l);
            if (sym == INVALID) return b.n < 15 ? SPAA_PNG_INPUT_END : SPAA_PNG_BAD_SYMBOL;
            if (l > b.n) return SPAA_PNG_INPUT_END;
            take(b, l);
            if (sym < 256) {
                if (out >= expect) return SPAA_PNG_OUTPUT_LONG;
                p.hist(out) = (uint8_t)sym;
                ++out;
                p.produced(out);
                continue;
            }
            if (sym == 256) break;
            sym -= 257;
            if (sym >= 29) return SPAA_PNG_BAD_SYMBOL;
            if (lext[sym] > b.n) return SPAA_PNG_INPUT_END;       // (>= 28 bits are left after a refill unless the input ends)
            const uint32_t len = lbase[sym] + take(b, lext[sym]);
            refill(p, b);
            const int ds = decode(t.dist, (uint32_t)b.hold, l);
            if (ds == INVALID) return b.n < 15 ? SPAA_PNG_INPUT_END : SPAA_PNG_BAD_SYMBOL;
            if (l > b.n) return SPAA_PNG_INPUT_END;
            take(b, l);
            if (ds >= 30) return SPAA_PNG_BAD_SYMBOL;
            if (dext[ds] > b.n) return SPAA_PNG_INPUT_END;
            const uint32_t dist = dbase[ds] + take(b, dext[ds]);
            if (dist > out) return SPAA_PNG_DIST_TOO_FAR;
            if (len > expect - out) return SPAA_PNG_OUTPUT_LONG;
            // lanes: byte i of the match repeats the `dist` bytes before it; every source lies before `out`, so no byte of the
            // match is read after it was written
            p.sync();
            const uint32_t src = out - dist;
            if (dist >= len)
                for (uint32_t i = (uint32_t)p.lane(); i < len; i += (uint32_t)p.lanes()) p.hist(out + i) = p.hist(src + i);
            else
                for (uint32_t i = (uint32_t)p.lane(); i < len; i += (uint32_t)p.lanes()) p.hist(out + i) = p.hist(src + i % dist);
            p.sync();
            out += len;
            p.produced(out);
        }
    } while (!last);
    out_len = out;
    return out == expect ? SPAA_PNG_OK : SPAA_PNG_OUTPUT_SHORT;
}

}  // namespace pngi
