// png_inflate.h -- the part of the PNG decoder that touches untrusted bytes (png_decode.hip): the bit reader, the
// builder of the Huffman tables and the symbol decoder of RFC 1951.  It compiles for the device and, unchanged, for the host
// (tests/tools/png_inflate_host.cpp runs it under the host sanitizers): no HIP call, no wave intrinsic, no dynamic memory.
//
// What differs between the two is the SINK, a template parameter: it receives literals, matches and stored stretches and owns every
// store.  On the device all 64 lanes of a wavefront run the decoder on the same bits (loads of one address are one transaction) and
// the sink spreads the stores over the lanes; on the host the sink writes bytes.  A sink has
//   bool    lit(uint8_t v)                             false: the output is full
//   int32_t match(uint32_t dist, uint32_t len)         0, PNG_CORRUPT (reaches before the output's start) or PNG_WRONG_LENGTH (full)
//   int32_t stored(const uint8_t *z, int64_t from, uint32_t len)   the bytes z[from, from + len), which the caller has checked
//   void    finish()
// Bounds: every load of the stream goes through Bits::word or the check in front of a stored block, both against [0, n); every
// table index is a symbol or a bit pattern masked to the table's size; the sink checks every store against its own range.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PNGI_HD __host__ __device__ __forceinline__
#else
#define PNGI_HD inline
#endif

namespace soar {
namespace pngi {

// a file's status (SOAR_PNG_* of include/soar_hip.h)
constexpr int32_t PNG_OK = 0, PNG_BAD_STRUCTURE = 1, PNG_UNSUPPORTED = 2, PNG_BAD_CRC = 3, PNG_CORRUPT = 4, PNG_WRONG_LENGTH = 5,
                  PNG_BAD_ADLER = 6, PNG_BAD_FILTER = 7;

constexpr int LIT_FAST = 9, DIST_FAST = 6;      // bits answered by one look-up; longer codes are walked length by length
constexpr int MAX_LIT = 288, MAX_DIST = 32;

// The stream z[0, n), read from its least significant bits.  Bytes beyond n read as zeros, so a decoder that runs off the end stays
// inside the buffer and learns it from past_end().
struct Bits {
    const uint8_t *z;
    int64_t n;
    int64_t pos;                // bytes taken into buf
    uint64_t buf;
    int cnt;                    // valid bits of buf
    PNGI_HD Bits(const uint8_t *z_, int64_t n_, int64_t at) : z(z_), n(n_), pos(at), buf(0), cnt(0) {}
    PNGI_HD uint32_t word(int64_t p) const
    {
        uint32_t w = 0;
        if (p >= 0 && p + 4 <= n) {
            w = (uint32_t)z[p] | (uint32_t)z[p + 1] << 8 | (uint32_t)z[p + 2] << 16 | (uint32_t)z[p + 3] << 24;
        } else {
            for (int k = 0; k < 4; k++)
                if (p + k >= 0 && p + k < n) w |= (uint32_t)z[p + k] << (8 * k);
        }
        return w;
    }
    PNGI_HD void need()         // at least 33 bits behind it
    {
        if (cnt <= 32) {
            buf |= (uint64_t)word(pos) << cnt;
            pos += 4;
            cnt += 32;
        }
    }
    PNGI_HD uint32_t peek(int k) const { return (uint32_t)buf & ((1u << k) - 1u); }    // k <= 31
    PNGI_HD void drop(int k) { buf >>= k; cnt -= k; }
    PNGI_HD uint32_t take(int k) { need(); const uint32_t v = peek(k); drop(k); return v; }
    PNGI_HD int64_t bitpos() const { return 8 * pos - cnt; }
    PNGI_HD bool past_end() const { return bitpos() > 8 * n; }
    PNGI_HD void seek(int64_t byte) { pos = byte; buf = 0; cnt = 0; }
};

// A canonical code as counts per length and the symbols in code order, and the look-up of its short codes: sym | length << 9, 0
// where the bits begin no short code.
struct Code {
    uint16_t count[16];
    uint16_t offs[16];
    uint16_t symbol[MAX_LIT];
};

// everything the decoder indexes by data: in LDS on the device, so that nothing spills to scratch
struct Tables {
    Code lit, dist;
    uint16_t lit_fast[1 << LIT_FAST];
    uint16_t dist_fast[1 << DIST_FAST];
    uint8_t lens[MAX_LIT + MAX_DIST];
    uint16_t next[16];
};

PNGI_HD uint32_t reverse_bits(uint32_t v, int n)
{
    uint32_t r = 0;
    for (int i = 0; i < n; i++) { r = r << 1 | (v & 1u); v >>= 1; }
    return r;
}

// lens[0, n) -> code and look-up.  -1: over-subscribed; otherwise what the code lacks to be complete (0: complete; all lengths zero
// give 1 << 15).
PNGI_HD int build_code(Code &c, uint16_t *fast, int fast_bits, uint16_t *next, const uint8_t *lens, int n)
{
    for (int l = 0; l < 16; l++) c.count[l] = 0;
    for (int s = 0; s < n; s++) c.count[lens[s] & 15]++;
    int left = 1;
    for (int l = 1; l < 16; l++) {
        left = (left << 1) - (int)c.count[l];
        if (left < 0) return -1;
    }
    c.offs[1] = 0;
    for (int l = 1; l < 15; l++) c.offs[l + 1] = (uint16_t)(c.offs[l] + c.count[l]);
    for (int s = 0; s < n; s++) {
        const int l = lens[s] & 15;
        if (l) c.symbol[c.offs[l]++] = (uint16_t)s;
    }
    for (int i = 0; i < (1 << fast_bits); i++) fast[i] = 0;
    uint32_t code = 0;
    for (int l = 1; l < 16; l++) {                               // the first code of every length (RFC 1951, 3.2.2)
        code = (code + (l > 1 ? c.count[l - 1] : 0u)) << 1;
        next[l] = (uint16_t)code;
    }
    for (int s = 0; s < n; s++) {
        const int l = lens[s] & 15;
        if (l == 0 || l > fast_bits) continue;
        const uint32_t r = reverse_bits(next[l]++, l);
        for (uint32_t i = r; i < (1u << fast_bits); i += 1u << l) fast[i] = (uint16_t)(s | l << 9);
    }
    return left;
}

// one symbol; -1 where the bits are no code of an incomplete (or empty) code.  At most 15 bits are taken; need() first.
PNGI_HD int decode(Bits &br, const Code &c, const uint16_t *fast, int fast_bits)
{
    const uint32_t e = fast[br.peek(fast_bits)];
    if (e) {
        br.drop((int)(e >> 9));
        return (int)(e & 511u);
    }
    uint32_t v = br.peek(15);
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        code |= (int)(v & 1u);
        v >>= 1;
        const int count = c.count[l];
        if (code - count < first) {
            br.drop(l);
            const int at = index + (code - first);               // (below the number of symbols; clamped all the same)
            return c.symbol[at < MAX_LIT ? at : MAX_LIT - 1];
        }
        index += count;
        first = (first + count) << 1;
        code <<= 1;
    }
    return -1;
}

PNGI_HD void fixed_lengths(uint8_t *lens)
{
    for (int s = 0; s < 144; s++) lens[s] = 8;
    for (int s = 144; s < 256; s++) lens[s] = 9;
    for (int s = 256; s < 280; s++) lens[s] = 7;
    for (int s = 280; s < 288; s++) lens[s] = 8;
    for (int s = 0; s < 32; s++) lens[MAX_LIT + s] = 5;
}

// a dynamic block's header -> lens[0, 288) and lens[288, 320), the tables built.  0 or PNG_CORRUPT.
PNGI_HD int32_t dynamic_header(Bits &br, Tables &t)
{
    const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int nlen = (int)br.take(5) + 257, ndist = (int)br.take(5) + 1, ncode = (int)br.take(4) + 4;
    if (nlen > 286 || ndist > 30) return PNG_CORRUPT;
    // the code-length code borrows the distance code's tables
    for (int i = 0; i < 19; i++) t.lens[i] = 0;
    for (int i = 0; i < ncode; i++) t.lens[order[i]] = (uint8_t)br.take(3);
    if (build_code(t.dist, t.dist_fast, DIST_FAST, t.next, t.lens, 19) != 0) return PNG_CORRUPT;
    // (its own lengths are in the tables now: lens is free for the lengths it decodes)
    int i = 0;
    uint8_t prev = 0;
    while (i < nlen + ndist) {
        br.need();
        const int sym = decode(br, t.dist, t.dist_fast, DIST_FAST);
        if (sym < 0 || br.past_end()) return PNG_CORRUPT;
        if (sym < 16) {
            prev = (uint8_t)sym;
            t.lens[i < nlen ? i : MAX_LIT + (i - nlen)] = prev;
            i++;
            continue;
        }
        int rep;
        uint8_t v = 0;
        if (sym == 16) {
            if (i == 0) return PNG_CORRUPT;                      // nothing to repeat
            v = prev;
            rep = 3 + (int)br.take(2);
        } else if (sym == 17) {
            rep = 3 + (int)br.take(3);
        } else {
            rep = 11 + (int)br.take(7);
        }
        if (i + rep > nlen + ndist) return PNG_CORRUPT;
        for (; rep > 0; rep--, i++) t.lens[i < nlen ? i : MAX_LIT + (i - nlen)] = v;
        prev = v;
    }
    if (br.past_end()) return PNG_CORRUPT;
    if (t.lens[256] == 0) return PNG_CORRUPT;                    // no end of block
    for (int s = nlen; s < MAX_LIT; s++) t.lens[s] = 0;
    for (int s = ndist; s < MAX_DIST; s++) t.lens[MAX_LIT + s] = 0;
    if (build_code(t.lit, t.lit_fast, LIT_FAST, t.next, t.lens, MAX_LIT) != 0) return PNG_CORRUPT;
    const int left = build_code(t.dist, t.dist_fast, DIST_FAST, t.next, t.lens + MAX_LIT, MAX_DIST);
    // complete; or no distance code at all (a block of literals: using one is the error); or the one code of one bit that zlib
    // and png.hip write
    if (left != 0 && left != (1 << 15) && !(left == (1 << 14) && t.dist.count[1] == 1)) return PNG_CORRUPT;
    return PNG_OK;
}

// Decodes blocks from br's place.  last: the stream's final stretch, which ends with the final block, behind which exactly the four
// Adler bytes remain.  Otherwise the stretch z[.., n) of a stream cut at a block boundary: it ends where a block that is not final
// ends with the bit position exactly 8 n; a final block, or running past n, is an error.  -> a status.
template <class Sink> PNGI_HD int32_t inflate(Bits &br, Tables &t, Sink &sink, bool last)
{
    const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                                    4097, 6145, 8193, 12289, 16385, 24577};
    for (;;) {
        const uint32_t final = br.take(1), type = br.take(2);
        if (br.past_end()) return PNG_CORRUPT;
        if (type == 3) return PNG_CORRUPT;
        if (type == 0) {
            br.drop(br.cnt & 7);                                 // to the byte
            const uint32_t len = br.take(16), nlen = br.take(16);
            if (br.past_end()) return PNG_CORRUPT;
            if ((len ^ nlen) != 0xFFFFu) return PNG_CORRUPT;
            const int64_t from = br.bitpos() >> 3;
            if (from + (int64_t)len > br.n) return PNG_CORRUPT;  // the input ends inside the block
            const int32_t st = sink.stored(br.z, from, len);
            if (st) return st;
            br.seek(from + len);
        } else {
            if (type == 1) {
                fixed_lengths(t.lens);
                (void)build_code(t.lit, t.lit_fast, LIT_FAST, t.next, t.lens, MAX_LIT);
                (void)build_code(t.dist, t.dist_fast, DIST_FAST, t.next, t.lens + MAX_LIT, MAX_DIST);
            } else {
                const int32_t st = dynamic_header(br, t);
                if (st) return st;
            }
            for (;;) {
                br.need();
                const int sym = decode(br, t.lit, t.lit_fast, LIT_FAST);
                if (sym < 0 || br.past_end()) return PNG_CORRUPT;
                if (sym < 256) {
                    if (!sink.lit((uint8_t)sym)) return PNG_WRONG_LENGTH;
                    continue;
                }
                if (sym == 256) break;
                if (sym > 285) return PNG_CORRUPT;
                const int ls = sym - 257;
                const int leb = ls < 8 || ls == 28 ? 0 : (ls - 4) >> 2;
                const uint32_t len = len_base[ls] + br.peek(leb);
                br.drop(leb);
                br.need();
                const int ds = decode(br, t.dist, t.dist_fast, DIST_FAST);
                if (ds < 0 || ds > 29) return PNG_CORRUPT;
                const int deb = ds < 4 ? 0 : (ds - 2) >> 1;
                const uint32_t dist = dist_base[ds] + br.peek(deb);
                br.drop(deb);
                if (br.past_end()) return PNG_CORRUPT;
                const int32_t st = sink.match(dist, len);
                if (st) return st;
            }
        }
        if (final) {
            sink.finish();
            if (!last) return PNG_CORRUPT;
            const int64_t left = br.n - ((br.bitpos() + 7) >> 3);
            return left < 4 ? PNG_CORRUPT : (left > 4 ? PNG_WRONG_LENGTH : PNG_OK);
        }
        if (!last && br.bitpos() == 8 * br.n) {
            sink.finish();
            return PNG_OK;
        }
    }
}

// the zlib header's two bytes (RFC 1950)
PNGI_HD int32_t zlib_header(uint32_t cmf, uint32_t flg)
{
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u) return PNG_UNSUPPORTED;
    if ((cmf * 256u + flg) % 31u) return PNG_CORRUPT;
    if (flg & 32u) return PNG_UNSUPPORTED;                       // FDICT
    return PNG_OK;
}

// a sink that writes nothing: the first pass over a segment
struct CountSink {
    int64_t cap, pos;
    PNGI_HD CountSink(int64_t cap_) : cap(cap_), pos(0) {}
    PNGI_HD bool lit(uint8_t) { if (pos >= cap) return false; pos++; return true; }
    PNGI_HD int32_t match(uint32_t dist, uint32_t len)
    {
        if ((int64_t)dist > pos) return PNG_CORRUPT;
        if (pos + (int64_t)len > cap) return PNG_WRONG_LENGTH;
        pos += len;
        return PNG_OK;
    }
    PNGI_HD int32_t stored(const uint8_t *, int64_t, uint32_t len)
    {
        if (pos + (int64_t)len > cap) return PNG_WRONG_LENGTH;
        pos += len;
        return PNG_OK;
    }
    PNGI_HD void finish() {}
};

}  // namespace pngi
}  // namespace soar
