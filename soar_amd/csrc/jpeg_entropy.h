// jpeg_entropy.h -- the part of the JPEG decoder that touches untrusted bytes (jpeg_decode.hip): the marker walk from
// SOI to the end of SOS, the builder of the Huffman tables, the bit reader with FF 00 unstuffing and the Huffman decode of a block and
// of a restart interval.  It compiles for the device and, unchanged, for the host (tests/tools/jpeg_entropy_host.cpp runs it under the
// host sanitizers): no HIP call, no wave intrinsic, no dynamic memory.
//
// Bounds: every read of the file is checked against its length L first (the walk) or goes through Bits::fill against [pos, end) (the
// scan); every table index is a symbol, a count checked at most 256, or bits masked to the table's size; a block is written at an
// index checked against the record's block count.  Every loop is bounded before it starts: the walk advances by at least two bytes
// per turn, a table has at most 256 codes, a block at most 63 AC symbols of at most 31 bits each, an interval the MCUs the frame
// header gives it.  Arithmetic on decoded values is unsigned where it could overflow (the DC predictor), and a shift is 1 .. 15.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JPGD_HD __host__ __device__ __forceinline__
#else
#define JPGD_HD inline
#endif

namespace soar {
namespace jpgd {

// a file's status (SOAR_JPEG_* of include/soar_hip.h)
constexpr int32_t JPEG_OK = 0, JPEG_BAD_STRUCTURE = 1, JPEG_UNSUPPORTED = 2, JPEG_MISSING_TABLE = 3, JPEG_CORRUPT = 4, JPEG_TRUNCATED = 5;

// A canonical code (Annex C): per length the first code, the index of its symbol and the count; and the look-up of the codes of 8
// bits and less: length << 8 | symbol, 0 where the 8 bits begin a longer code or none.
struct Huff {
    int32_t first[17], index[17];
    uint16_t count[17];
    uint16_t look[256];
    uint8_t vals[256];
    int32_t defined;
};

// what the walk learns of a file, and what the decoder needs of it
struct Rec {
    int32_t status;             // (first: the device's kernels merge the intervals' statuses into it)
    int32_t H, W, nc, ri;
    int32_t ids[3], hs[3], vs[3], tq[3], td[3], ta[3];
    int32_t mcu_cols, mcu_rows, mcus, blocks;
    int32_t bw[3], bh[3], off[3];   // a component's grid of blocks and its first block; its sample plane is [8 bh][8 bw] at 64 off
    int32_t n_int, has_end;         // the restart intervals, and whether a marker other than RSTn ends the segment
    int64_t scan, seg_end;          // the entropy-coded segment f[scan, seg_end)
    int32_t qdef[4];
    uint8_t q[4][64];               // natural order
    Huff dc[4], ac[4];
};

JPGD_HD int zigzag_of(int k)
{
    const uint8_t z[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return z[k & 63];
}

// bits: the 16 counts, vals: n = their sum <= 256 symbols.  false: the counts are no prefix code
JPGD_HD bool build_huff(Huff &t, const uint8_t *bits, const uint8_t *vals, int n)
{
    int32_t code = 0, k = 0;
    bool ok = true;
    t.first[0] = 0; t.index[0] = 0; t.count[0] = 0;
    for (int l = 1; l <= 16; l++) {
        t.first[l] = code;
        t.index[l] = k;
        t.count[l] = bits[l - 1];
        code += bits[l - 1];
        k += bits[l - 1];
        if (code > (1 << l)) ok = false;
        code <<= 1;
    }
    if (!ok || k != n || n > 256) return false;
    for (int i = 0; i < 256; i++) { t.vals[i] = i < n ? vals[i] : 0; t.look[i] = 0; }
    for (int l = 1; l <= 8; l++)
        for (int j = 0; j < t.count[l]; j++) {
            const int c = (t.first[l] + j) << (8 - l);           // (first + j < 2^l: the check above)
            for (int e = 0; e < (1 << (8 - l)); e++) t.look[(c + e) & 255] = (uint16_t)(l << 8 | t.vals[(t.index[l] + j) & 255]);
        }
    t.defined = 1;
    return true;
}

// Annex K's four tables: what a file without any DHT means (an MJPG chunk of an AVI)
JPGD_HD void standard_tables(Rec &r)
{
    const uint8_t dc_lum[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, dc_chr[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
    const uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    const uint8_t ac_lum[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, ac_chr[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
    const uint8_t ac_lum_vals[162] = {
        0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
        0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
        0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
        0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
        0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
        0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
        0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
        0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    const uint8_t ac_chr_vals[162] = {
        0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
        0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
        0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
        0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
        0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
        0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
        0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
        0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
    build_huff(r.dc[0], dc_lum, dc_vals, 12);
    build_huff(r.dc[1], dc_chr, dc_vals, 12);
    build_huff(r.ac[0], ac_lum, ac_lum_vals, 162);
    build_huff(r.ac[1], ac_chr, ac_chr_vals, 162);
}

JPGD_HD void geometry(Rec &r)
{
    r.mcu_cols = (r.W + 8 * r.hs[0] - 1) / (8 * r.hs[0]);
    r.mcu_rows = (r.H + 8 * r.vs[0] - 1) / (8 * r.vs[0]);
    r.mcus = r.mcu_cols * r.mcu_rows;                            // (at most 8192 x 8192)
    int32_t at = 0;
    for (int c = 0; c < 3; c++) {
        r.bw[c] = c < r.nc ? r.mcu_cols * r.hs[c] : 0;
        r.bh[c] = c < r.nc ? r.mcu_rows * r.vs[c] : 0;
        r.off[c] = at;
        at += r.bw[c] * r.bh[c];
    }
    r.blocks = at;
}

// The walk over f[0, L): SOI, the segments, to the end of SOS.  want_c = 0: any size and component count; otherwise the file must
// have want_h x want_w with want_c components.  -> the status; with JPEG_OK the record is complete up to r.scan and the geometry.
JPGD_HD int32_t parse(const uint8_t *f, int64_t L, int32_t want_h, int32_t want_w, int32_t want_c, Rec &r)
{
    r.nc = 0; r.ri = 0; r.H = 0; r.W = 0; r.blocks = 0; r.mcus = 0; r.n_int = 0; r.has_end = 0; r.scan = 0; r.seg_end = 0;
    for (int i = 0; i < 4; i++) { r.qdef[i] = 0; r.dc[i].defined = 0; r.ac[i].defined = 0; }
    bool any_dht = false;
    if (L < 2 || f[0] != 0xFF || f[1] != 0xD8) return JPEG_BAD_STRUCTURE;
    if (L > 0x7FFFFFFF) return JPEG_UNSUPPORTED;
    int64_t pos = 2;
    for (int64_t turn = 0; turn < L; turn++) {                  // (every turn takes at least four bytes)
        if (pos >= L || f[pos] != 0xFF) return JPEG_BAD_STRUCTURE;
        while (pos + 1 < L && f[pos + 1] == 0xFF) pos++;         // fill bytes
        if (pos + 1 >= L) return JPEG_BAD_STRUCTURE;
        const int m = f[pos + 1];
        pos += 2;
        if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD9)) return JPEG_BAD_STRUCTURE;
        if (pos + 2 > L) return JPEG_BAD_STRUCTURE;
        const int64_t n = (int64_t)f[pos] << 8 | f[pos + 1];
        if (n < 2 || pos + n > L) return JPEG_BAD_STRUCTURE;
        int64_t p = pos + 2;
        const int64_t e = pos + n;
        if (m == 0xC0) {
            if (r.nc || n < 8) return JPEG_BAD_STRUCTURE;
            const int prec = f[p], hh = f[p + 1] << 8 | f[p + 2], ww = f[p + 3] << 8 | f[p + 4], nc = f[p + 5];
            if (n != 8 + 3 * nc) return JPEG_BAD_STRUCTURE;
            if (prec != 8) return JPEG_UNSUPPORTED;
            if (hh == 0 || ww == 0) return JPEG_BAD_STRUCTURE;
            if (nc != 1 && nc != 3) return JPEG_UNSUPPORTED;
            bool tq_ok = true;
            for (int c = 0; c < nc; c++) {
                r.ids[c] = f[p + 6 + 3 * c];
                r.hs[c] = f[p + 7 + 3 * c] >> 4;
                r.vs[c] = f[p + 7 + 3 * c] & 15;
                r.tq[c] = f[p + 8 + 3 * c];
                if (r.tq[c] > 3) tq_ok = false;
            }
            if (!tq_ok) return JPEG_BAD_STRUCTURE;
            if (nc == 1) {
                if (r.hs[0] != 1 || r.vs[0] != 1) return JPEG_UNSUPPORTED;
            } else {
                if (r.hs[1] != 1 || r.vs[1] != 1 || r.hs[2] != 1 || r.vs[2] != 1) return JPEG_UNSUPPORTED;
                if (!((r.hs[0] == 1 && r.vs[0] == 1) || (r.hs[0] == 2 && r.vs[0] == 1) || (r.hs[0] == 2 && r.vs[0] == 2))) return JPEG_UNSUPPORTED;
            }
            if (want_c && (hh != want_h || ww != want_w || nc != want_c)) return JPEG_UNSUPPORTED;
            r.H = hh; r.W = ww; r.nc = nc;
        } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4) {
            return JPEG_UNSUPPORTED;                             // every other frame type, JPG and DAC
        } else if (m == 0xDC || m == 0xDE || m == 0xDF) {
            return JPEG_UNSUPPORTED;                             // DNL, DHP, EXP
        } else if (m == 0xDB) {
            while (p < e) {                                      // (a table takes 65 bytes)
                const int pq = f[p] >> 4, tq = f[p] & 15;
                if (pq > 1 || tq > 3) return JPEG_BAD_STRUCTURE;
                if (pq == 1) return JPEG_UNSUPPORTED;
                if (p + 65 > e) return JPEG_BAD_STRUCTURE;
                for (int k = 0; k < 64; k++) r.q[tq][zigzag_of(k)] = f[p + 1 + k];
                r.qdef[tq] = 1;
                p += 65;
            }
        } else if (m == 0xC4) {
            while (p < e) {                                      // (a table takes 17 bytes at the least)
                const int tc = f[p] >> 4, th = f[p] & 15;
                if (tc > 1 || th > 3 || p + 17 > e) return JPEG_BAD_STRUCTURE;
                int cnt = 0;
                for (int k = 0; k < 16; k++) cnt += f[p + 1 + k];
                if (cnt > 256 || p + 17 + cnt > e) return JPEG_BAD_STRUCTURE;
                Huff &t = tc ? r.ac[th] : r.dc[th];
                t.defined = 0;
                if (!build_huff(t, f + p + 1, f + p + 17, cnt)) return JPEG_BAD_STRUCTURE;
                any_dht = true;
                p += 17 + cnt;
            }
        } else if (m == 0xDD) {
            if (n != 4) return JPEG_BAD_STRUCTURE;
            r.ri = f[p] << 8 | f[p + 1];
        } else if (m == 0xDA) {
            if (!r.nc || n < 3) return JPEG_BAD_STRUCTURE;
            const int ns = f[p];
            if (n != 6 + 2 * ns) return JPEG_BAD_STRUCTURE;
            if (ns != r.nc) return JPEG_UNSUPPORTED;             // one interleaved scan of all components
            bool t_ok = true;
            for (int c = 0; c < ns; c++) {
                if (f[p + 1 + 2 * c] != r.ids[c]) return JPEG_UNSUPPORTED;
                r.td[c] = f[p + 2 + 2 * c] >> 4;
                r.ta[c] = f[p + 2 + 2 * c] & 15;
                if (r.td[c] > 3 || r.ta[c] > 3) t_ok = false;
            }
            if (!t_ok) return JPEG_BAD_STRUCTURE;
            if (f[p + 1 + 2 * ns] != 0 || f[p + 2 + 2 * ns] != 63 || f[p + 3 + 2 * ns] != 0) return JPEG_UNSUPPORTED;
            if (!any_dht) standard_tables(r);
            for (int c = 0; c < ns; c++)
                if (!r.qdef[r.tq[c]] || !r.dc[r.td[c]].defined || !r.ac[r.ta[c]].defined) return JPEG_MISSING_TABLE;
            r.scan = e;
            geometry(r);
            return JPEG_OK;
        }
        pos = e;
    }
    return JPEG_BAD_STRUCTURE;
}

// a marker inside entropy-coded data: FF followed by anything but 00 or FF
JPGD_HD bool marker_at(const uint8_t *f, int64_t L, int64_t p) { return p >= 0 && p + 1 < L && f[p] == 0xFF && f[p + 1] != 0x00 && f[p + 1] != 0xFF; }

// with k RSTn found in front of the segment's end: the interval count and the status of the count
JPGD_HD int32_t intervals_of(Rec &r, int64_t k)
{
    r.n_int = r.ri ? (r.mcus + r.ri - 1) / r.ri : 1;
    if (k != r.n_int - 1) return (k < r.n_int - 1 && !r.has_end) ? JPEG_TRUNCATED : JPEG_CORRUPT;
    return JPEG_OK;
}

// f[pos, end) from the most significant bit, FF 00 unstuffed.  Behind the end, or an FF that no 00 follows, the bits are zeros, and
// past_end() says that one of those was taken.
struct Bits {
    const uint8_t *f;
    int64_t pos, end;
    uint32_t acc;
    int32_t cnt, fake;
    JPGD_HD Bits(const uint8_t *f_, int64_t pos_, int64_t end_) : f(f_), pos(pos_), end(end_), acc(0), cnt(0), fake(0) {}
    JPGD_HD void fill()
    {
        while (cnt <= 24) {                                      // (four turns at the most)
            uint32_t b = 0;
            if (pos < end) {
                b = f[pos++];
                if (b == 0xFF) {
                    if (pos < end && f[pos] == 0) { pos++; } else { pos = end; b = 0; fake += 8; }
                }
            } else {
                fake += 8;
            }
            acc = acc << 8 | b;
            cnt += 8;
        }
    }
    JPGD_HD uint32_t peek16() { fill(); return (acc >> (cnt - 16)) & 0xFFFFu; }
    JPGD_HD void drop(int n) { cnt -= n; }
    JPGD_HD uint32_t take(int n) { const uint32_t v = peek16() >> (16 - n); cnt -= n; return v; }   // n 1 .. 15
    JPGD_HD bool past_end() const { return fake > cnt; }
};

// -> the symbol, or -1 where the next 16 bits begin no code
JPGD_HD int decode_symbol(Bits &br, const Huff &t)
{
    const uint32_t v = br.peek16();
    const uint32_t e = t.look[v >> 8];
    if (e) { br.drop((int)(e >> 8)); return (int)(e & 255u); }
    for (int l = 9; l <= 16; l++) {
        const int32_t d = (int32_t)(v >> (16 - l)) - t.first[l];
        if (d >= 0 && d < (int32_t)t.count[l]) { br.drop(l); return t.vals[(t.index[l] + d) & 255]; }
    }
    return -1;
}

JPGD_HD int32_t extend(uint32_t v, int s) { return v >= (1u << (s - 1)) ? (int32_t)v : (int32_t)v - ((1 << s) - 1); }   // s 1 .. 15

// one block into out[64], natural order, zeros before; pred: the component's DC predictor
JPGD_HD int32_t decode_block(Bits &br, const Huff &dc, const Huff &ac, uint32_t &pred, int16_t *out)
{
    const int s0 = decode_symbol(br, dc);
    if (s0 < 0 || s0 > 15) return JPEG_CORRUPT;
    int32_t diff = 0;
    if (s0) diff = extend(br.take(s0), s0);
    pred += (uint32_t)diff;
    out[0] = (int16_t)(uint16_t)(pred & 0xFFFFu);
    int k = 1;
    for (int turn = 0; turn < 63 && k < 64; turn++) {           // (every turn takes k up by one at the least)
        const int rs = decode_symbol(br, ac);
        if (rs < 0) return JPEG_CORRUPT;
        const int run = rs >> 4, s = rs & 15;
        if (s) {
            k += run;
            if (k > 63) return JPEG_CORRUPT;
            out[zigzag_of(k)] = (int16_t)extend(br.take(s), s);
            k++;
        } else if (run == 15) {
            k += 16;
            if (k > 64) return JPEG_CORRUPT;
        } else {
            break;
        }
    }
    return JPEG_OK;
}

// the MCUs [mcu0, mcu0 + n) from f[start, end) into the file's coefficients coef[blocks][64].  last_open: the file's last interval
// with no marker behind it, where running out of bits means a truncated file; anywhere else a misplaced marker.
JPGD_HD int32_t decode_interval(const uint8_t *f, const Rec &r, int16_t *coef, int64_t start, int64_t end, int32_t mcu0, int32_t n, bool last_open)
{
    Bits br(f, start, end);
    uint32_t pred[3] = {0u, 0u, 0u};
    for (int32_t m = mcu0; m < mcu0 + n; m++) {
        const int32_t my = m / r.mcu_cols, mx = m - my * r.mcu_cols;
        for (int c = 0; c < r.nc; c++)
            for (int v = 0; v < r.vs[c]; v++)
                for (int u = 0; u < r.hs[c]; u++) {
                    const int32_t blk = r.off[c] + (my * r.vs[c] + v) * r.bw[c] + mx * r.hs[c] + u;
                    if (blk < 0 || blk >= r.blocks) return JPEG_CORRUPT;            // (cannot happen: m < mcus)
                    const int32_t st = decode_block(br, r.dc[r.td[c] & 3], r.ac[r.ta[c] & 3], pred[c], coef + (int64_t)blk * 64);
                    if (br.past_end()) return last_open ? JPEG_TRUNCATED : JPEG_CORRUPT;
                    if (st != JPEG_OK) return st;
                }
    }
    return JPEG_OK;
}

}  // namespace jpgd
}  // namespace soar
