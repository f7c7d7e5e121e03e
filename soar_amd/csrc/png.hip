// png.hip -- PNG files on the device (soar_amd/png.py): B images of uint8 grey, RGB or RGBA in, B complete PNG files in one
// buffer out, so that only compressed bytes leave the device.  8 bit, colour types 0, 2 and 6, no interlace; the zlib stream is cut into
// independent pieces, each one deflate block with a Huffman code of its own over literals and run-length matches (distance 1 only).
// Every rule is stated in include/soar_hip.h and restated in tests/png_ref.py; all of it is integer arithmetic.
//   filter_kernel    a workgroup per row: the five filters' sums of |residual as int8|, the smallest (ties to the lowest type) or the
//                    forced type, and the filtered row (type byte first) into the workspace.  A row needs only the RAW row above.
//   measure_kernel   one wavefront per piece, lane k on byte 64 step + k: a ballot of the run starts gives every byte its offset in its
//                    run, which with the two bytes behind it decides its token (a match is charged to the LAST byte it covers, so no
//                    lane looks further ahead); symbol counts by LDS atomics; code lengths from the counts by wave reductions and
//                    ballots with the lengths in registers; the piece's size, its Adler-32 and the choice dynamic / stored.
//   emit_kernel      one wavefront per piece, after a scan of the sizes: the chunk framing, the block header and the tokens again, now
//                    placed by a wave prefix sum into an LDS bit buffer that is drained in whole bytes after every step; then the
//                    CRC-32 over what was written, 64 stretches in parallel, joined by multiplying with powers of x modulo the CRC's
//                    polynomial.  The first piece of an image also writes the signature and IHDR, the last the final IDAT and IEND.
// A piece is one wavefront's serial work (piece_bytes / 64 steps); the number of pieces is the parallelism.
#include "codec_common.h"
#include "png_common.h"

namespace soar {
namespace {

constexpr int NSYM = 286;                       // literal/length symbols
constexpr int LEN_STRIDE = 320;                 // bytes of a piece's code lengths in the workspace (5 per lane)
constexpr int SLOTS = 5;                        // symbols per lane: symbol s is slot s / 64 of lane s % 64
constexpr int HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4;
constexpr int FIRST_BYTES = 8 + 25 + 2;         // in front of an image's first piece: signature, IHDR, and 78 01 inside its IDAT
constexpr int LAST_BYTES = 18 + 12;             // behind its last: the final IDAT and IEND
constexpr int FILTER_THREADS = 256;

struct PngDev {
    const uint8_t *images;
    int64_t stride;             // bytes from image to image
    int32_t H, W, C, filter;    // filter: 0 .. 4 forced, -1 adaptive
    int32_t piece, np;          // bytes of a piece, pieces of an image
    int64_t S, n;               // filtered bytes of an image, B np
    uint8_t *filt;              // [B][S] the filtered streams
    uint8_t *lens;              // [n][LEN_STRIDE] code lengths
    uint32_t *adler;            // [n] the pieces' Adler-32
    int32_t *payload;           // [n] bytes of the piece's deflate blocks; negative: stored
    int64_t *sizes;             // [n + 1] measure: bytes of every piece with its chunk framing (and what an image's first and last carry); [n] = 0
    const int64_t *offs;        // [n + 1] emit: the exclusive scan of sizes; [n] = the total
    uint8_t *out;
    int64_t capacity;
};

// ---- filtering ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

// x: the byte, a: left, b: above, c: above left
__device__ __forceinline__ int residual(int type, int x, int a, int b, int c)
{
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255;
}

// grid (rows, images)
__global__ void __launch_bounds__(FILTER_THREADS) filter_kernel(PngDev a)
{
    __shared__ int sums[FILTER_THREADS / WAVE][5];
    const int tid = threadIdx.x, y = blockIdx.x, C = a.C, row = a.W * C;
    const uint8_t *cur = a.images + (int64_t)blockIdx.y * a.stride + (int64_t)y * row;
    const uint8_t *up = cur - row;                              // read for y > 0 only
    int type = a.filter;
    if (type < 0) {
        int s[5] = {0, 0, 0, 0, 0};
        for (int x = tid; x < row; x += FILTER_THREADS) {
            const int v = cur[x], l = x >= C ? cur[x - C] : 0, u = y > 0 ? up[x] : 0, ul = (y > 0 && x >= C) ? up[x - C] : 0;
#pragma unroll
            for (int t = 0; t < 5; t++) {
                const int r = residual(t, v, l, u, ul);
                s[t] += r < 128 ? r : 256 - r;
            }
        }
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const int w = wave_sum_i(s[t]);                     // (a row of 65535 x 4 bytes sums to 2^25 at the most)
            if ((tid & (WAVE - 1)) == 0) sums[tid / WAVE][t] = w;
        }
        __syncthreads();
        int best = 0;
        type = 0;
#pragma unroll
        for (int t = 0; t < 5; t++) {
            int w = 0;
            for (int k = 0; k < FILTER_THREADS / WAVE; k++) w += sums[k][t];
            if (t == 0 || w < best) { best = w; type = t; }
        }
    }
    uint8_t *dst = a.filt + (int64_t)blockIdx.y * a.S + (int64_t)y * (row + 1);
    if (tid == 0) dst[0] = (uint8_t)type;
    for (int x = tid; x < row; x += FILTER_THREADS) {
        const int v = cur[x], l = x >= C ? cur[x - C] : 0, u = y > 0 ? up[x] : 0, ul = (y > 0 && x >= C) ? up[x - C] : 0;
        dst[1 + x] = (uint8_t)residual(type, v, l, u, ul);
    }
}

// ---- tokens -------------------------------------------------------------------------------------------------------------------------
// A wavefront's walk over a piece, 64 bytes a step.  Of its byte (-1 behind the piece's end) every lane learns the two bytes behind it
// and k, its offset in its run of equal bytes.
struct Walk {
    const uint8_t *d;
    int n, lane;
    int nxt, prevlast, kprev;
    int cur, n1, n2, k;
    __device__ __forceinline__ Walk(const uint8_t *d_, int n_, int lane_) : d(d_), n(n_), lane(lane_), prevlast(-1), kprev(0)
    {
        nxt = lane < n ? (int)d[lane] : -1;
    }
    __device__ __forceinline__ void step(int i0)
    {
        const int i = i0 + lane;
        cur = nxt;
        nxt = i + WAVE < n ? (int)d[i + WAVE] : -1;
        const int w1 = __shfl(nxt, 0), w2 = __shfl(nxt, 1);
        n1 = __shfl_down(cur, 1);
        n2 = __shfl_down(cur, 2);
        if (lane == WAVE - 1) { n1 = w1; n2 = w2; }
        if (lane == WAVE - 2) n2 = w1;
        int p = __shfl_up(cur, 1);
        if (lane == 0) p = prevlast;
        const unsigned long long starts = __ballot(p != cur), below = starts & ((2ull << lane) - 1ull);
        k = below ? lane - (63 - __clzll((long long)below)) : kprev + 1 + lane;
        prevlast = __shfl(cur, WAVE - 1);
        kprev = __shfl(k, WAVE - 1);
    }
};

// The byte's token: sym < 0 none (behind the end, or inside a match), < 256 a literal, >= 257 a match of that length symbol at
// distance 1 with eb extra bits of value ev.  A run is one literal, then rest = N - 1 bytes in slots of 258: a slot with 3 bytes or
// more is a match, charged to its last byte; a last slot of 1 or 2 bytes is literals.
__device__ __forceinline__ void token_of(int cur, int n1, int n2, int k, int &sym, int &eb, int &ev)
{
    sym = -1; eb = 0; ev = 0;
    if (cur < 0) return;
    if (k == 0) { sym = cur; return; }
    const int r = (k - 1) % 258;                                // place in the slot
    if (r == 257 || n1 != cur) {                                // the slot's last byte
        const int len = r + 1;
        if (len < 3) { sym = cur; return; }
        if (len == 258) { sym = 285; return; }
        const int l = len - 3;
        if (l < 8) { sym = 257 + l; return; }
        eb = 29 - __clz(l);                                     // floor(log2 l) - 2
        sym = 261 + 4 * eb + ((l >> eb) & 3);
        ev = l & ((1 << eb) - 1);
    } else if (r == 0 && n2 != cur) {
        sym = cur;                                              // the first of a slot of 2
    }
}

__device__ __forceinline__ void piece_of(const PngDev &a, int64_t g, int64_t &image, int &p, int &n, const uint8_t *&d)
{
    image = g / a.np;
    p = (int)(g - image * a.np);
    const int64_t off = (int64_t)p * a.piece;
    n = (int)min((int64_t)a.piece, a.S - off);
    d = a.filt + image * a.S + off;
}

// ---- measuring ----------------------------------------------------------------------------------------------------------------------
// one wavefront (one workgroup: __syncthreads is the wave's own barrier) per piece
__global__ void __launch_bounds__(WAVE) measure_kernel(PngDev a)
{
    __shared__ uint32_t hist[SLOTS * WAVE];
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    int64_t image;
    int p, n;
    const uint8_t *d;
    piece_of(a, g, image, p, n, d);
#pragma unroll
    for (int j = 0; j < SLOTS; j++) hist[j * WAVE + lane] = 0u;
    __syncthreads();

    Walk w(d, n, lane);
    unsigned long long sa = 0ull, sb = 0ull;
    int extra = 0;
    for (int i0 = 0; i0 < n; i0 += WAVE) {
        w.step(i0);
        int sym, eb, ev;
        token_of(w.cur, w.n1, w.n2, w.k, sym, eb, ev);
        if (sym >= 0) atomicAdd(&hist[sym], 1u);
        if (sym >= 257) extra += eb + 1;                        // the extra bits and the distance code's one bit
        if (w.cur >= 0) {
            sa += (unsigned)w.cur;
            sb += (unsigned long long)(n - (i0 + lane)) * (unsigned)w.cur;
        }
    }
    if (lane == 0) atomicAdd(&hist[256], 1u);                   // the end of the block
    __syncthreads();

    // code lengths: Shannon's from counts raised to f, then shortened until the code is complete
    int c[SLOTS], l[SLOTS];
    int T = 0;
#pragma unroll
    for (int j = 0; j < SLOTS; j++) { c[j] = j * WAVE + lane < NSYM ? (int)hist[j * WAVE + lane] : 0; T += c[j]; }
    T = wave_sum_i(T);
    const int f = 1 + T / 32000;
    int T2 = 0;
#pragma unroll
    for (int j = 0; j < SLOTS; j++) T2 += c[j] > 0 ? max(c[j], f) : 0;
    T2 = wave_sum_i(T2);
    int K = 0, bits = 0;
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        l[j] = 0;
        if (c[j] > 0) {
            const uint32_t r = (uint32_t)max(c[j], f);
            int len = 1;
            while (len < 15 && (r << len) < (uint32_t)T2) len++;
            l[j] = len;
            K += 1 << (15 - len);
        }
    }
    int D = 32768 - wave_sum_i(K);
    for (int sweep = 0; D > 0 && sweep < 16; sweep++) {         // (a sweep shortens the longest code at least; 14 sweeps at the most)
        for (int L = 2; L <= 15; L++) {
#pragma unroll
            for (int j = 0; j < SLOTS; j++) {
                const unsigned long long at = __ballot(l[j] == L);
                const int take = min(__builtin_popcountll(at), D >> (15 - L));
                if (l[j] == L && __builtin_popcountll(at & ((1ull << lane) - 1ull)) < take) l[j] = L - 1;
                D -= take << (15 - L);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SLOTS; j++) {
        bits += c[j] * l[j];
        a.lens[g * LEN_STRIDE + j * WAVE + lane] = (uint8_t)l[j];
    }
    bits = wave_sum_i(bits) + wave_sum_i(extra);
    const int A = wave_sum_i((int)(sa % ADLER_MOD)), Bs = wave_sum_i((int)(sb % ADLER_MOD));
    if (lane == 0) {
        const int dynamic = (HEADER_BITS + bits + 3 + 7) / 8 + 4;       // with the empty stored block that aligns it
        const bool stored = dynamic >= n + 5;
        const int payload = stored ? n + 5 : dynamic;
        a.payload[g] = stored ? -payload : payload;
        a.adler[g] = ((uint32_t)(n + Bs) % ADLER_MOD) << 16 | ((1u + (uint32_t)A) % ADLER_MOD);
        a.sizes[g] = 12 + payload + (p == 0 ? FIRST_BYTES : 0) + (p == a.np - 1 ? LAST_BYTES : 0);
        if (g == 0) a.sizes[a.n] = 0;
    }
}

// ---- emitting -----------------------------------------------------------------------------------------------------------------------
// where a piece's wavefront may write: [lo, hi) of out
struct Sink {
    uint8_t *out;
    int64_t lo, hi;
    __device__ __forceinline__ void put(int64_t o, uint32_t v) const
    {
        if (o >= lo && o < hi) out[o] = (uint8_t)v;
    }
    __device__ __forceinline__ void put32(int64_t o, uint32_t v) const       // big-endian
    {
        put(o, v >> 24); put(o + 1, v >> 16); put(o + 2, v >> 8); put(o + 3, v);
    }
};

// len bits of v at bit p of the buffer: deflate fills a byte from its least significant end
__device__ __forceinline__ void put_bits(uint32_t *buf, uint32_t p, uint32_t v, int len)
{
    if (len == 0) return;
    const unsigned long long x = (unsigned long long)v << (p & 31u);
    if ((uint32_t)x) atomicOr(&buf[p >> 5], (uint32_t)x);
    if (x >> 32) atomicOr(&buf[(p >> 5) + 1], (uint32_t)(x >> 32));
}

// the whole bytes of the bit buffer go out at w; the bits of the last, partial byte move to the front
__device__ __forceinline__ void drain(uint32_t *buf, uint32_t &pos, int lane, const Sink &sink, int64_t &w)
{
    __syncthreads();
    const int nbytes = (int)(pos >> 3);
    for (int j = lane; j < nbytes; j += WAVE) sink.put(w + j, (buf[j >> 2] >> (8 * (j & 3))) & 255u);
    const uint32_t part = (buf[nbytes >> 2] >> (8 * (nbytes & 3))) & 255u;
    __syncthreads();
    buf[lane] = lane == 0 ? part : 0u;
    w += nbytes;
    pos &= 7u;
    __syncthreads();
}

__global__ void __launch_bounds__(WAVE) emit_kernel(PngDev a)
{
    __shared__ uint32_t table[SLOTS * WAVE];                    // symbol -> its code, first bit lowest | length << 16
    __shared__ uint32_t crctab[256];
    __shared__ uint32_t buf[WAVE];                              // the bit buffer: at most 7 + 64 x 21 bits in a step, 1222 in the header
    __shared__ uint8_t head[40];
    const int lane = threadIdx.x;
    const int64_t g = blockIdx.x;
    int64_t image;
    int p, n;
    const uint8_t *d;
    piece_of(a, g, image, p, n, d);
    const bool first = p == 0, last = p == a.np - 1;
    const int pl = a.payload[g];
    const bool stored = pl < 0;
    const int payload = stored ? -pl : pl;
    Sink sink;
    sink.out = a.out; sink.lo = a.offs[g]; sink.hi = a.offs[g + 1];
    // too small: nothing is written (the offsets say what is needed).  Offsets and sizes that are not a measure's write nothing either
    if (a.offs[a.n] > a.capacity || sink.lo < 0 || sink.hi > a.offs[a.n] ||
        sink.hi - sink.lo != 12 + (int64_t)payload + (first ? FIRST_BYTES : 0) + (last ? LAST_BYTES : 0) ||
        (stored ? payload != n + 5 : (payload < (HEADER_BITS + 3 + 7) / 8 + 4 || payload >= n + 5)))
        return;

    for (int i = lane; i < 256; i += WAVE) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
        crctab[i] = c;
    }
    buf[lane] = 0u;
    if (!stored) {
        // canonical codes (RFC 1951, 3.2.2): the codes of a length are consecutive, in symbol order
        int l[SLOTS];
        uint32_t code[SLOTS];
#pragma unroll
        for (int j = 0; j < SLOTS; j++) {
            l[j] = j * WAVE + lane < NSYM ? (int)(a.lens[g * LEN_STRIDE + j * WAVE + lane] & 15u) : 0;
            code[j] = 0u;
        }
        uint32_t next = 0u, count = 0u;
        for (int L = 1; L <= 15; L++) {
            next = (next + count) << 1;
            count = 0u;
#pragma unroll
            for (int j = 0; j < SLOTS; j++) {
                const unsigned long long at = __ballot(l[j] == L);
                if (l[j] == L) code[j] = next + count + (uint32_t)__builtin_popcountll(at & ((1ull << lane) - 1ull));
                count += (uint32_t)__builtin_popcountll(at);
            }
        }
#pragma unroll
        for (int j = 0; j < SLOTS; j++)
            table[j * WAVE + lane] = l[j] ? (__brev(code[j]) >> (32 - l[j])) | (uint32_t)l[j] << 16 : 0u;
    }
    __syncthreads();

    int64_t w = sink.lo;
    if (first) {
        if (lane == 0) {
            const uint8_t sig[16] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n', 0, 0, 0, 13, 'I', 'H', 'D', 'R'};
            for (int i = 0; i < 16; i++) head[i] = sig[i];
            for (int i = 0; i < 4; i++) { head[16 + i] = (uint8_t)((uint32_t)a.W >> (24 - 8 * i)); head[20 + i] = (uint8_t)((uint32_t)a.H >> (24 - 8 * i)); }
            head[24] = 8; head[25] = a.C == 1 ? 0 : (a.C == 3 ? 2 : 6); head[26] = 0; head[27] = 0; head[28] = 0;
            const uint32_t c = ~crc_bytes(crctab, 0xFFFFFFFFu, head + 12, 17);
            for (int i = 0; i < 4; i++) head[29 + i] = (uint8_t)(c >> (24 - 8 * i));
        }
        __syncthreads();
        if (lane < 33) sink.put(w + lane, head[lane]);
        w += 33;
    }
    const int64_t type_at = w + 4;
    if (lane == 0) {
        sink.put32(w, (uint32_t)(payload + (first ? 2 : 0)));
        sink.put(w + 4, 'I'); sink.put(w + 5, 'D'); sink.put(w + 6, 'A'); sink.put(w + 7, 'T');
        if (first) { sink.put(w + 8, 0x78); sink.put(w + 9, 0x01); }
    }
    w += 8 + (first ? 2 : 0);
    const int64_t data_end = w + payload;

    if (stored) {
        if (lane == 0) {
            sink.put(w, 0); sink.put(w + 1, (uint32_t)n); sink.put(w + 2, (uint32_t)n >> 8);
            sink.put(w + 3, ~(uint32_t)n); sink.put(w + 4, ~(uint32_t)n >> 8);
        }
        for (int i = lane; i < n; i += WAVE) sink.put(w + 5 + i, d[i]);
    } else {
        // the block's header: not final, dynamic; 286 literal/length codes, 1 distance code, 19 code-length codes of which 0 .. 15 have
        // 4 bits (so a length's code is the length) and 16 .. 18 none; then the 286 + 1 lengths
        uint32_t pos = 0u;
        if (lane == 0) put_bits(buf, 0u, 4u | 29u << 3 | 0u << 8 | 15u << 13, 17);
        if (lane >= 3 && lane < 19) put_bits(buf, 17u + 3u * lane, 4u, 3);
        for (int s = lane; s < NSYM + 1; s += WAVE) {
            const uint32_t len = s < NSYM ? table[s] >> 16 : 1u;
            put_bits(buf, 74u + 4u * s, __brev(len) >> 28, 4);
        }
        pos = HEADER_BITS;
        drain(buf, pos, lane, sink, w);

        Walk walk(d, n, lane);
        for (int i0 = 0; i0 < n; i0 += WAVE) {
            walk.step(i0);
            int sym, eb, ev;
            token_of(walk.cur, walk.n1, walk.n2, walk.k, sym, eb, ev);
            uint32_t v = 0u;
            int len = 0;
            if (sym >= 0) {
                const uint32_t e = table[sym];
                len = (int)(e >> 16);
                v = e & 0xFFFFu;
                if (sym >= 257) {                               // the extra bits, lowest first, and the distance code: one 0 bit
                    v |= (uint32_t)ev << len;
                    len += eb + 1;
                }
            }
            int inc = len;
            for (int s = 1; s < WAVE; s <<= 1) {
                const int o = __shfl_up(inc, s);
                if (lane >= s) inc += o;
            }
            put_bits(buf, pos + (uint32_t)(inc - len), v, len);
            pos += (uint32_t)__shfl(inc, WAVE - 1);
            drain(buf, pos, lane, sink, w);
        }
        // the end of the block, and an empty stored block: 000, zeros up to the byte, 00 00 FF FF
        const uint32_t eob = table[256];
        if (lane == 0) put_bits(buf, pos, eob & 0xFFFFu, (int)(eob >> 16));
        pos = (pos + (eob >> 16) + 3u + 7u) & ~7u;
        if (lane == 0) put_bits(buf, pos, 0xFFFF0000u, 32);
        pos += 32u;
        drain(buf, pos, lane, sink, w);
    }

    const uint32_t crc = crc_written(crctab, a.out, type_at, data_end, lane);
    if (lane == 0) sink.put32(data_end, crc);
    if (!last) return;

    // the final IDAT: an empty fixed block that is final, and the Adler-32 of the image's stream from its pieces'; then IEND
    const int64_t g0 = image * a.np;
    const int per = (a.np + WAVE - 1) / WAVE;
    uint32_t ad = 1u, len_mod = 0u;                             // of this lane's stretch of pieces
    for (int q = lane * per; q < min(a.np, (lane + 1) * per); q++) {
        const uint32_t nq = (uint32_t)min((int64_t)a.piece, a.S - (int64_t)q * a.piece);
        ad = adler_join(ad, a.adler[g0 + q], nq % ADLER_MOD);
        len_mod = (len_mod + nq) % ADLER_MOD;
    }
    uint32_t all = 1u;
    for (int j = 0; j < WAVE; j++) all = adler_join(all, (uint32_t)__shfl((int)ad, j), (uint32_t)__shfl((int)len_mod, j));
    if (lane == 0) {
        int64_t o = data_end + 4;
        const uint8_t tail[8] = {'I', 'D', 'A', 'T', 0x03, 0x00};
        for (int i = 0; i < 6; i++) head[i] = tail[i];
        for (int i = 0; i < 4; i++) head[6 + i] = (uint8_t)(all >> (24 - 8 * i));
        sink.put32(o, 6u);
        for (int i = 0; i < 10; i++) sink.put(o + 4 + i, head[i]);
        sink.put32(o + 14, ~crc_bytes(crctab, 0xFFFFFFFFu, head, 10));
        o += 18;
        const uint8_t iend[4] = {'I', 'E', 'N', 'D'};
        for (int i = 0; i < 4; i++) head[i] = iend[i];
        sink.put32(o, 0u);
        for (int i = 0; i < 4; i++) sink.put(o + 4 + i, head[i]);
        sink.put32(o + 8, ~crc_bytes(crctab, 0xFFFFFFFFu, head, 4));
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
struct Plan {
    PngDev d;
    SizeScan scan;
    size_t bytes;
};

bool plan_of(const char *me, const SoarPngArgs *args, void *workspace, Plan &p)
{
    if (!args) { set_error("%s: NULL args", me); return false; }
    const SoarPngArgs &a = *args;
    if (a.B < 0 || a.B > 65535 || a.H < 1 || a.W < 1 || a.H > 65535 || a.W > 65535 || (a.channels != 1 && a.channels != 3 && a.channels != 4) ||
        a.filter < -1 || a.filter > 4 || a.piece_bytes < 32 || a.piece_bytes > 65535) {
        set_error("%s: bad arguments (B=%d, H=%d, W=%d, channels=%d, filter=%d, piece_bytes=%d; need 0 <= B <= 65535, 1 <= H, W <= 65535, "
                  "channels 1, 3 or 4, filter -1 (adaptive) or 0 .. 4, 32 <= piece_bytes <= 65535)", me, a.B, a.H, a.W, a.channels, a.filter,
                  a.piece_bytes);
        return false;
    }
    PngDev &d = p.d;
    d.images = a.images; d.stride = a.image_stride; d.H = a.H; d.W = a.W; d.C = a.channels; d.filter = a.filter; d.piece = a.piece_bytes;
    d.S = (int64_t)a.H * (1 + (int64_t)a.W * a.channels);
    const int64_t np = (d.S + a.piece_bytes - 1) / a.piece_bytes;
    d.n = np * a.B;
    if (np > (1ll << 30) || d.n > (1ll << 30)) { set_error("%s: bad arguments (%lld pieces in the call; at most 2^30)", me, (long long)d.n); return false; }
    d.np = (int32_t)np;
    const size_t cnt = (size_t)d.n + 1;
    Carver c(workspace);
    d.filt = c.take<uint8_t>((size_t)a.B * (size_t)d.S);
    d.lens = c.take<uint8_t>((size_t)d.n * LEN_STRIDE);
    d.adler = c.take<uint32_t>(cnt);
    d.payload = c.take<int32_t>(cnt);
    carve_size_scan(c, p.scan, cnt);
    d.sizes = p.scan.sizes; d.offs = p.scan.offs;
    p.bytes = c.bytes();
    d.out = nullptr; d.capacity = 0;
    return true;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_png_workspace_bytes(const SoarPngArgs *args, size_t *bytes)
{
    return workspace_bytes_of("soar_png_workspace_bytes", plan_of, args, bytes);
}

int soar_png_measure(const SoarPngArgs *args, void *workspace, size_t workspace_bytes, int64_t *offsets, void *stream_)
{
    const char *me = "soar_png_measure";
    Plan p;
    if (!plan_of(me, args, workspace, p)) return 1;
    const SoarPngArgs &a = *args;
    if (!offsets) { set_error("%s: NULL offsets", me); return 1; }
    if (!workspace_ok(me, workspace, workspace_bytes, p.bytes, "soar_png_workspace_bytes")) return 1;
    if (!batch_ok(me, a.B, a.images, a.image_stride, (int64_t)a.H * a.W * a.channels, "images", "an image")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (a.B == 0) return no_item_offsets(offsets, stream);
    hipLaunchKernelGGL(filter_kernel, dim3((unsigned)a.H, (unsigned)a.B), dim3(FILTER_THREADS), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_filter", stream, 0);
    hipLaunchKernelGGL(measure_kernel, dim3((unsigned)p.d.n), dim3(WAVE), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_measure", stream, 0);
    return item_offsets("png_image_offsets", p.scan, a.B, p.d.np, offsets, stream);
}

int soar_png_emit(const SoarPngArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int64_t capacity, void *stream_)
{
    const char *me = "soar_png_emit";
    Plan p;
    if (!plan_of(me, args, workspace, p)) return 1;
    if (!emit_out_ok(me, out, capacity)) return 1;
    if (!workspace_ok(me, workspace, workspace_bytes, p.bytes, "soar_png_workspace_bytes")) return 1;
    if (args->B == 0) return 0;
    p.d.out = out; p.d.capacity = capacity;
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)p.d.n), dim3(WAVE), 0, static_cast<hipStream_t>(stream_), p.d);
    SOAR_LAUNCH_OK("png_emit", static_cast<hipStream_t>(stream_), 0);
    return 0;
}

}  // extern "C"
