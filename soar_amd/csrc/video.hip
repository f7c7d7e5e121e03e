// video.hip -- baseline JPEG on the device (soar_amd/video.py): B frames of uint8 RGB(A) in, B complete JPEG files in one
// buffer out, so that only compressed bytes leave the device.  Baseline sequential, 8 bit, three components, 4:4:4 or 4:2:0, the four
// Annex K Huffman tables, restart markers.  Every rule is libjpeg's and exact in integers (include/soar_hip.h states them).
//   transform_kernel   a tile of 64 x 8 (4:4:4) or 64 x 16 (4:2:0) pixels per workgroup: colour conversion and chroma downsampling into
//                      LDS, then 8 threads per 8x8 block run jfdctint's row and column passes, quantise and zigzag; the tile's 24
//                      blocks leave as int16 coefficients in coding order (MCU after MCU).  A frame's pixels are read once.
//   entropy_kernel     one wavefront per restart interval, lane k holding zigzag coefficient k of the block in hand: a ballot gives
//                      the non-zero mask, a lane's run is the distance to the set bit below it, its bits are its ZRLs, its code and its
//                      value (59 bits at the most), a wave prefix sum places them in an LDS bit buffer.  After every block the whole
//                      bytes are drained: 0xFF bytes counted by ballot and, when writing, followed by 0x00.  The restart intervals are
//                      byte-aligned and independent, so this kernel runs twice: once counting (soar_jpeg_measure; the stuffed lengths
//                      go through a scan), once writing at the final offsets (soar_jpeg_emit).  Coding twice was chosen over a buffer of
//                      unstuffed bits, which would have to hold the worst case (208 bytes a block) and be written and read back.
// An interval is one wavefront's serial work: a large restart_interval is correct and slow (one wavefront per frame at the extreme).
#include "codec_common.h"

namespace soar {
namespace {

constexpr int HEADER_BYTES = 629;               // SOI, APP0, DQT x 2, SOF0, DHT x 4, DRI, SOS
constexpr int TILE_W = 64;                      // pixels of a transform tile across
constexpr int TILE_BLOCKS = 24;                 // 8 MCUs of 3 blocks, or 4 MCUs of 6
constexpr int TRANSFORM_THREADS = 256;

// ---- literal data: Annex K ----------------------------------------------------------------------------------------------------------
struct HuffSpec {
    uint8_t bits[16];           // codes of length 1 .. 16
    uint8_t vals[162];
    int n;
};
constexpr HuffSpec DC_LUM = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec DC_CHR = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec AC_LUM = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}, 162};
constexpr HuffSpec AC_CHR = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}, 162};
// zigzag position k -> natural index, and the inverse
constexpr uint8_t NATURAL_OF_ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct Zigzag { uint8_t pos[64]; };
constexpr Zigzag zigzag_of_natural()
{
    Zigzag z{};
    for (int k = 0; k < 64; k++) z.pos[NATURAL_OF_ZIGZAG[k]] = (uint8_t)k;
    return z;
}
__device__ const Zigzag ZIGZAG_OF_NATURAL = zigzag_of_natural();

// symbol -> code << 8 | length (Annex C's canonical assignment), worked out by the compiler from the literal tables
struct HuffCodes { uint32_t e[256]; };
constexpr HuffCodes derive(const HuffSpec &s)
{
    HuffCodes t{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int i = 0; i < s.bits[len - 1]; i++) t.e[s.vals[k++]] = code++ << 8 | (uint32_t)len;
        code <<= 1;
    }
    return t;
}
__device__ const HuffCodes DC_LUM_CODES = derive(DC_LUM), DC_CHR_CODES = derive(DC_CHR), AC_LUM_CODES = derive(AC_LUM), AC_CHR_CODES = derive(AC_CHR);

// ---- the transform ------------------------------------------------------------------------------------------------------------------
struct TransformDev {
    const uint8_t *frames;
    int64_t stride;             // bytes from frame to frame
    int32_t H, W, C, wide;      // wide: C == 4 and every pixel on 4 bytes -- one load per pixel
    int32_t mcux;
    int64_t nmcu;
    int16_t *coef;
    uint16_t q8[2][64];         // 8 Q, natural order
};

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint's pass over eight values; FIRST: the row pass, whose outputs stay scaled up by PASS1_BITS = 2 (CONST_BITS = 13)
template <bool FIRST> __device__ __forceinline__ void dct8(const int (&d)[8], int (&o)[8])
{
    constexpr int N = FIRST ? 13 - 2 : 13 + 2;
    int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    o[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    o[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    o[2] = descale(z1 + t13 * 6270, N);
    o[6] = descale(z1 - t12 * 15137, N);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    o[7] = descale(t4 + z1 + z3, N);
    o[5] = descale(t5 + z2 + z4, N);
    o[3] = descale(t6 + z2 + z3, N);
    o[1] = descale(t7 + z1 + z4, N);
}

__device__ __forceinline__ void load_rgb(const TransformDev &a, const uint8_t *frame, int y, int x, int &r, int &g, int &b)
{
    const int64_t p = (int64_t)y * a.W + x;
    if (a.wide) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(frame + p * 4);
        r = v & 255u; g = (v >> 8) & 255u; b = (v >> 16) & 255u;
    } else {
        const uint8_t *q = frame + p * a.C;
        r = q[0]; g = q[1]; b = q[2];
    }
}

// HS = 1: 4:4:4, a tile of 64 x 8 pixels = 8 MCUs of (Y, Cb, Cr).  HS = 2: 4:2:0, 64 x 16 pixels = 4 MCUs of (Y00, Y01, Y10, Y11, Cb, Cr).
// grid (tiles across, MCU rows, frames).  Pixels beyond the image are the clamped ones (replication of the last column and row);
// at 4:2:0 the chroma rows follow libjpeg: the last row replicated to an even height, and below that copies of the last
// DOWNSAMPLED row -- for an even H not a multiple of 16 those average rows H - 2 and H - 1, not row H - 1 alone.
template <int HS>
__global__ void __launch_bounds__(TRANSFORM_THREADS) transform_kernel(TransformDev a)
{
    constexpr int ROWS = 8 * HS, G = 8 / HS, BPM = HS == 2 ? 6 : 3;
    __shared__ uint8_t sY[ROWS][TILE_W];
    __shared__ uint8_t sC[2][ROWS][TILE_W];
    __shared__ uint8_t sD[2][8][TILE_W / 2];                    // the downsampled chroma (4:2:0 only)
    __shared__ int32_t work[TILE_BLOCKS][64];
    __shared__ __align__(4) int16_t zz[TILE_BLOCKS][64];
    const int tid = threadIdx.x, tile = blockIdx.x, my = blockIdx.y;
    const int x0 = tile * TILE_W, y0 = my * ROWS, H = a.H, W = a.W;
    const uint8_t *frame = a.frames + (int64_t)blockIdx.z * a.stride;

    for (int p = tid; p < TILE_W * ROWS; p += TRANSFORM_THREADS) {
        const int x = p & (TILE_W - 1), y = p / TILE_W;
        const int gx = min(x0 + x, W - 1), gy = min(y0 + y, H - 1);
        int r, g, b;
        load_rgb(a, frame, gy, gx, r, g, b);
        sY[y][x] = (uint8_t)((19595 * r + 38470 * g + 7471 * b + 32768) >> 16);
        if (HS == 2) {
            const int cj = min((y0 + y) >> 1, ((H + 1) >> 1) - 1), gyc = min(2 * cj + (y & 1), H - 1);
            if (gyc != gy) load_rgb(a, frame, gyc, gx, r, g, b);
        }
        sC[0][y][x] = (uint8_t)((-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16);
        sC[1][y][x] = (uint8_t)((32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16);
    }
    __syncthreads();
    if (HS == 2) {
        for (int o = tid; o < 2 * 8 * (TILE_W / 2); o += TRANSFORM_THREADS) {
            const int c = o >> 8, oy = (o >> 5) & 7, ox = o & 31;
            const int s = sC[c][2 * oy][2 * ox] + sC[c][2 * oy][2 * ox + 1] + sC[c][2 * oy + 1][2 * ox] + sC[c][2 * oy + 1][2 * ox + 1];
            sD[c][oy][ox] = (uint8_t)((s + 1 + (ox & 1)) >> 2);
        }
        __syncthreads();
    }

    // 8 threads per block: thread i of a block takes row i, then column i
    const int blk = tid >> 3, i = tid & 7;
    const int m = blk / BPM, k = blk - m * BPM;                 // MCU of the tile, block of the MCU
    const bool works = blk < TILE_BLOCKS;
    if (works) {
        const uint8_t *row;
        if (HS == 1) row = k == 0 ? &sY[i][m * 8] : &sC[k - 1][i][m * 8];
        else row = k < 4 ? &sY[(k >> 1) * 8 + i][m * 16 + (k & 1) * 8] : &sD[k - 4][i][m * 8];
        int d[8], o[8];
#pragma unroll
        for (int c = 0; c < 8; c++) d[c] = (int)row[c] - 128;
        dct8<true>(d, o);
#pragma unroll
        for (int c = 0; c < 8; c++) work[blk][i * 8 + c] = o[c];
    }
    __syncthreads();
    if (works) {
        // a luma block of a 4:2:0 MCU beyond the ceil(W / 8) x ceil(H / 8) real ones is a dummy: no AC, and its DC set below
        const bool dummy = HS == 2 && k < 4 && ((tile * G + m) * 2 + (k & 1) >= (W + 7) / 8 || my * 2 + (k >> 1) >= (H + 7) / 8);
        const uint16_t *q8 = a.q8[(HS == 1 ? k : k - 3) > 0 ? 1 : 0];
        int d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; r++) d[r] = work[blk][r * 8 + i];
        dct8<false>(d, o);
#pragma unroll
        for (int r = 0; r < 8; r++) {
            const int nat = r * 8 + i;
            const uint32_t q = q8[nat], mag = ((uint32_t)abs(o[r]) + (q >> 1)) / q;
            zz[blk][ZIGZAG_OF_NATURAL.pos[nat]] = dummy ? (int16_t)0 : (int16_t)(o[r] < 0 ? -(int)mag : (int)mag);
        }
    }
    __syncthreads();
    if (HS == 2) {
        // a dummy block's DC is the DC of the block coded before it in the MCU: one thread per MCU, in coding order
        if (tid < G) {
            for (int kk = 1; kk < 4; kk++)
                if ((tile * G + tid) * 2 + (kk & 1) >= (W + 7) / 8 || my * 2 + (kk >> 1) >= (H + 7) / 8) zz[tid * BPM + kk][0] = zz[tid * BPM + kk - 1][0];
        }
        __syncthreads();
    }
    // the tile's MCUs that exist are consecutive in coding order
    const int nm = min(G, a.mcux - tile * G);
    const int64_t first = ((int64_t)blockIdx.z * a.nmcu + (int64_t)my * a.mcux + (int64_t)tile * G) * BPM;
    uint32_t *dst = reinterpret_cast<uint32_t *>(a.coef + first * 64);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(&zz[0][0]);
    for (int w = tid; w < nm * BPM * 32; w += TRANSFORM_THREADS) dst[w] = src[w];
}

// ---- the entropy coder --------------------------------------------------------------------------------------------------------------
struct EntropyDev {
    const int16_t *coef;
    int64_t *sizes;             // [n + 1] measure: bytes of every interval with its marker (and the header in front of a frame's first); [n] = 0
    const int64_t *offs;        // [n + 1] emit: the exclusive scan of sizes; [n] = the total
    uint8_t *out;
    int64_t capacity;
    int64_t n_int, nmcu, n;     // intervals per frame, MCUs per frame, B n_int
    int32_t ri, bpm;
    uint8_t header[HEADER_BYTES + 3];
};

// drain the whole bytes of the bit buffer: counted, and with WRITE written at dst + outpos, every 0xFF followed by 0x00 (never at or
// behind dst + limit); the bits of the last, partial byte move to the front
template <bool WRITE>
__device__ __forceinline__ void drain(uint32_t *buf, uint32_t &pos, int lane, uint8_t *dst, int64_t limit, int64_t &outpos)
{
    __syncthreads();
    const int nbytes = (int)(pos >> 3);
    for (int c0 = 0; c0 < nbytes; c0 += WAVE) {
        const int j = c0 + lane;
        const bool valid = j < nbytes;
        const uint32_t byte = valid ? (buf[j >> 2] >> (24 - 8 * (j & 3))) & 255u : 0u;
        const bool ff = byte == 255u;
        const unsigned long long m = __ballot(ff);
        if (WRITE && valid) {
            const int64_t o = outpos + lane + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            if (o + (ff ? 1 : 0) < limit) {
                dst[o] = (uint8_t)byte;
                if (ff) dst[o + 1] = 0;
            }
        }
        outpos += min(WAVE, nbytes - c0) + __builtin_popcountll(m);
    }
    const uint32_t part = (buf[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u;
    __syncthreads();
    buf[lane] = lane == 0 ? part << 24 : 0u;
    pos &= 7u;
    __syncthreads();
}

// one wavefront (one workgroup: __syncthreads is the wave's own barrier) per restart interval
template <bool WRITE>
__global__ void __launch_bounds__(WAVE) entropy_kernel(EntropyDev a)
{
    __shared__ uint32_t ac[2][256], dc[2][16];
    __shared__ uint32_t buf[WAVE];                              // the bit buffer, most significant bit first: at most 7 + 1660 bits
    const int lane = threadIdx.x;
    const int64_t gi = blockIdx.x;
    if (WRITE) {
        // too small: nothing is written (the offsets say what is needed).  Offsets that are not a measure's (out of order, or not
        // leaving room for the header and the marker) write nothing either
        const int64_t lo = a.offs[gi], hi = a.offs[gi + 1];
        if (a.offs[a.n] > a.capacity || lo < 0 || hi > a.offs[a.n] || hi - lo < 2 + (gi % a.n_int == 0 ? HEADER_BYTES : 0)) return;
    }
    for (int i = lane; i < 256; i += WAVE) { ac[0][i] = AC_LUM_CODES.e[i]; ac[1][i] = AC_CHR_CODES.e[i]; }
    if (lane < 16) { dc[0][lane] = DC_LUM_CODES.e[lane]; dc[1][lane] = DC_CHR_CODES.e[lane]; }
    buf[lane] = 0u;
    __syncthreads();

    const int64_t frame = gi / a.n_int, ii = gi - frame * a.n_int;
    const int64_t m0 = ii * a.ri, m1 = min(m0 + a.ri, a.nmcu);
    const int64_t nblk = (m1 - m0) * a.bpm;
    const int16_t *coef = a.coef + (frame * a.nmcu + m0) * a.bpm * 64;
    uint8_t *dst = nullptr;
    int64_t limit = 0, outpos = 0;
    if (WRITE) {
        int64_t base = a.offs[gi];
        if (ii == 0) {
            for (int i = lane; i < HEADER_BYTES; i += WAVE) a.out[base + i] = a.header[i];
            base += HEADER_BYTES;
        }
        dst = a.out + base;
        limit = a.offs[gi + 1] - base - 2;                      // the interval's own bytes; its marker follows
    }

    int pred[3] = {0, 0, 0};
    uint32_t pos = 0;
    int bi = 0;                                                 // block of the MCU
    int next = nblk > 0 ? (int)coef[lane] : 0;
    for (int64_t j = 0; j < nblk; j++) {
        const int v = next;
        if (j + 1 < nblk) next = (int)coef[(j + 1) * 64 + lane];
        const int comp = a.bpm == 3 ? bi : (bi < 4 ? 0 : bi - 3);
        const int t = comp ? 1 : 0;
        bi = bi + 1 == a.bpm ? 0 : bi + 1;
        const int dcv = __shfl(v, 0);
        const int diff = dcv - pred[comp];
        pred[comp] = dcv;
        const unsigned long long nz = __ballot(v != 0);
        unsigned long long bits = 0ull;
        int len = 0;
        if (lane == 0) {
            const int n = min(32 - __clz(abs(diff)), 11);       // (8-bit samples give 11 at the most; the bound keeps the buffer's)
            const uint32_t e = dc[t][n];
            bits = (unsigned long long)(e >> 8) << n | (uint32_t)((diff > 0 ? diff : diff - 1) & ((1 << n) - 1));
            len = (int)(e & 255u) + n;
        } else if (v != 0) {
            const unsigned long long below = nz & ((1ull << lane) - 1ull) & ~1ull;
            const int prev = below ? 63 - __clzll((long long)below) : 0;
            const int run = lane - prev - 1;
            const uint32_t zrl = ac[t][0xF0];
            for (int z = 0; z < (run >> 4); z++) { bits = bits << (zrl & 255u) | (zrl >> 8); len += (int)(zrl & 255u); }
            const int n = min(32 - __clz(abs(v)), 10);          // (8-bit samples give 10 at the most)
            const uint32_t e = ac[t][((run & 15) << 4) | n];
            bits = (bits << (e & 255u) | (e >> 8)) << n | (uint32_t)((v > 0 ? v : v - 1) & ((1 << n) - 1));
            len += (int)(e & 255u) + n;
        } else if (lane == 63) {
            const uint32_t e = ac[t][0x00];                     // EOB: the block ends in zeros
            bits = e >> 8;
            len = (int)(e & 255u);
        }
        int inc = len;
        for (int d = 1; d < WAVE; d <<= 1) {
            const int o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (len) {
            const uint32_t p = pos + (uint32_t)(inc - len), s = p & 31u, w = p >> 5;
            const unsigned long long x = bits << (64 - len), hi = x >> s;
            const uint32_t lo = s ? (uint32_t)((x << (64u - s)) >> 32) : 0u;
            if (hi >> 32) atomicOr(&buf[w], (uint32_t)(hi >> 32));
            if ((uint32_t)hi) atomicOr(&buf[w + 1], (uint32_t)hi);
            if (lo) atomicOr(&buf[w + 2], lo);
        }
        pos += (uint32_t)__shfl(inc, 63);
        drain<WRITE>(buf, pos, lane, dst, limit, outpos);
    }
    if (pos) {                                                  // 1-bits up to the byte
        if (lane == 0) buf[0] |= ((1u << (8u - pos)) - 1u) << 24;
        pos = 8u;
        drain<WRITE>(buf, pos, lane, dst, limit, outpos);
    }
    if (lane == 0) {
        if (WRITE) {
            if (outpos == limit) {
                dst[outpos] = 0xFF;
                dst[outpos + 1] = ii + 1 < a.n_int ? (uint8_t)(0xD0 + (ii & 7)) : (uint8_t)0xD9;      // RSTm, or EOI behind the frame's last
            }
        } else {
            a.sizes[gi] = outpos + 2 + (ii == 0 ? HEADER_BYTES : 0);
            if (gi == 0) a.sizes[a.n] = 0;
        }
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
struct Plan {
    int hs, bpm, mcux, mcuy;
    int64_t nmcu, n_int, n;
    int16_t *coef;
    SizeScan scan;
    size_t bytes;
};

bool plan_of(const char *me, const SoarJpegArgs *args, void *workspace, Plan &p)
{
    if (!args) { set_error("%s: NULL args", me); return false; }
    const SoarJpegArgs &a = *args;
    if (a.B < 0 || a.B > 65535 || a.H < 1 || a.W < 1 || a.H > 65535 || a.W > 65535 || (a.channels != 3 && a.channels != 4) ||
        (a.subsampling != 444 && a.subsampling != 420) || a.restart_interval < 1 || a.restart_interval > 65535) {
        set_error("%s: bad arguments (B=%d, H=%d, W=%d, channels=%d, subsampling=%d, restart_interval=%d; need 0 <= B <= 65535, 1 <= H, W <= 65535, "
                  "channels 3 or 4, subsampling 444 or 420, 1 <= restart_interval <= 65535)", me, a.B, a.H, a.W, a.channels, a.subsampling,
                  a.restart_interval);
        return false;
    }
    for (int i = 0; i < 128; i++)
        if (a.qtables[i / 64][i % 64] == 0) { set_error("%s: bad arguments (a quantisation table entry is 0; need 1 .. 255)", me); return false; }
    p.hs = a.subsampling == 420 ? 2 : 1;
    p.bpm = p.hs == 2 ? 6 : 3;
    p.mcux = (a.W + 8 * p.hs - 1) / (8 * p.hs);
    p.mcuy = (a.H + 8 * p.hs - 1) / (8 * p.hs);
    p.nmcu = (int64_t)p.mcux * p.mcuy;
    p.n_int = (p.nmcu + a.restart_interval - 1) / a.restart_interval;
    p.n = p.n_int * a.B;
    if (p.n > (1ll << 30)) { set_error("%s: bad arguments (%lld restart intervals in the call; at most 2^30)", me, (long long)p.n); return false; }
    const size_t cnt = (size_t)p.n + 1;
    Carver c(workspace);
    p.coef = c.take<int16_t>((size_t)a.B * (size_t)p.nmcu * p.bpm * 64 + 64);
    carve_size_scan(c, p.scan, cnt);
    p.bytes = c.bytes();
    return true;
}

void put_segment(uint8_t *&w, int marker, const uint8_t *payload, int n)
{
    *w++ = 0xFF; *w++ = (uint8_t)marker; *w++ = (uint8_t)((n + 2) >> 8); *w++ = (uint8_t)(n + 2);
    for (int i = 0; i < n; i++) *w++ = payload[i];
}

// the same bytes for every frame of a call; -> their number
int build_header(const SoarJpegArgs &a, uint8_t *out)
{
    uint8_t *w = out, seg[192];
    *w++ = 0xFF; *w++ = 0xD8;
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};      // 1.01, no units, 1:1, no thumbnail
    put_segment(w, 0xE0, jfif, 14);
    for (int t = 0; t < 2; t++) {
        seg[0] = (uint8_t)t;
        for (int k = 0; k < 64; k++) seg[1 + k] = a.qtables[t][NATURAL_OF_ZIGZAG[k]];
        put_segment(w, 0xDB, seg, 65);
    }
    const uint8_t s = a.subsampling == 420 ? 0x22 : 0x11;
    const uint8_t sof[15] = {8, (uint8_t)(a.H >> 8), (uint8_t)a.H, (uint8_t)(a.W >> 8), (uint8_t)a.W, 3, 1, s, 0, 2, 0x11, 1, 3, 0x11, 1};
    put_segment(w, 0xC0, sof, 15);
    const HuffSpec *specs[4] = {&DC_LUM, &AC_LUM, &DC_CHR, &AC_CHR};
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; t++) {
        seg[0] = ids[t];
        for (int i = 0; i < 16; i++) seg[1 + i] = specs[t]->bits[i];
        for (int i = 0; i < specs[t]->n; i++) seg[17 + i] = specs[t]->vals[i];
        put_segment(w, 0xC4, seg, 17 + specs[t]->n);
    }
    const uint8_t dri[2] = {(uint8_t)(a.restart_interval >> 8), (uint8_t)a.restart_interval};
    put_segment(w, 0xDD, dri, 2);
    const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    put_segment(w, 0xDA, sos, 10);
    return (int)(w - out);
}

void entropy_args(const SoarJpegArgs &a, const Plan &p, EntropyDev &d)
{
    d.coef = p.coef; d.sizes = p.scan.sizes; d.offs = p.scan.offs; d.out = nullptr; d.capacity = 0;
    d.n_int = p.n_int; d.nmcu = p.nmcu; d.n = p.n; d.ri = a.restart_interval; d.bpm = p.bpm;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_jpeg_workspace_bytes(const SoarJpegArgs *args, size_t *bytes)
{
    return workspace_bytes_of("soar_jpeg_workspace_bytes", plan_of, args, bytes);
}

int soar_jpeg_measure(const SoarJpegArgs *args, void *workspace, size_t workspace_bytes, int64_t *offsets, void *stream_)
{
    const char *me = "soar_jpeg_measure";
    Plan p;
    if (!plan_of(me, args, workspace, p)) return 1;
    const SoarJpegArgs &a = *args;
    if (!offsets) { set_error("%s: NULL offsets", me); return 1; }
    if (!workspace_ok(me, workspace, workspace_bytes, p.bytes, "soar_jpeg_workspace_bytes")) return 1;
    if (!batch_ok(me, a.B, a.frames, a.frame_stride, (int64_t)a.H * a.W * a.channels, "frames", "a frame")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (a.B == 0) return no_item_offsets(offsets, stream);
    TransformDev t;
    t.frames = a.frames; t.stride = a.frame_stride; t.H = a.H; t.W = a.W; t.C = a.channels;
    t.wide = a.channels == 4 && ((uintptr_t)a.frames & 3) == 0 && (a.frame_stride & 3) == 0;
    t.mcux = p.mcux; t.nmcu = p.nmcu; t.coef = p.coef;
    for (int i = 0; i < 128; i++) t.q8[i / 64][i % 64] = (uint16_t)(8 * a.qtables[i / 64][i % 64]);
    const int per_tile = 8 / p.hs;
    const dim3 grid((unsigned)((p.mcux + per_tile - 1) / per_tile), (unsigned)p.mcuy, (unsigned)a.B);
    if (p.hs == 2)
        hipLaunchKernelGGL(transform_kernel<2>, grid, dim3(TRANSFORM_THREADS), 0, stream, t);
    else
        hipLaunchKernelGGL(transform_kernel<1>, grid, dim3(TRANSFORM_THREADS), 0, stream, t);
    SOAR_LAUNCH_OK("jpeg_transform", stream, 0);
    EntropyDev d;
    entropy_args(a, p, d);
    hipLaunchKernelGGL(entropy_kernel<false>, dim3((unsigned)p.n), dim3(WAVE), 0, stream, d);
    SOAR_LAUNCH_OK("jpeg_measure", stream, 0);
    return item_offsets("jpeg_frame_offsets", p.scan, a.B, p.n_int, offsets, stream);
}

int soar_jpeg_emit(const SoarJpegArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int64_t capacity, void *stream_)
{
    const char *me = "soar_jpeg_emit";
    Plan p;
    if (!plan_of(me, args, workspace, p)) return 1;
    const SoarJpegArgs &a = *args;
    if (!emit_out_ok(me, out, capacity)) return 1;
    if (!workspace_ok(me, workspace, workspace_bytes, p.bytes, "soar_jpeg_workspace_bytes")) return 1;
    if (a.B == 0) return 0;
    EntropyDev d;
    entropy_args(a, p, d);
    d.out = out; d.capacity = capacity;
    if (build_header(a, d.header) != HEADER_BYTES) { set_error("%s: the header is not %d bytes long", me, HEADER_BYTES); return 1; }
    hipLaunchKernelGGL(entropy_kernel<true>, dim3((unsigned)p.n), dim3(WAVE), 0, static_cast<hipStream_t>(stream_), d);
    SOAR_LAUNCH_OK("jpeg_emit", static_cast<hipStream_t>(stream_), 0);
    return 0;
}

}  // extern "C"
