// png_decode.hip -- PNG files read on the device (soar_amd/png.py): B files' bytes in one buffer in, B images of uint8
// grey, RGB or RGBA out, each with a status.  8 bit, colour types 0, 2 and 6, no interlace; all of RFC 1951.  Integer arithmetic and
// integer atomics only (sums, and a compare-and-swap of a status that every writer would set to the same value).
//   scan_kernel      one wavefront per file: signature, chunk walk, IHDR, the CRC-32 of IHDR and of every IDAT (64 stretches in
//                    parallel, png_common.h), the IDAT payloads compacted into the file's slot of the workspace as one zlib stream Z,
//                    the zlib header, and the table of segment candidates.
//   probe_kernel     one wavefront per candidate segment of a file that has more than one: the segment decoded from its byte start
//                    without a store; its output length, or -1.
//   plan_kernel      one wavefront per file: if every segment succeeded and the lengths sum to H (1 + W C), their exclusive scan;
//                    otherwise the file becomes one segment from byte 2.
//   inflate_kernel   one wavefront per segment: png_inflate.h's decoder run by all 64 lanes on the same bits (a load of one address
//                    is one transaction), and a sink that spreads the stores over the lanes -- up to 64 literals are kept one per lane
//                    and stored together, a match or a stored stretch is copied 64 bytes a step.  Matches read a 32 KiB ring in LDS, not
//                    the output: LDS is in order for a wavefront, so no fence stands between a store and the match that reads it.
//                    With the tables that is 36 KiB, four wavefronts per CU and 1024 on the chip, more than a call has segments; the
//                    alternative, matches read back from global memory, pays a fence and a memory round trip per match.
//   adler_kernel     256 threads per 64 KiB of a file's filtered stream: sum d[i] and sum (S - i) d[i], added to the file's two sums.
//   unfilter_kernel  one wavefront per file, 64 rows a band: lane r has row y0 + r and runs one pixel behind lane r - 1, so the pixel
//                    above and the one above left come from the neighbour's registers whatever the rows' filter types; a band takes
//                    W + 63 steps and hands its last row to the next through the output.  Also the file's last word: Adler-32, a
//                    filter byte above 4, the status, and zeros for a failed file.
// Bounds hold by construction: a file's bytes are read through rd() against the file's range, which itself is clamped to the buffer;
// Z is written inside the file's slot (as long as the file) and read through png_inflate.h's checked reader; every sink checks a store
// against the segment's stretch of the filtered stream, and every stretch against the stream.
#include "codec_common.h"
#include "png_common.h"
#include "png_inflate.h"

namespace soar {
namespace {

using namespace pngi;

static_assert(PNG_BAD_STRUCTURE == SOAR_PNG_BAD_STRUCTURE && PNG_UNSUPPORTED == SOAR_PNG_UNSUPPORTED && PNG_BAD_CRC == SOAR_PNG_BAD_CRC &&
              PNG_CORRUPT == SOAR_PNG_CORRUPT && PNG_WRONG_LENGTH == SOAR_PNG_WRONG_LENGTH && PNG_BAD_ADLER == SOAR_PNG_BAD_ADLER &&
              PNG_BAD_FILTER == SOAR_PNG_BAD_FILTER, "png_inflate.h and soar_hip.h name the same statuses");

constexpr int RING = 32768;
constexpr int ADLER_THREADS = 256;
constexpr int ADLER_CHUNK = 65536;
constexpr int MAX_BLOCKS = 4096;                // of the two kernels that stride over the segment table

struct FileRec {
    int64_t lo, len;            // the file's bytes in data, clamped to the buffer
    int64_t first;              // its first entry of the segment table
    int32_t status, nseg, zlen, segments;
    uint32_t adler_want, pad;
    unsigned long long sum_a, sum_b;
};

struct DecDev {
    int32_t B, H, W, C;
    const uint8_t *data;
    const int64_t *offsets;
    int64_t total, S, E;        // bytes of data; filtered bytes of an image; entries of the segment table
    uint8_t *z;                 // [total] the zlib streams, file b's in its own byte range
    uint8_t *filt;              // [B][S]
    FileRec *rec;               // [B]
    int32_t *seg_start;         // [E] the segment's first byte in Z; -1: no segment
    int32_t *seg_file;          // [E]
    int32_t *seg_len;           // [E] bytes it gives (probe; the plan makes it the stretch's length in every case)
    int32_t *seg_out;           // [E] where they go in the filtered stream
    uint8_t *out;               // [B][H][W][C]
    int32_t *status, *segments; // [B]
};

// file b's entries of the segment table: a candidate costs 12 bytes of chunk framing at the least, so len / 12 + 1 entries suffice and
// the files' stretches do not meet
__device__ __forceinline__ int64_t entry_first(int64_t lo, int b) { return lo / 12 + b; }
__device__ __forceinline__ int64_t entry_cap(int64_t len) { return len / 12 + 1; }

__device__ __forceinline__ uint32_t rd(const uint8_t *f, int64_t len, int64_t p) { return p >= 0 && p < len ? f[p] : 0u; }
__device__ __forceinline__ uint32_t rd32(const uint8_t *f, int64_t len, int64_t p)
{
    return rd(f, len, p) << 24 | rd(f, len, p + 1) << 16 | rd(f, len, p + 2) << 8 | rd(f, len, p + 3);
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x)
{
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// ---- the chunk walk -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) scan_kernel(DecDev a)
{
    __shared__ uint32_t crctab[256];
    const int lane = threadIdx.x, b = blockIdx.x;
    crc_table(crctab, lane);
    // the offsets are the caller's: ascending inside [0, total], or no file of the call is looked at
    bool ok = true;
    for (int i = lane; i < a.B; i += WAVE) {
        const int64_t o0 = a.offsets[i], o1 = a.offsets[i + 1];
        if (o0 < 0 || o1 < o0 || o1 > a.total) ok = false;
    }
    ok = __ballot(!ok) == 0ull;
    const int64_t lo = ok ? a.offsets[b] : 0, L = ok ? a.offsets[b + 1] - lo : 0;
    const uint8_t *f = a.data + lo;
    uint8_t *z = a.z + lo;
    const int64_t first_entry = entry_first(lo, b), cap = entry_cap(L);
    for (int64_t e = lane; e < cap; e += WAVE) a.seg_start[first_entry + e] = -1;
    __threadfence_block();
    __syncthreads();

    int32_t status = PNG_OK;
    int64_t zpos = 0, pos = 8, last_start = 2;
    int32_t nseg = 1;
    uint32_t tail = 0, head = 0;                                 // Z's last four bytes, and its first two
    bool first = true, idat = false, prev_stored = false, table_full = false;
    const uint32_t sig0 = 0x89504E47u, sig1 = 0x0D0A1A0Au;
    if (!ok || L < 8 || rd32(f, L, 0) != sig0 || rd32(f, L, 4) != sig1) status = PNG_BAD_STRUCTURE;
    if (status == PNG_OK && L > 0x7FFFFFFF) status = PNG_UNSUPPORTED;
    while (status == PNG_OK) {
        if (pos + 12 > L) { status = PNG_BAD_STRUCTURE; break; }
        const int64_t len = rd32(f, L, pos);
        const uint32_t type = rd32(f, L, pos + 4);
        if (len > 0x7FFFFFFF || pos + 12 + len > L) { status = PNG_BAD_STRUCTURE; break; }
        const bool is_ihdr = type == 0x49484452u, is_idat = type == 0x49444154u;
        bool crc_ok = true;
        if (is_ihdr || is_idat) crc_ok = crc_written(crctab, f, pos + 4, pos + 8 + len, lane) == rd32(f, L, pos + 8 + len);
        if (first) {
            if (!is_ihdr || len != 13) { status = PNG_BAD_STRUCTURE; break; }
            if (!crc_ok) { status = PNG_BAD_CRC; break; }
            const uint32_t w = rd32(f, L, pos + 8), h = rd32(f, L, pos + 12), colour = rd(f, L, pos + 17);
            if (w == 0 || h == 0 || w > 0x7FFFFFFFu || h > 0x7FFFFFFFu) { status = PNG_BAD_STRUCTURE; break; }
            if (rd(f, L, pos + 16) != 8 || (colour != 0 && colour != 2 && colour != 6) || rd(f, L, pos + 18) || rd(f, L, pos + 19) ||
                rd(f, L, pos + 20)) { status = PNG_UNSUPPORTED; break; }
            if ((int64_t)h != a.H || (int64_t)w != a.W || (colour == 0 ? 1 : (colour == 2 ? 3 : 4)) != a.C) { status = PNG_UNSUPPORTED; break; }
            first = false;
        } else if (is_ihdr) {
            status = PNG_BAD_STRUCTURE;
            break;
        } else if (is_idat) {
            if (!crc_ok) { status = PNG_BAD_CRC; break; }
            const int64_t p = zpos;
            // a candidate: behind 00 00 FF FF, or behind an IDAT that is exactly one stored block
            if (idat && p >= 6 && p > last_start && (tail == 0x0000FFFFu || prev_stored)) {
                if (nseg < cap) {
                    if (lane == 0) { a.seg_start[first_entry + nseg] = (int32_t)p; a.seg_file[first_entry + nseg] = b; }
                    nseg++;
                    last_start = p;
                } else {
                    table_full = true;                           // (cannot happen: see entry_cap; the file is decoded as one segment)
                }
            }
            if (zpos + len > L) { status = PNG_BAD_STRUCTURE; break; }       // (cannot happen: the payloads are parts of the file)
            const int64_t src = pos + 8;
            for (int64_t i = lane; i < len; i += WAVE) z[zpos + i] = (uint8_t)rd(f, L, src + i);
            for (int64_t i = len > 4 ? len - 4 : 0; i < len; i++) tail = tail << 8 | rd(f, L, src + i);
            for (int64_t i = 0; i < len && zpos + i < 2; i++) head = head << 8 | rd(f, L, src + i);
            const int64_t s0 = p == 0 ? 2 : 0, n0 = len - s0;       // the payload behind the zlib header
            const uint32_t l0 = rd(f, L, src + s0 + 1), l1 = rd(f, L, src + s0 + 2);
            prev_stored = n0 >= 5 && rd(f, L, src + s0) == 0 && (l0 ^ rd(f, L, src + s0 + 3)) == 0xFFu &&
                          (l1 ^ rd(f, L, src + s0 + 4)) == 0xFFu && n0 == 5 + (int64_t)(l0 | l1 << 8);
            zpos += len;
            idat = true;
        } else if (type == 0x49454E44u) {                        // IEND
            break;
        } else if (!(type & 0x20000000u) && type != 0x504C5445u) {
            status = PNG_UNSUPPORTED;                            // a critical chunk other than PLTE
            break;
        }
        pos += 12 + len;
    }
    if (status == PNG_OK && !idat) status = PNG_BAD_STRUCTURE;
    if (status == PNG_OK && zpos < 2) status = PNG_CORRUPT;
    if (status == PNG_OK) status = zlib_header(head >> 8, head & 255u);
    if (table_full) nseg = 1;
    if (nseg > 1 && last_start >= zpos) nseg--;                  // a candidate needs a byte of its own
    __threadfence_block();
    __syncthreads();
    // the entries that are no segments after all; entry 0 is the stream from byte 2
    const int32_t live = status == PNG_OK ? nseg : 0;
    for (int64_t e = lane; e < cap; e += WAVE) {
        if (e >= live) a.seg_start[first_entry + e] = -1;
        else if (e == 0) { a.seg_start[first_entry] = 2; a.seg_file[first_entry] = b; }
    }
    if (lane == 0) {
        FileRec r;
        r.lo = lo; r.len = L; r.first = first_entry;
        r.status = status; r.nseg = live; r.zlen = (int32_t)zpos; r.segments = 1;
        r.adler_want = tail; r.pad = 0u; r.sum_a = 0ull; r.sum_b = 0ull;
        a.rec[b] = r;
    }
}

// the segment of entry e, checked against its file: false if e is none
struct Segment {
    int b;
    int64_t start, end;         // Z[start, end) is the reader's range (for the last segment: to Z's end)
    bool last;
    const uint8_t *z;
};

__device__ __forceinline__ bool segment_of(const DecDev &a, int64_t e, Segment &s, FileRec &r)
{
    const int32_t st = a.seg_start[e];
    if (st < 0) return false;
    s.b = a.seg_file[e];
    if (s.b < 0 || s.b >= a.B) return false;
    r = a.rec[s.b];
    const int64_t k = e - r.first;
    if (r.status != PNG_OK || k < 0 || k >= r.nseg || r.lo < 0 || r.len < 0 || r.lo + r.len > a.total || r.zlen > r.len) return false;
    s.last = k == r.nseg - 1;
    s.start = st;
    s.end = s.last ? r.zlen : a.seg_start[e + 1];
    s.z = a.z + r.lo;
    return s.start >= 2 && s.start <= s.end && s.end <= r.zlen;
}

// ---- the first pass -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) probe_kernel(DecDev a)
{
    __shared__ Tables t;
    for (int64_t e = blockIdx.x; e < a.E; e += gridDim.x) {
        Segment s;
        FileRec r;
        if (!segment_of(a, e, s, r) || r.nseg < 2) continue;
        Bits br(s.z, s.end, s.start);
        CountSink sink(a.S);
        const int32_t st = inflate(br, t, sink, s.last);
        if (threadIdx.x == 0) a.seg_len[e] = st == PNG_OK ? (int32_t)sink.pos : -1;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(WAVE) plan_kernel(DecDev a)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    FileRec r = a.rec[b];
    if (r.status != PNG_OK || r.nseg < 1) return;
    const int64_t e0 = r.first;
    const int32_t n = r.nseg, per = (n + WAVE - 1) / WAVE;
    const int32_t k0 = min(n, lane * per), k1 = min(n, k0 + per);
    bool parallel = n > 1;
    long long mine = 0;
    int32_t gave = 0;
    if (parallel) {
        for (int32_t k = k0; k < k1; k++) {
            const int32_t l = a.seg_len[e0 + k];
            if (l < 0) parallel = false; else { mine += l; gave += l > 0; }
        }
        parallel = __ballot(!parallel) == 0ull;
    }
    long long inc = mine;                                       // the inclusive scan over the lanes
    for (int s = 1; s < WAVE; s <<= 1) {
        const long long o = __shfl_up(inc, s);
        if (lane >= s) inc += o;
    }
    const long long total = __shfl(inc, WAVE - 1);
    if (parallel && total == a.S) {
        long long at = inc - mine;
        for (int32_t k = k0; k < k1; k++) {
            a.seg_out[e0 + k] = (int32_t)at;
            at += a.seg_len[e0 + k];
        }
        gave = wave_sum_i(gave);
        if (lane == 0) a.rec[b].segments = gave;
    } else {
        // one segment from byte 2, with the whole stream as its stretch
        for (int32_t k = 1 + lane; k < n; k += WAVE) a.seg_start[e0 + k] = -1;
        if (lane == 0) {
            a.seg_out[e0] = 0;
            a.seg_len[e0] = (int32_t)a.S;
            a.rec[b].nseg = 1;
            a.rec[b].segments = 1;
        }
    }
}

// ---- the second pass ------------------------------------------------------------------------------------------------------------------
// the device's sink: the segment's stretch out[0, cap) of the filtered stream and the last 32 KiB of it in LDS
struct WaveSink {
    uint8_t *out, *ring;
    int64_t cap, pos;
    int lane, npend;
    uint32_t pend;
    __device__ __forceinline__ WaveSink(uint8_t *out_, int64_t cap_, uint8_t *ring_, int lane_)
        : out(out_), ring(ring_), cap(cap_), pos(0), lane(lane_), npend(0), pend(0u) {}
    __device__ __forceinline__ void flush()
    {
        if (lane < npend) {                                      // (pos + npend <= cap: lit() saw to it)
            ring[(pos + lane) & (RING - 1)] = (uint8_t)pend;
            out[pos + lane] = (uint8_t)pend;
        }
        pos += npend;
        npend = 0;
    }
    __device__ __forceinline__ bool lit(uint8_t v)
    {
        if (pos + npend >= cap) return false;
        if (lane == npend) pend = v;
        if (++npend == WAVE) flush();
        return true;
    }
    __device__ __forceinline__ int32_t match(uint32_t dist, uint32_t len)
    {
        flush();
        if ((int64_t)dist > pos || dist > (uint32_t)RING) return PNG_CORRUPT;
        if (pos + (int64_t)len > cap) return PNG_WRONG_LENGTH;
        __syncthreads();                                         // the ring's earlier stores, before these loads
        // every source byte lies before pos, so no step reads what this match writes: an overlapping copy repeats its dist bytes
        for (uint32_t i = lane; i < len; i += WAVE) {
            const uint32_t back = dist >= len ? i : i % dist;
            const uint8_t v = ring[(pos - dist + back) & (RING - 1)];
            ring[(pos + i) & (RING - 1)] = v;
            out[pos + i] = v;
        }
        pos += len;
        return PNG_OK;
    }
    __device__ __forceinline__ int32_t stored(const uint8_t *z, int64_t from, uint32_t len)
    {
        flush();
        if (pos + (int64_t)len > cap) return PNG_WRONG_LENGTH;
        for (uint32_t i = lane; i < len; i += WAVE) {
            const uint8_t v = z[from + i];                       // (inside the reader's range: inflate() checked from + len)
            ring[(pos + i) & (RING - 1)] = v;
            out[pos + i] = v;
        }
        pos += len;
        return PNG_OK;
    }
    __device__ __forceinline__ void finish() { flush(); }
};

__global__ void __launch_bounds__(WAVE) inflate_kernel(DecDev a)
{
    __shared__ Tables t;
    __shared__ uint8_t ring[RING];
    const int lane = threadIdx.x;
    for (int64_t e = blockIdx.x; e < a.E; e += gridDim.x) {
        Segment s;
        FileRec r;
        if (!segment_of(a, e, s, r)) continue;
        const int64_t at = a.seg_out[e], cap = a.seg_len[e];
        int32_t st;
        if (at < 0 || cap < 0 || at + cap > a.S) {
            st = PNG_WRONG_LENGTH;                               // (cannot happen: the plan's scan)
        } else {
            Bits br(s.z, s.end, s.start);
            WaveSink sink(a.filt + (int64_t)s.b * a.S + at, cap, ring, lane);
            st = inflate(br, t, sink, s.last);
            if (st == PNG_OK && sink.pos != cap) st = PNG_WRONG_LENGTH;
        }
        if (st != PNG_OK && lane == 0) atomicCAS(&a.rec[s.b].status, PNG_OK, st);
        __syncthreads();
    }
}

// ---- Adler-32 ---------------------------------------------------------------------------------------------------------------------------
// grid (chunks, files).  1 + sum d[i] and S + sum (S - i) d[i], modulo 65521, are the checksum's two halves.
__global__ void __launch_bounds__(ADLER_THREADS) adler_kernel(DecDev a)
{
    __shared__ unsigned long long part[2][ADLER_THREADS / WAVE];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (a.rec[b].status != PNG_OK) return;
    const uint8_t *d = a.filt + (int64_t)b * a.S;
    const int64_t i0 = (int64_t)blockIdx.x * ADLER_CHUNK, i1 = min(a.S, i0 + ADLER_CHUNK);
    unsigned long long sa = 0ull, sb = 0ull;                     // (256 terms below 2^8 and 2^24)
    for (int64_t i = i0 + tid; i < i1; i += ADLER_THREADS) {
        const uint32_t v = d[i];
        sa += v;
        sb += (unsigned long long)((uint32_t)((a.S - i) % ADLER_MOD)) * v;
    }
    sa = wave_sum_u64(sa);
    sb = wave_sum_u64(sb);
    if ((tid & (WAVE - 1)) == 0) { part[0][tid / WAVE] = sa; part[1][tid / WAVE] = sb; }
    __syncthreads();
    if (tid == 0) {
        sa = sb = 0ull;
        for (int k = 0; k < ADLER_THREADS / WAVE; k++) { sa += part[0][k]; sb += part[1][k]; }
        atomicAdd(&a.rec[b].sum_a, sa % ADLER_MOD);
        atomicAdd(&a.rec[b].sum_b, sb % ADLER_MOD);
    }
}

// ---- the row filters ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth_of(int a, int b, int c)
{
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
}

template <int C> __device__ __forceinline__ uint32_t load_pixel(const uint8_t *p)
{
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < C; k++) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

template <int C> __device__ __forceinline__ void zero_image(uint8_t *img, int64_t n, int lane)
{
    __threadfence_block();
    __syncthreads();
    for (int64_t i = lane; i < n; i += WAVE) img[i] = 0;
}

// a pixel is C bytes in one register, the first in the lowest byte
template <int C> __device__ void unfilter_file(const DecDev &a, int b, int lane)
{
    FileRec r = a.rec[b];
    int32_t st = r.status;
    if (st == PNG_OK) {
        const uint32_t A = (uint32_t)((1ull + r.sum_a) % ADLER_MOD), Bv = (uint32_t)(((unsigned long long)(a.S % ADLER_MOD) + r.sum_b) % ADLER_MOD);
        if ((Bv << 16 | A) != r.adler_want) st = PNG_BAD_ADLER;
    }
    const int64_t row = (int64_t)a.W * C, stride = row + 1, n = (int64_t)a.H * row;
    uint8_t *img = a.out + (int64_t)b * n;
    const uint8_t *src = a.filt + (int64_t)b * a.S;
    for (int y0 = 0; st == PNG_OK && y0 < a.H; y0 += WAVE) {
        const int y = y0 + lane;
        const bool have = y < a.H;
        const int ft = have ? (int)src[(int64_t)y * stride] : 0;
        if (__ballot(ft > 4) != 0ull) { st = PNG_BAD_FILTER; break; }
        if (y0 > 0) {                                            // lane 63's row of the band before, through the output
            __threadfence_block();
            __syncthreads();
        }
        const uint8_t *in = src + (int64_t)(have ? y : 0) * stride + 1;
        uint8_t *dst = img + (int64_t)(have ? y : 0) * row;
        const uint8_t *above = img + (int64_t)(y0 > 0 ? y0 - 1 : 0) * row;  // read by lane 0, for y0 > 0
        uint32_t res = 0u, c = 0u;
        uint32_t nxt = have && lane == 0 ? load_pixel<C>(in) : 0u;          // the pixel of the step to come
        uint32_t up_nxt = lane == 0 && y0 > 0 ? load_pixel<C>(above) : 0u;
        for (int t = 0; t < a.W + WAVE - 1; t++) {
            const int x = t - lane;
            const bool on = have && x >= 0 && x < a.W;
            uint32_t bup = (uint32_t)__shfl_up((int)res, 1);     // the neighbour's pixel of the step before: x of the row above
            if (lane == 0) bup = up_nxt;
            const uint32_t left = res, cur = nxt;
            const int xn = x + 1;                                // fetch for the step to come
            nxt = have && xn >= 0 && xn < a.W ? load_pixel<C>(in + (int64_t)xn * C) : 0u;
            if (lane == 0) up_nxt = y0 > 0 && xn < a.W ? load_pixel<C>(above + (int64_t)xn * C) : 0u;
            uint32_t v = 0u;
            if (on) {
#pragma unroll
                for (int k = 0; k < C; k++) {
                    const int f = (cur >> (8 * k)) & 255, la = (left >> (8 * k)) & 255, ub = (bup >> (8 * k)) & 255, uc = (c >> (8 * k)) & 255;
                    const int pred = ft == 0 ? 0 : ft == 1 ? la : ft == 2 ? ub : ft == 3 ? (la + ub) >> 1 : paeth_of(la, ub, uc);
                    const uint32_t o = (uint32_t)(f + pred) & 255u;
                    dst[(int64_t)x * C + k] = (uint8_t)o;
                    v |= o << (8 * k);
                }
            }
            res = v;
            c = on ? bup : 0u;
        }
    }
    if (st != PNG_OK) zero_image<C>(img, n, lane);
    if (lane == 0) {
        a.status[b] = st;
        a.segments[b] = r.segments;
    }
}

__global__ void __launch_bounds__(WAVE) unfilter_kernel(DecDev a)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    if (a.C == 1) unfilter_file<1>(a, b, lane);
    else if (a.C == 3) unfilter_file<3>(a, b, lane);
    else unfilter_file<4>(a, b, lane);
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
struct Plan {
    DecDev d;
    size_t bytes;
};

bool plan_of(const char *me, const SoarPngDecodeArgs *args, void *workspace, Plan &p)
{
    if (!args) { set_error("%s: NULL args", me); return false; }
    const SoarPngDecodeArgs &a = *args;
    const int64_t S = (int64_t)a.H * (1 + (int64_t)a.W * a.channels);
    if (a.B < 0 || a.B > 65535 || a.H < 1 || a.W < 1 || (a.channels != 1 && a.channels != 3 && a.channels != 4) || a.total_bytes < 0 ||
        S > 0x7FFFFFFF) {
        set_error("%s: bad arguments (B=%d, H=%d, W=%d, channels=%d, total_bytes=%lld; need 0 <= B <= 65535, H, W >= 1 with "
                  "H (1 + W channels) < 2^31, channels 1, 3 or 4, total_bytes >= 0)", me, a.B, a.H, a.W, a.channels, (long long)a.total_bytes);
        return false;
    }
    DecDev &d = p.d;
    d.B = a.B; d.H = a.H; d.W = a.W; d.C = a.channels; d.data = a.data; d.offsets = a.offsets; d.total = a.total_bytes; d.S = S;
    d.E = a.total_bytes / 12 + a.B + 1;
    Carver c(workspace);
    d.z = c.take<uint8_t>((size_t)a.total_bytes);
    d.filt = c.take<uint8_t>((size_t)a.B * (size_t)S);
    d.rec = c.take<FileRec>((size_t)a.B);
    d.seg_start = c.take<int32_t>((size_t)d.E);
    d.seg_file = c.take<int32_t>((size_t)d.E);
    d.seg_len = c.take<int32_t>((size_t)d.E);
    d.seg_out = c.take<int32_t>((size_t)d.E);
    p.bytes = c.bytes();
    d.out = nullptr; d.status = nullptr; d.segments = nullptr;
    return true;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_png_decode_workspace_bytes(const SoarPngDecodeArgs *args, size_t *bytes)
{
    return workspace_bytes_of("soar_png_decode_workspace_bytes", plan_of, args, bytes);
}

int soar_png_decode(const SoarPngDecodeArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int32_t *status, int32_t *segments,
                    void *stream_)
{
    const char *me = "soar_png_decode";
    Plan p;
    if (!plan_of(me, args, workspace, p)) return 1;
    const SoarPngDecodeArgs &a = *args;
    if (a.B == 0) return 0;
    if (!decode_ok(me, a, out, status, segments, "segments", workspace, workspace_bytes, p.bytes, "soar_png_decode_workspace_bytes")) return 1;
    p.d.out = out; p.d.status = status; p.d.segments = segments;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned strided = (unsigned)std::min<int64_t>(p.d.E, MAX_BLOCKS);
    hipLaunchKernelGGL(scan_kernel, dim3((unsigned)a.B), dim3(WAVE), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_decode_scan", stream, 0);
    hipLaunchKernelGGL(probe_kernel, dim3(strided), dim3(WAVE), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_decode_probe", stream, 0);
    hipLaunchKernelGGL(plan_kernel, dim3((unsigned)a.B), dim3(WAVE), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_decode_plan", stream, 0);
    hipLaunchKernelGGL(inflate_kernel, dim3(strided), dim3(WAVE), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_decode_inflate", stream, 0);
    hipLaunchKernelGGL(adler_kernel, dim3((unsigned)((p.d.S + ADLER_CHUNK - 1) / ADLER_CHUNK), (unsigned)a.B), dim3(ADLER_THREADS), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_decode_adler", stream, 0);
    hipLaunchKernelGGL(unfilter_kernel, dim3((unsigned)a.B), dim3(WAVE), 0, stream, p.d);
    SOAR_LAUNCH_OK("png_decode_unfilter", stream, 0);
    return 0;
}

}  // extern "C"
