// jpeg_decode.hip -- baseline JPEG files read on the device (soar_amd/jpeg.py): B files' bytes in one buffer in, B
// images of uint8 grey or RGB out, each with a status.  SOF0, 8 bit, Huffman; one component, or YCbCr at 4:4:4, 4:2:2 or 4:2:0; one
// interleaved scan; any tables, any restart interval.  Integer arithmetic only, and the one atomic is on a status whose outcome does
// not depend on the order of its writers (see merge_status).
//   parse_kernel     one wavefront per file.  Lane 0 walks the markers from SOI to the end of SOS into the file's record
//                    (jpeg_entropy.h: frame, sampling, quantiser tables, the Huffman codes' decoding tables).  Then all 64 lanes scan
//                    the entropy-coded segment for markers, 512 bytes a step, lane l bytes 8 l .. 8 l + 7 of them: the RSTn
//                    positions are compacted in order into the file's table by a prefix sum over the lanes, the first other marker
//                    ends the segment; the count must be ceil(MCUs / Ri) - 1 and the markers must count 0 .. 7 cyclically.
//   entropy_kernel   one LANE per restart interval, all intervals of all files: the DC predictors reset at a marker, so the
//                    intervals are independent.  Coefficients as int16 in natural order; blocks never reached stay zero.  A file
//                    without markers is one lane's serial work.
//   idct_kernel      one thread per 8 x 8 block: dequantisation and jidctint's two passes into the component's 8-bit sample plane.
//   colour_kernel    one thread per output pixel: libjpeg's triangle-filter chroma upsampling and its fixed-point YCbCr -> RGB in one
//                    pass; zeros for a failed file; the file's status and interval count.
// Bounds hold by construction: a file's bytes are read through jpeg_entropy.h against the file's range, which itself is clamped to
// the buffer; the marker table has a slot per 8 x 8 block of the image, more than a file of that size can have intervals, and a
// write to it is checked; a block index is checked against the record's count, which parse() derives from the call's own H and W.
#include "codec_common.h"
#include "jpeg_entropy.h"

namespace soar {
namespace {

using namespace jpgd;

static_assert(JPEG_BAD_STRUCTURE == SOAR_JPEG_BAD_STRUCTURE && JPEG_UNSUPPORTED == SOAR_JPEG_UNSUPPORTED &&
              JPEG_MISSING_TABLE == SOAR_JPEG_MISSING_TABLE && JPEG_CORRUPT == SOAR_JPEG_CORRUPT && JPEG_TRUNCATED == SOAR_JPEG_TRUNCATED,
              "jpeg_entropy.h and soar_hip.h name the same statuses");

constexpr int THREADS = 256;
constexpr int SCAN_BYTES = 8;                   // per lane and step of the marker scan

struct DecDev {
    int32_t B, H, W, C;
    const uint8_t *data;
    const int64_t *offsets;
    int64_t total;
    int64_t icap;               // slots of a file's marker table
    int64_t bcap;               // blocks of a file's slice of coef and samp
    Rec *rec;                   // [B]
    int64_t *lo;                // [B] the file's first byte in data
    int64_t *len;               // [B]
    int32_t *mark;              // [B][icap] the RSTn markers' positions in the file
    int16_t *coef;              // [B][bcap][64]
    uint8_t *samp;              // [B][bcap][64]
    uint8_t *out;               // [B][H][W][C]
    int32_t *status, *intervals;    // [B]
};

// ---- the marker walk and the restart scan ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(WAVE) parse_kernel(DecDev a)
{
    const int lane = threadIdx.x, b = blockIdx.x;
    // the offsets are the caller's: ascending inside [0, total], or no file of the call is looked at
    bool ok = true;
    for (int i = lane; i < a.B; i += WAVE) {
        const int64_t o0 = a.offsets[i], o1 = a.offsets[i + 1];
        if (o0 < 0 || o1 < o0 || o1 > a.total) ok = false;
    }
    ok = __ballot(!ok) == 0ull;
    const int64_t lo = ok ? a.offsets[b] : 0, L = ok ? a.offsets[b + 1] - lo : 0;
    const uint8_t *f = a.data + lo;
    Rec &r = a.rec[b];
    int32_t status = JPEG_OK;
    if (lane == 0) {
        status = parse(f, L, a.H, a.W, a.C, r);                  // (bad offsets: L = 0, and the file has no SOI)
        if (status == JPEG_OK && (r.mcus > a.icap || r.blocks > a.bcap)) status = JPEG_UNSUPPORTED;   // (cannot happen: H, W and C are the call's)
        r.status = status;
        a.lo[b] = lo;
        a.len[b] = L;
    }
    __threadfence_block();
    __syncthreads();
    status = __shfl(status, 0);
    if (status != JPEG_OK) return;
    const int64_t scan = r.scan;
    int32_t *mark = a.mark + (int64_t)b * a.icap;
    int64_t k = 0, seg_end = L;                                  // RSTn so far; uniform over the lanes
    bool sequence = true, has_end = false;
    for (int64_t base = scan; base < L && !has_end; base += WAVE * SCAN_BYTES) {
        const int64_t p0 = base + (int64_t)lane * SCAN_BYTES;
        uint32_t rst = 0u, code[SCAN_BYTES];
        int first_other = SCAN_BYTES;
#pragma unroll
        for (int j = 0; j < SCAN_BYTES; j++) {
            code[j] = 0u;
            if (marker_at(f, L, p0 + j)) {
                code[j] = f[p0 + j + 1];
                if (code[j] >= 0xD0u && code[j] <= 0xD7u) rst |= 1u << j;
                else if (first_other == SCAN_BYTES) first_other = j;
            }
        }
        const unsigned long long others = __ballot(first_other < SCAN_BYTES);
        int end_lane = WAVE, end_j = 0;
        if (others) {
            end_lane = (int)__builtin_ctzll(others);
            end_j = __shfl(first_other, end_lane);
            has_end = true;
            seg_end = base + (int64_t)end_lane * SCAN_BYTES + end_j;
        }
        // the RSTn in front of the segment's end
        if (lane > end_lane) rst = 0u;
        else if (lane == end_lane) rst &= (1u << end_j) - 1u;
        const int mine = __builtin_popcount(rst);
        int inc = mine;
        for (int s = 1; s < WAVE; s <<= 1) {
            const int o = __shfl_up(inc, s);
            if (lane >= s) inc += o;
        }
        int64_t at = k + inc - mine;
#pragma unroll
        for (int j = 0; j < SCAN_BYTES; j++)
            if (rst >> j & 1u) {
                if (code[j] != 0xD0u + (uint32_t)(at & 7)) sequence = false;
                if (at < a.icap) mark[at] = (int32_t)(p0 + j);
                at++;
            }
        k += __shfl(inc, WAVE - 1);
    }
    sequence = __ballot(!sequence) == 0ull;
    if (lane == 0) {
        r.has_end = has_end ? 1 : 0;
        r.seg_end = seg_end;
        status = intervals_of(r, k);
        if (status == JPEG_OK && !sequence) status = JPEG_CORRUPT;
        if (status == JPEG_OK && r.n_int > a.icap) status = JPEG_CORRUPT;          // (cannot happen: n_int <= mcus <= icap)
        if (status != JPEG_OK) r.n_int = 0;                      // nothing of the file is decoded
        r.status = status;
    }
}

// CORRUPT wins over TRUNCATED (which only a file's last interval gives), whichever interval reports first
__device__ __forceinline__ void merge_status(int32_t *status, int32_t st)
{
    if (st == JPEG_CORRUPT) atomicExch(status, JPEG_CORRUPT);
    else if (st != JPEG_OK) atomicCAS(status, JPEG_OK, st);
}

// ---- the entropy-coded segment, interval by interval ----------------------------------------------------------------------------------
// grid (ceil(icap / THREADS), B).  A file's status is read here only as the parse kernel left it (0: decode); what the intervals
// merge into it is read by the kernels behind.
__global__ void __launch_bounds__(THREADS) entropy_kernel(DecDev a)
{
    const int b = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    Rec &r = a.rec[b];
    const int32_t n_int = r.n_int;
    const int64_t L = a.len[b];
    // (status is not read: a file that failed before this kernel has n_int = 0 -- see parse(), which clears it first)
    if (j >= n_int || j >= a.icap) return;
    const int32_t *mark = a.mark + (int64_t)b * a.icap;
    int64_t start = j ? (int64_t)mark[j - 1] + 2 : r.scan, end = j < n_int - 1 ? (int64_t)mark[j] : r.seg_end;
    end = min(max(end, (int64_t)0), L);
    start = min(max(start, (int64_t)0), end);
    const int32_t per = r.ri ? r.ri : r.mcus;
    const int64_t mcu0 = j * per;
    if (mcu0 >= r.mcus) return;                                  // (cannot happen: j < ceil(mcus / per))
    const int32_t n = (int32_t)min((int64_t)per, r.mcus - mcu0);
    const int32_t st = decode_interval(a.data + a.lo[b], r, a.coef + (int64_t)b * a.bcap * 64, start, end, (int32_t)mcu0, n,
                                       j == n_int - 1 && !r.has_end);
    if (st != JPEG_OK) merge_status(&r.status, st);
}

// ---- dequantisation and the inverse DCT -----------------------------------------------------------------------------------------------
// jidctint.c's pass over eight values; the caller descales
__device__ __forceinline__ void idct8(const int64_t d[8], int64_t o[8])
{
    int64_t z2 = d[2], z3 = d[6];
    int64_t z1 = (z2 + z3) * 4433;
    const int64_t e2 = z1 + z3 * -15137, e3 = z1 + z2 * 6270;
    const int64_t e0 = (d[0] + d[4]) << 13, e1 = (d[0] - d[4]) << 13;
    const int64_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int64_t t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
    int64_t z4 = t1 + t3;
    const int64_t z5 = (z3 + z4) * 9633;
    t0 *= 2446; t1 *= 16819; t2 *= 25172; t3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    o[0] = t10 + t3; o[7] = t10 - t3; o[1] = t11 + t2; o[6] = t11 - t2;
    o[2] = t12 + t1; o[5] = t12 - t1; o[3] = t13 + t0; o[4] = t13 - t0;
}

// grid (ceil(bcap / THREADS), B)
__global__ void __launch_bounds__(THREADS) idct_kernel(DecDev a)
{
    const int b = blockIdx.y;
    const int64_t blk = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    const Rec &r = a.rec[b];
    if (r.status != JPEG_OK || blk >= r.blocks || blk >= a.bcap) return;
    const int c = r.nc == 3 ? (blk >= r.off[2] ? 2 : (blk >= r.off[1] ? 1 : 0)) : 0;
    const int32_t local = (int32_t)blk - r.off[c], by = local / r.bw[c], bx = local - by * r.bw[c];
    const int16_t *src = a.coef + ((int64_t)b * a.bcap + blk) * 64;
    const uint8_t *q = r.q[r.tq[c] & 3];
    int32_t ws[64];
#pragma unroll
    for (int x = 0; x < 8; x++) {                                // columns (unrolled: ws stays in registers)
        int64_t d[8], o[8];
#pragma unroll
        for (int y = 0; y < 8; y++) d[y] = (int64_t)src[y * 8 + x] * q[y * 8 + x];
        idct8(d, o);
#pragma unroll
        for (int y = 0; y < 8; y++) ws[y * 8 + x] = (int32_t)((o[y] + (1 << 10)) >> 11);
    }
    const int64_t stride = (int64_t)r.bw[c] * 8;
    uint8_t *dst = a.samp + ((int64_t)b * a.bcap + r.off[c]) * 64 + (int64_t)by * 8 * stride + (int64_t)bx * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {                                // rows
        int64_t d[8], o[8];
#pragma unroll
        for (int x = 0; x < 8; x++) d[x] = ws[y * 8 + x];
        idct8(d, o);
        uint32_t w0 = 0u, w1 = 0u;
#pragma unroll
        for (int x = 0; x < 8; x++) {
            const int64_t v = ((o[x] + (1 << 17)) >> 18) + 128;
            const uint32_t u = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
            if (x < 4) w0 |= u << (8 * x); else w1 |= u << (8 * (x - 4));
        }
        uint32_t *row = reinterpret_cast<uint32_t *>(dst + y * stride);      // (8-byte aligned: samp is, and every term is a multiple of 8)
        row[0] = w0;
        row[1] = w1;
    }
}

// ---- upsampling and colour ------------------------------------------------------------------------------------------------------------
// the chroma sample of output pixel (x, y): jdsample.c's h2v1 and h2v2 triangle filters with the true downsampled size [ch][cw] as
// the edge, or plain replication where cw <= 2 (libjpeg chooses so)
__device__ __forceinline__ int chroma_at(const uint8_t *p, int64_t stride, int cw, int ch, int hs, int vs, int x, int y)
{
    if (hs == 1) return p[y * stride + x];
    if (cw <= 2) return p[(int64_t)(y / vs) * stride + x / hs];
    const int i = x >> 1, xn = (x & 1) ? min(i + 1, cw - 1) : max(i - 1, 0);
    if (vs == 1) return (3 * p[y * stride + i] + p[y * stride + xn] + ((x & 1) ? 2 : 1)) >> 2;
    const int j = y >> 1, yn = (y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0);
    const int here = 3 * p[j * stride + i] + p[yn * stride + i], next = 3 * p[j * stride + xn] + p[yn * stride + xn];
    return (3 * here + next + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ __forceinline__ uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// grid (ceil(H W / THREADS), B)
__global__ void __launch_bounds__(THREADS) colour_kernel(DecDev a)
{
    const int b = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x, n = (int64_t)a.H * a.W;
    const Rec &r = a.rec[b];
    const int32_t st = r.status;
    if (i == 0) {
        a.status[b] = st;
        a.intervals[b] = r.n_int;
    }
    if (i >= n) return;
    uint8_t *dst = a.out + ((int64_t)b * n + i) * a.C;
    if (st != JPEG_OK) {
        for (int k = 0; k < a.C; k++) dst[k] = 0;
        return;
    }
    const int y = (int)(i / a.W), x = (int)(i - (int64_t)y * a.W);
    const uint8_t *s = a.samp + (int64_t)b * a.bcap * 64;
    const int Y = s[(int64_t)y * r.bw[0] * 8 + x];
    if (a.C == 1) { dst[0] = (uint8_t)Y; return; }
    const int hs = r.hs[0], vs = r.vs[0], cw = (a.W + hs - 1) / hs, ch = (a.H + vs - 1) / vs;
    const int64_t stride = (int64_t)r.bw[1] * 8;
    const int cb = chroma_at(s + (int64_t)r.off[1] * 64, stride, cw, ch, hs, vs, x, y) - 128;
    const int cr = chroma_at(s + (int64_t)r.off[2] * 64, stride, cw, ch, hs, vs, x, y) - 128;
    dst[0] = clamp8(Y + ((91881 * cr + 32768) >> 16));
    dst[1] = clamp8(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    dst[2] = clamp8(Y + ((116130 * cb + 32768) >> 16));
}

// ---- the host side ------------------------------------------------------------------------------------------------------------------
struct Plan {
    DecDev d;
    size_t bytes, coef_bytes;
};

bool plan_of(const char *me, const SoarJpegDecodeArgs *args, void *workspace, Plan &p)
{
    if (!args) { set_error("%s: NULL args", me); return false; }
    const SoarJpegDecodeArgs &a = *args;
    if (a.B < 0 || a.B > 65535 || a.H < 1 || a.W < 1 || a.H > 65535 || a.W > 65535 || (a.channels != 1 && a.channels != 3) || a.total_bytes < 0) {
        set_error("%s: bad arguments (B=%d, H=%d, W=%d, channels=%d, total_bytes=%lld; need 0 <= B <= 65535, 1 <= H, W <= 65535, "
                  "channels 1 or 3, total_bytes >= 0)", me, a.B, a.H, a.W, a.channels, (long long)a.total_bytes);
        return false;
    }
    DecDev &d = p.d;
    d.B = a.B; d.H = a.H; d.W = a.W; d.C = a.channels; d.data = a.data; d.offsets = a.offsets; d.total = a.total_bytes;
    const int64_t h8 = (a.H + 7) / 8, w8 = (a.W + 7) / 8, h16 = (a.H + 15) / 16, w16 = (a.W + 15) / 16;
    d.icap = h8 * w8;                                            // the MCUs at 4:4:4: no sampling has more
    d.bcap = a.channels == 1 ? h8 * w8 : std::max(3 * h8 * w8, std::max(4 * h8 * w16, 6 * h16 * w16));
    Carver c(workspace);
    d.rec = c.take<Rec>((size_t)a.B);
    d.lo = c.take<int64_t>((size_t)a.B);
    d.len = c.take<int64_t>((size_t)a.B);
    d.mark = c.take<int32_t>((size_t)a.B * (size_t)d.icap);
    p.coef_bytes = (size_t)a.B * (size_t)d.bcap * 64 * sizeof(int16_t);
    d.coef = c.take<int16_t>((size_t)a.B * (size_t)d.bcap * 64);
    d.samp = c.take<uint8_t>((size_t)a.B * (size_t)d.bcap * 64);
    p.bytes = c.bytes();
    d.out = nullptr; d.status = nullptr; d.intervals = nullptr;
    return true;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_jpeg_decode_workspace_bytes(const SoarJpegDecodeArgs *args, size_t *bytes)
{
    return workspace_bytes_of("soar_jpeg_decode_workspace_bytes", plan_of, args, bytes);
}

int soar_jpeg_decode(const SoarJpegDecodeArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int32_t *status, int32_t *intervals,
                     void *stream_)
{
    const char *me = "soar_jpeg_decode";
    Plan p;
    if (!plan_of(me, args, workspace, p)) return 1;
    const SoarJpegDecodeArgs &a = *args;
    if (a.B == 0) return 0;
    if (!decode_ok(me, a, out, status, intervals, "intervals", workspace, workspace_bytes, p.bytes, "soar_jpeg_decode_workspace_bytes")) return 1;
    p.d.out = out; p.d.status = status; p.d.intervals = intervals;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const unsigned B = (unsigned)a.B;
    const int64_t pixels = (int64_t)a.H * a.W;
    SOAR_HIP_OK(hipMemsetAsync(p.d.coef, 0, p.coef_bytes, stream));
    hipLaunchKernelGGL(parse_kernel, dim3(B), dim3(WAVE), 0, stream, p.d);
    SOAR_LAUNCH_OK("jpeg_decode_parse", stream, 0);
    hipLaunchKernelGGL(entropy_kernel, dim3((unsigned)((p.d.icap + THREADS - 1) / THREADS), B), dim3(THREADS), 0, stream, p.d);
    SOAR_LAUNCH_OK("jpeg_decode_entropy", stream, 0);
    hipLaunchKernelGGL(idct_kernel, dim3((unsigned)((p.d.bcap + THREADS - 1) / THREADS), B), dim3(THREADS), 0, stream, p.d);
    SOAR_LAUNCH_OK("jpeg_decode_idct", stream, 0);
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)((pixels + THREADS - 1) / THREADS), B), dim3(THREADS), 0, stream, p.d);
    SOAR_LAUNCH_OK("jpeg_decode_colour", stream, 0);
    return 0;
}

}  // extern "C"
