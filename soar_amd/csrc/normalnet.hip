// normalnet.hip -- the normal-map networks of the preprocessing stage (soar_amd/normals.py): two pix2pixHD global generators,
// netF on [image, prior_F] and netB on [image, prior_B], inference only, as include/soar_hip.h and DESIGN.md 9l state them.
//
//   (conv_pack_kernel      conv_gemm.hip: torch [Cout][Cin][k][k] -> [Cout][tap][Cin])
//   nn_pack_up_kernel      the transposed convolution's torch [Cin][Cout][3][3] -> its four output-parity phases, each
//                          [Cout][tap of the phase][Cin] (1 + 2 + 2 + 4 taps)
//   nn_first_kernel        reflection pad 3 + conv 7x7, 6 -> ngf, on the VALU: reads the caller's strided NCHW planes, writes NHWC
//   (conv_gemm_kernel      conv_gemm.hip: every other convolution but the last, as the shared implicit GEMM with M = pixels of the
//                          whole batch.  Its A loader does the padding as index arithmetic: zero (stride-2 convolutions, the phases
//                          of the transposed one) or mirrored (the residual trunk))
//   nn_in_partial_kernel   InstanceNorm statistics: per (image, chunk of pixels, channel) sum and sum of squares in double
//   nn_in_final_kernel     ... the chunks added in order -> mean, 1 / sqrt(biased variance + 1e-5)
//   nn_in_apply_kernel     y = relu((x - mean) rstd), or y = res + (x - mean) rstd at the end of a residual block
//   nn_last_kernel         reflection pad 3 + conv 7x7, ngf -> 3, bias, tanh, n / |n|, the image's mask; writes NCHW
//
// A convolution bias in front of an InstanceNorm without affine parameters cancels in (x - mean): those biases are not read.
// No atomics: every output has one fixed order of summation, the same whatever the tile and the batch (a batch of N is bit-equal to
// N single calls).  No host synchronisation, no allocation.
#include "conv_gemm.h"
#include "workspace.h"

namespace soar {

namespace {

constexpr int CIN0 = 6;                 // image + prior
constexpr int MAX_DOWN = 4;
constexpr int64_t MAX_PIX = int64_t(1) << 30;
constexpr int MAX_N = 65535;             // the InstanceNorm launches carry the image in gridDim.y
constexpr int MAX_NGF = 512;            // the trunk then has 8192 channels: K = 9 Cin, N C and the tap tables stay in int (and one trunk
                                        // convolution already weighs 2.4 GB)
// pixels per partial sum of the InstanceNorm statistics: about 256 chunks per image (at most 265), at least 32 pixels each, so that the trunk's
// 1024 pixels are summed by 32 workgroups per image and not by one.  A function of H W alone: the order does not depend on the batch
inline int in_chunk(int64_t hw) { return hw / 256 < 32 ? 32 : (int)(hw / 256); }
inline int in_chunks(int64_t hw) { return (int)((hw + in_chunk(hw) - 1) / in_chunk(hw)); }
constexpr float IN_EPS = 1e-5f;

struct Cfg {
    int ngf, n_down, n_blocks;
    int ctrunk() const { return ngf << n_down; }
};

bool check_cfg(const char *what, int32_t ngf, int32_t n_down, int32_t n_blocks)
{
    if (ngf < 8 || ngf % 8 != 0 || ngf > MAX_NGF) { set_error("%s: ngf must be a multiple of 8 in 8 .. %d (got %d)", what, MAX_NGF, ngf); return false; }
    if (n_down < 1 || n_down > MAX_DOWN) { set_error("%s: n_down must be 1 .. %d (got %d)", what, MAX_DOWN, n_down); return false; }
    if (n_blocks < 0) { set_error("%s: n_blocks must be >= 0 (got %d)", what, n_blocks); return false; }
    return true;
}
bool check_size(const char *what, const Cfg &c, int32_t N, int32_t H, int32_t W)
{
    if (N < 0 || N > MAX_N) { set_error("%s: N must be 0 .. %d (got %d)", what, MAX_N, N); return false; }
    const int m = 1 << c.n_down;
    if (H < 4 || W < 4 || H % m || W % m || H / m < 2 || W / m < 2) {
        set_error("%s: H and W must be multiples of 2^n_down = %d, at least 4, with at least 2 pixels at the bottom level "
                  "(the reflection padding needs them) (got H=%d, W=%d)", what, m, H, W);
        return false;
    }
    if ((int64_t)(N > 0 ? N : 1) * H * W > MAX_PIX) { set_error("%s: need N * H * W <= 2^30 (N=%d, H=%d, W=%d)", what, N, H, W); return false; }
    return true;
}

// ---- the packed weights of one generator: float offsets, every region 256-byte aligned ----
struct WLayout {
    size_t first, down[MAX_DOWN], up[MAX_DOWN][4], last, last_bias, total;
    size_t block(int j) const { return block0 + (size_t)j * block_stride; }     // convolution j of the trunk (two per block)
    size_t block0, block_stride;
};
// taps of the transposed convolution's phase (py, px): output (2y + py, 2x + px) = sum over the phase's taps of
// in(y + dy, x + dx) w[ky][kx], zero behind the last row / column.  py = 0: (ky 1, dy 0); py = 1: (ky 2, dy 0), (ky 0, dy 1).
inline int phase_axis_taps(int p, int k[2], int d[2])
{
    if (p == 0) { k[0] = 1; d[0] = 0; return 1; }
    k[0] = 2; d[0] = 0; k[1] = 0; d[1] = 1;
    return 2;
}
inline int phase_taps(int ph) { return ((ph >> 1) + 1) * ((ph & 1) + 1); }     // ph = py * 2 + px
WLayout wlayout(const Cfg &c)
{
    WLayout L{};
    Carver pk;
    L.first = pk.float_offset((size_t)c.ngf * 49 * CIN0);
    for (int i = 0; i < c.n_down; i++) L.down[i] = pk.float_offset((size_t)(c.ngf << (i + 1)) * 9 * (c.ngf << i));
    const size_t ct = (size_t)c.ctrunk();
    L.block_stride = align_up(ct * 9 * ct * sizeof(float)) / sizeof(float);
    L.block0 = pk.float_offset(L.block_stride * 2 * (size_t)c.n_blocks);
    for (int i = 0; i < c.n_down; i++) {
        const size_t cin = (size_t)c.ngf << (c.n_down - i), cout = cin / 2;
        for (int ph = 0; ph < 4; ph++) L.up[i][ph] = pk.float_offset(cout * phase_taps(ph) * cin);
    }
    L.last = pk.float_offset((size_t)3 * 49 * c.ngf);
    L.last_bias = pk.float_offset(3);
    L.total = pk.bytes() / sizeof(float);
    return L;
}
inline int n_tensors(const Cfg &c) { return 1 + c.n_down + 2 * c.n_blocks + c.n_down + 2; }

// ---- the workspace: byte offsets ----
struct WsLayout {
    size_t buf[3];          // three activation buffers of the widest level (level 0: N H W ngf floats)
    size_t part;            // double [N][chunks][C][2]
    size_t stats;           // float [N][C][2]: mean, rstd
    size_t total;
};
WsLayout ws_layout(const Cfg &c, int N, int H, int W)
{
    WsLayout L{};
    Carver ws;
    for (int b = 0; b < 3; b++) L.buf[b] = ws.offset<float>((size_t)N * H * W * c.ngf);
    size_t part = 0;
    for (int l = 0; l <= c.n_down; l++) {
        const size_t hw = (size_t)(H >> l) * (W >> l), ch = (size_t)c.ngf << l;
        const size_t v = (size_t)N * in_chunks((int64_t)hw) * ch * 2 * sizeof(double);
        part = v > part ? v : part;
    }
    L.part = ws.offset<char>(part);
    L.stats = ws.offset<float>((size_t)N * c.ctrunk() * 2);
    L.total = ws.bytes() == 0 ? ALIGN : ws.bytes();
    return L;
}

// ---- weight packing ----
struct PackUpK {
    const float *w;         // torch ConvTranspose2d: [Cin][Cout][3][3]
    float *out[4];
    int Cin, Cout;
};
__global__ void __launch_bounds__(256) nn_pack_up_kernel(PackUpK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)k.Cin * k.Cout * 9) return;
    const int t = (int)(e % 9), ky = t / 3, kx = t % 3;
    const int64_t r = e / 9;
    const int co = (int)(r % k.Cout), ci = (int)(r / k.Cout);
    // ky = 1 belongs to the even rows (its only tap); ky = 2, 0 are taps 0, 1 of the odd rows; the same along x
    const int py = ky == 1 ? 0 : 1, ty = ky == 0 ? 1 : 0;
    const int px = kx == 1 ? 0 : 1, tx = kx == 0 ? 1 : 0;
    const int ntx = px + 1, nt = (py + 1) * ntx;
    k.out[py * 2 + px][((size_t)co * nt + ty * ntx + tx) * k.Cin + ci] = k.w[e];
}

// ---- the first layer: thread = pixel, 8 output channels of blockIdx.y; the weights' addresses are uniform over the wave ----
struct FirstK {
    const float *img, *prior;      // [N][3][H][W] at their strides
    int64_t is[4], ps[4];
    const float *w;                // [ngf][49][6]
    float *y;                      // [N][H][W][ngf]
    int64_t npix;
    int H, W, ngf;
};
__global__ void __launch_bounds__(256) nn_first_kernel(FirstK k)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= k.npix) return;
    const int co0 = blockIdx.y * 8;
    const int64_t hw = (int64_t)k.H * k.W;
    const int64_t n = p / hw;
    const int q = (int)(p - n * hw), y = q / k.W, x = q - y * k.W;
    float acc[8];
#pragma unroll
    for (int o = 0; o < 8; o++) acc[o] = 0.f;
    const float *w = k.w + (size_t)co0 * 49 * CIN0;
    for (int t = 0; t < 49; t++) {
        const int yy = mirror(y + t / 7 - 3, k.H), xx = mirror(x + t % 7 - 3, k.W);
        const float *ip = k.img + n * k.is[0] + yy * k.is[2] + xx * k.is[3];
        const float *pp = k.prior + n * k.ps[0] + yy * k.ps[2] + xx * k.ps[3];
        float v[CIN0];
#pragma unroll
        for (int c = 0; c < 3; c++) { v[c] = ip[c * k.is[1]]; v[3 + c] = pp[c * k.ps[1]]; }
#pragma unroll
        for (int c = 0; c < CIN0; c++)
#pragma unroll
            for (int o = 0; o < 8; o++) acc[o] = fmaf(v[c], w[(size_t)o * 49 * CIN0 + t * CIN0 + c], acc[o]);
    }
    float4 *dst = reinterpret_cast<float4 *>(k.y + (size_t)p * k.ngf + co0);
    dst[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    dst[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// ---- InstanceNorm ----
struct InK {
    const float *x;        // [N][HW][C]
    const float *res;      // added after the normalisation (no ReLU then), or NULL (ReLU)
    float *y;
    double *part;          // [N][nchunk][C][2]
    float *stats;          // [N][C][2]
    int64_t hw, n4;        // n4 = N HW C / 4
    int C, nchunk, chunk;
};
// grid (nchunk, N, ceil(C / 4 / 256)); thread t: channel quad t % cq (+ 256 blockIdx.z), pixel row t / cq of the chunk.  A thread
// adds its pixels in order; the rows are then added in order by the first one.
__global__ void __launch_bounds__(256) nn_in_partial_kernel(InK k)
{
    __shared__ double sh[256][8];
    const int t = threadIdx.x, n = blockIdx.y, chunk = blockIdx.x;
    const int c4 = k.C / 4, cqb = c4 < 256 ? c4 : 256, rows = 256 / cqb;
    const int cl = t % cqb, pr = t / cqb, cq = blockIdx.z * 256 + cl;
    const int64_t p0 = (int64_t)chunk * k.chunk, p1 = min(p0 + (int64_t)k.chunk, k.hw);
    double s[8];
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] = 0.0;
    const bool on = pr < rows && cq < c4;
    if (on) {
        for (int64_t p = p0 + pr; p < p1; p += rows) {
            const float4 v = *reinterpret_cast<const float4 *>(k.x + ((size_t)n * k.hw + p) * k.C + cq * 4);
            const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; j++) { s[2 * j] += (double)xs[j]; s[2 * j + 1] += (double)xs[j] * (double)xs[j]; }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) sh[t][j] = s[j];
    __syncthreads();
    if (on && pr == 0) {
        for (int r = 1; r < rows; r++)
#pragma unroll
            for (int j = 0; j < 8; j++) s[j] += sh[r * cqb + cl][j];
        double *dst = k.part + (((size_t)n * k.nchunk + chunk) * k.C + cq * 4) * 2;
#pragma unroll
        for (int j = 0; j < 8; j++) dst[j] = s[j];
    }
}
// thread = (image, channel)
__global__ void __launch_bounds__(256) nn_in_final_kernel(InK k, int N)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N * k.C) return;
    const int n = e / k.C, c = e - n * k.C;
    double s0 = 0.0, s1 = 0.0;
    for (int ch = 0; ch < k.nchunk; ch++) {
        const double *p = k.part + (((size_t)n * k.nchunk + ch) * k.C + c) * 2;
        s0 += p[0];
        s1 += p[1];
    }
    const double mean = s0 / (double)k.hw;
    double var = s1 / (double)k.hw - mean * mean;
    var = var > 0.0 ? var : 0.0;
    k.stats[(size_t)e * 2] = (float)mean;
    k.stats[(size_t)e * 2 + 1] = (float)(1.0 / sqrt(var + (double)IN_EPS));
}
__global__ void __launch_bounds__(256) nn_in_apply_kernel(InK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.n4) return;
    const int c4 = k.C / 4;
    const int cq = (int)(e % c4);
    const int64_t n = e / c4 / k.hw;
    const float4 v = reinterpret_cast<const float4 *>(k.x)[e];
    const float4 *st = reinterpret_cast<const float4 *>(k.stats + ((size_t)n * k.C + cq * 4) * 2);
    const float4 s01 = st[0], s23 = st[1];          // mean0, rstd0, mean1, rstd1 | mean2, rstd2, mean3, rstd3
    float4 o;
    o.x = (v.x - s01.x) * s01.y;
    o.y = (v.y - s01.z) * s01.w;
    o.z = (v.z - s23.x) * s23.y;
    o.w = (v.w - s23.z) * s23.w;
    if (k.res) {
        const float4 r = reinterpret_cast<const float4 *>(k.res)[e];
        o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
    } else {
        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
    }
    reinterpret_cast<float4 *>(k.y)[e] = o;
}

// ---- the last layer and the head: 16 lanes per pixel, lane j holds the channel quads j, j + 16, ... ----
struct LastK {
    const float *x;                // [N][H][W][ngf]
    const float *w, *bias;         // [3][49][ngf], [3]
    const float *img;              // the mask's source: [N][3][H][W] at is
    int64_t is[4];
    float *out;                    // [N][3][H][W]
    int64_t npix;
    int H, W, ngf;
};
__global__ void __launch_bounds__(256) nn_last_kernel(LastK k)
{
    const int j = threadIdx.x & 15;
    const int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool on = p < k.npix;
    const int64_t hw = (int64_t)k.H * k.W;
    const int64_t n = on ? p / hw : 0;
    const int q = on ? (int)(p - n * hw) : 0, y = q / k.W, x = q - y * k.W;
    const int c4 = k.ngf / 4;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int t = 0; t < 49; t++) {
        const int yy = mirror(y + t / 7 - 3, k.H), xx = mirror(x + t % 7 - 3, k.W);
        const float4 *xp = reinterpret_cast<const float4 *>(k.x + ((size_t)n * hw + (size_t)yy * k.W + xx) * k.ngf);
        for (int cq = j; cq < c4; cq += 16) {
            const float4 v = xp[cq];
#pragma unroll
            for (int o = 0; o < 3; o++) {
                const float4 w = reinterpret_cast<const float4 *>(k.w + ((size_t)o * 49 + t) * k.ngf)[cq];
                acc[o] = fmaf(v.x, w.x, acc[o]);
                acc[o] = fmaf(v.y, w.y, acc[o]);
                acc[o] = fmaf(v.z, w.z, acc[o]);
                acc[o] = fmaf(v.w, w.w, acc[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < 3; o++)
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) acc[o] += __shfl_xor(acc[o], m, 16);
    if (!on || j != 0) return;
    const float v0 = tanhf(acc[0] + k.bias[0]), v1 = tanhf(acc[1] + k.bias[1]), v2 = tanhf(acc[2] + k.bias[2]);
    const float nrm = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
    const float *ip = k.img + n * k.is[0] + y * k.is[2] + x * k.is[3];
    const bool inside = fabsf(ip[0]) + fabsf(ip[k.is[1]]) + fabsf(ip[2 * k.is[1]]) != 0.f;
    // where the image is zero the result is exactly 0 (the composition's n / |n| * 0)
    float *o = k.out + (size_t)n * 3 * hw + q;
    o[0] = inside ? v0 / nrm : 0.f;
    o[hw] = inside ? v1 / nrm : 0.f;
    o[2 * hw] = inside ? v2 / nrm : 0.f;
}

// ---- host side ----
int instance_norm(const float *x, const float *res, float *y, int N, int64_t hw, int C, double *part, float *stats, hipStream_t stream)
{
    InK k{};
    k.x = x; k.res = res; k.y = y; k.part = part; k.stats = stats;
    k.hw = hw; k.C = C; k.chunk = in_chunk(hw); k.nchunk = in_chunks(hw);
    k.n4 = (int64_t)N * hw * C / 4;
    hipLaunchKernelGGL(nn_in_partial_kernel, dim3((unsigned)k.nchunk, (unsigned)N, (unsigned)((C / 4 + 255) / 256)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("nn_in_partial", stream, 0);
    hipLaunchKernelGGL(nn_in_final_kernel, dim3(blocks((int64_t)N * C)), dim3(256), 0, stream, k, N);
    SOAR_LAUNCH_OK("nn_in_final", stream, 0);
    hipLaunchKernelGGL(nn_in_apply_kernel, dim3(blocks(k.n4)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("nn_in_apply", stream, 0);
    return 0;
}

// one convolution over the batch's flat rows: grid Hg x Wg, input (gy stride + dy, gx stride + dx), output (gy os + py, gx os + px)
ConvGemm conv_k(const float *x, float *y, int N, int Hin, int Win, int Cin, int Cout, int Hg, int Wg, int stride, int os, int reflect)
{
    ConvGemm k{};
    k.x = x; k.ldx = Cin; k.xim = (int64_t)Hin * Win;
    k.y = y; k.ldy = Cout; k.yim = (int64_t)Hg * os * Wg * os; k.Wout = Wg * os; k.os = os;
    k.alpha = 1.f;
    k.N = N; k.Hg = Hg; k.Wg = Wg; k.Hin = Hin; k.Win = Win; k.Cin = Cin; k.Cout = Cout;
    k.stride = stride; k.dil = 1; k.reflect = reflect;
    k.nph = 1;
    return k;
}

int run_generator(const Cfg &c, const SoarNormalNetArgs *a, const float *prior, const int64_t *prior_stride, const float *P, float *out,
                  char *ws, const WsLayout &L, hipStream_t stream)
{
    const WLayout WL = wlayout(c);
    float *buf[3] = {reinterpret_cast<float *>(ws + L.buf[0]), reinterpret_cast<float *>(ws + L.buf[1]), reinterpret_cast<float *>(ws + L.buf[2])};
    double *part = reinterpret_cast<double *>(ws + L.part);
    float *stats = reinterpret_cast<float *>(ws + L.stats);
    const int N = a->N;
    int H = a->H, W = a->W, C = c.ngf;
    const int64_t npix0 = (int64_t)N * H * W;

    FirstK fk{};
    fk.img = a->image; fk.prior = prior;
    for (int j = 0; j < 4; j++) { fk.is[j] = a->image_stride[j]; fk.ps[j] = prior_stride[j]; }
    fk.w = P + WL.first; fk.y = buf[0]; fk.npix = npix0; fk.H = H; fk.W = W; fk.ngf = c.ngf;
    hipLaunchKernelGGL(nn_first_kernel, dim3(blocks(npix0), (unsigned)(c.ngf / 8)), dim3(256), 0, stream, fk);
    SOAR_LAUNCH_OK("nn_first", stream, 0);
    if (instance_norm(buf[0], nullptr, buf[0], N, (int64_t)H * W, C, part, stats, stream)) return 1;
    int cur = 0;

    for (int i = 0; i < c.n_down; i++) {
        const int nxt = (cur + 1) % 3;
        ConvGemm k = conv_k(buf[cur], buf[nxt], N, H, W, C, 2 * C, H / 2, W / 2, 2, 1, 0);
        square_taps(k.ph[0], P + WL.down[i], 9 * C, 3, -1);
        if (launch_conv_gemm(k, stream)) return 1;
        H /= 2; W /= 2; C *= 2;
        if (instance_norm(buf[nxt], nullptr, buf[nxt], N, (int64_t)H * W, C, part, stats, stream)) return 1;
        cur = nxt;
    }
    for (int b = 0; b < c.n_blocks; b++) {
        const int t1 = (cur + 1) % 3, t2 = (cur + 2) % 3;
        ConvGemm k = conv_k(buf[cur], buf[t1], N, H, W, C, C, H, W, 1, 1, 1);
        square_taps(k.ph[0], P + WL.block(2 * b), 9 * C, 3, -1);
        if (launch_conv_gemm(k, stream)) return 1;
        if (instance_norm(buf[t1], nullptr, buf[t1], N, (int64_t)H * W, C, part, stats, stream)) return 1;
        k.x = buf[t1]; k.y = buf[t2];
        square_taps(k.ph[0], P + WL.block(2 * b + 1), 9 * C, 3, -1);
        if (launch_conv_gemm(k, stream)) return 1;
        if (instance_norm(buf[t2], buf[cur], buf[t2], N, (int64_t)H * W, C, part, stats, stream)) return 1;
        cur = t2;
    }
    for (int i = 0; i < c.n_down; i++) {
        const int nxt = (cur + 1) % 3;
        ConvGemm k = conv_k(buf[cur], buf[nxt], N, H, W, C, C / 2, H, W, 1, 2, 0);
        k.nph = 4;
        for (int ph = 0; ph < 4; ph++) {
            ConvTaps &p = k.ph[ph];
            p.w = P + WL.up[i][ph];
            p.py = ph >> 1; p.px = ph & 1;
            int ky[2], dy[2], kx[2], dx[2];
            const int ny = phase_axis_taps(p.py, ky, dy), nx = phase_axis_taps(p.px, kx, dx);
            p.ntaps = ny * nx;
            p.ldw = (int64_t)p.ntaps * C;
            for (int ty = 0; ty < ny; ty++)
                for (int tx = 0; tx < nx; tx++) { p.dy[ty * nx + tx] = (signed char)dy[ty]; p.dx[ty * nx + tx] = (signed char)dx[tx]; }
        }
        if (launch_conv_gemm(k, stream)) return 1;
        H *= 2; W *= 2; C /= 2;
        if (instance_norm(buf[nxt], nullptr, buf[nxt], N, (int64_t)H * W, C, part, stats, stream)) return 1;
        cur = nxt;
    }
    LastK lk{};
    lk.x = buf[cur]; lk.w = P + WL.last; lk.bias = P + WL.last_bias; lk.img = a->image;
    for (int j = 0; j < 4; j++) lk.is[j] = a->image_stride[j];
    lk.out = out; lk.npix = npix0; lk.H = H; lk.W = W; lk.ngf = c.ngf;
    hipLaunchKernelGGL(nn_last_kernel, dim3((unsigned)((npix0 + 15) / 16)), dim3(256), 0, stream, lk);
    SOAR_LAUNCH_OK("nn_last", stream, 0);
    return 0;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_normalnet_weights_bytes(int32_t ngf, int32_t n_down, int32_t n_blocks, size_t *bytes)
{
    if (!bytes) { set_error("soar_normalnet_weights_bytes: NULL bytes"); return 1; }
    if (!check_cfg("soar_normalnet_weights_bytes", ngf, n_down, n_blocks)) return 1;
    *bytes = wlayout(Cfg{ngf, n_down, n_blocks}).total * sizeof(float);
    return 0;
}

extern "C" int soar_normalnet_pack_weights(int32_t ngf, int32_t n_down, int32_t n_blocks, const float *const *tensors, int32_t count,
                                           void *packed, size_t packed_bytes, void *stream_)
{
    const char *what = "soar_normalnet_pack_weights";
    if (!check_cfg(what, ngf, n_down, n_blocks)) return 1;
    const Cfg c{ngf, n_down, n_blocks};
    if (!tensors || count != n_tensors(c)) { set_error("%s: need %d tensors (got %d)", what, n_tensors(c), tensors ? count : 0); return 1; }
    for (int i = 0; i < count; i++)
        if (!tensors[i]) { set_error("%s: NULL tensor %d", what, i); return 1; }
    const WLayout L = wlayout(c);
    if (!packed || packed_bytes < L.total * sizeof(float) || ((uintptr_t)packed & (ALIGN - 1))) {
        set_error("%s: packed must be %zu bytes, 256-byte aligned (got %zu)", what, L.total * sizeof(float), packed_bytes);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *P = static_cast<float *>(packed);
    int ti = 0;
    auto pack = [&](const float *w, float *dst, int cout, int cin, int kk) { return launch_conv_pack(w, dst, nullptr, cout, cin, kk, 0, stream); };
    if (pack(tensors[ti++], P + L.first, ngf, CIN0, 49)) return 1;
    for (int i = 0; i < n_down; i++)
        if (pack(tensors[ti++], P + L.down[i], ngf << (i + 1), ngf << i, 9)) return 1;
    for (int j = 0; j < 2 * n_blocks; j++)
        if (pack(tensors[ti++], P + L.block(j), c.ctrunk(), c.ctrunk(), 9)) return 1;
    for (int i = 0; i < n_down; i++) {
        PackUpK k{};
        k.w = tensors[ti++];
        k.Cin = ngf << (n_down - i);
        k.Cout = k.Cin / 2;
        for (int ph = 0; ph < 4; ph++) k.out[ph] = P + L.up[i][ph];
        hipLaunchKernelGGL(nn_pack_up_kernel, dim3(blocks((int64_t)k.Cin * k.Cout * 9)), dim3(256), 0, stream, k);
        SOAR_LAUNCH_OK("nn_pack_up", stream, 0);
    }
    if (pack(tensors[ti++], P + L.last, 3, ngf, 49)) return 1;
    SOAR_HIP_OK(hipMemcpyAsync(P + L.last_bias, tensors[ti++], 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

extern "C" int soar_normalnet_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t ngf, int32_t n_down, int32_t n_blocks, size_t *bytes)
{
    const char *what = "soar_normalnet_workspace_bytes";
    if (!bytes) { set_error("%s: NULL bytes", what); return 1; }
    if (!check_cfg(what, ngf, n_down, n_blocks)) return 1;
    const Cfg c{ngf, n_down, n_blocks};
    if (!check_size(what, c, N, H, W)) return 1;
    *bytes = ws_layout(c, N, H, W).total;
    return 0;
}

extern "C" int soar_normalnet_forward(const SoarNormalNetArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *what = "soar_normalnet_forward";
    if (!a) { set_error("%s: NULL args", what); return 1; }
    if (!check_cfg(what, a->ngf, a->n_down, a->n_blocks)) return 1;
    const Cfg c{a->ngf, a->n_down, a->n_blocks};
    if (!check_size(what, c, a->N, a->H, a->W)) return 1;
    if (a->N == 0) return 0;
    if (!a->image || !a->prior_F || !a->prior_B || !a->weights_F || !a->weights_B || !a->normal_F || !a->normal_B) {
        set_error("%s: NULL image / prior / weights / output", what);
        return 1;
    }
    if (((uintptr_t)a->weights_F | (uintptr_t)a->weights_B) & (ALIGN - 1)) { set_error("%s: the packed weights must be 256-byte aligned", what); return 1; }
    const WsLayout L = ws_layout(c, a->N, a->H, a->W);
    if (!workspace_ok(what, workspace, workspace_bytes, L.total, "soar_normalnet_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    char *ws = static_cast<char *>(workspace);
    if (run_generator(c, a, a->prior_F, a->prior_F_stride, static_cast<const float *>(a->weights_F), a->normal_F, ws, L, stream)) return 1;
    return run_generator(c, a, a->prior_B, a->prior_B_stride, static_cast<const float *>(a->weights_B), a->normal_B, ws, L, stream);
}
