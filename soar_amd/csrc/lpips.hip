// lpips.hip -- LPIPS-VGG (soar_amd/lpips.py): lpips 0.1, net='vgg', eval mode, as include/soar_hip.h and DESIGN.md 9e state it.
//
//   (conv_pack_kernel        conv_gemm.hip: torch [Cout][Cin][3][3] -> [Cout][tap][Cin] (forward) and, spatially flipped and
//                            transposed, [Cin][tap][Cout] (data gradient): both directions are then the same implicit GEMM)
//   lpips_first_kernel       conv1_1: scaling layer on load (strided NCHW input, zero padding in scaled space), 27 -> 64, bias, ReLU
//   lpips_conv_kernel        conv3x3 pad 1 on NHWC activations as an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact f32 products):
//                            M = pixels, N = output channels, K = 9 Cin ordered (tap, cin).  A wave owns WM x WN blocks of 32 x 32
//                            and reads its operands straight from global memory (16 contiguous floats of one pixel / one weight
//                            row per lane and chunk of 32 k), the next chunk in flight while the MFMAs of this one run.
//                            Epilogue: bias + ReLU (forward), the ReLU mask of the layer below (data gradient) or nothing
//   lpips_pool_kernel        2x2 max pool, floor mode
//   lpips_head_kernel        one wave per tap pixel: norms, s = sum_c w_c (u0_c - u1_c)^2 and the tap's gradient planes
//   lpips_sum_kernel         per image, the pixels' s of every tap in double, in a fixed order -> out[n]
//   lpips_gate_kernel        data gradient at a tap: the pool's gradient routed to the window's first maximum (recomputed from
//                            the stored activation), + g_out[n] * the tap's gradient plane, times the ReLU mask
//   lpips_first_bwd_kernel   conv1_1's data gradient, / scale, written through the caller's strides
//
// No atomics: every value and gradient has one fixed order of summation (bitwise reproducible).  No host synchronisation, no
// allocation.
#include "conv_gemm.h"
#include "workspace.h"

namespace soar {

namespace {

constexpr int NL = SOAR_LPIPS_LAYERS;
constexpr int NT = SOAR_LPIPS_TAPS;
constexpr int MIN_SIZE = 16;
constexpr int64_t MAX_PIX = int64_t(1) << 30;
constexpr float EPS = 1e-10f;

const int CIN[NL] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int COUT[NL] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
const int LEVEL[NL] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
const int TAP_LAYER[NT] = {1, 3, 6, 9, 12};
const int TAP_C[NT] = {64, 128, 256, 512, 512};
inline bool pool_before(int i) { return i == 2 || i == 4 || i == 7 || i == 10; }
inline int tap_of_layer(int i)
{
    for (int k = 0; k < NT; k++)
        if (TAP_LAYER[k] == i) return k;
    return -1;
}

// ---- the packed weights: float offsets, every region 256-byte aligned ----
struct WLayout {
    size_t fwd[NL], bwd[NL], bias[NL], lin[NT], shift, scale, total;   // floats
};
WLayout wlayout()
{
    WLayout L{};
    Carver pk;
    for (int i = 0; i < NL; i++) {
        L.fwd[i] = pk.float_offset((size_t)COUT[i] * 9 * CIN[i]);         // conv1_1: the torch layout [64][3][3][3]
        L.bwd[i] = i == 0 ? 0 : pk.float_offset((size_t)COUT[i] * 9 * CIN[i]);
        L.bias[i] = pk.float_offset(COUT[i]);
    }
    for (int k = 0; k < NT; k++) L.lin[k] = pk.float_offset(TAP_C[k]);
    L.shift = pk.float_offset(3);
    L.scale = pk.float_offset(3);
    L.total = pk.bytes() / sizeof(float);
    return L;
}

// ---- the workspace: byte offsets ----
struct Dims {
    int N, H[5], W[5];
    int64_t pix(int lev) const { return (int64_t)N * H[lev] * W[lev]; }
};
Dims dims_of(int N, int H, int W)
{
    Dims d{};
    d.N = N;
    d.H[0] = H; d.W[0] = W;
    for (int l = 1; l < 5; l++) { d.H[l] = d.H[l - 1] / 2; d.W[l] = d.W[l - 1] / 2; }
    return d;
}
struct WsLayout {
    size_t act[2][NL];      // kept branch: every layer's output (the ReLU masks, the pools' windows, the taps)
    size_t gtap[2][NT];     // kept branch: the taps' gradient planes (without g_out)
    size_t ping[2][2];      // branch not kept: two buffers of the widest level, used in turn
    size_t pool;            // the last pool's output (the next layer's input)
    size_t s[NT];           // per tap pixel: s
    size_t gbuf[2];         // backward: the data gradient, two buffers used in turn
    size_t total;
};
WsLayout ws_layout(const Dims &d, int grads)
{
    WsLayout L{};
    Carver ws;
    const int64_t widest = d.pix(0) * 64;                      // level 0 at 64 channels holds the most of any level
    for (int b = 0; b < 2; b++) {
        if (grads & (1 << b)) {
            for (int i = 0; i < NL; i++) L.act[b][i] = ws.offset<float>(d.pix(LEVEL[i]) * COUT[i]);
            for (int k = 0; k < NT; k++) L.gtap[b][k] = ws.offset<float>(d.pix(LEVEL[TAP_LAYER[k]]) * TAP_C[k]);
        } else {
            L.ping[b][0] = ws.offset<float>(widest);
            L.ping[b][1] = ws.offset<float>(widest);
        }
    }
    L.pool = ws.offset<float>(d.pix(1) * 64);
    for (int k = 0; k < NT; k++) L.s[k] = ws.offset<float>(d.pix(LEVEL[TAP_LAYER[k]]));
    if (grads) {
        L.gbuf[0] = ws.offset<float>(widest);
        L.gbuf[1] = ws.offset<float>(widest);
    }
    L.total = ws.bytes() == 0 ? ALIGN : ws.bytes();
    return L;
}

// ---- conv1_1 with the scaling layer ----
struct FirstK {
    const float *x;                // [N][3][H][W] at xs
    int64_t xs[4];
    const float *w, *bias, *shift, *scale;   // w: torch [64][3][3][3]
    float *y;                      // [N][H][W][64]
    const float *gpre;             // backward: [N][H][W][64] gradient of conv1_1's pre-activation
    float *g;                      // backward: [N][3][H][W] at gs
    int64_t gs[4];
    int64_t npix;
    int H, W;
};

// thread = (pixel, 4 output channels)
__global__ void __launch_bounds__(256) lpips_first_kernel(FirstK k)
{
    __shared__ float Ws[64 * 27], Bs[64];
    for (int e = threadIdx.x; e < 64 * 27; e += 256) Ws[e] = k.w[e];
    if (threadIdx.x < 64) Bs[threadIdx.x] = k.bias[threadIdx.x];
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t p = t >> 4;
    const int co = (int)(t & 15) * 4;
    if (p >= k.npix) return;
    const int64_t hw = (int64_t)k.H * k.W;
    const int64_t n = p / hw;
    const int q = (int)(p - n * hw), y = q / k.W, x = q - y * k.W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int ci = 0; ci < 3; ci++) {
        const float sh = k.shift[ci], sc = k.scale[ci];
#pragma unroll
        for (int t9 = 0; t9 < 9; t9++) {
            const int yy = y + t9 / 3 - 1, xx = x + t9 % 3 - 1;
            float v = 0.f;                                           // zero padding of the scaled image
            if (yy >= 0 && yy < k.H && xx >= 0 && xx < k.W)
                v = (k.x[n * k.xs[0] + ci * k.xs[1] + yy * k.xs[2] + xx * k.xs[3]] - sh) / sc;
#pragma unroll
            for (int o = 0; o < 4; o++) acc[o] = fmaf(v, Ws[(co + o) * 27 + ci * 9 + t9], acc[o]);
        }
    }
    float4 r;
    r.x = fmaxf(acc[0] + Bs[co], 0.f);
    r.y = fmaxf(acc[1] + Bs[co + 1], 0.f);
    r.z = fmaxf(acc[2] + Bs[co + 2], 0.f);
    r.w = fmaxf(acc[3] + Bs[co + 3], 0.f);
    *reinterpret_cast<float4 *>(k.y + (size_t)p * 64 + co) = r;
}

// thread = input pixel: g[ci] = sum over the 9 taps and 64 channels of gpre at the output pixel that reads (y, x) through the
// tap, times w[co][ci][tap]; / scale[ci]
__global__ void __launch_bounds__(256) lpips_first_bwd_kernel(FirstK k)
{
    __shared__ float Ws[64 * 27];
    for (int e = threadIdx.x; e < 64 * 27; e += 256) Ws[e] = k.w[e];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= k.npix) return;
    const int64_t hw = (int64_t)k.H * k.W;
    const int64_t n = p / hw;
    const int q = (int)(p - n * hw), y = q / k.W, x = q - y * k.W;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int t9 = 0; t9 < 9; t9++) {
        const int oy = y - (t9 / 3 - 1), ox = x - (t9 % 3 - 1);
        if (oy < 0 || oy >= k.H || ox < 0 || ox >= k.W) continue;
        const float4 *g4 = reinterpret_cast<const float4 *>(k.gpre + ((size_t)n * hw + (size_t)oy * k.W + ox) * 64);
        for (int c4 = 0; c4 < 16; c4++) {
            const float4 gv = g4[c4];
            const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const int co = c4 * 4 + o;
#pragma unroll
                for (int ci = 0; ci < 3; ci++) acc[ci] = fmaf(gg[o], Ws[co * 27 + ci * 9 + t9], acc[ci]);
            }
        }
    }
#pragma unroll
    for (int ci = 0; ci < 3; ci++) k.g[n * k.gs[0] + ci * k.gs[1] + y * k.gs[2] + x * k.gs[3]] = acc[ci] / k.scale[ci];
}

// ---- conv3x3 as an implicit GEMM on the f32-input MFMA ----
enum { EPI_BIAS_RELU = 0, EPI_MASK = 1, EPI_PLAIN = 2 };
struct ConvK {
    const float *x;        // [M][Cin] NHWC
    const float *w;        // [Cout][9][Cin]
    const float *bias;     // EPI_BIAS_RELU: [Cout]
    const float *mask;     // EPI_MASK: [M][Cout]; the output is kept where mask > 0
    float *y;              // [M][Cout]
    int64_t M;
    int H, W, Cin, Cout, epi;
};

// Lane l of a wave: row / column i = l & 31 of every 32 x 32 block, k half h = l >> 5.  In a chunk of 32 k (one tap, 32 input
// channels) step s of the MFMA sums k = s (h = 0) and k = 16 + s (h = 1), so that a lane's operands are 16 contiguous floats.
// The order of the sum of every output is the same whatever WM, WN and the output's place in the tile.
template <int WM, int WN>
__global__ void __launch_bounds__(256) lpips_conv_kernel(ConvK k)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntn = k.Cout / (32 * WN);
    const int64_t tile = (int64_t)blockIdx.x * 4 + wave;
    const int64_t tm = tile / ntn;
    const int tn = (int)(tile - tm * ntn);
    const int64_t p0 = tm * 32 * WM;
    if (p0 >= k.M) return;
    const int i = lane & 31, h = lane >> 5;
    const int64_t hw = (int64_t)k.H * k.W;
    int py[WM], px[WM];
    int64_t pimg[WM];
    bool pv[WM];
#pragma unroll
    for (int r = 0; r < WM; r++) {
        const int64_t p = p0 + r * 32 + i;
        pv[r] = p < k.M;
        const int64_t n = pv[r] ? p / hw : 0;
        const int q = pv[r] ? (int)(p - n * hw) : 0;
        py[r] = q / k.W;
        px[r] = q - py[r] * k.W;
        pimg[r] = n * hw;
    }
    const int K = 9 * k.Cin, cpt = k.Cin / 32, nch = K / 32;
    const float *wrow[WN];
#pragma unroll
    for (int c = 0; c < WN; c++) wrow[c] = k.w + (size_t)(tn * 32 * WN + c * 32 + i) * K + h * 16;

    f32x16 acc[WM][WN];
#pragma unroll
    for (int r = 0; r < WM; r++)
#pragma unroll
        for (int c = 0; c < WN; c++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[r][c][e] = 0.f;

    float4 a[WM][4], b[WN][4], an[WM][4], bn[WN][4];
    auto load = [&](int ch, float4 (&A)[WM][4], float4 (&B)[WN][4]) {
        const int t = ch / cpt;
        const int ci0 = (ch - t * cpt) * 32 + h * 16;
        const int dy = t / 3 - 1, dx = t % 3 - 1;
#pragma unroll
        for (int r = 0; r < WM; r++) {
            const int yy = py[r] + dy, xx = px[r] + dx;
            if (pv[r] && yy >= 0 && yy < k.H && xx >= 0 && xx < k.W) {
                const float4 *s = reinterpret_cast<const float4 *>(k.x + (size_t)(pimg[r] + (int64_t)yy * k.W + xx) * k.Cin + ci0);
#pragma unroll
                for (int j = 0; j < 4; j++) A[r][j] = s[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; j++) A[r][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int c = 0; c < WN; c++) {
            const float4 *s = reinterpret_cast<const float4 *>(wrow[c] + (size_t)ch * 32);
#pragma unroll
            for (int j = 0; j < 4; j++) B[c][j] = s[j];
        }
    };
    load(0, a, b);
    for (int ch = 0; ch < nch; ch++) {
        if (ch + 1 < nch) load(ch + 1, an, bn);
#pragma unroll
        for (int s = 0; s < 16; s++)
#pragma unroll
            for (int r = 0; r < WM; r++)
#pragma unroll
                for (int c = 0; c < WN; c++)
                    acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(a[r][s >> 2], s & 3), comp(b[c][s >> 2], s & 3), acc[r][c], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < WM; r++)
#pragma unroll
            for (int j = 0; j < 4; j++) a[r][j] = an[r][j];
#pragma unroll
        for (int c = 0; c < WN; c++)
#pragma unroll
            for (int j = 0; j < 4; j++) b[c][j] = bn[c][j];
    }
#pragma unroll
    for (int c = 0; c < WN; c++) {
        const int co = tn * 32 * WN + c * 32 + i;
        const float bias = k.epi == EPI_BIAS_RELU ? k.bias[co] : 0.f;
#pragma unroll
        for (int r = 0; r < WM; r++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int64_t p = p0 + r * 32 + mfma_row(e, h);
                if (p >= k.M) continue;
                const size_t idx = (size_t)p * k.Cout + co;
                float v = acc[r][c][e];
                if (k.epi == EPI_BIAS_RELU) v = fmaxf(v + bias, 0.f);
                else if (k.epi == EPI_MASK) v = k.mask[idx] > 0.f ? v : 0.f;
                k.y[idx] = v;
            }
    }
}

// ---- 2x2 max pool, floor mode (NHWC, four channels per thread) ----
struct PoolK {
    const float *x;
    float *y;
    int64_t n4;            // N * Ho * Wo * C / 4
    int H, W, Ho, Wo, C;
};
__global__ void __launch_bounds__(256) lpips_pool_kernel(PoolK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.n4) return;
    const int c4 = k.C / 4;
    const int cq = (int)(e % c4);
    const int64_t pix = e / c4;
    const int64_t ohw = (int64_t)k.Ho * k.Wo;
    const int64_t n = pix / ohw;
    const int q = (int)(pix - n * ohw), oy = q / k.Wo, ox = q - oy * k.Wo;
    const float4 *x4 = reinterpret_cast<const float4 *>(k.x);
    const size_t base = ((size_t)n * k.H * k.W + (size_t)(2 * oy) * k.W + 2 * ox) * c4 + cq;
    const size_t row = (size_t)k.W * c4;
    const float4 v00 = x4[base], v01 = x4[base + c4], v10 = x4[base + row], v11 = x4[base + row + c4];
    float4 m;
    m.x = fmaxf(fmaxf(v00.x, v01.x), fmaxf(v10.x, v11.x));
    m.y = fmaxf(fmaxf(v00.y, v01.y), fmaxf(v10.y, v11.y));
    m.z = fmaxf(fmaxf(v00.z, v01.z), fmaxf(v10.z, v11.z));
    m.w = fmaxf(fmaxf(v00.w, v01.w), fmaxf(v10.w, v11.w));
    reinterpret_cast<float4 *>(k.y)[e] = m;
}

// ---- the head: one wave per tap pixel, lane j holds channels j, j + 64, ... ----
struct HeadK {
    const float *f0, *f1, *w;
    float *s, *g0, *g1;    // g0 / g1: NULL when that branch is not kept
    int64_t npix;
    int C;
    float inv_hw;          // 1 / (H_k W_k)
};
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// the gradient of the tap's mean of s with respect to f (the other side's u fixed): a = 2 w (u - u_other) / (H_k W_k),
// g = a / (n + eps) - f (sum_i a_i f_i) / (n (n + eps)^2); 0 where n = 0 (f = 0 there, and the ReLU mask below drops it anyway).
// Written for either side alike, so that a call with in0 and in1 swapped gives the same gradient bit for bit.
template <int J>
__device__ __forceinline__ void head_grad(const float (&f)[J], const float (&u)[J], const float (&uo)[J], const float (&w)[J], float n,
                                          float e, float inv_hw, float *g, int lane)
{
    float a[J], dot = 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) {
        a[j] = 2.f * w[j] * (u[j] - uo[j]) * inv_hw;
        dot += a[j] * f[j];
    }
    dot = wave_sum(dot);
    const float c = n > 0.f ? dot / (n * e * e) : 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) g[j * 64 + lane] = n > 0.f ? a[j] / e - f[j] * c : 0.f;
}
template <int J>
__global__ void __launch_bounds__(256) lpips_head_kernel(HeadK k)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= k.npix) return;
    const float *f0p = k.f0 + (size_t)p * k.C, *f1p = k.f1 + (size_t)p * k.C;
    float f0[J], f1[J], w[J], ss0 = 0.f, ss1 = 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) {
        f0[j] = f0p[j * 64 + lane];
        f1[j] = f1p[j * 64 + lane];
        w[j] = k.w[j * 64 + lane];
        ss0 += f0[j] * f0[j];
        ss1 += f1[j] * f1[j];
    }
    const float n0 = sqrtf(wave_sum(ss0)), n1 = sqrtf(wave_sum(ss1));
    const float e0 = n0 + EPS, e1 = n1 + EPS;
    float u0[J], u1[J], sd = 0.f;
#pragma unroll
    for (int j = 0; j < J; j++) {
        u0[j] = f0[j] / e0;
        u1[j] = f1[j] / e1;
        const float d = u0[j] - u1[j];
        sd += w[j] * (d * d);
    }
    sd = wave_sum(sd);
    if (lane == 0) k.s[p] = sd;
    if (k.g0) head_grad<J>(f0, u0, u1, w, n0, e0, k.inv_hw, k.g0 + (size_t)p * k.C, lane);
    if (k.g1) head_grad<J>(f1, u1, u0, w, n1, e1, k.inv_hw, k.g1 + (size_t)p * k.C, lane);
}

// ---- out[n] = sum over the taps of the mean of s: one workgroup per image, in double, in a fixed order ----
struct SumK {
    const float *s[NT];
    int64_t hw[NT];
    float *out;
};
constexpr int SUM_THREADS = 1024;
__global__ void __launch_bounds__(SUM_THREADS) lpips_sum_kernel(SumK k)
{
    __shared__ double part[SUM_THREADS];
    const int n = blockIdx.x, t = threadIdx.x;
    double total = 0.0;
    for (int tap = 0; tap < NT; tap++) {
        const float *s = k.s[tap] + (size_t)n * k.hw[tap];
        double v = 0.0;
#pragma unroll 8
        for (int64_t q = t; q < k.hw[tap]; q += SUM_THREADS) v += (double)s[q];      // (eight loads in flight, the adds in order)
        part[t] = v;
        __syncthreads();
        for (int m = SUM_THREADS / 2; m >= 1; m >>= 1) {
            if (t < m) part[t] += part[t + m];
            __syncthreads();
        }
        total += part[0] / (double)k.hw[tap];
        __syncthreads();
    }
    if (t == 0) k.out[n] = (float)total;
}

// ---- data gradient at a tap: pool routing + g_out * tap plane, then the ReLU mask ----
struct GateK {
    const float *glow;     // [N][Ho][Wo][C] gradient of the pool's output, or NULL (relu5_3)
    const float *act;      // [N][H][W][C] the layer's output (before the pool)
    const float *gtap;     // [N][H][W][C]
    const float *g_out;    // [N]
    float *g;              // [N][H][W][C]
    int64_t n4;            // N * H * W * C / 4
    int H, W, Ho, Wo, C;
};
__global__ void __launch_bounds__(256) lpips_gate_kernel(GateK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.n4) return;
    const int c4 = k.C / 4;
    const int cq = (int)(e % c4);
    const int64_t pix = e / c4;
    const int64_t hw = (int64_t)k.H * k.W;
    const int64_t n = pix / hw;
    const int q = (int)(pix - n * hw), y = q / k.W, x = q - y * k.W;
    const float4 *a4 = reinterpret_cast<const float4 *>(k.act);
    const float4 av = a4[e];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    // rows and columns the floor pool dropped get nothing from it
    if (k.glow && (y >> 1) < k.Ho && (x >> 1) < k.Wo) {
        // the window's first maximum in row-major order (only a strictly greater value replaces it), as torch's max_pool2d
        const int wy = y >> 1, wx = x >> 1, pos = (y & 1) * 2 + (x & 1);
        const size_t base = ((size_t)n * hw + (size_t)(2 * wy) * k.W + 2 * wx) * c4 + cq;
        const size_t row = (size_t)k.W * c4;
        const float4 w4[4] = {a4[base], a4[base + c4], a4[base + row], a4[base + row + c4]};
        const float4 gl = reinterpret_cast<const float4 *>(k.glow)[((size_t)n * k.Ho * k.Wo + (size_t)wy * k.Wo + wx) * c4 + cq];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            int sel = 0;
            float m = comp(w4[0], o);
#pragma unroll
            for (int j = 1; j < 4; j++)
                if (comp(w4[j], o) > m) { m = comp(w4[j], o); sel = j; }
            if (sel == pos) v[o] = comp(gl, o);
        }
    }
    const float go = k.g_out[n];
    const float4 gt = reinterpret_cast<const float4 *>(k.gtap)[e];
#pragma unroll
    for (int o = 0; o < 4; o++) v[o] += go * comp(gt, o);
    float4 r;
    r.x = av.x > 0.f ? v[0] : 0.f;
    r.y = av.y > 0.f ? v[1] : 0.f;
    r.z = av.z > 0.f ? v[2] : 0.f;
    r.w = av.w > 0.f ? v[3] : 0.f;
    reinterpret_cast<float4 *>(k.g)[e] = r;
}

// ---- host side ----
int launch_conv(const ConvK &k, hipStream_t stream)
{
    // the widest wave tile that still gives every SIMD (1024) two waves
    auto waves = [&](int wm, int wn) { return (k.M + 32 * wm - 1) / (32 * wm) * (k.Cout / (32 * wn)); };
    if (waves(2, 2) >= 2048) {
        hipLaunchKernelGGL((lpips_conv_kernel<2, 2>), dim3(blocks(waves(2, 2) * 64)), dim3(256), 0, stream, k);
    } else if (waves(1, 2) >= 2048) {
        hipLaunchKernelGGL((lpips_conv_kernel<1, 2>), dim3(blocks(waves(1, 2) * 64)), dim3(256), 0, stream, k);
    } else {
        hipLaunchKernelGGL((lpips_conv_kernel<1, 1>), dim3(blocks(waves(1, 1) * 64)), dim3(256), 0, stream, k);
    }
    SOAR_LAUNCH_OK("lpips_conv", stream, 0);
    return 0;
}

bool check_size(const char *what, int32_t N, int32_t H, int32_t W)
{
    if (N < 0) { set_error("%s: N must be >= 0 (got %d)", what, N); return false; }
    if (H < MIN_SIZE || W < MIN_SIZE) {
        set_error("%s: LPIPS-VGG needs H, W >= %d so that relu5_3 has at least one pixel (got H=%d, W=%d)", what, MIN_SIZE, H, W);
        return false;
    }
    if ((int64_t)N * H * W > MAX_PIX) { set_error("%s: need N * H * W <= 2^30 (N=%d, H=%d, W=%d)", what, N, H, W); return false; }
    return true;
}

bool check_args(const char *what, const SoarLpipsArgs *a, const void *ws, size_t ws_bytes)
{
    if (!a) { set_error("%s: NULL args", what); return false; }
    if (!check_size(what, a->N, a->H, a->W)) return false;
    if (a->grads < 0 || a->grads > 3) { set_error("%s: grads is a bitmask of 1 (in0) and 2 (in1) (got %d)", what, a->grads); return false; }
    if (a->N == 0) return true;
    if (!a->in0 || !a->in1 || !a->weights) { set_error("%s: NULL in0 / in1 / weights", what); return false; }
    if ((uintptr_t)a->weights & (ALIGN - 1)) { set_error("%s: the packed weights must be 256-byte aligned", what); return false; }
    return workspace_ok(what, ws, ws_bytes, ws_layout(dims_of(a->N, a->H, a->W), a->grads).total, "soar_lpips_workspace_bytes");
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_lpips_weights_bytes(size_t *bytes)
{
    if (!bytes) { set_error("soar_lpips_weights_bytes: NULL bytes"); return 1; }
    *bytes = wlayout().total * sizeof(float);
    return 0;
}

extern "C" int soar_lpips_pack_weights(const SoarLpipsWeights *w, void *packed, size_t packed_bytes, void *stream_)
{
    if (!w) { set_error("soar_lpips_pack_weights: NULL weights"); return 1; }
    const WLayout L = wlayout();
    if (!packed || packed_bytes < L.total * sizeof(float) || ((uintptr_t)packed & (ALIGN - 1))) {
        set_error("soar_lpips_pack_weights: packed must be %zu bytes, 256-byte aligned (got %zu)", L.total * sizeof(float), packed_bytes);
        return 1;
    }
    for (int i = 0; i < NL; i++)
        if (!w->conv_w[i] || !w->conv_b[i]) { set_error("soar_lpips_pack_weights: NULL conv weight / bias of layer %d", i); return 1; }
    for (int t = 0; t < NT; t++)
        if (!w->lin[t]) { set_error("soar_lpips_pack_weights: NULL lin%d", t); return 1; }
    if (!w->shift || !w->scale) { set_error("soar_lpips_pack_weights: NULL shift / scale"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *P = static_cast<float *>(packed);
    for (int i = 0; i < NL; i++) {
        const size_t n = (size_t)COUT[i] * CIN[i] * 9;
        if (i == 0) {
            SOAR_HIP_OK(hipMemcpyAsync(P + L.fwd[0], w->conv_w[0], n * sizeof(float), hipMemcpyDeviceToDevice, stream));
        } else if (launch_conv_pack(w->conv_w[i], P + L.fwd[i], P + L.bwd[i], COUT[i], CIN[i], 9, COUT[i], stream)) {
            return 1;
        }
        SOAR_HIP_OK(hipMemcpyAsync(P + L.bias[i], w->conv_b[i], COUT[i] * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    for (int t = 0; t < NT; t++)
        SOAR_HIP_OK(hipMemcpyAsync(P + L.lin[t], w->lin[t], TAP_C[t] * sizeof(float), hipMemcpyDeviceToDevice, stream));
    SOAR_HIP_OK(hipMemcpyAsync(P + L.shift, w->shift, 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    SOAR_HIP_OK(hipMemcpyAsync(P + L.scale, w->scale, 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

extern "C" int soar_lpips_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t grads, size_t *bytes)
{
    if (!bytes) { set_error("soar_lpips_workspace_bytes: NULL bytes"); return 1; }
    if (!check_size("soar_lpips_workspace_bytes", N, H, W)) return 1;
    if (grads < 0 || grads > 3) { set_error("soar_lpips_workspace_bytes: grads is a bitmask of 1 (in0) and 2 (in1) (got %d)", grads); return 1; }
    *bytes = ws_layout(dims_of(N, H, W), grads).total;
    return 0;
}

extern "C" int soar_lpips_forward(const SoarLpipsArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_args("soar_lpips_forward", a, workspace, workspace_bytes)) return 1;
    if (a->N == 0) return 0;
    if (!a->out) { set_error("soar_lpips_forward: NULL out"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Dims d = dims_of(a->N, a->H, a->W);
    const WsLayout L = ws_layout(d, a->grads);
    const WLayout WL = wlayout();
    const float *P = static_cast<const float *>(a->weights);
    char *ws = static_cast<char *>(workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    auto out_of = [&](int b, int i) { return (a->grads & (1 << b)) ? F(L.act[b][i]) : F(L.ping[b][i & 1]); };
    const float *in[2] = {a->in0, a->in1};
    const int64_t *ins[2] = {a->in0_stride, a->in1_stride};

    // layer by layer, both branches, so that a branch that is not kept needs its last two layers only; the head right after a tap
    for (int i = 0; i < NL; i++) {
        const int lev = LEVEL[i];
        for (int b = 0; b < 2; b++) {
            if (i == 0) {
                FirstK k{};
                k.x = in[b];
                for (int j = 0; j < 4; j++) k.xs[j] = ins[b][j];
                k.w = P + WL.fwd[0]; k.bias = P + WL.bias[0]; k.shift = P + WL.shift; k.scale = P + WL.scale;
                k.y = out_of(b, 0);
                k.npix = d.pix(0); k.H = d.H[0]; k.W = d.W[0];
                hipLaunchKernelGGL(lpips_first_kernel, dim3(blocks(k.npix * 16)), dim3(256), 0, stream, k);
                SOAR_LAUNCH_OK("lpips_first", stream, 0);
                continue;
            }
            const float *x = out_of(b, i - 1);
            if (pool_before(i)) {
                PoolK pk{};
                pk.x = x; pk.y = F(L.pool);
                pk.H = d.H[lev - 1]; pk.W = d.W[lev - 1]; pk.Ho = d.H[lev]; pk.Wo = d.W[lev]; pk.C = CIN[i];
                pk.n4 = d.pix(lev) * CIN[i] / 4;
                hipLaunchKernelGGL(lpips_pool_kernel, dim3(blocks(pk.n4)), dim3(256), 0, stream, pk);
                SOAR_LAUNCH_OK("lpips_pool", stream, 0);
                x = F(L.pool);
            }
            ConvK k{};
            k.x = x; k.w = P + WL.fwd[i]; k.bias = P + WL.bias[i]; k.y = out_of(b, i);
            k.M = d.pix(lev); k.H = d.H[lev]; k.W = d.W[lev]; k.Cin = CIN[i]; k.Cout = COUT[i]; k.epi = EPI_BIAS_RELU;
            if (launch_conv(k, stream)) return 1;
        }
        const int t = tap_of_layer(i);
        if (t < 0) continue;
        HeadK hk{};
        hk.f0 = out_of(0, i); hk.f1 = out_of(1, i); hk.w = P + WL.lin[t];
        hk.s = F(L.s[t]);
        hk.g0 = (a->grads & 1) ? F(L.gtap[0][t]) : nullptr;
        hk.g1 = (a->grads & 2) ? F(L.gtap[1][t]) : nullptr;
        hk.npix = d.pix(lev); hk.C = TAP_C[t];
        hk.inv_hw = 1.f / (float)((int64_t)d.H[lev] * d.W[lev]);
        const dim3 g((unsigned)((hk.npix + 3) / 4));
        switch (hk.C) {
        case 64: hipLaunchKernelGGL(lpips_head_kernel<1>, g, dim3(256), 0, stream, hk); break;
        case 128: hipLaunchKernelGGL(lpips_head_kernel<2>, g, dim3(256), 0, stream, hk); break;
        case 256: hipLaunchKernelGGL(lpips_head_kernel<4>, g, dim3(256), 0, stream, hk); break;
        default: hipLaunchKernelGGL(lpips_head_kernel<8>, g, dim3(256), 0, stream, hk); break;
        }
        SOAR_LAUNCH_OK("lpips_head", stream, 0);
    }
    SumK sk{};
    for (int t = 0; t < NT; t++) {
        sk.s[t] = F(L.s[t]);
        const int lev = LEVEL[TAP_LAYER[t]];
        sk.hw[t] = (int64_t)d.H[lev] * d.W[lev];
    }
    sk.out = a->out;
    hipLaunchKernelGGL(lpips_sum_kernel, dim3((unsigned)a->N), dim3(SUM_THREADS), 0, stream, sk);
    SOAR_LAUNCH_OK("lpips_sum", stream, 0);
    return 0;
}

extern "C" int soar_lpips_backward(const SoarLpipsArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_args("soar_lpips_backward", a, workspace, workspace_bytes)) return 1;
    if ((a->g_in0 && !(a->grads & 1)) || (a->g_in1 && !(a->grads & 2))) {
        set_error("soar_lpips_backward: a gradient was asked of a branch the forward did not keep (grads=%d)", a->grads);
        return 1;
    }
    if (a->N == 0) return 0;
    if ((a->g_in0 || a->g_in1) && !a->g_out) { set_error("soar_lpips_backward: NULL g_out"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Dims d = dims_of(a->N, a->H, a->W);
    const WsLayout L = ws_layout(d, a->grads);
    const WLayout WL = wlayout();
    const float *P = static_cast<const float *>(a->weights);
    char *ws = static_cast<char *>(workspace);
    auto F = [&](size_t off) { return reinterpret_cast<float *>(ws + off); };
    float *gin[2] = {a->g_in0, a->g_in1};
    const int64_t *gs[2] = {a->g_in0_stride, a->g_in1_stride};

    for (int b = 0; b < 2; b++) {
        if (!gin[b]) continue;
        float *G = F(L.gbuf[0]), *Gn = F(L.gbuf[1]);
        // the gradient of tap layer i's output (pool routing from glow, the tap's plane, the ReLU mask) into dst
        auto gate = [&](const float *glow, int i, float *dst) -> int {
            const int lev = LEVEL[i], t = tap_of_layer(i);
            GateK gk{};
            gk.glow = glow; gk.act = F(L.act[b][i]); gk.gtap = F(L.gtap[b][t]); gk.g_out = a->g_out; gk.g = dst;
            gk.H = d.H[lev]; gk.W = d.W[lev]; gk.C = COUT[i];
            gk.Ho = lev < 4 ? d.H[lev + 1] : 0; gk.Wo = lev < 4 ? d.W[lev + 1] : 0;
            gk.n4 = d.pix(lev) * COUT[i] / 4;
            hipLaunchKernelGGL(lpips_gate_kernel, dim3(blocks(gk.n4)), dim3(256), 0, stream, gk);
            SOAR_LAUNCH_OK("lpips_gate", stream, 0);
            return 0;
        };
        if (gate(nullptr, NL - 1, G)) return 1;
        for (int i = NL - 1; i >= 1; i--) {
            const int lev = LEVEL[i];
            ConvK k{};
            k.x = G; k.w = P + WL.bwd[i]; k.y = Gn;
            k.M = d.pix(lev); k.H = d.H[lev]; k.W = d.W[lev]; k.Cin = COUT[i]; k.Cout = CIN[i];
            if (pool_before(i)) {
                k.epi = EPI_PLAIN;
                if (launch_conv(k, stream)) return 1;
                if (gate(Gn, i - 1, G)) return 1;
            } else {
                k.epi = EPI_MASK;
                k.mask = F(L.act[b][i - 1]);
                if (launch_conv(k, stream)) return 1;
                float *t = G; G = Gn; Gn = t;
            }
        }
        FirstK fk{};
        fk.w = P + WL.fwd[0]; fk.scale = P + WL.scale;
        fk.gpre = G; fk.g = gin[b];
        for (int j = 0; j < 4; j++) fk.gs[j] = gs[b][j];
        fk.npix = d.pix(0); fk.H = d.H[0]; fk.W = d.W[0];
        hipLaunchKernelGGL(lpips_first_bwd_kernel, dim3(blocks(fk.npix)), dim3(256), 0, stream, fk);
        SOAR_LAUNCH_OK("lpips_first_bwd", stream, 0);
    }
    return 0;
}
