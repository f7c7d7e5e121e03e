// pose_common.h -- what the keypoint networks share (pose.hip: the body; pose_parts.hip: hands and face): the weight packer that moves
// runs of input channels to where a padded activation row holds them, the small layer kernels round the shared convolution
// (conv_gemm.hip), and the bicubic x8 upsampling rule of the heat maps.  Everything sits in an anonymous namespace: each translation
// unit has its own copy, compiled under its own flags (both with -ffp-contract=off).
#pragma once

#include "conv_gemm.h"

namespace soar {

namespace {

constexpr int IMGP = 8;                         // the image's three channels, padded to a multiple of 8

struct Seg { int dst, src, len; };              // input channels src .. src + len of the tensor lie at dst .. of the packed row

// ---- weight packing ----
struct PackK {
    const float *w;
    float *out;
    int cin, cout, kk, cinp, nseg;
    Seg seg[3];
    int64_t n;
};
#if defined(__HIPCC__)
__global__ void __launch_bounds__(256) pose_pack_kernel(PackK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.n) return;
    // e walks the packed layout [co][t][cip]
    const int cip = (int)(e % k.cinp);
    const int64_t r = e / k.cinp;
    const int t = (int)(r % k.kk), co = (int)(r / k.kk);
    int ci = -1;
    for (int s = 0; s < k.nseg; s++)
        if (cip >= k.seg[s].dst && cip < k.seg[s].dst + k.seg[s].len) ci = k.seg[s].src + (cip - k.seg[s].dst);
    k.out[e] = co < k.cout && ci >= 0 ? k.w[((size_t)co * k.cin + ci) * k.kk + t] : 0.f;
}
// [cout] -> [coutp], zeros behind
__global__ void __launch_bounds__(256) pose_pad_kernel(const float *src, float *dst, int cout, int coutp)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < coutp) dst[e] = e < cout ? src[e] : 0.f;
}

// ---- small layer kernels ----
struct IngestK {
    const float *x;
    int64_t xs[4];
    float *y;
    int64_t npix;
    int H, W;
};
// the caller's strided [B][3][H][W] -> NHWC rows of 8 floats (3 values, 5 zeros)
__global__ void __launch_bounds__(256) pose_ingest_kernel(IngestK k)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= k.npix) return;
    const int64_t hw = (int64_t)k.H * k.W, n = p / hw;
    const int q = (int)(p - n * hw), y = q / k.W, x = q - y * k.W;
    const float *s = k.x + n * k.xs[0] + y * k.xs[2] + x * k.xs[3];
    float4 *dst = reinterpret_cast<float4 *>(k.y + (size_t)p * IMGP);
    dst[0] = make_float4(s[0], s[k.xs[1]], s[2 * k.xs[1]], 0.f);
    dst[1] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// x [N][H][W][C] -> y [N][H/2][W/2][C]; thread = (output pixel, channel quad)
__global__ void __launch_bounds__(256) pose_pool_kernel(const float *x, float *y, int64_t n4, int H, int W, int C)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const int c4 = C / 4, cq = (int)(e % c4);
    const int64_t p = e / c4;
    const int Wo = W / 2, Ho = H / 2;
    const int ox = (int)(p % Wo);
    const int64_t r = p / Wo;
    const int oy = (int)(r % Ho);
    const int64_t n = r / Ho;
    const float4 *s = reinterpret_cast<const float4 *>(x + ((size_t)(n * H + 2 * oy) * W + 2 * ox) * C) + cq;
    const float4 a = s[0], b = s[c4], c = s[(size_t)W * c4], d = s[(size_t)W * c4 + c4];
    float4 o;
    o.x = fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x));
    o.y = fmaxf(fmaxf(a.y, b.y), fmaxf(c.y, d.y));
    o.z = fmaxf(fmaxf(a.z, b.z), fmaxf(c.z, d.z));
    o.w = fmaxf(fmaxf(a.w, b.w), fmaxf(c.w, d.w));
    reinterpret_cast<float4 *>(y)[e] = o;
}
// channels off .. off + C of rows ld apart -> dense [rows][C]
__global__ void __launch_bounds__(256) pose_slice_kernel(const float *x, int64_t ld, int off, int C, float *y, int64_t n)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    y[e] = x[(e / C) * ld + off + (int)(e % C)];
}

// ---- the heat maps' upsampling by 8: bicubic, a = -0.75 ----
// source sample of upsampled coordinate Y: (Y + 0.5) / 8 - 0.5 = i + t with i = floor((2 Y - 7) / 16) and t = (2 ph + 1) / 16,
// ph = ((2 Y - 7) mod 16) / 2: eight phases
__device__ __forceinline__ int up_cell(int Y) { return (2 * Y - 7) >> 4; }
__device__ __forceinline__ int up_phase(int Y) { return ((2 * Y - 7) & 15) >> 1; }
// the four weights of phase ph, for the cells i - 1 .. i + 2
__device__ __forceinline__ void up_weights(int ph, float *wt)
{
    const float a = -0.75f, t = (float)(2 * ph + 1) / 16.f, t1 = t + 1.f, u = 1.f - t;
    const float w0 = ((a * t1 - 5.f * a) * t1 + 8.f * a) * t1 - 4.f * a;
    const float w1 = ((a + 2.f) * t - (a + 3.f)) * t * t + 1.f;
    const float w2 = ((a + 2.f) * u - (a + 3.f)) * u * u + 1.f;
    wt[0] = w0; wt[1] = w1; wt[2] = w2; wt[3] = 1.f - w0 - w1 - w2;
}
// four weighted samples, summed left to right: a row's four cells, then the four rows top to bottom
__device__ __forceinline__ float up_sum4(const float *w, float s0, float s1, float s2, float s3)
{
    return ((w[0] * s0 + w[1] * s1) + w[2] * s2) + w[3] * s3;
}
#endif

}  // namespace

}  // namespace soar
