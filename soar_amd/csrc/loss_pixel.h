// loss_pixel.h -- what image_losses.hip and step_terms.hip share: the cosine loss's per-pixel arithmetic, the 1- / 4-pixel load
// helpers and the two-stage {sum, count} reduction.  The kernels of both files leave the same bits for the same pixels: the
// selection cos < cos(thrsh) sits on a rounding, so the expressions live here once.
#pragma once

#include "soar_common.h"

#include <cstdint>

namespace soar {

// ---- the cosine term: o = 2 output - 1, g = 2 gt - 1, cos = sum_c o_c g_c weight (TS/system/gaussian_surfel_mvdream.py:622-630) ----
// Every rounding is written out, so the bits depend neither on the flags of the file that includes this nor on what the compiler
// would choose to fuse in a given kernel: t = round(o g), cs = round(t weight + cs) -- the product's last factor fuses with the
// running sum, which is what image_losses.hip has always computed.  (x * 2 is exact: 2 x - 1 rounds once with or without an FMA.)
__device__ __forceinline__ void cos_accumulate(float &cs, float x, float y, float weight)
{
#pragma clang fp contract(off)
    const float o = __builtin_fmaf(x, 2.f, -1.f), g = __builtin_fmaf(y, 2.f, -1.f);      // (= round(2 x - 1): 2 x is exact)
    const float t = __fmul_rn(o, g);
    cs = __builtin_fmaf(t, weight, cs);
}
// d (1 - cos) / d output_c = -2 weight (2 gt_c - 1), times upstream / count: three products, each rounded
__device__ __forceinline__ float cos_grad_value(float weight, float y, float scale)
{
#pragma clang fp contract(off)
    const float g = __builtin_fmaf(y, 2.f, -1.f);
    return __fmul_rn(__fmul_rn(-2.f * weight, g), scale);
}

// V = 4: four consecutive pixels per thread and trip through 16-byte loads / stores (pixel count a multiple of 4, planes 16-byte
// aligned: every image of the path); V = 1: any size
template <int V> struct PixVec;
template <> struct PixVec<4> { typedef float4 F; typedef uchar4 M; };
template <> struct PixVec<1> { typedef float F; typedef uint8_t M; };
__device__ __forceinline__ void unpack(const float4 &v, float (&o)[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ void unpack(const float &v, float (&o)[1]) { o[0] = v; }
__device__ __forceinline__ void unpack(const uchar4 &v, bool (&o)[4]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
__device__ __forceinline__ void unpack(const uint8_t &v, bool (&o)[1]) { o[0] = v; }
__device__ __forceinline__ float4 pack(const float (&o)[4]) { return make_float4(o[0], o[1], o[2], o[3]); }
__device__ __forceinline__ float pack(const float (&o)[1]) { return o[0]; }

// a workgroup of 256 threads leaves its {sum, count}: butterfly over the wavefront, then (w0 + w1) + (w2 + w3).  (One use per
// kernel, or a __syncthreads() between two: the four rows of LDS are the function's own.)
__device__ __forceinline__ void block_sum2(float s, float c, float *partials)
{
    __shared__ float red[4][2];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); c += __shfl_xor(c, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        partials[2 * blockIdx.x + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
}

// one workgroup of 256 threads folds the workgroups' pairs: stats = {sum / (count * per), count}; an empty selection gives NaN like
// the reference's mean of an empty tensor
__device__ __forceinline__ void mean_finish_block(const float *partials, int nblocks, float per, float *stats)
{
    __shared__ float red[4][2];
    float s = 0.f, c = 0.f;
    for (int k = threadIdx.x; k < nblocks; k += 256) { s += partials[2 * k]; c += partials[2 * k + 1]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); c += __shfl_xor(c, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float st = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]), ct = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        stats[0] = st / (ct * per);
        stats[1] = ct;
    }
}

constexpr int LOSS_BLOCKS = 1024;          // workgroups of a loss walk at the most (= pairs of partial sums per term)

}  // namespace soar
