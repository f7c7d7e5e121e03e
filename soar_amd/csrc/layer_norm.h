// layer_norm.h -- LayerNorm over rows, shared by the transformers (sam.hip, unet.hip, clip.hip).
#pragma once

#include "conv_gemm.h"

namespace soar {
namespace {

// ---- LayerNorm over rows of C floats, a wave a row; act = ACT_GELU: GELU behind it.  y may be x: a lane rewrites what it read. -------
__global__ void __launch_bounds__(256) ln_rows_kernel(const float *x, const float *__restrict__ w, const float *__restrict__ bb,
                                                      float *y, int64_t rows, int C, float eps, int act)
{
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float *xr = x + row * C;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
    for (int d = 32; d; d >>= 1) s += __shfl_xor(s, d);
    const float mean = s / (float)C;
    float v = 0.f;
    for (int c = lane; c < C; c += 64) { const float t = xr[c] - mean; v += t * t; }
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    const float rstd = 1.f / sqrtf(v / (float)C + eps);
    for (int c = lane; c < C; c += 64) {
        float t = (xr[c] - mean) * rstd * w[c] + bb[c];
        if (act == ACT_GELU) t = gelu_erf(t);
        y[row * C + c] = t;
    }
}
int layer_norm(const float *x, const float *w, const float *b, float *y, int64_t rows, int C, float eps, int act, hipStream_t stream)
{
    if (rows == 0) return 0;
    hipLaunchKernelGGL(ln_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, x, w, b, y, rows, C, eps, act);
    SOAR_LAUNCH_OK("layer_norm", stream, 0);
    return 0;
}

}  // namespace
}  // namespace soar
