// geometry.hip -- the two per-surfel passes of the geometry model (soar_amd/geometry.py, the reference's "gaussiansurfel-base").
//
// 1. The five activations the renderer reads (TS/geometry/surfel_base.py:441-476 get_scaling / get_rotation / get_colors /
//    get_opacity / get_occ): normalize(_rotation), exp(_scaling), sigmoid(_opacity), sigmoid(_occ), sigmoid(_colors) -- five torch
//    launches forward and about fifteen backward per call in the reference, one launch each way here.
// 2. The per-surfel regularizers of training_step (TS/system/gaussian_surfel_mvdream.py:257-296): lambda_position, lambda_delta,
//    lambda_opacity, lambda_sparsity, lambda_scales -- values and gradients from one pass over the rows, the sums as per-workgroup
//    partial sums in double that a second, one-workgroup launch adds in a fixed order (bitwise reproducible, no float atomics).
//
// Both are memory-bound streams of about 100 bytes per surfel: one thread per surfel, wave64, no LDS beyond the block reduction.
#include "workspace.h"

#include <cmath>
#include <cstdint>

namespace soar {

namespace {

constexpr int GEO_BLOCK = 256;
constexpr float NORMALIZE_EPS = 1e-12f;       // F.normalize's eps

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

struct ActArgs {
    int P, S;
    const float *rotation, *scaling, *opacity, *occ, *colors;                     // raw leaves
    float *rotation_out, *scaling_out, *opacity_out, *occ_out, *colors_out;       // activated (saved for the backward)
    const float *g_rotation, *g_scaling, *g_opacity, *g_occ, *g_colors;           // gradients of the outputs (NULL = zero)
    float *d_rotation, *d_scaling, *d_opacity, *d_occ, *d_colors;                 // gradients of the leaves
};

__global__ void __launch_bounds__(GEO_BLOCK) activations_forward_kernel(ActArgs a)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= (size_t)a.P) return;
    if (a.rotation) {
        const float x = a.rotation[4 * i], y = a.rotation[4 * i + 1], z = a.rotation[4 * i + 2], w = a.rotation[4 * i + 3];
        // torch: x / max(|x|_2, eps)
        const float n = fmaxf(sqrtf(x * x + y * y + z * z + w * w), NORMALIZE_EPS);
        a.rotation_out[4 * i] = x / n;
        a.rotation_out[4 * i + 1] = y / n;
        a.rotation_out[4 * i + 2] = z / n;
        a.rotation_out[4 * i + 3] = w / n;
    }
    if (a.scaling)
        for (int k = 0; k < a.S; k++) a.scaling_out[(size_t)a.S * i + k] = expf(a.scaling[(size_t)a.S * i + k]);
    if (a.opacity) a.opacity_out[i] = sigmoidf(a.opacity[i]);
    if (a.occ) a.occ_out[i] = sigmoidf(a.occ[i]);
    if (a.colors)
        for (int k = 0; k < 3; k++) a.colors_out[3 * i + k] = sigmoidf(a.colors[3 * i + k]);
}

__global__ void __launch_bounds__(GEO_BLOCK) activations_backward_kernel(ActArgs a)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    if (i >= (size_t)a.P) return;
    if (a.d_rotation) {
        float d[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.g_rotation) {
            // y = x / c, c = max(n, eps): dx = g / c - [n >= eps] (g . y) x / (n c)  (division, clamp_min, norm backward of torch; the
            // norm's gradient at the zero vector is zero).  n is one square root of the leaf; y is the saved output.
            float x[4], y[4], g[4];
            for (int k = 0; k < 4; k++) { x[k] = a.rotation[4 * i + k]; y[k] = a.rotation_out[4 * i + k]; g[k] = a.g_rotation[4 * i + k]; }
            const float n = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
            const float c = fmaxf(n, NORMALIZE_EPS);
            const float gy = g[0] * y[0] + g[1] * y[1] + g[2] * y[2] + g[3] * y[3];
            const bool through = n >= NORMALIZE_EPS;
            for (int k = 0; k < 4; k++) d[k] = through ? (g[k] - gy * y[k]) / c : g[k] / c;
        }
        for (int k = 0; k < 4; k++) a.d_rotation[4 * i + k] = d[k];
    }
    if (a.d_scaling)
        for (int k = 0; k < a.S; k++) {
            const size_t j = (size_t)a.S * i + k;
            a.d_scaling[j] = a.g_scaling ? a.g_scaling[j] * a.scaling_out[j] : 0.f;
        }
    auto dsig = [](float g, float y) { return g * ((1.f - y) * y); };
    if (a.d_opacity) a.d_opacity[i] = a.g_opacity ? dsig(a.g_opacity[i], a.opacity_out[i]) : 0.f;
    if (a.d_occ) a.d_occ[i] = a.g_occ ? dsig(a.g_occ[i], a.occ_out[i]) : 0.f;
    if (a.d_colors)
        for (int k = 0; k < 3; k++) a.d_colors[3 * i + k] = a.g_colors ? dsig(a.g_colors[3 * i + k], a.colors_out[3 * i + k]) : 0.f;
}

// ---- regularizers ---------------------------------------------------------------------------------------------------------
constexpr int REG_TERMS = 5;       // position, delta, opacity, sparsity, scales

struct RegArgs {
    int P, S, K;
    const float *xyz, *original_pos, *scaling, *opacity, *scales;
    const float *coef;             // [5] device
    const float *upstream;         // device scalar or NULL (= 1)
    float *g_xyz, *g_opacity, *g_scales;
    double *partials;              // [blocks][5]
};

__global__ void __launch_bounds__(GEO_BLOCK) regularizers_kernel(RegArgs a)
{
#pragma clang fp contract(off)
    __shared__ double red[REG_TERMS][GEO_BLOCK];
    const size_t i = (size_t)blockIdx.x * GEO_BLOCK + threadIdx.x;
    const float up = a.upstream ? a.upstream[0] : 1.f;
    float c[REG_TERMS];
    for (int t = 0; t < REG_TERMS; t++) c[t] = a.coef[t];
    double v[REG_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < (size_t)a.P) {
        const float fP = (float)a.P;
        float gx[3] = {0.f, 0.f, 0.f};
        float p[3] = {0.f, 0.f, 0.f};
        if (a.xyz && (c[0] != 0.f || c[1] != 0.f))
            for (int k = 0; k < 3; k++) p[k] = a.xyz[3 * i + k];
        if (c[0] != 0.f && a.xyz) {                                     // mean(|xyz|_2)
            const float n = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
            v[0] = (double)n;
            if (!(n == 0.f))                                            // a NaN row keeps its NaN, as in torch
                for (int k = 0; k < 3; k++) gx[k] += ((c[0] * up) / fP) * (p[k] / n);
        }
        if (c[1] != 0.f && a.xyz && a.original_pos) {                   // mean(|xyz - original_pos|_2): zero gradient at a zero vector
            float d[3];
            for (int k = 0; k < 3; k++) d[k] = p[k] - a.original_pos[3 * i + k];
            const float n = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            v[1] = (double)n;
            if (!(n == 0.f))
                for (int k = 0; k < 3; k++) gx[k] += ((c[1] * up) / fP) * (d[k] / n);
        }
        if (a.g_xyz)
            for (int k = 0; k < 3; k++) a.g_xyz[3 * i + k] = gx[k];
        float go = 0.f;
        if ((c[2] != 0.f || c[3] != 0.f) && a.opacity) {
            const float o = a.opacity[i];
            if (c[2] != 0.f && a.scaling) {                             // sum(|scaling|_2.detach() * opacity): no gradient to scaling
                float s2 = 0.f;
                for (int k = 0; k < a.S; k++) { const float s = a.scaling[(size_t)a.S * i + k]; s2 += s * s; }
                const float sn = sqrtf(s2);
                v[2] = (double)(sn * o);
                go += (c[2] * up) * sn;
            }
            if (c[3] != 0.f) {                                          // -mean((opacity - 0.5)^2)
                const float e = o - 0.5f;
                v[3] = -(double)(e * e);
                go += ((c[3] * up) / fP) * (-2.f * e);
            }
        }
        if (a.g_opacity) a.g_opacity[i] = go;
        if (a.scales && c[4] != 0.f) {                                  // mean(scales)
            double s = 0.0;
            for (int k = 0; k < a.K; k++) s += (double)a.scales[(size_t)a.K * i + k];
            v[4] = s;
        }
        if (a.g_scales) {
            const float gs = (a.scales && c[4] != 0.f) ? (c[4] * up) / ((float)a.P * (float)a.K) : 0.f;
            for (int k = 0; k < a.K; k++) a.g_scales[(size_t)a.K * i + k] = gs;
        }
    }
    for (int t = 0; t < REG_TERMS; t++) red[t][threadIdx.x] = v[t];
    __syncthreads();
    for (int s = GEO_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int t = 0; t < REG_TERMS; t++) red[t][threadIdx.x] += red[t][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < REG_TERMS) a.partials[(size_t)blockIdx.x * REG_TERMS + threadIdx.x] = red[threadIdx.x][0];
}

// one workgroup: thread t adds the partial sums of the blocks t, t + 256, ... in that order, then the same tree
__global__ void __launch_bounds__(GEO_BLOCK) regularizers_finish_kernel(int P, int K, int blocks, const double *__restrict__ partials,
                                                                        const float *__restrict__ coef, float *__restrict__ terms)
{
    __shared__ double red[REG_TERMS][GEO_BLOCK];
    double v[REG_TERMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < blocks; b += GEO_BLOCK)
        for (int t = 0; t < REG_TERMS; t++) v[t] += partials[(size_t)b * REG_TERMS + t];
    for (int t = 0; t < REG_TERMS; t++) red[t][threadIdx.x] = v[t];
    __syncthreads();
    for (int s = GEO_BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int t = 0; t < REG_TERMS; t++) red[t][threadIdx.x] += red[t][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = (double)P;
        const double div[REG_TERMS] = {n, n, 1.0, n, n * (double)K};
        double total = 0.0;
        for (int t = 0; t < REG_TERMS; t++) {
            const float c = coef[t];
            const float value = c != 0.f ? (float)(red[t][0] / div[t]) : 0.f;       // a term whose coefficient is zero is skipped
            terms[t] = value;
            if (c != 0.f) total += (double)c * (double)value;
        }
        terms[REG_TERMS] = (float)total;
    }
}

inline int reg_blocks(int P) { return (int)(((int64_t)P + GEO_BLOCK - 1) / GEO_BLOCK); }

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_surfel_activations_forward(int32_t P, int32_t S, const float *rotation, const float *scaling, const float *opacity,
                                               const float *occ, const float *colors, float *rotation_out, float *scaling_out,
                                               float *opacity_out, float *occ_out, float *colors_out, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (P < 0 || S < 1 || S > 3) {
        set_error("soar_surfel_activations_forward: bad arguments (P=%d >= 0, S=%d in 1..3)", P, S);
        return 1;
    }
    if (P == 0) return 0;
    if ((rotation && !rotation_out) || (scaling && !scaling_out) || (opacity && !opacity_out) || (occ && !occ_out) || (colors && !colors_out)) {
        set_error("soar_surfel_activations_forward: an input is given without its output (NULL)");
        return 1;
    }
    ActArgs a = {};
    a.P = P; a.S = S;
    a.rotation = rotation; a.scaling = scaling; a.opacity = opacity; a.occ = occ; a.colors = colors;
    a.rotation_out = rotation_out; a.scaling_out = scaling_out; a.opacity_out = opacity_out; a.occ_out = occ_out; a.colors_out = colors_out;
    hipLaunchKernelGGL(activations_forward_kernel, dim3((unsigned)reg_blocks(P)), dim3(GEO_BLOCK), 0, stream, a);
    SOAR_LAUNCH_OK("surfel_activations_forward", stream, 0);
    return 0;
}

extern "C" int soar_surfel_activations_backward(int32_t P, int32_t S, const float *rotation, const float *rotation_out, const float *scaling_out,
                                                const float *opacity_out, const float *occ_out, const float *colors_out,
                                                const float *g_rotation, const float *g_scaling, const float *g_opacity, const float *g_occ,
                                                const float *g_colors, float *d_rotation, float *d_scaling, float *d_opacity, float *d_occ,
                                                float *d_colors, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (P < 0 || S < 1 || S > 3) {
        set_error("soar_surfel_activations_backward: bad arguments (P=%d >= 0, S=%d in 1..3)", P, S);
        return 1;
    }
    if (P == 0) return 0;
    if ((d_rotation && g_rotation && (!rotation || !rotation_out)) || (d_scaling && g_scaling && !scaling_out) ||
        (d_opacity && g_opacity && !opacity_out) || (d_occ && g_occ && !occ_out) || (d_colors && g_colors && !colors_out)) {
        set_error("soar_surfel_activations_backward: a gradient is asked for without the saved output it needs (NULL)");
        return 1;
    }
    ActArgs a = {};
    a.P = P; a.S = S;
    a.rotation = rotation;
    a.rotation_out = const_cast<float *>(rotation_out); a.scaling_out = const_cast<float *>(scaling_out);
    a.opacity_out = const_cast<float *>(opacity_out); a.occ_out = const_cast<float *>(occ_out); a.colors_out = const_cast<float *>(colors_out);
    a.g_rotation = g_rotation; a.g_scaling = g_scaling; a.g_opacity = g_opacity; a.g_occ = g_occ; a.g_colors = g_colors;
    a.d_rotation = d_rotation; a.d_scaling = d_scaling; a.d_opacity = d_opacity; a.d_occ = d_occ; a.d_colors = d_colors;
    hipLaunchKernelGGL(activations_backward_kernel, dim3((unsigned)reg_blocks(P)), dim3(GEO_BLOCK), 0, stream, a);
    SOAR_LAUNCH_OK("surfel_activations_backward", stream, 0);
    return 0;
}

extern "C" int soar_surfel_regularizers_workspace_bytes(int32_t P, size_t *bytes)
{
    if (P < 0 || !bytes) {
        set_error("soar_surfel_regularizers_workspace_bytes: bad arguments (P=%d >= 0, bytes must be given)", P);
        return 1;
    }
    *bytes = align_up((size_t)reg_blocks(P) * REG_TERMS * sizeof(double));
    return 0;
}

extern "C" int soar_surfel_regularizers(int32_t P, int32_t S, int32_t K, const float *xyz, const float *original_pos, const float *scaling,
                                        const float *opacity, const float *scales, const float *coef_dev, const float *upstream_dev,
                                        float *terms_dev, float *g_xyz, float *g_opacity, float *g_scales, void *workspace,
                                        size_t workspace_bytes, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (P < 0 || S < 1 || S > 3 || K < 1 || K > 3 || !coef_dev || !terms_dev) {
        set_error("soar_surfel_regularizers: bad arguments (P=%d >= 0, S=%d and K=%d in 1..3, coefficients and terms must be given)", P, S, K);
        return 1;
    }
    if (P == 0) return 0;
    size_t need = 0;
    soar_surfel_regularizers_workspace_bytes(P, &need);
    // one block of doubles: 8-byte alignment is all it needs
    if (!workspace_ok("soar_surfel_regularizers", workspace, workspace_bytes, need, "soar_surfel_regularizers_workspace_bytes", 8)) return 1;
    RegArgs a = {};
    a.P = P; a.S = S; a.K = K;
    a.xyz = xyz; a.original_pos = original_pos; a.scaling = scaling; a.opacity = opacity; a.scales = scales;
    a.coef = coef_dev; a.upstream = upstream_dev;
    a.g_xyz = g_xyz; a.g_opacity = g_opacity; a.g_scales = g_scales;
    a.partials = static_cast<double *>(workspace);
    const int blocks = reg_blocks(P);
    hipLaunchKernelGGL(regularizers_kernel, dim3((unsigned)blocks), dim3(GEO_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(regularizers_finish_kernel, dim3(1), dim3(GEO_BLOCK), 0, stream, P, K, blocks, (const double *)a.partials, coef_dev,
                       terms_dev);
    SOAR_LAUNCH_OK("surfel_regularizers", stream, 0);
    return 0;
}
