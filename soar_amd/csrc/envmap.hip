// envmap.hip -- the environment-map background (soar_amd/background.py): the reference's NeuralEnvironmentMapBackground
// ("gaussiandreamer-background") as tiny-cuda-nn's SphericalHarmonics (degree 3) and threestudio's VanillaMLP compute it
// (include/soar_hip.h).
//
//   envmap_forward_kernel  one thread per pixel: x = ((d + 1) / 2) * 2 - 1, the 9 SH values, 9 -> 16 -> 16 -> 3 without bias
//                          (weights in LDS, broadcast reads), sigmoid -> bg [B][H][W][3]; for the first n_comp rows also
//                          comp = r + (1 - m) * bg [n_comp][3][H][W].  With a constant colour (aug / eval) bg = color[row]
//                          and the MLP is skipped.
//   envmap_bwd_kernel      chunks of 128 pixels: a thread recomputes its pixel, forms g_mask = -sum_c g_c * bg_c and the
//                          layers' gradients, and leaves its pixel's factors in LDS; then thread (slice s, unit r) adds the
//                          28 products of unit r over the chunk's pixels s, s + 8, ... in double.  The 8 slices are added in
//                          order, one row of 448 doubles per workgroup (no atomics)
//   envmap_reduce_kernel   the rows summed in double in a fixed order (16 slices, then the slices in order)
//
// The whole file is compiled without contraction (build.py): comp is then rounded as torch's three separate operations, and
// the backward's recomputed bg is the forward's bg.  No host synchronisation, no allocation.
#include "workspace.h"

namespace soar {

namespace {

constexpr int ENC = SOAR_ENVMAP_ENC;          // 9 SH values (degree 3 = bands 0..2)
constexpr int HID = SOAR_ENVMAP_HIDDEN;       // 16
constexpr int OUT = 3;
constexpr int W1_OFF = 0;                     // w1 [16][9]
constexpr int W2_OFF = HID * ENC;             // w2 [16][16]
constexpr int W3_OFF = W2_OFF + HID * HID;    // w3 [3][16]
constexpr int NW = SOAR_ENVMAP_WEIGHTS;       // 448
static_assert(W3_OFF + OUT * HID == NW, "weight layout");
constexpr int64_t MAX_PIX = int64_t(1) << 30;
constexpr int FWD_BLOCK = 256;
constexpr int CHUNK = 128;                    // pixels per step of the backward = threads per workgroup
constexpr int SLICES = CHUNK / HID;           // 8: thread t sums unit t % 16 over the pixels t / 16 + 8 k of a chunk
constexpr int MAX_G = 1024;                   // workgroups of the backward (at most): partial rows

struct EnvK {
    int64_t npix, hw;                         // B * H * W, H * W
    int B, W, n_comp, color_rows;
    int64_t rs, ms;                           // render / mask image strides (elements)
    int64_t gs[4];                            // g_comp strides, NCHW order
    const float *dirs, *color, *render, *mask, *g_comp, *g_bg;
    const float *w1, *w2, *w3;
    float *bg, *comp, *g_mask;
    double *partial;                          // [G][448]
    int G, need_w;
    float *d_w1, *d_w2, *d_w3;
};

__device__ inline float env_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// tcnn's SphericalHarmonics, degree 3, of the component-wise round trip x = ((d + 1) / 2) * 2 - 1
__device__ inline void sh9(const float *d, float *e)
{
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float u = (d[c] + 1.f) / 2.f;
        v[c] = u * 2.f - 1.f;
    }
    const float x = v[0], y = v[1], z = v[2];
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    e[0] = 0.28209479177387814f;
    e[1] = -0.48860251190291987f * y;
    e[2] = 0.48860251190291987f * z;
    e[3] = -0.48860251190291987f * x;
    e[4] = 1.0925484305920792f * xy;
    e[5] = -1.0925484305920792f * yz;
    e[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    e[7] = -1.0925484305920792f * xz;
    e[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
}

// weights into LDS in the nn.Linear layouts, back to back
__device__ inline void load_weights(const EnvK &a, float *W)
{
    for (int e = threadIdx.x; e < NW; e += blockDim.x)
        W[e] = e < W2_OFF ? a.w1[e] : e < W3_OFF ? a.w2[e - W2_OFF] : a.w3[e - W3_OFF];
}

// the three layers: h1 = relu(w1 e), h2 = relu(w2 h1), z = w3 h2 (sums in input order, as one row of a matrix product)
__device__ inline void mlp(const float *W, const float *e, float *h1, float *h2, float *z)
{
#pragma unroll
    for (int i = 0; i < HID; i++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < ENC; k++) s += W[W1_OFF + i * ENC + k] * e[k];
        h1[i] = fmaxf(s, 0.f);
    }
#pragma unroll
    for (int j = 0; j < HID; j++) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < HID; i++) s += W[W2_OFF + j * HID + i] * h1[i];
        h2[j] = fmaxf(s, 0.f);
    }
#pragma unroll
    for (int o = 0; o < OUT; o++) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < HID; j++) s += W[W3_OFF + o * HID + j] * h2[j];
        z[o] = s;
    }
}

__device__ inline void const_color(const EnvK &a, int b, float *bg)
{
    const int r = a.color_rows == 1 ? 0 : b;
#pragma unroll
    for (int c = 0; c < OUT; c++) bg[c] = a.color[3 * r + c];
}

__global__ void __launch_bounds__(FWD_BLOCK) envmap_forward_kernel(EnvK a)
{
    __shared__ float W[NW];
    if (!a.color) {
        load_weights(a, W);
        __syncthreads();
    }
    const int64_t p = (int64_t)blockIdx.x * FWD_BLOCK + threadIdx.x;
    if (p >= a.npix) return;
    const int b = (int)(p / a.hw);
    const int64_t q = p - (int64_t)b * a.hw;
    float bg[OUT];
    if (a.color) {
        const_color(a, b, bg);
    } else {
        const float d[3] = {a.dirs[3 * p], a.dirs[3 * p + 1], a.dirs[3 * p + 2]};
        float e[ENC], h1[HID], h2[HID], z[OUT];
        sh9(d, e);
        mlp(W, e, h1, h2, z);
#pragma unroll
        for (int c = 0; c < OUT; c++) bg[c] = env_sigmoid(z[c]);
    }
#pragma unroll
    for (int c = 0; c < OUT; c++) a.bg[3 * p + c] = bg[c];
    if (b < a.n_comp) {
        const float om = 1.f - a.mask[(int64_t)b * a.ms + q];
#pragma unroll
        for (int c = 0; c < OUT; c++) {
            const float t = om * bg[c];
            a.comp[((int64_t)b * OUT + c) * a.hw + q] = a.render[(int64_t)b * a.rs + (int64_t)c * a.hw + q] + t;
        }
    }
}

// LDS of the backward: a chunk's per-pixel factors (phase 1), then the slices' sums (phase 2)
struct BwdFactors {
    float E[CHUNK][ENC + OUT];                // the SH values and dL/dz
    float H1[CHUNK][HID], H2[CHUNK][HID];     // layer outputs after ReLU
    float D1[CHUNK][HID], D2[CHUNK][HID];     // dL/d(pre-activation) of layers 1 and 2
};
union BwdLds {
    BwdFactors f;
    double sums[SLICES][NW];
};

__global__ void __launch_bounds__(CHUNK) envmap_bwd_kernel(EnvK a)
{
    __shared__ float W[NW];
    __shared__ BwdLds L;
    const bool mlp_on = a.color == nullptr;
    if (mlp_on) load_weights(a, W);
    __syncthreads();
    const int t = threadIdx.x;
    const int r = t % HID, s = t / HID;
    // the products of two floats are exact in double, and the sums of a workgroup's pixels do not drift with their order
    double acc1[ENC], acc2[HID], acc3[OUT];
#pragma unroll
    for (int k = 0; k < ENC; k++) acc1[k] = 0.0;
#pragma unroll
    for (int i = 0; i < HID; i++) acc2[i] = 0.0;
#pragma unroll
    for (int o = 0; o < OUT; o++) acc3[o] = 0.0;
    const int64_t chunks = (a.npix + CHUNK - 1) / CHUNK;
    for (int64_t c = blockIdx.x; c < chunks; c += a.G) {
        const int64_t p = c * CHUNK + t;
        float e[ENC], h1[HID], h2[HID], dz[OUT], d1[HID], d2[HID];
#pragma unroll
        for (int k = 0; k < ENC; k++) e[k] = 0.f;
#pragma unroll
        for (int i = 0; i < HID; i++) { h1[i] = 0.f; h2[i] = 0.f; d1[i] = 0.f; d2[i] = 0.f; }
#pragma unroll
        for (int o = 0; o < OUT; o++) dz[o] = 0.f;
        if (p < a.npix) {
            const int b = (int)(p / a.hw);
            const int64_t q = p - (int64_t)b * a.hw;
            float bg[OUT], z[OUT];
            if (mlp_on) {
                const float d[3] = {a.dirs[3 * p], a.dirs[3 * p + 1], a.dirs[3 * p + 2]};
                sh9(d, e);
                mlp(W, e, h1, h2, z);
#pragma unroll
                for (int o = 0; o < OUT; o++) bg[o] = env_sigmoid(z[o]);
            } else {
                const_color(a, b, bg);
            }
            float gbg[OUT] = {0.f, 0.f, 0.f};
            if (b < a.n_comp && a.g_comp) {
                const int64_t y = q / a.W, x = q - y * a.W;
                const float om = 1.f - a.mask[(int64_t)b * a.ms + q];
                float g[OUT];
#pragma unroll
                for (int o = 0; o < OUT; o++) {
                    g[o] = a.g_comp[b * a.gs[0] + o * a.gs[1] + y * a.gs[2] + x * a.gs[3]];
                    gbg[o] = om * g[o];
                }
                if (a.g_mask) a.g_mask[p] = -(g[0] * bg[0] + g[1] * bg[1] + g[2] * bg[2]);
            }
            if (a.g_bg)
#pragma unroll
                for (int o = 0; o < OUT; o++) gbg[o] += a.g_bg[3 * p + o];
            if (mlp_on && a.need_w) {
#pragma unroll
                for (int o = 0; o < OUT; o++) dz[o] = gbg[o] * (bg[o] * (1.f - bg[o]));
#pragma unroll
                for (int j = 0; j < HID; j++) {
                    float v = 0.f;
#pragma unroll
                    for (int o = 0; o < OUT; o++) v += W[W3_OFF + o * HID + j] * dz[o];
                    d2[j] = h2[j] > 0.f ? v : 0.f;
                }
#pragma unroll
                for (int i = 0; i < HID; i++) {
                    float v = 0.f;
#pragma unroll
                    for (int j = 0; j < HID; j++) v += W[W2_OFF + j * HID + i] * d2[j];
                    d1[i] = h1[i] > 0.f ? v : 0.f;
                }
            }
        }
        if (!a.need_w) continue;                      // (uniform: no barrier is skipped by part of the workgroup)
#pragma unroll
        for (int k = 0; k < ENC; k++) L.f.E[t][k] = e[k];
#pragma unroll
        for (int o = 0; o < OUT; o++) L.f.E[t][ENC + o] = dz[o];
#pragma unroll
        for (int i = 0; i < HID; i++) { L.f.H1[t][i] = h1[i]; L.f.H2[t][i] = h2[i]; L.f.D1[t][i] = d1[i]; L.f.D2[t][i] = d2[i]; }
        __syncthreads();
        for (int m = s; m < CHUNK; m += SLICES) {
            const double u1 = L.f.D1[m][r], u2 = L.f.D2[m][r], v3 = L.f.H2[m][r];
#pragma unroll
            for (int k = 0; k < ENC; k++) acc1[k] += u1 * (double)L.f.E[m][k];
#pragma unroll
            for (int i = 0; i < HID; i++) acc2[i] += u2 * (double)L.f.H1[m][i];
#pragma unroll
            for (int o = 0; o < OUT; o++) acc3[o] += (double)L.f.E[m][ENC + o] * v3;
        }
        __syncthreads();
    }
    if (!a.need_w) return;
    // the slices' sums in the partial row's layout (dw1 [16][9], dw2 [16][16], dw3 [3][16]), added in slice order
#pragma unroll
    for (int k = 0; k < ENC; k++) L.sums[s][W1_OFF + r * ENC + k] = acc1[k];
#pragma unroll
    for (int i = 0; i < HID; i++) L.sums[s][W2_OFF + r * HID + i] = acc2[i];
#pragma unroll
    for (int o = 0; o < OUT; o++) L.sums[s][W3_OFF + o * HID + r] = acc3[o];
    __syncthreads();
    double *row = a.partial + (size_t)blockIdx.x * NW;
    for (int e = t; e < NW; e += CHUNK) {
        double v = 0.0;
        for (int q = 0; q < SLICES; q++) v += L.sums[q][e];
        row[e] = v;
    }
}

// grid ceil(448 / 64), 1024 threads: wave w sums the rows [w * G / 16, (w + 1) * G / 16), wave 0 adds the 16 slices in order
constexpr int RED_WAVES = 16;
__global__ void __launch_bounds__(RED_WAVES * 64) envmap_reduce_kernel(EnvK a)
{
    __shared__ double part[RED_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const int g0 = (int)((int64_t)a.G * w / RED_WAVES), g1 = (int)((int64_t)a.G * (w + 1) / RED_WAVES);
    double s = 0.0;
    if (e < NW) {
#pragma unroll 8
        for (int gi = g0; gi < g1; gi++) s += a.partial[(size_t)gi * NW + e];
    }
    part[w][lane] = s;
    __syncthreads();
    if (w != 0 || e >= NW) return;
    double v = part[0][lane];
    for (int q = 1; q < RED_WAVES; q++) v += part[q][lane];
    float *dst = e < W2_OFF ? a.d_w1 + e : e < W3_OFF ? a.d_w2 + (e - W2_OFF) : a.d_w3 + (e - W3_OFF);
    *dst = (float)v;
}

int blocks_of(int64_t npix)
{
    const int64_t chunks = (npix + CHUNK - 1) / CHUNK;
    return (int)(chunks < MAX_G ? chunks : MAX_G);
}
// one block: the backward's partial rows.  Never 0 bytes
size_t ws_bytes(int64_t npix)
{
    const size_t b = (size_t)blocks_of(npix) * NW * sizeof(double);
    return b == 0 ? ALIGN : align_up(b);
}

bool check_sizes(const char *what, int32_t B, int32_t H, int32_t W)
{
    if (B < 0 || H < 0 || W < 0) { set_error("%s: negative size (B=%d, H=%d, W=%d)", what, B, H, W); return false; }
    if ((int64_t)B * H * W > MAX_PIX) { set_error("%s: need B * H * W <= 2^30 (B=%d, H=%d, W=%d)", what, B, H, W); return false; }
    return true;
}

bool check_args(const char *what, const SoarEnvmapArgs *a)
{
    if (!a) { set_error("%s: NULL args", what); return false; }
    if (!check_sizes(what, a->B, a->H, a->W)) return false;
    if (a->n_comp < 0 || a->n_comp > a->B) { set_error("%s: need 0 <= n_comp <= B (n_comp=%d, B=%d)", what, a->n_comp, a->B); return false; }
    if (a->color && a->color_rows != 1 && a->color_rows != a->B) {
        set_error("%s: color_rows must be 1 or B (color_rows=%d, B=%d)", what, a->color_rows, a->B);
        return false;
    }
    const int64_t npix = (int64_t)a->B * a->H * a->W, hw = (int64_t)a->H * a->W;
    if (npix == 0) return true;
    if (!a->color && !a->dirs) { set_error("%s: NULL dirs", what); return false; }
    if (!a->color && (!a->w1 || !a->w2 || !a->w3)) { set_error("%s: NULL weight", what); return false; }
    if (a->n_comp > 0 && !a->mask) { set_error("%s: NULL mask", what); return false; }
    if (a->n_comp > 0 && (a->mask_stride < hw || a->render_stride < 3 * hw)) {
        set_error("%s: render / mask image strides must be at least 3 H W / H W (got %lld, %lld)", what,
                  (long long)a->render_stride, (long long)a->mask_stride);
        return false;
    }
    return true;
}

EnvK make_k(const SoarEnvmapArgs *a)
{
    EnvK k{};
    k.hw = (int64_t)a->H * a->W;
    k.npix = k.hw * a->B;
    k.B = a->B; k.W = a->W; k.n_comp = a->n_comp; k.color_rows = a->color_rows;
    k.rs = a->render_stride; k.ms = a->mask_stride;
    for (int i = 0; i < 4; i++) k.gs[i] = a->g_comp_stride[i];
    k.dirs = a->dirs; k.color = a->color; k.render = a->render; k.mask = a->mask; k.g_comp = a->g_comp; k.g_bg = a->g_bg;
    k.w1 = a->w1; k.w2 = a->w2; k.w3 = a->w3;
    k.bg = a->bg; k.comp = a->comp; k.g_mask = a->g_mask;
    k.d_w1 = a->d_w1; k.d_w2 = a->d_w2; k.d_w3 = a->d_w3;
    k.G = blocks_of(k.npix);
    return k;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_envmap_workspace_bytes(int32_t B, int32_t H, int32_t W, size_t *bytes)
{
    if (!bytes) { set_error("soar_envmap_workspace_bytes: NULL bytes"); return 1; }
    if (!check_sizes("soar_envmap_workspace_bytes", B, H, W)) return 1;
    *bytes = ws_bytes((int64_t)B * H * W);
    return 0;
}

extern "C" int soar_envmap_forward(const SoarEnvmapArgs *args, void *stream_)
{
    if (!check_args("soar_envmap_forward", args)) return 1;
    const EnvK k = make_k(args);
    if (k.npix == 0) return 0;
    if (!args->bg) { set_error("soar_envmap_forward: NULL bg"); return 1; }
    if (args->n_comp > 0 && (!args->render || !args->comp)) { set_error("soar_envmap_forward: NULL render / comp"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(envmap_forward_kernel, dim3((unsigned)((k.npix + FWD_BLOCK - 1) / FWD_BLOCK)), dim3(FWD_BLOCK), 0, stream, k);
    SOAR_LAUNCH_OK("envmap_forward", stream, 0);
    return 0;
}

extern "C" int soar_envmap_backward(const SoarEnvmapArgs *args, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_args("soar_envmap_backward", args)) return 1;
    const size_t need = ws_bytes((int64_t)args->B * args->H * args->W);
    if (!workspace_ok("soar_envmap_backward", workspace, workspace_bytes, need, "soar_envmap_workspace_bytes")) return 1;
    const bool want_w = args->d_w1 || args->d_w2 || args->d_w3;
    if (want_w && !(args->d_w1 && args->d_w2 && args->d_w3)) {
        set_error("soar_envmap_backward: d_w1, d_w2 and d_w3 are wanted together or not at all");
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    EnvK k = make_k(args);
    const bool any_g = args->g_comp || args->g_bg;
    // the weights' gradients are exact zeros without the MLP (a constant colour) or without an upstream gradient
    k.need_w = want_w && any_g && !args->color && k.npix > 0;
    if (want_w && !k.need_w) {
        if (args->d_w1) SOAR_HIP_OK(hipMemsetAsync(args->d_w1, 0, HID * ENC * sizeof(float), stream));
        if (args->d_w2) SOAR_HIP_OK(hipMemsetAsync(args->d_w2, 0, HID * HID * sizeof(float), stream));
        if (args->d_w3) SOAR_HIP_OK(hipMemsetAsync(args->d_w3, 0, OUT * HID * sizeof(float), stream));
    }
    if (k.npix == 0) return 0;
    const bool want_mask = args->g_mask && args->n_comp > 0;
    if (want_mask && !args->g_comp) {
        SOAR_HIP_OK(hipMemsetAsync(args->g_mask, 0, (size_t)args->n_comp * k.hw * sizeof(float), stream));
        k.g_mask = nullptr;
    }
    if (!k.need_w && !(want_mask && args->g_comp)) return 0;
    // without the weights' sums a plain grid over the pixels; with them the fixed grid the partial rows are laid out for
    if (k.need_w) {
        k.partial = static_cast<double *>(workspace);
    } else {
        const int64_t chunks = (k.npix + CHUNK - 1) / CHUNK;
        k.G = (int)(chunks < (int64_t)1 << 30 ? chunks : (int64_t)1 << 30);
    }
    hipLaunchKernelGGL(envmap_bwd_kernel, dim3(k.G), dim3(CHUNK), 0, stream, k);
    SOAR_LAUNCH_OK("envmap_bwd", stream, 0);
    if (k.need_w) {
        hipLaunchKernelGGL(envmap_reduce_kernel, dim3((NW + 63) / 64), dim3(RED_WAVES * 64), 0, stream, k);
        SOAR_LAUNCH_OK("envmap_reduce", stream, 0);
    }
    return 0;
}
