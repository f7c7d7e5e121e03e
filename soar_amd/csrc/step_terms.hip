// step_terms.hip -- the image terms of the training step that had no kernel (soar_amd/step_losses.py):
//
//   soar_consistency_loss[_backward]   cos_loss(pred_normal, normal, thrsh) over B <= 8 views with the gradient of BOTH images
//                                      (TS/system/gaussian_surfel_mvdream.py:429-453: the reference's .detach() is commented out)
//   soar_normal_view_terms             the front / back normal views in one pass: 0.2 cos_loss per view, the normal-mask L1 and the
//                                      four LPIPS inputs ((n * m) - 0.5) * 2 (:332-399); one pass back
//   soar_frame_extra_terms[_backward]  loss_occ = mean(1 - comp_occ[gt_mask > 0]) with the count kept on the device (:412-417) and
//                                      gt_rgb_blended = gt_rgb * m + rand_bg * (1 - m) (:307-309)
//   soar_abs_mean[_backward]           mean|x| (:455-460)
//
// The cosine and L1 terms are the kernels of image_losses.hip pixel for pixel: the arithmetic comes from loss_pixel.h, a thread
// walks the same pixels in the same order (four consecutive pixels per trip when the planes allow 16-byte accesses, one otherwise:
// the rule of image_losses.hip; one width for the views of a launch), a workgroup and the finish fold their pairs the same way --
// so a value here has the bits of soar_cos_loss / soar_masked_l1 on the same image.  The occlusion and |x| means sum in float64 (as eval.hip does): per thread, over
// the wavefront, over the workgroup, over the workgroups, each in a fixed order.  No atomics anywhere: the same bits in every run.
// Compiled with -ffp-contract=off: the LPIPS inputs and the composite are torch's multiply, subtract, multiply / multiply, subtract,
// multiply, add, each rounded once (loss_pixel.h writes the cosine's own roundings out, fused multiply-add included).
#include "soar_common.h"
#include "loss_pixel.h"

#include <cstdint>

namespace soar {
namespace {

inline bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0u; }
inline bool al4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0u; }
inline int walk_blocks(int n, bool vec4) { return min(LOSS_BLOCKS, ((vec4 ? n / 4 : n) + 255) / 256); }

// V pixels from p * V: one 16-byte access when the plane allows it, else V 4-byte ones (V = 1: always)
template <int V>
__device__ __forceinline__ void load_px(const float *plane, int p, bool wide, float (&o)[V])
{
    if constexpr (V == 4) {
        if (wide) { const float4 v = reinterpret_cast<const float4 *>(plane)[p]; o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; return; }
    }
#pragma unroll
    for (int k = 0; k < V; k++) o[k] = plane[(size_t)p * V + k];
}
template <int V>
__device__ __forceinline__ void store_px(float *plane, int p, bool wide, const float (&o)[V])
{
    if constexpr (V == 4) {
        if (wide) { reinterpret_cast<float4 *>(plane)[p] = make_float4(o[0], o[1], o[2], o[3]); return; }
    }
#pragma unroll
    for (int k = 0; k < V; k++) plane[(size_t)p * V + k] = o[k];
}

// ---- predicted-normal consistency ------------------------------------------------------------------------------------------
struct ConsView {
    const float *a, *b;                // [3,n] planes of the two images
    float *ga, *gb;                    // backward out [3,n]
    float *partials;                   // [nblk][2]
    const float *stats;                // backward: {loss, count} of the view
    const float *up;                   // backward: upstream factor of the view (device scalar)
    int vec4, nblk;                    // walk four pixels per trip; workgroups of this view's walk
};
struct ConsArgs {
    ConsView v[MAX_BATCH];
    int n;
    float cos_limit, weight;
};

template <bool BACKWARD, int V>
__device__ __forceinline__ void cons_walk(const ConsView &v, int n, float cos_limit, float weight)
{
    float s = 0.f, cnt = 0.f, scale = 0.f;
    if (BACKWARD) scale = *v.up / fmaxf(v.stats[1], 1.f);
    const int nv = n / V;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < nv; p += v.nblk * 256) {
        float x[3][V], y[3][V], cs[V];
#pragma unroll
        for (int k = 0; k < V; k++) cs[k] = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            load_px<V>(v.a + (size_t)c * n, p, true, x[c]);
            load_px<V>(v.b + (size_t)c * n, p, true, y[c]);
#pragma unroll
            for (int k = 0; k < V; k++) cos_accumulate(cs[k], x[c][k], y[c][k], weight);
        }
        bool sel[V];
#pragma unroll
        for (int k = 0; k < V; k++) sel[k] = cs[k] < cos_limit;
        if (BACKWARD) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                float g[V], h[V];
#pragma unroll
                for (int k = 0; k < V; k++) {
                    g[k] = sel[k] ? cos_grad_value(weight, y[c][k], scale) : 0.f;
                    h[k] = sel[k] ? cos_grad_value(weight, x[c][k], scale) : 0.f;
                }
                store_px<V>(v.ga + (size_t)c * n, p, true, g);
                store_px<V>(v.gb + (size_t)c * n, p, true, h);
            }
        } else {
#pragma unroll
            for (int k = 0; k < V; k++) { s += sel[k] ? 1.f - cs[k] : 0.f; cnt += sel[k] ? 1.f : 0.f; }
        }
    }
    if (!BACKWARD) block_sum2(s, cnt, v.partials);
}

template <bool BACKWARD>
__global__ void __launch_bounds__(256) consistency_kernel(ConsArgs a)
{
    const ConsView &v = a.v[blockIdx.y];
    if (v.vec4) cons_walk<BACKWARD, 4>(v, a.n, a.cos_limit, a.weight);
    else cons_walk<BACKWARD, 1>(v, a.n, a.cos_limit, a.weight);
}

struct FinishArgs {
    const float *partials[MAX_BATCH];
    float *stats[MAX_BATCH];
    float *scaled[MAX_BATCH];          // or null: scaled[0] = factor * stats[0]
    int nblk[MAX_BATCH];
    float factor[MAX_BATCH];
};
__global__ void __launch_bounds__(256) pairs_finish_kernel(FinishArgs f)
{
    const int y = blockIdx.y;
    mean_finish_block(f.partials[y], f.nblk[y], 1.0f, f.stats[y]);
    if (threadIdx.x == 0 && f.scaled[y]) *f.scaled[y] = f.factor[y] * f.stats[y][0];     // (the thread that wrote stats[0])
}

// ---- the two normal views ---------------------------------------------------------------------------------------------------
struct NormalViewDev {
    int n, views;
    const float *normal[2], *gt[2];    // [3,n] planes of the rendered normal view and of its target
    const float *mask0, *gt_mask;      // [n]: comp_normal_mask[0], the float target mask
    float *lpips_in;                   // [2 views][3][n]: the rendered views, then the targets
    float *part_cos[2], *part_l1;
    int vec_cos[2], vec_l1, nblk_cos[2], nblk_l1;
    int wide_mask;                     // the float target mask takes 16-byte loads (the images of a four-pixel walk always do)
    // backward
    const float *stats;                // {cos F, count, cos B, count, L1, count}
    const float *up;                   // [3] device: upstream of the two 0.2 cos terms and of the L1 term
    const float *g_lpips;              // [views][3][n] upstream of the rendered views' LPIPS inputs, or null
    float *g_normal, *g_mask0;         // [views][3][n], [n]
};

template <int V>
__device__ __forceinline__ void normal_cos_walk(const NormalViewDev &a, int v)
{
    float s = 0.f, cnt = 0.f;
    const int n = a.n, nv = n / V;
    const bool wide_out = (n & 3) == 0;
    float *out_x = a.lpips_in + (size_t)v * 3 * n, *out_y = a.lpips_in + (size_t)(a.views + v) * 3 * n;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < nv; p += a.nblk_cos[v] * 256) {
        float m[V], mm[V], cs[V];
        bool sel[V];
        load_px<V>(a.gt_mask, p, a.wide_mask, m);
#pragma unroll
        for (int k = 0; k < V; k++) {
            sel[k] = m[k] > 1e-5f;
            // the reference multiplies the front view by the float mask and the back view by its binarisation (:346, :378)
            mm[k] = v == 0 ? m[k] : (sel[k] ? 1.f : 0.f);
            cs[k] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float x[V], y[V], ox[V], oy[V];
            load_px<V>(a.normal[v] + (size_t)c * n, p, true, x);
            load_px<V>(a.gt[v] + (size_t)c * n, p, true, y);
#pragma unroll
            for (int k = 0; k < V; k++) {
                cos_accumulate(cs[k], x[k], y[k], 1.f);
                ox[k] = ((x[k] * mm[k]) - 0.5f) * 2.f;
                oy[k] = ((y[k] * mm[k]) - 0.5f) * 2.f;
            }
            store_px<V>(out_x + (size_t)c * n, p, wide_out, ox);
            store_px<V>(out_y + (size_t)c * n, p, wide_out, oy);
        }
#pragma unroll
        for (int k = 0; k < V; k++) {
            sel[k] = sel[k] && cs[k] < 1.f;                // thrsh = 0
            s += sel[k] ? 1.f - cs[k] : 0.f;
            cnt += sel[k] ? 1.f : 0.f;
        }
    }
    block_sum2(s, cnt, a.part_cos[v]);
}

template <int V>
__device__ __forceinline__ void normal_l1_walk(const NormalViewDev &a)
{
    float s = 0.f, cnt = 0.f;
    const int nv = a.n / V;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < nv; p += a.nblk_l1 * 256) {
        float x[V], y[V];
        load_px<V>(a.mask0, p, true, x);
        load_px<V>(a.gt_mask, p, true, y);
#pragma unroll
        for (int k = 0; k < V; k++) { cnt += 1.f; s += fabsf(x[k] - y[k]); }
    }
    block_sum2(s, cnt, a.part_l1);
}

__global__ void __launch_bounds__(256) normal_view_values_kernel(NormalViewDev a)
{
    const int v = blockIdx.y;
    if ((int)blockIdx.x < a.nblk_cos[v]) {
        if (a.vec_cos[v]) normal_cos_walk<4>(a, v);
        else normal_cos_walk<1>(a, v);
    }
    if (v == 0 && (int)blockIdx.x < a.nblk_l1) {
        __syncthreads();                                   // (block_sum2's LDS rows are read by thread 0 of the walk above)
        if (a.vec_l1) normal_l1_walk<4>(a);
        else normal_l1_walk<1>(a);
    }
}

// gradients are element-wise: one width for the whole launch (16-byte accesses when every plane allows them)
template <int V>
__global__ void __launch_bounds__(256) normal_view_grads_kernel(NormalViewDev a)
{
    const int v = blockIdx.y, n = a.n, nv = n / V;
    const float sc_cos = (a.up[v] * 0.2f) / fmaxf(a.stats[2 * v + 1], 1.f);
    const float sc_l1 = a.up[2] / fmaxf(a.stats[5] * 1.f, 1.f);
    for (int p = blockIdx.x * 256 + threadIdx.x; p < nv; p += gridDim.x * 256) {
        float m[V], mm[V], cs[V], y[3][V];
        bool sel[V];
        load_px<V>(a.gt_mask, p, true, m);
#pragma unroll
        for (int k = 0; k < V; k++) {
            sel[k] = m[k] > 1e-5f;
            mm[k] = v == 0 ? m[k] : (sel[k] ? 1.f : 0.f);
            cs[k] = 0.f;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float x[V];
            load_px<V>(a.normal[v] + (size_t)c * n, p, true, x);
            load_px<V>(a.gt[v] + (size_t)c * n, p, true, y[c]);
#pragma unroll
            for (int k = 0; k < V; k++) cos_accumulate(cs[k], x[k], y[c][k], 1.f);
        }
#pragma unroll
        for (int k = 0; k < V; k++) sel[k] = sel[k] && cs[k] < 1.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float g[V], gl[V];
            if (a.g_lpips) load_px<V>(a.g_lpips + ((size_t)v * 3 + c) * n, p, true, gl);
#pragma unroll
            for (int k = 0; k < V; k++) {
                g[k] = sel[k] ? cos_grad_value(1.f, y[c][k], sc_cos) : 0.f;
                if (a.g_lpips) g[k] = g[k] + (gl[k] * 2.f) * mm[k];          // d ((x m) - 0.5) 2 / d x
            }
            store_px<V>(a.g_normal + ((size_t)v * 3 + c) * n, p, true, g);
        }
        if (v == 0) {
            float x[V], g[V];
            load_px<V>(a.mask0, p, true, x);
#pragma unroll
            for (int k = 0; k < V; k++) {
                const float d = x[k] - m[k];
                g[k] = d > 0.f ? sc_l1 : (d < 0.f ? -sc_l1 : 0.f);
            }
            store_px<V>(a.g_mask0, p, true, g);
        }
    }
}

// ---- float64 means ------------------------------------------------------------------------------------------------------------
// a workgroup of 256 threads leaves {sum, count} in float64, in a fixed order
__device__ __forceinline__ void block_sum2d(double s, double c, double *partials)
{
    __shared__ double red[4][2];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); c += __shfl_xor(c, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
        partials[2 * blockIdx.x + 1] = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    }
}
// stats = {(float)(sum / count), (float)count}: 0 / 0 = NaN for an empty selection
__global__ void __launch_bounds__(256) mean_finish64_kernel(const double *partials, int nblocks, float *stats)
{
    __shared__ double red[4][2];
    double s = 0.0, c = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 256) { s += partials[2 * k]; c += partials[2 * k + 1]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); c += __shfl_xor(c, off); }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = s; red[threadIdx.x >> 6][1] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double st = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]), ct = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
        stats[0] = (float)(st / ct);
        stats[1] = (float)ct;
    }
}

struct FrameExtraDev {
    int n;
    const float *occ;                  // [3,n] planes
    const float *rgb, *mask, *bg;      // element strides below: any layout whose H and W fold into one pixel stride
    int64_t rgb_c, rgb_p, bg_c, bg_p;
    float *blended;                    // [3,n] planes
    double *partials;
    // backward
    const float *stats, *up;
    float *g_occ;                      // [3,n]
};

__global__ void __launch_bounds__(256) frame_extra_kernel(FrameExtraDev a)
{
    double s = 0.0, cnt = 0.0;
    const size_t n = (size_t)a.n;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < a.n; p += gridDim.x * 256) {
        const float m = a.mask[p];
        const bool sel = m > 0.f;
        const float om = 1.f - m;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (sel) { s += 1.0 - (double)a.occ[c * n + p]; cnt += 1.0; }
            a.blended[c * n + p] = a.rgb[c * a.rgb_c + p * a.rgb_p] * m + a.bg[c * a.bg_c + p * a.bg_p] * om;
        }
    }
    block_sum2d(s, cnt, a.partials);
}

__global__ void __launch_bounds__(256) frame_extra_backward_kernel(FrameExtraDev a)
{
    const float sc = *a.up / a.stats[1];                 // (no selected pixel: never used)
    const size_t n = (size_t)a.n;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < a.n; p += gridDim.x * 256) {
        const float g = a.mask[p] > 0.f ? -sc : 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) a.g_occ[c * n + p] = g;
    }
}

template <bool BACKWARD>
__global__ void __launch_bounds__(256) abs_mean_kernel(const float *x, int64_t n, double *partials, const float *up, float *grad)
{
    double s = 0.0, cnt = 0.0;
    float sc = 0.f;
    if (BACKWARD) sc = *up / (float)n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = x[i];
        if (BACKWARD) grad[i] = v > 0.f ? sc : (v < 0.f ? -sc : 0.f);          // sign(0) = 0, as torch.abs has it
        else { s += (double)fabsf(v); cnt += 1.0; }
    }
    if (!BACKWARD) block_sum2d(s, cnt, partials);
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_step_terms_scratch_bytes(size_t *bytes)
{
    if (!bytes) { set_error("soar_step_terms_scratch_bytes: NULL"); return 1; }
    *bytes = (size_t)MAX_BATCH * 2 * LOSS_BLOCKS * sizeof(double);
    return 0;
}

static int cons_fill(const char *me, ConsArgs &a, int32_t B, int32_t H, int32_t W, const float *pa, int64_t sa, const float *pb, int64_t sb,
                     float cos_thrsh, float weight, float *ga, float *gb)
{
    const int64_t n64 = (int64_t)H * W;
    if (B < 1 || B > MAX_BATCH || H <= 0 || W <= 0 || n64 > (1 << 28) || !pa || !pb) {
        set_error("%s: bad arguments (B=%d, H=%d, W=%d; need 1 <= B <= %d, H W <= 2^28, images)", me, B, H, W, MAX_BATCH);
        return 1;
    }
    if (sa < 3 * n64 || sb < 3 * n64) { set_error("%s: a view stride is shorter than a view (3 H W floats)", me); return 1; }
    if (!al4(pa) || !al4(pb)) { set_error("%s: the images must be 4-byte aligned", me); return 1; }
    a.n = (int)n64; a.cos_limit = cos_thrsh; a.weight = weight;
    // (the rule of image_losses.hip's loss_vec4; one width for the views of a launch, as a batch of soar_cos_loss calls has it)
    bool vec4 = (n64 & 3) == 0;
    for (int v = 0; v < B; v++) {
        ConsView &q = a.v[v];
        q = ConsView{};
        q.a = pa + v * sa; q.b = pb + v * sb;
        if (ga) { q.ga = ga + (size_t)v * 3 * n64; q.gb = gb + (size_t)v * 3 * n64; }
        vec4 = vec4 && al16(q.a) && al16(q.b) && (!ga || (al16(q.ga) && al16(q.gb)));
    }
    for (int v = 0; v < B; v++) {
        a.v[v].vec4 = vec4;
        a.v[v].nblk = walk_blocks(a.n, vec4);
    }
    return 0;
}

int soar_consistency_loss(int32_t B, int32_t H, int32_t W, const float *a, int64_t a_stride, const float *b, int64_t b_stride,
                          float cos_thrsh, float weight, float *stats, float *scratch, void *stream_)
{
    const char *me = "soar_consistency_loss";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    ConsArgs q;
    if (cons_fill(me, q, B, H, W, a, a_stride, b, b_stride, cos_thrsh, weight, nullptr, nullptr)) return 1;
    if (!stats || !scratch) { set_error("%s: NULL stats / scratch", me); return 1; }
    FinishArgs f = {};
    int grid = 0;
    for (int v = 0; v < B; v++) {
        q.v[v].partials = scratch + (size_t)v * 2 * LOSS_BLOCKS;
        f.partials[v] = q.v[v].partials; f.stats[v] = stats + 2 * v; f.nblk[v] = q.v[v].nblk;
        grid = max(grid, q.v[v].nblk);
    }
    StageTimer timer(ST_FRAME_LOSS, stream);
    hipLaunchKernelGGL(consistency_kernel<false>, dim3(grid, B), dim3(256), 0, stream, q);
    hipLaunchKernelGGL(pairs_finish_kernel, dim3(1, B), dim3(256), 0, stream, f);
    SOAR_LAUNCH_OK("consistency_loss", stream, 0);
    return 0;
}

int soar_consistency_loss_backward(int32_t B, int32_t H, int32_t W, const float *a, int64_t a_stride, const float *b, int64_t b_stride,
                                   float cos_thrsh, float weight, const float *stats, const float *upstream_dev, float *dL_da,
                                   float *dL_db, void *stream_)
{
    const char *me = "soar_consistency_loss_backward";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!stats || !upstream_dev || !dL_da || !dL_db) { set_error("%s: NULL stats / upstream / gradient", me); return 1; }
    if (!al4(dL_da) || !al4(dL_db)) { set_error("%s: the gradients must be 4-byte aligned", me); return 1; }
    ConsArgs q;
    if (cons_fill(me, q, B, H, W, a, a_stride, b, b_stride, cos_thrsh, weight, dL_da, dL_db)) return 1;
    int grid = 0;
    for (int v = 0; v < B; v++) {
        q.v[v].stats = stats + 2 * v; q.v[v].up = upstream_dev + v;
        grid = max(grid, q.v[v].nblk);
    }
    StageTimer timer(ST_FRAME_LOSS, stream);
    hipLaunchKernelGGL(consistency_kernel<true>, dim3(grid, B), dim3(256), 0, stream, q);
    SOAR_LAUNCH_OK("consistency_loss_backward", stream, 0);
    return 0;
}

int soar_normal_view_terms(const SoarNormalViewArgs *args, int32_t mode, void *stream_)
{
    const char *me = "soar_normal_view_terms";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarNormalViewArgs &q = *args;
    const int64_t n64 = (int64_t)q.R * q.R;
    if (q.R <= 0 || n64 > (1 << 28) || q.views < 1 || q.views > 2 || (mode != 1 && mode != 2)) {
        set_error("%s: bad arguments (R=%d, views=%d, mode=%d; need R^2 <= 2^28, views 1 or 2, mode 1 (values) or 2 (gradients))", me, q.R, q.views, mode);
        return 1;
    }
    if (!q.normal || !q.mask0 || !q.gt_F || (q.views == 2 && !q.gt_B) || !q.gt_mask || !q.stats) { set_error("%s: NULL image, target or stats", me); return 1; }
    if (q.normal_stride < 3 * n64) { set_error("%s: the view stride is shorter than a view (3 R R floats)", me); return 1; }
    if (!al4(q.normal) || !al4(q.mask0) || !al4(q.gt_F) || !al4(q.gt_B) || !al4(q.gt_mask)) { set_error("%s: the images must be 4-byte aligned", me); return 1; }
    NormalViewDev a = {};
    a.n = (int)n64; a.views = q.views;
    a.normal[0] = q.normal; a.normal[1] = q.normal + q.normal_stride;
    a.gt[0] = q.gt_F; a.gt[1] = q.gt_B;
    a.mask0 = q.mask0; a.gt_mask = q.gt_mask; a.stats = q.stats;
    const bool n4 = (n64 & 3) == 0;
    StageTimer timer(ST_FRAME_LOSS, stream);
    if (mode == 1) {
        if (!q.lpips_in || !q.values || !q.scratch || !al16(q.lpips_in)) { set_error("%s: NULL lpips_in / values / scratch, or lpips_in not 16-byte aligned", me); return 1; }
        a.lpips_in = q.lpips_in;
        int grid = 0;
        FinishArgs f = {};
        for (int v = 0; v < q.views; v++) {
            // the width of the walk is what soar_cos_loss takes for the view (its byte mask is a tensor of its own: aligned)
            a.vec_cos[v] = n4 && al16(a.normal[v]) && al16(a.gt[v]);
            a.nblk_cos[v] = walk_blocks(a.n, a.vec_cos[v]);
            a.part_cos[v] = q.scratch + (size_t)v * 2 * LOSS_BLOCKS;
            f.partials[v] = a.part_cos[v]; f.stats[v] = q.stats + 2 * v; f.nblk[v] = a.nblk_cos[v];
            f.scaled[v] = q.values + v; f.factor[v] = 0.2f;
            grid = max(grid, a.nblk_cos[v]);
        }
        a.wide_mask = n4 && al16(q.gt_mask);
        a.vec_l1 = a.wide_mask && al16(q.mask0);
        a.nblk_l1 = walk_blocks(a.n, a.vec_l1);
        a.part_l1 = q.scratch + (size_t)2 * 2 * LOSS_BLOCKS;
        f.partials[q.views] = a.part_l1; f.stats[q.views] = q.stats + 4; f.nblk[q.views] = a.nblk_l1;
        f.scaled[q.views] = q.values + 2; f.factor[q.views] = 1.0f;
        grid = max(grid, a.nblk_l1);
        hipLaunchKernelGGL(normal_view_values_kernel, dim3(grid, q.views), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(pairs_finish_kernel, dim3(1, q.views + 1), dim3(256), 0, stream, f);
    } else {
        if (!q.up || !q.g_normal || !q.g_mask0 || !al4(q.g_lpips) || !al4(q.g_normal) || !al4(q.g_mask0)) { set_error("%s: NULL or misaligned up / g_normal / g_mask0", me); return 1; }
        a.up = q.up; a.g_lpips = q.g_lpips; a.g_normal = q.g_normal; a.g_mask0 = q.g_mask0;
        bool wide = n4 && al16(q.normal) && (q.normal_stride & 3) == 0 && al16(q.mask0) && al16(q.gt_F) && al16(q.gt_B) && al16(q.gt_mask) && al16(q.g_lpips) &&
            al16(q.g_normal) && al16(q.g_mask0);
        if (wide) hipLaunchKernelGGL(normal_view_grads_kernel<4>, dim3(walk_blocks(a.n, true), q.views), dim3(256), 0, stream, a);
        else hipLaunchKernelGGL(normal_view_grads_kernel<1>, dim3(walk_blocks(a.n, false), q.views), dim3(256), 0, stream, a);
    }
    SOAR_LAUNCH_OK("normal_view_terms", stream, 0);
    return 0;
}

static int frame_extra_fill(const char *me, const SoarFrameExtraArgs *args, FrameExtraDev &a)
{
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarFrameExtraArgs &q = *args;
    const int64_t n64 = (int64_t)q.H * q.W;
    if (q.H <= 0 || q.W <= 0 || n64 > (1 << 28)) { set_error("%s: bad arguments (H=%d, W=%d; need H W <= 2^28)", me, q.H, q.W); return 1; }
    if (!q.gt_mask || !q.stats || !al4(q.gt_mask) || !al4(q.occ)) { set_error("%s: NULL or misaligned gt_mask / stats / occ", me); return 1; }
    a = FrameExtraDev{};
    a.n = (int)n64; a.occ = q.occ; a.mask = q.gt_mask; a.stats = q.stats;
    return 0;
}

int soar_frame_extra_terms(const SoarFrameExtraArgs *args, void *stream_)
{
    const char *me = "soar_frame_extra_terms";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FrameExtraDev a;
    if (frame_extra_fill(me, args, a)) return 1;
    const SoarFrameExtraArgs &q = *args;
    if (!q.occ || !q.gt_rgb || !q.rand_bg || !q.blended || !q.scratch || !al4(q.gt_rgb) || !al4(q.rand_bg) || !al4(q.blended)) {
        set_error("%s: NULL or misaligned occ / gt_rgb / rand_bg / blended / scratch", me);
        return 1;
    }
    if (q.rgb_stride[0] < 0 || q.rgb_stride[1] < 0 || q.bg_stride[0] < 0 || q.bg_stride[1] < 0) { set_error("%s: negative stride", me); return 1; }
    a.rgb = q.gt_rgb; a.bg = q.rand_bg; a.blended = q.blended; a.partials = static_cast<double *>(q.scratch);
    a.rgb_c = q.rgb_stride[0]; a.rgb_p = q.rgb_stride[1]; a.bg_c = q.bg_stride[0]; a.bg_p = q.bg_stride[1];
    const int blocks = walk_blocks(a.n, false);
    StageTimer timer(ST_FRAME_LOSS, stream);
    hipLaunchKernelGGL(frame_extra_kernel, dim3(blocks), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(mean_finish64_kernel, dim3(1), dim3(256), 0, stream, a.partials, blocks, q.stats);
    SOAR_LAUNCH_OK("frame_extra_terms", stream, 0);
    return 0;
}

int soar_frame_extra_terms_backward(const SoarFrameExtraArgs *args, void *stream_)
{
    const char *me = "soar_frame_extra_terms_backward";
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FrameExtraDev a;
    if (frame_extra_fill(me, args, a)) return 1;
    if (!args->up || !args->g_occ || !al4(args->g_occ)) { set_error("%s: NULL or misaligned up / g_occ", me); return 1; }
    a.up = args->up; a.g_occ = args->g_occ;
    StageTimer timer(ST_FRAME_LOSS, stream);
    hipLaunchKernelGGL(frame_extra_backward_kernel, dim3(walk_blocks(a.n, false)), dim3(256), 0, stream, a);
    SOAR_LAUNCH_OK("frame_extra_terms_backward", stream, 0);
    return 0;
}

int soar_abs_mean(int64_t n, const float *x, float *stats, void *scratch, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n < 1 || n > ((int64_t)1 << 30) || !x || !stats || !scratch || !al4(x)) { set_error("soar_abs_mean: bad arguments (n=%lld; need 1 <= n <= 2^30, x 4-byte aligned)", (long long)n); return 1; }
    const int blocks = (int)min((int64_t)LOSS_BLOCKS, (n + 255) / 256);
    double *partials = static_cast<double *>(scratch);
    StageTimer timer(ST_FRAME_LOSS, stream);
    hipLaunchKernelGGL(abs_mean_kernel<false>, dim3(blocks), dim3(256), 0, stream, x, n, partials, (const float *)nullptr, (float *)nullptr);
    hipLaunchKernelGGL(mean_finish64_kernel, dim3(1), dim3(256), 0, stream, (const double *)partials, blocks, stats);
    SOAR_LAUNCH_OK("abs_mean", stream, 0);
    return 0;
}

int soar_abs_mean_backward(int64_t n, const float *x, const float *upstream_dev, float *dL_dx, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n < 1 || n > ((int64_t)1 << 30) || !x || !upstream_dev || !dL_dx || !al4(x) || !al4(dL_dx)) {
        set_error("soar_abs_mean_backward: bad arguments (n=%lld; need 1 <= n <= 2^30, 4-byte aligned x and gradient)", (long long)n);
        return 1;
    }
    const int blocks = (int)min((int64_t)LOSS_BLOCKS, (n + 255) / 256);
    StageTimer timer(ST_FRAME_LOSS, stream);
    hipLaunchKernelGGL(abs_mean_kernel<true>, dim3(blocks), dim3(256), 0, stream, x, n, (double *)nullptr, upstream_dev, dL_dx);
    SOAR_LAUNCH_OK("abs_mean_backward", stream, 0);
    return 0;
}

}  // extern "C"
