// frame_loss.hip -- per-frame image loss, value and pixel gradients in ONE pass over the rasterizer outputs.
//
// L = wc * mean|color - target| + wm * mean|opac - mask| + wn * mean(normal . n_target) + wd * mean(depth)
// is the dense four-output loss SURVEY.md section 8(d) prescribes for the per-frame benchmark (the reference's
// per-frame losses -- masked L1, cosine normal loss, TS/system/gaussian_surfel_mvdream.py:311-330,622-630 -- have
// the same structure: per-pixel terms averaged over the image).  In eager torch this is ~25 full-image kernels per
// frame; here every pixel is read once and its four gradient planes are written once.
#include "soar_common.h"
#include "frame_loss_terms.h"
#include "loss_finish.h"

namespace soar {

namespace {

// LossArgs, the pixel arithmetic and the walk of a thread: frame_loss_terms.h (shared with the backward blend's loss form)
template <int V>
__global__ void __launch_bounds__(256) frame_loss_kernel(Batch<LossArgs> batch)
{
    LossArgs a = batch.v[blockIdx.y];                 // (a copy: the pooled form points it at its frame's target planes)
    loss_pick_target_set(a);
    float s_c = 0.f, s_m = 0.f, s_n = 0.f, s_d = 0.f;
    frame_loss_walk<V, true>(a, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256, s_c, s_m, s_n, s_d);
    __shared__ float part[4][4];
    s_c = wave_sum(s_c); s_m = wave_sum(s_m); s_n = wave_sum(s_n); s_d = wave_sum(s_d);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { part[wave][0] = s_c; part[wave][1] = s_m; part[wave][2] = s_n; part[wave][3] = s_d; }
    __syncthreads();
    if (threadIdx.x < 4)
        a.sums[4 * blockIdx.x + threadIdx.x] = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// the sum of the partials and the value: loss_finish_sum (loss_finish.h)
struct LossFinishArgs {
    const float *sums;
    int blocks, n;
    float wc, wm, wn, wd;
    float *loss;
};
__global__ void __launch_bounds__(256) frame_loss_finish_kernel(Batch<LossFinishArgs> batch)
{
    const LossFinishArgs &fa = batch.v[blockIdx.y];
    __shared__ float4 red[256];
    loss_finish_sum(fa.sums, fa.blocks, fa.n, fa.wc, fa.wm, fa.wn, fa.wd, fa.loss, red);
}

}  // namespace

}  // namespace soar

using namespace soar;

static int frame_loss_launch(int32_t W, int32_t H, const float *color, const float *normal, const float *depth, const float *opac,
                             const float *target_color, const float *target_mask, const float *target_normal,
                             const int32_t *set_index_dev, int32_t n_sets, float w_color, float w_mask, float w_normal,
                             float w_depth, float *loss_out, float *sums4, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                             float *dL_dopac, const void *image_buffer, const float *background, int32_t normalize_depth, hipStream_t stream,
                             SoarLossFinish *finish_out = nullptr);

extern "C" int soar_frame_loss(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                               const float *opac, const float *target_color, const float *target_mask,
                               const float *target_normal, float w_color, float w_mask, float w_normal, float w_depth,
                               float *loss_out, float *sums4, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                               float *dL_dopac, const void *image_buffer, const float *background, int32_t normalize_depth,
                               void *stream_)
{
    return frame_loss_launch(W, H, color, normal, depth, opac, target_color, target_mask, target_normal, nullptr, 1, w_color,
                             w_mask, w_normal, w_depth, loss_out, sums4, dL_dcolor, dL_dnormal, dL_ddepth, dL_dopac, image_buffer,
                             background, normalize_depth, static_cast<hipStream_t>(stream_));
}

extern "C" int soar_frame_loss_pooled(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                                      const float *opac, const float *target_pool, int32_t n_sets,
                                      const int32_t *set_index_dev, float w_color, float w_mask, float w_normal, float w_depth,
                                      float *loss_out, float *sums4, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                                      float *dL_dopac, const void *image_buffer, const float *background,
                                      int32_t normalize_depth, void *stream_)
{
    if (n_sets <= 0 || !set_index_dev) { set_error("soar_frame_loss_pooled: need n_sets > 0 and a device index"); return 1; }
    return frame_loss_launch(W, H, color, normal, depth, opac, target_pool, target_pool, target_pool, set_index_dev, n_sets,
                             w_color, w_mask, w_normal, w_depth, loss_out, sums4, dL_dcolor, dL_dnormal, dL_ddepth, dL_dopac,
                             image_buffer, background, normalize_depth, static_cast<hipStream_t>(stream_));
}

extern "C" int soar_frame_loss_partials(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                                        const float *opac, const float *target_color, const float *target_mask,
                                        const float *target_normal, float w_color, float w_mask, float w_normal, float w_depth,
                                        float *loss_out, float *sums4, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                                        float *dL_dopac, const void *image_buffer, const float *background, int32_t normalize_depth,
                                        SoarLossFinish *finish_out, void *stream_)
{
    if (!finish_out) { set_error("soar_frame_loss_partials: finish_out is NULL"); return 1; }
    return frame_loss_launch(W, H, color, normal, depth, opac, target_color, target_mask, target_normal, nullptr, 1, w_color,
                             w_mask, w_normal, w_depth, loss_out, sums4, dL_dcolor, dL_dnormal, dL_ddepth, dL_dopac, image_buffer,
                             background, normalize_depth, static_cast<hipStream_t>(stream_), finish_out);
}

extern "C" int soar_frame_loss_pooled_partials(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                                               const float *opac, const float *target_pool, int32_t n_sets,
                                               const int32_t *set_index_dev, float w_color, float w_mask, float w_normal, float w_depth,
                                               float *loss_out, float *sums4, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                                               float *dL_dopac, const void *image_buffer, const float *background,
                                               int32_t normalize_depth, SoarLossFinish *finish_out, void *stream_)
{
    if (!finish_out) { set_error("soar_frame_loss_pooled_partials: finish_out is NULL"); return 1; }
    if (n_sets <= 0 || !set_index_dev) { set_error("soar_frame_loss_pooled_partials: need n_sets > 0 and a device index"); return 1; }
    return frame_loss_launch(W, H, color, normal, depth, opac, target_pool, target_pool, target_pool, set_index_dev, n_sets,
                             w_color, w_mask, w_normal, w_depth, loss_out, sums4, dL_dcolor, dL_dnormal, dL_ddepth, dL_dopac,
                             image_buffer, background, normalize_depth, static_cast<hipStream_t>(stream_), finish_out);
}

static int frame_loss_launch(int32_t W, int32_t H, const float *color, const float *normal, const float *depth, const float *opac,
                             const float *target_color, const float *target_mask, const float *target_normal,
                             const int32_t *set_index_dev, int32_t n_sets, float w_color, float w_mask, float w_normal,
                             float w_depth, float *loss_out, float *sums4, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                             float *dL_dopac, const void *image_buffer, const float *background, int32_t normalize_depth, hipStream_t stream,
                             SoarLossFinish *finish_out)
{
    if (W <= 0 || H <= 0) { set_error("soar_frame_loss: bad image size %dx%d", W, H); return 1; }
    if (!color || !normal || !depth || !opac || !target_color || !target_mask || !target_normal || !loss_out || !sums4 ||
        !dL_dcolor || !dL_dnormal || !dL_ddepth || !dL_dopac) {
        set_error("soar_frame_loss: NULL pointer");
        return 1;
    }
    LossArgs a;
    a.n = W * H;
    a.color = color; a.normal = normal; a.depth = depth; a.opac = opac;
    a.t_color = target_color; a.t_mask = target_mask; a.t_normal = target_normal;
    a.wc = w_color; a.wm = w_mask; a.wn = w_normal; a.wd = w_depth;
    a.dcolor = dL_dcolor; a.dnormal = dL_dnormal; a.ddepth = dL_ddepth; a.dopac = dL_dopac;
    a.sums = sums4;
    a.set_index = set_index_dev; a.n_sets = n_sets;
    a.n_contrib = nullptr; a.bg_tiles = nullptr; a.W = W; a.gx = (W + TILE - 1) / TILE;
    a.bg = image_buffer ? background : nullptr; a.normalize_depth = normalize_depth;
    if (image_buffer) {                      // the rasterizer's image buffer of these outputs: gate the gradient planes by n_contrib
        ImageBuf img;
        carve_image(const_cast<void *>(image_buffer), W, H, &img);
        a.n_contrib = img.n_contrib;
        if (W % 4 == 0) a.bg_tiles = img.bg_tiles;       // (four consecutive pixels of the flat planes lie in one tile)
    }
    StageTimer timer(ST_FRAME_LOSS, stream);
    bool vec4;
    int blocks;
    frame_loss_grid(a, vec4, blocks);
    if (vec4) SOAR_LAUNCH_BATCHED(frame_loss_kernel<4>, dim3(blocks), dim3(256), 0, stream, a);
    else SOAR_LAUNCH_BATCHED(frame_loss_kernel<1>, dim3(blocks), dim3(256), 0, stream, a);
    if (finish_out) {
        // (the partial sums wait for soar_frames_geometry_warp_backward_losses: nothing between here and there reads the value)
        *finish_out = SoarLossFinish{sums4, loss_out, blocks, a.n, w_color, w_mask, w_normal, w_depth};
        SOAR_LAUNCH_OK("frame_loss", stream, 0);
        return 0;
    }
    const soar::LossFinishArgs fa = {sums4, blocks, a.n, w_color, w_mask, w_normal, w_depth, loss_out};
    SOAR_LAUNCH_BATCHED(frame_loss_finish_kernel, dim3(1), dim3(256), 0, stream, fa);
    SOAR_LAUNCH_OK("frame_loss", stream, 0);
    return 0;
}


// ---- step-level helpers of the frame data-parallel step (soar_amd/step_plan.py) -------------------------------------------------
namespace soar {
namespace {
// out[j] = sum over the frames of in[f][j]: the per-frame gradient blocks of one leaf -> its slice of the flat gradient buffer
// (VEC = 4: 16-byte aligned blocks of a multiple of 4 floats; VEC = 1: anything)
template <int VEC>
__global__ void __launch_bounds__(256) sum_frames_kernel(int n_frames, size_t count, const float *__restrict__ in, float *__restrict__ out)
{
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (i >= count) return;
    if (VEC == 4) {
        float4 acc = *reinterpret_cast<const float4 *>(in + i);
        for (int f = 1; f < n_frames; f++) {
            const float4 v = *reinterpret_cast<const float4 *>(in + (size_t)f * count + i);
            acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
        }
        *reinterpret_cast<float4 *>(out + i) = acc;
    } else {
        float acc = in[i];
        for (int f = 1; f < n_frames; f++) acc += in[(size_t)f * count + i];
        out[i] = acc;
    }
}
// the per-step inputs of a plan: joint transforms of the step's frames gathered from the sequence table, target-set index of
// every frame.  frame_ids live in device memory (the host only refreshes those few integers per step).
__global__ void gather_step_inputs_kernel(int n_frames, int num_frames_seq, int floats_per_frame, int n_sets,
                                          const int32_t *__restrict__ frame_ids, const float *__restrict__ table,
                                          float *__restrict__ mats_out, int32_t *__restrict__ set_out)
{
    const int f = blockIdx.x;
    int id = frame_ids[f] % num_frames_seq;
    if (id < 0) id += num_frames_seq;
    for (int k = threadIdx.x; k < floats_per_frame; k += blockDim.x) mats_out[(size_t)f * floats_per_frame + k] = table[(size_t)id * floats_per_frame + k];
    if (threadIdx.x == 0 && set_out) set_out[f] = n_sets > 0 ? id % n_sets : 0;
}
// ... with the frame ids in the kernel's arguments (the eager plan: no host -> device copy of n integers in front of every step)
struct StepFrameIds { int32_t id[MAX_BATCH]; };
__global__ void gather_step_inputs_ids_kernel(int n_frames, int num_frames_seq, int floats_per_frame, int n_sets, StepFrameIds ids,
                                              const float *__restrict__ table, float *__restrict__ mats_out, int32_t *__restrict__ set_out)
{
    const int f = blockIdx.x;
    int id = ids.id[f] % num_frames_seq;
    if (id < 0) id += num_frames_seq;
    for (int k = threadIdx.x; k < floats_per_frame; k += blockDim.x) mats_out[(size_t)f * floats_per_frame + k] = table[(size_t)id * floats_per_frame + k];
    if (threadIdx.x == 0 && set_out) set_out[f] = n_sets > 0 ? id % n_sets : 0;
}
}  // namespace
}  // namespace soar

extern "C" int soar_sum_frames(int32_t n_frames, int64_t count, const float *in_dev, float *out_dev, void *stream_)
{
    using namespace soar;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_frames <= 0 || count < 0 || !in_dev || !out_dev) { set_error("soar_sum_frames: bad arguments"); return 1; }
    if (count == 0) return 0;
    const bool vec = ((((uintptr_t)in_dev | (uintptr_t)out_dev) & 15) == 0) && ((count & 3) == 0);
    if (vec) hipLaunchKernelGGL(sum_frames_kernel<4>, dim3((unsigned)((count / 4 + 255) / 256)), dim3(256), 0, stream, n_frames, (size_t)count, in_dev, out_dev);
    else hipLaunchKernelGGL(sum_frames_kernel<1>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, n_frames, (size_t)count, in_dev, out_dev);
    SOAR_LAUNCH_OK("sum_frames", stream, 0);
    return 0;
}

extern "C" int soar_gather_step_inputs(int32_t n_frames, int32_t num_frames_seq, int32_t floats_per_frame, int32_t n_sets,
                                       const int32_t *frame_ids_dev, const float *table_dev, float *mats_out_dev,
                                       int32_t *set_index_out_dev, void *stream_)
{
    using namespace soar;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_frames <= 0 || num_frames_seq <= 0 || floats_per_frame <= 0 || !frame_ids_dev || !table_dev || !mats_out_dev) {
        set_error("soar_gather_step_inputs: bad arguments");
        return 1;
    }
    hipLaunchKernelGGL(gather_step_inputs_kernel, dim3(n_frames), dim3(256), 0, stream, n_frames, num_frames_seq, floats_per_frame, n_sets,
                       frame_ids_dev, table_dev, mats_out_dev, set_index_out_dev);
    SOAR_LAUNCH_OK("gather_step_inputs", stream, 0);
    return 0;
}

extern "C" int soar_gather_step_inputs_ids(int32_t n_frames, int32_t num_frames_seq, int32_t floats_per_frame, int32_t n_sets,
                                           const int32_t *frame_ids_host, const float *table_dev, float *mats_out_dev,
                                           int32_t *set_index_out_dev, void *stream_)
{
    using namespace soar;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_frames <= 0 || n_frames > MAX_BATCH || num_frames_seq <= 0 || floats_per_frame <= 0 || !frame_ids_host || !table_dev || !mats_out_dev) {
        set_error("soar_gather_step_inputs_ids: bad arguments (at most %d frames per step)", MAX_BATCH);
        return 1;
    }
    StepFrameIds ids = {};
    for (int f = 0; f < n_frames; f++) ids.id[f] = frame_ids_host[f];
    hipLaunchKernelGGL(gather_step_inputs_ids_kernel, dim3(n_frames), dim3(256), 0, stream, n_frames, num_frames_seq, floats_per_frame, n_sets, ids,
                       table_dev, mats_out_dev, set_index_out_dev);
    SOAR_LAUNCH_OK("gather_step_inputs", stream, 0);
    return 0;
}
