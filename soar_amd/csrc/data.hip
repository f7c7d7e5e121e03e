// data.hip -- the training data module's device side (soar_amd/data.py): the video stays on the device as bytes.
//   soar_data_mask_bbox    the masks' bounding boxes, N frames in one launch (construction time)
//   soar_data_crops        the 512 x 512 ImageDream crops (TS/data/uncond_multiview.py:246-313), boxes read on the device
//   soar_data_step_batch   a training step's whole batch in ONE launch (:340-681): the rays of the random views and of the
//                          frame's own camera, the frame gathered and converted to float32, the projection matrices
// Compiled with -ffp-contract=off: every value is pinned to a torch-CPU restatement (tests/data_ref.py); the two places where
// torch itself fuses a multiply-add (linspace, grid_sample's un-normalisation) say so with an explicit fmaf.
#include "soar_common.h"

namespace soar {
namespace {

constexpr int CROP = SOAR_DATA_CROP;
constexpr int THREADS = 256;
constexpr int RAY_PIX = 4 * THREADS;          // pixels of one workgroup of a ray job (4 rounds of 256)
constexpr int CONV_BYTES = 16 * THREADS;      // source bytes of one workgroup of a conversion job
constexpr int MASK_STAGE = 1408;              // (CONV_BYTES / 3 + 1 + 15 bytes of alignment slack, rounded up to 16) mask bytes
constexpr int COPY_FLOATS = 16 * THREADS;     // floats of one workgroup of a copy job

// ---- bounding boxes ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) mask_bbox_kernel(int H, int W, const uint8_t *__restrict__ masks, int32_t *__restrict__ boxes, int vec)
{
    __shared__ int s_box[4];
    const int t = threadIdx.x;
    const int HW = H * W;
    const uint8_t *m = masks + (size_t)blockIdx.x * HW;
    if (t == 0) { s_box[0] = W; s_box[1] = H; s_box[2] = -1; s_box[3] = -1; }
    __syncthreads();
    int x0 = W, y0 = H, x1 = -1, y1 = -1;
    auto hit = [&](int idx) {
        const int y = idx / W, x = idx - y * W;
        x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
    };
    const int chunks = vec ? HW / 16 : 0;
    for (int c = t; c < chunks; c += 1024) {
        const uint4 v = reinterpret_cast<const uint4 *>(m)[c];
        if ((v.x | v.y | v.z | v.w) == 0u) continue;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        for (int k = 0; k < 16; k++)
            if ((w[k >> 2] >> (8 * (k & 3))) & 0xffu) hit(16 * c + k);
    }
    for (int idx = 16 * chunks + t; idx < HW; idx += 1024)
        if (m[idx]) hit(idx);
    if (x1 >= 0) {                            // integer min / max: the order of the lanes does not reach the result
        atomicMin(&s_box[0], x0); atomicMin(&s_box[1], y0); atomicMax(&s_box[2], x1); atomicMax(&s_box[3], y1);
    }
    __syncthreads();
    if (t < 4) boxes[4 * blockIdx.x + t] = s_box[t];
}

// ---- crops --------------------------------------------------------------------------------------------------------------------
// torch.linspace(start, end, CROP)[i] on the CPU: one fused multiply-add from the nearer end
__device__ inline float linspace_at(float start, float end, int i)
{
    const float step = (end - start) / (float)(CROP - 1);
    return i < CROP / 2 ? fmaf(step, (float)i, start) : fmaf(-step, (float)(CROP - 1 - i), end);
}

// the position F.grid_sample(align_corners=False) samples for the reference's grid value lin / size * 2 - 1
__device__ inline float crop_position(float lin, int size)
{
    float g = lin / (float)size;
    g = g * 2.0f;
    g = g - 1.0f;
    return fmaf(g + 1.0f, (float)size / 2.0f, -0.5f);
}

__global__ void __launch_bounds__(THREADS) crops_kernel(int H, int W, const uint8_t *__restrict__ images, const uint8_t *__restrict__ masks,
                                                        const int32_t *__restrict__ boxes, float *__restrict__ rgb_crop,
                                                        float *__restrict__ mask_crop)
{
    const int n = blockIdx.y;
    const int idx = blockIdx.x * THREADS + threadIdx.x;          // < CROP * CROP (the grid is exact)
    const int v = idx / CROP, u = idx - v * CROP;
    const size_t out = (size_t)n * CROP * CROP + idx;
    const int bx0 = boxes[4 * n], by0 = boxes[4 * n + 1], bx1 = boxes[4 * n + 2], by1 = boxes[4 * n + 3];
    float r = 0.f, g = 0.f, b = 0.f, a = 0.f;
    if (bx1 >= bx0 && by1 >= by0) {
        const float cx = (float)bx0 + (float)(bx1 - bx0) / 2.0f, cy = (float)by0 + (float)(by1 - by0) / 2.0f;
        const float hs = (float)((double)max(bx1 - bx0, by1 - by0) * 1.1 / 2.0);
        const float x = crop_position(linspace_at(cx - hs, cx + hs, u), W);
        const float y = crop_position(linspace_at(cy - hs, cy + hs, v), H);
        const float xw = floorf(x), yn = floorf(y);
        const float w = x - xw, e = 1.0f - w, nn = y - yn, s = 1.0f - nn;
        const float wt[4] = {e * s, w * s, e * nn, w * nn};      // nw, ne, sw, se
        const int ix = (int)xw, iy = (int)yn;
        const uint8_t *img = images + (size_t)n * H * W * 3;
        const uint8_t *msk = masks + (size_t)n * H * W;
        float tr[4], tg[4], tb[4], ta[4];
        for (int k = 0; k < 4; k++) {
            const int px = ix + (k & 1), py = iy + (k >> 1);
            tr[k] = tg[k] = tb[k] = ta[k] = 0.f;
            if (px >= 0 && px < W && py >= 0 && py < H) {
                const size_t p = (size_t)py * W + px;
                const float m = (float)msk[p];
                ta[k] = m;
                tr[k] = (float)img[3 * p] / 255.0f * m;
                tg[k] = (float)img[3 * p + 1] / 255.0f * m;
                tb[k] = (float)img[3 * p + 2] / 255.0f * m;
            }
        }
        r = tr[0] * wt[0] + tr[1] * wt[1] + tr[2] * wt[2] + tr[3] * wt[3];
        g = tg[0] * wt[0] + tg[1] * wt[1] + tg[2] * wt[2] + tg[3] * wt[3];
        b = tb[0] * wt[0] + tb[1] * wt[1] + tb[2] * wt[2] + tb[3] * wt[3];
        a = ta[0] * wt[0] + ta[1] * wt[1] + ta[2] * wt[2] + ta[3] * wt[3];
    }
    rgb_crop[3 * out] = r; rgb_crop[3 * out + 1] = g; rgb_crop[3 * out + 2] = b;
    mask_crop[out] = a;
}

// ---- the step's batch ---------------------------------------------------------------------------------------------------------
enum Job { J_RAYS, J_GT_RAYS, J_RGB, J_MASK, J_NORMAL_F, J_NORMAL_B, J_NORMAL_MASK, J_RGB_CROP, J_MASK_CROP, J_SMALL, N_JOBS };
struct Jobs {
    int32_t first[N_JOBS + 1];    // the workgroups [first[j], first[j + 1]) belong to job j
    int32_t vec_rgb, vec_mask, vec_nf, vec_nb, vec_nm;       // 16-byte loads allowed (the frame's row starts on a 16-byte boundary)
};

union alignas(16) Stage {
    float rays[2][3 * THREADS];                              // cam_d, rays_d of 256 pixels
    struct { uint8_t src[CONV_BYTES]; uint8_t mask[MASK_STAGE]; } conv;
};

struct RayCam {
    float cx, cy, fx, fy;
    float R[9];
};

// 256 pixels per round: every lane computes one pixel into LDS, then neighbouring lanes store neighbouring 16 bytes
__device__ void rays_block(Stage &st, int blk, int n_views, int H, int W, const RayCam *cams, bool normalize, float *__restrict__ cam_d,
                           float *__restrict__ rays_d)
{
    const int t = threadIdx.x;
    const int HW = H * W;
    const int total = n_views * HW;
    for (int round = 0; round < RAY_PIX / THREADS; round++) {
        const int base = blk * RAY_PIX + round * THREADS;
        if (base >= total) break;                            // (uniform)
        const int p = base + t;
        if (p < total) {
            const int b = p / HW, r = p - b * HW, j = r / W, i = r - j * W;
            const RayCam &c = cams[b];
            float d[3];
            d[0] = (((float)i + 0.5f) - c.cx) / c.fx;
            d[1] = -((((float)j + 0.5f) - c.cy) / c.fy);
            d[2] = -1.0f;
            float o[3];
            for (int k = 0; k < 3; k++) o[k] = d[0] * c.R[3 * k] + d[1] * c.R[3 * k + 1] + d[2] * c.R[3 * k + 2];
            if (normalize) {
                const float len = fmaxf(sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]), 1e-12f);
                for (int k = 0; k < 3; k++) o[k] = o[k] / len;
            }
            for (int k = 0; k < 3; k++) { st.rays[0][3 * t + k] = d[k]; st.rays[1][3 * t + k] = o[k]; }
        }
        __syncthreads();
        const int floats = 3 * min(THREADS, total - base);
        float *dst[2] = {cam_d, rays_d};
        for (int a = 0; a < 2; a++) {
            if (!dst[a] || 4 * t >= floats) continue;
            float *out = dst[a] + (size_t)3 * base + 4 * t;
            if (4 * t + 4 <= floats) *reinterpret_cast<float4 *>(out) = *reinterpret_cast<const float4 *>(&st.rays[a][4 * t]);
            else for (int k = 0; 4 * t + k < floats; k++) out[k] = st.rays[a][4 * t + k];
        }
        __syncthreads();
    }
}

// n source bytes -> n floats: byte [/ 255] [* mask byte of pixel index / 3].  One workgroup takes CONV_BYTES bytes.
__device__ void convert_block(Stage &st, int blk, const uint8_t *__restrict__ src, int64_t n, bool vec, const uint8_t *__restrict__ mask,
                              bool vec_mask, bool div255, float *__restrict__ dst)
{
    const int t = threadIdx.x;
    const int64_t t0 = (int64_t)blk * CONV_BYTES;
    const int cnt = (int)(n - t0 < CONV_BYTES ? n - t0 : CONV_BYTES);
    if (vec && 16 * t + 16 <= cnt) {
        *reinterpret_cast<uint4 *>(&st.conv.src[16 * t]) = *reinterpret_cast<const uint4 *>(src + t0 + 16 * t);
    } else {
        for (int k = 0; k < 16; k++) st.conv.src[16 * t + k] = 16 * t + k < cnt ? src[t0 + 16 * t + k] : (uint8_t)0;
    }
    const int64_t n_mask = n / 3;
    const int64_t m_base = (t0 / 3) & ~(int64_t)15;          // the first staged mask byte
    const int rem = (int)(t0 - 3 * m_base);                 // source byte e of this block belongs to staged mask byte (rem + e) / 3
    if (mask) {
        const int m_cnt = (rem + cnt - 1) / 3 + 1;          // staged mask bytes in use
        if (16 * t < m_cnt) {
            const int64_t at = m_base + 16 * t;
            if (vec_mask && at + 16 <= n_mask) {
                *reinterpret_cast<uint4 *>(&st.conv.mask[16 * t]) = *reinterpret_cast<const uint4 *>(mask + at);
            } else {
                for (int k = 0; k < 16; k++) st.conv.mask[16 * t + k] = at + k < n_mask ? mask[at + k] : (uint8_t)0;
            }
        }
    }
    __syncthreads();
    for (int q = 0; q < CONV_BYTES / (4 * THREADS); q++) {
        const int e = 4 * (q * THREADS + t);
        if (e >= cnt) break;
        const uint32_t w = *reinterpret_cast<const uint32_t *>(&st.conv.src[e]);
        float v[4];
        for (int k = 0; k < 4; k++) {
            v[k] = (float)((w >> (8 * k)) & 0xffu);
            if (div255) v[k] = v[k] / 255.0f;
            if (mask) v[k] = v[k] * (float)st.conv.mask[(rem + e + k) / 3];
        }
        float *out = dst + t0 + e;
        if (e + 4 <= cnt) *reinterpret_cast<float4 *>(out) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int k = 0; e + k < cnt; k++) out[k] = v[k];
    }
}

__device__ void copy_block(int blk, const float *__restrict__ src, int64_t n, float *__restrict__ dst)
{
    const int64_t t0 = (int64_t)blk * COPY_FLOATS;
    for (int q = 0; q < COPY_FLOATS / (4 * THREADS); q++) {
        const int64_t e = t0 + 4 * (q * THREADS + (int)threadIdx.x);
        if (e >= n) break;
        if (e + 4 <= n) *reinterpret_cast<float4 *>(dst + e) = *reinterpret_cast<const float4 *>(src + e);
        else for (int k = 0; e + k < n; k++) dst[e + k] = src[e + k];
    }
}

// proj @ [R^T | -R^T t] of one camera (threestudio's get_projection_matrix[_cxcy] and get_mvp_matrix)
__device__ void write_mvp(const float *c2w, float tan_half, double aspect, double near, double far, bool cxcy, float cx, float cy, int Wi, int Hi,
                          float *proj_out, float *mvp_out)
{
    float P[16], V[16];
    for (int k = 0; k < 16; k++) { P[k] = 0.f; V[k] = 0.f; }
    P[0] = 1.0f / (tan_half * (float)aspect);
    P[5] = -1.0f / tan_half;
    P[10] = (float)(-(far + near) / (far - near));
    P[11] = (float)(-2.0 * far * near / (far - near));
    P[14] = -1.0f;
    if (cxcy) {
        P[2] = (float)(-(2.0 * (double)cx - Wi) / Wi);
        P[6] = (float)(-(2.0 * (double)cy - Hi) / Hi);
    }
    for (int i = 0; i < 3; i++) {
        float acc = 0.f;
        for (int k = 0; k < 3; k++) {
            V[4 * i + k] = c2w[4 * k + i];
            acc = acc + (-c2w[4 * k + i]) * c2w[4 * k + 3];
        }
        V[4 * i + 3] = acc;
    }
    V[15] = 1.0f;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            float acc = 0.f;
            for (int k = 0; k < 4; k++) acc = acc + P[4 * i + k] * V[4 * k + j];
            mvp_out[4 * i + j] = acc;
        }
    if (proj_out)
        for (int k = 0; k < 16; k++) proj_out[k] = P[k];
}

__global__ void __launch_bounds__(THREADS) step_batch_kernel(const SoarDataStepArgs a, const Jobs jobs)
{
    __shared__ Stage st;
    __shared__ RayCam cams[SOAR_DATA_MAX_VIEWS];
    int job = 0;
    while (job + 1 < N_JOBS && (int)blockIdx.x >= jobs.first[job + 1]) job++;            // (uniform)
    const int blk = blockIdx.x - jobs.first[job];
    const int t = threadIdx.x;
    const size_t frame = (size_t)a.frame;
    const int64_t HWv = (int64_t)a.Hv * a.Wv;
    const int64_t NPIX = (int64_t)CROP * CROP;
    switch (job) {
    case J_RAYS:
        if (t < a.B) {
            RayCam &c = cams[t];
            c.cx = (float)a.W * 0.5f; c.cy = (float)a.H * 0.5f; c.fx = c.fy = a.focal[t];
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) c.R[3 * r + k] = a.c2w[t][4 * r + k];
        }
        __syncthreads();
        rays_block(st, blk, a.B, a.H, a.W, cams, a.rays_d_normalize != 0, a.cam_d, a.rays_d);
        break;
    case J_GT_RAYS:
        if (t == 0) {
            RayCam &c = cams[0];
            const float *K = a.normal_Ks + 9 * frame;
            c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5];
            for (int r = 0; r < 3; r++)
                for (int k = 0; k < 3; k++) c.R[3 * r + k] = a.gt_c2w[4 * r + k];
        }
        __syncthreads();
        rays_block(st, blk, 1, CROP, CROP, cams, true, a.gt_cam_d, a.gt_rays_d);
        break;
    case J_RGB:
        convert_block(st, blk, a.images + frame * HWv * 3, HWv * 3, jobs.vec_rgb, a.masks + frame * HWv, jobs.vec_mask, true, a.gt_rgb);
        break;
    case J_MASK:
        convert_block(st, blk, a.masks + frame * HWv, HWv, jobs.vec_mask, nullptr, false, false, a.gt_mask);
        break;
    case J_NORMAL_F:
        convert_block(st, blk, a.normal_F + frame * NPIX * 3, NPIX * 3, jobs.vec_nf, nullptr, false, true, a.gt_normal_F);
        break;
    case J_NORMAL_B:
        convert_block(st, blk, a.normal_B + frame * NPIX * 3, NPIX * 3, jobs.vec_nb, nullptr, false, true, a.gt_normal_B);
        break;
    case J_NORMAL_MASK:
        convert_block(st, blk, a.normal_mask + frame * NPIX, NPIX, jobs.vec_nm, nullptr, false, true, a.gt_normal_mask);
        break;
    case J_RGB_CROP:
        copy_block(blk, a.rgb_crop + frame * NPIX * 3, NPIX * 3, a.gt_rgb_crop);
        break;
    case J_MASK_CROP:
        copy_block(blk, a.mask_crop + frame * NPIX, NPIX, a.gt_mask_crop);
        break;
    default:
        if (a.small_out)
            for (int k = t; k < a.n_small; k += THREADS) a.small_out[k] = a.small[k];
        if (a.mvp_mtx && t < a.B)
            write_mvp(a.c2w[t], a.tan_half[t], (double)a.W / (double)a.H, a.near_plane, a.far_plane, false, 0.f, 0.f, 1, 1,
                      a.proj ? a.proj + 16 * t : nullptr, a.mvp_mtx + 16 * t);
        if (a.gt_mvp_mtx && t == SOAR_DATA_MAX_VIEWS)
            write_mvp(a.gt_c2w, a.gt_tan_half, (double)a.Wv / (double)a.Hv, a.gt_near, 1000.0, a.gt_has_cxcy != 0, a.gt_cx, a.gt_cy, a.Wv, a.Hv,
                      nullptr, a.gt_mvp_mtx);
        break;
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline int blocks_of(int64_t n, int per) { return (int)((n + per - 1) / per); }

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_data_mask_bbox(int32_t N, int32_t H, int32_t W, const uint8_t *masks, int32_t *boxes, void *stream_)
{
    if (N < 0 || H < 1 || W < 1 || (int64_t)H * W > (1 << 30)) {
        set_error("soar_data_mask_bbox: bad arguments (N=%d, H=%d, W=%d; need N >= 0 and 1 <= H W <= 2^30)", N, H, W);
        return 1;
    }
    if (N == 0) return 0;
    if (!masks || !boxes) { set_error("soar_data_mask_bbox: NULL masks / boxes"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int vec = aligned16(masks) && ((int64_t)H * W) % 16 == 0;
    hipLaunchKernelGGL(mask_bbox_kernel, dim3(N), dim3(1024), 0, stream, H, W, masks, boxes, vec);
    SOAR_LAUNCH_OK("data_mask_bbox", stream, 0);
    return 0;
}

int soar_data_crops(int32_t N, int32_t H, int32_t W, const uint8_t *images, const uint8_t *masks, const int32_t *boxes, float *rgb_crop,
                    float *mask_crop, void *stream_)
{
    if (N < 0 || H < 1 || W < 1 || (int64_t)H * W > (1 << 30)) {
        set_error("soar_data_crops: bad arguments (N=%d, H=%d, W=%d; need N >= 0 and 1 <= H W <= 2^30)", N, H, W);
        return 1;
    }
    if (N == 0) return 0;
    if (!images || !masks || !boxes || !rgb_crop || !mask_crop) { set_error("soar_data_crops: NULL images / masks / boxes / output"); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    for (int n0 = 0; n0 < N; n0 += 32768) {                  // (gridDim.y)
        const int n = N - n0 < 32768 ? N - n0 : 32768;
        hipLaunchKernelGGL(crops_kernel, dim3(CROP * CROP / THREADS, n), dim3(THREADS), 0, stream, H, W, images + (size_t)n0 * H * W * 3,
                           masks + (size_t)n0 * H * W, boxes + 4 * (size_t)n0, rgb_crop + (size_t)n0 * CROP * CROP * 3,
                           mask_crop + (size_t)n0 * CROP * CROP);
        SOAR_LAUNCH_OK("data_crops", stream, 0);
    }
    return 0;
}

int soar_data_step_batch(const SoarDataStepArgs *args, void *stream_)
{
    const char *me = "soar_data_step_batch";
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarDataStepArgs &a = *args;
    if (a.B < 0 || a.B > SOAR_DATA_MAX_VIEWS) { set_error("%s: need 0 <= B <= %d views (B=%d)", me, SOAR_DATA_MAX_VIEWS, a.B); return 1; }
    const bool rays = a.B > 0 && (a.rays_d || a.cam_d);
    if (rays && (a.H < 1 || a.W < 1 || (int64_t)a.B * a.H * a.W > (1 << 28))) {
        set_error("%s: zero-size or oversized view (H=%d, W=%d; need 1 <= B H W <= 2^28)", me, a.H, a.W);
        return 1;
    }
    if (a.B > 0 && a.mvp_mtx && (a.H < 1 || a.W < 1)) { set_error("%s: zero-size view (H=%d, W=%d)", me, a.H, a.W); return 1; }
    const bool gt_rays = a.gt_rays_d || a.gt_cam_d;
    const bool frame_wanted = gt_rays || a.gt_rgb || a.gt_mask || a.gt_normal_F || a.gt_normal_B || a.gt_normal_mask || a.gt_rgb_crop ||
                              a.gt_mask_crop;
    if (frame_wanted && (a.frame < 0 || a.frame >= a.n_frames)) {
        set_error("%s: frame index %d out of range (n_frames=%d)", me, a.frame, a.n_frames);
        return 1;
    }
    if ((a.gt_rgb || a.gt_mask || a.gt_mvp_mtx) && (a.Hv < 1 || a.Wv < 1 || (int64_t)a.Hv * a.Wv > (1 << 28))) {
        set_error("%s: zero-size or oversized video image (Hv=%d, Wv=%d; need 1 <= Hv Wv <= 2^28)", me, a.Hv, a.Wv);
        return 1;
    }
    if (a.n_small < 0 || a.n_small > SOAR_DATA_SMALL_FLOATS) { set_error("%s: need 0 <= n_small <= %d (n_small=%d)", me, SOAR_DATA_SMALL_FLOATS, a.n_small); return 1; }
    if (a.B > 0 && a.mvp_mtx && !(a.far_plane > a.near_plane)) { set_error("%s: need far_plane > near_plane", me); return 1; }
    if (gt_rays && !a.normal_Ks) { set_error("%s: NULL normal_Ks", me); return 1; }
    if ((a.gt_rgb && (!a.images || !a.masks)) || (a.gt_mask && !a.masks) || (a.gt_normal_F && !a.normal_F) || (a.gt_normal_B && !a.normal_B) ||
        (a.gt_normal_mask && !a.normal_mask) || (a.gt_rgb_crop && !a.rgb_crop) || (a.gt_mask_crop && !a.mask_crop)) {
        set_error("%s: NULL source of a wanted output (images / masks / normal_F / normal_B / normal_mask / rgb_crop / mask_crop)", me);
        return 1;
    }
    const void *outs[] = {a.rays_d, a.cam_d, a.gt_rays_d, a.gt_cam_d, a.gt_rgb, a.gt_mask, a.gt_normal_F, a.gt_normal_B, a.gt_normal_mask,
                          a.gt_rgb_crop, a.gt_mask_crop, a.rgb_crop, a.mask_crop};
    for (const void *p : outs)
        if (!aligned16(p)) { set_error("%s: the float images must be 16-byte aligned", me); return 1; }
    const int64_t HWv = (int64_t)a.Hv * a.Wv, NPIX = (int64_t)CROP * CROP;
    Jobs jobs;
    int32_t n[N_JOBS];
    n[J_RAYS] = rays ? blocks_of((int64_t)a.B * a.H * a.W, RAY_PIX) : 0;
    n[J_GT_RAYS] = gt_rays ? blocks_of(NPIX, RAY_PIX) : 0;
    n[J_RGB] = a.gt_rgb ? blocks_of(HWv * 3, CONV_BYTES) : 0;
    n[J_MASK] = a.gt_mask ? blocks_of(HWv, CONV_BYTES) : 0;
    n[J_NORMAL_F] = a.gt_normal_F ? blocks_of(NPIX * 3, CONV_BYTES) : 0;
    n[J_NORMAL_B] = a.gt_normal_B ? blocks_of(NPIX * 3, CONV_BYTES) : 0;
    n[J_NORMAL_MASK] = a.gt_normal_mask ? blocks_of(NPIX, CONV_BYTES) : 0;
    n[J_RGB_CROP] = a.gt_rgb_crop ? blocks_of(NPIX * 3, COPY_FLOATS) : 0;
    n[J_MASK_CROP] = a.gt_mask_crop ? blocks_of(NPIX, COPY_FLOATS) : 0;
    n[J_SMALL] = ((a.small_out && a.n_small > 0) || (a.B > 0 && a.mvp_mtx) || a.gt_mvp_mtx) ? 1 : 0;
    jobs.first[0] = 0;
    for (int j = 0; j < N_JOBS; j++) jobs.first[j + 1] = jobs.first[j] + n[j];
    // a frame's rows start on a 16-byte boundary when the array does and the frame's size is a multiple of 16
    jobs.vec_rgb = aligned16(a.images) && (HWv * 3) % 16 == 0;
    jobs.vec_mask = aligned16(a.masks) && HWv % 16 == 0;
    jobs.vec_nf = aligned16(a.normal_F);
    jobs.vec_nb = aligned16(a.normal_B);
    jobs.vec_nm = aligned16(a.normal_mask);
    if (jobs.first[N_JOBS] == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(step_batch_kernel, dim3(jobs.first[N_JOBS]), dim3(THREADS), 0, stream, a, jobs);
    SOAR_LAUNCH_OK("data_step_batch", stream, 0);
    return 0;
}

}  // extern "C"
