// eval.hip -- test-split evaluation (soar_amd/evaluate.py): what the reference's test_step computes on the host with
// skimage, in one pass over the pixels on the device.
//   soar_eval_image_metrics   per image: the white-composited target, PSNR (skimage's arithmetic: float32 difference and square,
//                             float64 sum), structural_similarity(channel_axis=-1, data_range=1) (7x7 uniform window, sample
//                             covariance, float64), the two LPIPS inputs x * 2 - 1 and, when asked for, the side-by-side byte image
// One workgroup per TILE_H x TILE_W block of pixels.  It stages the block and the 6 further rows and columns that the windows
// starting inside it reach (the 3-pixel halo on either side of a window's centre) in LDS as float32, writes the per-pixel outputs of
// its own pixels, then every thread walks one (column, channel) down the rows: the 7-tap row sums of x, y, xx, yy, xy in float64,
// the last 7 of them kept in registers, their sum is the window's.  No float atomics: a workgroup leaves four float64 partial sums
// in the caller's scratch, a second small kernel adds them per image in a fixed order.
// Compiled with -ffp-contract=off: the values are pinned on a NumPy restatement (tests/eval_ref.py).
#include "workspace.h"

namespace soar {
namespace {

constexpr int TILE_H = 16, TILE_W = 64;                    // pixels (= window origins) of a workgroup
constexpr int WIN = 7, HALO = WIN - 1;
constexpr int ROWS = TILE_H + HALO, COLS = TILE_W + HALO;  // staged pixels
constexpr int ROW_F = COLS * 3;                            // floats of a staged row (channels interleaved, as in memory)
constexpr int THREADS = TILE_W * 3;                        // one thread per (column, channel) of the tile: 3 wavefronts
constexpr int WAVES = THREADS / WAVE;
constexpr int FIN_THREADS = 256;
constexpr double C1 = 1e-4, C2 = 9e-4;                     // (0.01 * data_range)^2, (0.03 * data_range)^2
static_assert(THREADS % WAVE == 0, "whole wavefronts");

struct EvalDev {
    int32_t H, W;
    const float *pred, *gt_rgb, *gt_mask;
    int64_t ps[4], gs[4], ms[3];
    float *gt_white, *pred2, *gt2;
    uint8_t *grid;
    double *partials;                                      // [N][tiles][4]: SSE, SSIM sums of the three channels
};

__device__ __forceinline__ uint8_t to_byte(float v)
{
    return (uint8_t)(int)(fminf(fmaxf(v, 0.f), 1.f) * 255.f);          // clip(0, 1) * 255, truncated (astype(np.uint8))
}

// fixed-order sum over the 64 lanes (the same tree in every run); lane 0 holds the result
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, WAVE);
    return v;
}

__global__ void __launch_bounds__(THREADS) eval_tile_kernel(EvalDev a)
{
    __shared__ float sx[ROWS * ROW_F], sy[ROWS * ROW_F];
    __shared__ double s_part[WAVES][4];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const int H = a.H, W = a.W;

    // ---- stage the tile; the per-pixel outputs and the squared error of the pixels this workgroup owns ----
    double sse = 0.0;
    for (int e = tid; e < ROWS * ROW_F; e += THREADS) {
        const int ly = e / ROW_F, rem = e - ly * ROW_F, lx = rem / 3, c = rem - lx * 3;
        const int gy = y0 + ly, gx = x0 + lx;
        float p = 0.f, gw = 0.f;
        if (gy < H && gx < W) {
            p = a.pred[n * a.ps[0] + gy * a.ps[1] + gx * a.ps[2] + c * a.ps[3]];
            const float g = a.gt_rgb[n * a.gs[0] + gy * a.gs[1] + gx * a.gs[2] + c * a.gs[3]];
            const float m = a.gt_mask[n * a.ms[0] + gy * a.ms[1] + gx * a.ms[2]];
            gw = m > 0.5f ? g : 1.0f;
            if (ly < TILE_H && lx < TILE_W) {
                const int64_t row = (int64_t)n * H + gy;
                const int64_t o = (row * W + gx) * 3 + c;
                a.gt_white[o] = gw;
                a.pred2[o] = p * 2.f - 1.f;
                a.gt2[o] = gw * 2.f - 1.f;
                if (a.grid) {
                    const int64_t q = (row * 2 * W + gx) * 3 + c;
                    a.grid[q] = to_byte(p);
                    a.grid[q + (int64_t)W * 3] = to_byte(gw);
                }
                const float d = gw - p;
                sse += (double)(d * d);
            }
        }
        sx[e] = p;
        sy[e] = gw;
    }
    __syncthreads();

    // ---- windows: thread = (column j, channel c) of the tile, walking down the staged rows ----
    const int c = tid % 3;
    const bool col_ok = x0 + tid / 3 <= W - WIN;
    double ring[WIN][5];
    double ssum = 0.0;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        double h[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < WIN; t++) {
            const double x = (double)sx[r * ROW_F + tid + 3 * t], y = (double)sy[r * ROW_F + tid + 3 * t];
            h[0] += x; h[1] += y; h[2] += x * x; h[3] += y * y; h[4] += x * y;
        }
#pragma unroll
        for (int k = 0; k < 5; k++) ring[r % WIN][k] = h[k];
        if (r >= HALO) {
            double w[5];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                w[k] = ring[(r - HALO) % WIN][k];
#pragma unroll
                for (int i = 1; i < WIN; i++) w[k] += ring[(r - HALO + i) % WIN][k];
                w[k] /= 49.0;
            }
            const double ux = w[0], uy = w[1];
            const double cov = 49.0 / 48.0;
            const double vx = cov * (w[2] - ux * ux), vy = cov * (w[3] - uy * uy), vxy = cov * (w[4] - ux * uy);
            const double S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
            if (col_ok && y0 + (r - HALO) <= H - WIN) ssum += S;
        }
    }

    // ---- the workgroup's four partial sums, in a fixed order ----
    double v[4] = {sse, c == 0 ? ssum : 0.0, c == 1 ? ssum : 0.0, c == 2 ? ssum : 0.0};
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = wave_sum(v[k]);
    if (tid % WAVE == 0)
        for (int k = 0; k < 4; k++) s_part[tid / WAVE][k] = v[k];
    __syncthreads();
    if (tid < 4) {
        double t = s_part[0][tid];
        for (int w = 1; w < WAVES; w++) t += s_part[w][tid];
        const int64_t tile = ((int64_t)n * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.partials[tile * 4 + tid] = t;
    }
}

// one workgroup per image: the tiles' partial sums in a fixed order, then metrics[n] = {psnr, ssim, mse}
__global__ void __launch_bounds__(FIN_THREADS) eval_finish_kernel(const double *__restrict__ partials, int tiles, int H, int W,
                                                                  double *__restrict__ metrics)
{
    __shared__ double s[FIN_THREADS][4];
    const int tid = threadIdx.x, n = blockIdx.x;
    const double *p = partials + (int64_t)n * tiles * 4;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = tid; t < tiles; t += FIN_THREADS)
        for (int k = 0; k < 4; k++) v[k] += p[(int64_t)t * 4 + k];
    for (int k = 0; k < 4; k++) s[tid][k] = v[k];
    __syncthreads();
    for (int half = FIN_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half)
            for (int k = 0; k < 4; k++) s[tid][k] += s[tid + half][k];
        __syncthreads();
    }
    if (tid == 0) {
        const double mse = s[0][0] / (3.0 * (double)H * (double)W);
        const double windows = (double)(H - HALO) * (double)(W - HALO);
        const double ssim = (s[0][1] / windows + s[0][2] / windows + s[0][3] / windows) / 3.0;
        metrics[n * 3 + 0] = 10.0 * log10(1.0 / mse);                   // +inf when mse == 0
        metrics[n * 3 + 1] = ssim;
        metrics[n * 3 + 2] = mse;
    }
}

inline int64_t tiles_of(int32_t H, int32_t W)
{
    return (int64_t)((H + TILE_H - 1) / TILE_H) * ((W + TILE_W - 1) / TILE_W);
}

// H, W >= 7 (a 7x7 window must fit: skimage raises otherwise), 1 <= N <= 65535 (gridDim.z), N H W <= 2^30
inline bool sizes_ok(int32_t N, int32_t H, int32_t W)
{
    return N >= 1 && N <= 65535 && H >= WIN && W >= WIN && (int64_t)N * H * W <= (1 << 30);
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_eval_scratch_bytes(int32_t N, int32_t H, int32_t W, size_t *bytes)
{
    if (!bytes || !sizes_ok(N, H, W)) {
        set_error("soar_eval_scratch_bytes: bad arguments (N=%d, H=%d, W=%d; need 1 <= N <= 65535, H, W >= 7, N H W <= 2^30)", N, H, W);
        return 1;
    }
    *bytes = align_up((size_t)N * (size_t)tiles_of(H, W) * 4 * sizeof(double));
    return 0;
}

int soar_eval_image_metrics(const SoarEvalArgs *args, void *scratch, size_t scratch_bytes, void *stream_)
{
    const char *me = "soar_eval_image_metrics";
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarEvalArgs &a = *args;
    if (!sizes_ok(a.N, a.H, a.W)) {
        set_error("%s: bad arguments (N=%d, H=%d, W=%d; need 1 <= N <= 65535, H, W >= 7 for one 7x7 window, N H W <= 2^30)", me, a.N, a.H, a.W);
        return 1;
    }
    if (!a.pred || !a.gt_rgb || !a.gt_mask) { set_error("%s: NULL pred / gt_rgb / gt_mask", me); return 1; }
    if (!a.gt_white || !a.pred2 || !a.gt2 || !a.metrics) { set_error("%s: NULL gt_white / pred2 / gt2 / metrics", me); return 1; }
    size_t need = 0;
    if (soar_eval_scratch_bytes(a.N, a.H, a.W, &need)) return 1;
    if (!workspace_ok(me, scratch, scratch_bytes, need, "soar_eval_scratch_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    EvalDev d;
    d.H = a.H; d.W = a.W;
    d.pred = a.pred; d.gt_rgb = a.gt_rgb; d.gt_mask = a.gt_mask;
    for (int i = 0; i < 4; i++) { d.ps[i] = a.pred_stride[i]; d.gs[i] = a.gt_stride[i]; }
    for (int i = 0; i < 3; i++) d.ms[i] = a.mask_stride[i];
    d.gt_white = a.gt_white; d.pred2 = a.pred2; d.gt2 = a.gt2; d.grid = a.grid;
    d.partials = static_cast<double *>(scratch);
    const dim3 grid((a.W + TILE_W - 1) / TILE_W, (a.H + TILE_H - 1) / TILE_H, a.N);
    hipLaunchKernelGGL(eval_tile_kernel, grid, dim3(THREADS), 0, stream, d);
    SOAR_LAUNCH_OK("eval_tile", stream, 0);
    hipLaunchKernelGGL(eval_finish_kernel, dim3(a.N), dim3(FIN_THREADS), 0, stream, d.partials, (int)tiles_of(a.H, a.W), a.H, a.W, a.metrics);
    SOAR_LAUNCH_OK("eval_finish", stream, 0);
    return 0;
}

}  // extern "C"
