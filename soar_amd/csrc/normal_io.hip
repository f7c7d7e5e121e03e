// normal_io.hip -- what stands in front of and behind the normal networks (soar_amd/normals.py; include/soar_hip.h):
//
//   normal_box_kernel      one workgroup per frame: the bounding box of the non-zero mask pixels, the square crop box of 1.1 x its
//                          longer side around its centre, the crop's intrinsics and a status word (empty mask); nothing is read back
//   normal_crop_kernel     S x S bilinear samples (grid-sample arithmetic, align_corners = False, zeros outside) of
//                          (rgb / 255 * 2 - 1) * mask / 255 and of mask / 255, all frames in one launch
//   normal_bytes_kernel    trunc(((n + 1) / 2 * mask) * 255) and trunc(mask * 255) as bytes: float32 operations in exactly that
//                          order (this file is built without FMA contraction), so the bytes are those of the torch composition
//
// The box and the sample positions are worked out in double from the integer bounding box: the float32 results then do not depend
// on the order of a float32 evaluation (torch's own linspace differs between its CPU and GPU kernels in the last bit).
#include "soar_common.h"

namespace soar {

namespace {

struct BoxK {
    const uint8_t *mask;           // [N][H][W] at ms (bytes)
    int64_t ms[3];
    const float *Ks;               // [N][3][3]
    double *boxes;                 // [N][4]: x1, y1, x2, y2 (pixel coordinates, may leave the image)
    float *normal_Ks;              // [N][3][3]
    int32_t *status;               // [N]: 0, 1 = empty mask, 2 = the mask's box has no extent
    int H, W, S;
};
__global__ void __launch_bounds__(256) normal_box_kernel(BoxK k)
{
    __shared__ int sh[4][256];
    const int n = blockIdx.x, t = threadIdx.x;
    int x0 = k.W, y0 = k.H, x1 = -1, y1 = -1;
    const uint8_t *m = k.mask + n * k.ms[0];
    const int hw = k.H * k.W;
    for (int q = t; q < hw; q += 256) {
        const int y = q / k.W, x = q - y * k.W;
        if (m[y * k.ms[1] + x * k.ms[2]]) {
            x0 = min(x0, x); y0 = min(y0, y); x1 = max(x1, x); y1 = max(y1, y);
        }
    }
    sh[0][t] = x0; sh[1][t] = y0; sh[2][t] = x1; sh[3][t] = y1;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (t < s) {
            sh[0][t] = min(sh[0][t], sh[0][t + s]);
            sh[1][t] = min(sh[1][t], sh[1][t + s]);
            sh[2][t] = max(sh[2][t], sh[2][t + s]);
            sh[3][t] = max(sh[3][t], sh[3][t + s]);
        }
        __syncthreads();
    }
    if (t != 0) return;
    x0 = sh[0][0]; y0 = sh[1][0]; x1 = sh[2][0]; y1 = sh[3][0];
    int st = 0;
    if (x1 < 0) { st = 1; x0 = 0; y0 = 0; x1 = k.W; y1 = k.H; }              // the whole frame stands in: every later index stays valid
    else if (x1 == x0 && y1 == y0) { st = 2; x1 = x0 + 1; y1 = y0 + 1; }
    const double cx = x0 + (x1 - x0) / 2.0, cy = y0 + (y1 - y0) / 2.0;
    const double half = max(x1 - x0, y1 - y0) * 1.1 / 2.0;
    const double bx1 = cx - half, by1 = cy - half, bx2 = cx + half, by2 = cy + half;
    double *b = k.boxes + (size_t)n * 4;
    b[0] = bx1; b[1] = by1; b[2] = bx2; b[3] = by2;
    const float *K = k.Ks + (size_t)n * 9;
    const double sx = (double)k.S / (bx2 - bx1), sy = (double)k.S / (by2 - by1);
    float *o = k.normal_Ks + (size_t)n * 9;
    o[0] = (float)(sx * (double)K[0]); o[1] = 0.f; o[2] = (float)(sx * ((double)K[2] - bx1));
    o[3] = 0.f; o[4] = (float)(sy * (double)K[4]); o[5] = (float)(sy * ((double)K[5] - by1));
    o[6] = 0.f; o[7] = 0.f; o[8] = 1.f;
    k.status[n] = st;
}

struct CropK {
    const uint8_t *img;            // [N][H][W][3] at is (bytes)
    const uint8_t *mask;
    int64_t is[4], ms[3];
    const double *boxes;
    float *out_img;                // [N][3][S][S]
    float *out_mask;               // [N][S][S]
    int64_t total;                 // N S S
    int H, W, S;
};
__global__ void __launch_bounds__(256) normal_crop_kernel(CropK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.total) return;
    const int64_t ss = (int64_t)k.S * k.S;
    const int64_t n = e / ss;
    const int q = (int)(e - n * ss), jy = q / k.S, jx = q - jy * k.S;
    const double *b = k.boxes + (size_t)n * 4;
    // the grid's pixel coordinate x1 + (x2 - x1) j / (S - 1); as a normalised coordinate 2 x / W - 1 it samples the pixel position
    // ((g + 1) W - 1) / 2 = x - 1/2
    const double px = b[0] + (b[2] - b[0]) * ((double)jx / (double)(k.S - 1)) - 0.5;
    const double py = b[1] + (b[3] - b[1]) * ((double)jy / (double)(k.S - 1)) - 0.5;
    const double fx = floor(px), fy = floor(py);
    const double wx = px - fx, wy = py - fy;
    const bool far = !(fx >= -2.0 && fx <= (double)k.W && fy >= -2.0 && fy <= (double)k.H);
    const int ix = far ? -2 : (int)fx, iy = far ? -2 : (int)fy;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int xx = ix + (c & 1), yy = iy + (c >> 1);
        if (xx < 0 || xx >= k.W || yy < 0 || yy >= k.H) continue;
        const double w = ((c & 1) ? wx : 1.0 - wx) * ((c >> 1) ? wy : 1.0 - wy);
        const double m = (double)k.mask[n * k.ms[0] + yy * k.ms[1] + xx * k.ms[2]] / 255.0;
        const uint8_t *p = k.img + n * k.is[0] + yy * k.is[1] + xx * k.is[2];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) acc[ch] += w * (((double)p[ch * k.is[3]] / 255.0 * 2.0 - 1.0) * m);
        acc[3] += w * m;
    }
    float *o = k.out_img + (size_t)n * 3 * ss + q;
    o[0] = (float)acc[0];
    o[ss] = (float)acc[1];
    o[2 * ss] = (float)acc[2];
    k.out_mask[e] = (float)acc[3];
}

struct BytesK {
    const float *nF, *nB, *mask;   // [N][3][HW], [N][3][HW], [N][HW]
    uint8_t *oF, *oB, *oM;         // [N][HW][3], [N][HW][3], [N][HW]
    int64_t total, hw;
};
__device__ __forceinline__ uint8_t to_byte(float v) { return (uint8_t)(int)fminf(fmaxf(v, 0.f), 255.f); }     // truncates; NaN -> 0
__global__ void __launch_bounds__(256) normal_bytes_kernel(BytesK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.total) return;
    const int64_t n = e / k.hw, q = e - n * k.hw;
    const float m = k.mask[e];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const size_t src = ((size_t)n * 3 + c) * k.hw + q;
        k.oF[(size_t)e * 3 + c] = to_byte(((k.nF[src] + 1.f) / 2.f * m) * 255.f);
        k.oB[(size_t)e * 3 + c] = to_byte(((k.nB[src] + 1.f) / 2.f * m) * 255.f);
    }
    k.oM[e] = to_byte(m * 255.f);
}

inline unsigned blocks(int64_t threads) { return (unsigned)((threads + 255) / 256); }

bool check_frames(const char *what, int32_t N, int32_t H, int32_t W, int32_t S)
{
    if (N < 0 || N > 65535) { set_error("%s: N must be 0 .. 65535 (got %d)", what, N); return false; }
    if (H < 1 || W < 1 || H > 16384 || W > 16384) { set_error("%s: H and W must be 1 .. 16384 (got H=%d, W=%d)", what, H, W); return false; }
    if (S < 2 || S > 4096) { set_error("%s: the crop size must be 2 .. 4096 (got %d)", what, S); return false; }
    return true;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_normal_crop_boxes(int32_t N, int32_t H, int32_t W, int32_t S, const uint8_t *mask, const int64_t *mask_stride,
                                      const float *Ks, double *boxes, float *normal_Ks, int32_t *status, void *stream_)
{
    const char *what = "soar_normal_crop_boxes";
    if (!check_frames(what, N, H, W, S)) return 1;
    if (N == 0) return 0;
    if (!mask || !mask_stride || !Ks || !boxes || !normal_Ks || !status) { set_error("%s: NULL mask / strides / Ks / boxes / normal_Ks / status", what); return 1; }
    BoxK k{};
    k.mask = mask; k.Ks = Ks; k.boxes = boxes; k.normal_Ks = normal_Ks; k.status = status;
    for (int j = 0; j < 3; j++) k.ms[j] = mask_stride[j];
    k.H = H; k.W = W; k.S = S;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(normal_box_kernel, dim3((unsigned)N), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("normal_box", stream, 0);
    return 0;
}

extern "C" int soar_normal_crop_sample(int32_t N, int32_t H, int32_t W, int32_t S, const uint8_t *images, const int64_t *image_stride,
                                       const uint8_t *mask, const int64_t *mask_stride, const double *boxes, float *out_image,
                                       float *out_mask, void *stream_)
{
    const char *what = "soar_normal_crop_sample";
    if (!check_frames(what, N, H, W, S)) return 1;
    if (N == 0) return 0;
    if (!images || !image_stride || !mask || !mask_stride || !boxes || !out_image || !out_mask) { set_error("%s: NULL images / mask / strides / boxes / outputs", what); return 1; }
    CropK k{};
    k.img = images; k.mask = mask; k.boxes = boxes; k.out_img = out_image; k.out_mask = out_mask;
    for (int j = 0; j < 4; j++) k.is[j] = image_stride[j];
    for (int j = 0; j < 3; j++) k.ms[j] = mask_stride[j];
    k.H = H; k.W = W; k.S = S;
    k.total = (int64_t)N * S * S;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(normal_crop_kernel, dim3(blocks(k.total)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("normal_crop", stream, 0);
    return 0;
}

extern "C" int soar_normal_crop_bytes(int32_t N, int32_t H, int32_t W, const float *normal_F, const float *normal_B, const float *mask,
                                      uint8_t *out_F, uint8_t *out_B, uint8_t *out_mask, void *stream_)
{
    const char *what = "soar_normal_crop_bytes";
    if (N < 0 || H < 1 || W < 1 || (int64_t)(N > 0 ? N : 1) * H * W > (int64_t(1) << 30)) {
        set_error("%s: need N >= 0, H, W >= 1 and N * H * W <= 2^30 (N=%d, H=%d, W=%d)", what, N, H, W);
        return 1;
    }
    if (N == 0) return 0;
    if (!normal_F || !normal_B || !mask || !out_F || !out_B || !out_mask) { set_error("%s: NULL input / output", what); return 1; }
    BytesK k{};
    k.nF = normal_F; k.nB = normal_B; k.mask = mask; k.oF = out_F; k.oB = out_B; k.oM = out_mask;
    k.hw = (int64_t)H * W;
    k.total = (int64_t)N * k.hw;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(normal_bytes_kernel, dim3(blocks(k.total)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("normal_bytes", stream, 0);
    return 0;
}
