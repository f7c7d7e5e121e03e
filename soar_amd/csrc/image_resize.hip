// image_resize.hip -- Pillow's resize of 8-bit images (Resample.c, ImagingResample) on the device (soar_amd/jpeg.py resize_images;
// DESIGN.md 9u): a horizontal pass into an 8-bit intermediate, then a vertical one, each an integer convolution with per-output bounds
// and 22-bit fixed-point coefficients.  The tables are the caller's, built on the host exactly as Pillow builds them (they are
// tiny); the kernel checks every bound it reads from them, and an output whose bounds do not fit its axis is written as 0.
// One kernel serves both passes: the tensor is [outer][length][inner] and the convolution runs along `length`.
#include "soar_common.h"

namespace soar {
namespace {

constexpr int THREADS = 256;
constexpr int PRECISION_BITS = 32 - 8 - 2;

struct PassDev {
    const uint8_t *in;
    uint8_t *out;
    int64_t outer, in_len, out_len, inner;
    const int32_t *bounds;      // [out_len][2]: first sample, count
    const int32_t *coef;        // [out_len][ksize]
    int32_t ksize;
};

__global__ void __launch_bounds__(THREADS) resize_pass_kernel(PassDev a)
{
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x, row = a.out_len * a.inner;
    if (i >= a.outer * row) return;
    const int64_t o = i / row, rest = i - o * row, xx = rest / a.inner, k = rest - xx * a.inner;
    const int32_t x0 = a.bounds[2 * xx], n = a.bounds[2 * xx + 1];
    uint8_t v = 0;
    if (x0 >= 0 && n >= 0 && n <= a.ksize && (int64_t)x0 + n <= a.in_len) {
        const uint8_t *src = a.in + (o * a.in_len + x0) * a.inner + k;
        const int32_t *c = a.coef + xx * a.ksize;
        // Pillow's accumulator is an int: the products wrap there exactly as they do in this unsigned sum
        uint32_t ss = 1u << (PRECISION_BITS - 1);
        for (int32_t x = 0; x < n; x++) ss += (uint32_t)src[(int64_t)x * a.inner] * (uint32_t)c[x];
        const int32_t s = (int32_t)ss >> PRECISION_BITS;
        v = (uint8_t)(s < 0 ? 0 : (s > 255 ? 255 : s));
    }
    a.out[i] = v;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_resize_u8(const SoarResizeArgs *args, uint8_t *out, void *stream_)
{
    const char *me = "soar_resize_u8";
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarResizeArgs &a = *args;
    if (a.B < 0 || a.H < 1 || a.W < 1 || a.out_h < 1 || a.out_w < 1 || a.channels < 1 || a.channels > 4 || a.ksize_h < 1 || a.ksize_v < 1 ||
        a.H > 65535 || a.W > 65535 || a.out_h > 65535 || a.out_w > 65535) {
        set_error("%s: bad arguments (B=%d, H=%d, W=%d, channels=%d, out_h=%d, out_w=%d, ksize_h=%d, ksize_v=%d; need B >= 0, sizes "
                  "1 .. 65535, channels 1 .. 4, ksize >= 1)", me, a.B, a.H, a.W, a.channels, a.out_h, a.out_w, a.ksize_h, a.ksize_v);
        return 1;
    }
    if (a.B == 0) return 0;
    if (!a.images || !a.temp || !a.bounds_h || !a.coef_h || !a.bounds_v || !a.coef_v || !out) {
        set_error("%s: NULL images, temp, tables or out", me);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    PassDev h{a.images, a.temp, (int64_t)a.B * a.H, a.W, a.out_w, a.channels, a.bounds_h, a.coef_h, a.ksize_h};
    PassDev v{a.temp, out, a.B, a.H, a.out_h, (int64_t)a.out_w * a.channels, a.bounds_v, a.coef_v, a.ksize_v};
    const int64_t nh = h.outer * h.out_len * h.inner, nv = v.outer * v.out_len * v.inner;
    if ((nh + THREADS - 1) / THREADS > 0x7FFFFFFF || (nv + THREADS - 1) / THREADS > 0x7FFFFFFF) { set_error("%s: too many pixels for one launch", me); return 1; }
    hipLaunchKernelGGL(resize_pass_kernel, dim3((unsigned)((nh + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, h);
    SOAR_LAUNCH_OK("resize_horizontal", stream, 0);
    hipLaunchKernelGGL(resize_pass_kernel, dim3((unsigned)((nv + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, v);
    SOAR_LAUNCH_OK("resize_vertical", stream, 0);
    return 0;
}

}  // extern "C"
