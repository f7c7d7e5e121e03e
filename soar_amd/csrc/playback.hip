// playback.hip -- avatar playback (soar_amd/playback.py): the two per-frame stages either side of the renderer when a
// trained avatar is looked at (the reference's TS/test/render_rot.py does both on the host, one frame at a time).
//   soar_motion_resample    a key-pose sequence sampled at F times: per joint axis-angle -> quaternion -> slerp -> axis-angle, the root
//                           joint optionally turned about y (the turntable), transl / expression linear.  One thread per (frame, joint).
//   soar_playback_finish    B rendered frames -> the four byte images the reference writes (rgb, normal, occ with the mask as a fourth
//                           channel, and the mask), torchvision's save_image conversion.  One launch, 10 floats read and 13 bytes
//                           written per pixel.
// Compiled with -ffp-contract=off: both are pinned on a NumPy restatement (tests/playback_ref.py) that follows the operations below in
// their order; only sinf / cosf / acosf / atan2f differ from NumPy's by a few ulp.
#include "soar_common.h"

namespace soar {
namespace {

constexpr int JOINTS = 55;                        // SMPL-X: the 165 floats of full_pose
constexpr int MOTION_THREADS = 256;
constexpr int FINISH_THREADS = 256;
// DESIGN.md 9k states these three
constexpr float SMALL_ANGLE = 1e-3f;              // below it sin(t/2)/t = 1/2 - t^2/48 and (2 atan2(n, w))/n = 2 + n^2/3
constexpr float LERP_DOT = 0.999999f;             // |q0 . q1| above it: normalised lerp instead of slerp (the angle is below 1.5e-3)

struct Quat { float w, x, y, z; };

__device__ __forceinline__ Quat quat_of_axis_angle(float ax, float ay, float az)
{
    const float t2 = ax * ax + ay * ay + az * az;
    const float t = sqrtf(t2);
    const float h = 0.5f * t;
    const float s = t < SMALL_ANGLE ? 0.5f - t2 / 48.0f : sinf(h) / t;
    return {cosf(h), s * ax, s * ay, s * az};
}

__device__ __forceinline__ Quat normalised(Quat q)
{
    const float n = sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
    return {q.w / n, q.x / n, q.y / n, q.z / n};
}

// the rotation of q at weight 1 - u and of r at weight u, along the shorter arc
__device__ __forceinline__ Quat slerp(Quat q, Quat r, float u)
{
    float dot = q.w * r.w + q.x * r.x + q.y * r.y + q.z * r.z;
    if (dot < 0.f) { r = {-r.w, -r.x, -r.y, -r.z}; dot = -dot; }
    float a, b;
    if (dot > LERP_DOT) {
        a = 1.0f - u;
        b = u;
    } else {
        const float t = acosf(dot), sn = sinf(t);
        a = sinf((1.0f - u) * t) / sn;
        b = sinf(u * t) / sn;
    }
    return normalised({a * q.w + b * r.w, a * q.x + b * r.x, a * q.y + b * r.y, a * q.z + b * r.z});
}

// q (x) (cos(yaw / 2), 0, sin(yaw / 2), 0): R <- R Ry(yaw)
__device__ __forceinline__ Quat times_yaw(Quat q, float yaw)
{
    const float c = cosf(0.5f * yaw), s = sinf(0.5f * yaw);
    return {q.w * c - q.y * s, q.x * c - q.z * s, q.y * c + q.w * s, q.z * c + q.x * s};
}

// unit quaternion -> axis-angle with the angle in [0, pi] (w >= 0 enforced)
__device__ __forceinline__ void axis_angle_of_quat(Quat q, float *out)
{
    if (q.w < 0.f) q = {-q.w, -q.x, -q.y, -q.z};
    const float n2 = q.x * q.x + q.y * q.y + q.z * q.z;
    const float n = sqrtf(n2);
    const float k = n < SMALL_ANGLE ? 2.0f + n2 / 3.0f : (2.0f * atan2f(n, q.w)) / n;
    out[0] = k * q.x;
    out[1] = k * q.y;
    out[2] = k * q.z;
}

struct MotionDev {
    int32_t K, F, E;
    const float *key_pose, *key_transl, *key_expr, *t, *yaw;
    float *pose, *transl, *expr;
};

__global__ void __launch_bounds__(MOTION_THREADS) motion_resample_kernel(MotionDev a)
{
    const int64_t idx = (int64_t)blockIdx.x * MOTION_THREADS + threadIdx.x;
    if (idx >= (int64_t)a.F * JOINTS) return;
    const int f = (int)(idx / JOINTS), j = (int)(idx - (int64_t)f * JOINTS);
    const float tc = fminf(fmaxf(a.t[f], 0.f), (float)(a.K - 1));       // (a NaN time samples key 0)
    const int i0 = (int)floorf(tc);
    const int i1 = i0 + 1 < a.K ? i0 + 1 : a.K - 1;
    const float u = tc - (float)i0;
    const float yaw = (j == 0 && a.yaw) ? a.yaw[f] : 0.f;

    const float *p0 = a.key_pose + ((int64_t)i0 * JOINTS + j) * 3;
    float *out = a.pose + ((int64_t)f * JOINTS + j) * 3;
    if (u == 0.f && yaw == 0.f) {
        // on a key, nothing to turn: the key's own numbers (sin(0) is not asked)
        out[0] = p0[0]; out[1] = p0[1]; out[2] = p0[2];
    } else {
        Quat q = quat_of_axis_angle(p0[0], p0[1], p0[2]);
        if (u != 0.f) {
            const float *p1 = a.key_pose + ((int64_t)i1 * JOINTS + j) * 3;
            q = slerp(q, quat_of_axis_angle(p1[0], p1[1], p1[2]), u);
        }
        if (yaw != 0.f) q = times_yaw(q, yaw);
        axis_angle_of_quat(q, out);
    }

    // the frame's 3 + E linear values, shared out among its 55 threads
    for (int s = j; s < 3 + a.E; s += JOINTS) {
        const bool tr = s < 3;
        const int width = tr ? 3 : a.E, col = tr ? s : s - 3;
        const float *src = tr ? a.key_transl : a.key_expr;
        float *dst = tr ? a.transl : a.expr;
        const float v0 = src[(int64_t)i0 * width + col];
        dst[(int64_t)f * width + col] = u == 0.f ? v0 : (1.0f - u) * v0 + u * src[(int64_t)i1 * width + col];
    }
}

// ---- the output stage -------------------------------------------------------------------------------------------------------
// torchvision's save_image: x.mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- a multiply, an add, a clamp, a truncation.  NaN -> 0
// (fmaxf returns the operand that is a number).
__device__ __forceinline__ uint32_t to_byte(float v)
{
    const float s = v * 255.0f + 0.5f;                                  // (un-contracted: -ffp-contract=off)
    return (uint32_t)(int)fminf(fmaxf(s, 0.f), 255.f);
}

struct FinishDev {
    int64_t HW;
    int32_t normal_as_rgb;
    const float *render, *normal, *mask, *occ;
    int64_t rs, ns, ms, os;                                             // floats from one frame to the next
    uint32_t *rgb, *normal_out, *occ_out;
    uint8_t *mask_out;
};

// PIX pixels per thread: 4 (16-byte loads and stores; the host has checked that H W is a multiple of 4 and every address aligned)
// or 1 (any size, any 4-byte aligned address).  A frame's planes and byte images are contiguous, so pixels are counted through the
// frame; nothing is read or written at or behind pixel H W.
template <int PIX>
__global__ void __launch_bounds__(FINISH_THREADS) playback_finish_kernel(FinishDev a)
{
    const int64_t p = ((int64_t)blockIdx.x * FINISH_THREADS + threadIdx.x) * PIX;
    if (p >= a.HW) return;
    const int64_t b = blockIdx.y, HW = a.HW;
    float v[10][PIX] = {};
    const float *planes[10];
    for (int c = 0; c < 3; c++) {
        planes[c] = a.render + b * a.rs + c * HW;
        planes[3 + c] = a.normal + b * a.ns + c * HW;
        planes[6 + c] = a.occ ? a.occ + b * a.os + c * HW : nullptr;
    }
    planes[9] = a.mask + b * a.ms;
#pragma unroll
    for (int c = 0; c < 10; c++) {
        if (!planes[c]) continue;
        if constexpr (PIX == 4) {
            const float4 q = *reinterpret_cast<const float4 *>(planes[c] + p);
            v[c][0] = q.x; v[c][1] = q.y; v[c][2] = q.z; v[c][3] = q.w;
        } else {
            v[c][0] = planes[c][p];
        }
    }
    uint32_t rgb[PIX], nrm[PIX], occ[PIX], alpha[PIX];
#pragma unroll
    for (int i = 0; i < PIX; i++) {
        alpha[i] = to_byte(v[9][i]);
        const uint32_t top = alpha[i] << 24;
        rgb[i] = to_byte(v[0][i]) | to_byte(v[1][i]) << 8 | to_byte(v[2][i]) << 16 | top;
        float n0 = v[3][i], n1 = v[4][i], n2 = v[5][i];
        if (a.normal_as_rgb) { n0 = n0 * 0.5f + 0.5f; n1 = n1 * 0.5f + 0.5f; n2 = n2 * 0.5f + 0.5f; }
        nrm[i] = to_byte(n0) | to_byte(n1) << 8 | to_byte(n2) << 16 | top;
        occ[i] = a.occ ? (to_byte(v[6][i]) | to_byte(v[7][i]) << 8 | to_byte(v[8][i]) << 16 | top) : 0u;
    }
    const int64_t o = b * HW + p;
    if constexpr (PIX == 4) {
        *reinterpret_cast<uint4 *>(a.rgb + o) = make_uint4(rgb[0], rgb[1], rgb[2], rgb[3]);
        *reinterpret_cast<uint4 *>(a.normal_out + o) = make_uint4(nrm[0], nrm[1], nrm[2], nrm[3]);
        if (a.occ) *reinterpret_cast<uint4 *>(a.occ_out + o) = make_uint4(occ[0], occ[1], occ[2], occ[3]);
        *reinterpret_cast<uint32_t *>(a.mask_out + o) = alpha[0] | alpha[1] << 8 | alpha[2] << 16 | alpha[3] << 24;
    } else {
        a.rgb[o] = rgb[0];
        a.normal_out[o] = nrm[0];
        if (a.occ) a.occ_out[o] = occ[0];
        a.mask_out[o] = (uint8_t)alpha[0];
    }
}

inline bool aligned(const void *p, size_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_motion_resample(int32_t K, int32_t F, int32_t E, const float *key_pose, const float *key_transl, const float *key_expr,
                         const float *t, const float *yaw, float *pose, float *transl, float *expr, void *stream_)
{
    const char *me = "soar_motion_resample";
    if (K < 1 || F < 0 || E < 0 || K > (1 << 24) || (int64_t)F * JOINTS > (1ll << 30)) {
        set_error("%s: bad arguments (K=%d, F=%d, E=%d; need 1 <= K <= 2^24, F >= 0 with 55 F <= 2^30, E >= 0)", me, K, F, E);
        return 1;
    }
    if (F == 0) return 0;
    if (!key_pose || !key_transl || !t || !pose || !transl || (E > 0 && (!key_expr || !expr))) {
        set_error("%s: NULL key_pose / key_transl / key_expr / t / pose / transl / expr (only yaw may be NULL)", me);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    MotionDev d;
    d.K = K; d.F = F; d.E = E;
    d.key_pose = key_pose; d.key_transl = key_transl; d.key_expr = key_expr; d.t = t; d.yaw = yaw;
    d.pose = pose; d.transl = transl; d.expr = expr;
    const unsigned blocks = (unsigned)(((int64_t)F * JOINTS + MOTION_THREADS - 1) / MOTION_THREADS);
    hipLaunchKernelGGL(motion_resample_kernel, dim3(blocks), dim3(MOTION_THREADS), 0, stream, d);
    SOAR_LAUNCH_OK("motion_resample", stream, 0);
    return 0;
}

int soar_playback_finish(const SoarPlaybackArgs *args, void *stream_)
{
    const char *me = "soar_playback_finish";
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarPlaybackArgs &a = *args;
    if (a.B < 0 || a.B > 65535 || a.H < 1 || a.W < 1 || (int64_t)a.B * a.H * a.W > (1ll << 30)) {
        set_error("%s: bad arguments (B=%d, H=%d, W=%d; need 0 <= B <= 65535, H, W >= 1, B H W <= 2^30)", me, a.B, a.H, a.W);
        return 1;
    }
    if (a.B == 0) return 0;
    if (!a.render || !a.normal || !a.mask) { set_error("%s: NULL render / normal / mask", me); return 1; }
    if (!a.rgb || !a.normal_out || !a.mask_out || (a.occ && !a.occ_out)) { set_error("%s: NULL rgb / normal_out / mask_out / occ_out", me); return 1; }
    const int64_t HW = (int64_t)a.H * a.W;
    if (a.render_stride < 3 * HW || a.normal_stride < 3 * HW || a.mask_stride < HW || (a.occ && a.occ_stride < 3 * HW)) {
        set_error("%s: a frame stride is shorter than the frame (render %lld, normal %lld, mask %lld, occ %lld floats for H W = %lld)", me,
                  (long long)a.render_stride, (long long)a.normal_stride, (long long)a.mask_stride, (long long)a.occ_stride, (long long)HW);
        return 1;
    }
    if (!aligned(a.render, 4) || !aligned(a.normal, 4) || !aligned(a.mask, 4) || !aligned(a.occ, 4) || !aligned(a.rgb, 4) ||
        !aligned(a.normal_out, 4) || !aligned(a.occ_out, 4)) {
        set_error("%s: the float inputs and the RGBA outputs must be 4-byte aligned", me);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    FinishDev d;
    d.HW = HW; d.normal_as_rgb = a.normal_as_rgb;
    d.render = a.render; d.normal = a.normal; d.mask = a.mask; d.occ = a.occ;
    d.rs = a.render_stride; d.ns = a.normal_stride; d.ms = a.mask_stride; d.os = a.occ ? a.occ_stride : 0;
    d.rgb = reinterpret_cast<uint32_t *>(a.rgb); d.normal_out = reinterpret_cast<uint32_t *>(a.normal_out);
    d.occ_out = reinterpret_cast<uint32_t *>(a.occ_out); d.mask_out = a.mask_out;
    // 16-byte accesses when every one of them is aligned: H W and the frame strides multiples of 4, the bases on 16 bytes
    // (the mask image then on 4: its 4 bytes of a thread go out as one word)
    const bool wide = HW % 4 == 0 && d.rs % 4 == 0 && d.ns % 4 == 0 && d.ms % 4 == 0 && d.os % 4 == 0 && aligned(a.render, 16) &&
                      aligned(a.normal, 16) && aligned(a.mask, 16) && aligned(a.occ, 16) && aligned(a.rgb, 16) &&
                      aligned(a.normal_out, 16) && aligned(a.occ_out, 16) && aligned(a.mask_out, 4);
    const int pix = wide ? 4 : 1;
    const dim3 grid((unsigned)((HW / pix + FINISH_THREADS - 1) / FINISH_THREADS), (unsigned)a.B);
    if (wide)
        hipLaunchKernelGGL(playback_finish_kernel<4>, grid, dim3(FINISH_THREADS), 0, stream, d);
    else
        hipLaunchKernelGGL(playback_finish_kernel<1>, grid, dim3(FINISH_THREADS), 0, stream, d);
    SOAR_LAUNCH_OK("playback_finish", stream, 0);
    return 0;
}

}  // extern "C"
