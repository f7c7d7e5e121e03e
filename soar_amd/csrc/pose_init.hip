// pose_init.hip -- SMPL-X initialisation from keypoints alone on gfx950 (soar_amd/pose_init.py).
//
// **This stands in for the reference's SMPLer-X call (preproc/compute_smplx.py:36-53) and is a different algorithm**: the classical
// SMPLify start.  A bank of pose hypotheses (B base poses x H root rotations), a closed-form camera translation for each, the fit's
// own keypoint term as the score, and a shortest path through the frames.  **The bank, the intrinsics rule and every default are this
// project's definitions, not tuned on real video; nothing was compared with SMPLer-X or with the licensed SMPL-X model.**
//
// pose_search_kernel: one workgroup per frame, 16 wavefronts, a wavefront per state s = b H + h, looping over the states.  The
//   frame's 137 targets are staged in LDS once: the weight c_k, the normalised image point (a_k, b_k) = K^-1 (u_k, v_k, 1) in double
//   (back-substitution through the upper-triangular K, skew honoured), the pixel target, and the model point behind keypoint k.  A
//   lane owns the rows k = lane, lane + 64, lane + 128: it rotates its model point about the pivot, applies convert_kps (a lane
//   that owns row 8, 9 or 12 rotates the points behind 9 and 12 itself, so no lane waits for another), takes R_w2c of it, and
//   accumulates its rows in that order in double; the wavefront joins the lanes by the xor butterfly 32, 16, .., 1.  Every sum is
//   that one fixed tree, so a frame's outputs are the same bits alone, in any batch and in any order.  The 3 x 3 normal equations
//     [ W 0 -Sa ; 0 W -Sb ; -Sa -Sb Sq ] t' = [ -Srx ; -Sry ; Sar ],   rx = Yc_x - a Yc_z, ry = Yc_y - b Yc_z
//   are solved in double in closed form (den = W Sq - Sa^2 - Sb^2, det = W den).  The cost is the fit's keypoint term of the frame
//   (smplify.hip: projection with the divisor max(z, 1e-5), Geman-McClure) without the mean and the weight.
// pose_viterbi_kernel: one workgroup, 1024 / S threads per state: D[n][s] = (min_s' (D[n-1][s'] + T[s'][s])) + U[n][s] in float32 in
//   that order of additions, ties to the lowest s' (a strict < over ascending s', within a thread's chunk and then over the chunks),
//   the final minimum to the lowest s.  Where a thread's chunk is at most 32 predecessors (S <= 170 or so) its piece of T's column
//   stays in registers for all frames.  A unary row that is all +inf counts as zeros.  Unary rows come in, and back-pointers go to
//   the caller's tensor and come back for the walk, 4096 / S frames at a time through LDS (a load, a store or a dependent load per
//   frame would have every frame wait for device memory); thread 0 walks them.  Then a thread per frame writes the path's translation, linearly interpolated
//   over frames that are not valid and held at the ends.
// No atomics; nothing is read back; scratch (the back-pointers) is the caller's tensor.  Compiled with -ffp-contract=off: the
// frame-only sums W, Sa, Sb, Sq and with them the sign of the determinant are restated operation by operation (tests/pose_init_ref.py).
#include "soar_common.h"

namespace soar {

namespace {

constexpr int PKP = 137;            // OpenPose keypoints
constexpr int P_THREADS = 1024;
constexpr int P_WAVES = P_THREADS / 64;
constexpr int V_MAX_S = 1024, V_REG = 32, V_WALK = 4096;
constexpr int UNMAPPED = -1, CONTOUR = -2;

// rows in ascending order per lane (the caller adds them), then the xor butterfly: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}

// R (p - pivot) + pivot
__device__ __forceinline__ void rotate_about(const float *R, const float *p, const float *piv, float *out)
{
    const float d[3] = {p[0] - piv[0], p[1] - piv[1], p[2] - piv[2]};
    for (int r = 0; r < 3; r++) out[r] = fmaf(R[r * 3 + 2], d[2], fmaf(R[r * 3 + 1], d[1], R[r * 3] * d[0])) + piv[r];
}

__global__ void __launch_bounds__(P_THREADS) pose_search_kernel(SoarPoseSearch a)
{
    __shared__ int ksrc[PKP];
    __shared__ float cw[PKP], tgx[PKP], tgy[PKP];
    __shared__ double na[PKP], nb[PKP];
    __shared__ int any_valid[P_WAVES];
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int S = a.B * a.H;
    const float *K = a.Ks + (size_t)n * 9, *M = a.w2c;

    // ---- the frame's targets, once ----
    if (tid < PKP) ksrc[tid] = UNMAPPED;
    __syncthreads();
    if (tid < a.P) ksrc[a.dst_inds[tid]] = a.src_inds[tid] < a.PA ? a.src_inds[tid] : CONTOUR;      // dst_inds are distinct
    __syncthreads();
    if (tid < PKP) {
        const float *t = a.target_kps + ((size_t)n * PKP + tid) * 3;
        float c = t[2] * a.kp_mask[tid];
        if (tid >= 25 && tid < PKP - 70) c = 0.f;                  // the hands, as in the fit's stage one
        if (t[2] < a.conf_min) c = 0.f;
        if (ksrc[tid] == CONTOUR) c = 0.f;
        cw[tid] = c;
        tgx[tid] = t[0] * a.img_w;
        tgy[tid] = t[1] * a.img_h;
        const double u = (double)t[0] * (double)a.img_w, v = (double)t[1] * (double)a.img_h;
        const double x3 = 1.0 / (double)K[8];
        const double x2 = (v - (double)K[5] * x3) / (double)K[4];
        const double x1 = ((u - (double)K[1] * x2) - (double)K[2] * x3) / (double)K[0];
        na[tid] = x1 / x3;
        nb[tid] = x2 / x3;
    }
    __syncthreads();

    // ---- the sums that depend on the frame alone (every wavefront computes them: the same bits) ----
    double W = 0.0, Sa = 0.0, Sb = 0.0, Sq = 0.0, cnt = 0.0;
    for (int k = lane; k < PKP; k += 64) {
        const double c = (double)cw[k], ak = na[k], bk = nb[k];
        W += c;
        Sa += c * ak;
        Sb += c * bk;
        Sq += c * (ak * ak + bk * bk);
        cnt += cw[k] > 0.f ? 1.0 : 0.0;
    }
    W = wave_sum(W); Sa = wave_sum(Sa); Sb = wave_sum(Sb); Sq = wave_sum(Sq); cnt = wave_sum(cnt);
    const double den = (W * Sq - Sa * Sa) - Sb * Sb, det = W * den;
    const bool usable = cnt >= (double)a.min_points && det > 0.0;
    const float scale = a.scales[n], s2 = a.sigma * a.sigma;

    bool mine = false;
    for (int s = wave; s < S; s += P_WAVES) {
        const int b = s / a.H, h = s % a.H;
        const float *R = a.rotations + (size_t)h * 9, *piv = a.pivot + (size_t)b * 3, *pts = a.points0 + (size_t)b * a.PA * 3;
        float Yc[3][3];
        double Srx = 0.0, Sry = 0.0, Sar = 0.0;
        for (int i = 0; i < 3; i++) {
            const int k = lane + 64 * i;
            Yc[i][0] = Yc[i][1] = Yc[i][2] = 0.f;
            if (k >= PKP) continue;
            float Y[3] = {0.f, 0.f, 0.f};
            if (k == 8 || k == 9 || k == 12) {
                // convert_kps: keypoint 8 is the mean of 9 and 12, then x and y of 9 and 12 move (smplify.hip, statement for statement)
                float k9[3] = {0.f, 0.f, 0.f}, k12[3] = {0.f, 0.f, 0.f}, k8[3];
                if (ksrc[9] >= 0) rotate_about(R, pts + (size_t)ksrc[9] * 3, piv, k9);
                if (ksrc[12] >= 0) rotate_about(R, pts + (size_t)ksrc[12] * 3, piv, k12);
                for (int c = 0; c < 3; c++) k8[c] = 0.5f * (k9[c] + k12[c]);
                for (int c = 0; c < 3; c++) Y[c] = k == 8 ? k8[c] : (k == 9 ? k9[c] : k12[c]);
                if (k != 8)
                    for (int c = 0; c < 2; c++) {
                        const float own = k == 9 ? k9[c] : k12[c], other = k == 9 ? k12[c] : k9[c];
                        Y[c] = own + 0.25f * (own - other) + 0.5f * (k8[c] - 0.5f * (own + other));
                    }
            } else if (ksrc[k] >= 0) {
                rotate_about(R, pts + (size_t)ksrc[k] * 3, piv, Y);
            }
            for (int r = 0; r < 3; r++) Yc[i][r] = fmaf(M[r * 4 + 2], Y[2], fmaf(M[r * 4 + 1], Y[1], M[r * 4] * Y[0]));
            const double c = (double)cw[k], rx = (double)Yc[i][0] - na[k] * (double)Yc[i][2], ry = (double)Yc[i][1] - nb[k] * (double)Yc[i][2];
            Srx += c * rx;
            Sry += c * ry;
            Sar += c * (na[k] * rx + nb[k] * ry);
        }
        Srx = wave_sum(Srx); Sry = wave_sum(Sry); Sar = wave_sum(Sar);
        double t[3] = {0.0, 0.0, 0.0}, zmin = 1.0e300, value = 0.0;
        bool ok = usable;
        if (usable) {
            t[2] = ((W * Sar - Sa * Srx) - Sb * Sry) / den;
            t[0] = (Sa * t[2] - Srx) / W;
            t[1] = (Sb * t[2] - Sry) / W;
            const float tf[3] = {(float)t[0], (float)t[1], (float)t[2]};
            for (int i = 0; i < 3; i++) {
                const int k = lane + 64 * i;
                if (k >= PKP || !(cw[k] > 0.f)) continue;
                zmin = fmin(zmin, (double)Yc[i][2] + t[2]);
                const float pc[3] = {Yc[i][0] + tf[0], Yc[i][1] + tf[1], Yc[i][2] + tf[2]};
                float q[3];
                for (int r = 0; r < 3; r++) q[r] = fmaf(K[r * 3 + 2], pc[2], fmaf(K[r * 3 + 1], pc[1], K[r * 3] * pc[0]));
                const float zc = fmaxf(q[2], 1e-5f);
                const float e[2] = {(q[0] / zc - tgx[k]) / scale * 200.f, (q[1] / zc - tgy[k]) / scale * 200.f};
                const float g0 = (s2 * (e[0] * e[0])) / (s2 + e[0] * e[0]), g1 = (s2 * (e[1] * e[1])) / (s2 + e[1] * e[1]);
                value += (double)cw[k] * ((double)g0 + (double)g1);
            }
            zmin = wave_min(zmin);
            value = wave_sum(value);
            ok = zmin >= (double)a.z_min && isfinite(value);
        }
        if (lane == 0) {
            a.cost[(size_t)n * S + s] = ok ? (float)value : INFINITY;
            for (int c = 0; c < 3; c++) {
                // transl = R_w2c^T (t' - t_w2c)
                const double w = (double)M[c] * (t[0] - (double)M[3]) + (double)M[4 + c] * (t[1] - (double)M[7]) + (double)M[8 + c] * (t[2] - (double)M[11]);
                a.transl[((size_t)n * S + s) * 3 + c] = ok ? (float)w : 0.f;
            }
        }
        mine = mine || ok;
    }
    if (lane == 0) any_valid[wave] = mine ? 1 : 0;
    __syncthreads();
    if (tid == 0) {
        int v = 0;
        for (int w = 0; w < P_WAVES; w++) v |= any_valid[w];
        a.valid[n] = (uint8_t)v;
    }
}

// REG: a thread's chunk of its column of T (at most V_REG predecessors) stays in registers for all frames
template <bool REG>
__global__ void __launch_bounds__(V_MAX_S) pose_viterbi_kernel(int N, int S, const float *__restrict__ unary, const float *__restrict__ trans,
                                                               int32_t *__restrict__ bp, int64_t *path, float *__restrict__ total,
                                                               const float *__restrict__ transl, const uint8_t *__restrict__ valid,
                                                               float *__restrict__ transl_path)
{
    __shared__ float D[2][V_MAX_S];
    __shared__ float part_best[V_MAX_S];
    __shared__ int part_arg[V_MAX_S];
    __shared__ int rows[V_WALK];
    __shared__ float ubuf[V_WALK];
    __shared__ unsigned char evidence[V_WALK];
    __shared__ int walk;
    // G = 1024 / S threads per state: thread (g, s) scans the predecessors [g chunk, (g + 1) chunk) with a strict <, thread (0, s)
    // joins the G chunks in ascending order with a strict <: the first predecessor that attains the minimum wins, as in one scan
    const int tid = threadIdx.x, G = V_MAX_S / S, chunk = (S + G - 1) / G;
    const int g = tid / S, s = tid - g * S;
    const int q0 = min(S, g * chunk), q1 = g < G ? min(S, q0 + chunk) : q0;
    float tl[REG ? V_REG : 1];
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < V_REG; i++) tl[i] = q0 + i < q1 ? trans[(size_t)(q0 + i) * S + s] : INFINITY;      // + inf: never below the best
    }
    // F frames at a time: their unary rows come into LDS with one round of loads and their back-pointers leave it with one round of
    // stores (a load or a store per frame would have every frame wait for device memory), and a wavefront per row looks for evidence
    const int F = V_WALK / S;
    for (int first = 0; first < N; first += F) {
        const int frames = min(F, N - first), count = frames * S;
        __syncthreads();
        for (int i = tid; i < count; i += V_MAX_S) ubuf[i] = unary[(size_t)first * S + i];
        __syncthreads();
        for (int f = tid >> 6; f < frames; f += V_MAX_S / 64) {
            bool any = false;
            for (int q = tid & 63; q < S; q += 64) any = any || ubuf[f * S + q] < INFINITY;
            const bool row = __any(any);
            if ((tid & 63) == 0) evidence[f] = row ? 1 : 0;
        }
        for (int f = 0; f < frames; f++) {
            const int n = first + f;
            __syncthreads();                                          // the barrier between the frames
            const float add = (tid < S && evidence[f]) ? ubuf[f * S + tid] : 0.f;
            if (n == 0) {
                if (tid < S) { D[0][tid] = add; rows[tid] = 0; }
                continue;
            }
            const float *prev = D[(n - 1) & 1];
            float best = INFINITY;
            int arg = q0;
            if constexpr (REG) {
                best = prev[q0 & (V_MAX_S - 1)] + tl[0];
#pragma unroll
                for (int i = 1; i < V_REG; i++) {
                    if (i >= chunk) break;                            // (uniform: every thread has the same chunk length)
                    const float v = prev[(q0 + i) & (V_MAX_S - 1)] + tl[i];
                    if (v < best) { best = v; arg = q0 + i; }
                }
            } else if (q0 < q1) {
                best = prev[q0] + trans[(size_t)q0 * S + s];
                for (int q = q0 + 1; q < q1; q++) {
                    const float v = prev[q] + trans[(size_t)q * S + s];
                    if (v < best) { best = v; arg = q; }
                }
            }
            part_best[tid] = best;
            part_arg[tid] = arg;
            __syncthreads();
            if (tid < S) {
                for (int k = 1; k < G; k++)
                    if (part_best[k * S + tid] < best) { best = part_best[k * S + tid]; arg = part_arg[k * S + tid]; }
                D[n & 1][tid] = best + add;
                rows[f * S + tid] = arg;
            }
        }
        __syncthreads();
        for (int i = tid; i < count; i += V_MAX_S) bp[(size_t)first * S + i] = rows[i];
    }
    __syncthreads();
    if (tid == 0) {
        const float *last = D[(N - 1) & 1];
        float best = last[0];
        int arg = 0;
        for (int q = 1; q < S; q++)
            if (last[q] < best) { best = last[q]; arg = q; }
        total[0] = best;
        walk = arg;
    }
    // the walk back, V_WALK / S frames at a time: all threads bring those rows of back-pointers into LDS with one round of loads,
    // thread 0 follows them there (a walk through device memory pays a load's latency per frame)
    for (int hi = N - 1; hi >= 0; hi -= F) {
        const int lo = max(0, hi - F + 1), count = (hi - lo + 1) * S;
        __syncthreads();
        for (int i = tid; i < count; i += V_MAX_S) rows[i] = bp[(size_t)lo * S + i];
        __syncthreads();
        if (tid == 0) {
            int arg = walk;
            for (int n = hi; n >= lo; n--) {
                path[n] = arg;
                arg = rows[(n - lo) * S + arg];          // row 0 holds zeros: the value after frame 0 is not used
            }
            walk = arg;
        }
    }
    if (!transl_path) return;
    __syncthreads();
    for (int n = tid; n < N; n += V_MAX_S) {
        int lo = n, hi = n;
        while (lo >= 0 && !valid[lo]) lo--;
        while (hi < N && !valid[hi]) hi++;
        for (int c = 0; c < 3; c++) {
            float v = 0.f;
            if (lo >= 0 && hi < N) {
                const float p = transl[((size_t)lo * S + path[lo]) * 3 + c], q = transl[((size_t)hi * S + path[hi]) * 3 + c];
                v = hi == lo ? p : p + (q - p) * ((float)(n - lo) / (float)(hi - lo));
            } else if (lo >= 0) {
                v = transl[((size_t)lo * S + path[lo]) * 3 + c];
            } else if (hi < N) {
                v = transl[((size_t)hi * S + path[hi]) * 3 + c];
            }
            transl_path[(size_t)n * 3 + c] = v;
        }
    }
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_pose_init_search(const SoarPoseSearch *args, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!args) { set_error("soar_pose_init_search: NULL args"); return 1; }
    const SoarPoseSearch &a = *args;
    if (a.N <= 0 || a.B < 1 || a.H < 1 || (int64_t)a.B * a.H > V_MAX_S) {
        set_error("soar_pose_init_search: need N >= 1, B >= 1, H >= 1 and S = B H <= %d states (N=%d B=%d H=%d)", V_MAX_S, a.N, a.B, a.H);
        return 1;
    }
    if (a.PA < 1 || a.P < 0 || a.P > PKP || (int64_t)a.B * a.PA > 0x7fffffff / 3 || (int64_t)a.N * a.B * a.H > 0x7fffffff / 3) {
        set_error("soar_pose_init_search: need PA >= 1 model points, 0 <= P <= %d table entries and sizes below 2^31 (PA=%d P=%d)", PKP, a.PA, a.P);
        return 1;
    }
    if (a.min_points < 1) { set_error("soar_pose_init_search: min_points=%d: need at least 1", a.min_points); return 1; }
    if (!(a.sigma > 0.f) || !(a.img_w > 0.f) || !(a.img_h > 0.f)) { set_error("soar_pose_init_search: sigma and the image size must be positive"); return 1; }
    if (!a.points0 || !a.pivot || !a.rotations || (a.P > 0 && (!a.src_inds || !a.dst_inds)) || !a.kp_mask || !a.target_kps || !a.Ks || !a.w2c
        || !a.scales || !a.cost || !a.transl || !a.valid) {
        set_error("soar_pose_init_search: NULL pointer");
        return 1;
    }
    hipLaunchKernelGGL(pose_search_kernel, dim3(a.N), dim3(P_THREADS), 0, stream, a);
    SOAR_LAUNCH_OK("pose_init_search", stream, 0);
    return 0;
}

extern "C" int soar_pose_init_viterbi(int32_t N, int32_t S, const float *unary, const float *trans, int32_t *backptr, int64_t *path, float *total,
                                      const float *transl, const uint8_t *valid, float *transl_path, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (N <= 0 || S < 1 || S > V_MAX_S || (int64_t)N * S > 0x7fffffff / 3) {
        set_error("soar_pose_init_viterbi: need N >= 1 frames and 1 <= S <= %d states with N S 3 below 2^31 (N=%d S=%d)", V_MAX_S, N, S);
        return 1;
    }
    if (!unary || !trans || !backptr || !path || !total) { set_error("soar_pose_init_viterbi: NULL pointer"); return 1; }
    if ((transl != nullptr) != (valid != nullptr) || (transl != nullptr) != (transl_path != nullptr)) {
        set_error("soar_pose_init_viterbi: transl, valid and transl_path come together");
        return 1;
    }
    const int G = V_MAX_S / S, chunk = (S + G - 1) / G;
    if (chunk <= V_REG)
        hipLaunchKernelGGL(pose_viterbi_kernel<true>, dim3(1), dim3(V_MAX_S), 0, stream, N, S, unary, trans, backptr, path, total, transl, valid, transl_path);
    else
        hipLaunchKernelGGL(pose_viterbi_kernel<false>, dim3(1), dim3(V_MAX_S), 0, stream, N, S, unary, trans, backptr, path, total, transl, valid, transl_path);
    SOAR_LAUNCH_OK("pose_init_viterbi", stream, 0);
    return 0;
}
