// smplify.hip -- the SMPLify keypoint objective and its gradient on gfx950 (soar_amd/smplify.py).
//
// Restates what one closure evaluation of the reference's SMPLify.fit does (preproc/utils.py:626-685, :805-845) for N frames:
//   6-D -> rotation (Gram-Schmidt, :155-161); the body model's lbs() restricted to what the objective reads -- the 55 posed joints
//   and the <= 256 gathered vertices behind the selected vertices and the landmark triangles (TS/utils/smplx/lbs.py:197-241,
//   :104-144); convert_kps (:574-588); projection with w2c[:3] and K and the divisor clamp(z, 1e-5); the Geman-McClure keypoint
//   term; the preserve term (row 2-norms); the smooth term (squared angle of R[t+1] R[t]^T, :149-152).
// smplify_frame_kernel: one workgroup per frame, forward then the analytic adjoint in reverse tree order back to the 6-D
//   parameters, transl and the frame's betas partial.  Everything between stays in LDS or registers.  A closure evaluation is a
//   launch-latency problem (a few hundred kFLOP per frame): the torch composition runs the full 10 475-vertex model through
//   autograd in some two hundred launches.
// smplify_finish_kernel: one workgroup: the smooth term, a thread per (frame, joint) reading both neighbours, added to the
//   gradients in place, then the sums over frames (betas partials, loss partials) in a fixed order, in double.
// No atomics anywhere: every sum is a loop or a tree in a fixed order, so two runs agree bit for bit, and a frame's keypoint and
// preserve gradients depend on nothing but the frame's own inputs and the scales.
// The reference sends every optimised rotation through rotmat -> rotvec -> batch_rodrigues before lbs(); that is the identity map
// and is skipped.  Jaw and eyes are rotation vectors and go through batch_rodrigues (soar_rodrigues.h) as there.
//
// smplify_frame_kernel<true> (soar_smplify_objective_body) adds the two things SMPLX.forward does for the model the reference
// creates (use_face_contour=True, flat_hand_mean=False); smplify_frame_kernel<false> is the kernel above, statement for statement.
//   Contour landmarks: after the chain the workgroup computes the table row from Rw[neck] (rot_mat_to_euler and the rounding of
//   find_dynamic_lmk_idx_and_bcoords, lbs.py:82-99) and fills smap[slot] -> row of the gathered arrays: slots 0 .. VS-1 are the
//   static rows themselves, slot VS + 3 l + k is corner k of contour landmark l in the chosen row.  The gathered arrays hold the
//   union of all 79 rows (VU rows, any count); a frame's active set, VS + 3 L_dyn <= 256 slots, lives in LDS as before, and every
//   loop over vertices (blend shapes, correctives, skinning, their adjoints, the betas partial) reads device memory through
//   smap.  The row is not differentiated.
//   Pose mean: a joint whose bit is set in mean_mask enters the body model as rodrigues(log(R) + mean_j) (R from Gram-Schmidt for an
//   optimised joint; for jaw and eyes the mean is added to the rotation vector).  log: a = vee(R - R^T) / 2, s = |a|,
//   c = (tr R - 1) / 2, v = a atan2(s, c) / s; for s < 1e-3 with c > 0 the series 1 + s^2/6 + 3 s^4/40 of asin(s)/s (the next term
//   is below 5e-20), so v = 0 with a finite gradient at R = I.  Specified for angles up to 3.0 rad: towards pi, s -> 0 divides.
//   The adjoint runs Rodrigues' adjoint, then log's, then Gram-Schmidt's.  The preserve and smooth terms read the 6-D vectors.
//
// smplify_points_kernel (soar_smplify_model_points) is a kernel of its own: the forward up to the model points, for every static
//   point and not only the mapped ones, through the same device functions.  It feeds the pose search of pose_init.hip
//   and adds nothing to the kernels above: their instructions are the parent's, one for one.
#include <type_traits>

#include "soar_common.h"
#include "soar_rodrigues.h"

namespace soar {

namespace {

constexpr int SJ = 55;              // SMPL-X joints
constexpr int SOPT = 52;            // optimised joints: global 1, body 21, left hand 15, right hand 15
constexpr int SKP = 137;            // OpenPose keypoints
constexpr int SFEAT = (SJ - 1) * 9;
constexpr int S_THREADS = 256;
constexpr int S_MAX_VS = 256;
constexpr int S_MAX_P = 160;
constexpr int S_MAX_NB = 64;
constexpr int S_MAX_DEPTH = 32;
constexpr int F_THREADS = 1024;
constexpr float NORM_EPS = 1e-12f;  // F.normalize

__device__ __forceinline__ float dot3(const float *a, const float *b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }

// rotation_6d_to_matrix: rows b1, b2, b3 = b1 x b2
__device__ __forceinline__ void rot6d(const float *x, float *R)
{
    const float n1 = fmaxf(sqrtf(dot3(x, x)), NORM_EPS);
    float b1[3] = {x[0] / n1, x[1] / n1, x[2] / n1};
    const float d = dot3(b1, x + 3);
    float u[3] = {x[3] - d * b1[0], x[4] - d * b1[1], x[5] - d * b1[2]};
    const float n2 = fmaxf(sqrtf(dot3(u, u)), NORM_EPS);
    float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    R[0] = b1[0]; R[1] = b1[1]; R[2] = b1[2];
    R[3] = b2[0]; R[4] = b2[1]; R[5] = b2[2];
    R[6] = b1[1] * b2[2] - b1[2] * b2[1];
    R[7] = b1[2] * b2[0] - b1[0] * b2[2];
    R[8] = b1[0] * b2[1] - b1[1] * b2[0];
}

// the adjoint of rot6d: g [9] (rows) -> gx [6]
__device__ __forceinline__ void rot6d_backward(const float *x, const float *g, float *gx)
{
    const float l1 = sqrtf(dot3(x, x)), n1 = fmaxf(l1, NORM_EPS);
    const float b1[3] = {x[0] / n1, x[1] / n1, x[2] / n1};
    const float d = dot3(b1, x + 3);
    const float u[3] = {x[3] - d * b1[0], x[4] - d * b1[1], x[5] - d * b1[2]};
    const float l2 = sqrtf(dot3(u, u)), n2 = fmaxf(l2, NORM_EPS);
    const float b2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
    const float *g1 = g, *g2 = g + 3, *g3 = g + 6;
    // b3 = b1 x b2
    float gb1[3] = {g1[0] + (b2[1] * g3[2] - b2[2] * g3[1]), g1[1] + (b2[2] * g3[0] - b2[0] * g3[2]), g1[2] + (b2[0] * g3[1] - b2[1] * g3[0])};
    float gb2[3] = {g2[0] + (g3[1] * b1[2] - g3[2] * b1[1]), g2[1] + (g3[2] * b1[0] - g3[0] * b1[2]), g2[2] + (g3[0] * b1[1] - g3[1] * b1[0])};
    // b2 = u / max(|u|, eps)
    float gu[3];
    if (l2 > NORM_EPS) {
        const float t = dot3(b2, gb2);
        for (int c = 0; c < 3; c++) gu[c] = (gb2[c] - b2[c] * t) / n2;
    } else {
        for (int c = 0; c < 3; c++) gu[c] = gb2[c] / n2;
    }
    // u = a2 - (b1 . a2) b1
    const float gd = -dot3(b1, gu);
    for (int c = 0; c < 3; c++) {
        gx[3 + c] = fmaf(gd, b1[c], gu[c]);
        gb1[c] += fmaf(gd, x[3 + c], -d * gu[c]);
    }
    if (l1 > NORM_EPS) {
        const float t = dot3(b1, gb1);
        for (int c = 0; c < 3; c++) gx[c] = (gb1[c] - b1[c] * t) / n1;
    } else {
        for (int c = 0; c < 3; c++) gx[c] = gb1[c] / n1;
    }
}

// ---- the pose mean's detour: log, and the adjoints of log and of rodrigues<3> ----
constexpr float LOG_SERIES = 1e-3f;

__device__ __forceinline__ void so3_log(const float *R, float *v)
{
    const float a[3] = {0.5f * (R[7] - R[5]), 0.5f * (R[2] - R[6]), 0.5f * (R[3] - R[1])};
    const float c = 0.5f * (R[0] + R[4] + R[8] - 1.f);
    const float s2 = dot3(a, a), s = sqrtf(s2);
    const float f = (s < LOG_SERIES && c > 0.f) ? fmaf(s2, fmaf(s2, 0.075f, 1.f / 6.f), 1.f) : atan2f(s, c) / fmaxf(s, 1e-30f);
    for (int k = 0; k < 3; k++) v[k] = a[k] * f;
}

// gv [3] -> gR [9] (overwritten)
__device__ __forceinline__ void so3_log_backward(const float *R, const float *gv, float *gR)
{
    const float a[3] = {0.5f * (R[7] - R[5]), 0.5f * (R[2] - R[6]), 0.5f * (R[3] - R[1])};
    const float c = 0.5f * (R[0] + R[4] + R[8] - 1.f);
    const float s2 = dot3(a, a), s = sqrtf(s2);
    float f, fs, fc;                       // f, (df/ds) / s, df/dc
    if (s < LOG_SERIES && c > 0.f) {
        f = fmaf(s2, fmaf(s2, 0.075f, 1.f / 6.f), 1.f);
        fs = fmaf(s2, 0.3f, 1.f / 3.f);
        fc = 0.f;
    } else {
        const float den = fmaf(s, s, c * c);
        f = atan2f(s, c) / fmaxf(s, 1e-30f);
        fs = s2 > 0.f ? (c / den - f) / s2 : 0.f;
        fc = den > 0.f ? -1.f / den : 0.f;
    }
    const float gf = dot3(a, gv);
    const float ga[3] = {fmaf(a[0], gf * fs, f * gv[0]), fmaf(a[1], gf * fs, f * gv[1]), fmaf(a[2], gf * fs, f * gv[2])};
    const float gc = 0.5f * (gf * fc);
    gR[0] = gc; gR[4] = gc; gR[8] = gc;
    gR[7] = 0.5f * ga[0]; gR[5] = -0.5f * ga[0];
    gR[2] = 0.5f * ga[1]; gR[6] = -0.5f * ga[1];
    gR[3] = 0.5f * ga[2]; gR[1] = -0.5f * ga[2];
}

// the adjoint of rodrigues<3> (soar_rodrigues.h): g [9] -> gv [3]
__device__ __forceinline__ void rodrigues_backward(const float *v, const float *g, float *gv)
{
    const float e[3] = {v[0] + 1e-8f, v[1] + 1e-8f, v[2] + 1e-8f};
    const float angle = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
    const float rx = v[0] / angle, ry = v[1] / angle, rz = v[2] / angle;
    const float sn = sinf(angle), cn = cosf(angle), cs = 1.f - cn;
    const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
    float gsn = 0.f, gcs = 0.f, gK[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            float kk = 0.f, t = 0.f;
            for (int m = 0; m < 3; m++) {
                kk += K[r * 3 + m] * K[m * 3 + c];
                t += g[r * 3 + m] * K[c * 3 + m] + K[m * 3 + r] * g[m * 3 + c];     // g K^T + K^T g
            }
            gsn = fmaf(g[r * 3 + c], K[r * 3 + c], gsn);
            gcs = fmaf(g[r * 3 + c], kk, gcs);
            gK[r * 3 + c] = fmaf(cs, t, sn * g[r * 3 + c]);
        }
    const float gr[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
    const float gang = fmaf(gsn, cn, gcs * sn) - dot3(gr, v) / (angle * angle);
    for (int k = 0; k < 3; k++) gv[k] = gr[k] / angle + gang * (e[k] / angle);
}

// the table row of find_dynamic_lmk_idx_and_bcoords from the neck's world rotation R (row-major)
__device__ __forceinline__ int contour_row(const float *R, int n_rows)
{
    const float e = atan2f(-R[6], sqrtf(fmaf(R[0], R[0], R[3] * R[3])));
    const int y = (int)rintf(fminf(-e * 180.f / 3.14159265358979323846f, 39.f));      // half to even, as torch.round
    const int row = y >= 0 ? y : (y < -39 ? 78 : 39 - y);
    return min(row, n_rows - 1);
}

// C = A B (3x3 row-major)
__device__ __forceinline__ void mm3(const float *A, const float *B, float *C)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[r * 3 + c] = fmaf(A[r * 3 + 2], B[6 + c], fmaf(A[r * 3 + 1], B[3 + c], A[r * 3] * B[c]));
}
// C = A B^T
__device__ __forceinline__ void mm3_nt(const float *A, const float *B, float *C)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[r * 3 + c] = fmaf(A[r * 3 + 2], B[c * 3 + 2], fmaf(A[r * 3 + 1], B[c * 3 + 1], A[r * 3] * B[c * 3]));
}
// C = A^T B
__device__ __forceinline__ void mm3_tn(const float *A, const float *B, float *C)
{
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) C[r * 3 + c] = fmaf(A[6 + r], B[6 + c], fmaf(A[3 + r], B[3 + c], A[r] * B[c]));
}

// the optimised joint o (0 .. 51) -> its body-model joint, its key (0 global, 1 body, 2 left hand, 3 right hand), its place in the key
__device__ __forceinline__ void opt_joint(int o, int &j, int &key, int &jk)
{
    if (o == 0) { j = 0; key = 0; jk = 0; }
    else if (o < 22) { j = o; key = 1; jk = o - 1; }
    else if (o < 37) { j = o + 3; key = 2; jk = o - 22; }
    else { j = o + 3; key = 3; jk = o - 37; }
}
__device__ __forceinline__ int joint_to_opt(int j) { return j < 22 ? j : (j < 25 ? -1 : j - 3); }
__host__ __device__ __forceinline__ int key_joints(int key) { return key == 0 ? 1 : (key == 1 ? 21 : 15); }

struct FrameArgs {
    SoarSmplifyRig rig;
    SoarSmplifyArgs a;
};
struct BodyFrameArgs {
    SoarSmplifyRig rig;
    SoarSmplifyArgs a;
    SoarSmplifyBody b;
};
constexpr int S_DYN_ROWS = 79;      // rows of the contour table
constexpr int S_MAX_DYN = 17;       // contour landmarks

__device__ __forceinline__ const float *pose_ptr(const SoarSmplifyArgs &a, int key, bool init)
{
    switch (key) {
    case 0: return init ? a.global_orient0 : a.global_orient;
    case 1: return init ? a.body_pose0 : a.body_pose;
    case 2: return init ? a.left_hand_pose0 : a.left_hand_pose;
    default: return init ? a.right_hand_pose0 : a.right_hand_pose;
    }
}
__device__ __forceinline__ float *grad_ptr(const SoarSmplifyArgs &a, int key)
{
    switch (key) {
    case 0: return a.g_global_orient;
    case 1: return a.g_body_pose;
    case 2: return a.g_left_hand_pose;
    default: return a.g_right_hand_pose;
    }
}

// |p - p0|_2 of a row of n floats and, with g != nullptr, scale (p - p0) / |p - p0| (0 at a zero difference, as torch gives)
__device__ __forceinline__ float row_norm(const float *p, const float *p0, int n, float scale, float *g)
{
    float s = 0.f;
    for (int c = 0; c < n; c++) { const float d = p[c] - p0[c]; s = fmaf(d, d, s); }
    const float nrm = sqrtf(s);
    if (g)
        for (int c = 0; c < n; c++) g[c] = nrm > 0.f ? scale * ((p[c] - p0[c]) / nrm) : 0.f;
    return nrm;
}

// BODY: per-frame contour landmarks and the pose mean (SoarSmplifyBody).  Without it VS counts the gathered rows and the slots
// alike; with it rig.VS is the static rows' count, VS below the frame's active slots and PS3 the row length of posedirs.
template <bool BODY>
__global__ void __launch_bounds__(S_THREADS) smplify_frame_kernel(std::conditional_t<BODY, BodyFrameArgs, FrameArgs> fa)
{
    const SoarSmplifyRig &rig = fa.rig;
    const SoarSmplifyArgs &a = fa.a;
    const int n = blockIdx.x, tid = threadIdx.x;
    int VS_ = rig.VS, PS3_ = rig.VS * 3;
    if constexpr (BODY) { VS_ = rig.VS + 3 * fa.b.L_dyn; PS3_ = fa.b.VU * 3; }
    const int NB = rig.NBS + rig.NE, VS = VS_, VS3 = VS_ * 3, PS3 = PS3_, P = rig.P;
    __shared__ int smap[BODY ? S_MAX_VS : 1];       // slot -> row of the gathered arrays
    auto row_of = [&](int slot) -> int { if constexpr (BODY) return smap[slot]; else return slot; };
    auto col_of = [&](int col) -> int { if constexpr (BODY) return smap[col / 3] * 3 + col % 3; else return col; };

    __shared__ float coef[S_MAX_NB];
    __shared__ float Rl[SJ][9], Rw[SJ][9], Jr[SJ][3], tw[SJ][3], At[SJ][3];
    __shared__ float feat[SFEAT];            // R_j - I, j >= 1; in the adjoint: its gradient
    __shared__ float vposed[S_MAX_VS][3];    // in the adjoint: the gradient of v_posed
    __shared__ float Ts[S_MAX_VS][12];       // in the adjoint: the gradient of T
    __shared__ float vert[S_MAX_VS][3];      // in the adjoint: the gradient of the vertex
    __shared__ float kp[SKP][3], gk[SKP][3];
    __shared__ float gA[SJ][12], gRw[SJ][9], gtw[SJ][3], gJr[SJ][3], grel[SJ][3];
    __shared__ int par[SJ], depth[SJ];
    __shared__ int ptk[S_MAX_P], pti[S_MAX_P][3], ptd[S_MAX_P];
    __shared__ float ptw[S_MAX_P][3];
    __shared__ float red[S_THREADS];
    __shared__ float bpart[8][S_MAX_NB];
    __shared__ float tr[3];

    // ---- inputs ----
    if (tid < NB) coef[tid] = tid < rig.NBS ? a.betas[tid] : a.expression[(size_t)n * rig.NE + (tid - rig.NBS)];
    if (tid < 3) tr[tid] = a.transl[(size_t)n * 3 + tid];
    if (tid < SJ) {
        par[tid] = rig.parents[tid];
        const int o = joint_to_opt(tid);
        if (o >= 0) {
            int j, key, jk;
            opt_joint(o, j, key, jk);
            float x[6];
            const float *src = pose_ptr(a, key, false) + ((size_t)n * key_joints(key) + jk) * 6;
            for (int c = 0; c < 6; c++) x[c] = src[c];
            bool direct = true;
            if constexpr (BODY) {
                if ((fa.b.mean_mask >> tid) & 1ull) {              // rodrigues(log(R) + mean)
                    float R6[9], v[3];
                    rot6d(x, R6);
                    so3_log(R6, v);
                    for (int c = 0; c < 3; c++) v[c] += fa.b.pose_mean[tid * 3 + c];
                    rodrigues<3>(v, Rl[tid]);
                    direct = false;
                }
            }
            if (direct) rot6d(x, Rl[tid]);
        } else {
            const float *src = (tid == 22 ? a.jaw_pose : (tid == 23 ? a.leye_pose : a.reye_pose)) + (size_t)n * 3;
            bool direct = true;
            if constexpr (BODY) {
                if ((fa.b.mean_mask >> tid) & 1ull) {
                    const float v[3] = {src[0] + fa.b.pose_mean[tid * 3], src[1] + fa.b.pose_mean[tid * 3 + 1], src[2] + fa.b.pose_mean[tid * 3 + 2]};
                    rodrigues<3>(v, Rl[tid]);
                    direct = false;
                }
            }
            if (direct) rodrigues<3>(src, Rl[tid]);
        }
    }
    for (int p = tid; p < P; p += S_THREADS) {
        ptk[p] = rig.pt_kind[p];
        ptd[p] = rig.pt_dst[p];
        for (int k = 0; k < 3; k++) { pti[p][k] = rig.pt_idx[p * 3 + k]; ptw[p][k] = rig.pt_w[p * 3 + k]; }
    }
    for (int i = tid; i < SKP * 3; i += S_THREADS) (&kp[0][0])[i] = 0.f;
    __syncthreads();

    // ---- rest joints and pose features ----
    if (tid < SJ) {
        for (int c = 0; c < 3; c++) {
            float s = 0.f;
            const float *jd = rig.J_dirs + ((size_t)tid * 3 + c) * NB;
            for (int l = 0; l < NB; l++) s = fmaf(coef[l], jd[l], s);
            Jr[tid][c] = rig.J_template[tid * 3 + c] + s;
        }
    }
    for (int k = tid; k < SFEAT; k += S_THREADS) {
        const int j = 1 + k / 9, e = k % 9;
        feat[k] = Rl[j][e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    }
    __syncthreads();

    // ---- the chain: every lane multiplies down its own root path, associated like the reference's loop ----
    if (tid < SJ) {
        int path[S_MAX_DEPTH];
        int dp = 0;
        for (int p = tid; p >= 0 && dp < S_MAX_DEPTH; p = par[p]) path[dp++] = p;
        depth[tid] = dp - 1;
        float W[12];
        {
            const int r0 = path[dp - 1];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) W[r * 4 + c] = Rl[r0][r * 3 + c];
                W[r * 4 + 3] = Jr[r0][r];
            }
        }
        for (int d = dp - 2; d >= 0; d--) {
            const int j = path[d], p = path[d + 1];
            const float rel[3] = {Jr[j][0] - Jr[p][0], Jr[j][1] - Jr[p][1], Jr[j][2] - Jr[p][2]};
            float Nw[12];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++)
                    Nw[r * 4 + c] = fmaf(W[r * 4 + 2], Rl[j][6 + c], fmaf(W[r * 4 + 1], Rl[j][3 + c], W[r * 4] * Rl[j][c]));
                Nw[r * 4 + 3] = fmaf(W[r * 4 + 2], rel[2], fmaf(W[r * 4 + 1], rel[1], W[r * 4] * rel[0])) + W[r * 4 + 3];
            }
            for (int k = 0; k < 12; k++) W[k] = Nw[k];
        }
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Rw[tid][r * 3 + c] = W[r * 4 + c];
            tw[tid][r] = W[r * 4 + 3];
            At[tid][r] = W[r * 4 + 3] - fmaf(W[r * 4 + 2], Jr[tid][2], fmaf(W[r * 4 + 1], Jr[tid][1], W[r * 4] * Jr[tid][0]));
        }
    }
    if constexpr (BODY) {
        // ---- the contour landmarks' row: every thread derives it from Rw[neck]; the slot map and the landmarks' point entries ----
        __syncthreads();
        const SoarSmplifyBody &b = fa.b;
        const int row = b.L_dyn > 0 ? contour_row(Rw[b.neck], S_DYN_ROWS) : 0;
        if (tid < rig.VS) smap[tid] = tid;
        if (tid < b.L_dyn * 3) {
            const int l = tid / 3, k = tid % 3, slot = rig.VS + tid;
            const size_t at = ((size_t)row * b.L_dyn + l) * 3 + k;
            smap[slot] = b.dyn_vrow[at];
            const int p = b.dyn_point[l];
            if (p >= 0) { pti[p][k] = slot; ptw[p][k] = b.dyn_bary[at]; }
        }
        if (tid == 0 && b.rows_out && b.L_dyn > 0) b.rows_out[n] = row;
        __syncthreads();
    }
    // ---- shape blend and pose correctives of the gathered vertices: a thread per (vertex, component) column ----
    for (int col = tid; col < VS3; col += S_THREADS) {
        const int gcol = col_of(col);
        float sh = 0.f;
        const float *sd = rig.shapedirs + (size_t)gcol * NB;
        for (int l = 0; l < NB; l++) sh = fmaf(coef[l], sd[l], sh);
        const float *pd = rig.posedirs + gcol;
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;                 // three chains, joined in a fixed order
        for (int k = 0; k < SFEAT; k += 3) {
            acc0 = fmaf(feat[k], pd[(size_t)k * PS3], acc0);
            acc1 = fmaf(feat[k + 1], pd[(size_t)(k + 1) * PS3], acc1);
            acc2 = fmaf(feat[k + 2], pd[(size_t)(k + 2) * PS3], acc2);
        }
        (&vposed[0][0])[col] = ((acc0 + acc1) + acc2) + (rig.v_template[gcol] + sh);
    }
    __syncthreads();

    // ---- skinning ----
    if (tid < VS) {
        float T[12];
        for (int c = 0; c < 12; c++) T[c] = 0.f;
        const float *w = rig.lbs_weights + (size_t)row_of(tid) * SJ;
        for (int j = 0; j < SJ; j++) {
            const float wj = w[j];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) T[r * 4 + c] = fmaf(wj, Rw[j][r * 3 + c], T[r * 4 + c]);
                T[r * 4 + 3] = fmaf(wj, At[j][r], T[r * 4 + 3]);
            }
        }
        for (int c = 0; c < 12; c++) Ts[tid][c] = T[c];
        for (int r = 0; r < 3; r++)
            vert[tid][r] = fmaf(T[r * 4 + 2], vposed[tid][2], fmaf(T[r * 4 + 1], vposed[tid][1], T[r * 4] * vposed[tid][0])) + T[r * 4 + 3];
    }
    __syncthreads();

    // ---- model points -> keypoints ----
    if (tid < P) {
        float pos[3];
        if (ptk[tid] == 0) {
            for (int c = 0; c < 3; c++) pos[c] = tw[pti[tid][0]][c];
        } else {
            for (int c = 0; c < 3; c++)
                pos[c] = fmaf(ptw[tid][2], vert[pti[tid][2]][c], fmaf(ptw[tid][1], vert[pti[tid][1]][c], ptw[tid][0] * vert[pti[tid][0]][c]));
        }
        for (int c = 0; c < 3; c++) kp[ptd[tid]][c] = pos[c] + tr[c];
    }
    __syncthreads();
    if (tid == 0) {
        // convert_kps: keypoint 8 is the mean of 9 and 12, then x and y of 9 and 12 move
        for (int c = 0; c < 3; c++) kp[8][c] = 0.5f * (kp[9][c] + kp[12][c]);
        for (int c = 0; c < 2; c++) {
            const float k9 = kp[9][c], k12 = kp[12][c], k8 = kp[8][c];
            kp[9][c] = k9 + 0.25f * (k9 - k12) + 0.5f * (k8 - 0.5f * (k9 + k12));
            kp[12][c] = k12 + 0.25f * (k12 - k9) + 0.5f * (k8 - 0.5f * (k12 + k9));
        }
    }
    __syncthreads();

    // ---- projection, Geman-McClure ----
    float value = 0.f;
    if (tid < SKP) {
        const float *K = a.Ks + (size_t)n * 9, *M = a.w2c;
        const float p[3] = {kp[tid][0], kp[tid][1], kp[tid][2]};
        float pc[3], q[3];
        for (int r = 0; r < 3; r++) pc[r] = fmaf(M[r * 4 + 2], p[2], fmaf(M[r * 4 + 1], p[1], M[r * 4] * p[0])) + M[r * 4 + 3];
        for (int r = 0; r < 3; r++) q[r] = fmaf(K[r * 3 + 2], pc[2], fmaf(K[r * 3 + 1], pc[1], K[r * 3] * pc[0]));
        const float zc = fmaxf(q[2], 1e-5f);
        const float uv[2] = {q[0] / zc, q[1] / zc};
        if (a.kps) { a.kps[((size_t)n * SKP + tid) * 2] = uv[0]; a.kps[((size_t)n * SKP + tid) * 2 + 1] = uv[1]; }
        const float *t = a.target_kps + ((size_t)n * SKP + tid) * 3;
        float conf = t[2] * rig.kp_mask[tid];
        if (a.ignore_hands && tid >= 25 && tid < SKP - 70) conf = 0.f;
        const float scale = a.target_scales[n], s2 = a.sigma * a.sigma;
        const float tgt[2] = {t[0] * a.img_w, t[1] * a.img_h};
        float guv[2];
        for (int c = 0; c < 2; c++) {
            const float r = (uv[c] - tgt[c]) / scale * 200.f;
            const float r2 = r * r, den = s2 + r2;
            value += (s2 * r2) / den * conf;
            guv[c] = a.kp_scale * conf * (2.f * s2 * s2 * r / (den * den)) * 200.f / scale;
        }
        const float gq[3] = {guv[0] / zc, guv[1] / zc, q[2] >= 1e-5f ? -(guv[0] * uv[0] + guv[1] * uv[1]) / zc : 0.f};
        float gpc[3];
        for (int c = 0; c < 3; c++) gpc[c] = fmaf(K[6 + c], gq[2], fmaf(K[3 + c], gq[1], K[c] * gq[0]));
        for (int c = 0; c < 3; c++) gk[tid][c] = fmaf(M[8 + c], gpc[2], fmaf(M[4 + c], gpc[1], M[c] * gpc[0]));
    }
    red[tid] = value;
    __syncthreads();
    for (int s = S_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0 && a.frame_loss) a.frame_loss[(size_t)n * 2] = a.kp_scale * red[0];
    if (!a.grads) return;
    __syncthreads();

    // ================= the adjoint =================
    if (tid == 0) {
        // convert_kps: the values scattered to 9 and 12 get (x, y) 1 g9 - 1/2 g12 + 1/2 g8' with g8' = g8 + (g9 + g12) / 2, z: g + g8 / 2;
        // whatever was scattered to 8 is overwritten
        for (int c = 0; c < 3; c++) {
            const float g8 = gk[8][c], g9 = gk[9][c], g12 = gk[12][c];
            if (c < 2) {
                const float g8t = g8 + 0.5f * (g9 + g12);
                gk[9][c] = g9 - 0.5f * g12 + 0.5f * g8t;
                gk[12][c] = g12 - 0.5f * g9 + 0.5f * g8t;
            } else {
                gk[9][c] = g9 + 0.5f * g8;
                gk[12][c] = g12 + 0.5f * g8;
            }
            gk[8][c] = 0.f;
        }
    }
    __syncthreads();
    // points -> vertices, joints, transl: every target gathers its points in ascending order
    if (tid < VS) {
        float g[3] = {0.f, 0.f, 0.f};
        for (int p = 0; p < P; p++) {
            if (ptk[p] == 0) continue;
            for (int k = 0; k < 3; k++)
                if (pti[p][k] == tid)
                    for (int c = 0; c < 3; c++) g[c] = fmaf(ptw[p][k], gk[ptd[p]][c], g[c]);
        }
        // vertex = T [v_posed, 1]
        float gvp[3];
        for (int c = 0; c < 3; c++) gvp[c] = fmaf(Ts[tid][8 + c], g[2], fmaf(Ts[tid][4 + c], g[1], Ts[tid][c] * g[0]));
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Ts[tid][r * 4 + c] = g[r] * vposed[tid][c];
            Ts[tid][r * 4 + 3] = g[r];
        }
        for (int c = 0; c < 3; c++) vposed[tid][c] = gvp[c];
    }
    if (tid < SJ) {
        float g[3] = {0.f, 0.f, 0.f};
        for (int p = 0; p < P; p++)
            if (ptk[p] == 0 && pti[p][0] == tid)
                for (int c = 0; c < 3; c++) g[c] += gk[ptd[p]][c];
        for (int c = 0; c < 3; c++) gtw[tid][c] = g[c];
    }
    float preserve = 0.f;              // this thread's share of the frame's preserve term
    if (tid == S_THREADS - 1) {
        float g[3] = {0.f, 0.f, 0.f}, gp[3];
        for (int p = 0; p < P; p++)
            for (int c = 0; c < 3; c++) g[c] += gk[ptd[p]][c];
        preserve += a.row_scale * row_norm(a.transl + (size_t)n * 3, a.transl0 + (size_t)n * 3, 3, a.row_scale, gp);
        for (int c = 0; c < 3; c++) a.g_transl[(size_t)n * 3 + c] = g[c] + gp[c];
        if (rig.NE > 0)
            preserve += a.row_scale * row_norm(a.expression + (size_t)n * rig.NE, a.expression0 + (size_t)n * rig.NE, rig.NE, 0.f, nullptr);
    }
    __syncthreads();

    // T = sum_j w_vj A_j: the gradient of A_j gathers the vertices in ascending order
    for (int i = tid; i < SJ * 12; i += S_THREADS) {
        const int j = i / 12, e = i % 12;
        float s = 0.f;
        for (int v = 0; v < VS; v++) s = fmaf(rig.lbs_weights[(size_t)row_of(v) * SJ + j], Ts[v][e], s);
        gA[j][e] = s;
    }
    // pose correctives: the gradient of feature k is row k of posedirs against the gradient of v_posed -- a wave per row
    {
        const int wave = tid >> 6, lane = tid & 63;
        for (int k = wave; k < SFEAT; k += S_THREADS / 64) {
            const float *pd = rig.posedirs + (size_t)k * PS3;
            float s = 0.f;
            for (int col = lane; col < VS3; col += 64) s = fmaf(pd[col_of(col)], (&vposed[0][0])[col], s);
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (lane == 0) feat[k] = s;
        }
    }
    __syncthreads();

    // A_j = [Rw_j | tw_j - Rw_j J_j]
    if (tid < SJ) {
        const float *g = gA[tid];
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) gRw[tid][r * 3 + c] = g[r * 4 + c] - g[r * 4 + 3] * Jr[tid][c];
            gtw[tid][r] += g[r * 4 + 3];
        }
        for (int c = 0; c < 3; c++)
            gJr[tid][c] = -fmaf(Rw[tid][6 + c], g[11], fmaf(Rw[tid][3 + c], g[7], Rw[tid][c] * g[3]));
    }
    __syncthreads();
    // the chain, leaves first: a joint adds its children (ascending) once they are complete
    int max_depth = 0;
    for (int j = 0; j < SJ; j++) max_depth = max(max_depth, depth[j]);
    for (int lvl = max_depth - 1; lvl >= 0; lvl--) {
        if (tid < SJ && depth[tid] == lvl) {
            for (int ch = tid + 1; ch < SJ; ch++) {
                if (par[ch] != tid) continue;
                const float rel[3] = {Jr[ch][0] - Jr[tid][0], Jr[ch][1] - Jr[tid][1], Jr[ch][2] - Jr[tid][2]};
                float t[9];
                mm3_nt(gRw[ch], Rl[ch], t);                        // Rw_c = Rw_p R_c
                for (int r = 0; r < 3; r++) {
                    for (int c = 0; c < 3; c++) gRw[tid][r * 3 + c] += t[r * 3 + c] + gtw[ch][r] * rel[c];      // tw_c = Rw_p rel_c + tw_p
                    gtw[tid][r] += gtw[ch][r];
                }
            }
        }
        __syncthreads();
    }
    if (tid < SJ) {
        const int p = par[tid];
        for (int c = 0; c < 3; c++)
            grel[tid][c] = p >= 0 ? fmaf(Rw[p][6 + c], gtw[tid][2], fmaf(Rw[p][3 + c], gtw[tid][1], Rw[p][c] * gtw[tid][0])) : gtw[tid][c];
    }
    __syncthreads();
    if (tid < SJ) {
        // rest joints: J_j enters A_j, rel_j and the rel of its children
        for (int c = 0; c < 3; c++) {
            float g = gJr[tid][c] + grel[tid][c];
            for (int ch = tid + 1; ch < SJ; ch++)
                if (par[ch] == tid) g -= grel[ch][c];
            gJr[tid][c] = g;
        }
        // the joint's own rotation: Rw_j = Rw_p R_j, plus its pose feature
        const int o = joint_to_opt(tid);
        if (o >= 0) {
            const int p = par[tid];
            float gR[9];
            if (p >= 0) mm3_tn(Rw[p], gRw[tid], gR);
            else
                for (int e = 0; e < 9; e++) gR[e] = gRw[tid][e];
            if (tid >= 1)
                for (int e = 0; e < 9; e++) gR[e] += feat[(tid - 1) * 9 + e];
            int j, key, jk;
            opt_joint(o, j, key, jk);
            const size_t at = ((size_t)n * key_joints(key) + jk) * 6;
            const float *src = pose_ptr(a, key, false) + at, *src0 = pose_ptr(a, key, true) + at;
            float x[6], x0[6], gx[6], gp[6];
            for (int c = 0; c < 6; c++) { x[c] = src[c]; x0[c] = src0[c]; }
            if constexpr (BODY) {
                if ((fa.b.mean_mask >> tid) & 1ull) {              // back through rodrigues(log(R6) + mean)
                    float R6[9], v[3], gv[3];
                    rot6d(x, R6);
                    so3_log(R6, v);
                    for (int c = 0; c < 3; c++) v[c] += fa.b.pose_mean[tid * 3 + c];
                    rodrigues_backward(v, gR, gv);
                    so3_log_backward(R6, gv, gR);
                }
            }
            rot6d_backward(x, gR, gx);
            preserve += a.pose_scale[key] * row_norm(x, x0, 6, a.pose_scale[key], gp);
            float *dst = grad_ptr(a, key) + at;
            for (int c = 0; c < 6; c++) dst[c] = gx[c] + gp[c];
        } else {
            const float *src = tid == 22 ? a.jaw_pose : (tid == 23 ? a.leye_pose : a.reye_pose);
            const float *src0 = tid == 22 ? a.jaw_pose0 : (tid == 23 ? a.leye_pose0 : a.reye_pose0);
            preserve += a.row_scale * row_norm(src + (size_t)n * 3, src0 + (size_t)n * 3, 3, 0.f, nullptr);
        }
    }
    red[tid] = preserve;
    __syncthreads();

    // betas: v_shaped = v_template + shapedirs coef (its gradient is v_posed's), J = J_template + J_dirs coef
    {
        const int q = tid >> 5, l0 = tid & 31;
        const int per = (VS3 + 7) / 8, c0 = q * per, c1 = min(VS3, c0 + per);
        for (int l = l0; l < rig.NBS; l += 32) {
            float s = 0.f;
            for (int col = c0; col < c1; col++) s = fmaf(rig.shapedirs[(size_t)col_of(col) * NB + l], (&vposed[0][0])[col], s);
            bpart[q][l] = s;
        }
    }
    for (int s = S_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.frame_loss[(size_t)n * 2 + 1] = red[0];
    if (tid < rig.NBS) {
        float s = 0.f;
        for (int q = 0; q < 8; q++) s += bpart[q][tid];
        float sj = 0.f;
        for (int jc = 0; jc < SJ * 3; jc++) sj = fmaf(rig.J_dirs[(size_t)jc * NB + tid], (&gJr[0][0])[jc], sj);
        a.frame_betas[(size_t)n * rig.NBS + tid] = s + sj;
    }
}

// ---- the smooth term and the sums over frames ----
__device__ __forceinline__ void load6(const float *p, float *x) { for (int c = 0; c < 6; c++) x[c] = p[c]; }

// theta^2 of M = A B^T and its gradient G with respect to M
__device__ __forceinline__ float angle2(const float *A, const float *B, float *G)
{
    float M[9];
    mm3_nt(A, B, M);
    const float ax[3] = {0.5f * (M[7] - M[5]), 0.5f * (M[2] - M[6]), 0.5f * (M[3] - M[1])};
    const float c = 0.5f * (M[0] + M[4] + M[8] - 1.f);
    const float s = sqrtf(dot3(ax, ax));
    const float th = atan2f(s, c);
    const float den = fmaf(s, s, c * c);
    const float gs = s > 0.f ? 2.f * th * c / den / s : 0.f;      // times the axial vector: the gradient of |a|
    const float gc = 0.5f * (den > 0.f ? -2.f * th * s / den : 0.f);
    const float ga[3] = {0.5f * gs * ax[0], 0.5f * gs * ax[1], 0.5f * gs * ax[2]};
    G[0] = gc; G[4] = gc; G[8] = gc;
    G[7] = ga[0]; G[5] = -ga[0];
    G[2] = ga[1]; G[6] = -ga[1];
    G[3] = ga[2]; G[1] = -ga[2];
    return th * th;
}

__device__ __forceinline__ double block_sum(double v, double *buf)
{
    const int tid = threadIdx.x;
    __syncthreads();
    buf[tid] = v;
    __syncthreads();
    for (int s = F_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) buf[tid] += buf[tid + s];
        __syncthreads();
    }
    return buf[0];
}

__global__ void __launch_bounds__(F_THREADS) smplify_finish_kernel(SoarSmplifyArgs a, int NBS)
{
    __shared__ double buf[F_THREADS];
    const int tid = threadIdx.x, N = a.N;
    double smooth = 0.0;
    for (int i = tid; i < N * SOPT && N > 1; i += F_THREADS) {
        const int t = i / SOPT;
        int j, key, jk;
        opt_joint(i % SOPT, j, key, jk);
        const int JK = key_joints(key);
        const float *base = pose_ptr(a, key, false);
        const float sc = a.smooth_scale[key];
        float x[6], y[6], R[9], Q[9], G[9], gR[9];
        load6(base + ((size_t)t * JK + jk) * 6, x);
        rot6d(x, R);
        for (int e = 0; e < 9; e++) gR[e] = 0.f;
        if (t > 0) {                                             // M = R[t] R[t-1]^T: dR[t] = G R[t-1]
            load6(base + ((size_t)(t - 1) * JK + jk) * 6, y);
            rot6d(y, Q);
            (void)angle2(R, Q, G);
            float tmp[9];
            mm3(G, Q, tmp);
            for (int e = 0; e < 9; e++) gR[e] += tmp[e];
        }
        if (t < N - 1) {                                         // M = R[t+1] R[t]^T: dR[t] = G^T R[t+1]; the pair's value is frame t's
            load6(base + ((size_t)(t + 1) * JK + jk) * 6, y);
            rot6d(y, Q);
            smooth += (double)(sc * angle2(Q, R, G));
            float tmp[9];
            mm3_tn(G, Q, tmp);
            for (int e = 0; e < 9; e++) gR[e] += tmp[e];
        }
        float gx[6];
        rot6d_backward(x, gR, gx);
        float *dst = grad_ptr(a, key) + ((size_t)t * JK + jk) * 6;
        for (int c = 0; c < 6; c++) dst[c] = fmaf(sc, gx[c], dst[c]);
    }
    const double smooth_sum = block_sum(smooth, buf);
    double kpv = 0.0, prv = 0.0;
    for (int t = tid; t < N; t += F_THREADS) { kpv += (double)a.frame_loss[(size_t)t * 2]; prv += (double)a.frame_loss[(size_t)t * 2 + 1]; }
    const double kp_sum = block_sum(kpv, buf);
    const double pr_sum = block_sum(prv, buf);
    // betas: one row for all frames
    float nb = 0.f;
    for (int l = 0; l < NBS; l++) { const float d = a.betas[l] - a.betas0[l]; nb = fmaf(d, d, nb); }
    nb = sqrtf(nb);
    if (tid < NBS) {
        double s = 0.0;
        for (int t = 0; t < N; t++) s += (double)a.frame_betas[(size_t)t * NBS + tid];
        const float gp = nb > 0.f ? a.w_preserve * ((a.betas[tid] - a.betas0[tid]) / nb) : 0.f;
        a.g_betas[tid] = (float)s + gp;
    }
    if (tid == 0) {
        a.loss[0] = (float)kp_sum;
        a.loss[1] = (float)(pr_sum + (double)(a.w_preserve * nb));
        a.loss[2] = (float)smooth_sum;
    }
}

__global__ void __launch_bounds__(256) target_scales_kernel(int N, const float *__restrict__ t, float img_w, float img_h, float *__restrict__ out)
{
    __shared__ float lo[2][256], hi[2][256];
    const int n = blockIdx.x, tid = threadIdx.x;
    float mn[2] = {3.0e38f, 3.0e38f}, mx[2] = {-3.0e38f, -3.0e38f};
    if (tid < SKP) {
        const float *p = t + ((size_t)n * SKP + tid) * 3;
        if (p[2] > 0.3f) {
            const float x = p[0] * img_w, y = p[1] * img_h;
            mn[0] = mx[0] = x;
            mn[1] = mx[1] = y;
        }
    }
    for (int c = 0; c < 2; c++) { lo[c][tid] = mn[c]; hi[c][tid] = mx[c]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
            for (int c = 0; c < 2; c++) { lo[c][tid] = fminf(lo[c][tid], lo[c][tid + s]); hi[c][tid] = fmaxf(hi[c][tid], hi[c][tid + s]); }
        __syncthreads();
    }
    if (tid == 0) out[n] = hi[0][0] < lo[0][0] ? -1.f : fmaxf(hi[0][0] - lo[0][0], hi[1][0] - lo[1][0]);
}

// ---- the static model points alone (soar_smplify_model_points; pose_init.hip searches over them) ----
// The forward half of smplify_frame_kernel up to the model points, statement for statement, for ALL PA = 55 + NX + L static points
// (mp_idx / mp_w: point p < 55 is joint p, the others weighted sums of gathered rows) instead of the P mapped ones, and without the
// contour table: the static rows are the first VS of the gathered arrays, PS3 their posedirs row length.  The pose mean is applied.
struct PointsArgs {
    SoarSmplifyRig rig;
    SoarSmplifyArgs a;
    const float *pose_mean;
    uint64_t mean_mask;
    const int32_t *mp_idx;      // [PA][3]
    const float *mp_w;          // [PA][3]
    float *out;                 // [N][PA][3]
    int PA, PS3;
};

__global__ void __launch_bounds__(S_THREADS) smplify_points_kernel(PointsArgs fa)
{
    const SoarSmplifyRig &rig = fa.rig;
    const SoarSmplifyArgs &a = fa.a;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int NB = rig.NBS + rig.NE, VS = rig.VS, VS3 = rig.VS * 3, PS3 = fa.PS3;
    __shared__ float coef[S_MAX_NB];
    __shared__ float Rl[SJ][9], Rw[SJ][9], Jr[SJ][3], tw[SJ][3], At[SJ][3];
    __shared__ float feat[SFEAT];
    __shared__ float vposed[S_MAX_VS][3], vert[S_MAX_VS][3];
    __shared__ int par[SJ];
    __shared__ float tr[3];

    if (tid < NB) coef[tid] = tid < rig.NBS ? a.betas[tid] : a.expression[(size_t)n * rig.NE + (tid - rig.NBS)];
    if (tid < 3) tr[tid] = a.transl[(size_t)n * 3 + tid];
    if (tid < SJ) {
        par[tid] = rig.parents[tid];
        const bool mean = (fa.mean_mask >> tid) & 1ull;
        const int o = joint_to_opt(tid);
        if (o >= 0) {
            int j, key, jk;
            opt_joint(o, j, key, jk);
            float x[6];
            const float *src = pose_ptr(a, key, false) + ((size_t)n * key_joints(key) + jk) * 6;
            for (int c = 0; c < 6; c++) x[c] = src[c];
            if (mean) {                                            // rodrigues(log(R) + mean)
                float R6[9], v[3];
                rot6d(x, R6);
                so3_log(R6, v);
                for (int c = 0; c < 3; c++) v[c] += fa.pose_mean[tid * 3 + c];
                rodrigues<3>(v, Rl[tid]);
            } else {
                rot6d(x, Rl[tid]);
            }
        } else {
            const float *src = (tid == 22 ? a.jaw_pose : (tid == 23 ? a.leye_pose : a.reye_pose)) + (size_t)n * 3;
            if (mean) {
                const float v[3] = {src[0] + fa.pose_mean[tid * 3], src[1] + fa.pose_mean[tid * 3 + 1], src[2] + fa.pose_mean[tid * 3 + 2]};
                rodrigues<3>(v, Rl[tid]);
            } else {
                rodrigues<3>(src, Rl[tid]);
            }
        }
    }
    __syncthreads();
    // ---- rest joints and pose features ----
    if (tid < SJ) {
        for (int c = 0; c < 3; c++) {
            float s = 0.f;
            const float *jd = rig.J_dirs + ((size_t)tid * 3 + c) * NB;
            for (int l = 0; l < NB; l++) s = fmaf(coef[l], jd[l], s);
            Jr[tid][c] = rig.J_template[tid * 3 + c] + s;
        }
    }
    for (int k = tid; k < SFEAT; k += S_THREADS) {
        const int j = 1 + k / 9, e = k % 9;
        feat[k] = Rl[j][e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
    }
    __syncthreads();
    // ---- the chain ----
    if (tid < SJ) {
        int path[S_MAX_DEPTH];
        int dp = 0;
        for (int p = tid; p >= 0 && dp < S_MAX_DEPTH; p = par[p]) path[dp++] = p;
        float W[12];
        {
            const int r0 = path[dp - 1];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) W[r * 4 + c] = Rl[r0][r * 3 + c];
                W[r * 4 + 3] = Jr[r0][r];
            }
        }
        for (int d = dp - 2; d >= 0; d--) {
            const int j = path[d], p = path[d + 1];
            const float rel[3] = {Jr[j][0] - Jr[p][0], Jr[j][1] - Jr[p][1], Jr[j][2] - Jr[p][2]};
            float Nw[12];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++)
                    Nw[r * 4 + c] = fmaf(W[r * 4 + 2], Rl[j][6 + c], fmaf(W[r * 4 + 1], Rl[j][3 + c], W[r * 4] * Rl[j][c]));
                Nw[r * 4 + 3] = fmaf(W[r * 4 + 2], rel[2], fmaf(W[r * 4 + 1], rel[1], W[r * 4] * rel[0])) + W[r * 4 + 3];
            }
            for (int k = 0; k < 12; k++) W[k] = Nw[k];
        }
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Rw[tid][r * 3 + c] = W[r * 4 + c];
            tw[tid][r] = W[r * 4 + 3];
            At[tid][r] = W[r * 4 + 3] - fmaf(W[r * 4 + 2], Jr[tid][2], fmaf(W[r * 4 + 1], Jr[tid][1], W[r * 4] * Jr[tid][0]));
        }
    }
    // ---- shape blend and pose correctives of the static rows ----
    for (int col = tid; col < VS3; col += S_THREADS) {
        float sh = 0.f;
        const float *sd = rig.shapedirs + (size_t)col * NB;
        for (int l = 0; l < NB; l++) sh = fmaf(coef[l], sd[l], sh);
        const float *pd = rig.posedirs + col;
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
        for (int k = 0; k < SFEAT; k += 3) {
            acc0 = fmaf(feat[k], pd[(size_t)k * PS3], acc0);
            acc1 = fmaf(feat[k + 1], pd[(size_t)(k + 1) * PS3], acc1);
            acc2 = fmaf(feat[k + 2], pd[(size_t)(k + 2) * PS3], acc2);
        }
        (&vposed[0][0])[col] = ((acc0 + acc1) + acc2) + (rig.v_template[col] + sh);
    }
    __syncthreads();
    // ---- skinning ----
    if (tid < VS) {
        float T[12];
        for (int c = 0; c < 12; c++) T[c] = 0.f;
        const float *w = rig.lbs_weights + (size_t)tid * SJ;
        for (int j = 0; j < SJ; j++) {
            const float wj = w[j];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) T[r * 4 + c] = fmaf(wj, Rw[j][r * 3 + c], T[r * 4 + c]);
                T[r * 4 + 3] = fmaf(wj, At[j][r], T[r * 4 + 3]);
            }
        }
        for (int r = 0; r < 3; r++)
            vert[tid][r] = fmaf(T[r * 4 + 2], vposed[tid][2], fmaf(T[r * 4 + 1], vposed[tid][1], T[r * 4] * vposed[tid][0])) + T[r * 4 + 3];
    }
    __syncthreads();
    // ---- the model points ----
    for (int p = tid; p < fa.PA; p += S_THREADS) {
        float pos[3];
        if (p < SJ) {
            for (int c = 0; c < 3; c++) pos[c] = tw[p][c];
        } else {
            const int i0 = fa.mp_idx[p * 3], i1 = fa.mp_idx[p * 3 + 1], i2 = fa.mp_idx[p * 3 + 2];
            const float w0 = fa.mp_w[p * 3], w1 = fa.mp_w[p * 3 + 1], w2 = fa.mp_w[p * 3 + 2];
            for (int c = 0; c < 3; c++) pos[c] = fmaf(w2, vert[i2][c], fmaf(w1, vert[i1][c], w0 * vert[i0][c]));
        }
        for (int c = 0; c < 3; c++) fa.out[((size_t)n * fa.PA + p) * 3 + c] = pos[c] + tr[c];
    }
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_smplify_objective(const SoarSmplifyRig *rig, const SoarSmplifyArgs *args, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!rig || !args) { set_error("soar_smplify_objective: NULL rig / args"); return 1; }
    const SoarSmplifyRig &r = *rig;
    const SoarSmplifyArgs &a = *args;
    if (r.J != SJ || r.NBS < 1 || r.NE < 0 || r.NBS + r.NE > S_MAX_NB || r.VS < 1 || r.VS > S_MAX_VS || r.P < 0 || r.P > S_MAX_P) {
        set_error("soar_smplify_objective: need J = %d, 1 <= NBS, NBS + NE <= %d, 1 <= VS <= %d, 0 <= P <= %d (J=%d NBS=%d NE=%d VS=%d P=%d)",
                  SJ, S_MAX_NB, S_MAX_VS, S_MAX_P, r.J, r.NBS, r.NE, r.VS, r.P);
        return 1;
    }
    if (a.N < 0 || a.N > 0x7fffffff / (SKP * 3)) { set_error("soar_smplify_objective: N=%d out of range", a.N); return 1; }
    if (!r.J_template || !r.J_dirs || !r.parents || !r.v_template || !r.shapedirs || !r.posedirs || !r.lbs_weights || !r.kp_mask
        || (r.P > 0 && (!r.pt_kind || !r.pt_idx || !r.pt_w || !r.pt_dst))) {
        set_error("soar_smplify_objective: NULL rig table");
        return 1;
    }
    if (a.N == 0) return 0;
    if (!a.global_orient || !a.body_pose || !a.left_hand_pose || !a.right_hand_pose || !a.betas || !a.transl || !a.jaw_pose || !a.leye_pose
        || !a.reye_pose || (r.NE > 0 && !a.expression) || !a.Ks || !a.w2c || !a.target_kps || !a.target_scales) {
        set_error("soar_smplify_objective: NULL input");
        return 1;
    }
    if (a.grads && (!a.global_orient0 || !a.body_pose0 || !a.left_hand_pose0 || !a.right_hand_pose0 || !a.betas0 || !a.transl0 || !a.jaw_pose0
                    || !a.leye_pose0 || !a.reye_pose0 || (r.NE > 0 && !a.expression0) || !a.g_global_orient || !a.g_body_pose
                    || !a.g_left_hand_pose || !a.g_right_hand_pose || !a.g_betas || !a.g_transl || !a.loss || !a.frame_betas || !a.frame_loss)) {
        set_error("soar_smplify_objective: NULL initial value, gradient or scratch pointer");
        return 1;
    }
    if (!a.grads && !a.kps && !a.frame_loss) { set_error("soar_smplify_objective: nothing to compute (grads = 0, kps = NULL)"); return 1; }
    if (!(a.sigma > 0.f)) { set_error("soar_smplify_objective: sigma must be positive"); return 1; }
    FrameArgs fa;
    fa.rig = r;
    fa.a = a;
    hipLaunchKernelGGL(smplify_frame_kernel<false>, dim3(a.N), dim3(S_THREADS), 0, stream, fa);
    SOAR_LAUNCH_OK("smplify_frame", stream, 0);
    if (a.grads) {
        hipLaunchKernelGGL(smplify_finish_kernel, dim3(1), dim3(F_THREADS), 0, stream, a, r.NBS);
        SOAR_LAUNCH_OK("smplify_finish", stream, 0);
    }
    return 0;
}

extern "C" int soar_smplify_objective_body(const SoarSmplifyRig *rig, const SoarSmplifyBody *body, const SoarSmplifyArgs *args, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!rig || !body || !args) { set_error("soar_smplify_objective_body: NULL rig / body / args"); return 1; }
    const SoarSmplifyRig &r = *rig;
    const SoarSmplifyBody &b = *body;
    const SoarSmplifyArgs &a = *args;
    if (a.N <= 0) { set_error("soar_smplify_objective_body: N=%d: need at least one frame", a.N); return 1; }
    if (b.L_dyn < 0 || b.L_dyn > S_MAX_DYN || (b.L_dyn > 0 && (b.n_rows != S_DYN_ROWS || b.neck < 0 || b.neck >= SJ))) {
        set_error("soar_smplify_objective_body: need 0 <= L_dyn <= %d, and with L_dyn > 0 n_rows = %d and 0 <= neck < %d (L_dyn=%d n_rows=%d neck=%d)",
                  S_MAX_DYN, S_DYN_ROWS, SJ, b.L_dyn, b.n_rows, b.neck);
        return 1;
    }
    if (r.VS < 1 || r.VS + 3 * b.L_dyn > S_MAX_VS || b.VU < r.VS) {
        set_error("soar_smplify_objective_body: %d static slots + 3 x %d contour slots exceed the %d a frame may use, or the union VU=%d is below "
                  "the static rows", r.VS, b.L_dyn, S_MAX_VS, b.VU);
        return 1;
    }
    if ((b.L_dyn > 0 && (!b.dyn_vrow || !b.dyn_bary || !b.dyn_point)) || (b.mean_mask != 0 && !b.pose_mean) || (b.mean_mask >> SJ) != 0) {
        set_error("soar_smplify_objective_body: NULL contour table or pose_mean, or a mean_mask bit past joint %d", SJ - 1);
        return 1;
    }
    if (b.L_dyn == 0 && b.mean_mask == 0) {                       // nothing to add: the static kernel, its bits
        if (b.VU != r.VS) { set_error("soar_smplify_objective_body: without a contour table VU=%d must equal VS=%d", b.VU, r.VS); return 1; }
        return soar_smplify_objective(rig, args, stream_);
    }
    // the remaining checks are soar_smplify_objective's, on a rig whose VS is the static rows' count
    if (r.J != SJ || r.NBS < 1 || r.NE < 0 || r.NBS + r.NE > S_MAX_NB || r.P < 0 || r.P > S_MAX_P) {
        set_error("soar_smplify_objective_body: need J = %d, 1 <= NBS, NBS + NE <= %d, 0 <= P <= %d (J=%d NBS=%d NE=%d P=%d)",
                  SJ, S_MAX_NB, S_MAX_P, r.J, r.NBS, r.NE, r.P);
        return 1;
    }
    if (a.N > 0x7fffffff / (SKP * 3)) { set_error("soar_smplify_objective_body: N=%d out of range", a.N); return 1; }
    if (!r.J_template || !r.J_dirs || !r.parents || !r.v_template || !r.shapedirs || !r.posedirs || !r.lbs_weights || !r.kp_mask
        || (r.P > 0 && (!r.pt_kind || !r.pt_idx || !r.pt_w || !r.pt_dst))) {
        set_error("soar_smplify_objective_body: NULL rig table");
        return 1;
    }
    if (!a.global_orient || !a.body_pose || !a.left_hand_pose || !a.right_hand_pose || !a.betas || !a.transl || !a.jaw_pose || !a.leye_pose
        || !a.reye_pose || (r.NE > 0 && !a.expression) || !a.Ks || !a.w2c || !a.target_kps || !a.target_scales) {
        set_error("soar_smplify_objective_body: NULL input");
        return 1;
    }
    if (a.grads && (!a.global_orient0 || !a.body_pose0 || !a.left_hand_pose0 || !a.right_hand_pose0 || !a.betas0 || !a.transl0 || !a.jaw_pose0
                    || !a.leye_pose0 || !a.reye_pose0 || (r.NE > 0 && !a.expression0) || !a.g_global_orient || !a.g_body_pose
                    || !a.g_left_hand_pose || !a.g_right_hand_pose || !a.g_betas || !a.g_transl || !a.loss || !a.frame_betas || !a.frame_loss)) {
        set_error("soar_smplify_objective_body: NULL initial value, gradient or scratch pointer");
        return 1;
    }
    if (!a.grads && !a.kps && !a.frame_loss) { set_error("soar_smplify_objective_body: nothing to compute (grads = 0, kps = NULL)"); return 1; }
    if (!(a.sigma > 0.f)) { set_error("soar_smplify_objective_body: sigma must be positive"); return 1; }
    BodyFrameArgs fa;
    fa.rig = r;
    fa.a = a;
    fa.b = b;
    hipLaunchKernelGGL(smplify_frame_kernel<true>, dim3(a.N), dim3(S_THREADS), 0, stream, fa);
    SOAR_LAUNCH_OK("smplify_frame_body", stream, 0);
    if (a.grads) {
        hipLaunchKernelGGL(smplify_finish_kernel, dim3(1), dim3(F_THREADS), 0, stream, a, r.NBS);
        SOAR_LAUNCH_OK("smplify_finish", stream, 0);
    }
    return 0;
}

extern "C" int soar_smplify_model_points(const SoarSmplifyRig *rig, const SoarSmplifyBody *body, const SoarSmplifyArgs *args, int32_t PA,
                                         const int32_t *mp_idx, const float *mp_w, float *points, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!rig || !args) { set_error("soar_smplify_model_points: NULL rig / args"); return 1; }
    const SoarSmplifyRig &r = *rig;
    const SoarSmplifyArgs &a = *args;
    if (r.J != SJ || r.NBS < 1 || r.NE < 0 || r.NBS + r.NE > S_MAX_NB || r.VS < 1 || r.VS > S_MAX_VS) {
        set_error("soar_smplify_model_points: need J = %d, 1 <= NBS, NBS + NE <= %d, 1 <= VS <= %d (J=%d NBS=%d NE=%d VS=%d)",
                  SJ, S_MAX_NB, S_MAX_VS, r.J, r.NBS, r.NE, r.VS);
        return 1;
    }
    if (a.N <= 0 || PA < SJ || (int64_t)a.N * PA > 0x7fffffff / 3) {
        set_error("soar_smplify_model_points: need N >= 1 and PA >= %d with N PA 3 below 2^31 (N=%d PA=%d)", SJ, a.N, PA);
        return 1;
    }
    int PS3 = r.VS * 3;
    uint64_t mean_mask = 0;
    if (body) {
        if (body->VU < r.VS || (body->mean_mask >> SJ) != 0 || (body->mean_mask != 0 && !body->pose_mean)) {
            set_error("soar_smplify_model_points: the union VU=%d is below the static rows VS=%d, or a mean_mask without pose_mean or past "
                      "joint %d", body->VU, r.VS, SJ - 1);
            return 1;
        }
        PS3 = body->VU * 3;
        mean_mask = body->mean_mask;
    }
    if (!r.J_template || !r.J_dirs || !r.parents || !r.v_template || !r.shapedirs || !r.posedirs || !r.lbs_weights
        || (PA > SJ && (!mp_idx || !mp_w))) {
        set_error("soar_smplify_model_points: NULL rig table");
        return 1;
    }
    if (!a.global_orient || !a.body_pose || !a.left_hand_pose || !a.right_hand_pose || !a.betas || !a.transl || !a.jaw_pose || !a.leye_pose
        || !a.reye_pose || (r.NE > 0 && !a.expression) || !points) {
        set_error("soar_smplify_model_points: NULL input or output");
        return 1;
    }
    PointsArgs fa;
    fa.rig = r;
    fa.a = a;
    fa.pose_mean = mean_mask ? body->pose_mean : nullptr;
    fa.mean_mask = mean_mask;
    fa.mp_idx = mp_idx;
    fa.mp_w = mp_w;
    fa.out = points;
    fa.PA = PA;
    fa.PS3 = PS3;
    hipLaunchKernelGGL(smplify_points_kernel, dim3(a.N), dim3(S_THREADS), 0, stream, fa);
    SOAR_LAUNCH_OK("smplify_points", stream, 0);
    return 0;
}

extern "C" int soar_smplify_target_scales(int32_t N, const float *target_kps, float img_w, float img_h, float *scales, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (N < 0 || N > 0x7fffffff / (SKP * 3)) { set_error("soar_smplify_target_scales: N=%d out of range", N); return 1; }
    if (N == 0) return 0;
    if (!target_kps || !scales) { set_error("soar_smplify_target_scales: NULL argument"); return 1; }
    hipLaunchKernelGGL(target_scales_kernel, dim3(N), dim3(256), 0, stream, N, target_kps, img_w, img_h, scales);
    SOAR_LAUNCH_OK("smplify_target_scales", stream, 0);
    return 0;
}
