// soar_quat.h -- the candidate table of matrix_to_quaternion (public pytorch3d convention, real part first), shared by the
// skinning warp (lbs.hip) and the surfel frames of the avatar initialisation (body.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace soar {

// candidate table of matrix_to_quaternion: returns best index, fills cand[4] and a = q_abs[best]
__device__ __forceinline__ int mat_to_quat_candidates(const float m[9], float cand[4], float &a_best, float &x_best)
{
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    const float xs[4] = {1.0f + m00 + m11 + m22, 1.0f + m00 - m11 - m22, 1.0f - m00 + m11 - m22, 1.0f - m00 - m11 + m22};
    float qa[4];
    int best = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) qa[t] = xs[t] > 0.f ? sqrtf(xs[t]) : 0.f;
#pragma unroll
    for (int t = 1; t < 4; t++)
        if (qa[t] > qa[best]) best = t;
    a_best = qa[best];
    x_best = xs[best];
    const float sq = a_best * a_best;
    if (best == 0) { cand[0] = sq; cand[1] = m21 - m12; cand[2] = m02 - m20; cand[3] = m10 - m01; }
    else if (best == 1) { cand[0] = m21 - m12; cand[1] = sq; cand[2] = m10 + m01; cand[3] = m02 + m20; }
    else if (best == 2) { cand[0] = m02 - m20; cand[1] = m10 + m01; cand[2] = sq; cand[3] = m12 + m21; }
    else { cand[0] = m10 - m01; cand[1] = m20 + m02; cand[2] = m21 + m12; cand[3] = sq; }
    return best;
}

}  // namespace soar
