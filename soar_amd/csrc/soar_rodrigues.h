// soar_rodrigues.h -- batch_rodrigues of the vendored body model (TS/utils/smplx/lbs.py:293-327), shared by the joint chain
// (smplx_joints.hip) and the vertex forward (body.hip): both must see the same rotation of the same axis-angle vector.
#pragma once

#include <hip/hip_runtime.h>

namespace soar {

// v: axis-angle [3] -> R row-major 3x3 with ROW floats per row (R[r * ROW + c]).  angle = |v + 1e-8|, K = skew(v / angle), R = I + sin K + (1 - cos) K K
template <int ROW>
__device__ __forceinline__ void rodrigues(const float *v, float *R)
{
    const float vx = v[0], vy = v[1], vz = v[2];
    const float ex = vx + 1e-8f, ey = vy + 1e-8f, ez = vz + 1e-8f;
    const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
    const float rx = vx / angle, ry = vy / angle, rz = vz / angle;
    const float sn = sinf(angle), cs = 1.f - cosf(angle);
    const float K[9] = {0.f, -rz, ry, rz, 0.f, -rx, -ry, rx, 0.f};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            float kk = 0.f;
            for (int m = 0; m < 3; m++) kk += K[r * 3 + m] * K[m * 3 + c];
            R[r * ROW + c] = (r == c ? 1.f : 0.f) + sn * K[r * 3 + c] + cs * kk;
        }
}

}  // namespace soar
