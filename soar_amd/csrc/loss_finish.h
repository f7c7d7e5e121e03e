// loss_finish.h -- the fixed-order sum of the frame loss's per-workgroup partials, shared by frame_loss_finish_kernel (frame_loss.hip)
// and the workgroups of geom_warp_backward_frames_kernel (lbs.hip) that take that launch's work over in the step plan.
#pragma once

#include "soar_common.h"

namespace soar {

// loss = wc*S[0]/(3n) + wm*S[1]/n + wn*S[2]/(3n) + wd*S[3]/n,  S = the workgroups' partial sums added in a fixed order (thread t
// takes workgroups t, t + 256, ...; then a fixed tree): no atomics, the value does not depend on who finished first.
// One workgroup of 256 threads; red: 256 float4 of LDS.
__device__ __forceinline__ void loss_finish_sum(const float *sums, int blocks, int n, float wc, float wm, float wn, float wd, float *loss,
                                                float4 *red)
{
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = threadIdx.x; b < blocks; b += 256) {
        const float4 v = reinterpret_cast<const float4 *>(sums)[b];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const float4 o = red[threadIdx.x + off];
            float4 m = red[threadIdx.x];
            m.x += o.x; m.y += o.y; m.z += o.z; m.w += o.w;
            red[threadIdx.x] = m;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float4 S = red[0];
        *loss = (wc * S.x / (3.f * n) + wm * S.y / n) + (wn * S.z / (3.f * n) + wd * S.w / n);
    }
}

}  // namespace soar
