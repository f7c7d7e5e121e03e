// loss_finish.h -- the fixed-order sum of the frame loss's per-workgroup partials, shared by frame_loss_finish_kernel (frame_loss.hip)
// and the workgroups of geom_warp_backward_frames_kernel (lbs.hip) that take that launch's work over in the step plan.
#pragma once

#include "soar_common.h"

namespace soar {

// loss = wc*S[0]/(3n) + wm*S[1]/n + wn*S[2]/(3n) + wd*S[3]/n,  S = the workgroups' partial sums added in a fixed order (thread t
// takes workgroups t, t + 256, ...; then a fixed tree): no atomics, the value does not depend on who finished first.
// One workgroup of 256 threads; red: 256 float4 of LDS.
// WAVES: `sums` holds one partial per WAVEFRONT of the loss's grid, four per workgroup (the riders of the backward blend's launch,
// rast_render_bwd.hip, leave them): a workgroup's partial is formed first, (w0 + w1) + (w2 + w3) as frame_loss_kernel forms it.
template <bool WAVES = false>
__device__ __forceinline__ void loss_finish_sum(const float *sums, int blocks, int n, float wc, float wm, float wn, float wd, float *loss,
                                                float4 *red)
{
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b = threadIdx.x; b < blocks; b += 256) {
        float4 v;
        if (WAVES) {
            const float4 *w = reinterpret_cast<const float4 *>(sums) + 4 * (size_t)b;
            const float4 w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
            v = make_float4((w0.x + w1.x) + (w2.x + w3.x), (w0.y + w1.y) + (w2.y + w3.y), (w0.z + w1.z) + (w2.z + w3.z), (w0.w + w1.w) + (w2.w + w3.w));
        } else {
            v = reinterpret_cast<const float4 *>(sums)[b];
        }
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
