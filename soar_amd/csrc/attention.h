// attention.h -- multi-head attention with separate query, key and value sources and any number of keys (unet.hip, clip.hip).
//
//   kv_attn_kernel         out = softmax(q k^T scale) v  (+ w2 softmax(q k2^T scale) v2: a second key / value set in the same launch,
//                          the query read once).  An online softmax over tiles of 32 keys, both products on
//                          v_mfma_f32_32x32x2_f32, nothing of the score matrix in memory.  The last tile's missing keys are masked, not
//                          padded in memory; the head dimension is padded to 32, 64 or 96 in LDS only.  CAUSAL (clip.hip; one key
//                          set, Lq = Lk): key j counts for query i when j <= i -- masked inside a tile, and the key tiles wholly
//                          behind the workgroup's last query are not visited.  Key 0 is visible to every query, so a row's running
//                          maximum is finite from the first tile on and a tile without a visible key adds exp(-inf) = 0
// The scheme is sam_attn_kernel's (sam.hip): transposed products, a lane owns one query, p stays in its registers.
// No atomics; a (batch, head, query tile)'s sums do not depend on the rest of the launch.
#pragma once

#include "conv_gemm.h"

namespace soar {
namespace {

constexpr int KVA_Q = 128;             // queries per workgroup: four waves of 32
constexpr int KVA_K = 32;              // keys per tile

template <int HDP, bool CAUSAL>
__global__ void __launch_bounds__(256) kv_attn_kernel(SoarUnetAttnArgs a)
{
    constexpr int PITCH = HDP + 4, NC = HDP / 32;
    __shared__ float Ks[KVA_K][PITCH], Vs[KVA_K][PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int qi = blockIdx.x * KVA_Q + wave * 32 + i;           // this lane's query
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // the query, scaled, in the k order of the S^T product: chunk c, group g holds channels 32 c + 16 h + 4 g .. + 4
    float4 qreg[NC][4];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int d = c * 32 + h * 16 + 4 * g;
            float4 v = zero4;
            if (qi < a.Lq && d < a.hd) v = *reinterpret_cast<const float4 *>(a.q + ((size_t)b * a.Lq + qi) * a.ldq + head * a.hd + d);
            v.x *= a.scale; v.y *= a.scale; v.z *= a.scale; v.w *= a.scale;
            qreg[c][g] = v;
        }

    f32x16 total[NC];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int e = 0; e < 16; e++) total[c][e] = 0.f;

    // one key / value set: its normalised result times wgt is added to total
    auto run = [&](const float *kp, const float *vp, int64_t ldk, int64_t ldv, int nk, float wgt) {
        float m = -INFINITY, l = 0.f;
        f32x16 o[NC];
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int e = 0; e < 16; e++) o[c][e] = 0.f;
        int ntiles = (nk + KVA_K - 1) / KVA_K;
        if (CAUSAL) {                                            // the workgroup's last query sees keys 0 .. itself
            const int last = min(a.Lq, ((int)blockIdx.x + 1) * KVA_Q) - 1;
            ntiles = min(ntiles, last / KVA_K + 1);
        }
        for (int kt = 0; kt < ntiles; kt++) {
            // K and V of 32 keys, eight threads a key; rows past the last key and channels past hd are zeros
            {
                const int r = tid >> 3, j = kt * KVA_K + r;
                for (int f = tid & 7; f < HDP / 4; f += 8) {
                    const int d = f * 4;
                    float4 kk = zero4, vv = zero4;
                    if (j < nk && d < a.hd) {
                        kk = *reinterpret_cast<const float4 *>(kp + ((size_t)b * nk + j) * ldk + head * a.hd + d);
                        vv = *reinterpret_cast<const float4 *>(vp + ((size_t)b * nk + j) * ldv + head * a.hd + d);
                    }
                    *reinterpret_cast<float4 *>(&Ks[r][d]) = kk;
                    *reinterpret_cast<float4 *>(&Vs[r][d]) = vv;
                }
            }
            __syncthreads();
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; e++) s[e] = 0.f;
#pragma unroll
            for (int c = 0; c < NC; c++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const float4 k4 = *reinterpret_cast<const float4 *>(&Ks[i][c * 32 + h * 16 + 4 * g]);
#pragma unroll
                    for (int u = 0; u < 4; u++) s = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(k4, u), comp(qreg[c][g], u), s, 0, 0, 0);
                }
            float mx = -INFINITY;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int j = kt * KVA_K + mfma_row(e, h);
                s[e] = j < nk && (!CAUSAL || j <= qi) ? s[e] : -INFINITY;    // the tail of the last tile; the keys behind the query
                mx = fmaxf(mx, s[e]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            const float mn = fmaxf(m, mx);                       // finite: every tile has its first key, and a causal row has key 0
            const float corr = expf(m - mn);                     // (0 at the first tile)
            float sum = 0.f;
#pragma unroll
            for (int e = 0; e < 16; e++) { s[e] = expf(s[e] - mn); sum += s[e]; }
            sum += __shfl_xor(sum, 32);
            l = l * corr + sum;
            m = mn;
#pragma unroll
            for (int c = 0; c < NC; c++) {
#pragma unroll
                for (int e = 0; e < 16; e++) o[c][e] *= corr;
#pragma unroll
                for (int u = 0; u < 16; u++) o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[mfma_row(u, h)][c * 32 + i], s[u], o[c], 0, 0, 0);
            }
            __syncthreads();
        }
        const float inv = 1.f / l;
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int e = 0; e < 16; e++) total[c][e] += wgt * (o[c][e] * inv);
    };
    run(a.k, a.v, a.ldk, a.ldv, a.Lk, 1.f);
    if (a.k2) run(a.k2, a.v2, a.ldk2, a.ldv2, a.Lk2, a.w2);

    if (qi >= a.Lq) return;                                      // the tail of the last query tile
    float *dst = a.out + ((size_t)b * a.Lq + qi) * a.ldo + head * a.hd;
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int d = c * 32 + 8 * g + 4 * h;                // registers 4 g .. 4 g + 3: channels d .. d + 3
            if (d < a.hd) *reinterpret_cast<float4 *>(dst + d) = make_float4(total[c][4 * g], total[c][4 * g + 1], total[c][4 * g + 2], total[c][4 * g + 3]);
        }
}

// TOWER (clip.hip's calls): also the causal mask and head dimensions up to 96; the UNet's calls keep their two instantiations
template <bool TOWER = false>
int launch_kv_attention(const SoarUnetAttnArgs &a, hipStream_t stream, bool causal = false, const char *me = "unet attention")
{
    constexpr int hd_max = TOWER ? 96 : 64;
    const int64_t C = (int64_t)a.heads * a.hd;
    if (a.B < 0 || a.B > 65535 || a.Lq < 1 || a.Lk < 1 || a.heads < 1 || a.heads > 65535 || a.hd < 4 || a.hd > hd_max || a.hd % 4 ||
        (int64_t)a.B * a.Lq > (int64_t(1) << 30) || (int64_t)a.B * a.Lk > (int64_t(1) << 30)) {
        set_error("%s: bad sizes (B=%d <= 65535, Lq=%d, Lk=%d from 1, heads=%d, hd=%d: a multiple of 4 up to %d)", me, a.B, a.Lq, a.Lk, a.heads, a.hd, hd_max);
        return 1;
    }
    if (a.B == 0) return 0;
    if (!a.q || !a.k || !a.v || !a.out || (!a.k2 != !a.v2) || (a.k2 && (a.Lk2 < 1 || (int64_t)a.B * a.Lk2 > (int64_t(1) << 30)))) {
        set_error("%s: NULL q, k, v or out, or a second key set without its values or with Lk2 = %d below 1", me, a.Lk2);
        return 1;
    }
    const int64_t lds[6] = {a.ldq, a.ldk, a.ldv, a.ldo, a.k2 ? a.ldk2 : C, a.k2 ? a.ldv2 : C};
    for (int64_t ld : lds)
        if (ld < C || ld % 4) { set_error("%s: a row pitch of %lld floats: need a multiple of 4 from heads hd = %lld", me, (long long)ld, (long long)C); return 1; }
    if (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out | (uintptr_t)a.k2 | (uintptr_t)a.v2) & 15) {
        set_error("%s: pointers must be 16-byte aligned", me);
        return 1;
    }
    if (causal && (!TOWER || a.k2 || a.Lq != a.Lk)) { set_error("%s: a causal mask needs one key set and Lq = Lk (Lq=%d, Lk=%d)", me, a.Lq, a.Lk); return 1; }
    const dim3 grid((unsigned)((a.Lq + KVA_Q - 1) / KVA_Q), (unsigned)a.heads, (unsigned)a.B);
    if constexpr (TOWER) {
        if (causal) {
            if (a.hd <= 32) hipLaunchKernelGGL((kv_attn_kernel<32, true>), grid, dim3(256), 0, stream, a);
            else if (a.hd <= 64) hipLaunchKernelGGL((kv_attn_kernel<64, true>), grid, dim3(256), 0, stream, a);
            else hipLaunchKernelGGL((kv_attn_kernel<96, true>), grid, dim3(256), 0, stream, a);
            SOAR_LAUNCH_OK("kv_attn", stream, 0);
            return 0;
        }
        if (a.hd > 64) {
            hipLaunchKernelGGL((kv_attn_kernel<96, false>), grid, dim3(256), 0, stream, a);
            SOAR_LAUNCH_OK("kv_attn", stream, 0);
            return 0;
        }
    }
    if (a.hd <= 32) hipLaunchKernelGGL((kv_attn_kernel<32, false>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((kv_attn_kernel<64, false>), grid, dim3(256), 0, stream, a);
    SOAR_LAUNCH_OK("kv_attn", stream, 0);
    return 0;
}

}  // namespace
}  // namespace soar
