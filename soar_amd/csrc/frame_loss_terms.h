// frame_loss_terms.h -- the per-pixel arithmetic of the frame loss (frame_loss.hip), shared with the backward blend's form that makes
// its own upstream gradients and carries the value pass as riders of its launch (rast_render_bwd.hip: soar_rast_backward_plan_loss).
// Both compile THIS source: the gradients the blend computes in its pixel prologue and the partial sums its riders leave are the
// bits frame_loss_kernel writes.
#pragma once

#include "soar_common.h"

#include <type_traits>

namespace soar {

struct LossArgs {
    int n;                       // pixels
    const float *color, *normal, *depth, *opac;            // [3,n] [3,n] [n] [n]
    const float *t_color, *t_mask, *t_normal;              // [3,n] [n] [3,n]
    float wc, wm, wn, wd;
    float *dcolor, *dnormal, *ddepth, *dopac;
    float *sums;                 // [gridDim.x][4] per-workgroup un-normalised sums of the four terms (riders: [4 gridDim.x][4], per wavefront)
    const int *set_index;        // optional: the targets are set (*set_index mod n_sets) of a resident pool [n_sets][7][n]
    int n_sets;
    const float *bg;             // optional [3] (with n_contrib): background colour of the forward blend that wrote the images --
                                 // pixels nothing contributed to are not read, their values are the blend's background constants
    int normalize_depth;
    const uint32_t *n_contrib;   // optional [n]: the forward blend's contributor count; gradients of pixels nothing contributed to
                                 // are never read by the backward blend (its walk starts at n_contrib) and are not written
    const uint32_t *bg_tiles;    // optional (with n_contrib; ImageBuf::bg_tiles): 1 = the 16x16 tile had no list, all its counts are 0 --
    int W, gx;                   // its 1 KB of counts is not read either (80 % of the tiles of a frame of one person)
};

// the grid of frame_loss_kernel<V> for these arguments: V = 4 when every plane allows 16-byte accesses (a plane that is not given does
// not object), one thread per group of V pixels up to the scratch's SOAR_FRAME_LOSS_SCRATCH_FLOATS / 4 workgroups, a stride walk beyond.
// The backward blend's riders (rast_render_bwd.hip) take the wavefronts of exactly this grid.
inline void frame_loss_grid(const LossArgs &a, bool &vec4, int &blocks)
{
    vec4 = (a.n & 3) == 0 && (((uintptr_t)a.n_contrib | (uintptr_t)a.color | (uintptr_t)a.normal | (uintptr_t)a.depth | (uintptr_t)a.opac | (uintptr_t)a.t_color |
                               (uintptr_t)a.t_mask | (uintptr_t)a.t_normal | (uintptr_t)a.dcolor | (uintptr_t)a.dnormal |
                               (uintptr_t)a.ddepth | (uintptr_t)a.dopac) & 15) == 0;
    blocks = min(SOAR_FRAME_LOSS_SCRATCH_FLOATS / 4, max(1, (a.n / (vec4 ? 4 : 1) + 255) / 256));
}

__device__ __forceinline__ float sign_of(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// frame data resident in HBM: pick this frame's planes (colour 3, mask 1, normal 3)
__device__ __forceinline__ void loss_pick_target_set(LossArgs &a)
{
    if (a.set_index) {
        const float *set = a.t_color + (size_t)((unsigned)*a.set_index % (unsigned)a.n_sets) * 7u * (size_t)a.n;
        a.t_color = set; a.t_mask = set + 3 * (size_t)a.n; a.t_normal = set + 4 * (size_t)a.n;
    }
}

// the factors of the four terms' pixel gradients: d|c - t| = gc sign(c - t), d|o - m| = gm sign(o - m), d(n . n_t) = gn n_t, d depth = gd
struct LossScales { float gc, gm, gn, gd; };
__device__ __forceinline__ LossScales loss_scales(const LossArgs &a)
{
    LossScales s;
    s.gc = a.wc / (3.f * a.n); s.gm = a.wm / a.n; s.gn = a.wn / (3.f * a.n); s.gd = a.wd / a.n;
    return s;
}

// one element's gradient of an L1 term (d = value - target) / of a dot-product term (t = the target's component): ONE rounded product
// each -- the walk below and the backward blend's pixel prologue (rast_render_bwd.hip) both call these
__device__ __forceinline__ float loss_grad_l1(float k, float d) { return k * sign_of(d); }
__device__ __forceinline__ float loss_grad_dot(float k, float t) { return k * t; }

// V = 4: float4 accesses (planes of a [3,n] tensor are 16-byte aligned only when n % 4 == 0); V = 1: any image size
template <int V> struct Vec;
template <> struct Vec<4> { typedef float4 type; };
template <> struct Vec<1> { typedef float type; };
__device__ __forceinline__ float4 ld(const float4 *p, int i) { return p[i]; }
__device__ __forceinline__ float4 ld(const float *p, int i) { return make_float4(p[i], 0.f, 0.f, 0.f); }
__device__ __forceinline__ void st(float4 *p, int i, float4 v) { p[i] = v; }
__device__ __forceinline__ void st(float *p, int i, float4 v) { p[i] = v.x; }
__device__ __forceinline__ bool any_contrib(const uint4 *p, int i) { const uint4 v = p[i]; return (v.x | v.y | v.z | v.w) != 0u; }
__device__ __forceinline__ bool any_contrib(const uint32_t *p, int i) { return p[i] != 0u; }

// One thread's walk over the groups of V pixels first, first + stride, ...: its sums of the four terms and, with GRADS, the
// gradient planes of the groups somebody will read.  `a`: the target set already picked.
template <int V, bool GRADS>
__device__ __forceinline__ void frame_loss_walk(const LossArgs &a, int first, int stride, float &s_c, float &s_m, float &s_n, float &s_d)
{
    typedef typename Vec<V>::type T;
    const int nv = a.n / V;
    const LossScales g = loss_scales(a);
    const float gc = g.gc, gm = g.gm, gn = g.gn, gd = g.gd;
    const float4 pad = V == 4 ? make_float4(1.f, 1.f, 1.f, 1.f) : make_float4(1.f, 0.f, 0.f, 0.f);   // lanes that exist
    typedef typename std::conditional<V == 4, uint4, uint32_t>::type U;
    // what the blend writes where nothing contributed (T = 1; forward.cu:618-633, the same expressions as its epilogue)
    const float Tc = (float)(1 - 0.000001);
    const bool known = a.n_contrib && a.bg;
    float bgc[3] = {0.f, 0.f, 0.f};
    if (known) { bgc[0] = 0.f + Tc * a.bg[0]; bgc[1] = 0.f + Tc * a.bg[1]; bgc[2] = 0.f + Tc * a.bg[2]; }
    const float bg_depth = a.normalize_depth ? 0.f / (1.f - Tc) : 0.f + Tc * 10.f, bg_opac = 1.f - Tc;
    for (int i = first; i < nv; i += stride) {
        bool wr = true;                                                                                // someone will read the gradients
        if (a.n_contrib) {
            bool empty_tile = false;
            if (a.bg_tiles) {
                const int p = i * V, y = p / a.W, x = p - y * a.W;
                empty_tile = a.bg_tiles[(y >> 4) * a.gx + (x >> 4)] != 0u;
            }
            wr = !empty_tile && any_contrib(reinterpret_cast<const U *>(a.n_contrib), i);
        }
        const bool rd = wr || !known;                                                                  // the images have to be read
        float4 nsum = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float4 c = rd ? ld(reinterpret_cast<const T *>(a.color + (size_t)ch * a.n), i) : make_float4(bgc[ch], bgc[ch], bgc[ch], bgc[ch]);
            const float4 t = ld(reinterpret_cast<const T *>(a.t_color + (size_t)ch * a.n), i);
            const float4 d = make_float4(c.x - t.x, c.y - t.y, c.z - t.z, c.w - t.w);
            s_c += (fabsf(d.x) + fabsf(d.y)) + (fabsf(d.z) + fabsf(d.w));
            if (GRADS && wr) st(reinterpret_cast<T *>(a.dcolor + (size_t)ch * a.n), i,
                                make_float4(loss_grad_l1(gc, d.x), loss_grad_l1(gc, d.y), loss_grad_l1(gc, d.z), loss_grad_l1(gc, d.w)));
            const float4 nr = rd ? ld(reinterpret_cast<const T *>(a.normal + (size_t)ch * a.n), i) : make_float4(0.f, 0.f, 0.f, 0.f);
            // (where nothing was rendered the normal image is exactly 0: its product with the target adds +-0 to the sum whatever the
            // (finite) target is -- the target's 12 bytes per pixel of the 85 % background of a frame are not read: 25 of the launch's
            // 86 MB per 1080p frame)
            const float4 nt = rd ? ld(reinterpret_cast<const T *>(a.t_normal + (size_t)ch * a.n), i) : make_float4(0.f, 0.f, 0.f, 0.f);
            nsum.x += nr.x * nt.x; nsum.y += nr.y * nt.y; nsum.z += nr.z * nt.z; nsum.w += nr.w * nt.w;
            if (GRADS && wr) st(reinterpret_cast<T *>(a.dnormal + (size_t)ch * a.n), i, make_float4(loss_grad_dot(gn, nt.x), loss_grad_dot(gn, nt.y), loss_grad_dot(gn, nt.z), loss_grad_dot(gn, nt.w)));
        }
        s_n += (nsum.x + nsum.y) + (nsum.z + nsum.w);
        const float4 o = rd ? ld(reinterpret_cast<const T *>(a.opac), i) : make_float4(bg_opac, bg_opac, bg_opac, bg_opac);
        const float4 m = ld(reinterpret_cast<const T *>(a.t_mask), i);
        const float4 e = make_float4(o.x - m.x, o.y - m.y, o.z - m.z, o.w - m.w);
        s_m += (fabsf(e.x) + fabsf(e.y)) + (fabsf(e.z) + fabsf(e.w));
        if (GRADS && wr) st(reinterpret_cast<T *>(a.dopac), i, make_float4(loss_grad_l1(gm, e.x), loss_grad_l1(gm, e.y), loss_grad_l1(gm, e.z), loss_grad_l1(gm, e.w)));
        const float4 dp = rd ? ld(reinterpret_cast<const T *>(a.depth), i) : make_float4(bg_depth, bg_depth, bg_depth, bg_depth);
        s_d += (dp.x + dp.y) + (dp.z + dp.w);
        if (GRADS && wr) st(reinterpret_cast<T *>(a.ddepth), i, make_float4(loss_grad_dot(gd, pad.x), loss_grad_dot(gd, pad.y), loss_grad_dot(gd, pad.z), loss_grad_dot(gd, pad.w)));
    }
}

}  // namespace soar
