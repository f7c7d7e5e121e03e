// mesh_texture.hip -- the texture atlas of the exported mesh (soar_amd/texture.py: build_atlas, bake_texture): MeshLab's "trivial
// per-triangle parametrization" and "transfer vertex attributes to texture" on the device.  DESIGN.md 9b, "Texture atlas" states the
// layout and why cells are disjoint and bilinear taps stay inside their face; tests/texture_ref.py restates every rule in NumPy.
//
//   atlas_levels_kernel    one lane per face: float32 area (every operation rounded as written: the file is built with
//                          -ffp-contract=off, the square root is sqrtf, correctly rounded under the build's flags), level = the number of ladder
//                          thresholds <= area by binary search (no logarithm), -1 for an area that is not a positive finite
//                          number; a histogram of the levels through LDS (integer atomics: the counts do not depend on their order).
//   atlas_classes_kernel   one lane: from the histogram and the step j the host picked, the faces and cells of every side
//                          s = 2^L, where each size starts in the order and on the Morton curve, and whether all of it fits.
//   atlas_keys_kernel      key = 15 - L per face; a STABLE radix sort of (key, face) is the order "decreasing s, then face index".
//   atlas_place_kernel     one lane per place in that order: rank in its size -> cell and half, the cell's first Morton unit -> x0, y0;
//                          writes cell, the three uv corners and the uv_faces row of its face.
//   texel_counts_kernel    one lane per face: checks the cell (inside the image, aligned to its side) and the corners, counts the
//                          texels the face owns; an exclusive scan gives every face its range of the texel enumeration.
//   texels_kernel          one lane per owned texel t of a chunk: its face by binary search in the scan, (a, b) from the place
//                          inside the face (rows b and s-1-b of a lower half have s+1 texels together), barycentrics from the
//                          integers, the 3-D point, the image address.  A point that is not finite is flagged (address ~addr)
//                          and queried at the origin: the grid search has no neighbour for it and the colour transfer refuses.
//   texture_write_kernel   bytes = floor(255 c + 0.5) at the chunk's addresses, zero for a flagged texel.
//
// Integer arithmetic decides every position; no float atomics: two runs give the same bytes.
#include "mesh_common.h"

namespace soar {

namespace {

constexpr int32_t TEX_MAX_F = 1 << 28;
constexpr int32_t TEX_MAX_V = 1 << 30;
constexpr int TEX_MIN_T = 16, TEX_MAX_T = 16384;
constexpr int TEX_MAX_LADDER = 1024;
constexpr int TEX_HIST = TEX_MAX_LADDER + 2;      // levels 0 .. n_ladder, then the degenerate faces at n_ladder + 1
constexpr int TEX_CLASSES = 16;                   // L = log2 s, 2 .. 13

struct AtlasClasses {
    uint32_t n[TEX_CLASSES];        // faces of side 2^L
    uint32_t off[TEX_CLASSES];      // where they start in the order
    uint64_t base[TEX_CLASSES];     // their first Morton unit
    uint64_t units;                 // units used by all cells
    uint32_t fits;
};

struct AtlasBuf {
    int32_t *level;                 // [F]
    uint32_t *keys, *keys_sorted, *vals, *vals_sorted;   // [F] each
    uint32_t *hist;                 // [TEX_HIST]
    AtlasClasses *classes;
    uint32_t *bad;
    void *sort_temp;
    size_t sort_bytes;
};

size_t carve_atlas(AtlasBuf &b, void *base, size_t F)
{
    const size_t N = F > 0 ? F : 1;
    Carver c(base);
    b.level = c.take<int32_t>(N);
    b.keys = c.take<uint32_t>(N);
    b.keys_sorted = c.take<uint32_t>(N);
    b.vals = c.take<uint32_t>(N);
    b.vals_sorted = c.take<uint32_t>(N);
    b.hist = c.take<uint32_t>(TEX_HIST);
    b.classes = c.take<AtlasClasses>(1);
    b.bad = c.take<uint32_t>(1);
    b.sort_bytes = sort_pairs_temp_bytes<uint32_t, uint32_t>(N, 4u);
    b.sort_temp = c.take<char>(b.sort_bytes);
    return c.bytes();
}

__global__ void __launch_bounds__(256) atlas_levels_kernel(int V, int F, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                           const float *__restrict__ ladder, int n_ladder, int32_t *__restrict__ level,
                                                           uint32_t *__restrict__ hist, uint32_t *__restrict__ bad)
{
    __shared__ uint32_t local[TEX_HIST];
    for (int i = threadIdx.x; i < n_ladder + 2; i += 256) local[i] = 0u;
    __syncthreads();
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < F) {
        const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
        int e = -1;
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
            atomicAdd(bad, 1u);                       // reported by the host; nothing is read through the index
        } else {
            const float *p0 = verts + (size_t)i0 * 3, *p1 = verts + (size_t)i1 * 3, *p2 = verts + (size_t)i2 * 3;
            const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
            const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
            const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const float n2 = (cx * cx + cy * cy) + cz * cz;
            // sqrtf, not __fsqrt_rn: under -fhip-fp32-correctly-rounded-divide-sqrt (build.py) sqrtf is the hardware square root plus
            // its correction step, correctly rounded like numpy's; __fsqrt_rn is the bare 1-ulp instruction in this toolchain
            const float area = 0.5f * sqrtf(n2);
            if (area > 0.f && area <= 3.402823466e38f) {
                int lo = 0, hi = n_ladder;            // the number of thresholds <= area
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (ladder[mid] <= area) lo = mid + 1;
                    else hi = mid;
                }
                e = lo;
            }
        }
        level[f] = e;
        atomicAdd(&local[e < 0 ? n_ladder + 1 : e], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n_ladder + 2; i += 256)
        if (local[i]) atomicAdd(&hist[i], local[i]);
}

// log2 of the side of a face of level e at step j in a T x T image (top = log2(T / 2))
__device__ __forceinline__ int side_log2(int e, int j, int top)
{
    if (e < 0) return 2;
    const int t = e + j;
    const int q = t >= 0 ? t / 8 : -((-t + 7) / 8);   // floor
    return q < 2 ? 2 : (q > top ? top : q);
}

__global__ void atlas_classes_kernel(int n_ladder, int j, int T, const uint32_t *__restrict__ hist, AtlasClasses *__restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int top = 30 - __clz(T);                    // log2(T) - 1
    AtlasClasses c;
    for (int L = 0; L < TEX_CLASSES; L++) { c.n[L] = 0u; c.off[L] = 0u; c.base[L] = 0ull; }
    for (int e = 0; e <= n_ladder; e++) c.n[side_log2(e, j, top)] += hist[e];
    c.n[2] += hist[n_ladder + 1];
    uint32_t off = 0u;
    uint64_t base = 0ull;
    for (int L = TEX_CLASSES - 1; L >= 2; L--) {      // decreasing side
        c.off[L] = off;
        c.base[L] = base;
        off += c.n[L];
        base += (uint64_t)((c.n[L] + 1u) >> 1) << (2 * (L - 2));
    }
    c.units = base;
    c.fits = base <= ((uint64_t)(T / 4) * (uint64_t)(T / 4)) ? 1u : 0u;
    *out = c;
}

__global__ void __launch_bounds__(256) atlas_keys_kernel(int F, int j, int T, const int32_t *__restrict__ level, uint32_t *__restrict__ keys,
                                                         uint32_t *__restrict__ vals)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    keys[f] = (uint32_t)(15 - side_log2(level[f], j, 30 - __clz(T)));
    vals[f] = (uint32_t)f;
}

__device__ __forceinline__ uint32_t even_bits(uint64_t u)
{
    u &= 0x5555555555555555ull;
    u = (u | (u >> 1)) & 0x3333333333333333ull;
    u = (u | (u >> 2)) & 0x0f0f0f0f0f0f0f0full;
    u = (u | (u >> 4)) & 0x00ff00ff00ff00ffull;
    u = (u | (u >> 8)) & 0x0000ffff0000ffffull;
    u = (u | (u >> 16)) & 0x00000000ffffffffull;
    return (uint32_t)u;
}

// the local texel (a, b) of corner k of a half (m = s - 3)
__device__ __forceinline__ void corner_texel(int s, int half, int k, int &a, int &b)
{
    const int m = s - 3;
    a = k == 1 ? m : 0;
    b = k == 2 ? m : 0;
    if (half) { a = s - 1 - a; b = s - 1 - b; }
}

__global__ void __launch_bounds__(256) atlas_place_kernel(int F, int T, const uint32_t *__restrict__ keys_sorted,
                                                          const uint32_t *__restrict__ vals_sorted, const AtlasClasses *__restrict__ classes,
                                                          float *__restrict__ uv, int32_t *__restrict__ uv_faces, int32_t *__restrict__ cell)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= F) return;
    const uint32_t f = vals_sorted[p];
    int L = 15 - (int)keys_sorted[p];
    if (f >= (uint32_t)F || L < 2 || L >= TEX_CLASSES) return;       // (cannot happen: the keys and values are this file's)
    const uint32_t r = (uint32_t)p - classes->off[L];
    const uint64_t u0 = classes->base[L] + ((uint64_t)(r >> 1) << (2 * (L - 2)));
    const int s = 1 << L, half = (int)(r & 1u);
    const int x0 = 4 * (int)even_bits(u0), y0 = 4 * (int)even_bits(u0 >> 1);
    int32_t *c = cell + (size_t)f * 4;
    c[0] = x0; c[1] = y0; c[2] = s; c[3] = half;
    const float den = (float)(2 * T);
    for (int k = 0; k < 3; k++) {
        int a, b;
        corner_texel(s, half, k, a, b);
        uv[((size_t)f * 3 + k) * 2] = (float)(2 * (x0 + a) + 1) / den;
        uv[((size_t)f * 3 + k) * 2 + 1] = (float)(2 * T - 2 * (y0 + b) - 1) / den;
        uv_faces[(size_t)f * 3 + k] = (int32_t)(f * 3u + (uint32_t)k);
    }
}

// ---- baking ------------------------------------------------------------------------------------------------------------------

struct TexelBuf {
    uint64_t *counts, *offsets;     // [F + 1] each
    uint32_t *bad;                  // [0] cells refused, [1] faces naming a vertex outside [0, V)
    void *scan_temp;
    size_t scan_bytes;
};

size_t carve_texels(TexelBuf &b, void *base, size_t F)
{
    Carver c(base);
    b.counts = c.take<uint64_t>(F + 1);
    b.offsets = c.take<uint64_t>(F + 1);
    b.bad = c.take<uint32_t>(2);
    b.scan_bytes = scan_temp_bytes<uint64_t>(F + 1);
    b.scan_temp = c.take<char>(b.scan_bytes);
    return c.bytes();
}

__device__ __forceinline__ bool cell_ok(int x0, int y0, int s, int half, int T)
{
    return s >= 4 && s <= T / 2 && (s & (s - 1)) == 0 && x0 >= 0 && y0 >= 0 && x0 <= T - s && y0 <= T - s && (x0 & (s - 1)) == 0 &&
           (y0 & (s - 1)) == 0 && (half == 0 || half == 1);
}

__global__ void __launch_bounds__(256) texel_counts_kernel(int V, int F, int T, const int32_t *__restrict__ faces, const int32_t *__restrict__ cell,
                                                           uint64_t *__restrict__ counts, uint32_t *__restrict__ bad)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f > F) return;
    if (f == F) { counts[f] = 0ull; return; }
    const int32_t *c = cell + (size_t)f * 4;
    const int s = c[2], half = c[3];
    uint64_t n = 0ull;
    if (!cell_ok(c[0], c[1], s, half, T)) atomicAdd(bad, 1u);
    else n = half ? (uint64_t)s * (uint64_t)(s - 1) / 2 : (uint64_t)s * (uint64_t)(s + 1) / 2;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) { atomicAdd(bad + 1, 1u); n = 0ull; }
    counts[f] = n;
}

__global__ void __launch_bounds__(256) texels_kernel(int V, int F, int T, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                     const int32_t *__restrict__ cell, const uint64_t *__restrict__ offsets, uint64_t t0, int n,
                                                     float *__restrict__ pos_out, int32_t *__restrict__ addr_out, int32_t *__restrict__ owner_img,
                                                     float *__restrict__ bary_img, float *__restrict__ position_img)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t t = t0 + (uint64_t)i;
    int lo = 0, hi = F;                               // the last face whose range starts at or before t: offsets[f] <= t < offsets[f + 1]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= t) lo = mid;
        else hi = mid;
    }
    const int f = lo;
    const int32_t *c = cell + (size_t)f * 4;
    const int x0 = c[0], y0 = c[1], s = c[2], half = c[3];
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    const bool ok = t >= offsets[f] && t < offsets[f + 1] && cell_ok(x0, y0, s, half, T) && i0 >= 0 && i0 < V && i1 >= 0 && i1 < V &&
                    i2 >= 0 && i2 < V;
    if (!ok) {                                        // (the host refused before this launch; nothing is written through a bad cell)
        pos_out[(size_t)i * 3] = 0.f; pos_out[(size_t)i * 3 + 1] = 0.f; pos_out[(size_t)i * 3 + 2] = 0.f;
        addr_out[i] = INT32_MIN;                      // ~INT32_MAX: beyond every image, the write kernel skips it
        return;
    }
    // (la, lb): the texel in the half's own frame, where the half is the lower one of a square of side w with la + lb <= w - 1
    const int q = (int)(t - offsets[f]);
    const int w = half ? s - 1 : s;                   // rows lb and w - 1 - lb have w + 1 texels together
    const int pr = q / (w + 1), rem = q % (w + 1);
    int la, lb;
    if (rem < w - pr) { la = rem; lb = pr; }
    else { la = rem - (w - pr); lb = w - 1 - pr; }
    const int a = half ? s - 1 - la : la, b = half ? s - 1 - lb : lb;
    const float m = (float)(s - 3);
    const float b1 = (float)la / m, b2 = (float)lb / m;
    float w0 = (1.f - b1) - b2, w1 = b1, w2 = b2;
    if (w0 < 0.f || w1 < 0.f || w2 < 0.f) {
        w0 = w0 < 0.f ? 0.f : w0;
        w1 = w1 < 0.f ? 0.f : w1;
        w2 = w2 < 0.f ? 0.f : w2;
        const float tot = (w0 + w1) + w2;
        w0 = w0 / tot; w1 = w1 / tot; w2 = w2 / tot;
    }
    const float *p0 = verts + (size_t)i0 * 3, *p1 = verts + (size_t)i1 * 3, *p2 = verts + (size_t)i2 * 3;
    const float x = (w0 * p0[0] + w1 * p1[0]) + w2 * p2[0];
    const float y = (w0 * p0[1] + w1 * p1[1]) + w2 * p2[1];
    const float z = (w0 * p0[2] + w1 * p1[2]) + w2 * p2[2];
    const bool finite = (x - x == 0.f) && (y - y == 0.f) && (z - z == 0.f);
    const int addr = (y0 + b) * T + (x0 + a);
    pos_out[(size_t)i * 3] = finite ? x : 0.f;
    pos_out[(size_t)i * 3 + 1] = finite ? y : 0.f;
    pos_out[(size_t)i * 3 + 2] = finite ? z : 0.f;
    addr_out[i] = finite ? addr : ~addr;
    if (owner_img) owner_img[addr] = f;
    if (bary_img) { bary_img[(size_t)addr * 3] = w0; bary_img[(size_t)addr * 3 + 1] = w1; bary_img[(size_t)addr * 3 + 2] = w2; }
    if (position_img) { position_img[(size_t)addr * 3] = x; position_img[(size_t)addr * 3 + 1] = y; position_img[(size_t)addr * 3 + 2] = z; }
}

__global__ void __launch_bounds__(256) texture_write_kernel(int n, int T, const int32_t *__restrict__ addr, const float *__restrict__ color,
                                                            uint8_t *__restrict__ texture, float *__restrict__ color_img)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int a = addr[i];
    const bool flagged = a < 0;
    if (flagged) a = ~a;
    if (a < 0 || a >= T * T) return;
    for (int k = 0; k < 3; k++) {
        const float c = flagged ? 0.f : fminf(fmaxf(color[(size_t)i * 3 + k], 0.f), 1.f);
        texture[(size_t)a * 3 + k] = (uint8_t)floorf(255.f * c + 0.5f);
        if (color_img) color_img[(size_t)a * 3 + k] = c;
    }
}

bool size_ok(const char *what, int32_t T)
{
    if (T < TEX_MIN_T || T > TEX_MAX_T || (T & (T - 1))) {
        set_error("%s: texture_size must be a power of two in [%d, %d] (texture_size=%d)", what, TEX_MIN_T, TEX_MAX_T, T);
        return false;
    }
    return true;
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_mesh_atlas_bytes(int32_t F, size_t *bytes)
{
    if (!bytes || F < 1 || F > TEX_MAX_F) { set_error("soar_mesh_atlas_bytes: need 1 <= F <= 2^28 and a result pointer (F=%d)", F); return 1; }
    AtlasBuf b;
    *bytes = carve_atlas(b, nullptr, (size_t)F);
    return 0;
}

extern "C" int soar_mesh_atlas_levels(int32_t V, int32_t F, const float *verts, const int32_t *faces, const float *ladder, int32_t n_ladder,
                                      void *workspace, size_t workspace_bytes, int64_t *hist_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (V < 1 || V > TEX_MAX_V || F < 1 || F > TEX_MAX_F) {
        set_error("soar_mesh_atlas_levels: need 1 <= V <= 2^30 and 1 <= F <= 2^28 (V=%d, F=%d)", V, F);
        return 1;
    }
    if (n_ladder < 1 || n_ladder > TEX_MAX_LADDER) { set_error("soar_mesh_atlas_levels: need 1 <= n_ladder <= %d (n_ladder=%d)", TEX_MAX_LADDER, n_ladder); return 1; }
    if (!verts || !faces || !ladder || !hist_host) { set_error("soar_mesh_atlas_levels: NULL argument"); return 1; }
    AtlasBuf b;
    if (!workspace_ok("soar_mesh_atlas_levels", workspace, workspace_bytes, carve_atlas(b, workspace, (size_t)F), "soar_mesh_atlas_bytes")) return 1;
    SOAR_HIP_OK(hipMemsetAsync(b.hist, 0, TEX_HIST * 4, stream));
    SOAR_HIP_OK(hipMemsetAsync(b.bad, 0, 4, stream));
    hipLaunchKernelGGL(atlas_levels_kernel, dim3((F + 255) / 256), dim3(256), 0, stream, V, F, verts, faces, ladder, n_ladder, b.level, b.hist, b.bad);
    SOAR_LAUNCH_OK("mesh_atlas_levels", stream, 0);
    static thread_local uint32_t host[TEX_HIST];
    uint32_t nbad = 0;
    SOAR_HIP_OK(hipMemcpyAsync(host, b.hist, (size_t)(n_ladder + 2) * 4, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipMemcpyAsync(&nbad, b.bad, 4, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    if (nbad) { set_error("soar_mesh_atlas_levels: %u faces name a vertex outside [0, %d)", nbad, V); return 1; }
    for (int i = 0; i < n_ladder + 2; i++) hist_host[i] = host[i];
    return 0;
}

extern "C" int soar_mesh_atlas_place(int32_t F, int32_t texture_size, int32_t n_ladder, int32_t scale_step, void *workspace,
                                     size_t workspace_bytes, float *uv_out, int32_t *uv_faces_out, int32_t *cell_out, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (F < 1 || F > TEX_MAX_F) { set_error("soar_mesh_atlas_place: need 1 <= F <= 2^28 (F=%d)", F); return 1; }
    if (!size_ok("soar_mesh_atlas_place", texture_size)) return 1;
    if (n_ladder < 1 || n_ladder > TEX_MAX_LADDER || scale_step < -2 * TEX_MAX_LADDER || scale_step > 2 * TEX_MAX_LADDER) {
        set_error("soar_mesh_atlas_place: need 1 <= n_ladder <= %d and |scale_step| <= %d (n_ladder=%d, scale_step=%d)", TEX_MAX_LADDER,
                  2 * TEX_MAX_LADDER, n_ladder, scale_step);
        return 1;
    }
    if (!uv_out || !uv_faces_out || !cell_out) { set_error("soar_mesh_atlas_place: NULL argument"); return 1; }
    AtlasBuf b;
    if (!workspace_ok("soar_mesh_atlas_place", workspace, workspace_bytes, carve_atlas(b, workspace, (size_t)F), "soar_mesh_atlas_bytes")) return 1;
    const dim3 gf((F + 255) / 256), blk(256);
    hipLaunchKernelGGL(atlas_classes_kernel, dim3(1), dim3(64), 0, stream, n_ladder, scale_step, texture_size, b.hist, b.classes);
    SOAR_LAUNCH_OK("mesh_atlas_classes", stream, 0);
    // refused before anything is placed: cells that do not fit would lie outside the image
    AtlasClasses host;
    SOAR_HIP_OK(hipMemcpyAsync(&host, b.classes, sizeof(host), hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    uint64_t total = 0;
    for (int L = 0; L < TEX_CLASSES; L++) total += host.n[L];
    if (total != (uint64_t)F) { set_error("soar_mesh_atlas_place: the workspace holds the levels of %llu faces, not of %d (call soar_mesh_atlas_levels first)", (unsigned long long)total, F); return 1; }
    if (!host.fits) {
        set_error("soar_mesh_atlas_place: scale_step=%d needs %llu units of 4 x 4 texels, texture_size=%d has %d", scale_step,
                  (unsigned long long)host.units, texture_size, (texture_size / 4) * (texture_size / 4));
        return 1;
    }
    hipLaunchKernelGGL(atlas_keys_kernel, gf, blk, 0, stream, F, scale_step, texture_size, b.level, b.keys, b.vals);
    SOAR_LAUNCH_OK("mesh_atlas_keys", stream, 0);
    SOAR_HIP_OK(sort_pairs(b.sort_temp, b.sort_bytes, b.keys, b.keys_sorted, b.vals, b.vals_sorted, (size_t)F, 4u, stream));
    hipLaunchKernelGGL(atlas_place_kernel, gf, blk, 0, stream, F, texture_size, b.keys_sorted, b.vals_sorted, b.classes, uv_out, uv_faces_out, cell_out);
    SOAR_LAUNCH_OK("mesh_atlas_place", stream, 0);
    return 0;
}

extern "C" int soar_mesh_texels_bytes(int32_t F, size_t *bytes)
{
    if (!bytes || F < 1 || F > TEX_MAX_F) { set_error("soar_mesh_texels_bytes: need 1 <= F <= 2^28 and a result pointer (F=%d)", F); return 1; }
    TexelBuf b;
    *bytes = carve_texels(b, nullptr, (size_t)F);
    return 0;
}

extern "C" int soar_mesh_texel_offsets(int32_t V, int32_t F, int32_t texture_size, const int32_t *faces, const int32_t *cell, void *workspace,
                                       size_t workspace_bytes, int64_t *total_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (V < 1 || V > TEX_MAX_V || F < 1 || F > TEX_MAX_F) {
        set_error("soar_mesh_texel_offsets: need 1 <= V <= 2^30 and 1 <= F <= 2^28 (V=%d, F=%d)", V, F);
        return 1;
    }
    if (!size_ok("soar_mesh_texel_offsets", texture_size)) return 1;
    if (!faces || !cell || !total_host) { set_error("soar_mesh_texel_offsets: NULL argument"); return 1; }
    TexelBuf b;
    if (!workspace_ok("soar_mesh_texel_offsets", workspace, workspace_bytes, carve_texels(b, workspace, (size_t)F), "soar_mesh_texels_bytes")) return 1;
    SOAR_HIP_OK(hipMemsetAsync(b.bad, 0, 8, stream));
    hipLaunchKernelGGL(texel_counts_kernel, dim3((F + 1 + 255) / 256), dim3(256), 0, stream, V, F, texture_size, faces, cell, b.counts, b.bad);
    SOAR_LAUNCH_OK("mesh_texel_counts", stream, 0);
    SOAR_HIP_OK(exclusive_scan_sum(b.scan_temp, b.scan_bytes, b.counts, b.offsets, (size_t)F + 1, stream));
    uint32_t bad[2] = {0, 0};
    uint64_t total = 0;
    SOAR_HIP_OK(hipMemcpyAsync(bad, b.bad, 8, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipMemcpyAsync(&total, b.offsets + F, 8, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    if (bad[0]) { set_error("soar_mesh_texel_offsets: %u cells are not a power-of-two square in [4, texture_size / 2], aligned to its side, inside the image, with half 0 or 1 (texture_size=%d)", bad[0], texture_size); return 1; }
    if (bad[1]) { set_error("soar_mesh_texel_offsets: %u faces name a vertex outside [0, %d)", bad[1], V); return 1; }
    if (total > (uint64_t)texture_size * (uint64_t)texture_size) { set_error("soar_mesh_texel_offsets: the cells own %llu texels, the image has only %d^2: some cells must overlap", (unsigned long long)total, texture_size); return 1; }
    *total_host = (int64_t)total;
    return 0;
}

extern "C" int soar_mesh_texels(int32_t V, int32_t F, int32_t texture_size, const float *verts, const int32_t *faces, const int32_t *cell,
                                const void *workspace, size_t workspace_bytes, int64_t first, int32_t count, float *pos_out, int32_t *addr_out,
                                int32_t *owner_img, float *bary_img, float *position_img, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (V < 1 || V > TEX_MAX_V || F < 1 || F > TEX_MAX_F || first < 0 || count < 1) {
        set_error("soar_mesh_texels: need 1 <= V <= 2^30, 1 <= F <= 2^28, first >= 0 and count >= 1 (V=%d, F=%d, first=%lld, count=%d)", V, F,
                  (long long)first, count);
        return 1;
    }
    if (!size_ok("soar_mesh_texels", texture_size)) return 1;
    if ((uint64_t)first + (uint64_t)count > (uint64_t)texture_size * (uint64_t)texture_size) {
        set_error("soar_mesh_texels: texels %lld .. %lld of an image of %d^2", (long long)first, (long long)first + count, texture_size);
        return 1;
    }
    if (!verts || !faces || !cell || !pos_out || !addr_out) { set_error("soar_mesh_texels: NULL argument"); return 1; }
    TexelBuf b;
    if (!workspace_ok("soar_mesh_texels", workspace, workspace_bytes, carve_texels(b, const_cast<void *>(workspace), (size_t)F), "soar_mesh_texels_bytes"))
        return 1;
    hipLaunchKernelGGL(texels_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, V, F, texture_size, verts, faces, cell, b.offsets,
                       (uint64_t)first, count, pos_out, addr_out, owner_img, bary_img, position_img);
    SOAR_LAUNCH_OK("mesh_texels", stream, 0);
    return 0;
}

extern "C" int soar_mesh_texture_write(int32_t count, int32_t texture_size, const int32_t *addr, const float *color, uint8_t *texture_out,
                                       float *color_img, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (count < 1) { set_error("soar_mesh_texture_write: need count >= 1 (count=%d)", count); return 1; }
    if (!size_ok("soar_mesh_texture_write", texture_size)) return 1;
    if (count > texture_size * texture_size) {
        set_error("soar_mesh_texture_write: count=%d texels for an image of %d^2", count, texture_size);
        return 1;
    }
    if (!addr || !color || !texture_out) { set_error("soar_mesh_texture_write: NULL argument"); return 1; }
    hipLaunchKernelGGL(texture_write_kernel, dim3((count + 255) / 256), dim3(256), 0, stream, count, texture_size, addr, color, texture_out, color_img);
    SOAR_LAUNCH_OK("mesh_texture_write", stream, 0);
    return 0;
}
