// mesh.hip -- mesh export of a surfel avatar (soar_amd/mesh.py): TSDF fusion of rendered depth, marching cubes, removal of
// small connected components.  The reference meshes a Gaussian density sampled in Python-driven blocks with CPU marching cubes
// and pymeshlab clean-up (TS/geometry/gaussian_io.py:176-262, geometry/mesh_utils.py:91-150); this file replaces the three
// stages with deterministic kernels (DESIGN.md section "Mesh export").
//
//   tsdf_integrate_kernel  one thread per voxel gathers over the views of a call, no atomics: sum += s, weight += 1 per
//                          observation (s = +1 in free space, min(1, (depth - z) / trunc) in front of / near the surface);
//                          a NaN opacity, or an opaque pixel with a NaN depth, is no observation
//   mc_count_kernel        per voxel: the edges it owns (+x, +y, +z) that carry a vertex and the triangle count of its cell,
//                          packed into one u64 (vertices low, triangles high) and exclusive-scanned (rocPRIM): vertex and
//                          triangle ids follow (voxel, axis) and (cell, table order) -- a welded mesh, bit-identical per run
//   mc_emit_kernel         writes the vertices (index coordinates) and the triangles (mcubes_table.h, gen_mcubes_table.py)
//   filt_* kernels         union-find over the faces' edges (atomicMin hooking: the root of a component is its least vertex
//                          id, whatever the order of the hooks), face counts and bounding boxes per component (integer atomics
//                          on an order-preserving encoding of the coordinates), keep flags; compact_mesh (mesh_common.h) then
//                          scans the flags and writes the kept vertices and faces
//
// Host read-backs: soar_mc_count and soar_mesh_filter_components read their totals back (one stream synchronisation each) to
// size the outputs.  This is the export path, not the training step; the launch functions allocate nothing.
// Built with -ffp-contract=off: the vertex positions and the fused signed distances follow an IEEE evaluation of the
// expressions as written, which the CPU restatements in tests/ reproduce.
#include "mesh_common.h"
#include "preprocess_point.h"

#include <climits>

#define SOAR_MC_TABLE_SPACE __constant__
#include "mcubes_table.h"

namespace soar {

namespace {

constexpr int TSDF_MAX_VIEWS = 64;          // views per soar_tsdf_integrate call (their matrices sit in LDS)
constexpr int VIEW_FLOATS = 34;             // viewmatrix 16, projmatrix 16, prcppoint 2

__global__ void __launch_bounds__(256) tsdf_integrate_kernel(int n_views, int H, int W, const float *__restrict__ depth,
                                                             const float *__restrict__ opac, const float *__restrict__ viewm,
                                                             const float *__restrict__ projm, const float *__restrict__ prcp,
                                                             float ox, float oy, float oz, float voxel, int X, int Y, int Z,
                                                             float trunc, float znear, float min_opac, float *__restrict__ sum,
                                                             float *__restrict__ weight)
{
    __shared__ float cam[TSDF_MAX_VIEWS * VIEW_FLOATS];
    for (int e = threadIdx.x; e < n_views * VIEW_FLOATS; e += 256) {
        const int k = e / VIEW_FLOATS, c = e - k * VIEW_FLOATS;
        cam[e] = c < 16 ? viewm[k * 16 + c] : c < 32 ? projm[k * 16 + c - 16] : prcp[k * 2 + c - 32];
    }
    __syncthreads();
    const int N = X * Y * Z;                 // < 2^31: checked by the host
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int x = i / (Y * Z), r = i - x * (Y * Z), y = r / Z, z = r - y * Z;
    const float px = ox + (float)x * voxel, py = oy + (float)y * voxel, pz = oz + (float)z * voxel;
    float acc = sum[i], wt = weight[i];
    const size_t plane = (size_t)H * W;
    for (int k = 0; k < n_views; k++) {
        const float *V = cam + k * VIEW_FLOATS, *P = V + 16, *pp = V + 32;
        // row-vector convention: p_c = [p, 1] . V (world_view_transform), h = [p, 1] . P (full_proj_transform)
        const float zc = px * V[2] + py * V[6] + pz * V[10] + V[14];
        if (!(zc > znear)) continue;
        const float hx = px * P[0] + py * P[4] + pz * P[8] + P[12];
        const float hy = px * P[1] + py * P[5] + pz * P[9] + P[13];
        const float hw = px * P[3] + py * P[7] + pz * P[11] + P[15];
        const float fi = floorf(pix_from_ndc(hx / hw, W, pp[0]) + 0.5f);
        const float fj = floorf(pix_from_ndc(hy / hw, H, pp[1]) + 0.5f);
        if (!(fi >= 0.f && fi < (float)W && fj >= 0.f && fj < (float)H)) continue;     // (NaN fails too)
        const size_t pix = (size_t)k * plane + (size_t)fj * W + (size_t)fi;
        float s = 1.f;                                                                    // free space
        const float o = opac[pix];
        if (o != o) continue;                                                             // NaN opacity: no observation
        if (!(o < min_opac)) {
            const float eta = depth[pix] - zc;
            if (!(eta >= -trunc)) continue;                                               // hidden behind the surface, or a NaN depth
            s = fminf(1.f, eta / trunc);
        }
        acc += s;
        wt += 1.f;
    }
    sum[i] = acc;
    weight[i] = wt;
}

// ---- marching cubes ----------------------------------------------------------------------------------------------------

struct McBuf {
    uint64_t *packed;      // [N] edges with a vertex | triangles << 32
    uint64_t *offs;        // [N] exclusive scan of packed
    uint16_t *info;        // [N] edge mask (bits 0-2) | cell complete (bit 3) | case << 8
    uint64_t *totals;      // [1]
    void *scan_temp;
    size_t scan_bytes;
};

inline size_t carve_mc(McBuf &b, void *base, size_t N)
{
    Carver c(base);
    b.packed = c.take<uint64_t>(N);
    b.offs = c.take<uint64_t>(N);
    b.info = c.take<uint16_t>(N);
    b.totals = c.take<uint64_t>(1);
    b.scan_bytes = scan_temp_bytes<uint64_t>(N > 0 ? N : 1);
    b.scan_temp = c.take<char>(b.scan_bytes);
    return c.bytes();
}

struct McArgs {
    int X, Y, Z;
    float level;
    const float *f;
    const uint8_t *valid;
};

__global__ void __launch_bounds__(256) mc_count_kernel(McArgs a, uint64_t *__restrict__ packed, uint16_t *__restrict__ info)
{
    const int N = a.X * a.Y * a.Z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int YZ = a.Y * a.Z;
    const int x = i / YZ, r = i - x * YZ, y = r / a.Z, z = r - y * a.Z;
    const int stride[3] = {YZ, a.Z, 1};
    const bool has[3] = {x + 1 < a.X, y + 1 < a.Y, z + 1 < a.Z};
    const bool v0 = a.valid ? a.valid[i] != 0 : true;
    const bool in0 = a.f[i] < a.level;
    unsigned mask = 0;
    for (int ax = 0; ax < 3; ax++) {
        if (!has[ax] || !v0) continue;
        const int j = i + stride[ax];
        const bool vj = a.valid ? a.valid[j] != 0 : true;
        if (vj && (in0 != (a.f[j] < a.level))) mask |= 1u << ax;
    }
    unsigned cube = 0, complete = 0, ntri = 0;
    if (has[0] && has[1] && has[2]) {
        complete = 1;
        for (int c = 0; c < 8; c++) {
            const int j = i + (c & 1) * stride[0] + ((c >> 1) & 1) * stride[1] + ((c >> 2) & 1) * stride[2];
            if (a.valid && !a.valid[j]) { complete = 0; break; }
            cube |= (a.f[j] < a.level ? 1u : 0u) << c;
        }
        if (complete) ntri = kMcNumTris[cube];
        else cube = 0;
    }
    packed[i] = (uint64_t)__popc(mask) | ((uint64_t)ntri << 32);
    info[i] = (uint16_t)(mask | (complete << 3) | (cube << 8));
}

__global__ void mc_totals_kernel(int N, const uint64_t *__restrict__ packed, const uint64_t *__restrict__ offs,
                                 uint64_t *__restrict__ totals)
{
    totals[0] = offs[N - 1] + packed[N - 1];
}

__global__ void __launch_bounds__(256) mc_emit_kernel(McArgs a, const uint64_t *__restrict__ offs, const uint16_t *__restrict__ info,
                                                      float *__restrict__ verts, int32_t *__restrict__ faces)
{
    const int N = a.X * a.Y * a.Z;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int YZ = a.Y * a.Z;
    const int x = i / YZ, r = i - x * YZ, y = r / a.Z, z = r - y * a.Z;
    const int stride[3] = {YZ, a.Z, 1};
    const unsigned inf = info[i];
    const uint64_t off = offs[i];
    uint32_t vid = (uint32_t)off;
    for (int ax = 0; ax < 3; ax++) {
        if (!(inf & (1u << ax))) continue;
        const float f0 = a.f[i], f1 = a.f[i + stride[ax]];
        const float t = (a.level - f0) / (f1 - f0);
        float p[3] = {(float)x, (float)y, (float)z};
        p[ax] = p[ax] + t;
        verts[(size_t)vid * 3 + 0] = p[0];
        verts[(size_t)vid * 3 + 1] = p[1];
        verts[(size_t)vid * 3 + 2] = p[2];
        vid++;
    }
    if (!(inf & 8u)) return;
    const unsigned cube = inf >> 8;
    const int nt = kMcNumTris[cube];
    const size_t t0 = (size_t)(off >> 32);
    for (int t = 0; t < nt; t++) {
        for (int k = 0; k < 3; k++) {
            const int e = kMcTris[cube][3 * t + k];
            const int c = kMcEdgeCorner[e], ax = e >> 2;
            const int j = i + (c & 1) * stride[0] + ((c >> 1) & 1) * stride[1] + ((c >> 2) & 1) * stride[2];
            const unsigned below = info[j] & ((1u << ax) - 1u);
            faces[(t0 + t) * 3 + k] = (int32_t)((uint32_t)offs[j] + (uint32_t)__popc(below));
        }
    }
}

// ---- small-component removal -----------------------------------------------------------------------------------------

struct FiltBuf {
    int32_t *parent;       // [V] union-find forest, then the component label (least vertex id of the component)
    int32_t *fcount;       // [V] faces per component (at the label's row)
    int32_t *bbox;         // [V][6] ordered-int min xyz, max xyz per component
    int32_t *gbox;         // [6] the whole mesh's
    uint8_t *ref;          // [V] vertex used by a face
    CompactBuf c;          // keep flags, their scans, totals ([2]: faces with an index out of range)
};

inline size_t carve_filt(FiltBuf &b, void *base, size_t V, size_t F)
{
    Carver c(base);
    b.parent = c.take<int32_t>(V);
    b.fcount = c.take<int32_t>(V);
    b.bbox = c.take<int32_t>(V * 6);
    b.gbox = c.take<int32_t>(6);
    b.ref = c.take<uint8_t>(V);
    const size_t sv = scan_temp_bytes<uint32_t>(V > 0 ? V : 1), sf = scan_temp_bytes<uint32_t>(F > 0 ? F : 1);
    carve_compact(c, b.c, V, F, sv > sf ? sv : sf);
    return c.bytes();
}

__global__ void __launch_bounds__(256) filt_init_kernel(int V, FiltBuf b)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v == 0) {
        for (int k = 0; k < 3; k++) { b.gbox[k] = INT_MAX; b.gbox[3 + k] = INT_MIN; b.c.totals[k] = 0; }
    }
    if (v >= V) return;
    b.parent[v] = v;
    b.fcount[v] = 0;
    b.ref[v] = 0;
    for (int k = 0; k < 3; k++) { b.bbox[(size_t)v * 6 + k] = INT_MAX; b.bbox[(size_t)v * 6 + 3 + k] = INT_MIN; }
}

__device__ __forceinline__ int uf_find(int32_t *parent, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

// hook the larger root under the smaller one.  When the larger one was hooked elsewhere in the meantime (atomicMin returns
// another parent), the union continues from that parent: no link is ever lost, and every component ends at its least id
__device__ __forceinline__ void uf_union(int32_t *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(256) filt_hook_kernel(int V, int F, const int32_t *__restrict__ faces, FiltBuf b)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int a, c1, c2;
    if (!face_corners(V, faces, f, a, c1, c2)) {
        atomicAdd(b.c.totals + 2, 1u);                    // reported by the host; the face is ignored
        return;
    }
    b.ref[a] = 1;
    b.ref[c1] = 1;
    b.ref[c2] = 1;
    uf_union(b.parent, a, c1);
    uf_union(b.parent, c1, c2);
}

// after the hooks the forest is static: one pass that writes every vertex's root (a concurrent reader sees the old parent or
// the root, both ancestors)
__global__ void __launch_bounds__(256) filt_label_kernel(int V, FiltBuf b)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    int r = v;
    while (b.parent[r] != r) r = b.parent[r];
    b.parent[v] = r;
}

// faces per component.  Almost every wave of faces lies in one component: then ONE atomic per wave (Guideline 12)
__global__ void __launch_bounds__(256) filt_face_stats_kernel(int V, int F, const int32_t *__restrict__ faces, FiltBuf b)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    int lab = -1;
    int a, c1, c2;
    if (f < F && face_corners(V, faces, f, a, c1, c2)) lab = b.parent[a];
    const int top = wave_max_i(lab);
    if (__all(lab == top || lab < 0)) {
        const int n = wave_sum_i(lab >= 0 ? 1 : 0);
        if ((threadIdx.x & 63) == 0 && top >= 0) atomicAdd(b.fcount + top, n);
    } else if (lab >= 0) {
        atomicAdd(b.fcount + lab, 1);
    }
}

// bounding boxes per component and of the whole mesh (vertices used by a face)
__global__ void __launch_bounds__(256) filt_vert_stats_kernel(int V, const float *__restrict__ verts, FiltBuf b)
{
    __shared__ int red[4][6];
    const int v = blockIdx.x * 256 + threadIdx.x;
    const bool use = v < V && b.ref[v];
    const int lab = use ? b.parent[v] : -1;
    int lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        const int q = use ? ford(verts[(size_t)v * 3 + k]) : 0;
        lo[k] = use ? q : INT_MAX;
        hi[k] = use ? q : INT_MIN;
    }
    const int top = wave_max_i(lab);
    const bool uni = __all(lab == top || lab < 0);
    for (int k = 0; k < 3; k++) { lo[k] = wave_min_i(lo[k]); hi[k] = wave_max_i(hi[k]); }
    if (uni) {
        if ((threadIdx.x & 63) == 0 && top >= 0) {
            for (int k = 0; k < 3; k++) {
                atomicMin(b.bbox + (size_t)top * 6 + k, lo[k]);
                atomicMax(b.bbox + (size_t)top * 6 + 3 + k, hi[k]);
            }
        }
    } else if (use) {
        for (int k = 0; k < 3; k++) {
            const int q = ford(verts[(size_t)v * 3 + k]);
            atomicMin(b.bbox + (size_t)lab * 6 + k, q);
            atomicMax(b.bbox + (size_t)lab * 6 + 3 + k, q);
        }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) { red[w][k] = lo[k]; red[w][3 + k] = hi[k]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        int m = red[0][k];
        for (int j = 1; j < 4; j++) m = k < 3 ? min(m, red[j][k]) : max(m, red[j][k]);
        if (k < 3 ? m != INT_MAX : m != INT_MIN) {
            if (k < 3) atomicMin(b.gbox + k, m);
            else atomicMax(b.gbox + k, m);
        }
    }
}

__device__ __forceinline__ float box_diag(const int32_t *bx)
{
    const float dx = fdec(bx[3]) - fdec(bx[0]), dy = fdec(bx[4]) - fdec(bx[1]), dz = fdec(bx[5]) - fdec(bx[2]);
    return sqrtf(dx * dx + dy * dy + dz * dz);
}

__global__ void __launch_bounds__(256) filt_keep_verts_kernel(int V, int min_faces, float min_diag_frac, FiltBuf b)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    uint32_t keep = 0;
    if (b.ref[v]) {
        const int lab = b.parent[v];
        keep = b.fcount[lab] >= min_faces && !(box_diag(b.bbox + (size_t)lab * 6) < min_diag_frac * box_diag(b.gbox));
    }
    b.c.vkeep[v] = keep;
}

__global__ void __launch_bounds__(256) filt_keep_faces_kernel(int V, int F, const int32_t *__restrict__ faces, FiltBuf b)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int a, c1, c2;
    const bool ok = face_corners(V, faces, f, a, c1, c2);
    b.c.fkeep[f] = ok ? b.c.vkeep[a] : 0u;      // the three corners share a component
}

inline bool grid_ok(const char *what, int32_t X, int32_t Y, int32_t Z)
{
    if (X <= 0 || Y <= 0 || Z <= 0) { set_error("%s: non-positive grid dimension (%d, %d, %d)", what, X, Y, Z); return false; }
    if ((int64_t)X * Y * Z >= ((int64_t)1 << 31)) {
        set_error("%s: %d x %d x %d voxels: need fewer than 2^31", what, X, Y, Z);
        return false;
    }
    return true;
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_tsdf_integrate(int32_t n_views, int32_t H, int32_t W, const float *depth, const float *opac, const float *viewmatrix,
                                   const float *projmatrix, const float *prcppoint, float origin_x, float origin_y, float origin_z,
                                   float voxel, int32_t X, int32_t Y, int32_t Z, float trunc, float znear, float min_opacity,
                                   float *sum, float *weight, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_views <= 0 || n_views > TSDF_MAX_VIEWS) {
        set_error("soar_tsdf_integrate: need 1 <= n_views <= %d (n_views=%d)", TSDF_MAX_VIEWS, n_views);
        return 1;
    }
    if (H <= 0 || W <= 0) { set_error("soar_tsdf_integrate: non-positive image size (%d x %d)", H, W); return 1; }
    if (!grid_ok("soar_tsdf_integrate", X, Y, Z)) return 1;
    if (!depth || !opac || !viewmatrix || !projmatrix || !prcppoint || !sum || !weight) {
        set_error("soar_tsdf_integrate: NULL argument");
        return 1;
    }
    if (!(voxel > 0.f) || !(trunc > 0.f)) { set_error("soar_tsdf_integrate: voxel and trunc must be positive"); return 1; }
    const int N = X * Y * Z;
    hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, n_views, H, W, depth, opac, viewmatrix,
                       projmatrix, prcppoint, origin_x, origin_y, origin_z, voxel, X, Y, Z, trunc, znear, min_opacity, sum, weight);
    SOAR_LAUNCH_OK("tsdf_integrate", stream, 0);
    return 0;
}

extern "C" int soar_mc_workspace_bytes(int32_t X, int32_t Y, int32_t Z, size_t *bytes)
{
    if (!bytes) { set_error("soar_mc_workspace_bytes: NULL argument"); return 1; }
    if (!grid_ok("soar_mc_workspace_bytes", X, Y, Z)) return 1;
    McBuf b;
    *bytes = carve_mc(b, nullptr, (size_t)X * Y * Z);
    return 0;
}

static int mc_check(const char *what, int32_t X, int32_t Y, int32_t Z, const float *values, void *workspace, size_t workspace_bytes, McBuf &b)
{
    if (!grid_ok(what, X, Y, Z)) return 1;
    if (!values) { set_error("%s: NULL argument", what); return 1; }
    return workspace_ok(what, workspace, workspace_bytes, carve_mc(b, workspace, (size_t)X * Y * Z), "soar_mc_workspace_bytes") ? 0 : 1;
}

extern "C" int soar_mc_count(int32_t X, int32_t Y, int32_t Z, const float *values, const uint8_t *valid, float level, void *workspace,
                             size_t workspace_bytes, int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    McBuf b;
    if (mc_check("soar_mc_count", X, Y, Z, values, workspace, workspace_bytes, b)) return 1;
    if (!counts_host) { set_error("soar_mc_count: NULL counts_host"); return 1; }
    const int N = X * Y * Z;
    const McArgs a = {X, Y, Z, level, values, valid};
    hipLaunchKernelGGL(mc_count_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, a, b.packed, b.info);
    SOAR_HIP_OK(exclusive_scan_sum(b.scan_temp, b.scan_bytes, b.packed, b.offs, (size_t)N, stream));
    hipLaunchKernelGGL(mc_totals_kernel, dim3(1), dim3(1), 0, stream, N, b.packed, b.offs, b.totals);
    SOAR_LAUNCH_OK("mc_count", stream, 0);
    uint64_t tot = 0;
    SOAR_HIP_OK(hipMemcpyAsync(&tot, b.totals, 8, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    counts_host[0] = (int64_t)(tot & 0xffffffffull);
    counts_host[1] = (int64_t)(tot >> 32);
    if (counts_host[0] >= ((int64_t)1 << 31) || counts_host[1] >= ((int64_t)1 << 31)) {
        set_error("soar_mc_count: %lld vertices / %lld triangles: more than int32 ids can hold", (long long)counts_host[0],
                  (long long)counts_host[1]);
        return 1;
    }
    return 0;
}

extern "C" int soar_mc_emit(int32_t X, int32_t Y, int32_t Z, const float *values, const uint8_t *valid, float level, const void *workspace,
                            size_t workspace_bytes, float *verts, int32_t *faces, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    McBuf b;
    if (mc_check("soar_mc_emit", X, Y, Z, values, const_cast<void *>(workspace), workspace_bytes, b)) return 1;
    if (!verts || !faces) { set_error("soar_mc_emit: NULL verts / faces"); return 1; }
    const int N = X * Y * Z;
    const McArgs a = {X, Y, Z, level, values, valid};
    hipLaunchKernelGGL(mc_emit_kernel, dim3((N + 255) / 256), dim3(256), 0, stream, a, b.offs, b.info, verts, faces);
    SOAR_LAUNCH_OK("mc_emit", stream, 0);
    return 0;
}

extern "C" int soar_mesh_filter_bytes(int32_t V, int32_t F, size_t *bytes)
{
    if (!bytes || V <= 0 || F <= 0) { set_error("soar_mesh_filter_bytes: need V > 0, F > 0 and a result pointer"); return 1; }
    FiltBuf b;
    *bytes = carve_filt(b, nullptr, (size_t)V, (size_t)F);
    return 0;
}

extern "C" int soar_mesh_filter_components(int32_t V, int32_t F, const float *verts, const int32_t *faces, int32_t min_faces,
                                           float min_diag_frac, void *workspace, size_t workspace_bytes, float *verts_out,
                                           int32_t *faces_out, int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (V <= 0 || F <= 0) { set_error("soar_mesh_filter_components: need V > 0 and F > 0 (V=%d, F=%d)", V, F); return 1; }
    if (!verts || !faces || !verts_out || !faces_out || !counts_host) { set_error("soar_mesh_filter_components: NULL argument"); return 1; }
    FiltBuf b;
    if (!workspace_ok("soar_mesh_filter_components", workspace, workspace_bytes, carve_filt(b, workspace, (size_t)V, (size_t)F),
                      "soar_mesh_filter_bytes"))
        return 1;
    const dim3 gv((V + 255) / 256), gf((F + 255) / 256), blk(256);
    hipLaunchKernelGGL(filt_init_kernel, gv, blk, 0, stream, V, b);
    hipLaunchKernelGGL(filt_hook_kernel, gf, blk, 0, stream, V, F, faces, b);
    hipLaunchKernelGGL(filt_label_kernel, gv, blk, 0, stream, V, b);
    hipLaunchKernelGGL(filt_face_stats_kernel, gf, blk, 0, stream, V, F, faces, b);
    hipLaunchKernelGGL(filt_vert_stats_kernel, gv, blk, 0, stream, V, verts, b);
    hipLaunchKernelGGL(filt_keep_verts_kernel, gv, blk, 0, stream, V, min_faces, min_diag_frac, b);
    hipLaunchKernelGGL(filt_keep_faces_kernel, gf, blk, 0, stream, V, F, faces, b);
    SOAR_LAUNCH_OK("mesh_filter_stats", stream, 0);
    return compact_mesh("soar_mesh_filter_components", V, F, verts, faces, b.c, verts_out, faces_out, nullptr, counts_host, stream);
}
