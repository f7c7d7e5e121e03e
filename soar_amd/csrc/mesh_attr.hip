// mesh_attr.hip -- what turns the exported mesh (mesh.hip, mesh_simplify.hip) into a coloured, smoothed asset (soar_amd/mesh.py:
// vertex_attributes, adjacency, smooth, prune_by_quality).  The reference's meshing helper does this on the CPU with pytorch3d's
// knn_points and pymeshlab (utils/general_utils.py:248-302); DESIGN.md 9b, "Colour, smoothing, skinning" states the computation
// and what differs.
//
//   attr_transfer_kernel   one lane per mesh vertex.  Reads the vertex's K <= 8 neighbour indices into the surfel centres, which the
//                          grid search of lbs_knn.hip found (soar_lbs_knn_query with knn_idx_out; its generic kernel serves every
//                          K != 30).  ORDER OF THE NEIGHBOURS: that kernel returns its K in ascending order of ITS float32 squared
//                          distance, equal distances among them by ascending index, and this kernel keeps that order: rank 0
//                          is the nearest.  WHICH K it returns is the search's matter: it admits a point only when it is
//                          strictly nearer than the K-th so far, so of several points at exactly the K-th distance the one its
//                          grid walk met first stays, not the one with the lower index.  The set is unique whenever the K-th and
//                          (K+1)-th distances differ.  Writes
//                          color = clamp((c_0 + c_1 + ... + c_{K-1}) / K, 0, 1) added in rank order in float32, quality = the
//                          squared distance to rank 0, (dx dx + dy dy) + dz dz in float32, and optionally all K of them.
//   adj_keys_kernel        per face its six directed entries (i << 32 | j): both other corners for each corner.  The sorted
//                          keys (radix sort) ARE the adjacency in CSR form: row i = the entries of vertex i, ascending in j, a
//                          neighbour across an edge of m faces m times.  No atomics decide a position: deterministic.  (One
//                          sort of the whole key array takes the place of a count, a scan, a placement and a sort per row.)  A
//                          face that cannot be used writes six all-ones keys: they sort behind every row and belong to none.
//   adj_rows_kernel        one lane per vertex: the two ends of its row by binary search, and the border flag: a neighbour that
//                          stands exactly once in the row is across an edge of exactly one face.
//   smooth_step_kernel     one lane per vertex, one Jacobi step: S = the sum of the row's positions in row order (a border vertex
//                          adds only the neighbours that stand once), P' = (P + S) / (n + 1), n the number of terms; n = 0 keeps P.
//                          Gathers only, no float atomics: two runs give the same bits.
//   prune_flags_kernel     keep flags (a vertex goes when quality > thresh, a face when it touches one); compact_mesh
//                          (mesh_common.h) then does the two scans and the compaction in input order: re-indexed faces and the
//                          map keep[new] = old.
//
// Host read-backs (one stream synchronisation each): soar_mesh_attr_transfer and soar_mesh_adjacency read back the number of
// indices / faces they had to refuse, soar_mesh_prune that and its totals.  This is the export path, not the training step; the
// launch functions allocate nothing and keep no device state.  Built with -ffp-contract=off: the sums and squares are IEEE
// evaluations of the expressions as written, which tests/mesh_attr_ref.py restates.
#include "mesh_common.h"

namespace soar {

namespace {

constexpr int ATTR_MAXK = 8;
constexpr int32_t ATTR_MAX_V = 1 << 30;
constexpr int32_t ATTR_MAX_F = 1 << 28;           // 6 F row entries stay in int32

// ---- attribute transfer ------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) attr_transfer_kernel(int V, int N, int K, const float *__restrict__ verts,
                                                            const float *__restrict__ points, const float *__restrict__ colors,
                                                            const int32_t *__restrict__ idx, float *__restrict__ color_out,
                                                            float *__restrict__ quality_out, float *__restrict__ d2_out,
                                                            uint32_t *__restrict__ bad)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const float x = verts[(size_t)v * 3], y = verts[(size_t)v * 3 + 1], z = verts[(size_t)v * 3 + 2];
    float r = 0.f, g = 0.f, b = 0.f, q = 0.f;
    bool ok = true;
    for (int k = 0; k < K; k++) {
        const int id = idx[(size_t)v * K + k];
        if (id < 0 || id >= N) { ok = false; continue; }          // reported by the host; nothing is read through it
        const float dx = x - points[(size_t)id * 3], dy = y - points[(size_t)id * 3 + 1], dz = z - points[(size_t)id * 3 + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (k == 0) q = d2;
        if (d2_out) d2_out[(size_t)v * K + k] = d2;
        r += colors[(size_t)id * 3];
        g += colors[(size_t)id * 3 + 1];
        b += colors[(size_t)id * 3 + 2];
    }
    if (!ok) atomicAdd(bad, 1u);
    const float n = (float)K;
    color_out[(size_t)v * 3] = fminf(fmaxf(r / n, 0.f), 1.f);
    color_out[(size_t)v * 3 + 1] = fminf(fmaxf(g / n, 0.f), 1.f);
    color_out[(size_t)v * 3 + 2] = fminf(fmaxf(b / n, 0.f), 1.f);
    quality_out[v] = q;
}

// ---- adjacency ---------------------------------------------------------------------------------------------------------------

struct AdjBuf {
    uint64_t *keys, *keys_sorted;   // [6F] each
    uint32_t *bad;                  // [1] faces that name a vertex outside [0, V) or one vertex twice
    void *sort_temp;
    size_t sort_bytes;
};

size_t carve_adj(AdjBuf &b, void *base, size_t F)
{
    const size_t N = 6 * (F > 0 ? F : 1);
    Carver c(base);
    b.keys = c.take<uint64_t>(N);
    b.keys_sorted = c.take<uint64_t>(N);
    b.bad = c.take<uint32_t>(1);
    b.sort_bytes = sort_keys_temp_bytes<uint64_t>(N, 64u);
    b.sort_temp = c.take<char>(b.sort_bytes);
    return c.bytes();
}

__global__ void __launch_bounds__(256) adj_keys_kernel(int V, int F, const int32_t *__restrict__ faces, uint64_t *__restrict__ keys,
                                                       uint32_t *__restrict__ bad)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int c[3] = {faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]};
    const bool ok = c[0] >= 0 && c[0] < V && c[1] >= 0 && c[1] < V && c[2] >= 0 && c[2] < V && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
    if (!ok) atomicAdd(bad, 1u);                      // reported by the host; its keys sort behind every row
    for (int k = 0; k < 3; k++) {
        const uint64_t i = (uint64_t)(uint32_t)c[k] << 32;
        keys[(size_t)f * 6 + 2 * k] = ok ? i | (uint32_t)c[(k + 1) % 3] : ~0ull;
        keys[(size_t)f * 6 + 2 * k + 1] = ok ? i | (uint32_t)c[(k + 2) % 3] : ~0ull;
    }
}

__device__ __forceinline__ int lower_bound_key(const uint64_t *__restrict__ keys, int n, uint64_t key)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) adj_rows_kernel(int V, int nnz, const uint64_t *__restrict__ keys, int32_t *__restrict__ row_start,
                                                       uint8_t *__restrict__ border)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v > V) return;
    const int lo = lower_bound_key(keys, nnz, (uint64_t)(uint32_t)v << 32);
    row_start[v] = lo;
    if (v == V) return;
    const int hi = lower_bound_key(keys, nnz, (uint64_t)((uint32_t)v + 1u) << 32);
    bool bd = false;
    uint32_t prev = 0xffffffffu;                      // no vertex: V <= 2^30
    int run = 0;
    for (int e = lo; e < hi; e++) {
        const uint32_t j = (uint32_t)keys[e];
        if (j != prev) { bd |= run == 1; run = 0; prev = j; }
        run++;
    }
    bd |= run == 1;
    border[v] = bd ? 1 : 0;
}

__global__ void __launch_bounds__(256) adj_nbr_kernel(int nnz, const uint64_t *__restrict__ keys, int32_t *__restrict__ nbr)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < nnz) nbr[e] = (int32_t)(uint32_t)keys[e];
}

// ---- smoothing ---------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256) smooth_step_kernel(int V, int nnz, const float *__restrict__ src, const int32_t *__restrict__ row_start,
                                                          const int32_t *__restrict__ nbr, const uint8_t *__restrict__ border,
                                                          float *__restrict__ dst)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    // (a row outside [0, nnz] or an entry outside [0, V) is skipped, never read through: the arrays are the caller's)
    const int lo = min(max(row_start[v], 0), nnz), hi = min(max(row_start[v + 1], lo), nnz);
    const bool bd = border[v] != 0;
    const float px = src[(size_t)v * 3], py = src[(size_t)v * 3 + 1], pz = src[(size_t)v * 3 + 2];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int n = 0;
    for (int e = lo; e < hi; e++) {
        const int j = nbr[e];
        if (j < 0 || j >= V) continue;
        if (bd && !((e == lo || nbr[e - 1] != j) && (e + 1 == hi || nbr[e + 1] != j))) continue;     // border vertex: border edges only
        sx += src[(size_t)j * 3];
        sy += src[(size_t)j * 3 + 1];
        sz += src[(size_t)j * 3 + 2];
        n++;
    }
    const float d = (float)(n + 1);
    dst[(size_t)v * 3] = n ? (px + sx) / d : px;
    dst[(size_t)v * 3 + 1] = n ? (py + sy) / d : py;
    dst[(size_t)v * 3 + 2] = n ? (pz + sz) / d : pz;
}

// ---- pruning -----------------------------------------------------------------------------------------------------------------

size_t carve_prune(CompactBuf &b, void *base, size_t V, size_t F)
{
    const size_t M = V > F ? V : F;
    Carver c(base);
    carve_compact(c, b, V, F, scan_temp_bytes<uint32_t>(M > 0 ? M : 1));
    return c.bytes();
}

__global__ void __launch_bounds__(256) prune_flags_kernel(int V, int F, const int32_t *__restrict__ faces, const float *__restrict__ quality,
                                                          float thresh, CompactBuf b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < V) b.vkeep[i] = quality[i] > thresh ? 0u : 1u;            // (a NaN quality is not above the threshold: kept)
    if (i < F) {
        int a, c1, c2;
        const bool ok = face_corners(V, faces, i, a, c1, c2);
        if (!ok) atomicAdd(b.totals + 2, 1u);
        b.fkeep[i] = ok && !(quality[a] > thresh) && !(quality[c1] > thresh) && !(quality[c2] > thresh) ? 1u : 0u;
    }
}

bool sizes_ok(const char *what, int32_t V, int32_t F)
{
    if (V < 1 || V > ATTR_MAX_V || F < 0 || F > ATTR_MAX_F) {
        set_error("%s: need 1 <= V <= 2^30 and 0 <= F <= 2^28 (V=%d, F=%d)", what, V, F);
        return false;
    }
    return true;
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_mesh_attr_transfer_bytes(int32_t V, int32_t K, size_t *bytes)
{
    if (!bytes || V < 1 || V > ATTR_MAX_V || K < 1 || K > ATTR_MAXK) {
        set_error("soar_mesh_attr_transfer_bytes: need 1 <= V <= 2^30, 1 <= K <= %d and a result pointer (V=%d, K=%d)", ATTR_MAXK, V, K);
        return 1;
    }
    *bytes = 256;
    return 0;
}

extern "C" int soar_mesh_attr_transfer(int32_t V, int32_t N, int32_t K, const float *verts, const float *points, const float *colors,
                                       const int32_t *idx, void *workspace, size_t workspace_bytes, float *color_out, float *quality_out,
                                       float *d2_out, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (K < 1 || K > ATTR_MAXK) { set_error("soar_mesh_attr_transfer: need 1 <= K <= %d (K=%d)", ATTR_MAXK, K); return 1; }
    if (V < 1 || V > ATTR_MAX_V || N < 1) { set_error("soar_mesh_attr_transfer: need 1 <= V <= 2^30 and N >= 1 (V=%d, N=%d)", V, N); return 1; }
    if (!verts || !points || !colors || !idx || !color_out || !quality_out) { set_error("soar_mesh_attr_transfer: NULL argument"); return 1; }
    if (!workspace_ok("soar_mesh_attr_transfer", workspace, workspace_bytes, 256, "soar_mesh_attr_transfer_bytes")) return 1;
    uint32_t *bad = static_cast<uint32_t *>(workspace);
    SOAR_HIP_OK(hipMemsetAsync(bad, 0, 4, stream));
    hipLaunchKernelGGL(attr_transfer_kernel, dim3((V + 255) / 256), dim3(256), 0, stream, V, N, K, verts, points, colors, idx, color_out,
                       quality_out, d2_out, bad);
    SOAR_LAUNCH_OK("mesh_attr_transfer", stream, 0);
    uint32_t nbad = 0;
    SOAR_HIP_OK(hipMemcpyAsync(&nbad, bad, 4, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    if (nbad) { set_error("soar_mesh_attr_transfer: %u vertices have a neighbour index outside [0, %d)", nbad, N); return 1; }
    return 0;
}

extern "C" int soar_mesh_adjacency_bytes(int32_t V, int32_t F, size_t *bytes)
{
    if (!bytes) { set_error("soar_mesh_adjacency_bytes: NULL result pointer"); return 1; }
    if (!sizes_ok("soar_mesh_adjacency_bytes", V, F)) return 1;
    AdjBuf b;
    *bytes = carve_adj(b, nullptr, (size_t)F);
    return 0;
}

extern "C" int soar_mesh_adjacency(int32_t V, int32_t F, const int32_t *faces, void *workspace, size_t workspace_bytes, int32_t *row_start,
                                   int32_t *nbr, uint8_t *border, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!sizes_ok("soar_mesh_adjacency", V, F)) return 1;
    if (!row_start || !border || (F > 0 && (!faces || !nbr))) { set_error("soar_mesh_adjacency: NULL argument"); return 1; }
    AdjBuf b;
    if (!workspace_ok("soar_mesh_adjacency", workspace, workspace_bytes, carve_adj(b, workspace, (size_t)F), "soar_mesh_adjacency_bytes")) return 1;
    const int nnz = 6 * F;
    if (F > 0) {
        SOAR_HIP_OK(hipMemsetAsync(b.bad, 0, 4, stream));
        hipLaunchKernelGGL(adj_keys_kernel, dim3((F + 255) / 256), dim3(256), 0, stream, V, F, faces, b.keys, b.bad);
        SOAR_LAUNCH_OK("mesh_adjacency_keys", stream, 0);
        SOAR_HIP_OK(sort_keys(b.sort_temp, b.sort_bytes, b.keys, b.keys_sorted, (size_t)nnz, 64u, stream));
        hipLaunchKernelGGL(adj_nbr_kernel, dim3((nnz + 255) / 256), dim3(256), 0, stream, nnz, b.keys_sorted, nbr);
    }
    hipLaunchKernelGGL(adj_rows_kernel, dim3((V + 1 + 255) / 256), dim3(256), 0, stream, V, nnz, b.keys_sorted, row_start, border);
    SOAR_LAUNCH_OK("mesh_adjacency_rows", stream, 0);
    if (F > 0) {                                      // the one read-back, after everything is queued
        uint32_t nbad = 0;
        SOAR_HIP_OK(hipMemcpyAsync(&nbad, b.bad, 4, hipMemcpyDeviceToHost, stream));
        SOAR_HIP_OK(hipStreamSynchronize(stream));
        if (nbad) { set_error("soar_mesh_adjacency: %u faces name a vertex outside [0, %d) or one vertex twice", nbad, V); return 1; }
    }
    return 0;
}

extern "C" int soar_mesh_smooth_bytes(int32_t V, size_t *bytes)
{
    if (!bytes || V < 1 || V > ATTR_MAX_V) { set_error("soar_mesh_smooth_bytes: need 1 <= V <= 2^30 and a result pointer (V=%d)", V); return 1; }
    *bytes = align_up((size_t)V * 12);
    return 0;
}

extern "C" int soar_mesh_smooth(int32_t V, int32_t nnz, const float *verts, const int32_t *row_start, const int32_t *nbr,
                                const uint8_t *border, int32_t steps, void *workspace, size_t workspace_bytes, float *verts_out,
                                void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (V < 1 || V > ATTR_MAX_V || nnz < 0 || steps < 0) {
        set_error("soar_mesh_smooth: need 1 <= V <= 2^30, nnz >= 0 and steps >= 0 (V=%d, nnz=%d, steps=%d)", V, nnz, steps);
        return 1;
    }
    if (!verts || !row_start || !border || !verts_out || (nnz > 0 && !nbr)) { set_error("soar_mesh_smooth: NULL argument"); return 1; }
    if (verts == verts_out) { set_error("soar_mesh_smooth: verts_out must not be verts (a step reads the old positions)"); return 1; }
    if (!workspace_ok("soar_mesh_smooth", workspace, workspace_bytes, align_up((size_t)V * 12), "soar_mesh_smooth_bytes")) return 1;
    float *other = static_cast<float *>(workspace);
    const dim3 gv((V + 255) / 256), blk(256);
    if (steps == 0) {
        hipLaunchKernelGGL(copy_floats_kernel<>, dim3(((size_t)V * 3 + 255) / 256), blk, 0, stream, (size_t)V * 3, verts, verts_out);
        SOAR_LAUNCH_OK("mesh_smooth_copy", stream, 0);
        return 0;
    }
    const float *src = verts;
    for (int s = 1; s <= steps; s++) {                 // the last step writes verts_out
        float *dst = ((steps - s) & 1) ? other : verts_out;
        hipLaunchKernelGGL(smooth_step_kernel, gv, blk, 0, stream, V, nnz, src, row_start, nbr, border, dst);
        src = dst;
    }
    SOAR_LAUNCH_OK("mesh_smooth", stream, 0);
    return 0;
}

extern "C" int soar_mesh_prune_bytes(int32_t V, int32_t F, size_t *bytes)
{
    if (!bytes) { set_error("soar_mesh_prune_bytes: NULL result pointer"); return 1; }
    if (!sizes_ok("soar_mesh_prune_bytes", V, F)) return 1;
    CompactBuf b;
    *bytes = carve_prune(b, nullptr, (size_t)V, (size_t)F);
    return 0;
}

extern "C" int soar_mesh_prune(int32_t V, int32_t F, const float *verts, const int32_t *faces, const float *quality, float thresh,
                               void *workspace, size_t workspace_bytes, float *verts_out, int32_t *faces_out, int32_t *keep_out,
                               int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!sizes_ok("soar_mesh_prune", V, F)) return 1;
    if (!verts || !quality || !verts_out || !keep_out || !counts_host || (F > 0 && (!faces || !faces_out))) {
        set_error("soar_mesh_prune: NULL argument");
        return 1;
    }
    if (thresh != thresh) { set_error("soar_mesh_prune: the threshold is not a number"); return 1; }
    CompactBuf b;
    if (!workspace_ok("soar_mesh_prune", workspace, workspace_bytes, carve_prune(b, workspace, (size_t)V, (size_t)F), "soar_mesh_prune_bytes")) return 1;
    SOAR_HIP_OK(hipMemsetAsync(b.totals, 0, 12, stream));
    hipLaunchKernelGGL(prune_flags_kernel, dim3(((V > F ? V : F) + 255) / 256), dim3(256), 0, stream, V, F, faces, quality, thresh, b);
    SOAR_LAUNCH_OK("mesh_prune_flags", stream, 0);
    return compact_mesh("soar_mesh_prune", V, F, verts, faces, b, verts_out, faces_out, keep_out, counts_host, stream);
}
