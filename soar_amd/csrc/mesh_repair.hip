// mesh_repair.hip -- removes the non-manifold edges and splits the non-manifold vertices of the exported mesh (soar_amd/mesh.py:
// repair_manifold, manifold_report), the two MeshLab filters of the reference's clean_mesh (geometry/mesh_utils.py:
// meshing_repair_non_manifold_edges(method=0), meshing_repair_non_manifold_vertices(vertdispratio=0)) as one order-free device
// computation.  DESIGN.md 9b, "Repairing non-manifold edges and vertices" states the definition; tests/mesh_repair_ref.py restates it.
//
// Half-edge h = 3 f + c runs faces[f][c] -> faces[f][(c + 1) % 3]; corner h is the corner of face f at faces[f][c], so the corners at
// the two ends of half-edge h are h and next(h).  The undirected edge key is lo << vb | hi with vb bits per vertex id (2^vb >= V); a
// face that is not used (a vertex outside [0, V), two equal corners) gets the key 1 << 2 vb, behind every edge.
//
//   repair_faces_kernel    one lane per face: refuses or drops it, or computes a2 = the squared length of (b - a) x (c - a), every
//                          operation rounded to float32 (-ffp-contract=off), and writes the face's live flag, its three (a2 bits,
//                          half-edge) pairs and its corners' union-find parents; one lane per vertex: its least-fan slot
//   (stable radix sort of the pairs by the a2 bits: ties stay in half-edge order, which is face order)
//   repair_keys_kernel     one lane per sorted entry: the edge key of its half-edge
//   (stable radix sort by the edge key: inside the run of an edge the faces now stand in ascending (a2 bits, face index), and a live
//    face stands once in it, because its three edges differ)
//   repair_mark_kernel     one lane per sorted entry: an entry with two more entries of its edge behind it is one of the first k - 2
//                          of k > 2, so its face goes (a same-value flag store; a face marked by several edges goes once).  No loop,
//                          and no limit on k.  The first entry of such a run counts the edge
//   repair_join_kernel     one lane per sorted entry, at work on the LAST entry of every run: all but the last two entries of the run
//                          were marked by this edge, so only these two can still be alive.  Both alive: the edge has exactly two
//                          faces; their corners at each end of the edge are joined (atomicMin hooking, the root of a set is its least
//                          corner, as in mesh.hip's component filter), and a pair that runs in the same direction is counted.  One
//                          alive: a border edge of the result
//   repair_fans_kernel     one lane per corner of a surviving face: its root (the fan's id) replaces its parent, and the vertex's
//                          least fan is taken with atomicMin
//   repair_flags_kernel    one lane per vertex: kept when a surviving face names it; one lane per corner: a root that is not its
//                          vertex's least fan asks for a copy; counts of kept vertices, surviving faces and copies
//   (soar_mesh_repair only: exclusive scan of the copy flags; compact_mesh (mesh_common.h) writes the kept vertices, their sources and
//    the surviving faces with the kept vertices' new ids)
//   repair_copies_kernel   one lane per corner of a surviving face whose fan is not its vertex's least: the face's output corner
//                          becomes the copy's id, kept vertices + the scan at the fan's root; the root's lane writes the copy and
//                          its source
//
// soar_mesh_repair runs the analysis again rather than trusting a workspace soar_mesh_repair_count filled: nothing is read that the
// same call did not write.  Integer atomics whose outcome does not depend on their order (atomicMin, same-value stores, counters),
// no float atomics, no host loop, no allocation; one stream synchronisation, for the counts.
#include "mesh_common.h"

#include <climits>

namespace soar {

namespace {

constexpr int32_t REPAIR_MAX_V = 1 << 30;
constexpr int32_t REPAIR_MAX_F = 1 << 28;           // 3 F corner ids stay in int32

enum { RC_MANY = 0, RC_NULL, RC_SAME, RC_BORDER, RC_VKEPT, RC_FKEPT, RC_COPIES, RC_N = 8 };

struct RepairBuf {
    uint32_t *akeys, *akeys_sorted;     // [3F] a2 bits of the half-edge's face
    uint32_t *ids, *ids_a, *ids_e;      // [3F] half-edges: in order, sorted by a2, then by edge
    uint64_t *ekeys, *ekeys_sorted;     // [3F] edge keys in ids_a's order, and sorted
    int32_t *parent;                    // [3F] union-find over the corners; after repair_fans_kernel the fan id of a surviving corner
    int32_t *vmin;                      // [V] least fan id at the vertex (INT_MAX: no surviving face names it)
    uint32_t *cflag, *coff;             // [3F] 1 at the root of a fan that gets a copy; exclusive scan
    uint32_t *counts;                   // [RC_N]
    CompactBuf c;                       // vkeep / fkeep (fkeep doubles as the faces' live flag from the first kernel on), scans, totals
    void *sort_temp;
    size_t sort_bytes;
};

// bits per vertex id in an edge key
inline unsigned vertex_bits(size_t V)
{
    unsigned vb = 1;
    while (((size_t)1 << vb) < V) vb++;
    return vb;
}

size_t carve_repair(RepairBuf &b, void *base, size_t V, size_t F)
{
    const size_t N = 3 * (F > 0 ? F : 1);
    Carver c(base);
    auto words = [&](size_t n) { return c.take<uint32_t>(n); };
    b.akeys = words(N);
    b.akeys_sorted = words(N);
    b.ids = words(N);
    b.ids_a = words(N);
    b.ids_e = words(N);
    b.ekeys = c.take<uint64_t>(N);
    b.ekeys_sorted = c.take<uint64_t>(N);
    b.parent = c.take<int32_t>(N);
    b.vmin = c.take<int32_t>(V);
    b.cflag = words(N);
    b.coff = words(N);
    b.counts = words(RC_N);
    const size_t sa = sort_pairs_temp_bytes<uint32_t, uint32_t>(N, 32u), se = sort_pairs_temp_bytes<uint64_t, uint32_t>(N, 2u * vertex_bits(V) + 1u);
    b.sort_bytes = sa > se ? sa : se;
    b.sort_temp = c.take<char>(b.sort_bytes);
    const size_t M = V > N ? V : N;
    carve_compact(c, b.c, V, F, scan_temp_bytes<uint32_t>(M));
    return c.bytes();
}

__device__ __forceinline__ uint32_t he_next(uint32_t h) { return h % 3u == 2u ? h - 2u : h + 1u; }

// one atomic per wavefront; every lane of the wavefront must arrive
__device__ __forceinline__ void count_wave(uint32_t *counter, bool one)
{
    const int n = wave_sum_i(one ? 1 : 0);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(counter, (uint32_t)n);
}

__device__ __forceinline__ int uf_find(int32_t *parent, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

// hook the larger root under the smaller one.  When the larger one was hooked elsewhere in the meantime (atomicMin returns another
// parent), the union continues from that parent: no link is ever lost, and every set ends at its least corner
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

// grid over max(V, F)
__global__ void __launch_bounds__(256) repair_faces_kernel(int V, int F, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                           RepairBuf b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < V) b.vmin[i] = INT_MAX;
    bool bad = false, null = false;
    if (i < F) {
        int c0, c1, c2;
        bad = !face_corners(V, faces, i, c0, c1, c2);
        null = !bad && (c0 == c1 || c1 == c2 || c0 == c2);
        uint32_t bits = 0u;
        if (!bad && !null) {
            const float *p0 = verts + (size_t)c0 * 3, *p1 = verts + (size_t)c1 * 3, *p2 = verts + (size_t)c2 * 3;
            const float ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
            const float vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
            const float nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const float a2 = (nx * nx + ny * ny) + nz * nz;
            __builtin_memcpy(&bits, &a2, 4);
        }
        b.c.fkeep[i] = bad || null ? 0u : 1u;
        for (int k = 0; k < 3; k++) {
            const size_t h = (size_t)i * 3 + k;
            b.akeys[h] = bits;
            b.ids[h] = (uint32_t)h;
            b.parent[h] = (int32_t)h;
        }
    }
    count_wave(b.c.totals + 2, bad);                  // reported by the host at the end of the call
    count_wave(b.counts + RC_NULL, null);
}

__global__ void __launch_bounds__(256) repair_keys_kernel(uint32_t n3, unsigned vb, const int32_t *__restrict__ faces, RepairBuf b)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n3) return;
    const uint32_t h = b.ids_a[i];
    uint64_t key = 1ull << (2u * vb);
    if (b.c.fkeep[h / 3u]) {                          // its corners are in [0, V) and differ
        const uint32_t p = (uint32_t)faces[h], q = (uint32_t)faces[he_next(h)];
        key = (uint64_t)(p < q ? p : q) << vb | (p < q ? q : p);
    }
    b.ekeys[i] = key;
}

__global__ void __launch_bounds__(256) repair_mark_kernel(uint32_t n3, unsigned vb, RepairBuf b)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool many = false;
    if (i < n3) {
        const uint64_t key = b.ekeys_sorted[i];
        if (key != 1ull << (2u * vb) && i + 2u < n3 && b.ekeys_sorted[i + 2u] == key) {
            b.c.fkeep[b.ids_e[i] / 3u] = 0u;
            many = i == 0u || b.ekeys_sorted[i - 1u] != key;
        }
    }
    count_wave(b.counts + RC_MANY, many);
}

__global__ void __launch_bounds__(256) repair_join_kernel(uint32_t n3, unsigned vb, const int32_t *__restrict__ faces, RepairBuf b)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool same = false, border = false;
    if (i < n3) {
        const uint64_t key = b.ekeys_sorted[i];
        if (key != 1ull << (2u * vb) && (i + 1u == n3 || b.ekeys_sorted[i + 1u] != key)) {
            const uint32_t h1 = b.ids_e[i];
            const bool s1 = b.c.fkeep[h1 / 3u] != 0u;
            bool s0 = false;
            uint32_t h0 = 0u;
            if (i > 0u && b.ekeys_sorted[i - 1u] == key) {
                h0 = b.ids_e[i - 1u];
                s0 = b.c.fkeep[h0 / 3u] != 0u;
            }
            if (s0 && s1) {
                same = faces[h0] == faces[h1];
                const uint32_t n0 = he_next(h0), n1 = he_next(h1);
                uf_union(b.parent, (int)h0, (int)(same ? h1 : n1));
                uf_union(b.parent, (int)n0, (int)(same ? n1 : h1));
            } else {
                border = s0 || s1;
            }
        }
    }
    count_wave(b.counts + RC_SAME, same);
    count_wave(b.counts + RC_BORDER, border);
}

// after the joins the forest is static: every surviving corner's root is written over its parent (a concurrent reader sees the old
// parent or the root, both ancestors)
__global__ void __launch_bounds__(256) repair_fans_kernel(uint32_t n3, const int32_t *__restrict__ faces, RepairBuf b)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n3 || !b.c.fkeep[i / 3u]) return;
    const int r = uf_find(b.parent, (int)i);
    __hip_atomic_store(b.parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicMin(b.vmin + faces[i], r);
}

// grid over max(V, 3 F)
__global__ void __launch_bounds__(256) repair_flags_kernel(int V, int F, uint32_t n3, const int32_t *__restrict__ faces, RepairBuf b)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    bool vk = false, fk = false, copy = false;
    if (i < (uint32_t)V) {
        vk = b.vmin[i] != INT_MAX;
        b.c.vkeep[i] = vk ? 1u : 0u;
    }
    if (i < (uint32_t)F) fk = b.c.fkeep[i] != 0u;
    if (i < n3) {
        copy = b.c.fkeep[i / 3u] && b.parent[i] == (int32_t)i && b.vmin[faces[i]] != (int32_t)i;
        b.cflag[i] = copy ? 1u : 0u;
    }
    count_wave(b.counts + RC_VKEPT, vk);
    count_wave(b.counts + RC_FKEPT, fk);
    count_wave(b.counts + RC_COPIES, copy);
}

__global__ void __launch_bounds__(256) repair_copies_kernel(uint32_t n3, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                            RepairBuf b, float *__restrict__ verts_out, int32_t *__restrict__ faces_out,
                                                            int32_t *__restrict__ source_out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n3) return;
    const uint32_t f = i / 3u;
    if (!b.c.fkeep[f]) return;
    const int v = faces[i], r = b.parent[i];
    if (r == b.vmin[v]) return;
    const size_t id = (size_t)b.c.totals[0] + b.coff[r];
    faces_out[(size_t)b.c.foff[f] * 3 + (i - 3u * f)] = (int32_t)id;
    if (r == (int)i) {
        for (int k = 0; k < 3; k++) verts_out[id * 3 + k] = verts[(size_t)v * 3 + k];
        source_out[id] = v;
    }
}

bool repair_sizes_ok(const char *what, int32_t V, int32_t F)
{
    if (V < 1 || V > REPAIR_MAX_V || F < 0 || F > REPAIR_MAX_F) {
        set_error("%s: need 1 <= V <= 2^30 and 0 <= F <= 2^28 (V=%d, F=%d)", what, V, F);
        return false;
    }
    return true;
}

void repair_empty_counts(int32_t V, int64_t *counts_host)
{
    for (int k = 0; k < 9; k++) counts_host[k] = 0;
    counts_host[6] = V;
}

// the analysis: everything up to the flags, nothing read back
int repair_analyse(const char *what, int32_t V, int32_t F, const float *verts, const int32_t *faces, const RepairBuf &b, hipStream_t stream)
{
    const uint32_t n3 = 3u * (uint32_t)F;
    const unsigned vb = vertex_bits((size_t)V);
    const dim3 blk(256), gh((n3 + 255u) / 256u);
    const uint32_t nvf = (uint32_t)(V > F ? V : F), nvh = (uint32_t)V > n3 ? (uint32_t)V : n3;
    SOAR_HIP_OK(hipMemsetAsync(b.counts, 0, RC_N * 4, stream));
    SOAR_HIP_OK(hipMemsetAsync(b.c.totals, 0, 12, stream));
    hipLaunchKernelGGL(repair_faces_kernel, dim3((nvf + 255u) / 256u), blk, 0, stream, V, F, verts, faces, b);
    SOAR_LAUNCH_OK("mesh_repair_faces", stream, 0);
    SOAR_HIP_OK(sort_pairs(b.sort_temp, b.sort_bytes, b.akeys, b.akeys_sorted, b.ids, b.ids_a, (size_t)n3, 32u, stream));
    hipLaunchKernelGGL(repair_keys_kernel, gh, blk, 0, stream, n3, vb, faces, b);
    SOAR_LAUNCH_OK("mesh_repair_keys", stream, 0);
    SOAR_HIP_OK(sort_pairs(b.sort_temp, b.sort_bytes, b.ekeys, b.ekeys_sorted, b.ids_a, b.ids_e, (size_t)n3, 2u * vb + 1u, stream));
    hipLaunchKernelGGL(repair_mark_kernel, gh, blk, 0, stream, n3, vb, b);
    hipLaunchKernelGGL(repair_join_kernel, gh, blk, 0, stream, n3, vb, faces, b);
    hipLaunchKernelGGL(repair_fans_kernel, gh, blk, 0, stream, n3, faces, b);
    hipLaunchKernelGGL(repair_flags_kernel, dim3((nvh + 255u) / 256u), blk, 0, stream, V, F, n3, faces, b);
    SOAR_LAUNCH_OK(what, stream, 0);
    return 0;
}

// tot = the device's counts, bad = faces refused
int repair_counts(const char *what, int32_t V, int32_t F, const uint32_t *tot, uint32_t bad, int64_t *counts_host)
{
    if (bad) { set_error("%s: %u faces name a vertex outside [0, %d)", what, bad, V); return 1; }
    counts_host[0] = (int64_t)tot[RC_VKEPT] + tot[RC_COPIES];
    counts_host[1] = tot[RC_FKEPT];
    counts_host[2] = tot[RC_MANY];
    counts_host[3] = (int64_t)F - tot[RC_NULL] - tot[RC_FKEPT];
    counts_host[4] = tot[RC_NULL];
    counts_host[5] = tot[RC_COPIES];
    counts_host[6] = (int64_t)V - tot[RC_VKEPT];
    counts_host[7] = tot[RC_SAME];
    counts_host[8] = tot[RC_BORDER];
    return 0;
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_mesh_repair_workspace_size(int32_t V, int32_t F, size_t *bytes)
{
    if (!bytes) { set_error("soar_mesh_repair_workspace_size: NULL result pointer"); return 1; }
    if (!repair_sizes_ok("soar_mesh_repair_workspace_size", V, F)) return 1;
    RepairBuf b;
    *bytes = carve_repair(b, nullptr, (size_t)V, (size_t)F);
    return 0;
}

extern "C" int soar_mesh_repair_count(int32_t V, int32_t F, const float *verts, const int32_t *faces, void *workspace,
                                      size_t workspace_bytes, int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!repair_sizes_ok("soar_mesh_repair_count", V, F)) return 1;
    if (!verts || !counts_host || (F > 0 && !faces)) { set_error("soar_mesh_repair_count: NULL argument"); return 1; }
    RepairBuf b;
    if (!workspace_ok("soar_mesh_repair_count", workspace, workspace_bytes, carve_repair(b, workspace, (size_t)V, (size_t)F),
                      "soar_mesh_repair_workspace_size"))
        return 1;
    if (F == 0) { repair_empty_counts(V, counts_host); return 0; }
    if (repair_analyse("mesh_repair_count", V, F, verts, faces, b, stream)) return 1;
    uint32_t tot[RC_N + 3];                           // the counts and the refused faces lie apart: two copies, one synchronisation
    SOAR_HIP_OK(hipMemcpyAsync(tot, b.counts, RC_N * 4, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipMemcpyAsync(tot + RC_N, b.c.totals, 12, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    return repair_counts("soar_mesh_repair_count", V, F, tot, tot[RC_N + 2], counts_host);
}

extern "C" int soar_mesh_repair(int32_t V, int32_t F, const float *verts, const int32_t *faces, void *workspace, size_t workspace_bytes,
                                float *verts_out, int32_t *faces_out, int32_t *source_out, int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!repair_sizes_ok("soar_mesh_repair", V, F)) return 1;
    if (!verts || !counts_host || (F > 0 && (!faces || !verts_out || !faces_out || !source_out))) {
        set_error("soar_mesh_repair: NULL argument");
        return 1;
    }
    if (F > 0 && (verts == verts_out || faces == faces_out)) { set_error("soar_mesh_repair: the outputs must not be the inputs"); return 1; }
    RepairBuf b;
    if (!workspace_ok("soar_mesh_repair", workspace, workspace_bytes, carve_repair(b, workspace, (size_t)V, (size_t)F), "soar_mesh_repair_workspace_size"))
        return 1;
    if (F == 0) { repair_empty_counts(V, counts_host); return 0; }
    const uint32_t n3 = 3u * (uint32_t)F;
    if (repair_analyse("mesh_repair", V, F, verts, faces, b, stream)) return 1;
    SOAR_HIP_OK(exclusive_scan_sum(b.c.scan_temp, b.c.scan_bytes, b.cflag, b.coff, (size_t)n3, stream));
    uint32_t tot[RC_N];                               // queued before compact_mesh: its synchronisation, the call's only one, delivers them
    SOAR_HIP_OK(hipMemcpyAsync(tot, b.counts, RC_N * 4, hipMemcpyDeviceToHost, stream));
    int64_t kept[2];
    if (compact_mesh("soar_mesh_repair", V, F, verts, faces, b.c, verts_out, faces_out, source_out, kept, stream)) return 1;
    hipLaunchKernelGGL(repair_copies_kernel, dim3((n3 + 255u) / 256u), dim3(256), 0, stream, n3, verts, faces, b, verts_out, faces_out,
                       source_out);
    SOAR_LAUNCH_OK("mesh_repair_copies", stream, 0);
    return repair_counts("soar_mesh_repair", V, F, tot, 0u, counts_host);
}
