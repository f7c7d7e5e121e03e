// mesh_holes.hip -- closes the holes that pruning leaves in the exported mesh (soar_amd/mesh.py: close_holes), the step of the
// reference's meshing helper that pymeshlab's meshing_close_holes(maxholesize=300) does on the CPU (utils/general_utils.py:296).
// NOT MeshLab's minimum-weight ear cutting: a deterministic loop search with a centroid fan.  DESIGN.md 9b, "Closing holes" states
// the definition; tests/mesh_holes_ref.py restates it.
//
// Half-edge h = 3 f + c runs from(h) = faces[f][c] -> to(h) = faces[f][(c + 1) % 3].
//
//   holes_keys_kernel      one lane per face: its three (undirected edge key, half-edge id) pairs, lo << 32 | hi.  A face that cannot
//                          be used (a vertex outside [0, V), one vertex twice) is counted and writes all-ones keys: they sort behind
//                          every edge and are never borders, so nothing is read through their corners.  Copies the face to the output.
//   (radix sort of the pairs by key: the runs of length 1 are the border edges, as in mesh_attr.hip's adjacency)
//   holes_border_kernel    one lane per sorted entry: flags its half-edge as border or not (every half-edge stands once in the sorted
//                          values, so every flag is written) and, for a border, counts it at its two ends with integer atomics and
//                          records it as the border half-edge that ARRIVES at to(h).  A vertex is simple when exactly one border
//                          half-edge leaves it and exactly one arrives; the recorded arrival is read only at simple vertices, where
//                          it had one writer.
//   holes_walk_kernel      one lane per border half-edge: at most max_hole_edges steps of succ(h) = the border half-edge arriving at
//                          from(h), against the faces' orientation.  succ is one-to-one where every vertex is simple, so a walk that
//                          meets only simple vertices comes back to its start; it then knows the loop's length n, its leader (the
//                          least half-edge id on it) and its own rank in the ring from the leader, (n - steps to the leader) % n.  A
//                          walk that meets a vertex that is not simple, or does not come back in time, leaves its half-edge open.
//                          Every lane of a loop reaches the same verdict.  The leader writes the loop's three counts.
//   (three exclusive scans over the half-edges: where each loop's faces, vertex and length go; loops are emitted by ascending leader)
//   holes_fill_kernel      one lane per half-edge of a closed loop writes its own triangle (to(h), from(h), c): the border edge
//                          reversed.  The leader also writes the loop's length and the new vertex c: the mean of verts[to(h_k)] added
//                          in double in ring order from the leader, divided by n in double and rounded once to float32 -- serial,
//                          because the order is part of the definition and n <= 65535.  A loop of three gets one face and no vertex.
//
// No float atomics, no host loop over holes or steps, no allocation; one stream synchronisation, for the totals.  Built with
// -ffp-contract=off like its siblings (the centroid is adds and one divide; nothing here could contract).
#include "mesh_common.h"

namespace soar {

namespace {

constexpr int32_t HOLES_MAX_V = 1 << 30;
constexpr int32_t HOLES_MAX_F = 1 << 28;           // 3 F half-edge ids and 4 F output faces stay in int32
constexpr int32_t HOLES_MIN_EDGES = 3, HOLES_MAX_EDGES = 65535;
constexpr uint64_t NO_EDGE = ~0ull;

struct HolesBuf {
    uint64_t *keys, *keys_sorted;       // [3F] undirected edge keys
    uint32_t *ids, *ids_sorted;         // [3F] their half-edges
    uint32_t *n_out, *n_in, *arrive;    // [V] border half-edges leaving / arriving, and one that arrives
    uint8_t *border;                    // [3F]
    int32_t *leader, *rank;             // [3F] leader of the closed loop the half-edge is on (-1: none), place in its ring
    uint32_t *loop_n;                   // [3F] at a leader: the loop's length
    uint32_t *cnt_f, *cnt_v, *cnt_l;    // [3F] at a leader: faces, vertices (0 / 1), loops (1) it emits; 0 elsewhere
    uint32_t *off_f, *off_v, *off_l;    // [3F] their exclusive scans
    uint32_t *totals;                   // [0] faces refused, [1] border half-edges left open, [2] new faces, [3] new vertices, [4] loops
    void *sort_temp, *scan_temp;
    size_t sort_bytes, scan_bytes;
};

size_t carve_holes(HolesBuf &b, void *base, size_t V, size_t F)
{
    const size_t N = 3 * (F > 0 ? F : 1);
    Carver c(base);
    auto words = [&](size_t n) { return c.take<uint32_t>(n); };
    b.keys = c.take<uint64_t>(N);
    b.keys_sorted = c.take<uint64_t>(N);
    b.ids = words(N);
    b.ids_sorted = words(N);
    b.n_out = words(2 * V);             // n_out and n_in side by side: one memset clears both
    b.n_in = b.n_out ? b.n_out + V : nullptr;
    b.arrive = words(V);
    b.border = c.take<uint8_t>(N);
    b.leader = reinterpret_cast<int32_t *>(words(N));
    b.rank = reinterpret_cast<int32_t *>(words(N));
    b.loop_n = words(N);
    b.cnt_f = words(N);
    b.cnt_v = words(N);
    b.cnt_l = words(N);
    b.off_f = words(N);
    b.off_v = words(N);
    b.off_l = words(N);
    b.totals = words(8);
    b.sort_bytes = sort_pairs_temp_bytes<uint64_t, uint32_t>(N, 64u);
    b.scan_bytes = scan_temp_bytes<uint32_t>(N);
    b.sort_temp = c.take<char>(b.sort_bytes);
    b.scan_temp = c.take<char>(b.scan_bytes);
    return c.bytes();
}

__device__ __forceinline__ int he_from(const int32_t *__restrict__ faces, uint32_t h) { return faces[h]; }
__device__ __forceinline__ int he_to(const int32_t *__restrict__ faces, uint32_t h) { return faces[h % 3u == 2u ? h - 2u : h + 1u]; }

__global__ void __launch_bounds__(256) holes_keys_kernel(int V, int F, const int32_t *__restrict__ faces, HolesBuf b,
                                                         int32_t *__restrict__ faces_out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    const int c[3] = {faces[(size_t)f * 3], faces[(size_t)f * 3 + 1], faces[(size_t)f * 3 + 2]};
    const bool ok = c[0] >= 0 && c[0] < V && c[1] >= 0 && c[1] < V && c[2] >= 0 && c[2] < V && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
    if (!ok) atomicAdd(b.totals, 1u);                 // reported by the host at the end of the call
    for (int k = 0; k < 3; k++) {
        const uint32_t i = (uint32_t)c[k], j = (uint32_t)c[(k + 1) % 3];
        const size_t h = (size_t)f * 3 + k;
        b.keys[h] = ok ? (uint64_t)(i < j ? i : j) << 32 | (i < j ? j : i) : NO_EDGE;
        b.ids[h] = (uint32_t)h;
        faces_out[h] = c[k];
    }
}

__global__ void __launch_bounds__(256) holes_border_kernel(uint32_t n3, const int32_t *__restrict__ faces, HolesBuf b)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n3) return;
    const uint64_t key = b.keys_sorted[i];
    const uint32_t h = b.ids_sorted[i];
    const bool bd = key != NO_EDGE && (i == 0u || b.keys_sorted[i - 1] != key) && (i + 1u == n3 || b.keys_sorted[i + 1] != key);
    b.border[h] = bd ? 1 : 0;
    if (!bd) return;
    const int from = he_from(faces, h), to = he_to(faces, h);      // in [0, V): the key is a usable face's
    atomicAdd(b.n_out + from, 1u);
    atomicAdd(b.n_in + to, 1u);
    b.arrive[to] = h;                                              // (several writers only where the vertex is not simple: never read)
}

__global__ void __launch_bounds__(256) holes_walk_kernel(uint32_t n3, const int32_t *__restrict__ faces, int max_edges, HolesBuf b)
{
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= n3) return;
    uint32_t n = 0u, lead = h, to_lead = 0u;
    if (b.border[h]) {
        bool one_face = true;
        uint32_t cur = h;
        for (uint32_t step = 1u; step <= (uint32_t)max_edges; step++) {
            const int v = he_from(faces, cur);
            if (b.n_out[v] != 1u || b.n_in[v] != 1u) break;
            cur = b.arrive[v];
            one_face &= cur / 3u == h / 3u;
            if (cur == h) { n = step; break; }
            if (cur < lead) { lead = cur; to_lead = step; }
        }
        if (n < (uint32_t)HOLES_MIN_EDGES || one_face) n = 0u;     // (a lone triangle is not capped with its own mirror image)
        if (n == 0u) atomicAdd(b.totals + 1, 1u);                  // border half-edges left open (the compiler adds once per wavefront)
    }
    const bool closed = n != 0u, is_lead = closed && lead == h;
    b.leader[h] = closed ? (int32_t)lead : -1;
    b.rank[h] = closed ? (int32_t)((n - to_lead) % n) : 0;
    b.loop_n[h] = is_lead ? n : 0u;
    b.cnt_f[h] = is_lead ? (n == 3u ? 1u : n) : 0u;
    b.cnt_v[h] = is_lead && n > 3u ? 1u : 0u;
    b.cnt_l[h] = is_lead ? 1u : 0u;
}

__global__ void holes_totals_kernel(uint32_t n3, HolesBuf b)
{
    b.totals[2] = b.off_f[n3 - 1] + b.cnt_f[n3 - 1];
    b.totals[3] = b.off_v[n3 - 1] + b.cnt_v[n3 - 1];
    b.totals[4] = b.off_l[n3 - 1] + b.cnt_l[n3 - 1];
}

__global__ void __launch_bounds__(256) holes_fill_kernel(int V, int F, uint32_t n3, const float *__restrict__ verts,
                                                         const int32_t *__restrict__ faces, HolesBuf b, float *__restrict__ verts_out,
                                                         int32_t *__restrict__ faces_out, int32_t *__restrict__ loop_edges_out)
{
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= n3) return;
    const int32_t lead = b.leader[h];
    if (lead < 0) return;
    const uint32_t n = b.loop_n[lead];
    const size_t face0 = (size_t)F + b.off_f[lead];
    const int from = he_from(faces, h), to = he_to(faces, h);
    const bool is_lead = (uint32_t)lead == h;
    if (n == 3u) {
        if (is_lead) {
            faces_out[face0 * 3] = to;
            faces_out[face0 * 3 + 1] = from;
            faces_out[face0 * 3 + 2] = he_from(faces, b.arrive[from]);
            loop_edges_out[b.off_l[lead]] = 3;
        }
        return;
    }
    const size_t c = (size_t)V + b.off_v[lead], o = face0 + (size_t)b.rank[h];
    faces_out[o * 3] = to;
    faces_out[o * 3 + 1] = from;
    faces_out[o * 3 + 2] = (int32_t)c;
    if (!is_lead) return;
    loop_edges_out[b.off_l[lead]] = (int32_t)n;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    uint32_t cur = h;
    for (uint32_t k = 0u; k < n; k++) {                 // ring order from the leader: ((p_0 + p_1) + p_2) + ...
        const size_t t = (size_t)he_to(faces, cur);
        sx += (double)verts[t * 3];
        sy += (double)verts[t * 3 + 1];
        sz += (double)verts[t * 3 + 2];
        cur = b.arrive[he_from(faces, cur)];
    }
    const double d = (double)n;
    verts_out[c * 3] = (float)(sx / d);
    verts_out[c * 3 + 1] = (float)(sy / d);
    verts_out[c * 3 + 2] = (float)(sz / d);
}

bool holes_sizes_ok(const char *what, int32_t V, int32_t F)
{
    if (V < 1 || V > HOLES_MAX_V || F < 0 || F > HOLES_MAX_F) {
        set_error("%s: need 1 <= V <= 2^30 and 0 <= F <= 2^28 (V=%d, F=%d)", what, V, F);
        return false;
    }
    return true;
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_mesh_close_holes_bytes(int32_t V, int32_t F, size_t *bytes)
{
    if (!bytes) { set_error("soar_mesh_close_holes_bytes: NULL result pointer"); return 1; }
    if (!holes_sizes_ok("soar_mesh_close_holes_bytes", V, F)) return 1;
    HolesBuf b;
    *bytes = carve_holes(b, nullptr, (size_t)V, (size_t)F);
    return 0;
}

extern "C" int soar_mesh_close_holes(int32_t V, int32_t F, const float *verts, const int32_t *faces, int32_t max_hole_edges,
                                     void *workspace, size_t workspace_bytes, float *verts_out, int32_t *faces_out,
                                     int32_t *loop_edges_out, int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (!holes_sizes_ok("soar_mesh_close_holes", V, F)) return 1;
    if (max_hole_edges < HOLES_MIN_EDGES || max_hole_edges > HOLES_MAX_EDGES) {
        set_error("soar_mesh_close_holes: need %d <= max_hole_edges <= %d (max_hole_edges=%d)", HOLES_MIN_EDGES, HOLES_MAX_EDGES, max_hole_edges);
        return 1;
    }
    if (!verts || !verts_out || !counts_host || (F > 0 && (!faces || !faces_out || !loop_edges_out))) {
        set_error("soar_mesh_close_holes: NULL argument");
        return 1;
    }
    if (verts == verts_out || (F > 0 && faces == faces_out)) { set_error("soar_mesh_close_holes: the outputs must not be the inputs"); return 1; }
    HolesBuf b;
    if (!workspace_ok("soar_mesh_close_holes", workspace, workspace_bytes, carve_holes(b, workspace, (size_t)V, (size_t)F),
                      "soar_mesh_close_holes_bytes"))
        return 1;
    const dim3 blk(256);
    hipLaunchKernelGGL(copy_floats_kernel<>, dim3((unsigned)(((size_t)V * 3 + 255) / 256)), blk, 0, stream, (size_t)V * 3, verts, verts_out);
    SOAR_LAUNCH_OK("mesh_close_holes_copy", stream, 0);
    if (F == 0) {
        counts_host[0] = V;
        counts_host[1] = counts_host[2] = counts_host[3] = 0;
        return 0;
    }
    const uint32_t n3 = 3u * (uint32_t)F;
    const dim3 gh((n3 + 255u) / 256u);
    SOAR_HIP_OK(hipMemsetAsync(b.totals, 0, 32, stream));
    SOAR_HIP_OK(hipMemsetAsync(b.n_out, 0, (size_t)V * 8, stream));
    hipLaunchKernelGGL(holes_keys_kernel, dim3((F + 255) / 256), blk, 0, stream, V, F, faces, b, faces_out);
    SOAR_LAUNCH_OK("mesh_close_holes_keys", stream, 0);
    SOAR_HIP_OK(sort_pairs(b.sort_temp, b.sort_bytes, b.keys, b.keys_sorted, b.ids, b.ids_sorted, (size_t)n3, 64u, stream));
    hipLaunchKernelGGL(holes_border_kernel, gh, blk, 0, stream, n3, faces, b);
    hipLaunchKernelGGL(holes_walk_kernel, gh, blk, 0, stream, n3, faces, (int)max_hole_edges, b);
    SOAR_LAUNCH_OK("mesh_close_holes_walk", stream, 0);
    uint32_t *const cnt[3] = {b.cnt_f, b.cnt_v, b.cnt_l}, *const off[3] = {b.off_f, b.off_v, b.off_l};
    for (int k = 0; k < 3; k++) SOAR_HIP_OK(exclusive_scan_sum(b.scan_temp, b.scan_bytes, cnt[k], off[k], (size_t)n3, stream));
    hipLaunchKernelGGL(holes_totals_kernel, dim3(1), dim3(1), 0, stream, n3, b);
    hipLaunchKernelGGL(holes_fill_kernel, gh, blk, 0, stream, V, F, n3, verts, faces, b, verts_out, faces_out, loop_edges_out);
    SOAR_LAUNCH_OK("mesh_close_holes_fill", stream, 0);
    uint32_t tot[5] = {0, 0, 0, 0, 0};
    SOAR_HIP_OK(hipMemcpyAsync(tot, b.totals, sizeof(tot), hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    if (tot[0]) { set_error("soar_mesh_close_holes: %u faces name a vertex outside [0, %d) or one vertex twice", tot[0], V); return 1; }
    counts_host[0] = (int64_t)V + tot[3];
    counts_host[1] = (int64_t)F + tot[2];
    counts_host[2] = tot[4];
    counts_host[3] = tot[1];
    return 0;
}
