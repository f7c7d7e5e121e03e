// mesh_simplify.hip -- decimation of an exported mesh by quadric vertex clustering (soar_amd/mesh.py: simplify, decimate).
// The reference decimates with pymeshlab's quadric edge collapse (TS/geometry/mesh_utils.py:45-88), a serial priority-queue
// algorithm on the host; this is its parallel, deterministic counterpart (Lindstrom 2000: one output vertex per occupied cell
// of a uniform grid, placed at the minimum of the summed face quadrics).  DESIGN.md section 9b states the computation.
//
//   simp_bbox_kernel     bounding box of the vertices (integer atomics on an order-preserving encoding: any order, same bits)
//   simp_vkey_kernel     cell key (ix * ny + iy) * nz + iz per vertex; a stable radix sort (rocPRIM) then lists the vertices
//                        cell by cell, in ascending vertex index inside a cell
//   simp_vhead / vassign head flags, a scan: clusters = occupied cells numbered in ascending key order
//   simp_fkey_kernel     per face the sorted triple of cluster ids as two keys (lo | mid, hi); two stable sorts bring equal
//                        triples together with the smallest input index first: that face survives (simp_fhead_kernel)
//   two scans            compact the surviving faces and the clusters they use
//   simp_pairs_kernel    the (cluster, face) stream: each face once per distinct used cluster of its corners; a stable sort by
//                        cluster leaves every cluster's faces in ascending input index
//   simp_place_kernel    one wavefront per used cluster.  The lanes fetch 64 faces (vertices) of the run at a time and form
//                        their float64 quadrics relative to the cell centre; the wave then adds them ONE AFTER THE OTHER in run
//                        order (v_readlane broadcasts), so a cluster's sum is the plain left-to-right sum over ascending face
//                        index whatever the launch shape -- no float atomics, no LDS, nothing that depends on scheduling.
//                        Lane 0 solves the 3 x 3 problem (cyclic Jacobi) and writes the vertex.
//   simp_faces_kernel    writes the surviving faces with their corners renumbered
//
// Host read-backs (the export path, like soar_mc_count): the bounding box, which sizes the grid, and the totals.
// Built with -ffp-contract=off: cell indices and float64 sums follow an IEEE evaluation of the expressions as written, which
// tests/mesh_simplify_ref.py restates.
#include "mesh_common.h"

#include <climits>
#include <cmath>

namespace soar {

namespace {

constexpr int SIMP_MAX_DIM = 1 << 21;          // cells per axis: three of them fit a 63-bit key
constexpr int SIMP_MAX_COUNT = 1 << 30;        // vertices, faces: 3 F pair positions fit 32 bits, (V + 255) / 256 an int
constexpr double SIMP_RANK_EPS = 1e-3;         // eigenvalues below this fraction of the largest count as zero (Lindstrom)

struct SimpGrid {
    float lo[3];
    float cell;
    int32_t n[3];
};

struct SimpBuf {
    int32_t *box;                       // [6] ordered-int min xyz, max xyz
    uint32_t *totals;                   // [4] clusters, output vertices, output faces, faces naming a vertex outside [0, V)
    uint64_t *vkey, *vkey_s;            // [V] cell key per vertex / sorted
    uint32_t *vidx, *vidx_s;            // [V] vertex ids / in key order
    uint32_t *vflag, *vscan;            // [V] first vertex of a cell, exclusive scan
    uint32_t *cid;                      // [V] cluster of a vertex
    uint32_t *cstart;                   // [V + 1] where a cluster's vertices start in vidx_s
    uint32_t *used, *voff;              // [V] cluster used by a surviving face, exclusive scan = output vertex id
    uint64_t *fk2, *fk2_s;              // [F] mid << cb | hi of the sorted cluster triple
    uint32_t *fk1, *fk1_g, *fk1_s;      // [F] lo of the triple: per face / in fk2 order / sorted
    uint32_t *fidx, *fidx_s, *fidx_s2;  // [F] face ids / after the first / after the second sort
    uint32_t *fkeep, *foff;             // [F] face survives, exclusive scan = output face id
    uint32_t *pk, *pk_s, *pv, *pv_s;    // [3 F] (cluster, face) pairs / sorted by cluster
    uint32_t *pbeg, *pend;              // [V] a cluster's run in pv_s
    void *temp;                         // rocPRIM
    size_t temp_bytes;
};

inline size_t simp_temp_bytes(size_t V, size_t F, hipStream_t stream)
{
    const size_t nv = V > 0 ? V : 1, nf = F > 0 ? F : 1;
    // the widest bit range.  In this rocPRIM the temporary size grows with the number of digit places; should another one need
    // more for a narrower range, its call is handed the size carved here, checks it and returns an error (never an overrun)
    const size_t sizes[5] = {scan_temp_bytes<uint32_t>(nv > nf ? nv : nf, stream), sort_pairs_temp_bytes<uint64_t, uint32_t>(nv, 64u, stream),
                             sort_pairs_temp_bytes<uint64_t, uint32_t>(nf, 64u, stream), sort_pairs_temp_bytes<uint32_t, uint32_t>(nf, 32u, stream),
                             sort_pairs_temp_bytes<uint32_t, uint32_t>(3 * nf, 32u, stream)};
    size_t best = 0;
    for (const size_t n : sizes) best = n > best ? n : best;
    return best;
}

inline size_t carve_simp(SimpBuf &b, void *base, size_t V, size_t F, hipStream_t stream)
{
    Carver c(base);
    auto u32 = [&](size_t n) { return c.take<uint32_t>(n); };
    auto u64 = [&](size_t n) { return c.take<uint64_t>(n); };
    b.box = c.take<int32_t>(6);
    b.totals = u32(4);
    b.vkey = u64(V); b.vkey_s = u64(V);
    b.vidx = u32(V); b.vidx_s = u32(V);
    b.vflag = u32(V); b.vscan = u32(V);
    b.cid = u32(V);
    b.cstart = u32(V + 1);
    b.used = u32(V); b.voff = u32(V);
    b.fk2 = u64(F); b.fk2_s = u64(F);
    b.fk1 = u32(F); b.fk1_g = u32(F); b.fk1_s = u32(F);
    b.fidx = u32(F); b.fidx_s = u32(F); b.fidx_s2 = u32(F);
    b.fkeep = u32(F); b.foff = u32(F);
    b.pk = u32(3 * F); b.pk_s = u32(3 * F); b.pv = u32(3 * F); b.pv_s = u32(3 * F);
    b.pbeg = u32(V); b.pend = u32(V);
    b.temp_bytes = simp_temp_bytes(V, F, stream);
    b.temp = c.take<char>(b.temp_bytes);
    return c.bytes();
}

__global__ void simp_init_kernel(SimpBuf b)
{
    for (int k = 0; k < 3; k++) { b.box[k] = INT_MAX; b.box[3 + k] = INT_MIN; }
    for (int k = 0; k < 4; k++) b.totals[k] = 0u;
}

__global__ void __launch_bounds__(256) simp_bbox_kernel(int V, const float *__restrict__ verts, SimpBuf b)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    int lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
        const int q = v < V ? ford(verts[(size_t)v * 3 + k]) : 0;
        lo[k] = wave_min_i(v < V ? q : INT_MAX);
        hi[k] = wave_max_i(v < V ? q : INT_MIN);
    }
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; k++) {
            atomicMin(b.box + k, lo[k]);
            atomicMax(b.box + 3 + k, hi[k]);
        }
}

__device__ __forceinline__ int simp_cell_index(float v, float lo, float cell, int n)
{
    const int i = (int)floorf((v - lo) / cell);
    return min(i, n - 1);
}

__global__ void __launch_bounds__(256) simp_vkey_kernel(int V, const float *__restrict__ verts, SimpGrid g, SimpBuf b)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    const int64_t ix = simp_cell_index(verts[(size_t)v * 3], g.lo[0], g.cell, g.n[0]);
    const int64_t iy = simp_cell_index(verts[(size_t)v * 3 + 1], g.lo[1], g.cell, g.n[1]);
    const int64_t iz = simp_cell_index(verts[(size_t)v * 3 + 2], g.lo[2], g.cell, g.n[2]);
    b.vkey[v] = (uint64_t)((ix * g.n[1] + iy) * g.n[2] + iz);
    b.vidx[v] = (uint32_t)v;
}

__global__ void __launch_bounds__(256) simp_vhead_kernel(int V, SimpBuf b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    b.vflag[i] = (i == 0 || b.vkey_s[i] != b.vkey_s[i - 1]) ? 1u : 0u;
    b.used[i] = 0u;
    b.pbeg[i] = 0u;
    b.pend[i] = 0u;
}

__global__ void __launch_bounds__(256) simp_vassign_kernel(int V, SimpBuf b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= V) return;
    const uint32_t c = b.vscan[i] + b.vflag[i] - 1u;
    b.cid[b.vidx_s[i]] = c;
    if (b.vflag[i]) b.cstart[c] = (uint32_t)i;
    if (i == V - 1) {
        b.cstart[c + 1] = (uint32_t)V;
        b.totals[0] = c + 1u;
    }
}

// cb = the bits that hold 0 .. V; the id V marks a face that is dropped (two corners in one cluster, or a bad index)
__global__ void __launch_bounds__(256) simp_fkey_kernel(int V, int F, const int32_t *__restrict__ faces, int cb, SimpBuf b)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int a, c1, c2;
    uint32_t lo = (uint32_t)V, mid = (uint32_t)V, hi = (uint32_t)V;
    if (!face_corners(V, faces, f, a, c1, c2)) {
        atomicAdd(b.totals + 3, 1u);
    } else {
        const uint32_t x = b.cid[a], y = b.cid[c1], z = b.cid[c2];
        if (x != y && y != z && x != z) {
            lo = min(x, min(y, z));
            hi = max(x, max(y, z));
            mid = (x ^ y ^ z) ^ lo ^ hi;
        }
    }
    b.fk1[f] = lo;
    b.fk2[f] = ((uint64_t)mid << cb) | hi;
    b.fidx[f] = (uint32_t)f;
}

__global__ void __launch_bounds__(256) simp_fgather_kernel(int F, SimpBuf b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < F) b.fk1_g[i] = b.fk1[b.fidx_s[i]];
}

// after the two sorts equal triples are neighbours, smallest input index first
__global__ void __launch_bounds__(256) simp_fhead_kernel(int V, int F, int cb, SimpBuf b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F) return;
    const uint32_t f = b.fidx_s2[i], lo = b.fk1_s[i];
    const uint64_t k2 = b.fk2[f];
    bool head = lo != (uint32_t)V;
    if (head && i > 0) head = lo != b.fk1_s[i - 1] || k2 != b.fk2[b.fidx_s2[i - 1]];
    b.fkeep[f] = head ? 1u : 0u;
    if (head) {
        b.used[lo] = 1u;
        b.used[(uint32_t)(k2 >> cb)] = 1u;
        b.used[(uint32_t)(k2 & ((1ull << cb) - 1ull))] = 1u;
    }
}

__global__ void simp_totals_kernel(int V, int F, SimpBuf b)
{
    b.totals[1] = b.voff[V - 1] + b.used[V - 1];
    b.totals[2] = b.foff[F - 1] + b.fkeep[F - 1];
}

__global__ void __launch_bounds__(256) simp_pairs_kernel(int V, int F, const int32_t *__restrict__ faces, SimpBuf b)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    int a, c1, c2;
    uint32_t k[3] = {(uint32_t)V, (uint32_t)V, (uint32_t)V};
    if (face_corners(V, faces, f, a, c1, c2)) {
        const uint32_t x = b.cid[a], y = b.cid[c1], z = b.cid[c2];
        if (b.used[x]) k[0] = x;
        if (y != x && b.used[y]) k[1] = y;
        if (z != x && z != y && b.used[z]) k[2] = z;
    }
    for (int j = 0; j < 3; j++) {
        b.pk[(size_t)f * 3 + j] = k[j];
        b.pv[(size_t)f * 3 + j] = (uint32_t)f;
    }
}

__global__ void __launch_bounds__(256) simp_pruns_kernel(int V, size_t N, SimpBuf b)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= N) return;
    const uint32_t k = b.pk_s[p];
    if (k == (uint32_t)V) return;
    if (p == 0 || b.pk_s[p - 1] != k) b.pbeg[k] = (uint32_t)p;
    if (p == N - 1 || b.pk_s[p + 1] != k) b.pend[k] = (uint32_t)(p + 1);
}

// the value lane j holds, in every lane (j is the same in all lanes)
__device__ __forceinline__ double simp_bcast(double x, int j)
{
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j);
    return __hiloint2double(hi, lo);
}

// eigenvalues w and eigenvectors (columns of v) of the symmetric matrix a, by cyclic Jacobi rotations
__device__ void simp_eigh3(double a[3][3], double w[3], double v[3][3])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 16; sweep++) {
        if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double g = 100.0 * fabs(apq);
                if (sweep > 3 && fabs(a[p][p]) + g == fabs(a[p][p]) && fabs(a[q][q]) + g == fabs(a[q][q])) {
                    a[p][q] = a[q][p] = 0.0;
                    continue;
                }
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                const int r = 3 - p - q;
                const double arp = a[r][p], arq = a[r][q];
                a[p][p] -= t * apq;
                a[q][q] += t * apq;
                a[p][q] = a[q][p] = 0.0;
                a[r][p] = a[p][r] = c * arp - s * arq;
                a[r][q] = a[q][r] = s * arp + c * arq;
                for (int i = 0; i < 3; i++) {
                    const double vip = v[i][p], viq = v[i][q];
                    v[i][p] = c * vip - s * viq;
                    v[i][q] = s * vip + c * viq;
                }
            }
    }
    for (int i = 0; i < 3; i++) w[i] = a[i][i];
}

__global__ void __launch_bounds__(256) simp_place_kernel(const float *__restrict__ verts, const int32_t *__restrict__ faces, SimpGrid g,
                                                         SimpBuf b, float *__restrict__ verts_out)
{
    const uint32_t c = blockIdx.x * 4u + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= b.totals[0] || !b.used[c]) return;                     // the same for the whole wavefront
    const uint32_t s0 = b.cstart[c], s1 = b.cstart[c + 1];
    const uint64_t key = b.vkey_s[s0];
    const uint64_t nz = (uint64_t)g.n[2], ny = (uint64_t)g.n[1];
    const uint64_t cell_i[3] = {key / nz / ny, key / nz % ny, key % nz};
    const double cell = (double)g.cell;
    double ctr[3];
    for (int k = 0; k < 3; k++) ctr[k] = (double)g.lo[k] + ((double)cell_i[k] + 0.5) * cell;

    // mean of the cluster's vertices, relative to the centre, summed in ascending vertex index
    double m[3] = {0.0, 0.0, 0.0};
    for (uint32_t s = s0; s < s1; s += 64u) {
        const int cnt = (int)min(64u, s1 - s);
        double p[3] = {0.0, 0.0, 0.0};
        if (lane < cnt) {
            const size_t v = b.vidx_s[s + lane];
            for (int k = 0; k < 3; k++) p[k] = (double)verts[v * 3 + k] - ctr[k];
        }
        for (int j = 0; j < cnt; j++)
            for (int k = 0; k < 3; k++) m[k] += simp_bcast(p[k], j);
    }
    for (int k = 0; k < 3; k++) m[k] /= (double)(s1 - s0);

    // the faces' quadrics a [u; d][u; d]^T as (xx, xy, xz, xd, yy, yz, yd, zz, zd, dd), summed in ascending face index
    double q[10];
    for (int t = 0; t < 10; t++) q[t] = 0.0;
    const uint32_t p0 = b.pbeg[c], p1 = b.pend[c];
    for (uint32_t s = p0; s < p1; s += 64u) {
        const int cnt = (int)min(64u, p1 - s);
        double fq[10];
        for (int t = 0; t < 10; t++) fq[t] = 0.0;
        if (lane < cnt) {
            const size_t f = b.pv_s[s + lane];
            double P[3][3];
            for (int j = 0; j < 3; j++) {
                const size_t v = (size_t)faces[f * 3 + j];
                for (int k = 0; k < 3; k++) P[j][k] = (double)verts[v * 3 + k] - ctr[k];
            }
            double e1[3], e2[3];
            for (int k = 0; k < 3; k++) { e1[k] = P[1][k] - P[0][k]; e2[k] = P[2][k] - P[0][k]; }
            const double n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
            const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (len != 0.0) {
                const double area = len / 2.0;
                double w[4];
                for (int k = 0; k < 3; k++) w[k] = n[k] / len;
                w[3] = -(w[0] * P[0][0] + w[1] * P[0][1] + w[2] * P[0][2]);
                int t = 0;
                for (int i = 0; i < 4; i++)
                    for (int j = i; j < 4; j++) fq[t++] = area * (w[i] * w[j]);
            }
        }
        for (int j = 0; j < cnt; j++)
            for (int t = 0; t < 10; t++) q[t] += simp_bcast(fq[t], j);
    }
    if (lane != 0) return;

    double A[3][3] = {{q[0], q[1], q[2]}, {q[1], q[4], q[5]}, {q[2], q[5], q[7]}};
    const double bv[3] = {q[3], q[6], q[8]};
    double r[3];
    for (int k = 0; k < 3; k++) r[k] = -bv[k] - (A[k][0] * m[0] + A[k][1] * m[1] + A[k][2] * m[2]);
    double w[3], E[3][3];
    simp_eigh3(A, w, E);
    const double wmax = fmax(w[0], fmax(w[1], w[2]));
    double x[3] = {m[0], m[1], m[2]};
    if (wmax > 0.0) {
        for (int i = 0; i < 3; i++) {
            if (w[i] < SIMP_RANK_EPS * wmax) continue;
            const double t = (E[0][i] * r[0] + E[1][i] * r[1] + E[2][i] * r[2]) / w[i];
            for (int k = 0; k < 3; k++) x[k] += E[k][i] * t;
        }
        if (!(fabs(x[0]) <= cell && fabs(x[1]) <= cell && fabs(x[2]) <= cell))
            for (int k = 0; k < 3; k++) x[k] = m[k];
    }
    const size_t o = b.voff[c];
    for (int k = 0; k < 3; k++) verts_out[o * 3 + k] = (float)(ctr[k] + x[k]);
}

__global__ void __launch_bounds__(256) simp_faces_kernel(int F, const int32_t *__restrict__ faces, SimpBuf b, int32_t *__restrict__ faces_out)
{
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= F || !b.fkeep[f]) return;
    const size_t o = b.foff[f];
    for (int k = 0; k < 3; k++) faces_out[o * 3 + k] = (int32_t)b.voff[b.cid[faces[(size_t)f * 3 + k]]];
}

inline int bit_width64(uint64_t x)
{
    int n = 0;
    while (x) { n++; x >>= 1; }
    return n;
}

// everything that can be refused without the device
int simp_check(const char *what, int32_t V, int32_t F, const float *verts, const int32_t *faces, float cell, void *workspace,
               size_t workspace_bytes, const int64_t *counts_host, hipStream_t stream, SimpBuf &b)
{
    if (V < 1 || F < 0) { set_error("%s: need V >= 1 and F >= 0 (V=%d, F=%d)", what, V, F); return 1; }
    if (V > SIMP_MAX_COUNT || F > SIMP_MAX_COUNT) { set_error("%s: at most 2^30 vertices and 2^30 faces (V=%d, F=%d)", what, V, F); return 1; }
    if (!(cell > 0.f) || !std::isfinite(cell)) { set_error("%s: the cell size must be positive and finite (cell=%g)", what, (double)cell); return 1; }
    if (!verts || (!faces && F > 0) || !counts_host) { set_error("%s: NULL argument", what); return 1; }
    // (the one place a call queries the sizes)
    return workspace_ok(what, workspace, workspace_bytes, carve_simp(b, workspace, (size_t)V, (size_t)F, stream), "soar_mesh_simplify_bytes") ? 0 : 1;
}

int simp_run(const char *what, int32_t V, int32_t F, const float *verts, const int32_t *faces, float cell, const SimpBuf &b,
             float *verts_out, int32_t *faces_out, int64_t *counts_host, hipStream_t stream)
{
    const dim3 gv((V + 255) / 256), gf((F + 255) / 256), blk(256);
    hipLaunchKernelGGL(simp_init_kernel, dim3(1), dim3(1), 0, stream, b);
    hipLaunchKernelGGL(simp_bbox_kernel, gv, blk, 0, stream, V, verts, b);
    SOAR_LAUNCH_OK("mesh_simplify_bbox", stream, 0);
    int32_t box[6];
    SOAR_HIP_OK(hipMemcpyAsync(box, b.box, 24, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    SimpGrid g;
    g.cell = cell;
    uint64_t cells = 1;
    for (int k = 0; k < 3; k++) {
        const float lo = fdec(box[k]), hi = fdec(box[3 + k]);
        if (!std::isfinite(lo) || !std::isfinite(hi)) { set_error("%s: a vertex coordinate is not finite", what); return 1; }
        const float q = (hi - lo) / cell;
        if (!(q < (float)SIMP_MAX_DIM)) {
            set_error("%s: the grid would have more than %d cells along axis %d (extent %g, cell %g)", what, SIMP_MAX_DIM, k,
                      (double)(hi - lo), (double)cell);
            return 1;
        }
        g.lo[k] = lo;
        g.n[k] = (int32_t)floorf(q) + 1;
        cells *= (uint64_t)g.n[k];
    }
    const unsigned vbits = (unsigned)(bit_width64(cells - 1) > 0 ? bit_width64(cells - 1) : 1);
    const int cb = bit_width64((uint64_t)V);

    hipLaunchKernelGGL(simp_vkey_kernel, gv, blk, 0, stream, V, verts, g, b);
    SOAR_HIP_OK(sort_pairs(b.temp, b.temp_bytes, b.vkey, b.vkey_s, b.vidx, b.vidx_s, (size_t)V, vbits, stream));
    hipLaunchKernelGGL(simp_vhead_kernel, gv, blk, 0, stream, V, b);
    SOAR_HIP_OK(exclusive_scan_sum(b.temp, b.temp_bytes, b.vflag, b.vscan, (size_t)V, stream));
    hipLaunchKernelGGL(simp_vassign_kernel, gv, blk, 0, stream, V, b);
    SOAR_LAUNCH_OK("mesh_simplify_clusters", stream, 0);
    counts_host[0] = counts_host[1] = 0;
    if (F == 0) return 0;

    hipLaunchKernelGGL(simp_fkey_kernel, gf, blk, 0, stream, V, F, faces, cb, b);
    SOAR_HIP_OK(sort_pairs(b.temp, b.temp_bytes, b.fk2, b.fk2_s, b.fidx, b.fidx_s, (size_t)F, (unsigned)(2 * cb), stream));
    hipLaunchKernelGGL(simp_fgather_kernel, gf, blk, 0, stream, F, b);
    SOAR_HIP_OK(sort_pairs(b.temp, b.temp_bytes, b.fk1_g, b.fk1_s, b.fidx_s, b.fidx_s2, (size_t)F, (unsigned)cb, stream));
    hipLaunchKernelGGL(simp_fhead_kernel, gf, blk, 0, stream, V, F, cb, b);
    SOAR_LAUNCH_OK("mesh_simplify_faces", stream, 0);
    SOAR_HIP_OK(exclusive_scan_sum(b.temp, b.temp_bytes, b.used, b.voff, (size_t)V, stream));
    SOAR_HIP_OK(exclusive_scan_sum(b.temp, b.temp_bytes, b.fkeep, b.foff, (size_t)F, stream));
    hipLaunchKernelGGL(simp_totals_kernel, dim3(1), dim3(1), 0, stream, V, F, b);
    SOAR_LAUNCH_OK("mesh_simplify_totals", stream, 0);
    uint32_t tot[4] = {0, 0, 0, 0};
    SOAR_HIP_OK(hipMemcpyAsync(tot, b.totals, 16, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    if (tot[3]) { set_error("%s: %u faces name a vertex outside [0, %d)", what, tot[3], V); return 1; }
    counts_host[0] = tot[1];
    counts_host[1] = tot[2];
    if (!verts_out || tot[2] == 0) return 0;

    const size_t N = (size_t)F * 3;
    hipLaunchKernelGGL(simp_pairs_kernel, gf, blk, 0, stream, V, F, faces, b);
    SOAR_HIP_OK(sort_pairs(b.temp, b.temp_bytes, b.pk, b.pk_s, b.pv, b.pv_s, N, (unsigned)cb, stream));
    hipLaunchKernelGGL(simp_pruns_kernel, dim3((unsigned)((N + 255) / 256)), blk, 0, stream, V, N, b);
    hipLaunchKernelGGL(simp_place_kernel, dim3((tot[0] + 3u) / 4u), blk, 0, stream, verts, faces, g, b, verts_out);
    hipLaunchKernelGGL(simp_faces_kernel, gf, blk, 0, stream, F, faces, b, faces_out);
    SOAR_LAUNCH_OK("mesh_simplify_write", stream, 0);
    return 0;
}

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_mesh_simplify_bytes(int32_t V, int32_t F, size_t *bytes)
{
    if (!bytes || V < 1 || F < 0 || V > SIMP_MAX_COUNT || F > SIMP_MAX_COUNT) {
        set_error("soar_mesh_simplify_bytes: need 1 <= V <= 2^30, 0 <= F <= 2^30 and a result pointer");
        return 1;
    }
    SimpBuf b;
    *bytes = carve_simp(b, nullptr, (size_t)V, (size_t)F, (hipStream_t)0);
    return 0;
}

extern "C" int soar_mesh_simplify_count(int32_t V, int32_t F, const float *verts, const int32_t *faces, float cell, void *workspace,
                                        size_t workspace_bytes, int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SimpBuf b;
    if (simp_check("soar_mesh_simplify_count", V, F, verts, faces, cell, workspace, workspace_bytes, counts_host, stream, b)) return 1;
    return simp_run("soar_mesh_simplify_count", V, F, verts, faces, cell, b, nullptr, nullptr, counts_host, stream);
}

extern "C" int soar_mesh_simplify(int32_t V, int32_t F, const float *verts, const int32_t *faces, float cell, void *workspace,
                                  size_t workspace_bytes, float *verts_out, int32_t *faces_out, int64_t *counts_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    SimpBuf b;
    if (simp_check("soar_mesh_simplify", V, F, verts, faces, cell, workspace, workspace_bytes, counts_host, stream, b)) return 1;
    if (!verts_out || !faces_out) { set_error("soar_mesh_simplify: NULL verts_out / faces_out"); return 1; }
    return simp_run("soar_mesh_simplify", V, F, verts, faces, cell, b, verts_out, faces_out, counts_host, stream);
}
