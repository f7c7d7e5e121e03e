// body.hip -- avatar initialisation on gfx950: the SMPL-X vertex forward, midpoint subdivision, vertex normals and surfel frames.
//
// Restates what the guidance's configure() gets from smplx / trimesh / pytorch3d (TS/utils/smpl.py:89-143, :367-374, :407):
//   * smplx_vertices_kernel : lbs() of the vendored body model (TS/utils/smplx/lbs.py:197-241) + transl, B frames in one launch.
//       v_shaped = v_template + shapedirs betas;  v_posed = v_shaped + (R[1:] - I) posedirs;  vertex = (sum_j W_vj A_j) [v_posed, 1] + transl
//     A workgroup owns 64 vertices and a tile of 8 frames.  Its 8 waves cut the K = 9 (J - 1) rows of posedirs into 8 slices: a lane
//     owns one vertex's three columns and keeps 8 x 3 accumulators, so every posedirs element it loads serves the 8 frames; the
//     tile's features sit in LDS ([K][8]: two broadcast 128-bit reads per row).  The slices' partial sums meet in LDS and are added in
//     slice order by wave f for frame f, which also adds the shape blend and skins the vertex; the joint matrices of that frame are
//     wave-uniform.  Plain FMAs, not the f32 MFMA: both peak at 64 FLOP/clk/SIMD, and at the batch sizes of an initialisation
//     (1 .. a few frames) the launch is bound by the 61 MB of posedirs, not by arithmetic.
//     Every sum is an fmaf chain in a fixed order that depends on neither B nor the frame's place in its tile; no atomics.
//   * subdivision           : one new vertex per unique edge (64-bit keys (min << 32) | max, radix-sorted, compacted; new vertices
//     follow the old ones in ascending key order), four faces per face in the parent's orientation.
//   * vertex normals        : (vertex, corner) pairs radix-sorted, every vertex adds its corners' weighted unit face normals in
//     ascending corner order -- no float atomics, bit-reproducible.
//   * surfel frames         : ux = normalize(uz x rand), uy = normalize(uz x ux), [ux uy uz] -> quaternion (soar_quat.h).
#include "mesh_common.h"
#include "soar_quat.h"
#include "soar_rodrigues.h"

namespace soar {

namespace {

// ------------------------------------------------------------------------------------------------------------------------------
// SMPL-X vertices
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int VT_VERTS = 64;       // vertices per workgroup = lanes of a wave
constexpr int VT_SLICES = 8;       // waves per workgroup = slices of the posedirs rows
constexpr int VT_FRAMES = 8;       // frames per workgroup (== VT_SLICES: wave f finishes frame f)
constexpr int VT_THREADS = VT_VERTS * VT_SLICES;
constexpr int VT_MAX_J = 64;
static_assert(VT_FRAMES == VT_SLICES, "wave f of a workgroup finishes frame f of its tile");

struct VertArgs {
    int B, V, J, NB, betas_batch;
    const float *betas;         // [betas_batch, NB]
    const float *v_template;    // [V,3]
    const float *shapedirs;     // [V,3,NB]
    const float *posedirs;      // [(J-1)*9, V*3]
    const float *lbs_weights;   // [V,J]
    const float *full_pose;     // [B, J*3]
    const float *A;             // [B,J,4,4] (without transl)
    const float *transl;        // [B,3] or nullptr
    float *out;                 // [B,V,3]
};

__global__ void __launch_bounds__(VT_THREADS) smplx_vertices_kernel(VertArgs a)
{
    // first the tile's pose features [K][VT_FRAMES], later the slices' partial sums [slice][frame][lane][3]
    __shared__ __attribute__((aligned(16))) float smem[VT_SLICES * VT_FRAMES * VT_VERTS * 3];
    static_assert((VT_MAX_J - 1) * 9 * VT_FRAMES <= VT_SLICES * VT_FRAMES * VT_VERTS * 3, "features must fit");
    const int tid = threadIdx.x, lane = tid & (VT_VERTS - 1);
    const int s = __builtin_amdgcn_readfirstlane(tid / VT_VERTS);
    const int v = blockIdx.x * VT_VERTS + lane, b0 = blockIdx.y * VT_FRAMES;
    const int J1 = a.J - 1, K = J1 * 9;

    // pose feature (R_j - I) of the joints 1 .. J-1 of every frame of the tile; frames past B are zero
    for (int t = tid; t < VT_FRAMES * J1; t += VT_THREADS) {
        const int f = t / J1, j = 1 + t % J1, b = b0 + f;
        float R[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (b < a.B) {
            rodrigues<3>(a.full_pose + ((size_t)b * a.J + j) * 3, R);
            R[0] -= 1.f; R[4] -= 1.f; R[8] -= 1.f;
        }
        for (int e = 0; e < 9; e++) smem[((j - 1) * 9 + e) * VT_FRAMES + f] = R[e];
    }
    __syncthreads();

    // this wave's slice of rows; the lanes past V read the last vertex and write nothing
    const int per = (K + VT_SLICES - 1) / VT_SLICES;
    const int k0 = s * per, k1 = min(K, k0 + per);
    const size_t row = (size_t)a.V * 3;
    const float *pd = a.posedirs + (size_t)min(v, a.V - 1) * 3;
    float acc[VT_FRAMES][3];
#pragma unroll
    for (int f = 0; f < VT_FRAMES; f++) acc[f][0] = acc[f][1] = acc[f][2] = 0.f;
#pragma unroll 4
    for (int k = k0; k < k1; k++) {
        const float *p = pd + (size_t)k * row;
        const float x = p[0], y = p[1], z = p[2];
        const float4 fa = *reinterpret_cast<const float4 *>(&smem[k * VT_FRAMES]);
        const float4 fb = *reinterpret_cast<const float4 *>(&smem[k * VT_FRAMES + 4]);
        const float ft[VT_FRAMES] = {fa.x, fa.y, fa.z, fa.w, fb.x, fb.y, fb.z, fb.w};
#pragma unroll
        for (int f = 0; f < VT_FRAMES; f++) {
            acc[f][0] = fmaf(ft[f], x, acc[f][0]);
            acc[f][1] = fmaf(ft[f], y, acc[f][1]);
            acc[f][2] = fmaf(ft[f], z, acc[f][2]);
        }
    }
    __syncthreads();                                   // every wave is done with the features
#pragma unroll
    for (int f = 0; f < VT_FRAMES; f++)
#pragma unroll
        for (int c = 0; c < 3; c++) smem[((s * VT_FRAMES + f) * VT_VERTS + lane) * 3 + c] = acc[f][c];
    __syncthreads();

    // wave f finishes frame f of the tile
    const int b = b0 + s;
    if (b >= a.B || v >= a.V) return;
    float vp[3];
    const float *be = a.betas + (size_t)(a.betas_batch > 1 ? b : 0) * a.NB;
    for (int c = 0; c < 3; c++) {
        float off = smem[((0 * VT_FRAMES + s) * VT_VERTS + lane) * 3 + c];
        for (int q = 1; q < VT_SLICES; q++) off += smem[((q * VT_FRAMES + s) * VT_VERTS + lane) * 3 + c];
        float sh = 0.f;
        const float *sd = a.shapedirs + ((size_t)v * 3 + c) * a.NB;
        for (int l = 0; l < a.NB; l++) sh = fmaf(be[l], sd[l], sh);
        vp[c] = off + (a.v_template[(size_t)v * 3 + c] + sh);
    }
    float T[12];
#pragma unroll
    for (int c = 0; c < 12; c++) T[c] = 0.f;
    const float *w = a.lbs_weights + (size_t)v * a.J;
    const float *Ab = a.A + (size_t)b * a.J * 16;
    for (int j = 0; j < a.J; j++) {
        const float wj = w[j];
#pragma unroll
        for (int c = 0; c < 12; c++) T[c] = fmaf(wj, Ab[j * 16 + c], T[c]);
    }
    float *o = a.out + ((size_t)b * a.V + v) * 3;
    for (int r = 0; r < 3; r++) {
        float t = T[r * 4] * vp[0];
        t = fmaf(T[r * 4 + 1], vp[1], t);
        t = fmaf(T[r * 4 + 2], vp[2], t);
        t = t + T[r * 4 + 3];
        if (a.transl) t = t + a.transl[b * 3 + r];
        o[r] = t;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// mesh helpers
// ------------------------------------------------------------------------------------------------------------------------------
// No FMA contraction from here on: a cross product of parallel vectors must be exactly zero (a1 b2 - a2 b1 with both products
// rounded), as in the float64 restatement, and the midpoints must equal numpy's float32 (a + b) * 0.5.
#pragma clang fp contract(off)

struct MeshBuf {
    uint64_t *keys, *keys_sorted, *ukeys;   // [3F] each
    uint32_t *head, *uid;                   // [3F] each
    uint32_t *totals;                       // [0] unique edges, [1] faces naming a vertex outside [0, V)
    void *sort_temp, *scan_temp;
    size_t sort_bytes, scan_bytes;
};

size_t carve_mesh(MeshBuf &b, void *base, size_t F)
{
    const size_t N = 3 * (F > 0 ? F : 1);
    Carver c(base);
    b.keys = c.take<uint64_t>(N);
    b.keys_sorted = c.take<uint64_t>(N);
    b.ukeys = c.take<uint64_t>(N);
    b.head = c.take<uint32_t>(N);
    b.uid = c.take<uint32_t>(N);
    b.totals = c.take<uint32_t>(64);
    b.sort_bytes = sort_keys_temp_bytes<uint64_t>(N, 64u);
    b.scan_bytes = scan_temp_bytes<uint32_t>(N);
    b.sort_temp = c.take<char>(b.sort_bytes);
    b.scan_temp = c.take<char>(b.scan_bytes);
    return c.bytes();
}

__device__ __forceinline__ uint64_t edge_key(int a, int b)
{
    const uint32_t lo = (uint32_t)min(a, b), hi = (uint32_t)max(a, b);
    return ((uint64_t)lo << 32) | hi;
}

// keys of the three edges (ab, bc, ca) of every face; a face naming a vertex outside [0, V) raises totals[1] and gets zero keys
__global__ void __launch_bounds__(256) edge_keys_kernel(int V, int F, const int *__restrict__ faces, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ totals)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int a, b, c;
    const bool ok = face_corners(V, faces, f, a, b, c);
    if (!ok) totals[1] = 1u;
    keys[3 * f] = ok ? edge_key(a, b) : 0ull;
    keys[3 * f + 1] = ok ? edge_key(b, c) : 0ull;
    keys[3 * f + 2] = ok ? edge_key(c, a) : 0ull;
}

// (vertex << 32) | corner id of the three corners of every face (corner id = 3 f + c)
__global__ void __launch_bounds__(256) corner_keys_kernel(int V, int F, const int *__restrict__ faces, uint64_t *__restrict__ keys,
                                                          uint32_t *__restrict__ totals)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    for (int c = 0; c < 3; c++) {
        const int v = faces[3 * f + c];
        const bool ok = v >= 0 && v < V;
        if (!ok) totals[1] = 1u;
        keys[3 * f + c] = ((uint64_t)(uint32_t)(ok ? v : 0) << 32) | (uint32_t)(3 * f + c);
    }
}

__global__ void __launch_bounds__(256) head_kernel(int N, const uint64_t *__restrict__ ks, uint32_t *__restrict__ head)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    head[i] = (i == 0 || ks[i] != ks[i - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) compact_kernel(int N, const uint64_t *__restrict__ ks, const uint32_t *__restrict__ head,
                                                      const uint32_t *__restrict__ uid, uint64_t *__restrict__ ukeys,
                                                      uint32_t *__restrict__ totals)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (head[i]) ukeys[uid[i]] = ks[i];
    if (i == N - 1) totals[0] = uid[i] + head[i];
}

__global__ void __launch_bounds__(256) midpoints_kernel(int V, int E, const float *__restrict__ verts, const uint64_t *__restrict__ ukeys,
                                                        float *__restrict__ out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const uint64_t key = ukeys[e];
    const size_t a = (size_t)(key >> 32), b = (size_t)(key & 0xffffffffull);
    if (a >= (size_t)V || b >= (size_t)V) return;           // a workspace that is not this mesh's: read nothing out of range
    for (int c = 0; c < 3; c++) out[((size_t)V + e) * 3 + c] = (verts[a * 3 + c] + verts[b * 3 + c]) * 0.5f;
}

__device__ __forceinline__ int find_edge(const uint64_t *__restrict__ ukeys, int E, uint64_t key)
{
    int lo = 0, hi = E - 1;                       // the key is in the table: it was built from these faces
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ukeys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// children of (a, b, c): (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca) at rows 4 f .. 4 f + 3
__global__ void __launch_bounds__(256) child_faces_kernel(int V, int F, int E, const int *__restrict__ faces,
                                                          const uint64_t *__restrict__ ukeys, int *__restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    const int ab = V + find_edge(ukeys, E, edge_key(a, b));
    const int bc = V + find_edge(ukeys, E, edge_key(b, c));
    const int ca = V + find_edge(ukeys, E, edge_key(c, a));
    const int ch[12] = {a, ab, ca, ab, b, bc, ca, bc, c, ab, bc, ca};
    for (int k = 0; k < 12; k++) out[(size_t)f * 12 + k] = ch[k];
}

__device__ __forceinline__ float norm3(const float v[3]) { return sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
__device__ __forceinline__ void cross3(const float a[3], const float b[3], float o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
// F.normalize: v / max(|v|, 1e-12)
__device__ __forceinline__ void normalize3(float v[3])
{
    const float n = fmaxf(norm3(v), 1e-12f);
    v[0] /= n; v[1] /= n; v[2] /= n;
}

// one thread per vertex: its corners, in ascending corner id, add weight * unit face normal
__global__ void __launch_bounds__(256) vertex_normals_kernel(int V, int N, int weighting, const float *__restrict__ verts,
                                                             const int *__restrict__ faces, const uint64_t *__restrict__ ks,
                                                             float *__restrict__ normals)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const uint64_t first = (uint64_t)(uint32_t)v << 32;
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ks[mid] < first) lo = mid + 1;
        else hi = mid;
    }
    float sum[3] = {0.f, 0.f, 0.f};
    for (int i = lo; i < N && (int)(ks[i] >> 32) == v; i++) {
        const uint32_t id = (uint32_t)(ks[i] & 0xffffffffull);
        const int f = (int)(id / 3u), c = (int)(id % 3u);
        float p[3][3];
        for (int q = 0; q < 3; q++)
            for (int k = 0; k < 3; k++) p[q][k] = verts[(size_t)faces[3 * f + q] * 3 + k];
        const float e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
        const float e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
        float n[3];
        cross3(e1, e2, n);
        const float len = norm3(n);
        float wgt = 1.f;
        if (weighting == SOAR_NORMALS_AREA) {
            wgt = 0.5f * len;
        } else if (weighting == SOAR_NORMALS_ANGLE) {
            // the corner's interior angle, atan2(|u x w|, u . w): well conditioned at every angle
            const int c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            const float u[3] = {p[c1][0] - p[c][0], p[c1][1] - p[c][1], p[c1][2] - p[c][2]};
            const float w[3] = {p[c2][0] - p[c][0], p[c2][1] - p[c][1], p[c2][2] - p[c][2]};
            float x[3];
            cross3(u, w, x);
            wgt = atan2f(norm3(x), u[0] * w[0] + u[1] * w[1] + u[2] * w[2]);
        }
        const float d = fmaxf(len, 1e-12f);
        for (int k = 0; k < 3; k++) sum[k] += wgt * (n[k] / d);
    }
    normalize3(sum);
    for (int k = 0; k < 3; k++) normals[(size_t)v * 3 + k] = sum[k];
}

__global__ void __launch_bounds__(256) vertex_frames_kernel(int P, const float *__restrict__ normals, const float *__restrict__ rand_dir,
                                                            float *__restrict__ quats)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const float uz[3] = {normals[(size_t)p * 3], normals[(size_t)p * 3 + 1], normals[(size_t)p * 3 + 2]};
    const float rd[3] = {rand_dir[(size_t)p * 3], rand_dir[(size_t)p * 3 + 1], rand_dir[(size_t)p * 3 + 2]};
    float ux[3], uy[3];
    cross3(uz, rd, ux);
    normalize3(ux);
    cross3(uz, ux, uy);
    normalize3(uy);
    const float m[9] = {ux[0], uy[0], uz[0], ux[1], uy[1], uz[1], ux[2], uy[2], uz[2]};      // columns are the axes
    float cand[4], a_best, x_best;
    mat_to_quat_candidates(m, cand, a_best, x_best);
    const float dn = 2.0f * fmaxf(a_best, 0.1f);
    float o[4] = {cand[0] / dn, cand[1] / dn, cand[2] / dn, cand[3] / dn};
    if (o[0] < 0.f) { o[0] = -o[0]; o[1] = -o[1]; o[2] = -o[2]; o[3] = -o[3]; }
    const float nrm = fmaxf(sqrtf(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]), 1e-12f);
    for (int k = 0; k < 4; k++) quats[(size_t)p * 4 + k] = o[k] / nrm;
}

int mesh_workspace_ok(const char *what, int32_t F, const void *workspace, size_t workspace_bytes, MeshBuf &b)
{
    const size_t need = carve_mesh(b, const_cast<void *>(workspace), (size_t)F);
    return workspace_ok(what, workspace, workspace_bytes, need, "soar_mesh_workspace_bytes") ? 0 : 1;
}

constexpr int32_t MAX_FACES = 0x7fffffff / 12;      // 12 F ints of child faces and 3 F corner ids stay in int32

}  // namespace

}  // namespace soar

using namespace soar;

extern "C" int soar_smplx_vertices(int32_t B, int32_t V, int32_t J, int32_t NB, const float *betas, int32_t betas_batch,
                                   const float *v_template, const float *shapedirs, const float *posedirs, const float *lbs_weights,
                                   const float *full_pose, const float *joint_mats, const float *transl, float *out, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (B < 0 || V < 0 || J < 2 || J > VT_MAX_J || NB < 0 || (betas_batch != 1 && betas_batch != B) || B > 65535 * VT_FRAMES
        || (int64_t)V * 3 * (J - 1) * 9 < 0) {
        set_error("soar_smplx_vertices: need B, V >= 0, 2 <= J <= %d, NB >= 0, betas_batch in {1, B}, B <= %d (B=%d V=%d J=%d NB=%d "
                  "betas_batch=%d)", VT_MAX_J, 65535 * VT_FRAMES, B, V, J, NB, betas_batch);
        return 1;
    }
    if ((NB > 0 && (!betas || !shapedirs)) || !v_template || !posedirs || !lbs_weights || !full_pose || !joint_mats || !out) {
        set_error("soar_smplx_vertices: NULL argument");
        return 1;
    }
    if (B == 0 || V == 0) return 0;
    const VertArgs a = {B, V, J, NB, betas_batch, betas, v_template, shapedirs, posedirs, lbs_weights, full_pose, joint_mats, transl, out};
    const dim3 grid((V + VT_VERTS - 1) / VT_VERTS, (B + VT_FRAMES - 1) / VT_FRAMES);
    hipLaunchKernelGGL(smplx_vertices_kernel, grid, dim3(VT_THREADS), 0, stream, a);
    SOAR_LAUNCH_OK("smplx_vertices", stream, 0);
    return 0;
}

extern "C" int soar_mesh_workspace_bytes(int32_t F, size_t *bytes)
{
    if (!bytes || F < 0 || F > MAX_FACES) {
        set_error("soar_mesh_workspace_bytes: need 0 <= F <= %d and a result pointer (F=%d)", MAX_FACES, F);
        return 1;
    }
    MeshBuf b;
    *bytes = carve_mesh(b, nullptr, (size_t)F);
    return 0;
}

static int mesh_args_ok(const char *what, int32_t V, int32_t F, const void *verts_or_null, bool need_verts, const int32_t *faces)
{
    if (V < 0 || F < 0 || F > MAX_FACES) { set_error("%s: need V >= 0 and 0 <= F <= %d (V=%d F=%d)", what, MAX_FACES, V, F); return 1; }
    if ((need_verts && !verts_or_null) || !faces) { set_error("%s: NULL argument", what); return 1; }
    if (F > 0 && V == 0) { set_error("%s: %d faces name a vertex outside [0, 0)", what, F); return 1; }
    return 0;
}

extern "C" int soar_mesh_subdivide_edges(int32_t V, int32_t F, const int32_t *faces, void *workspace, size_t workspace_bytes,
                                         int64_t *edges_host, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (mesh_args_ok("soar_mesh_subdivide_edges", V, F, nullptr, false, faces)) return 1;
    if (!edges_host) { set_error("soar_mesh_subdivide_edges: NULL edges_host"); return 1; }
    MeshBuf b;
    if (mesh_workspace_ok("soar_mesh_subdivide_edges", F, workspace, workspace_bytes, b)) return 1;
    *edges_host = 0;
    if (F == 0) return 0;
    const int N = 3 * F;
    const dim3 gf((F + 255) / 256), gn((N + 255) / 256), blk(256);
    SOAR_HIP_OK(hipMemsetAsync(b.totals, 0, 8, stream));
    hipLaunchKernelGGL(edge_keys_kernel, gf, blk, 0, stream, V, F, faces, b.keys, b.totals);
    SOAR_LAUNCH_OK("edge_keys", stream, 0);
    SOAR_HIP_OK(sort_keys(b.sort_temp, b.sort_bytes, b.keys, b.keys_sorted, (size_t)N, 64u, stream));
    hipLaunchKernelGGL(head_kernel, gn, blk, 0, stream, N, b.keys_sorted, b.head);
    SOAR_HIP_OK(exclusive_scan_sum(b.scan_temp, b.scan_bytes, b.head, b.uid, (size_t)N, stream));
    hipLaunchKernelGGL(compact_kernel, gn, blk, 0, stream, N, b.keys_sorted, b.head, b.uid, b.ukeys, b.totals);
    SOAR_LAUNCH_OK("edge_compact", stream, 0);
    uint32_t tot[2] = {0, 0};
    SOAR_HIP_OK(hipMemcpyAsync(tot, b.totals, 8, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    if (tot[1]) { set_error("soar_mesh_subdivide_edges: a face names a vertex outside [0, %d)", V); return 1; }
    if ((int64_t)V + tot[0] > 0x7fffffff) { set_error("soar_mesh_subdivide_edges: %d + %u vertices: more than int32 ids can hold", V, tot[0]); return 1; }
    *edges_host = tot[0];
    return 0;
}

extern "C" int soar_mesh_subdivide(int32_t V, int32_t F, int64_t E, const float *verts, const int32_t *faces, const void *workspace,
                                   size_t workspace_bytes, float *verts_out, int32_t *faces_out, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (mesh_args_ok("soar_mesh_subdivide", V, F, verts, true, faces)) return 1;
    if (E < 0 || E > 3 * (int64_t)F || (int64_t)V + E > 0x7fffffff) {
        set_error("soar_mesh_subdivide: E=%lld is not an edge count of %d faces (soar_mesh_subdivide_edges)", (long long)E, F);
        return 1;
    }
    if (!verts_out || !faces_out) { set_error("soar_mesh_subdivide: NULL verts_out / faces_out"); return 1; }
    MeshBuf b;
    if (mesh_workspace_ok("soar_mesh_subdivide", F, workspace, workspace_bytes, b)) return 1;
    if (V > 0) SOAR_HIP_OK(hipMemcpyAsync(verts_out, verts, (size_t)V * 12, hipMemcpyDeviceToDevice, stream));
    if (F == 0 || E == 0) return 0;
    hipLaunchKernelGGL(midpoints_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, V, (int)E, verts, b.ukeys, verts_out);
    hipLaunchKernelGGL(child_faces_kernel, dim3((F + 255) / 256), dim3(256), 0, stream, V, F, (int)E, faces, b.ukeys, faces_out);
    SOAR_LAUNCH_OK("mesh_subdivide", stream, 0);
    return 0;
}

extern "C" int soar_mesh_vertex_normals(int32_t V, int32_t F, const float *verts, const int32_t *faces, int32_t weighting,
                                        void *workspace, size_t workspace_bytes, float *normals, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (mesh_args_ok("soar_mesh_vertex_normals", V, F, verts, true, faces)) return 1;
    if (weighting != SOAR_NORMALS_ANGLE && weighting != SOAR_NORMALS_AREA && weighting != SOAR_NORMALS_UNIFORM) {
        set_error("soar_mesh_vertex_normals: weighting %d is none of SOAR_NORMALS_ANGLE / _AREA / _UNIFORM", weighting);
        return 1;
    }
    if (!normals) { set_error("soar_mesh_vertex_normals: NULL normals"); return 1; }
    MeshBuf b;
    if (mesh_workspace_ok("soar_mesh_vertex_normals", F, workspace, workspace_bytes, b)) return 1;
    if (V == 0) return 0;
    const int N = 3 * F;
    if (F > 0) {
        SOAR_HIP_OK(hipMemsetAsync(b.totals, 0, 8, stream));
        hipLaunchKernelGGL(corner_keys_kernel, dim3((F + 255) / 256), dim3(256), 0, stream, V, F, faces, b.keys, b.totals);
        SOAR_LAUNCH_OK("corner_keys", stream, 0);
        SOAR_HIP_OK(sort_keys(b.sort_temp, b.sort_bytes, b.keys, b.keys_sorted, (size_t)N, 64u, stream));
        // the gather reads vertices by these indices: nothing is gathered before they are known to be in range
        uint32_t tot[2] = {0, 0};
        SOAR_HIP_OK(hipMemcpyAsync(tot, b.totals, 8, hipMemcpyDeviceToHost, stream));
        SOAR_HIP_OK(hipStreamSynchronize(stream));
        if (tot[1]) { set_error("soar_mesh_vertex_normals: a face names a vertex outside [0, %d)", V); return 1; }
    }
    hipLaunchKernelGGL(vertex_normals_kernel, dim3((V + 255) / 256), dim3(256), 0, stream, V, N, weighting, verts, faces, b.keys_sorted, normals);
    SOAR_LAUNCH_OK("vertex_normals", stream, 0);
    return 0;
}

extern "C" int soar_mesh_vertex_frames(int32_t P, const float *normals, const float *rand_dir, float *quats, void *stream_)
{
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (P < 0) { set_error("soar_mesh_vertex_frames: need P >= 0 (P=%d)", P); return 1; }
    if (!normals || !rand_dir || !quats) { set_error("soar_mesh_vertex_frames: NULL argument"); return 1; }
    if (P == 0) return 0;
    hipLaunchKernelGGL(vertex_frames_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, normals, rand_dir, quats);
    SOAR_LAUNCH_OK("vertex_frames", stream, 0);
    return 0;
}
