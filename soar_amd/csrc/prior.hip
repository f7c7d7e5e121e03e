// prior.hip -- the SMPL-X normal priors: an indexed triangle mesh drawn as a normal map, from the front and from behind
// (soar_amd/prior.py; include/soar_hip.h).
//
//   prior_vertex_kernel    a thread per (frame, vertex): camera-space position, projection snapped to 1/256 pixel, 1 / z, and the
//                          area-weighted vertex normal (the vertex's faces in ascending (face, corner) order from a CSR table, no
//                          atomics) rotated into camera space
//   prior_box_kernel       a thread per (frame, face): the first and last pixel column and row whose sample the face's snapped
//                          bounding box holds, as four int16 -- an empty box for a face that is skipped (an invalid vertex, zero
//                          area) or that lies between the samples
//   prior_raster_kernel    a workgroup per (pixel tile, frame), both views: the frame's boxes are walked in slabs of one face per
//                          thread, the faces whose box meets the tile are compacted into an LDS ring with ballots (one barrier per
//                          slab), and whenever the ring holds a face per thread the workgroup rasterizes them, a face per lane, into two
//                          LDS z-buffers of 64-bit keys (depth bits above the face index) with atomicMin.  After a barrier every
//                          pixel is shaded from its winning face and stored.  Nothing passes through global memory between the depth
//                          test and the shading, and the minimum of a set does not depend on the order of its updates: the output
//                          does not depend on the order in which faces, waves or workgroups run.
//
// Coverage is exact integer arithmetic on the snapped vertices (int64 edge functions; the guard band of 2^20 pixels keeps them below
// 2^60).  This file is built without FMA contraction: the float32 expressions evaluate as written.
#include "soar_common.h"

namespace soar {

namespace {

#ifndef SOAR_PRIOR_TILE
#define SOAR_PRIOR_TILE 32                     // development builds try other sizes (16 and 64 lose)
#endif
constexpr int PRIOR_TILE = SOAR_PRIOR_TILE;    // pixels per side of a workgroup's tile (2 views x 1024 keys x 8 B = 16 KiB of LDS)
constexpr int PRIOR_THREADS = 256;             // = the slab: one face per thread
constexpr int PRIOR_RING = 4 * PRIOR_THREADS;  // the ring holds less than two slabs when a third is appended (see the walk)
constexpr int PRIOR_SUB = 256;                 // snapped units per pixel
constexpr int32_t PRIOR_INVALID = INT32_MIN;   // snapped x of a vertex behind the camera or past the guard band
constexpr float PRIOR_GUARD = 1048576.f;       // 2^20 pixels
constexpr unsigned long long PRIOR_EMPTY = ~0ull;

struct VertexK {
    const float *verts;            // [N][V][3] at vs (elements)
    int64_t vs[3];
    const float *w2c;              // [4][4], or [N][4][4] (w2c_step = 16)
    const float *Ks;               // [N][3][3]
    const int32_t *faces;          // [F][3]
    const int32_t *csr_off;        // [V + 1]
    const int32_t *csr_corner;     // [3 F]: 3 face + corner, ascending within a vertex
    int32_t *snapped;              // [N][V][2]
    float *inv_z;                  // [N][V]
    float *normals;                // [N][V][3], camera space
    int64_t total;                 // N V
    int V, w2c_step;
};

__device__ __forceinline__ void load_vertex(const VertexK &k, const float *base, int v, float &x, float &y, float &z)
{
    const float *p = base + v * k.vs[1];
    x = p[0]; y = p[k.vs[2]]; z = p[2 * k.vs[2]];
}

__global__ void __launch_bounds__(256) prior_vertex_kernel(VertexK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.total) return;
    const int64_t n = e / k.V;
    const int v = (int)(e - n * k.V);
    const float *base = k.verts + n * k.vs[0];
    const float *M = k.w2c + n * k.w2c_step;
    const float *K = k.Ks + n * 9;
    float x, y, z;
    load_vertex(k, base, v, x, y, z);
    const float px = M[0] * x + M[1] * y + M[2] * z + M[3];
    const float py = M[4] * x + M[5] * y + M[6] * z + M[7];
    const float pz = M[8] * x + M[9] * y + M[10] * z + M[11];
    const float u = K[0] * px / pz + K[2];
    const float w = K[4] * py / pz + K[5];
    const bool ok = pz > 1e-6f && fabsf(u) <= PRIOR_GUARD && fabsf(w) <= PRIOR_GUARD;          // a NaN fails the comparisons
    k.snapped[e * 2 + 0] = ok ? (int32_t)rintf(u * (float)PRIOR_SUB) : PRIOR_INVALID;
    k.snapped[e * 2 + 1] = ok ? (int32_t)rintf(w * (float)PRIOR_SUB) : PRIOR_INVALID;
    k.inv_z[e] = ok ? 1.f / pz : 0.f;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int c = k.csr_off[v]; c < k.csr_off[v + 1]; c++) {
        const int32_t *f = k.faces + (k.csr_corner[c] / 3) * 3;
        float ax, ay, az, bx, by, bz, cx, cy, cz;
        load_vertex(k, base, f[0], ax, ay, az);
        load_vertex(k, base, f[1], bx, by, bz);
        load_vertex(k, base, f[2], cx, cy, cz);
        const float e1x = bx - ax, e1y = by - ay, e1z = bz - az, e2x = cx - ax, e2y = cy - ay, e2z = cz - az;
        sx += e1y * e2z - e1z * e2y;
        sy += e1z * e2x - e1x * e2z;
        sz += e1x * e2y - e1y * e2x;
    }
    const float len = fmaxf(sqrtf(sx * sx + sy * sy + sz * sz), 1e-12f);
    sx /= len; sy /= len; sz /= len;
    float *o = k.normals + e * 3;
    o[0] = M[0] * sx + M[1] * sy + M[2] * sz;
    o[1] = M[4] * sx + M[5] * sy + M[6] * sz;
    o[2] = M[8] * sx + M[9] * sy + M[10] * sz;
}

struct RasterK {
    const int32_t *faces;          // [F][3]
    const int32_t *snapped;        // [N][V][2]
    const float *inv_z;            // [N][V]
    const float *normals;          // [N][V][3]
    const short4 *boxes;           // [N][F]: first / last column, first / last row
    float *prior;                  // [N][2][3][H][W]
    uint8_t *mask;                 // [N][2][H][W]
    int32_t *face;                 // [N][2][H][W]
    int V, F, H, W, tiles_x, opengl;
};

// a face as the rasterizer sees it: snapped vertices with a positive doubled area (vertices 1 and 2 swapped when it was negative)
struct Tri {
    int32_t i0, i1, i2;
    int64_t x0, y0, x1, y1, x2, y2, area;
};

__device__ __forceinline__ bool load_tri(const RasterK &k, const int32_t *snap, int f, Tri &t)
{
    const int32_t *idx = k.faces + (size_t)f * 3;
    t.i0 = idx[0]; t.i1 = idx[1]; t.i2 = idx[2];
    const int2 a = ((const int2 *)snap)[t.i0], b = ((const int2 *)snap)[t.i1], c = ((const int2 *)snap)[t.i2];
    if (a.x == PRIOR_INVALID || b.x == PRIOR_INVALID || c.x == PRIOR_INVALID) return false;
    t.x0 = a.x; t.y0 = a.y; t.x1 = b.x; t.y1 = b.y; t.x2 = c.x; t.y2 = c.y;
    t.area = (t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0);
    if (t.area < 0) {
        const int32_t i = t.i1; t.i1 = t.i2; t.i2 = i;
        int64_t s = t.x1; t.x1 = t.x2; t.x2 = s;
        s = t.y1; t.y1 = t.y2; t.y2 = s;
        t.area = -t.area;
    }
    return t.area != 0;
}

// the edge function of the edge (ax, ay) -> (bx, by) at (px, py): positive on the inner side of a face of positive area
__device__ __forceinline__ int64_t edge_fn(int64_t ax, int64_t ay, int64_t bx, int64_t by, int64_t px, int64_t py)
{
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}
// a sample exactly on an edge belongs to the face when the edge runs towards +y, or along +x: opposite answers for the two directions
__device__ __forceinline__ bool edge_owns(int64_t dx, int64_t dy) { return dy > 0 || (dy == 0 && dx > 0); }
__device__ __forceinline__ bool edge_in(int64_t e, bool owns) { return e > 0 || (e == 0 && owns); }

__device__ __forceinline__ float tri_q(const RasterK &k, const float *iz, const Tri &t, int64_t e0, int64_t e1, int64_t e2, float &w0,
                                       float &w1, float &w2)
{
    const float A = (float)t.area;
    w0 = (float)e0 / A * iz[t.i0];
    w1 = (float)e1 / A * iz[t.i1];
    w2 = (float)e2 / A * iz[t.i2];
    return w0 + w1 + w2;
}

struct BoxK {
    const int32_t *faces;
    const int32_t *snapped;
    short4 *boxes;                 // [N][F]
    int64_t total;                 // N F
    int V, F;
};
__global__ void __launch_bounds__(256) prior_box_kernel(BoxK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.total) return;
    const int64_t n = e / k.F;
    const int f = (int)(e - n * k.F);
    RasterK rk{};
    rk.faces = k.faces;
    Tri tr;
    short4 b = make_short4(32767, -32768, 32767, -32768);                                 // meets no tile
    if (load_tri(rk, k.snapped + (size_t)n * k.V * 2, f, tr)) {
        const int64_t minx = min(tr.x0, min(tr.x1, tr.x2)), maxx = max(tr.x0, max(tr.x1, tr.x2));
        const int64_t miny = min(tr.y0, min(tr.y1, tr.y2)), maxy = max(tr.y0, max(tr.y1, tr.y2));
        // pixel j is sampled at 256 j + 128: the first j with 256 j + 128 >= min, the last with 256 j + 128 <= max (floor division).
        // Clamped to int16: the image has at most 4096 pixels a side, a clamped end stays on its side of it
        const int64_t jx0 = (minx - 128 + 255) >> 8, jx1 = (maxx - 128) >> 8, jy0 = (miny - 128 + 255) >> 8, jy1 = (maxy - 128) >> 8;
        if (jx0 <= jx1 && jy0 <= jy1) {
            auto s16 = [](int64_t v) { return (short)max((int64_t)-32768, min((int64_t)32767, v)); };
            b = make_short4(s16(jx0), s16(jx1), s16(jy0), s16(jy1));
        }
    }
    k.boxes[e] = b;
}

__global__ void __launch_bounds__(PRIOR_THREADS) prior_raster_kernel(RasterK k)
{
    __shared__ unsigned long long zbuf[2][PRIOR_TILE * PRIOR_TILE];
    __shared__ int32_t ring[PRIOR_RING];
    __shared__ int32_t cnt[2][PRIOR_THREADS / WAVE];
    const int t = threadIdx.x, n = blockIdx.y;
    const int ty = blockIdx.x / k.tiles_x, tx = blockIdx.x - ty * k.tiles_x;
    const int px0 = tx * PRIOR_TILE, py0 = ty * PRIOR_TILE;                              // the tile's first pixel
    const int px1 = min(px0 + PRIOR_TILE, k.W) - 1, py1 = min(py0 + PRIOR_TILE, k.H) - 1;  // and its last one inside the image
    const int32_t *snap = k.snapped + (size_t)n * k.V * 2;
    const float *iz = k.inv_z + (size_t)n * k.V;
    for (int i = t; i < PRIOR_TILE * PRIOR_TILE; i += PRIOR_THREADS) { zbuf[0][i] = PRIOR_EMPTY; zbuf[1][i] = PRIOR_EMPTY; }
    __syncthreads();

    // one face of the ring per lane over (bounding box) x (tile)
    auto rasterize = [&](int f) {
        Tri tr;
        if (!load_tri(k, snap, f, tr)) return;
        const int64_t minx = min(tr.x0, min(tr.x1, tr.x2)), maxx = max(tr.x0, max(tr.x1, tr.x2));
        const int64_t miny = min(tr.y0, min(tr.y1, tr.y2)), maxy = max(tr.y0, max(tr.y1, tr.y2));
        // pixel j is sampled at 256 j + 128: the first j with 256 j + 128 >= min, the last with 256 j + 128 <= max (floor division)
        const int jx0 = max(px0, (int)((minx - 128 + 255) >> 8)), jx1 = min(px1, (int)((maxx - 128) >> 8));
        const int jy0 = max(py0, (int)((miny - 128 + 255) >> 8)), jy1 = min(py1, (int)((maxy - 128) >> 8));
        if (jx0 > jx1 || jy0 > jy1) return;
        const bool o0 = edge_owns(tr.x2 - tr.x1, tr.y2 - tr.y1), o1 = edge_owns(tr.x0 - tr.x2, tr.y0 - tr.y2),
                   o2 = edge_owns(tr.x1 - tr.x0, tr.y1 - tr.y0);
        const int64_t sx = (int64_t)PRIOR_SUB * jx0 + 128, sy = (int64_t)PRIOR_SUB * jy0 + 128;
        int64_t r0 = edge_fn(tr.x1, tr.y1, tr.x2, tr.y2, sx, sy), r1 = edge_fn(tr.x2, tr.y2, tr.x0, tr.y0, sx, sy),
                r2 = edge_fn(tr.x0, tr.y0, tr.x1, tr.y1, sx, sy);
        // a step of one pixel along x adds -256 (by - ay), along y +256 (bx - ax)
        const int64_t dx0 = -PRIOR_SUB * (tr.y2 - tr.y1), dx1 = -PRIOR_SUB * (tr.y0 - tr.y2), dx2 = -PRIOR_SUB * (tr.y1 - tr.y0);
        const int64_t dy0 = PRIOR_SUB * (tr.x2 - tr.x1), dy1 = PRIOR_SUB * (tr.x0 - tr.x2), dy2 = PRIOR_SUB * (tr.x1 - tr.x0);
        for (int jy = jy0; jy <= jy1; jy++) {
            int64_t e0 = r0, e1 = r1, e2 = r2;
            for (int jx = jx0; jx <= jx1; jx++) {
                if (edge_in(e0, o0) && edge_in(e1, o1) && edge_in(e2, o2)) {
                    float w0, w1, w2;
                    const uint32_t qb = __float_as_uint(tri_q(k, iz, tr, e0, e1, e2, w0, w1, w2));       // q > 0: its bits order as it does
                    const int p = (jy - py0) * PRIOR_TILE + (jx - px0);
                    atomicMin(&zbuf[0][p], ((unsigned long long)(~qb) << 32) | (uint32_t)f);              // front: the largest q
                    atomicMin(&zbuf[1][p], ((unsigned long long)qb << 32) | (uint32_t)f);                 // rear: the smallest
                }
                e0 += dx0; e1 += dx1; e2 += dx2;
            }
            r0 += dy0; r1 += dy1; r2 += dy2;
        }
    };

    // The walk.  Round r: every wave counts its hits into cnt[r & 1], one barrier, every thread adds up the four counts and the hits
    // go into the ring behind `tail`; then, if the ring held a face per thread BEFORE this round (entries the barrier has made
    // visible), those are rasterized.  head, tail and the decision are the same in every thread without a shared counter.  A wave
    // that runs ahead writes ring entries of round r + 1 only behind barrier r + 1, which every wave reaches after its reads of round
    // r; live entries span less than 3 slabs (below 2 pending, 1 appended), the ring holds 4.
    const short4 *boxes = k.boxes + (size_t)n * k.F;
    const int lane = t & (WAVE - 1), wave = t / WAVE;
    int head = 0, tail = 0;
    for (int s = 0, r = 0; s < k.F; s += PRIOR_THREADS, r ^= 1) {
        const int f = s + t;
        bool hit = false;
        if (f < k.F) {
            const short4 b = boxes[f];
            hit = b.x <= px1 && b.y >= px0 && b.z <= py1 && b.w >= py0;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) cnt[r][wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PRIOR_THREADS / WAVE; w++) {
            const int c = cnt[r][w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (hit) ring[(tail + before + __popcll(m & ((1ull << lane) - 1ull))) & (PRIOR_RING - 1)] = f;
        if (tail - head >= PRIOR_THREADS) {
            rasterize(ring[(head + t) & (PRIOR_RING - 1)]);
            head += PRIOR_THREADS;
        }
        tail += total;
    }
    __syncthreads();
    for (; head < tail; head += PRIOR_THREADS)
        if (head + t < tail) rasterize(ring[(head + t) & (PRIOR_RING - 1)]);
    __syncthreads();

    // resolve: shade every pixel of the tile from its winner
    const size_t hw = (size_t)k.H * k.W;
    const float *nrm = k.normals + (size_t)n * k.V * 3;
    for (int i = t; i < PRIOR_TILE * PRIOR_TILE; i += PRIOR_THREADS) {
        const int jy = py0 + i / PRIOR_TILE, jx = px0 + i % PRIOR_TILE;
        if (jx >= k.W || jy >= k.H) continue;
#pragma unroll
        for (int view = 0; view < 2; view++) {
            const unsigned long long key = zbuf[view][i];
            const size_t pix = ((size_t)n * 2 + view) * hw + (size_t)jy * k.W + jx;
            float *o = k.prior + ((size_t)n * 2 + view) * 3 * hw + (size_t)jy * k.W + jx;
            float nx = 0.f, ny = 0.f, nz = 0.f;
            const bool on = key != PRIOR_EMPTY;
            if (on) {
                const int f = (int)(uint32_t)key;
                Tri tr;
                load_tri(k, snap, f, tr);
                const int64_t sx = (int64_t)PRIOR_SUB * jx + 128, sy = (int64_t)PRIOR_SUB * jy + 128;
                float w0, w1, w2;
                tri_q(k, iz, tr, edge_fn(tr.x1, tr.y1, tr.x2, tr.y2, sx, sy), edge_fn(tr.x2, tr.y2, tr.x0, tr.y0, sx, sy),
                      edge_fn(tr.x0, tr.y0, tr.x1, tr.y1, sx, sy), w0, w1, w2);
                const float *n0 = nrm + (size_t)tr.i0 * 3, *n1 = nrm + (size_t)tr.i1 * 3, *n2 = nrm + (size_t)tr.i2 * 3;
                nx = w0 * n0[0] + w1 * n1[0] + w2 * n2[0];
                ny = w0 * n0[1] + w1 * n1[1] + w2 * n2[1];
                nz = w0 * n0[2] + w1 * n1[2] + w2 * n2[2];
                const float len = fmaxf(sqrtf(nx * nx + ny * ny + nz * nz), 1e-12f);
                nx /= len; ny /= len; nz /= len;
                if (k.opengl) { ny = -ny; nz = -nz; }
                k.face[pix] = f;
            } else {
                k.face[pix] = -1;
            }
            k.mask[pix] = on ? 1 : 0;
            o[0] = nx; o[hw] = ny; o[2 * hw] = nz;
        }
    }
}

bool check_mesh(const char *what, int32_t N, int32_t V, int32_t F)
{
    if (N < 0 || N > 65535) { set_error("%s: N must be 0 .. 65535 (got %d)", what, N); return false; }
    if (V < 1 || V > (1 << 24) || F < 0 || F > (1 << 24)) { set_error("%s: need 1 <= V <= 2^24 and 0 <= F <= 2^24 (V=%d, F=%d)", what, V, F); return false; }
    return true;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_prior_vertex_setup(int32_t N, int32_t V, int32_t F, const float *verts, const int64_t *verts_stride, const float *w2c,
                                       int32_t w2c_per_frame, const float *Ks, const int32_t *faces, const int32_t *csr_offsets,
                                       const int32_t *csr_corners, int32_t *snapped, float *inv_z, float *normals, void *stream_)
{
    const char *what = "soar_prior_vertex_setup";
    if (!check_mesh(what, N, V, F)) return 1;
    if (N == 0) return 0;
    if (!verts || !verts_stride || !w2c || !Ks || !csr_offsets || !snapped || !inv_z || !normals || (F > 0 && (!faces || !csr_corners))) {
        set_error("%s: NULL verts / strides / w2c / Ks / faces / CSR table / outputs", what);
        return 1;
    }
    VertexK k{};
    k.verts = verts; k.w2c = w2c; k.Ks = Ks; k.faces = faces; k.csr_off = csr_offsets; k.csr_corner = csr_corners;
    k.snapped = snapped; k.inv_z = inv_z; k.normals = normals;
    for (int j = 0; j < 3; j++) k.vs[j] = verts_stride[j];
    k.V = V; k.w2c_step = w2c_per_frame ? 16 : 0;
    k.total = (int64_t)N * V;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(prior_vertex_kernel, dim3((unsigned)((k.total + 255) / 256)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("prior_vertex", stream, 0);
    return 0;
}

extern "C" int soar_prior_face_boxes(int32_t N, int32_t V, int32_t F, const int32_t *faces, const int32_t *snapped, int16_t *boxes,
                                     void *stream_)
{
    const char *what = "soar_prior_face_boxes";
    if (!check_mesh(what, N, V, F)) return 1;
    if (N == 0 || F == 0) return 0;
    if (!faces || !snapped || !boxes) { set_error("%s: NULL faces / snapped / boxes", what); return 1; }
    BoxK k{};
    k.faces = faces; k.snapped = snapped; k.boxes = reinterpret_cast<short4 *>(boxes);
    k.V = V; k.F = F;
    k.total = (int64_t)N * F;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(prior_box_kernel, dim3((unsigned)((k.total + 255) / 256)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("prior_box", stream, 0);
    return 0;
}

extern "C" int soar_prior_raster(int32_t N, int32_t V, int32_t F, int32_t H, int32_t W, int32_t opengl, const int32_t *faces,
                                 const int32_t *snapped, const float *inv_z, const float *normals, const int16_t *boxes, float *prior,
                                 uint8_t *mask, int32_t *face, void *stream_)
{
    const char *what = "soar_prior_raster";
    if (!check_mesh(what, N, V, F)) return 1;
    if (H < 1 || W < 1 || H > 4096 || W > 4096) { set_error("%s: H and W must be 1 .. 4096 (got H=%d, W=%d)", what, H, W); return 1; }
    if (N == 0) return 0;
    if (!snapped || !inv_z || !normals || !prior || !mask || !face || (F > 0 && (!faces || !boxes))) {
        set_error("%s: NULL faces / snapped / inv_z / normals / boxes / outputs", what);
        return 1;
    }
    RasterK k{};
    k.faces = faces; k.snapped = snapped; k.inv_z = inv_z; k.normals = normals; k.boxes = reinterpret_cast<const short4 *>(boxes); k.prior = prior; k.mask = mask; k.face = face;
    k.V = V; k.F = F; k.H = H; k.W = W; k.opengl = opengl ? 1 : 0;
    k.tiles_x = (W + PRIOR_TILE - 1) / PRIOR_TILE;
    const int tiles_y = (H + PRIOR_TILE - 1) / PRIOR_TILE;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(prior_raster_kernel, dim3((unsigned)(k.tiles_x * tiles_y), (unsigned)N), dim3(PRIOR_THREADS), 0, stream, k);
    SOAR_LAUNCH_OK("prior_raster", stream, 0);
    return 0;
}
