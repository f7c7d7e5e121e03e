// mesh_common.h -- what the mesh-export files (mesh.hip, mesh_simplify.hip, mesh_attr.hip, mesh_holes.hip, mesh_texture.hip and the
// subdivision / normals half of body.hip) share: a few device helpers and the compaction of a mesh under keep flags.  It brings
// along the workspace carver and check (workspace.h) and the rocPRIM wrappers (scan_sort.h), which every one of these files uses.
//
// The kernels here and compact_mesh are templates on a parameter that never varies: hipcc emits every __global__ function a file
// defines, used or not, and instantiates rocPRIM's kernels behind every function it parses.  As templates they, and the uint32 scan
// behind compact_mesh, exist only in the files that use them.
#pragma once

#include "scan_sort.h"
#include "workspace.h"

namespace soar {

namespace {

// ---- device helpers ----------------------------------------------------------------------------------------------------------

// the three corners of face f; true when all of them are in [0, V)
__device__ __forceinline__ bool face_corners(int V, const int32_t *__restrict__ faces, int f, int &a, int &b, int &c)
{
    a = faces[(size_t)f * 3];
    b = faces[(size_t)f * 3 + 1];
    c = faces[(size_t)f * 3 + 2];
    return a >= 0 && a < V && b >= 0 && b < V && c >= 0 && c < V;
}

// floats as ints whose signed order is the floats' order (a NaN lies beyond the infinity of its sign)
__host__ __device__ __forceinline__ int ford(float f)
{
    int i;
    __builtin_memcpy(&i, &f, 4);
    return i >= 0 ? i : i ^ 0x7fffffff;
}

__host__ __device__ __forceinline__ float fdec(int i)
{
    i = i >= 0 ? i : i ^ 0x7fffffff;
    float f;
    __builtin_memcpy(&f, &i, 4);
    return f;
}

// over the 64 lanes of a wavefront; every lane gets the result
__device__ __forceinline__ int wave_max_i(int x)
{
    for (int m = 32; m >= 1; m >>= 1) x = max(x, __shfl_xor(x, m));
    return x;
}

__device__ __forceinline__ int wave_min_i(int x)
{
    for (int m = 32; m >= 1; m >>= 1) x = min(x, __shfl_xor(x, m));
    return x;
}

__device__ __forceinline__ int wave_sum_i(int x)
{
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

template <int = 0> __global__ void __launch_bounds__(256) copy_floats_kernel(size_t n, const float *__restrict__ src, float *__restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

// ---- compaction of a mesh under keep flags -------------------------------------------------------------------------------------
// The caller's own kernels write vkeep / fkeep (a kept face has its three corners in range and kept) and raise totals[2] for every
// face that names a vertex outside [0, V); compact_mesh then keeps the flagged vertices and faces in input order.

struct CompactBuf {
    uint32_t *vkeep, *voff;     // [V] keep flag, exclusive scan = output vertex id
    uint32_t *fkeep, *foff;     // [max(F, 1)] the same per face
    uint32_t *totals;           // [3] kept vertices, kept faces, faces naming a vertex outside [0, V)
    void *scan_temp;
    size_t scan_bytes;
};

inline void carve_compact(Carver &c, CompactBuf &b, size_t V, size_t F, size_t scan_bytes)
{
    b.vkeep = c.take<uint32_t>(V);
    b.voff = c.take<uint32_t>(V);
    b.fkeep = c.take<uint32_t>(F > 0 ? F : 1);
    b.foff = c.take<uint32_t>(F > 0 ? F : 1);
    b.totals = c.take<uint32_t>(3);
    b.scan_bytes = scan_bytes;
    b.scan_temp = c.take<char>(scan_bytes);
}

template <int = 0> __global__ void compact_totals_kernel(int V, int F, CompactBuf b)
{
    b.totals[0] = b.voff[V - 1] + b.vkeep[V - 1];
    b.totals[1] = F > 0 ? b.foff[F - 1] + b.fkeep[F - 1] : 0u;
}

// one grid over max(V, F); keep_out[new] = old when given
template <int = 0>
__global__ void __launch_bounds__(256) compact_write_kernel(int V, int F, const float *__restrict__ verts, const int32_t *__restrict__ faces,
                                                            CompactBuf b, float *__restrict__ verts_out, int32_t *__restrict__ faces_out,
                                                            int32_t *__restrict__ keep_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < V && b.vkeep[i]) {
        const size_t o = b.voff[i];
        for (int k = 0; k < 3; k++) verts_out[o * 3 + k] = verts[(size_t)i * 3 + k];
        if (keep_out) keep_out[o] = i;
    }
    if (i < F && b.fkeep[i]) {
        const size_t o = b.foff[i];
        for (int k = 0; k < 3; k++) faces_out[o * 3 + k] = (int32_t)b.voff[faces[(size_t)i * 3 + k]];
    }
}

// V >= 1, F >= 0.  One read-back (a stream synchronisation): the totals; counts_host = kept vertices, kept faces
template <int = 0>
inline int compact_mesh(const char *what, int32_t V, int32_t F, const float *verts, const int32_t *faces, const CompactBuf &b,
                        float *verts_out, int32_t *faces_out, int32_t *keep_out, int64_t *counts_host, hipStream_t stream)
{
    SOAR_HIP_OK(exclusive_scan_sum(b.scan_temp, b.scan_bytes, b.vkeep, b.voff, (size_t)V, stream));
    if (F > 0) SOAR_HIP_OK(exclusive_scan_sum(b.scan_temp, b.scan_bytes, b.fkeep, b.foff, (size_t)F, stream));
    hipLaunchKernelGGL(compact_totals_kernel<>, dim3(1), dim3(1), 0, stream, V, F, b);
    hipLaunchKernelGGL(compact_write_kernel<>, dim3(((V > F ? V : F) + 255) / 256), dim3(256), 0, stream, V, F, verts, faces, b, verts_out,
                       faces_out, keep_out);
    SOAR_LAUNCH_OK(what, stream, 0);
    uint32_t tot[3] = {0, 0, 0};
    SOAR_HIP_OK(hipMemcpyAsync(tot, b.totals, 12, hipMemcpyDeviceToHost, stream));
    SOAR_HIP_OK(hipStreamSynchronize(stream));
    if (tot[2]) { set_error("%s: %u faces name a vertex outside [0, %d)", what, tot[2], V); return 1; }
    counts_host[0] = tot[0];
    counts_host[1] = tot[1];
    return 0;
}

}  // namespace

}  // namespace soar
