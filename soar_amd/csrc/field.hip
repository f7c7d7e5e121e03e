// field.hip -- the surfels' attribute field (soar_amd/field.py): the reference's HashMLPSDFField (TS/geometry/sdf_fields.py:41-219)
// as nerfstudio's torch HashEncoding / MLP compute it, two hash encodings and five two-layer heads (include/soar_hip.h,
// DESIGN.md "Attribute field").
//
//   field_forward_kernel   one thread per point: both encodings (16 levels x 8 corners x 2 tables, gathers of 8 B), stored for
//                          the backward, then the five heads with every weight in LDS (broadcast reads)
//   field_head_bwd_kernel  grid (blocks, head): a wave takes 64 points at a time, recomputes the head's hidden layer, forms
//                          dL/dy, dL/dh and dL/de (stored per head), and sums the weight / bias gradients of its points in
//                          double registers (thread = hidden unit, the points' rows in LDS); one partial row per block, no atomics
//   field_reduce_kernel    the partial rows summed in double in a fixed order (four slices, then the slices in order)
//   field_dz_kernel        dL/dz = W1[:, 32:34]^T . (sum over points of dL/dh of the offsets head)
//   field_scatter_kernel   one thread per point: dL/de of the heads summed in a fixed order, scattered into the table
//                          gradients with float atomics (runs of equal rows in a wave summed first: wave_add; tables of at
//                          most 32 rows per level summed per block in LDS first), and dL/dxyz through the offsets o
//
// The table gradients are the only atomics: their last bits depend on arrival order.  Everything else is bit-identical
// from run to run.  No host synchronisation, no allocation.
#include "workspace.h"

namespace soar {

namespace {

constexpr int LEVELS = SOAR_FIELD_LEVELS;   // 16 levels x 2 features = 32 encoded values
constexpr int ENC = 2 * LEVELS;
constexpr int HID = SOAR_FIELD_HIDDEN;
constexpr int NHEAD = 5;
constexpr int HEAD_OFFSETS = 3;
constexpr int HEAD_QUATS = 2;
constexpr int CHUNK = 64;                   // points per wave step of the head backward
constexpr int CHUNKS_PER_BLOCK = 2;
constexpr int MAX_N = 1 << 26;
// the scatter sums runs of equal rows inside a wave before its atomics (wave_add); 0 = one atomic per lane, corner and feature
// (the A/B of DESIGN.md 9c: scripts/variant.py NAME field.hip -DSOAR_FIELD_WAVE_COMBINE=0)
#ifndef SOAR_FIELD_WAVE_COMBINE
#define SOAR_FIELD_WAVE_COMBINE 1
#endif

__host__ __device__ constexpr int head_in(int k) { return k == HEAD_OFFSETS ? ENC + 2 : ENC; }
__host__ __device__ constexpr int head_out(int k) { return k == 0 ? 3 : k == 1 ? 1 : k == 2 ? 4 : k == 3 ? 3 : 1; }
// LDS row stride of a head's first layer: the input padded to a multiple of 4 (float4 reads)
__host__ __device__ constexpr int head_stride(int k) { return (head_in(k) + 3) & ~3; }
__host__ __device__ constexpr int head_lds_floats(int k) { return (HID * head_stride(k) + HID + head_out(k) * HID + head_out(k) + 3) & ~3; }
__host__ __device__ constexpr int head_lds_offset(int k) { return k == 0 ? 0 : head_lds_offset(k - 1) + head_lds_floats(k - 1); }
constexpr int ALL_HEADS_LDS = head_lds_offset(NHEAD);
constexpr int MAX_HEAD_LDS = head_lds_floats(HEAD_OFFSETS);
__host__ __device__ constexpr int head_floats(int k) { return SOAR_FIELD_HEAD_FLOATS(head_in(k), head_out(k)); }

struct FieldK {
    int N, T, normalized;
    float res[LEVELS];
    const float *xyz, *aabb, *table, *qtable, *z;
    SoarFieldHead head[NHEAD];
    float *enc, *qenc;
    float *out[NHEAD];
    const float *g_out[NHEAD];
    float *d_table, *d_qtable;
    float *d_head[NHEAD];
    float *d_xyz, *d_z;
    float *de;                   // workspace: [NHEAD][N][32] dL/de of each head
    float *partial;              // workspace: per head [G][head_floats(k)]
    int G;                       // blocks of the head backward = partial rows per head
    int need_w[NHEAD];           // the head's weight gradients are wanted (d_head[k], or dz for the offsets head)
};

// the head's weights into LDS, laid out [64][stride] w1, b1 [64], w2 [out][64], b2 [out]
template <int K>
__device__ void load_head(const SoarFieldHead &h, float *W)
{
    constexpr int IN = head_in(K), S = head_stride(K), OUT = head_out(K);
    for (int e = threadIdx.x; e < HID * S; e += blockDim.x) {
        const int i = e / S, j = e - i * S;
        W[e] = j < IN ? h.w1[i * IN + j] : 0.f;
    }
    for (int e = threadIdx.x; e < HID; e += blockDim.x) W[HID * S + e] = h.b1[e];
    for (int e = threadIdx.x; e < OUT * HID; e += blockDim.x) W[HID * S + HID + e] = h.w2[e];
    for (int e = threadIdx.x; e < OUT; e += blockDim.x) W[HID * S + HID + OUT * HID + e] = h.b2[e];
}

// normalised position; sel = the reference's selector (1 when normalized)
__device__ inline void normalise(const FieldK &a, int n, float p[3], float inv_ext[3], bool &sel)
{
    const float x[3] = {a.xyz[3 * n], a.xyz[3 * n + 1], a.xyz[3 * n + 2]};
    if (a.normalized) {
        sel = true;
        for (int d = 0; d < 3; d++) { p[d] = x[d]; inv_ext[d] = 1.f; }
        return;
    }
    sel = true;
    for (int d = 0; d < 3; d++) {
        const float lo = a.aabb[d], ext = a.aabb[3 + d] - lo;
        p[d] = (x[d] - lo) / ext;
        inv_ext[d] = 1.f / ext;
        sel = sel && p[d] > 0.f && p[d] < 1.f;
    }
    if (!sel)
        for (int d = 0; d < 3; d++) p[d] = 0.f;
}

struct Cell {
    int c[3], f[3];
    float o[3];
};

__device__ inline Cell cell_of(const float p[3], float s)
{
    // q is rounded before o = q - f, as torch rounds it: fma(p, s, -f) would keep the product's low bits, half an ulp of q
    // (6e-5 at level 15) in o
#pragma clang fp contract(off)
    Cell r;
    for (int d = 0; d < 3; d++) {
        const float q = p[d] * s;
        r.c[d] = (int)ceilf(q);
        r.f[d] = (int)floorf(q);
        r.o[d] = q - (float)r.f[d];
    }
    return r;
}

// corner bits: x = bit 0, y = bit 1, z = bit 2; a set bit takes the ceiling on that axis
__device__ inline uint32_t corner_slot(const Cell &cl, int k, uint32_t mask)
{
    const uint32_t x = (uint32_t)((k & 1) ? cl.c[0] : cl.f[0]);
    const uint32_t y = (uint32_t)((k & 2) ? cl.c[1] : cl.f[1]);
    const uint32_t z = (uint32_t)((k & 4) ? cl.c[2] : cl.f[2]);
    return (x ^ (y * 2654435761u) ^ (z * 805459861u)) & mask;
}

__device__ inline float lerp_w(int bit, float o) { return bit ? o : 1.f - o; }

// first layer + ReLU + second layer of one head for one point; x padded to the head's stride
template <int K>
__device__ inline void head_eval(const float *W, const float *x, float *y)
{
    constexpr int S = head_stride(K), OUT = head_out(K);
    const float *b1 = W + HID * S, *w2 = b1 + HID, *b2 = w2 + OUT * HID;
    for (int o = 0; o < OUT; o++) y[o] = b2[o];
    for (int i = 0; i < HID; i++) {
        const float4 *r = reinterpret_cast<const float4 *>(W + i * S);
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < S / 4; j++) {
            const float4 w = r[j];
            acc += w.x * x[4 * j] + w.y * x[4 * j + 1] + w.z * x[4 * j + 2] + w.w * x[4 * j + 3];
        }
        const float h = fmaxf(acc + b1[i], 0.f);
#pragma unroll
        for (int o = 0; o < OUT; o++) y[o] += w2[o * HID + i] * h;
    }
}

__device__ inline float field_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

template <int K>
__device__ inline void head_finish(const float *y, float *out, int n)
{
    constexpr int OUT = head_out(K);
    if (K == 0 || K == 4) {
        for (int o = 0; o < OUT; o++) out[n * OUT + o] = field_sigmoid(y[o]);
    } else if (K == 1) {
        out[n] = field_sigmoid(y[0]) * 2e-2f;
    } else if (K == 2) {
        const float nrm = fmaxf(sqrtf(y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3]), 1e-12f);
        for (int o = 0; o < 4; o++) out[n * 4 + o] = y[o] / nrm;
    } else {
        for (int o = 0; o < OUT; o++) out[n * OUT + o] = y[o];
    }
}

template <int K>
__device__ inline void head_forward(const FieldK &a, const float *Wall, const float *e, float z0, float z1, int n)
{
    constexpr int S = head_stride(K);
    float x[S];
#pragma unroll
    for (int j = 0; j < ENC; j++) x[j] = e[j];
    if constexpr (S > ENC) {
        x[ENC] = z0;
        x[ENC + 1] = z1;
#pragma unroll
        for (int j = ENC + 2; j < S; j++) x[j] = 0.f;
    }
    float y[4];
    constexpr int OFF = head_lds_offset(K);
    head_eval<K>(Wall + OFF, x, y);
    head_finish<K>(y, a.out[K], n);
}

__global__ void __launch_bounds__(128) field_forward_kernel(FieldK a)
{
    __shared__ __attribute__((aligned(16))) float W[ALL_HEADS_LDS];
    constexpr int OFF[NHEAD] = {head_lds_offset(0), head_lds_offset(1), head_lds_offset(2), head_lds_offset(3), head_lds_offset(4)};
    load_head<0>(a.head[0], W + OFF[0]);
    load_head<1>(a.head[1], W + OFF[1]);
    load_head<2>(a.head[2], W + OFF[2]);
    load_head<3>(a.head[3], W + OFF[3]);
    load_head<4>(a.head[4], W + OFF[4]);
    __syncthreads();
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    float p[3], inv_ext[3];
    bool sel;
    normalise(a, n, p, inv_ext, sel);
    const uint32_t mask = (uint32_t)a.T - 1u;
    float e[ENC], qe[ENC];
    const float2 *t2 = reinterpret_cast<const float2 *>(a.table), *q2 = reinterpret_cast<const float2 *>(a.qtable);
#pragma unroll 2
    for (int l = 0; l < LEVELS; l++) {
        const Cell cl = cell_of(p, a.res[l]);
        const size_t base = (size_t)l * a.T;
        float2 tv[8], qv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const size_t r = base + corner_slot(cl, k, mask);
            tv[k] = t2[r];
            qv[k] = q2[r];
        }
        // nerfstudio's interpolation order: along x (f_03, f_12, f_47, f_56), then y, then z
        float ex[4][2], qx[4][2];
#pragma unroll
        for (int yz = 0; yz < 4; yz++) {
            const int kc = 1 | (yz << 1), kf = yz << 1;
            ex[yz][0] = tv[kc].x * cl.o[0] + tv[kf].x * (1.f - cl.o[0]);
            ex[yz][1] = tv[kc].y * cl.o[0] + tv[kf].y * (1.f - cl.o[0]);
            qx[yz][0] = qv[kc].x * cl.o[0] + qv[kf].x * (1.f - cl.o[0]);
            qx[yz][1] = qv[kc].y * cl.o[0] + qv[kf].y * (1.f - cl.o[0]);
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const float ez1 = ex[3][j] * cl.o[1] + ex[2][j] * (1.f - cl.o[1]);    // z = ceil: y ceil (yz = 3), y floor (2)
            const float ez0 = ex[1][j] * cl.o[1] + ex[0][j] * (1.f - cl.o[1]);
            e[2 * l + j] = ez1 * cl.o[2] + ez0 * (1.f - cl.o[2]);
            const float qz1 = qx[3][j] * cl.o[1] + qx[2][j] * (1.f - cl.o[1]);
            const float qz0 = qx[1][j] * cl.o[1] + qx[0][j] * (1.f - cl.o[1]);
            qe[2 * l + j] = qz1 * cl.o[2] + qz0 * (1.f - cl.o[2]);
        }
    }
    float4 *eo = reinterpret_cast<float4 *>(a.enc + (size_t)n * ENC), *qo = reinterpret_cast<float4 *>(a.qenc + (size_t)n * ENC);
#pragma unroll
    for (int j = 0; j < ENC / 4; j++) {
        eo[j] = make_float4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
        qo[j] = make_float4(qe[4 * j], qe[4 * j + 1], qe[4 * j + 2], qe[4 * j + 3]);
    }
    const float z0 = a.z ? a.z[0] : 0.f, z1 = a.z ? a.z[1] : 0.f;
    head_forward<0>(a, W, e, z0, z1, n);
    head_forward<1>(a, W, e, z0, z1, n);
    head_forward<2>(a, W, qe, z0, z1, n);
    head_forward<3>(a, W, e, z0, z1, n);
    head_forward<4>(a, W, e, z0, z1, n);
}

// dL/dy (pre-activation) of head K from the upstream gradient g and the second layer's output y
template <int K>
__device__ inline void head_dy(const float *y, const float *g, float *dy)
{
    if (K == 0 || K == 4) {
        for (int o = 0; o < head_out(K); o++) {
            const float s = field_sigmoid(y[o]);
            dy[o] = g[o] * (s * (1.f - s));
        }
    } else if (K == 1) {
        const float s = field_sigmoid(y[0]);
        dy[0] = g[0] * 2e-2f * (s * (1.f - s));
    } else if (K == 2) {
        // F.normalize: x / max(|x|, eps); below eps the divisor is constant
        const float nrm = sqrtf(y[0] * y[0] + y[1] * y[1] + y[2] * y[2] + y[3] * y[3]);
        if (nrm > 1e-12f) {
            const float dot = (g[0] * y[0] + g[1] * y[1] + g[2] * y[2] + g[3] * y[3]) / (nrm * nrm);
            for (int o = 0; o < 4; o++) dy[o] = (g[o] - y[o] * dot) / nrm;
        } else {
            for (int o = 0; o < 4; o++) dy[o] = g[o] / 1e-12f;
        }
    } else {
        for (int o = 0; o < head_out(K); o++) dy[o] = g[o];
    }
}

constexpr int HROW = HID + 1;               // LDS row of H / DH: 65 floats, so that a wave writing its own rows hits 64 banks
constexpr int XROW = ENC + 4;               // 36: the widest input, padded

struct BwdLds {
    float W[MAX_HEAD_LDS];
    float Hs[CHUNK * HROW], DHs[CHUNK * HROW], Xs[CHUNK * XROW], DYs[CHUNK * 4];
};

template <int K>
__device__ void head_backward(const FieldK &a, BwdLds &L)
{
    constexpr int IN = head_in(K), S = head_stride(K), OUT = head_out(K);
    float *W = L.W, *Hs = L.Hs, *DHs = L.DHs, *Xs = L.Xs, *DYs = L.DYs;
    load_head<K>(a.head[K], W);
    __syncthreads();
    const float *b1 = W + HID * S, *w2 = b1 + HID;
    const int lane = threadIdx.x;
    const bool need_w = a.need_w[K] != 0;
    const float *g = a.g_out[K];
    const float *src = K == HEAD_QUATS ? a.qenc : a.enc;
    float *de = a.de + (size_t)K * a.N * ENC;
    const float z0 = a.z ? a.z[0] : 0.f, z1 = a.z ? a.z[1] : 0.f;
    // the block's weight-gradient sums in double: the products of two floats are exact there, and the sums of its points do
    // not drift with their order
    double acc1[IN], accb1 = 0.0, acc2[OUT], accb2 = 0.0;
#pragma unroll
    for (int j = 0; j < IN; j++) acc1[j] = 0.0;
#pragma unroll
    for (int o = 0; o < OUT; o++) acc2[o] = 0.0;
    const int chunks = (a.N + CHUNK - 1) / CHUNK;
    const int c0 = blockIdx.x * CHUNKS_PER_BLOCK, c1 = min(chunks, c0 + CHUNKS_PER_BLOCK);
    for (int c = c0; c < c1; c++) {
        const int n = c * CHUNK + lane;
        float *X = Xs + lane * XROW, *Hr = Hs + lane * HROW, *DHr = DHs + lane * HROW;
        if (n < a.N) {
            float x[S];
            const float4 *s4 = reinterpret_cast<const float4 *>(src + (size_t)n * ENC);
#pragma unroll
            for (int j = 0; j < ENC / 4; j++) {
                const float4 v = s4[j];
                x[4 * j] = v.x; x[4 * j + 1] = v.y; x[4 * j + 2] = v.z; x[4 * j + 3] = v.w;
            }
            if constexpr (S > ENC) {
                x[ENC] = z0;
                x[ENC + 1] = z1;
#pragma unroll
                for (int j = ENC + 2; j < S; j++) x[j] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < S; j++) X[j] = x[j];
            float y[4], gg[4], dy[4];
            for (int o = 0; o < OUT; o++) y[o] = b1[HID + OUT * HID + o];
            for (int i = 0; i < HID; i++) {
                const float4 *r = reinterpret_cast<const float4 *>(W + i * S);
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < S / 4; j++) {
                    const float4 w = r[j];
                    acc += w.x * x[4 * j] + w.y * x[4 * j + 1] + w.z * x[4 * j + 2] + w.w * x[4 * j + 3];
                }
                const float h = fmaxf(acc + b1[i], 0.f);
                Hr[i] = h;
#pragma unroll
                for (int o = 0; o < OUT; o++) y[o] += w2[o * HID + i] * h;
            }
            for (int o = 0; o < OUT; o++) gg[o] = g[(size_t)n * OUT + o];
            head_dy<K>(y, gg, dy);
            for (int o = 0; o < OUT; o++) DYs[lane * 4 + o] = dy[o];
            float dx[ENC];
#pragma unroll
            for (int j = 0; j < ENC; j++) dx[j] = 0.f;
            for (int i = 0; i < HID; i++) {
                float d = 0.f;
#pragma unroll
                for (int o = 0; o < OUT; o++) d += w2[o * HID + i] * dy[o];
                d = Hr[i] > 0.f ? d : 0.f;
                DHr[i] = d;
                const float4 *r = reinterpret_cast<const float4 *>(W + i * S);
#pragma unroll
                for (int j = 0; j < ENC / 4; j++) {
                    const float4 w = r[j];
                    dx[4 * j] += w.x * d; dx[4 * j + 1] += w.y * d; dx[4 * j + 2] += w.z * d; dx[4 * j + 3] += w.w * d;
                }
            }
            float4 *d4 = reinterpret_cast<float4 *>(de + (size_t)n * ENC);
#pragma unroll
            for (int j = 0; j < ENC / 4; j++) d4[j] = make_float4(dx[4 * j], dx[4 * j + 1], dx[4 * j + 2], dx[4 * j + 3]);
        } else {
            for (int j = 0; j < XROW; j++) X[j] = 0.f;
            for (int i = 0; i < HID; i++) { Hr[i] = 0.f; DHr[i] = 0.f; }
            for (int o = 0; o < 4; o++) DYs[lane * 4 + o] = 0.f;
        }
        __syncthreads();
        if (need_w) {
            // thread = hidden unit i: the chunk's 64 points in order
            const int i = lane;
            for (int m = 0; m < CHUNK; m++) {
                const double d = DHs[m * HROW + i], hv = Hs[m * HROW + i];
                const float *xr = Xs + m * XROW;
#pragma unroll
                for (int j = 0; j < IN; j++) acc1[j] += d * (double)xr[j];
                accb1 += d;
#pragma unroll
                for (int o = 0; o < OUT; o++) acc2[o] += (double)DYs[m * 4 + o] * hv;
                if (i < OUT) accb2 += DYs[m * 4 + i];
            }
        }
        __syncthreads();
    }
    if (!need_w) return;
    float *row = a.partial;
    for (int k = 0; k < K; k++) row += (size_t)a.G * head_floats(k);
    row += (size_t)blockIdx.x * head_floats(K);
    const int i = lane;
#pragma unroll
    for (int j = 0; j < IN; j++) row[i * IN + j] = (float)acc1[j];
    row[HID * IN + i] = (float)accb1;
#pragma unroll
    for (int o = 0; o < OUT; o++) row[HID * IN + HID + o * HID + i] = (float)acc2[o];
    if (i < OUT) row[HID * IN + HID + OUT * HID + i] = (float)accb2;
}

__global__ void __launch_bounds__(CHUNK) field_head_bwd_kernel(FieldK a)
{
    __shared__ __attribute__((aligned(16))) BwdLds L;
    const int k = blockIdx.y;
    if (!a.g_out[k]) return;
    switch (k) {
    case 0: head_backward<0>(a, L); break;
    case 1: head_backward<1>(a, L); break;
    case 2: head_backward<2>(a, L); break;
    case 3: head_backward<3>(a, L); break;
    default: head_backward<4>(a, L); break;
    }
}

// grid (ceil(max head floats / 64), NHEAD), 256 threads: wave w sums the rows [w * G / 4, (w + 1) * G / 4) of 64 elements,
// wave 0 adds the four slices in order
__global__ void __launch_bounds__(256) field_reduce_kernel(FieldK a)
{
    const int k = blockIdx.y;
    if (!a.g_out[k] || !a.d_head[k]) return;
    __shared__ double part[4][64];
    const int F = head_floats(k);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const float *base = a.partial;
    for (int q = 0; q < k; q++) base += (size_t)a.G * head_floats(q);
    const int g0 = (int)((int64_t)a.G * w / 4), g1 = (int)((int64_t)a.G * (w + 1) / 4);
    double s = 0.0;                       // the partial rows summed in double: the sums run over up to 2^26 points
    if (e < F)
        for (int gi = g0; gi < g1; gi++) s += base[(size_t)gi * F + e];
    part[w][lane] = s;
    __syncthreads();
    if (w == 0 && e < F) a.d_head[k][e] = (float)(((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]);
}

// dL/dz_j = sum_i W1[i][32 + j] * (sum over points of dL/dh_i): one block of 64
__global__ void __launch_bounds__(64) field_dz_kernel(FieldK a)
{
    __shared__ double db1[HID];
    constexpr int IN = head_in(HEAD_OFFSETS), F = head_floats(HEAD_OFFSETS);
    const int i = threadIdx.x;
    const float *base = a.partial;
    for (int q = 0; q < HEAD_OFFSETS; q++) base += (size_t)a.G * head_floats(q);
    double s = 0.0;                       // in double: dL/dz is a short sum of long, cancelling ones
    if (a.g_out[HEAD_OFFSETS])
        for (int gi = 0; gi < a.G; gi++) s += base[(size_t)gi * F + HID * IN + i];
    db1[i] = s;
    __syncthreads();
    if (i < 2) {
        const float *w1 = a.head[HEAD_OFFSETS].w1;
        double acc = 0.0;
        for (int h = 0; h < HID; h++) acc += (double)w1[h * IN + ENC + i] * db1[h];
        a.d_z[i] = (float)acc;
    }
}

// Adds (v0, v1) to the row `key` of dt and (u0, u1) to that of dq for every active lane of the wave.  Lanes whose neighbours
// hold the same row (points kept in a spatial order share the cells of the coarse levels) are summed first by a segmented scan
// over the run, and the run's last lane adds once: one atomic per run instead of one per lane.  Where no two neighbouring lanes
// share a row (the fine levels, or points in random order) the wave takes the plain path after one shuffle and one ballot.
__device__ inline void wave_add(float *dt, float *dq, uint32_t key, bool act, float v0, float v1, float u0, float u1)
{
    const int lane = __lane_id();
    const uint32_t k = act ? key : (0x80000000u | (uint32_t)lane);    // rows are < 2^28: an inactive lane is a run of its own
    const uint32_t prev = __shfl_up(k, 1);
    const uint64_t starts = __ballot(lane == 0 || prev != k);
    if (SOAR_FIELD_WAVE_COMBINE && starts != ~0ull) {
        const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
        const int s = 63 - __builtin_clzll(starts & upto);               // first lane of this lane's run (lane 0 always starts one)
        for (int d = 1; d < 64; d <<= 1) {
            const bool take = lane - d >= s;
            if (!__any(take)) break;
            const float a0 = __shfl_up(v0, d), a1 = __shfl_up(v1, d), b0 = __shfl_up(u0, d), b1 = __shfl_up(u1, d);
            if (take) { v0 += a0; v1 += a1; u0 += b0; u1 += b1; }
        }
        const bool last = lane == 63 || ((starts >> (lane + 1)) & 1ull);
        act = act && last;
    }
    if (!act) return;
    if (dt) {
        atomicAdd(dt + 2 * (size_t)key, v0);
        atomicAdd(dt + 2 * (size_t)key + 1, v1);
    }
    if (dq) {
        atomicAdd(dq + 2 * (size_t)key, u0);
        atomicAdd(dq + 2 * (size_t)key + 1, u1);
    }
}

// A table with fewer rows per level than a wave has lanes (T <= 32) makes every wave, and every block, hit the same few rows
// over and over: N * 8 / T float atomics land on one element, one after the other, and their rounding grows with the root of
// that count (3 000 points on 2 rows: 3e-6 of the largest element, past the bar of DESIGN.md 9g).  SMALL sums the block's
// contributions in LDS first (both tables: 2 x 16 x T x 2 floats, 8 KB at most) and adds each element to HBM once per block.
constexpr int SMALL_T = 32;
constexpr int SMALL_FLOATS = 2 * LEVELS * SMALL_T * 2;

template <bool SMALL>
__global__ void __launch_bounds__(128) field_scatter_kernel(FieldK a)
{
    // no early exit: every lane of a wave takes part in wave_add's shuffles and in the block's barriers; lanes past N carry nothing
    __shared__ float acc[SMALL ? SMALL_FLOATS : 1];
    if constexpr (SMALL) {
        for (int e = threadIdx.x; e < SMALL_FLOATS; e += blockDim.x) acc[e] = 0.f;
        __syncthreads();
    }
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = n < a.N;
    float g[ENC], qg[ENC];
    bool any_g = false;
#pragma unroll
    for (int j = 0; j < ENC; j++) { g[j] = 0.f; qg[j] = 0.f; }
    for (int k = 0; k < NHEAD; k++) {               // fixed order: shs, scales, offsets, opacities
        if (k == HEAD_QUATS || !a.g_out[k]) continue;
        any_g = true;
        if (!valid) continue;
        const float4 *d4 = reinterpret_cast<const float4 *>(a.de + ((size_t)k * a.N + n) * ENC);
#pragma unroll
        for (int j = 0; j < ENC / 4; j++) {
            const float4 v = d4[j];
            g[4 * j] += v.x; g[4 * j + 1] += v.y; g[4 * j + 2] += v.z; g[4 * j + 3] += v.w;
        }
    }
    const bool any_q = a.g_out[HEAD_QUATS] != nullptr;
    if (any_q && valid) {
        const float4 *d4 = reinterpret_cast<const float4 *>(a.de + ((size_t)HEAD_QUATS * a.N + n) * ENC);
#pragma unroll
        for (int j = 0; j < ENC / 4; j++) {
            const float4 v = d4[j];
            qg[4 * j] = v.x; qg[4 * j + 1] = v.y; qg[4 * j + 2] = v.z; qg[4 * j + 3] = v.w;
        }
    }
    float p[3] = {0.f, 0.f, 0.f}, inv_ext[3] = {0.f, 0.f, 0.f};
    bool sel = false;
    if (valid) normalise(a, n, p, inv_ext, sel);
    const uint32_t mask = (uint32_t)a.T - 1u;
    float *dt = any_g ? a.d_table : nullptr, *dq = any_q ? a.d_qtable : nullptr;
    const bool scatter = valid && (dt || dq);
    const bool want_xyz = valid && a.d_xyz != nullptr && sel && (any_g || any_q);
    const float2 *t2 = reinterpret_cast<const float2 *>(a.table), *q2 = reinterpret_cast<const float2 *>(a.qtable);
    float dx[3] = {0.f, 0.f, 0.f};
    for (int l = 0; l < LEVELS; l++) {
        const Cell cl = cell_of(p, a.res[l]);
        const uint32_t base = (uint32_t)l * (uint32_t)a.T;              // < 2^28
        const float g0 = g[2 * l], g1 = g[2 * l + 1], h0 = qg[2 * l], h1 = qg[2 * l + 1];
        float dol[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t r = base + corner_slot(cl, k, mask);
            const float wx = lerp_w(k & 1, cl.o[0]), wy = lerp_w(k & 2, cl.o[1]), wz = lerp_w(k & 4, cl.o[2]);
            const float w = wx * wy * wz;
            if constexpr (SMALL) {
                // r < 16 * T <= 512: the first table's rows at acc[2 r], the second's behind them
                if (scatter && dt) { atomicAdd(&acc[2 * r], w * g0); atomicAdd(&acc[2 * r + 1], w * g1); }
                if (scatter && dq) { atomicAdd(&acc[2 * (LEVELS * a.T + r)], w * h0); atomicAdd(&acc[2 * (LEVELS * a.T + r) + 1], w * h1); }
            } else if (dt || dq) {
                wave_add(dt, dq, r, scatter, w * g0, w * g1, w * h0, w * h1);
            }
            if (want_xyz) {
                float v = 0.f;
                if (any_g) { const float2 t = t2[r]; v += g0 * t.x + g1 * t.y; }
                if (any_q) { const float2 t = q2[r]; v += h0 * t.x + h1 * t.y; }
                // d w / d o_d: the other two factors, signed by the corner's side on axis d
                dol[0] += v * ((k & 1) ? 1.f : -1.f) * wy * wz;
                dol[1] += v * ((k & 2) ? 1.f : -1.f) * wx * wz;
                dol[2] += v * ((k & 4) ? 1.f : -1.f) * wx * wy;
            }
        }
        for (int d = 0; d < 3; d++) dx[d] += dol[d] * a.res[l];
    }
    if (valid && a.d_xyz)
        for (int d = 0; d < 3; d++) a.d_xyz[3 * n + d] = want_xyz ? dx[d] * inv_ext[d] : 0.f;
    if constexpr (SMALL) {
        __syncthreads();
        const int floats = 2 * LEVELS * a.T;                              // of one table: <= SMALL_FLOATS / 2
        for (int e = threadIdx.x; e < floats; e += blockDim.x) {
            if (dt && acc[e] != 0.f) atomicAdd(dt + e, acc[e]);
            if (dq && acc[floats + e] != 0.f) atomicAdd(dq + e, acc[floats + e]);
        }
    }
}

constexpr int FWD_BLOCK = 128;

size_t de_floats(int N) { return (size_t)NHEAD * N * ENC; }
int blocks_of(int N) { return ((N + CHUNK - 1) / CHUNK + CHUNKS_PER_BLOCK - 1) / CHUNKS_PER_BLOCK; }
size_t partial_floats(int N)
{
    size_t s = 0;
    for (int k = 0; k < NHEAD; k++) s += (size_t)blocks_of(N) * head_floats(k);
    return s;
}
bool check_args(const char *what, const SoarFieldArgs *a)
{
    if (!a) { set_error("%s: NULL args", what); return false; }
    if (a->N < 0 || a->N > MAX_N) { set_error("%s: need 0 <= N <= 2^26 (N=%d)", what, a->N); return false; }
    if (a->log2_T < 1 || a->log2_T > 24) { set_error("%s: need 1 <= log2_T <= 24 (log2_T=%d)", what, a->log2_T); return false; }
    for (int l = 0; l < LEVELS; l++)
        if (!(a->res[l] >= 1.f && a->res[l] < 1e7f)) { set_error("%s: level resolution %d is not in [1, 1e7)", what, l); return false; }
    if (!a->table || !a->qtable) { set_error("%s: NULL table", what); return false; }
    if (a->N > 0 && !a->xyz) { set_error("%s: NULL xyz", what); return false; }
    if (!a->normalized && !a->aabb) { set_error("%s: NULL aabb", what); return false; }
    for (int k = 0; k < NHEAD; k++)
        if (!a->head[k].w1 || !a->head[k].b1 || !a->head[k].w2 || !a->head[k].b2) {
            set_error("%s: NULL weight of head %d", what, k);
            return false;
        }
    if (a->N > 0 && (!a->enc || !a->qenc)) { set_error("%s: NULL enc / qenc", what); return false; }
    const uintptr_t al = (uintptr_t)a->table | (uintptr_t)a->qtable | (uintptr_t)a->enc | (uintptr_t)a->qenc;
    if (al & 15) { set_error("%s: table / enc pointers must be 16-byte aligned", what); return false; }
    return true;
}

FieldK make_k(const SoarFieldArgs *a)
{
    FieldK k{};
    k.N = a->N;
    k.T = 1 << a->log2_T;
    k.normalized = a->normalized != 0;
    for (int l = 0; l < LEVELS; l++) k.res[l] = a->res[l];
    k.xyz = a->xyz; k.aabb = a->aabb; k.table = a->table; k.qtable = a->qtable; k.z = a->z;
    for (int h = 0; h < NHEAD; h++) {
        k.head[h] = a->head[h];
        k.out[h] = a->out[h];
        k.g_out[h] = a->g_out[h];
        k.d_head[h] = a->d_head[h];
    }
    k.enc = a->enc; k.qenc = a->qenc;
    k.d_table = a->d_table; k.d_qtable = a->d_qtable; k.d_xyz = a->d_xyz; k.d_z = a->d_z;
    k.G = blocks_of(a->N);
    return k;
}

// the backward's workspace: dL/de of every head, then the blocks' partial sums.  Never 0 bytes
size_t carve(int N, void *workspace, FieldK *k)
{
    Carver c(workspace);
    float *de = c.take<float>(de_floats(N));
    float *partial = c.take<float>(partial_floats(N));
    if (k) { k->de = de; k->partial = partial; }
    return c.bytes() ? c.bytes() : ALIGN;
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_field_workspace_bytes(int32_t N, size_t *bytes)
{
    if (!bytes || N < 0 || N > MAX_N) { set_error("soar_field_workspace_bytes: bad arguments (N=%d)", N); return 1; }
    *bytes = carve(N, nullptr, nullptr);
    return 0;
}

extern "C" int soar_field_forward(const SoarFieldArgs *args, void *stream_)
{
    if (!check_args("soar_field_forward", args)) return 1;
    for (int k = 0; k < NHEAD; k++)
        if (args->N > 0 && !args->out[k]) { set_error("soar_field_forward: NULL output %d", k); return 1; }
    if (args->N == 0) return 0;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const FieldK k = make_k(args);
    hipLaunchKernelGGL(field_forward_kernel, dim3((args->N + FWD_BLOCK - 1) / FWD_BLOCK), dim3(FWD_BLOCK), 0, stream, k);
    SOAR_LAUNCH_OK("field_forward", stream, 0);
    return 0;
}

extern "C" int soar_field_backward(const SoarFieldArgs *args, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_args("soar_field_backward", args)) return 1;
    if (!workspace_ok("soar_field_backward", workspace, workspace_bytes, carve(args->N, nullptr, nullptr), "soar_field_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t rows = (size_t)LEVELS << args->log2_T;
    if (args->d_table) SOAR_HIP_OK(hipMemsetAsync(args->d_table, 0, rows * 2 * sizeof(float), stream));
    if (args->d_qtable) SOAR_HIP_OK(hipMemsetAsync(args->d_qtable, 0, rows * 2 * sizeof(float), stream));
    if (args->d_z) SOAR_HIP_OK(hipMemsetAsync(args->d_z, 0, 2 * sizeof(float), stream));
    if (args->N == 0) {
        for (int h = 0; h < NHEAD; h++)
            if (args->d_head[h]) SOAR_HIP_OK(hipMemsetAsync(args->d_head[h], 0, head_floats(h) * sizeof(float), stream));
        return 0;
    }
    FieldK k = make_k(args);
    carve(args->N, workspace, &k);
    bool any = false;
    for (int h = 0; h < NHEAD; h++) {
        if (args->g_out[h]) any = true;
        k.need_w[h] = args->d_head[h] != nullptr || (h == HEAD_OFFSETS && args->d_z != nullptr);
        // a head without an upstream gradient has zero weight gradients
        if (!args->g_out[h] && args->d_head[h])
            SOAR_HIP_OK(hipMemsetAsync(args->d_head[h], 0, head_floats(h) * sizeof(float), stream));
    }
    if (!any) {
        if (args->d_xyz) SOAR_HIP_OK(hipMemsetAsync(args->d_xyz, 0, (size_t)args->N * 3 * sizeof(float), stream));
        return 0;
    }
    hipLaunchKernelGGL(field_head_bwd_kernel, dim3(k.G, NHEAD), dim3(CHUNK), 0, stream, k);
    SOAR_LAUNCH_OK("field_head_bwd", stream, 0);
    int maxF = 0;
    for (int h = 0; h < NHEAD; h++) maxF = head_floats(h) > maxF ? head_floats(h) : maxF;
    hipLaunchKernelGGL(field_reduce_kernel, dim3((maxF + 63) / 64, NHEAD), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("field_reduce", stream, 0);
    if (args->d_z && args->g_out[HEAD_OFFSETS]) {
        hipLaunchKernelGGL(field_dz_kernel, dim3(1), dim3(64), 0, stream, k);
        SOAR_LAUNCH_OK("field_dz", stream, 0);
    }
    if (args->d_table || args->d_qtable || args->d_xyz) {
        const dim3 grid((args->N + FWD_BLOCK - 1) / FWD_BLOCK);
        if (k.T <= SMALL_T) hipLaunchKernelGGL(field_scatter_kernel<true>, grid, dim3(FWD_BLOCK), 0, stream, k);
        else hipLaunchKernelGGL(field_scatter_kernel<false>, grid, dim3(FWD_BLOCK), 0, stream, k);
        SOAR_LAUNCH_OK("field_scatter", stream, 0);
    }
    return 0;
}
