// attention.hip -- the transformers' two tiled attentions (sam.hip, unet.hip, clip.hip).
//
//   sam_attn_kernel        SAM's grid attention with the decomposed relative-position bias, windows and whole grids alike.  Window
//                          partition, its zero padding and the un-partition are index arithmetic
//   kv_attn_kernel         out = softmax(q k^T scale) v  (+ w2 softmax(q k2^T scale) v2: a second key / value set in the same launch,
//                          the query read once), separate query, key and value sources and any number of keys.  The last tile's
//                          missing keys are masked, not padded in memory.  CAUSAL (one key set, Lq = Lk): key j counts for query i
//                          when j <= i -- masked inside a tile, and the key tiles wholly behind the workgroup's last query are not
//                          visited.  Key 0 is visible to every query, so a row's running maximum is finite from the first tile on and
//                          a tile without a visible key adds exp(-inf) = 0
// Both are an online softmax over tiles of 32 keys, q k^T and p v on v_mfma_f32_32x32x2_f32, nothing of the score matrix in memory,
// and both are written on the same three pieces (attn_query, attn_tile, attn_store).  Transposed products, so that a lane owns ONE
// query (column i = lane & 31) and the softmax statistics stay in the lane:
//   S^T = K Q^T: A = K tile (row = key), B = Q^T; the lane's 16 registers are keys mfma_row(e, h) of the tile, h = lane >> 5
//   O^T += V^T P^T: A = V^T (row = channel), B = P^T with the MFMA's k index walking the keys in the order the lane holds them
//   (k = step s, half h <-> key mfma_row(s, h)): p never leaves its registers.
// The head dimension is padded to HDP (32, 64 or 96) with zeros in LDS only.  What a kernel keeps to itself: where K and V rows come
// from (its tile loader and LDS layout), its workgroup and grid, and what it adds to or masks from a score.
// No atomics; a (batch, head, query tile)'s sums do not depend on the rest of the launch.
//
//   kv_attn16_kernel       kv_attn_kernel on v_mfma_f32_32x32x16_{bf16,f16} (the contract is attention.h's): the same
//                          sources, masks, second key set and orientation; q scale, k and v rounded to the type (nearest even) on their
//                          way into registers and LDS, p rounded only as the operand of p v, every sum and the softmax in float32.
//                          Its tile step is attn_tile16; attn_store and mfma_row are shared, the C / D layout being the same
#include "attention.h"
#include "conv_gemm.h"

namespace soar {
namespace {

constexpr int AQ = 64;                 // sam_attn_kernel: queries per workgroup, two waves of 32
constexpr int AK = 32;                 // keys per tile, both kernels
constexpr int AS = ATTN_SIDE;
constexpr int KVA_Q = 128;             // kv_attn_kernel: queries per workgroup, four waves of 32

// ---- the shared pieces.  i = lane & 31, h = lane >> 5 ----------------------------------------------------------------------------------
// the lane's query, scaled, in the k order of the S^T product: chunk c, group g holds channels 32 c + 16 h + 4 g .. + 4 of `row`
// (LDS or global memory); zeros where there is no query or the channel is past hd
template <int HDP>
__device__ __forceinline__ void attn_query(float4 (&qreg)[HDP / 32][4], const float *row, bool valid, int hd, float scale, int h)
{
#pragma unroll
    for (int c = 0; c < HDP / 32; c++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int d = c * 32 + h * 16 + 4 * g;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && d < hd) v = *reinterpret_cast<const float4 *>(row + d);
            v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
            qreg[c][g] = v;
        }
}

// One tile of 32 keys, K and V in LDS: the scores, the online softmax's update of m and l, o rescaled and o += p v.
// score(j, s): what key j's score s becomes -- a bias added, or -inf for a key that does not count.  The running maximum must come out
// finite: the tile's first key, or an earlier tile's, counts for every query.
template <int HDP, class Score>
__device__ __forceinline__ void attn_tile(const float (*Ks)[HDP + 4], const float (*Vs)[HDP + 4], const float4 (&qreg)[HDP / 32][4], int key0,
                                          int i, int h, Score score, float &m, float &l, f32x16 (&o)[HDP / 32])
{
    constexpr int NC = HDP / 32;
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; e++) s[e] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 k4 = *reinterpret_cast<const float4 *>(&Ks[i][c * 32 + h * 16 + 4 * g]);
#pragma unroll
            for (int u = 0; u < 4; u++) s = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(k4, u), comp(qreg[c][g], u), s, 0, 0, 0);
        }
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        s[e] = score(key0 + mfma_row(e, h), s[e]);
        mx = fmaxf(mx, s[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float corr = expf(m - mn);                             // (0 at the first tile)
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; e++) { s[e] = expf(s[e] - mn); sum += s[e]; }
    sum += __shfl_xor(sum, 32);
    l = l * corr + sum;
    m = mn;
#pragma unroll
    for (int c = 0; c < NC; c++) {
#pragma unroll
        for (int e = 0; e < 16; e++) o[c][e] *= corr;
#pragma unroll
        for (int u = 0; u < 16; u++) o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[mfma_row(u, h)][c * 32 + i], s[u], o[c], 0, 0, 0);
    }
}

// the lane's result times f to its row: registers 4 g .. 4 g + 3 of chunk c are channels 32 c + 8 g + 4 h .. + 3
template <int HDP>
__device__ __forceinline__ void attn_store(float *dst, const f32x16 (&o)[HDP / 32], float f, int hd, int h)
{
#pragma unroll
    for (int c = 0; c < HDP / 32; c++)
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const int d = c * 32 + 8 * g + 4 * h;
            if (d < hd) *reinterpret_cast<float4 *>(dst + d) = make_float4(o[c][4 * g] * f, o[c][4 * g + 1] * f, o[c][4 * g + 2] * f, o[c][4 * g + 3] * f);
        }
}

template <int NC>
__device__ __forceinline__ void attn_zero(f32x16 (&o)[NC])
{
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
        for (int e = 0; e < 16; e++) o[c][e] = 0.f;
}

// ---- SAM's grid attention ------------------------------------------------------------------------------------------------------------
struct AttnArgs {
    const float *qkv, *bias, *rel_h, *rel_w;
    float *out;
    int gh, gw, heads, hd, win;        // win = 0: one sequence, the grid
    int Sh, Sw, nwx;                   // the sequence's sides; windows per row of windows
    float scale;
};

// Workgroup: 64 queries of one sequence (a window, or the grid) and one head; wave w owns queries 32 w .. + 32.
// rel_h / rel_w: Sh + Sw dot products per query, once, into LDS; a key (ky, kx) adds rel_h[ky] + rel_w[kx].
template <int HDP>
__global__ void __launch_bounds__(128) sam_attn_kernel(AttnArgs a)
{
    constexpr int PITCH = HDP + 4, NC = HDP / 32;
    __shared__ float kv[2 * AK * PITCH];                         // K tile | V tile; first the 64 queries (AQ = 2 AK rows)
    __shared__ float relh[AQ][AS + 1], relw[AQ][AS + 1];
    float(*Ks)[PITCH] = reinterpret_cast<float(*)[PITCH]>(kv);
    float(*Vs)[PITCH] = reinterpret_cast<float(*)[PITCH]>(kv + AK * PITCH);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int head = blockIdx.z % a.heads, b = blockIdx.z / a.heads;
    const int wy = blockIdx.y / a.nwx, wx = blockIdx.y - wy * a.nwx;
    const int oy = wy * a.win, ox = wx * a.win;                  // the sequence's corner on the grid (0, 0 when global)
    const int nk = a.Sh * a.Sw, C = a.heads * a.hd;
    const size_t tok0 = (size_t)b * a.gh * a.gw;
    // token of position j of the sequence, or -1 where the window hangs over the grid's edge (or j is past the sequence)
    auto token = [&](int j) -> int {
        if (j >= nk) return -1;
        const int y = oy + j / a.Sw, x = ox + j % a.Sw;
        return y < a.gh && x < a.gw ? y * a.gw + x : -1;
    };
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // the queries, zero rows where there is none
    for (int f = tid; f < AQ * (HDP / 4); f += 128) {
        const int r = f / (HDP / 4), d = (f - r * (HDP / 4)) * 4;
        const int t = token(blockIdx.x * AQ + r);
        float4 v = zero4;
        if (t >= 0 && d < a.hd) v = *reinterpret_cast<const float4 *>(a.qkv + (tok0 + t) * 3 * C + head * a.hd + d);
        *reinterpret_cast<float4 *>(&Ks[r][d]) = v;              // (rows 32 .. 63 run on into the V tile)
    }
    __syncthreads();
    if (a.rel_h) {
        for (int e = tid; e < AQ * (a.Sh + a.Sw); e += 128) {
            const int q = e % AQ, r = e / AQ;
            const int j = blockIdx.x * AQ + q;
            float s = 0.f;
            if (j < nk) {
                const int qy = j / a.Sw, qx = j - qy * a.Sw;
                const float *tab = r < a.Sh ? a.rel_h + (size_t)(qy - r + a.Sh - 1) * a.hd : a.rel_w + (size_t)(qx - (r - a.Sh) + a.Sw - 1) * a.hd;
                for (int d = 0; d < a.hd; d += 4) {
                    const float4 qv = *reinterpret_cast<const float4 *>(&Ks[q][d]);
                    const float4 tv = *reinterpret_cast<const float4 *>(tab + d);
                    s += qv.x * tv.x + qv.y * tv.y + qv.z * tv.z + qv.w * tv.w;
                }
            }
            if (r < a.Sh) relh[q][r] = s; else relw[q][r - a.Sh] = s;
        }
    }
    const int ql = wave * 32 + i;                                // this lane's query in the tile
    float4 qreg[NC][4];
    attn_query<HDP>(qreg, Ks[ql], true, HDP, a.scale, h);        // (the LDS row is whole: zeros past hd)
    __syncthreads();

    float m = -INFINITY, l = 0.f;
    f32x16 o[NC];
    attn_zero(o);
    const int ntiles = (nk + AK - 1) / AK;
    for (int kt = 0; kt < ntiles; kt++) {
        // K and V of 32 keys: four threads a key; a key off the grid is the bias (the projection of a zero token)
        {
            const int r = tid >> 2, j = kt * AK + r;
            const int t = token(j);
            const float *kp = nullptr;
            if (t >= 0) kp = a.qkv + (tok0 + t) * 3 * C + C + head * a.hd;
            else if (j < nk) kp = a.bias + C + head * a.hd;
            for (int f = tid & 3; f < HDP / 4; f += 4) {
                const int d = f * 4;
                float4 kk = zero4, vv = zero4;
                if (kp && d < a.hd) { kk = *reinterpret_cast<const float4 *>(kp + d); vv = *reinterpret_cast<const float4 *>(kp + C + d); }
                *reinterpret_cast<float4 *>(&Ks[r][d]) = kk;
                *reinterpret_cast<float4 *>(&Vs[r][d]) = vv;
            }
        }
        __syncthreads();
        attn_tile<HDP>(Ks, Vs, qreg, kt * AK, i, h, [&](int j, float s) {
            float v = -INFINITY;                                 // the tail of the last tile
            if (j < nk) {
                v = s;
                if (a.rel_h) { const int ky = j / a.Sw; v += relh[ql][ky] + relw[ql][j - ky * a.Sw]; }
            }
            return v;
        }, m, l, o);
        __syncthreads();
    }
    const int t = token(blockIdx.x * AQ + ql);
    if (t < 0) return;                                           // no such query, or a padded one: dropped
    attn_store<HDP>(a.out + (tok0 + t) * C + head * a.hd, o, 1.f / l, a.hd, h);
}

// ---- separate query, key and value sources ---------------------------------------------------------------------------------------------
// Workgroup: 128 queries of one (batch, head); wave w owns queries 32 w .. + 32.
template <int HDP, bool CAUSAL>
__global__ void __launch_bounds__(256) kv_attn_kernel(SoarUnetAttnArgs a)
{
    constexpr int PITCH = HDP + 4, NC = HDP / 32;
    __shared__ float Ks[AK][PITCH], Vs[AK][PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int qi = blockIdx.x * KVA_Q + wave * 32 + i;           // this lane's query
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    float4 qreg[NC][4];
    attn_query<HDP>(qreg, a.q + ((size_t)b * a.Lq + qi) * a.ldq + head * a.hd, qi < a.Lq, a.hd, a.scale, h);
    f32x16 total[NC];
    attn_zero(total);

    // one key / value set: its normalised result times wgt is added to total
    auto run = [&](const float *kp, const float *vp, int64_t ldk, int64_t ldv, int nk, float wgt) {
        float m = -INFINITY, l = 0.f;
        f32x16 o[NC];
        attn_zero(o);
        int ntiles = (nk + AK - 1) / AK;
        if (CAUSAL) {                                            // the workgroup's last query sees keys 0 .. itself
            const int last = min(a.Lq, ((int)blockIdx.x + 1) * KVA_Q) - 1;
            ntiles = min(ntiles, last / AK + 1);
        }
        for (int kt = 0; kt < ntiles; kt++) {
            // K and V of 32 keys, eight threads a key; rows past the last key and channels past hd are zeros
            {
                const int r = tid >> 3, j = kt * AK + r;
                for (int f = tid & 7; f < HDP / 4; f += 8) {
                    const int d = f * 4;
                    float4 kk = zero4, vv = zero4;
                    if (j < nk && d < a.hd) {
                        kk = *reinterpret_cast<const float4 *>(kp + ((size_t)b * nk + j) * ldk + head * a.hd + d);
                        vv = *reinterpret_cast<const float4 *>(vp + ((size_t)b * nk + j) * ldv + head * a.hd + d);
                    }
                    *reinterpret_cast<float4 *>(&Ks[r][d]) = kk;
                    *reinterpret_cast<float4 *>(&Vs[r][d]) = vv;
                }
            }
            __syncthreads();
            // the tail of the last tile; the keys behind the query
            attn_tile<HDP>(Ks, Vs, qreg, kt * AK, i, h, [&](int j, float s) { return j < nk && (!CAUSAL || j <= qi) ? s : -INFINITY; }, m, l, o);
            __syncthreads();
        }
        const float inv = 1.f / l;
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int e = 0; e < 16; e++) total[c][e] += wgt * (o[c][e] * inv);
    };
    run(a.k, a.v, a.ldk, a.ldv, a.Lk, 1.f);
    if (a.k2) run(a.k2, a.v2, a.ldk2, a.ldv2, a.Lk2, a.w2);

    if (qi >= a.Lq) return;                                      // the tail of the last query tile
    attn_store<HDP>(a.out + ((size_t)b * a.Lq + qi) * a.ldo + head * a.hd, total, 1.f, a.hd, h);
}

// ---- 16-bit operands ----------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// float -> T is the compiler's conversion, which rounds to nearest even (v_cvt_pk_bf16_f32, v_cvt_f16_f32)
template <typename T> struct Op16;
template <> struct Op16<__bf16> {
    typedef bf16x8 v8;
    typedef __bf16 v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Op16<_Float16> {
    typedef f16x8 v8;
    typedef _Float16 v4 __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

// LDS row pitches in 16-bit elements.  K is [key][channel], pitch HDP + 8: 80, 144 or 208 bytes, an ODD number (5, 9, 13) of 16-byte
// slots.  V is transposed, [channel][key position], pitch 32 + 8: 80 bytes, five slots.  Every fragment is one ds_read_b128 of lane
// (i, h) at slot odd (row0 + i) + 2 step + h.  That instruction is served in groups of 16 lanes of one h whose i cover every residue
// modulo 16 ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}); a bank row is 16 slots wide and i -> odd i mod 16 is one-to-one, so a
// group's 16 lanes hit 16 different slots: conflict-free.  The staging writes are ds_write_b64 (groups of 16 consecutive lanes, 32
// banks): K's group is two keys' 64 contiguous bytes, pitch 20 / 4 / 20 banks apart (2-way on 4 / 12 / 4 of the 16 banks); V's group
// is 8 key positions' 64 bytes of two channel quads 320 bytes = 16 banks apart: conflict-free.
constexpr int KPAD16 = 8;
constexpr int VPITCH16 = AK + 8;
// where key kk of a tile lies in a V^T row: the k order in which the score registers, converted pairwise, are the P^T operand --
// element j of lane half h of step s is key 16 s + 8 (j >> 2) + 4 h + (j & 3), and sits at position 16 s + 8 h + j
__device__ __forceinline__ int vt_pos(int kk) { return (kk & 16) + 8 * ((kk >> 2) & 1) + 4 * ((kk >> 3) & 1) + (kk & 3); }

// the lane's query, scaled in float32 and then rounded to T, as the B operand of the S^T product: step c holds channels
// 16 c + 8 h .. + 8 of `row`; zeros where there is no query or the channel is past hd
template <typename T, int HDP>
__device__ __forceinline__ void attn_query16(typename Op16<T>::v8 (&qreg)[HDP / 16], const float *row, bool valid, int hd, float scale, int h)
{
#pragma unroll
    for (int c = 0; c < HDP / 16; c++)
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const int d = c * 16 + h * 8 + 4 * g;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && d < hd) v = *reinterpret_cast<const float4 *>(row + d);
            qreg[c][4 * g] = (T)(v.x * scale); qreg[c][4 * g + 1] = (T)(v.y * scale);
            qreg[c][4 * g + 2] = (T)(v.z * scale); qreg[c][4 * g + 3] = (T)(v.w * scale);
        }
}

// attn_tile with 16-bit operands: K [key][channel] and V^T [channel][vt_pos(key)] of T in LDS.  The scores, the mask, m, corr, p and l
// are float32 exactly as in attn_tile (l sums the unrounded p); p is rounded to T only as the operand of o += p v: registers
// 8 s .. 8 s + 7 are the B fragment of step s as they stand.
template <typename T, int HDP, class Score>
__device__ __forceinline__ void attn_tile16(const T (*Ks)[HDP + KPAD16], const T (*Vt)[VPITCH16], const typename Op16<T>::v8 (&qreg)[HDP / 16],
                                            int key0, int i, int h, Score score, float &m, float &l, f32x16 (&o)[HDP / 32])
{
    typedef typename Op16<T>::v8 v8;
    constexpr int NC = HDP / 32;
    f32x16 s;
#pragma unroll
    for (int e = 0; e < 16; e++) s[e] = 0.f;
#pragma unroll
    for (int c = 0; c < HDP / 16; c++) s = Op16<T>::mfma(*reinterpret_cast<const v8 *>(&Ks[i][c * 16 + h * 8]), qreg[c], s);
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        s[e] = score(key0 + mfma_row(e, h), s[e]);
        mx = fmaxf(mx, s[e]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float corr = expf(m - mn);                             // (0 at the first tile)
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 16; e++) { s[e] = expf(s[e] - mn); sum += s[e]; }
    sum += __shfl_xor(sum, 32);
    l = l * corr + sum;
    m = mn;
    v8 p[2];
#pragma unroll
    for (int e = 0; e < 16; e++) p[e >> 3][e & 7] = (T)s[e];
#pragma unroll
    for (int c = 0; c < NC; c++) {
#pragma unroll
        for (int e = 0; e < 16; e++) o[c][e] *= corr;
#pragma unroll
        for (int u = 0; u < 2; u++) o[c] = Op16<T>::mfma(*reinterpret_cast<const v8 *>(&Vt[c * 32 + i][u * 16 + h * 8]), p[u], o[c]);
    }
}

// kv_attn_kernel's workgroup, grid, sources and masks.  Staging is through registers, one tile ahead: the next tile's global loads are
// issued (and rounded) before this tile's products and written to LDS behind them.  K: eight threads a key, four channels each a pass
// (as kv_attn_kernel).  V: thread (kg = tid & 7, cq = tid >> 3) takes keys 4 kg .. + 3 at channels 4 cq .. + 3, transposes the
// 4 x 4 in registers and writes each channel's four keys (consecutive positions of vt_pos) as 8 bytes.
template <typename T, int HDP, bool CAUSAL>
__global__ void __launch_bounds__(256) kv_attn16_kernel(SoarUnetAttnArgs a)
{
    typedef typename Op16<T>::v8 v8;
    typedef typename Op16<T>::v4 v4;
    constexpr int NC = HDP / 32, KF = HDP / 32;                  // (K: HDP / 4 float4 a key over eight threads)
    __shared__ __attribute__((aligned(16))) T Ks[AK][HDP + KPAD16], Vt[HDP][VPITCH16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, h = lane >> 5;
    const int head = blockIdx.y, b = blockIdx.z;
    const int qi = blockIdx.x * KVA_Q + wave * 32 + i;           // this lane's query
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    v8 qreg[HDP / 16];
    attn_query16<T, HDP>(qreg, a.q + ((size_t)b * a.Lq + qi) * a.ldq + head * a.hd, qi < a.Lq, a.hd, a.scale, h);
    f32x16 total[NC];
    attn_zero(total);

    const int kr = tid >> 3, kf = tid & 7;                       // K staging: key of the tile, first float4
    const int kg = tid & 7, cq = tid >> 3;                       // V staging: group of four keys, channel quad
    const int vpos = vt_pos(4 * kg);

    // one key / value set: its normalised result times wgt is added to total
    auto run = [&](const float *kp, const float *vp, int64_t ldk, int64_t ldv, int nk, float wgt) {
        float m = -INFINITY, l = 0.f;
        f32x16 o[NC];
        attn_zero(o);
        int ntiles = (nk + AK - 1) / AK;
        if (CAUSAL) {                                            // the workgroup's last query sees keys 0 .. itself
            const int last = min(a.Lq, ((int)blockIdx.x + 1) * KVA_Q) - 1;
            ntiles = min(ntiles, last / AK + 1);
        }
        v4 kreg[KF], vreg[4];
        // tile kt, rounded, into registers; rows past the last key and channels past hd are zeros
        auto fetch = [&](int kt) {
#pragma unroll
            for (int u = 0; u < KF; u++) {
                const int j = kt * AK + kr, d = (kf + 8 * u) * 4;
                float4 kk = zero4;
                if (j < nk && d < a.hd) kk = *reinterpret_cast<const float4 *>(kp + ((size_t)b * nk + j) * ldk + head * a.hd + d);
                kreg[u][0] = (T)kk.x; kreg[u][1] = (T)kk.y; kreg[u][2] = (T)kk.z; kreg[u][3] = (T)kk.w;
            }
            if (cq < HDP / 4) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int j = kt * AK + 4 * kg + u, d = cq * 4;
                    float4 vv = zero4;
                    if (j < nk && d < a.hd) vv = *reinterpret_cast<const float4 *>(vp + ((size_t)b * nk + j) * ldv + head * a.hd + d);
                    vreg[0][u] = (T)vv.x; vreg[1][u] = (T)vv.y; vreg[2][u] = (T)vv.z; vreg[3][u] = (T)vv.w;
                }
            }
        };
        auto stash = [&]() {
#pragma unroll
            for (int u = 0; u < KF; u++) *reinterpret_cast<v4 *>(&Ks[kr][(kf + 8 * u) * 4]) = kreg[u];
            if (cq < HDP / 4) {
#pragma unroll
                for (int ch = 0; ch < 4; ch++) *reinterpret_cast<v4 *>(&Vt[cq * 4 + ch][vpos]) = vreg[ch];
            }
        };
        fetch(0);
        for (int kt = 0; kt < ntiles; kt++) {
            stash();
            __syncthreads();
            if (kt + 1 < ntiles) fetch(kt + 1);
            // the tail of the last tile; the keys behind the query
            attn_tile16<T, HDP>(Ks, Vt, qreg, kt * AK, i, h, [&](int j, float s) { return j < nk && (!CAUSAL || j <= qi) ? s : -INFINITY; }, m, l, o);
            __syncthreads();
        }
        const float inv = 1.f / l;
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
            for (int e = 0; e < 16; e++) total[c][e] += wgt * (o[c][e] * inv);
    };
    run(a.k, a.v, a.ldk, a.ldv, a.Lk, 1.f);
    if (a.k2) run(a.k2, a.v2, a.ldk2, a.ldv2, a.Lk2, a.w2);

    if (qi >= a.Lq) return;                                      // the tail of the last query tile
    attn_store<HDP>(a.out + ((size_t)b * a.Lq + qi) * a.ldo + head * a.hd, total, 1.f, a.hd, h);
}

}  // namespace

int launch_sam_attention(const float *qkv, const float *bias, const float *rel_h, const float *rel_w, float *out, int B, int gh, int gw,
                         int heads, int hd, int win, float scale, hipStream_t stream)
{
    const char *me = "sam attention";
    if (B < 0 || gh < 1 || gw < 1 || heads < 1 || hd < 4 || hd > 96 || hd % 4 || win < 0 || (int64_t)B * heads > 65535 ||
        (int64_t)B * gh * gw * heads * hd * 3 > (int64_t(1) << 40)) {
        set_error("%s: bad sizes (B=%d, grid %d x %d, heads=%d, hd=%d: a multiple of 4 up to 96, window=%d, B heads <= 65535)", me, B, gh, gw, heads, hd, win);
        return 1;
    }
    AttnArgs a{qkv, bias, rel_h, rel_w, out, gh, gw, heads, hd, win, win ? win : gh, win ? win : gw, win ? (gw + win - 1) / win : 1, scale};
    const int nwy = win ? (gh + win - 1) / win : 1;
    if (a.Sh > AS || a.Sw > AS) { set_error("%s: a sequence of %d x %d tokens: at most %d a side", me, a.Sh, a.Sw, AS); return 1; }
    if (B == 0) return 0;
    if (!qkv || !out || (win && !bias) || (!rel_h != !rel_w)) { set_error("%s: NULL qkv, out or (with windows) bias, or one rel table without the other", me); return 1; }
    if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)bias | (uintptr_t)rel_h | (uintptr_t)rel_w) & 15) { set_error("%s: pointers must be 16-byte aligned", me); return 1; }
    const dim3 grid((unsigned)((a.Sh * a.Sw + AQ - 1) / AQ), (unsigned)(nwy * a.nwx), (unsigned)(B * heads));
    void (*const kern[3])(AttnArgs) = {sam_attn_kernel<32>, sam_attn_kernel<64>, sam_attn_kernel<96>};
    hipLaunchKernelGGL(kern[(hd - 1) / 32], grid, dim3(128), 0, stream, a);
    SOAR_LAUNCH_OK("sam_attn", stream, 0);
    return 0;
}

// what both key / value launchers refuse; 0: launch, 1: refused (the error set), -1: B = 0, nothing to do
static int check_kv_attention(const SoarUnetAttnArgs &a, int hd_max, bool causal, const char *me)
{
    const int64_t C = (int64_t)a.heads * a.hd;
    if (a.B < 0 || a.B > 65535 || a.Lq < 1 || a.Lk < 1 || a.heads < 1 || a.heads > 65535 || a.hd < 4 || a.hd > hd_max || a.hd % 4 ||
        (int64_t)a.B * a.Lq > (int64_t(1) << 30) || (int64_t)a.B * a.Lk > (int64_t(1) << 30)) {
        set_error("%s: bad sizes (B=%d <= 65535, Lq=%d, Lk=%d from 1, heads=%d, hd=%d: a multiple of 4 up to %d)", me, a.B, a.Lq, a.Lk, a.heads, a.hd, hd_max);
        return 1;
    }
    if (a.B == 0) return -1;
    if (!a.q || !a.k || !a.v || !a.out || (!a.k2 != !a.v2) || (a.k2 && (a.Lk2 < 1 || (int64_t)a.B * a.Lk2 > (int64_t(1) << 30)))) {
        set_error("%s: NULL q, k, v or out, or a second key set without its values or with Lk2 = %d below 1", me, a.Lk2);
        return 1;
    }
    const int64_t lds[6] = {a.ldq, a.ldk, a.ldv, a.ldo, a.k2 ? a.ldk2 : C, a.k2 ? a.ldv2 : C};
    for (int64_t ld : lds)
        if (ld < C || ld % 4) { set_error("%s: a row pitch of %lld floats: need a multiple of 4 from heads hd = %lld", me, (long long)ld, (long long)C); return 1; }
    if (((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v | (uintptr_t)a.out | (uintptr_t)a.k2 | (uintptr_t)a.v2) & 15) {
        set_error("%s: pointers must be 16-byte aligned", me);
        return 1;
    }
    if (causal && (a.k2 || a.Lq != a.Lk)) { set_error("%s: a causal mask needs one key set and Lq = Lk (Lq=%d, Lk=%d)", me, a.Lq, a.Lk); return 1; }
    return 0;
}

int launch_kv_attention(const SoarUnetAttnArgs &a, int hd_max, bool causal, const char *me, hipStream_t stream)
{
    if (const int rc = check_kv_attention(a, hd_max, causal, me)) return rc > 0;
    const dim3 grid((unsigned)((a.Lq + KVA_Q - 1) / KVA_Q), (unsigned)a.heads, (unsigned)a.B);
    void (*const kern[3][2])(SoarUnetAttnArgs) = {{kv_attn_kernel<32, false>, kv_attn_kernel<32, true>},
                                                  {kv_attn_kernel<64, false>, kv_attn_kernel<64, true>},
                                                  {kv_attn_kernel<96, false>, kv_attn_kernel<96, true>}};
    hipLaunchKernelGGL(kern[(a.hd - 1) / 32][causal], grid, dim3(256), 0, stream, a);
    SOAR_LAUNCH_OK("kv_attn", stream, 0);
    return 0;
}

int launch_kv_attention16(const SoarUnetAttnArgs &a, int type, int hd_max, bool causal, const char *me, hipStream_t stream)
{
    if (type != WT_BF16 && type != WT_F16) { set_error("%s: the 16-bit attention's type must be 1 (bf16) or 2 (f16) (got %d)", me, type); return 1; }
    if (const int rc = check_kv_attention(a, hd_max, causal, me)) return rc > 0;
    const dim3 grid((unsigned)((a.Lq + KVA_Q - 1) / KVA_Q), (unsigned)a.heads, (unsigned)a.B);
    void (*const kern[2][3][2])(SoarUnetAttnArgs) = {{{kv_attn16_kernel<__bf16, 32, false>, kv_attn16_kernel<__bf16, 32, true>},
                                                      {kv_attn16_kernel<__bf16, 64, false>, kv_attn16_kernel<__bf16, 64, true>},
                                                      {kv_attn16_kernel<__bf16, 96, false>, kv_attn16_kernel<__bf16, 96, true>}},
                                                     {{kv_attn16_kernel<_Float16, 32, false>, kv_attn16_kernel<_Float16, 32, true>},
                                                      {kv_attn16_kernel<_Float16, 64, false>, kv_attn16_kernel<_Float16, 64, true>},
                                                      {kv_attn16_kernel<_Float16, 96, false>, kv_attn16_kernel<_Float16, 96, true>}}};
    hipLaunchKernelGGL(kern[type - 1][(a.hd - 1) / 32][causal], grid, dim3(256), 0, stream, a);
    SOAR_LAUNCH_OK("kv_attn16", stream, 0);
    return 0;
}

int launch_attention(const SoarUnetAttnArgs &a, int type, int hd_max, bool causal, const char *me, hipStream_t stream)
{
    return type ? launch_kv_attention16(a, type, hd_max, causal, me, stream) : launch_kv_attention(a, hd_max, causal, me, stream);
}

}  // namespace soar

extern "C" int soar_attention16(const SoarUnetAttnArgs *args, int32_t type, int32_t causal, void *stream)
{
    if (!args) { soar::set_error("soar_attention16: NULL args"); return 1; }
    return soar::launch_kv_attention16(*args, type, 96, causal != 0, "soar_attention16", static_cast<hipStream_t>(stream));
}
