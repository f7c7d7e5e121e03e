// conv_gemm.hip -- the implicit-GEMM convolution of the VAE encoder and the normal networks, and the three networks' weight packer
// (conv_gemm.h).
//
//   conv_pack_kernel       torch [Cout][Cin][kk] -> [Cout][tap][Cin] (forward) and, where asked, spatially flipped and transposed,
//                          [Cin][tap][ldb] (data gradient): both directions are then the same implicit GEMM
//   conv_gemm_kernel       an implicit GEMM on v_mfma_f32_32x32x2_f32 (exact f32 products): M = grid positions, N = output
//                          channels, K = (tap, cin), tiles staged through LDS.  The A loader does strides, padding (zero or mirrored)
//                          and zero dilation as index arithmetic over a table of taps.  Epilogue: y = act(alpha acc + bias) + res,
//                          scattered to the tap table's output parity (act: none, exact GELU or ReLU; or, with act none, a PReLU of
//                          one slope per output channel: ConvGemm::slope)
//   conv_pack16_kernel     torch [Cout][Cin][kk] float32 -> [Cout][tap][Cinp] bf16 / f16, rounded to nearest even (forward)
//   conv_pack16_bwd_kernel the same values spatially flipped and transposed, [Cin][tap][ldb] bf16 / f16: conv_pack_kernel's data-gradient
//                          form in the 16-bit type
//   conv_gemm16_kernel     the same implicit GEMM on v_mfma_f32_32x32x16_{bf16,f16}: B read as 16-bit values, A rounded to the type
//                          on its way into LDS, float32 accumulators and the same epilogue (ConvGemm::wtype)
//
// The launcher refuses the descriptors the kernel cannot run (conv_gemm.h); soar_selftest_conv_gemm / _conv_gemm16 / _conv_pack /
// _conv_pack16 / _conv_pack16_bwd at the end of the file reach the launcher and the packers by themselves (tests/test_conv_gemm_*.py).
// No atomics: every output has one fixed order of summation, the same whatever the tile and the batch.
#include "conv_gemm.h"

namespace soar {

namespace {

__global__ void __launch_bounds__(256) conv_pack_kernel(const float *__restrict__ w, float *__restrict__ fwd, float *__restrict__ bwd,
                                                        int Cout, int Cin, int kk, int64_t ldb)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Cout * Cin * kk) return;
    // e walks the torch layout [co][ci][t]
    const int t = (int)(e % kk);
    const int64_t r = e / kk;
    const int ci = (int)(r % Cin), co = (int)(r / Cin);
    const float v = w[e];
    fwd[((size_t)co * kk + t) * Cin + ci] = v;
    // the data gradient is the convolution of the output gradient with W'[ci][co][kk - 1 - t]
    if (bwd) bwd[((size_t)ci * kk + (kk - 1 - t)) * ldb + co] = v;
}

// torch [Cout][Cin][kk] float32 -> [Cout][kk][Cinp] of T, rounded to nearest even, channels Cin .. Cinp - 1 zeros
template <typename T>
__global__ void __launch_bounds__(256) conv_pack16_kernel(const float *__restrict__ w, T *__restrict__ out, int Cout, int Cin, int Cinp, int kk)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Cout * kk * Cinp) return;
    // e walks the packed layout [co][t][ci]
    const int ci = (int)(e % Cinp);
    const int64_t r = e / Cinp;
    const int t = (int)(r % kk), co = (int)(r / kk);
    out[e] = ci < Cin ? (T)w[((size_t)co * Cin + ci) * kk + t] : (T)0.f;
}

// torch [Cout][Cin][kk] float32 -> the data gradient's form [(ci kk + kk - 1 - t) ldb + co] of T, rounded to nearest even: columns
// 0 .. cols - 1 of every row are written, those from Cout on as zeros
template <typename T>
__global__ void __launch_bounds__(256) conv_pack16_bwd_kernel(const float *__restrict__ w, T *__restrict__ out, int Cout, int Cin, int kk,
                                                              int64_t ldb, int cols)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Cin * kk * cols) return;
    // e walks the written part of the packed layout [ci][kk - 1 - t][co]
    const int co = (int)(e % cols);
    const int64_t r = e / cols;
    const int t = kk - 1 - (int)(r % kk), ci = (int)(r / kk);
    out[(size_t)r * ldb + co] = co < Cout ? (T)w[((size_t)co * Cin + ci) * kk + t] : (T)0.f;
}

// The epilogue of both kernels: y = act(alpha acc + bias) + res (act none and a slope: y = prelu(alpha acc + bias) + res) of a wave's WM x WN accumulator blocks (C / D layout: mfma_row),
// scattered to the tap table's output parity.  Lane (i, h); the wave's blocks start at row r0 + wr, column c0 + wc of the product.
template <int WM, int WN>
__device__ __forceinline__ void conv_gemm_epilogue(const ConvGemm &k, const ConvTaps &ph, const f32x16 (&acc)[WM][WN], int img0, int rows,
                                                   int hwg, int r0, int c0, int wr, int wc, int i, int h)
{
    bool cv[WN];
    float bias[WN], slope[WN];
#pragma unroll
    for (int c = 0; c < WN; c++) {
        const int co = c0 + wc + c * 32 + i;
        cv[c] = co < k.Cout;
        bias[c] = k.bias && cv[c] ? k.bias[co] : 0.f;
        slope[c] = k.slope && cv[c] ? k.slope[co] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < WM; r++)
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int row = r0 + wr + r * 32 + mfma_row(e, h);
            if (row >= rows) continue;
            const int n = row / hwg;
            const int q = row - n * hwg, y = q / k.Wg, x = q - y * k.Wg;
            const size_t base = ((size_t)(img0 + n) * k.yim + (size_t)(y * k.os + ph.py) * k.Wout + (size_t)(x * k.os + ph.px)) * k.ldy;
#pragma unroll
            for (int c = 0; c < WN; c++) {
                if (!cv[c]) continue;
                const size_t idx = base + (c0 + wc + c * 32 + i);
                float v = acc[r][c][e] * k.alpha + bias[c];
                if (k.act) v = k.act == ACT_GELU ? gelu_erf(v) : fmaxf(v, 0.f);     // (act = 0: the arithmetic of every call before it)
                else if (k.slope) v = v > 0.f ? v : slope[c] * v;                   // (slope = NULL: likewise)
                if (k.res) v += k.res[idx];
                k.y[idx] = v;
            }
        }
}

// Block tile 64 WM x 64 WN, waves 2 x 2, each 32 WM x 32 WN as WM x WN MFMA blocks.  K runs flat over (tap, cin) in chunks of 32; a
// staging thread moves groups of 8 floats, which never straddle a tap because Cin is a multiple of 8; groups behind K, rows behind M
// and columns behind Cout are zeros.  One LDS buffer: a chunk is staged, a barrier, the next chunk's loads are issued and stay in
// flight while the MFMAs of this one run, a barrier.
// Lane (i, h) of a wave: row / column i of a 32 x 32 block, k half h; step s of a chunk sums k = s (h = 0) and k = 16 + s (h = 1).
// So every output's sum runs chunk by chunk and inside a chunk k = 0, 16, 1, 17, ... whatever WM, WN and its place in the tile.
template <int WM, int WN>
__global__ void __launch_bounds__(256) conv_gemm_kernel(ConvGemm k)
{
    constexpr int BM = 64 * WM, BN = 64 * WN;
    __shared__ float As[BM][LDSK], Bs[BN][LDSK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ConvTaps &ph = k.ph[blockIdx.y];
    const int tn = (int)(blockIdx.x % (unsigned)k.tiles_n);
    int tm = (int)(blockIdx.x / (unsigned)k.tiles_n);
    const int hwg = k.Hg * k.Wg;
    // the tile's rows r0 .. of image img0 on (flat: img0 = 0 and the rows run on through the batch)
    int img0 = 0, rows = k.N * hwg;
    if (k.per_image) { img0 = tm / k.tiles_img; tm -= img0 * k.tiles_img; rows = hwg; }
    const int r0 = tm * BM, c0 = tn * BN;
    const int Kp = ph.ntaps * k.Cin, nch = (Kp + BK - 1) / BK;
    const int dm = k.dil - 1;                       // dil = 1 or 2: mask and shift of a dilated coordinate

    // the staging thread's rows: tid >> 2 (+ 64 j), floats (tid & 3) * 8 .. + 8 of the chunk
    const int srow = tid >> 2, sk = (tid & 3) * 8;
    bool av[WM];
    int gy[WM], gx[WM];
    size_t abase[WM];
#pragma unroll
    for (int j = 0; j < WM; j++) {
        const int r = r0 + srow + 64 * j;
        av[j] = r < rows;
        const int n = av[j] ? r / hwg : 0;
        const int q = av[j] ? r - n * hwg : 0;
        gy[j] = q / k.Wg;
        gx[j] = q - gy[j] * k.Wg;
        abase[j] = (size_t)(img0 + n) * k.xim;
    }
    const float *wrow[WN];
    bool bv[WN];
#pragma unroll
    for (int j = 0; j < WN; j++) {
        const int co = c0 + srow + 64 * j;
        bv[j] = co < k.Cout;
        wrow[j] = ph.w + (size_t)img0 * k.wbat + (size_t)(bv[j] ? co : 0) * ph.ldw;
    }

    float4 na[WM][2], nb[WN][2];
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int ch) {
        const int kk = ch * BK + sk;
        const bool kv = kk < Kp;
        const int t = kv ? kk / k.Cin : 0;
        const int ci = kk - t * k.Cin;
        const int dy = ph.dy[t], dx = ph.dx[t];
#pragma unroll
        for (int j = 0; j < WM; j++) {
            int iy = gy[j] * k.stride + dy, ix = gx[j] * k.stride + dx;
            bool ok = kv && av[j];
            ok = ok && !((iy | ix) & dm);           // dilated by two: odd coordinates are zeros, even ones (negative ones stay negative)
            iy >>= dm; ix >>= dm;                   //   x at half
            if (k.reflect) { iy = mirror(iy, k.Hin); ix = mirror(ix, k.Win); }
            else ok = ok && iy >= 0 && iy < k.Hin && ix >= 0 && ix < k.Win;
            if (ok) {
                const float4 *s = reinterpret_cast<const float4 *>(k.x + (abase[j] + (size_t)iy * k.Win + ix) * k.ldx + ci);
                na[j][0] = s[0];
                na[j][1] = s[1];
            } else {
                na[j][0] = na[j][1] = zero4;
            }
        }
#pragma unroll
        for (int j = 0; j < WN; j++) {
            if (kv && bv[j]) {
                const float4 *s = reinterpret_cast<const float4 *>(wrow[j] + kk);
                nb[j][0] = s[0];
                nb[j][1] = s[1];
            } else {
                nb[j][0] = nb[j][1] = zero4;
            }
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < WM; j++) {
            *reinterpret_cast<float4 *>(&As[srow + 64 * j][sk]) = na[j][0];
            *reinterpret_cast<float4 *>(&As[srow + 64 * j][sk + 4]) = na[j][1];
        }
#pragma unroll
        for (int j = 0; j < WN; j++) {
            *reinterpret_cast<float4 *>(&Bs[srow + 64 * j][sk]) = nb[j][0];
            *reinterpret_cast<float4 *>(&Bs[srow + 64 * j][sk + 4]) = nb[j][1];
        }
    };

    const int i = lane & 31, h = lane >> 5;
    const int wr = (wave >> 1) * 32 * WM, wc = (wave & 1) * 32 * WN;
    f32x16 acc[WM][WN];
#pragma unroll
    for (int r = 0; r < WM; r++)
#pragma unroll
        for (int c = 0; c < WN; c++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[r][c][e] = 0.f;

    fetch(0);
    for (int ch = 0; ch < nch; ch++) {
        stage();
        lds_barrier();
        if (ch + 1 < nch) fetch(ch + 1);            // in flight while the MFMAs of this chunk run
#pragma unroll
        for (int g = 0; g < 4; g++) {
            float4 a4[WM], b4[WN];
#pragma unroll
            for (int r = 0; r < WM; r++) a4[r] = *reinterpret_cast<const float4 *>(&As[wr + r * 32 + i][h * 16 + 4 * g]);
#pragma unroll
            for (int c = 0; c < WN; c++) b4[c] = *reinterpret_cast<const float4 *>(&Bs[wc + c * 32 + i][h * 16 + 4 * g]);
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int r = 0; r < WM; r++)
#pragma unroll
                    for (int c = 0; c < WN; c++)
                        acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(comp(a4[r], s), comp(b4[c], s), acc[r][c], 0, 0, 0);
        }
        lds_barrier();
    }
    conv_gemm_epilogue<WM, WN>(k, ph, acc, img0, rows, hwg, r0, c0, wr, wc, i, h);
}

// ---- 16-bit operands ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
// float -> T is the compiler's conversion, which rounds to nearest even (v_cvt_pk_bf16_f32, v_cvt_f16_f32)
template <typename T> struct Op16;
template <> struct Op16<__bf16> {
    typedef bf16x8 v8;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Op16<_Float16> {
    typedef f16x8 v8;
    static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <typename T> __device__ __forceinline__ typename Op16<T>::v8 round8(const float4 &a, const float4 &b)
{
    typename Op16<T>::v8 v;
    v[0] = (T)a.x; v[1] = (T)a.y; v[2] = (T)a.z; v[3] = (T)a.w;
    v[4] = (T)b.x; v[5] = (T)b.y; v[6] = (T)b.z; v[7] = (T)b.w;
    return v;
}

constexpr int BK16 = 64;           // k per chunk
// LDS row pitch in 16-bit elements: 144 bytes, nine 16-byte slots.  A fragment read is one ds_read_b128 per lane: lane (i, h) reads
// slot 9 (row0 + i) + 2 s + h.  That instruction is served in groups of 16 lanes of one h whose i cover every residue modulo 16
// ({0-3, 12-15, 20-27} and {4-11, 16-19, 28-31}), and a bank row is 16 slots wide: since 9 is odd, i -> 9 i mod 16 is one-to-one, the
// 16 lanes of a group hit 16 different slots and the read is conflict-free.  A staging write (ds_write_b128, groups of 8 consecutive
// lanes over a 128-byte bank row) stores one row's eight slots side by side: conflict-free as well.
constexpr int LDSK16 = BK16 + 8;

// conv_gemm_kernel with B read as 16-bit values T and A rounded to T (nearest even) on its way into LDS: the same tiles, waves, tap
// tables, padding and epilogue; the accumulators are float32.  K runs flat over (tap, cin) in chunks of 64; a staging thread moves
// groups of 8 elements (two float4 of A, one 16-byte load of B; rows tid >> 3 (+ 32 j), elements (tid & 7) * 8 .. + 8 of the chunk),
// which never straddle a tap; groups behind K, rows behind M and columns behind Cout are zeros.  One LDS buffer, as above.
// Lane (i, h): row / column i of a 32 x 32 block, k half h.  Step s = 0 .. 3 of a chunk is one v_mfma_f32_32x32x16, which adds the
// sixteen products k = 16 s .. 16 s + 15 of the chunk to the accumulator (lane half h supplies k = 16 s + 8 h + j, j = 0 .. 7); how
// the instruction orders those sixteen is the hardware's, and the same for every output.  So every output's sum runs chunk by chunk
// and inside a chunk step by step, whatever WM, WN, its place in the tile and the batch.
template <typename T, int WM, int WN>
__global__ void __launch_bounds__(256) conv_gemm16_kernel(ConvGemm k)
{
    typedef typename Op16<T>::v8 v8;
    constexpr int BM = 64 * WM, BN = 64 * WN;
    __shared__ __attribute__((aligned(16))) T As[BM][LDSK16], Bs[BN][LDSK16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ConvTaps &ph = k.ph[blockIdx.y];
    // Workgroups go to the chip's eight XCDs in turn, each with an L2 of its own.  The tiles are dealt so that an XCD gets a
    // contiguous run of them: the column tiles of a row tile, which read the same A, and the row tiles next to it, which share its
    // halo, then find A in their L2 instead of each fetching it from the Infinity Cache (measured: DESIGN.md 9y).  XCD x's run
    // starts at x q + min(x, r) for 8 q + r tiles: one-to-one.  Which workgroup computes a tile changes no sum.
    const unsigned ntile = gridDim.x, xcd = blockIdx.x % 8, rem = ntile % 8;
    const unsigned tile = xcd * (ntile / 8) + (xcd < rem ? xcd : rem) + blockIdx.x / 8;
    const int tn = (int)(tile % (unsigned)k.tiles_n);
    int tm = (int)(tile / (unsigned)k.tiles_n);
    const int hwg = k.Hg * k.Wg;
    int img0 = 0, rows = k.N * hwg;
    if (k.per_image) { img0 = tm / k.tiles_img; tm -= img0 * k.tiles_img; rows = hwg; }
    const int r0 = tm * BM, c0 = tn * BN;
    const int Kp = ph.ntaps * k.Cin, nch = (Kp + BK16 - 1) / BK16;
    const int dm = k.dil - 1;

    const int srow = tid >> 3, sk = (tid & 7) * 8;
    bool av[2 * WM];
    int gy[2 * WM], gx[2 * WM];
    size_t abase[2 * WM];
#pragma unroll
    for (int j = 0; j < 2 * WM; j++) {
        const int r = r0 + srow + 32 * j;
        av[j] = r < rows;
        const int n = av[j] ? r / hwg : 0;
        const int q = av[j] ? r - n * hwg : 0;
        gy[j] = q / k.Wg;
        gx[j] = q - gy[j] * k.Wg;
        abase[j] = (size_t)(img0 + n) * k.xim;
    }
    const T *wrow[2 * WN];
    bool bv[2 * WN];
#pragma unroll
    for (int j = 0; j < 2 * WN; j++) {
        const int co = c0 + srow + 32 * j;
        bv[j] = co < k.Cout;
        wrow[j] = reinterpret_cast<const T *>(ph.w) + (size_t)img0 * k.wbat + (size_t)(bv[j] ? co : 0) * ph.ldw;
    }

    float4 na[2 * WM][2];
    v8 nb[2 * WN];
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int ch) {
        const int kk = ch * BK16 + sk;
        const bool kv = kk < Kp;
        const int t = kv ? kk / k.Cin : 0;
        const int ci = kk - t * k.Cin;
        const int dy = ph.dy[t], dx = ph.dx[t];
#pragma unroll
        for (int j = 0; j < 2 * WM; j++) {
            int iy = gy[j] * k.stride + dy, ix = gx[j] * k.stride + dx;
            bool ok = kv && av[j];
            ok = ok && !((iy | ix) & dm);
            iy >>= dm; ix >>= dm;
            if (k.reflect) { iy = mirror(iy, k.Hin); ix = mirror(ix, k.Win); }
            else ok = ok && iy >= 0 && iy < k.Hin && ix >= 0 && ix < k.Win;
            if (ok) {
                const float4 *s = reinterpret_cast<const float4 *>(k.x + (abase[j] + (size_t)iy * k.Win + ix) * k.ldx + ci);
                na[j][0] = s[0];
                na[j][1] = s[1];
            } else {
                na[j][0] = na[j][1] = zero4;
            }
        }
#pragma unroll
        for (int j = 0; j < 2 * WN; j++) {
            if (kv && bv[j]) nb[j] = *reinterpret_cast<const v8 *>(wrow[j] + kk);
            else
#pragma unroll
                for (int e = 0; e < 8; e++) nb[j][e] = (T)0.f;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int j = 0; j < 2 * WM; j++) *reinterpret_cast<v8 *>(&As[srow + 32 * j][sk]) = round8<T>(na[j][0], na[j][1]);
#pragma unroll
        for (int j = 0; j < 2 * WN; j++) *reinterpret_cast<v8 *>(&Bs[srow + 32 * j][sk]) = nb[j];
    };

    const int i = lane & 31, h = lane >> 5;
    const int wr = (wave >> 1) * 32 * WM, wc = (wave & 1) * 32 * WN;
    f32x16 acc[WM][WN];
#pragma unroll
    for (int r = 0; r < WM; r++)
#pragma unroll
        for (int c = 0; c < WN; c++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[r][c][e] = 0.f;

    fetch(0);
    for (int ch = 0; ch < nch; ch++) {
        stage();
        lds_barrier();
        if (ch + 1 < nch) fetch(ch + 1);            // in flight while the MFMAs of this chunk run
#pragma unroll
        for (int s = 0; s < BK16 / 16; s++) {
            v8 a8[WM], b8[WN];
#pragma unroll
            for (int r = 0; r < WM; r++) a8[r] = *reinterpret_cast<const v8 *>(&As[wr + r * 32 + i][s * 16 + h * 8]);
#pragma unroll
            for (int c = 0; c < WN; c++) b8[c] = *reinterpret_cast<const v8 *>(&Bs[wc + c * 32 + i][s * 16 + h * 8]);
#pragma unroll
            for (int r = 0; r < WM; r++)
#pragma unroll
                for (int c = 0; c < WN; c++) acc[r][c] = Op16<T>::mfma(a8[r], b8[c], acc[r][c]);
        }
        lds_barrier();
    }
    conv_gemm_epilogue<WM, WN>(k, ph, acc, img0, rows, hwg, r0, c0, wr, wc, i, h);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// what the kernel takes for granted of a descriptor with rows (conv_gemm.h); false and set_error where it does not hold
bool check_desc(const ConvGemm &k, int64_t M)
{
    if (k.N < 0 || k.Hg < 0 || k.Wg < 0 || M > (int64_t(1) << 30) || k.Cin < 8 || k.Cin % 8 || k.nph < 1 || k.nph > 4 || (!k.per_image && k.wbat)) {
        set_error("conv_gemm: need at most 2^30 rows, Cin a multiple of 8, 1 .. 4 tap tables, B per image only with tiles per image "
                  "(rows=%lld, Cin=%d, nph=%d)", (long long)M, k.Cin, k.nph);
        return false;
    }
    if ((k.dil != 1 && k.dil != 2) || (k.dil == 2 && k.reflect)) {
        set_error("conv_gemm: dil must be 1, or 2 with zero padding (dil=%d, reflect=%d)", k.dil, k.reflect);
        return false;
    }
    if (k.act < 0 || k.act > ACT_RELU) { set_error("conv_gemm: act must be 0 (none), 1 (GELU) or 2 (ReLU) (got %d)", k.act); return false; }
    if (k.slope && k.act != ACT_NONE) { set_error("conv_gemm: slope (PReLU) goes with act == 0 only (got act=%d)", k.act); return false; }
    if (k.wtype < 0 || k.wtype > WT_F16) { set_error("conv_gemm: wtype must be 0 (f32), 1 (bf16) or 2 (f16) (got %d)", k.wtype); return false; }
    if (k.stride < 1 || k.os < 1 || k.Cout < 1 || k.Hin < 1 || k.Win < 1) {
        set_error("conv_gemm: stride, os, Cout, Hin and Win must be at least 1 (stride=%d, os=%d, Cout=%d, Hin=%d, Win=%d)", k.stride, k.os,
                  k.Cout, k.Hin, k.Win);
        return false;
    }
    if (!k.x || !k.y) { set_error("conv_gemm: NULL %s", k.x ? "y" : "x"); return false; }
    if (!aligned16(k.x) || k.ldx % 4 || k.wbat % 4) {
        set_error("conv_gemm: x must be 16-byte aligned, ldx and wbat multiples of 4: the loads are float4 (x=%p, ldx=%lld, wbat=%lld)",
                  (const void *)k.x, (long long)k.ldx, (long long)k.wbat);
        return false;
    }
    if (k.wtype && k.wbat % 8) {
        set_error("conv_gemm: with 16-bit weights wbat must be a multiple of 8: the loads are 8 elements (wbat=%lld, wtype=%d)",
                  (long long)k.wbat, k.wtype);
        return false;
    }
    for (int p = 0; p < k.nph; p++) {
        const ConvTaps &t = k.ph[p];
        if (t.ntaps < 1 || t.ntaps > 9) { set_error("conv_gemm: tap table %d: ntaps must be 1 .. 9 (got %d)", p, t.ntaps); return false; }
        if (t.py < 0 || t.py >= k.os || t.px < 0 || t.px >= k.os) {
            set_error("conv_gemm: tap table %d: py and px must lie in [0, os) (py=%d, px=%d, os=%d)", p, t.py, t.px, k.os);
            return false;
        }
        if (!t.w) { set_error("conv_gemm: tap table %d: NULL w", p); return false; }
        if (!aligned16(t.w) || t.ldw % 4) {
            set_error("conv_gemm: tap table %d: w must be 16-byte aligned and ldw a multiple of 4: the loads are float4 (w=%p, ldw=%lld)", p,
                      (const void *)t.w, (long long)t.ldw);
            return false;
        }
        if (k.wtype && t.ldw % 8) {
            set_error("conv_gemm: tap table %d: with 16-bit weights ldw must be a multiple of 8: the loads are 8 elements (ldw=%lld, "
                      "wtype=%d)", p, (long long)t.ldw, k.wtype);
            return false;
        }
        if (!k.reflect) continue;
        // mirror() reflects once: a coordinate further out than the image is wide would land outside it again
        int dy0 = t.dy[0], dy1 = t.dy[0], dx0 = t.dx[0], dx1 = t.dx[0];
        for (int i = 1; i < t.ntaps; i++) {
            dy0 = t.dy[i] < dy0 ? t.dy[i] : dy0; dy1 = t.dy[i] > dy1 ? t.dy[i] : dy1;
            dx0 = t.dx[i] < dx0 ? t.dx[i] : dx0; dx1 = t.dx[i] > dx1 ? t.dx[i] : dx1;
        }
        const int64_t y1 = (int64_t)(k.Hg - 1) * k.stride + dy1, x1 = (int64_t)(k.Wg - 1) * k.stride + dx1;
        if (dy0 < -(k.Hin - 1) || y1 > 2 * (int64_t)(k.Hin - 1) || dx0 < -(k.Win - 1) || x1 > 2 * (int64_t)(k.Win - 1)) {
            set_error("conv_gemm: tap table %d: reflect mirrors once: rows %d .. %lld of a %d-row input, columns %d .. %lld of a %d-column "
                      "input must lie in [-(n - 1), 2 (n - 1)]", p, dy0, (long long)y1, k.Hin, dx0, (long long)x1, k.Win);
            return false;
        }
    }
    return true;
}

}  // namespace

// 128 x 128 tiles where they still fill the chip (256 compute units), 64 x 64 otherwise; the sums' order is the same
int conv_gemm_tile(const ConvGemm &k)
{
    const int64_t M = (int64_t)k.N * k.Hg * k.Wg;
    const int64_t big = (M + 127) / 128 * ((k.Cout + 127) / 128) * k.nph;
    return !k.per_image && big >= 256 && k.Cout >= 128 ? 128 : 64;
}

int launch_conv_gemm(const ConvGemm &desc, hipStream_t stream)
{
    ConvGemm k = desc;
    const int64_t hwg = (int64_t)k.Hg * k.Wg, M = k.N * hwg;
    if (M == 0) return 0;
    if (!check_desc(k, M)) return 1;
    const int bt = conv_gemm_tile(k);
    const bool big_tiles = bt == 128;
    k.tiles_n = (k.Cout + bt - 1) / bt;
    k.tiles_img = (int)((hwg + bt - 1) / bt);
    const int64_t tiles = (k.per_image ? (int64_t)k.N * k.tiles_img : (M + bt - 1) / bt) * k.tiles_n;
    const dim3 grid((unsigned)tiles, (unsigned)k.nph);
    if (k.wtype == WT_BF16) {
        if (big_tiles) hipLaunchKernelGGL((conv_gemm16_kernel<__bf16, 2, 2>), grid, dim3(256), 0, stream, k);
        else hipLaunchKernelGGL((conv_gemm16_kernel<__bf16, 1, 1>), grid, dim3(256), 0, stream, k);
    } else if (k.wtype == WT_F16) {
        if (big_tiles) hipLaunchKernelGGL((conv_gemm16_kernel<_Float16, 2, 2>), grid, dim3(256), 0, stream, k);
        else hipLaunchKernelGGL((conv_gemm16_kernel<_Float16, 1, 1>), grid, dim3(256), 0, stream, k);
    } else if (big_tiles) hipLaunchKernelGGL((conv_gemm_kernel<2, 2>), grid, dim3(256), 0, stream, k);
    else hipLaunchKernelGGL((conv_gemm_kernel<1, 1>), grid, dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("conv_gemm", stream, 0);
    return 0;
}

int launch_conv_pack16(const float *w, void *fwd, int Cout, int Cin, int Cinp, int kk, int wtype, hipStream_t stream)
{
    if (wtype != WT_BF16 && wtype != WT_F16) { set_error("conv_pack16: wtype must be 1 (bf16) or 2 (f16) (got %d)", wtype); return 1; }
    const dim3 grid(blocks((int64_t)Cout * kk * Cinp));
    if (wtype == WT_BF16) hipLaunchKernelGGL(conv_pack16_kernel<__bf16>, grid, dim3(256), 0, stream, w, static_cast<__bf16 *>(fwd), Cout, Cin, Cinp, kk);
    else hipLaunchKernelGGL(conv_pack16_kernel<_Float16>, grid, dim3(256), 0, stream, w, static_cast<_Float16 *>(fwd), Cout, Cin, Cinp, kk);
    SOAR_LAUNCH_OK("conv_pack16", stream, 0);
    return 0;
}

int launch_conv_pack16_bwd(const float *w, void *bwd, int Cout, int Cin, int kk, int64_t ldb, int cols, int wtype, hipStream_t stream)
{
    if (wtype != WT_BF16 && wtype != WT_F16) { set_error("conv_pack16_bwd: wtype must be 1 (bf16) or 2 (f16) (got %d)", wtype); return 1; }
    if (cols < Cout || cols > ldb || ldb % 8) {
        set_error("conv_pack16_bwd: need Cout <= cols <= ldb and ldb a multiple of 8 (Cout=%d, cols=%d, ldb=%lld)", Cout, cols, (long long)ldb);
        return 1;
    }
    const dim3 grid(blocks((int64_t)Cin * kk * cols));
    if (wtype == WT_BF16)
        hipLaunchKernelGGL(conv_pack16_bwd_kernel<__bf16>, grid, dim3(256), 0, stream, w, static_cast<__bf16 *>(bwd), Cout, Cin, kk, ldb, cols);
    else
        hipLaunchKernelGGL(conv_pack16_bwd_kernel<_Float16>, grid, dim3(256), 0, stream, w, static_cast<_Float16 *>(bwd), Cout, Cin, kk, ldb, cols);
    SOAR_LAUNCH_OK("conv_pack16_bwd", stream, 0);
    return 0;
}

int launch_conv_pack(const float *w, float *fwd, float *bwd, int Cout, int Cin, int kk, int64_t ldb, hipStream_t stream)
{
    hipLaunchKernelGGL(conv_pack_kernel, dim3(blocks((int64_t)Cout * Cin * kk)), dim3(256), 0, stream, w, fwd, bwd, Cout, Cin, kk, ldb);
    SOAR_LAUNCH_OK("conv_pack", stream, 0);
    return 0;
}

}  // namespace soar

// ---- the launcher and the packer by themselves (tests/test_conv_gemm_*.py) ----
static int selftest_conv_gemm(const char *me, const SoarConvGemmArgs *a, int wtype, int act, int32_t *tile_out, void *stream_,
                              const float *slope = nullptr)
{
    if (!a || !tile_out) { soar::set_error("%s: NULL %s", me, a ? "tile_out" : "args"); return 1; }
    soar::ConvGemm k{};
    k.wtype = wtype; k.act = act; k.slope = slope;
    k.x = a->x; k.ldx = a->ldx; k.xim = a->xim; k.wbat = a->wbat;
    k.bias = a->bias; k.res = a->res; k.y = a->y; k.ldy = a->ldy; k.yim = a->yim; k.alpha = a->alpha;
    k.N = a->N; k.Hg = a->Hg; k.Wg = a->Wg; k.Hin = a->Hin; k.Win = a->Win; k.Cin = a->Cin; k.Cout = a->Cout;
    k.stride = a->stride; k.dil = a->dil; k.reflect = a->reflect; k.Wout = a->Wout; k.os = a->os;
    k.per_image = a->per_image; k.nph = a->nph;
    for (int p = 0; p < 4; p++) {
        const SoarConvGemmTaps &s = a->ph[p];
        soar::ConvTaps &t = k.ph[p];
        t.w = s.w; t.ldw = s.ldw; t.ntaps = s.ntaps; t.py = s.py; t.px = s.px;
        for (int i = 0; i < 9; i++) { t.dy[i] = s.dy[i]; t.dx[i] = s.dx[i]; }
    }
    *tile_out = soar::conv_gemm_tile(k);
    return soar::launch_conv_gemm(k, static_cast<hipStream_t>(stream_));
}

extern "C" int soar_selftest_conv_gemm(const SoarConvGemmArgs *a, int32_t *tile_out, void *stream_)
{
    return selftest_conv_gemm("soar_selftest_conv_gemm", a, soar::WT_F32, soar::ACT_NONE, tile_out, stream_);
}

// the taps' w read as 16-bit values of wtype (1 bf16, 2 f16; anything else is the launcher's refusal)
extern "C" int soar_selftest_conv_gemm16(const SoarConvGemmArgs *a, int32_t wtype, int32_t *tile_out, void *stream_)
{
    if (wtype == soar::WT_F32) { soar::set_error("soar_selftest_conv_gemm16: wtype must be 1 (bf16) or 2 (f16) (got %d)", wtype); return 1; }
    return selftest_conv_gemm("soar_selftest_conv_gemm16", a, wtype, soar::ACT_NONE, tile_out, stream_);
}

// SoarConvGemmArgs carries no activation: the descriptor at either operand type (wtype 0 .. 2) with act (0 none, 1 GELU, 2 ReLU)
extern "C" int soar_selftest_conv_gemm_act(const SoarConvGemmArgs *a, int32_t wtype, int32_t act, int32_t *tile_out, void *stream_)
{
    return selftest_conv_gemm("soar_selftest_conv_gemm_act", a, wtype, act, tile_out, stream_);
}

// ... and with the epilogue's PReLU: slope [Cout] (NULL: off); the launcher refuses a slope together with act != 0
extern "C" int soar_selftest_conv_gemm_slope(const SoarConvGemmArgs *a, int32_t wtype, int32_t act, const float *slope, int32_t *tile_out,
                                             void *stream_)
{
    return selftest_conv_gemm("soar_selftest_conv_gemm_slope", a, wtype, act, tile_out, stream_, slope);
}

extern "C" int soar_selftest_conv_pack16(const float *w, void *fwd, int32_t Cout, int32_t Cin, int32_t Cinp, int32_t kk, int32_t wtype,
                                         void *stream_)
{
    if (!w || !fwd || Cout < 1 || Cin < 1 || kk < 1 || Cinp < Cin) {
        soar::set_error("soar_selftest_conv_pack16: need w, fwd, positive sizes and Cinp >= Cin (Cout=%d, Cin=%d, Cinp=%d, kk=%d)", Cout, Cin,
                        Cinp, kk);
        return 1;
    }
    return soar::launch_conv_pack16(w, fwd, Cout, Cin, Cinp, kk, wtype, static_cast<hipStream_t>(stream_));
}

// the data gradient's form, every column 0 .. ldb - 1 written (Cout .. ldb - 1 zeros)
extern "C" int soar_selftest_conv_pack16_bwd(const float *w, void *bwd, int32_t Cout, int32_t Cin, int32_t kk, int64_t ldb, int32_t wtype,
                                             void *stream_)
{
    if (!w || !bwd || Cout < 1 || Cin < 1 || kk < 1 || ldb < Cout || ldb % 8 || ldb > INT32_MAX) {
        soar::set_error("soar_selftest_conv_pack16_bwd: need w, bwd, positive sizes and ldb >= Cout, a multiple of 8 (Cout=%d, Cin=%d, kk=%d, "
                        "ldb=%lld)", Cout, Cin, kk, (long long)ldb);
        return 1;
    }
    return soar::launch_conv_pack16_bwd(w, bwd, Cout, Cin, kk, ldb, (int)ldb, wtype, static_cast<hipStream_t>(stream_));
}

extern "C" int soar_selftest_conv_pack(const float *w, float *fwd, float *bwd, int32_t Cout, int32_t Cin, int32_t kk, int64_t ldb,
                                       void *stream_)
{
    if (!w || !fwd || Cout < 1 || Cin < 1 || kk < 1 || (bwd && ldb < Cout)) {
        soar::set_error("soar_selftest_conv_pack: need w, fwd, positive sizes and ldb >= Cout (Cout=%d, Cin=%d, kk=%d, ldb=%lld)", Cout, Cin,
                        kk, (long long)ldb);
        return 1;
    }
    return soar::launch_conv_pack(w, fwd, bwd, Cout, Cin, kk, ldb, static_cast<hipStream_t>(stream_));
}
