// conv_gemm.h -- the implicit-GEMM convolution and the weight packer that the convolutional networks share (lpips.hip, vae.hip,
// normalnet.hip), the plain matrix product through it that is every linear layer of the transformers (sam.hip, unet.hip,
// clip.hip), its form with 16-bit operands (bf16 / f16), and the small pieces every kernel on v_mfma_f32_32x32x2_f32
// needs (attention.hip among them).
#pragma once

#include "soar_common.h"

namespace soar {

// One tap table: output (gy os + py, gx os + px) of grid row (n, gy, gx) sums, tap by tap, input (gy stride + dy, gx stride + dx)
// times w[co][tap][ci].  A 1 x 1 convolution and a plain matrix product are a table of one entry.
struct ConvTaps {
    const float *w;                // B: row co at w + image wbat + co ldw, k = tap Cin + ci (wtype != 0: 16-bit values behind this
                                   //   pointer, ldw and wbat counted in elements all the same)
    int64_t ldw;
    int ntaps, py, px;
    signed char dy[9], dx[9];
};
// a square kernel of side x side taps, tap (ky, kx) at offset (ky + off, kx + off)
inline void square_taps(ConvTaps &p, const float *w, int64_t ldw, int side, int off)
{
    p.w = w; p.ldw = ldw; p.ntaps = side * side; p.py = p.px = 0;
    for (int t = 0; t < side * side; t++) { p.dy[t] = (signed char)(t / side + off); p.dx[t] = (signed char)(t % side + off); }
}

enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2 };
// what B holds, and what A is rounded to (nearest even) on its way into LDS; the sums and the epilogue are float32 either way
enum { WT_F32 = 0, WT_BF16 = 1, WT_F16 = 2 };

// y = act(alpha * (A B^T) + bias) + res.  A row is one grid position's (tap, cin) window of x, gathered on load; nothing padded or
// zero-dilated is ever materialised.
struct ConvGemm {
    const float *x;                // A: image n's pixel (iy, ix) at x + (n xim + iy Win + ix) ldx, Cin floats (a multiple of 8, 16-byte aligned)
    int64_t ldx, xim;
    int64_t wbat;                  // B's per-image offset (per_image only)
    const float *bias;             // [Cout] or NULL
    const float *res;              // indexed as y, or NULL
    float *y;                      // image n's output pixel (oy, ox) at y + (n yim + oy Wout + ox) ldy, Cout floats
    int64_t ldy, yim;
    float alpha;
    int N, Hg, Wg;                 // the grid a row walks: N Hg Wg rows, at most 2^30
    int Hin, Win, Cin, Cout;
    int stride, dil;               // dil = 1, or 2: the input is x zero-dilated by two (odd coordinates load zeros, even ones x at half;
                                   //   with zero padding only)
    int reflect;                   // outside the input: mirrored (reflect) or zero
    int Wout, os;
    int per_image;                 // 1: 64 x 64 tiles that never cross an image (B and the padded row count may then be per image);
                                   // 0: tiles over the batch's flat rows, 128 x 128 where those still fill the chip
    int nph;                       // tap tables in use: gridDim.y picks one (the phases of a transposed convolution)
    ConvTaps ph[4];
    int tiles_n, tiles_img;        // (the launcher's)
    int act;                       // ACT_NONE (0: what a zero-initialised descriptor asks for), ACT_GELU (exact, erf) or ACT_RELU
    int wtype;                     // WT_F32 (0: what a zero-initialised descriptor asks for), WT_BF16 or WT_F16: conv_gemm16_kernel
    const float *slope;            // [Cout] or NULL (off: what a zero-initialised descriptor asks for).  PReLU, with act == ACT_NONE only:
                                   //   y = (v > 0 ? v : slope[co] v) + res with v = alpha acc + bias, at every wtype
};
// Refuses (set_error, 1, nothing launched) a descriptor the kernel cannot run: more than 2^30 rows; Cin no multiple of 8; nph outside
// 1 .. 4; act outside 0 .. 2; wbat without per_image; dil not 1 or 2, or 2 with reflect; stride, os, Cout, Hin or Win below 1; x, y or a table's w NULL; x
// or w off 16 bytes, or ldx, ldw, wbat no multiple of 4 (the loads are float4); a table with ntaps outside 1 .. 9 or py, px outside
// [0, os); with reflect, a coordinate gy stride + dy outside [-(Hin - 1), 2 (Hin - 1)] (mirror() reflects once), likewise along x;
// a wtype outside 0 .. 2; with wtype != 0, ldw or wbat no multiple of 8 (B's loads are 8 elements of 16 bits); a slope with act != 0.
int launch_conv_gemm(const ConvGemm &desc, hipStream_t stream);
// the side of the tile launch_conv_gemm picks for desc: 128 or 64
int conv_gemm_tile(const ConvGemm &desc);

// A plain matrix product, a table of one tap: y [N][rows][Cout] = act(alpha x [N][rows][K] w[Cout][K]^T + bias) + res, image n's rows
// at x + n xim ldx and y + n yim ldy (one image: every row ldx, ldy apart).  wtype: what w holds, 16-bit values behind the float pointer.
inline int gemm(const float *x, int64_t ldx, const float *w, int K, int Cout, const float *bias, const float *res, float *y, int64_t ldy,
                int64_t rows, hipStream_t stream, int act = ACT_NONE, int wtype = WT_F32, int N = 1, int64_t xim = 0, int64_t yim = 0,
                float alpha = 1.f)
{
    ConvGemm k{};
    k.x = x; k.ldx = ldx; k.xim = xim; k.bias = bias; k.res = res; k.y = y; k.ldy = ldy; k.yim = yim; k.alpha = alpha;
    k.N = N; k.Hg = 1; k.Wg = (int)rows; k.Hin = 1; k.Win = (int)rows; k.Cin = K; k.Cout = Cout; k.stride = 1; k.dil = 1; k.Wout = (int)rows; k.os = 1;
    k.nph = 1; k.act = act; k.wtype = wtype;
    square_taps(k.ph[0], w, K, 1, 0);
    return launch_conv_gemm(k, stream);
}

// torch [Cout][Cin][kk] -> fwd [Cout][kk][Cin] and, unless bwd is NULL, the data gradient's form, spatially flipped and transposed:
// bwd[(ci kk + kk - 1 - t) ldb + co]
int launch_conv_pack(const float *w, float *fwd, float *bwd, int Cout, int Cin, int kk, int64_t ldb, hipStream_t stream);

// torch [Cout][Cin][kk] float32 -> fwd [Cout][kk][Cinp] of wtype's 16-bit type, rounded to nearest even, channels Cin .. Cinp - 1
// zeros; kk = 1 converts a linear layer's matrix.
int launch_conv_pack16(const float *w, void *fwd, int Cout, int Cin, int Cinp, int kk, int wtype, hipStream_t stream);
// ... and the data gradient's form in the same type and rounding, launch_conv_pack's bwd: bwd[(ci kk + kk - 1 - t) ldb + co].  ldb is a
// multiple of 8 (conv_gemm16_kernel's loads); columns 0 .. cols - 1 of every row are written, Cout .. cols - 1 as zeros (cols = ldb:
// the whole row; cols = Cout: one column block of a wider matrix, the others left alone).
int launch_conv_pack16_bwd(const float *w, void *bwd, int Cout, int Cin, int kk, int64_t ldb, int cols, int wtype, hipStream_t stream);

inline unsigned blocks(int64_t threads) { return (unsigned)((threads + 255) / 256); }

#if defined(__HIPCC__)
typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int BK = 32;             // k per chunk
constexpr int LDSK = BK + 4;       // LDS row pitch in floats: rows 16 B apart in bank space, float4 reads conflict-free per quarter wave

__device__ __forceinline__ float comp(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
// C / D of the 32 x 32 MFMA: lane l holds column l & 31; its register e is row (e & 3) + 8 (e >> 2) + 4 h with h = l >> 5
__device__ __forceinline__ int mfma_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }
__device__ __forceinline__ int mirror(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
#endif

}  // namespace soar
