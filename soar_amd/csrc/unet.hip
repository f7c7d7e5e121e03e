// unet.hip -- the multi-view diffusion UNet of the SDS guidance, forward only, float32 (soar_amd/unet.py).
//
//   kv_attn_kernel         (attention.hip) self-attention over the views of a group and cross-attention with the text and image tokens
//   unet_gn_stats_kernel   GroupNorm (32 groups, any channels per group) mean and rstd of one (image, group) in double, fixed order;
//   unet_gn_apply_kernel   y = silu?((x (+ e[n][c]) - mean) rstd gamma + beta): the ResBlock's embedding term rides in on the read
//   ln_rows_kernel         (layer_norm.h)
//   unet_sum3_kernel       the three partial results of a small 3 x 3 convolution split by kernel rows (conv3x3 below), bias, residual
//   the rest               input staging (any strides, channels padded to 8), the sinusoidal embedding, SiLU, GEGLU's product, the
//                          concatenation with a skip, nearest 2 x up-sampling: plain VALU kernels
// Every matrix product (convolutions, linear layers: gemm()) is launch_conv_gemm (conv_gemm.h).  Activations are channels-last [N][H W][C].
// SoarUnetConfig::precision 1 (bf16) or 2 (f16): the products' weights are packed as 16-bit values and every product runs on the
// 16-bit matrix core, its A operand rounded on load (conv_gemm16_kernel); everything else, the activations in memory
// included, stays float32.  SoarUnetConfig::attn_precision 1 or 2, independently: both attentions run as kv_attn16_kernel
// (attention.h's contract).
// No atomics; no sum's order depends on the batch: a group's result does not depend on the other groups.
#include "attention.h"
#include "layer_norm.h"
#include "net_weights.h"
#include "workspace.h"

namespace soar {
namespace {

constexpr int GN_GROUPS = 32;
constexpr int CIN0 = 8;                // the first convolution's input channels, padded for the shared GEMM

// ---- the plan: blocks in the order they run, and where their tensors lie in the packed buffer -------------------------------------
struct Blk {
    int level = 0;                     // the resolution of the block's input: H >> level
    int cin = 0, cout = 0;             // cin includes skip_ch
    int res = -1, tr = -1, conv = -1;  // first tensor of the ResBlock, of the transformer, of the lone / down / up convolution
    int res2 = -1;                     // the middle block's second ResBlock
    int skip_ch = 0;                   // output blocks: channels of the skip concatenated behind h
    bool down = false, up = false;
};
struct Repack { int idx, Cout, Cin, Cinp; };
struct Plan : WeightPlan {             // (mat: the B operand of a gemm() or conv3x3())
    std::vector<Repack> convs;         // the 3 x 3 convolutions
    std::vector<Blk> in, out;
    Blk mid;
    int time0 = 0, cam0 = -1, out0 = 0;
    int tr_tail = 16;                  // the transformer's tensors behind attn2's keys and values start here
};

Plan make_plan(const SoarUnetConfig &c)
{
    Plan P;
    const size_t E = (size_t)4 * c.model_channels, ctx = c.context_dim;
    P.half = c.precision != WT_F32;    // a product's B operand as 16-bit values
    auto add = [&](size_t n, size_t packed = 0, bool mat = false) { return P.add(n, packed, mat); };
    auto mat = [&](size_t n) { return add(n, 0, true); };
    auto conv3 = [&](int Cout, int Cin, int Cinp) {
        const int i = add((size_t)Cout * Cin * 9, (size_t)Cout * Cinp * 9, true);
        P.convs.push_back({i, Cout, Cin, Cinp});
        add(Cout);
        return i;
    };
    auto res = [&](int cin, int cout) {
        const int i = add(cin); add(cin); conv3(cout, cin, cin); mat((size_t)cout * E); add(cout); add(cout); add(cout); conv3(cout, cout, cout);
        if (cin != cout) { mat((size_t)cout * cin); add(cout); }
        return i;
    };
    auto tr = [&](int C) {
        const size_t CC = (size_t)C * C;
        // (q | k | v of attn1, k | v of attn2 and of the image tokens are each read as one matrix: C C and C ctx are multiples of 8,
        // so they lie one behind the other in 16 bits as in 32)
        const int i = add(C); add(C); mat(CC); add(C);
        add(C); add(C); mat(CC); mat(CC); mat(CC); mat(CC); add(C);
        add(C); add(C); mat(CC); mat(C * ctx); mat(C * ctx);
        if (c.with_ip) { mat(C * ctx); mat(C * ctx); }
        mat(CC); add(C); add(C); add(C); mat(8 * CC); add((size_t)8 * C); mat(4 * CC); add(C); mat(CC); add(C);
        return i;
    };
    P.tr_tail = c.with_ip ? 18 : 16;
    const int mc = c.model_channels;
    P.time0 = mat(E * mc); add(E); mat(E * E); add(E);
    if (c.camera_dim) { P.cam0 = mat(E * c.camera_dim); add(E); mat(E * E); add(E); }
    std::vector<int> chans;
    Blk b0;
    b0.cin = c.in_channels; b0.cout = mc; b0.conv = conv3(mc, c.in_channels, CIN0);
    P.in.push_back(b0);
    chans.push_back(mc);
    int ch = mc;
    for (int l = 0; l < c.levels; l++) {
        for (int r = 0; r < c.num_res_blocks; r++) {
            Blk b;
            b.level = l; b.cin = ch; b.cout = mc * c.channel_mult[l];
            b.res = res(b.cin, b.cout);
            if (c.attention[l]) b.tr = tr(b.cout);
            ch = b.cout;
            P.in.push_back(b);
            chans.push_back(ch);
        }
        if (l != c.levels - 1) {
            Blk b;
            b.level = l; b.cin = b.cout = ch; b.down = true; b.conv = conv3(ch, ch, ch);
            P.in.push_back(b);
            chans.push_back(ch);
        }
    }
    P.mid.level = c.levels - 1; P.mid.cin = P.mid.cout = ch;
    P.mid.res = res(ch, ch); P.mid.tr = tr(ch); P.mid.res2 = res(ch, ch);
    for (int l = c.levels - 1; l >= 0; l--)
        for (int r = 0; r <= c.num_res_blocks; r++) {
            Blk b;
            b.level = l; b.skip_ch = chans.back(); chans.pop_back();
            b.cin = ch + b.skip_ch; b.cout = mc * c.channel_mult[l];
            b.res = res(b.cin, b.cout);
            if (c.attention[l]) b.tr = tr(b.cout);
            ch = b.cout;
            if (l > 0 && r == c.num_res_blocks) { b.up = true; b.conv = conv3(ch, ch, ch); }
            P.out.push_back(b);
        }
    P.out0 = add(ch); add(ch); conv3(c.out_channels, ch, ch);
    return P;
}

bool check_cfg(const SoarUnetConfig *cp, const char *me)
{
    if (!cp) { set_error("%s: NULL cfg", me); return false; }
    const SoarUnetConfig &c = *cp;
    bool ok = c.in_channels >= 1 && c.in_channels <= CIN0 && c.out_channels >= 1 && c.out_channels <= 4096 && c.model_channels >= 32 &&
              c.model_channels <= 4096 && c.levels >= 1 && c.levels <= SOAR_UNET_MAX_LEVELS && c.num_res_blocks >= 1 && c.num_res_blocks <= 8 &&
              c.context_dim >= 8 && c.context_dim % 8 == 0 && c.camera_dim >= 0 && c.camera_dim % 8 == 0 && c.head_channels >= 4 &&
              c.head_channels <= 64 && c.head_channels % 4 == 0 && c.n_view >= 1 && c.n_view <= 64 && c.precision >= WT_F32 &&
              c.precision <= WT_F16 && c.attn_precision >= WT_F32 && c.attn_precision <= WT_F16;
    for (int l = 0; ok && l < c.levels; l++) {
        const int64_t ch = (int64_t)c.model_channels * c.channel_mult[l];
        ok = c.channel_mult[l] >= 1 && ch <= 8192 && ch % GN_GROUPS == 0 && ch % c.head_channels == 0;
    }
    if (!ok)
        set_error("%s: a configuration the kernels cannot run (in %d <= 8, out %d, model_channels=%d, %d levels, %d ResBlocks a level, "
                  "context_dim=%d, camera_dim=%d: multiples of 8, head_channels=%d: a multiple of 4 up to 64, n_view=%d; every level's "
                  "width a multiple of 32 and of head_channels; precision=%d and attn_precision=%d: 0 f32, 1 bf16 or 2 f16)", me, c.in_channels,
                  c.out_channels, c.model_channels, c.levels, c.num_res_blocks, c.context_dim, c.camera_dim, c.head_channels, c.n_view, c.precision,
                  c.attn_precision);
    return ok;
}

// the sizes of a call; an odd side at a level that is down-sampled is refused by the level's name
bool check_sizes(const SoarUnetConfig &c, int N, int H, int W, int T, int n_ip, const char *me)
{
    if (N < 0 || N > 65535 || N % c.n_view || H < 1 || W < 1 || H > 4096 || W > 4096 || T < 1 || T > 65535 || n_ip < 0 || n_ip > 65535 ||
        (n_ip && !c.with_ip)) {
        set_error("%s: need 0 <= N <= 65535, a multiple of n_view = %d, H and W in 1 .. 4096, T >= 1, and image tokens only where the "
                  "weights have to_k_ip (N=%d, %d x %d, T=%d, image tokens %d)", me, c.n_view, N, H, W, T, n_ip);
        return false;
    }
    int h = H, w = W;
    for (int l = 0; l + 1 < c.levels; l++) {
        if ((h | w) & 1) { set_error("%s: level %d is %d x %d: an odd side cannot be down-sampled and up-sampled back (latents %d x %d)", me, l, h, w, H, W); return false; }
        h >>= 1; w >>= 1;
    }
    return true;
}

// ---- the 3 x 3 convolutions -------------------------------------------------------------------------------------------------------
// 3 x 3, pad 1, stride 1 or 2: x [N][H][W][Cin] -> y [N][H / stride][W / stride][Cout] (+ bias + res).
// An output of at most SPLIT_PIXELS pixels an image (the two deepest levels of the shipped model: 128 and 512 rows against K up to
// 23,040) is too few rows to fill the chip as one product.  It runs as three, the kernel's rows of three taps each, in ONE launch --
// the tap tables of the shared GEMM, whose output parities lay the three results side by side in `part` [N][2 Ho][2 Wo][Cout] -- and
// conv_sum3 adds them in a fixed order with bias and residual.  Which form runs depends on the image's size alone, never on N.
constexpr int SPLIT_PIXELS = 64;
int conv_sum3(const float *part, const float *bias, const float *res, float *y, int N, int Ho, int Wo, int Cout, hipStream_t stream);
int conv3x3(const float *x, int Cin, const float *w, const float *bias, const float *res, float *y, int Cout, int N, int H, int W, int stride,
            float *part, int wtype, hipStream_t stream)
{
    const int Ho = H / stride, Wo = W / stride;
    const bool split = Ho * Wo <= SPLIT_PIXELS && Cout % 4 == 0;
    const int wsz = wtype ? 2 : 4;                               // bytes of an element of w
    ConvGemm k{};
    k.wtype = wtype;
    k.x = x; k.ldx = Cin; k.xim = (int64_t)H * W; k.alpha = 1.f;
    k.N = N; k.Hg = Ho; k.Wg = Wo; k.Hin = H; k.Win = W; k.Cin = Cin; k.Cout = Cout; k.stride = stride; k.dil = 1;
    if (!split) {
        k.bias = bias; k.res = res; k.y = y; k.ldy = Cout; k.yim = (int64_t)Ho * Wo; k.Wout = Wo; k.os = 1; k.nph = 1;
        square_taps(k.ph[0], w, (int64_t)9 * Cin, 3, -1);
        return launch_conv_gemm(k, stream);
    }
    k.y = part; k.ldy = Cout; k.yim = (int64_t)4 * Ho * Wo; k.Wout = 2 * Wo; k.os = 2; k.nph = 3;
    for (int r = 0; r < 3; r++) {                                // kernel row r: taps 3 r .. 3 r + 2, to parity (r >> 1, r & 1)
        ConvTaps &t = k.ph[r];
        t.w = reinterpret_cast<const float *>(reinterpret_cast<const char *>(w) + (size_t)3 * r * Cin * wsz);
        t.ldw = (int64_t)9 * Cin; t.ntaps = 3; t.py = r >> 1; t.px = r & 1;
        for (int j = 0; j < 3; j++) { t.dy[j] = (signed char)(r - 1); t.dx[j] = (signed char)(j - 1); }
    }
    if (launch_conv_gemm(k, stream)) return 1;
    return conv_sum3(part, bias, res, y, N, Ho, Wo, Cout, stream);
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float silu(float z) { return z / (1.f + expf(-z)); }

// torch [Cout][Cin][kk] -> [Cout][kk][Cinp], channels Cin .. Cinp - 1 zeros
__global__ void __launch_bounds__(256) unet_pack_pad_kernel(const float *__restrict__ w, float *__restrict__ out, int Cout, int Cin, int Cinp, int kk)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Cout * kk * Cinp) return;
    const int ci = e % Cinp, t = (e / Cinp) % kk, co = e / (Cinp * kk);
    out[e] = ci < Cin ? w[((size_t)co * Cin + ci) * kk + t] : 0.f;
}
// x [N][C][H][W] with any strides -> [N][H W][8], channels C .. 7 zeros
__global__ void __launch_bounds__(256) unet_stage_kernel(const float *__restrict__ x, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                                                         float *__restrict__ y, int64_t total, int C, int H, int W)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % CIN0);
    const int64_t p = e / CIN0;
    const int xx = (int)(p % W), yy = (int)((p / W) % H);
    const int64_t n = p / ((int64_t)W * H);
    y[e] = c < C ? x[n * sn + c * sc + yy * sh + xx * sw] : 0.f;
}
// [N][2 half]: cos(t f_i) | sin(t f_i), f_i = exp(-ln(10000) i / half)
__global__ void __launch_bounds__(256) unet_time_kernel(const float *__restrict__ t, float *__restrict__ y, int N, int half)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N * 2 * half) return;
    const int d = e % (2 * half), n = e / (2 * half);
    const int i = d < half ? d : d - half;
    const float arg = t[n] * expf(-9.210340371976184f * (float)i / (float)half);
    y[e] = d < half ? cosf(arg) : sinf(arg);
}
__global__ void __launch_bounds__(256) unet_silu_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t total)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) y[e] = silu(x[e]);
}

// grid (32 groups, N).  A thread sums its elements of the group in double, the block adds the 256 partial sums as a fixed tree.
// add (or NULL) [N][C]: x + add[n][c] is what is normalised
__global__ void __launch_bounds__(256) unet_gn_stats_kernel(const float *__restrict__ x, const float *__restrict__ add, float *__restrict__ stats,
                                                            int64_t hw, int C, float eps)
{
    __shared__ double sh[2][256];
    const int g = blockIdx.x, n = blockIdx.y, t = threadIdx.x;
    const int cpg = C / GN_GROUPS;
    const int64_t cnt = hw * cpg;
    const float *xb = x + (size_t)n * hw * C + g * cpg;
    const float *ab = add ? add + (size_t)n * C + g * cpg : nullptr;
    double s0 = 0.0, s1 = 0.0;
    for (int64_t e = t; e < cnt; e += 256) {
        const int64_t p = e / cpg;
        const int c = (int)(e - p * cpg);
        float v = xb[p * C + c];
        if (ab) v += ab[c];
        s0 += (double)v;
        s1 += (double)v * (double)v;
    }
    sh[0][t] = s0;
    sh[1][t] = s1;
    __syncthreads();
    for (int d = 128; d; d >>= 1) {
        if (t < d) { sh[0][t] += sh[0][t + d]; sh[1][t] += sh[1][t + d]; }
        __syncthreads();
    }
    if (t == 0) {
        const double m = sh[0][0] / (double)cnt;
        const double var = fmax(sh[1][0] / (double)cnt - m * m, 0.0);
        stats[((size_t)n * GN_GROUPS + g) * 2] = (float)m;
        stats[((size_t)n * GN_GROUPS + g) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
    }
}
__global__ void __launch_bounds__(256) unet_gn_apply_kernel(const float *__restrict__ x, const float *__restrict__ add, const float *__restrict__ stats,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta, float *__restrict__ y,
                                                            int64_t total, int64_t hw, int C, int act)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const int64_t n = e / C / hw;
    const int g = c / (C / GN_GROUPS);
    const float mean = stats[((size_t)n * GN_GROUPS + g) * 2], rstd = stats[((size_t)n * GN_GROUPS + g) * 2 + 1];
    float v = x[e];
    if (add) v += add[n * C + c];
    const float z = (v - mean) * rstd * gamma[c] + beta[c];
    y[e] = act ? silu(z) : z;
}
// h [M][2 I] = a | g -> y [M][I] = a gelu(g)
__global__ void __launch_bounds__(256) unet_geglu_kernel(const float *__restrict__ h, float *__restrict__ y, int64_t total, int I)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t m = e / I;
    const int i = (int)(e - m * I);
    y[e] = h[m * 2 * I + i] * gelu_erf(h[m * 2 * I + I + i]);
}
// y [rows][Ca + Cb] = a [rows][Ca] | b [rows][Cb], four channels a thread
__global__ void __launch_bounds__(256) unet_cat_kernel(const float *__restrict__ a, int Ca, const float *__restrict__ b, int Cb, float *__restrict__ y, int64_t total4)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total4) return;
    const int q = (Ca + Cb) / 4;
    const int64_t r = e / q;
    const int c = (int)(e - r * q) * 4;
    const float4 v = c < Ca ? *reinterpret_cast<const float4 *>(a + r * Ca + c) : *reinterpret_cast<const float4 *>(b + r * Cb + (c - Ca));
    reinterpret_cast<float4 *>(y)[e] = v;
}
// nearest 2 x: x [N][H][W][C] -> y [N][2 H][2 W][C], four channels a thread
__global__ void __launch_bounds__(256) unet_up_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t total4, int H, int W, int C)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total4) return;
    const int q = C / 4;
    const int c = (int)(e % q);
    const int64_t p = e / q;
    const int ox = (int)(p % (2 * W)), oy = (int)((p / (2 * W)) % (2 * H));
    const int64_t n = p / ((int64_t)4 * W * H);
    reinterpret_cast<float4 *>(y)[e] = reinterpret_cast<const float4 *>(x)[((n * H + (oy >> 1)) * W + (ox >> 1)) * q + c];
}

// y [N][Ho][Wo][C] = ((p00 + p01) + p10) + bias (+ res) of part [N][2 Ho][2 Wo][C]'s parities, four channels a thread
__global__ void __launch_bounds__(256) unet_sum3_kernel(const float *__restrict__ part, const float *__restrict__ bias, const float *res, float *y,
                                                        int64_t total4, int Ho, int Wo, int C)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total4) return;
    const int q = C / 4;
    const int c = (int)(e % q);
    const int64_t p = e / q;
    const int x = (int)(p % Wo), yy = (int)((p / Wo) % Ho);
    const int64_t n = p / ((int64_t)Wo * Ho);
    const float4 *src = reinterpret_cast<const float4 *>(part) + ((n * 2 * Ho + 2 * yy) * 2 * Wo + 2 * x) * q + c;
    const float4 a = src[0], b = src[q], d = src[(int64_t)2 * Wo * q], bv = reinterpret_cast<const float4 *>(bias)[c];
    float4 v = make_float4(((a.x + b.x) + d.x) + bv.x, ((a.y + b.y) + d.y) + bv.y, ((a.z + b.z) + d.z) + bv.z, ((a.w + b.w) + d.w) + bv.w);
    if (res) {
        const float4 r = reinterpret_cast<const float4 *>(res)[e];
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    reinterpret_cast<float4 *>(y)[e] = v;
}
int conv_sum3(const float *part, const float *bias, const float *res, float *y, int N, int Ho, int Wo, int Cout, hipStream_t stream)
{
    const int64_t total4 = (int64_t)N * Ho * Wo * Cout / 4;
    hipLaunchKernelGGL(unet_sum3_kernel, dim3(blocks(total4)), dim3(256), 0, stream, part, bias, res, y, total4, Ho, Wo, Cout);
    SOAR_LAUNCH_OK("unet_sum3", stream, 0);
    return 0;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------
struct Ws {
    float *x0, *temb, *e1, *emb, *semb, *eo, *stats;
    float *act[2], *tmp, *h1, *cat, *up, *part;
    float *tx, *tn, *qkv, *ao, *kv, *kvip, *ff, *gg;
    std::vector<float *> skips;
};
size_t carve(const SoarUnetConfig &c, const Plan &P, int N, int H, int W, int T, int n_ip, void *base, Ws *out)
{
    Carver cv(base);
    Ws w;
    const size_t E = (size_t)4 * c.model_channels, hw = (size_t)H * W;
    size_t act = 0, tok = 0, cmax = 0, ctr = 0;
    auto rows = [&](int level) { return (size_t)N * (hw >> (2 * level)); };
    auto see = [&](const Blk &b) {
        const size_t r = rows(b.level), wide = (size_t)(b.cin > b.cout ? b.cin : b.cout);
        act = act > r * wide ? act : r * wide;
        if (b.up) act = act > 4 * r * b.cout ? act : 4 * r * b.cout;
        cmax = cmax > wide ? cmax : wide;
        if (b.tr >= 0) { tok = tok > r * b.cout ? tok : r * b.cout; ctr = ctr > (size_t)b.cout ? ctr : (size_t)b.cout; }
    };
    for (const Blk &b : P.in) see(b);
    see(P.mid);
    for (const Blk &b : P.out) see(b);
    w.x0 = cv.take<float>((size_t)N * hw * CIN0);
    w.temb = cv.take<float>((size_t)N * c.model_channels); w.e1 = cv.take<float>(N * E); w.emb = cv.take<float>(N * E); w.semb = cv.take<float>(N * E);
    w.eo = cv.take<float>(N * cmax); w.stats = cv.take<float>((size_t)N * GN_GROUPS * 2);
    for (const Blk &b : P.in) w.skips.push_back(cv.take<float>(rows(b.level) / (b.down ? 4 : 1) * b.cout));
    w.act[0] = cv.take<float>(act); w.act[1] = cv.take<float>(act); w.tmp = cv.take<float>(act); w.h1 = cv.take<float>(act);
    w.cat = cv.take<float>(act); w.up = cv.take<float>(act);
    w.part = cv.take<float>((size_t)N * SPLIT_PIXELS * 4 * cmax);        // a split convolution's three results: four parities of at most 64 pixels
    w.tx = cv.take<float>(tok); w.tn = cv.take<float>(tok); w.qkv = cv.take<float>(3 * tok); w.ao = cv.take<float>(tok);
    w.kv = cv.take<float>((size_t)N * T * 2 * ctr); w.kvip = cv.take<float>((size_t)N * n_ip * 2 * ctr);
    w.ff = cv.take<float>(8 * tok); w.gg = cv.take<float>(4 * tok);
    if (out) *out = w;
    return cv.bytes();
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_unet_weights_bytes(const SoarUnetConfig *cfg, size_t *bytes, int32_t *count, size_t *floats)
{
    if (!check_cfg(cfg, "soar_unet_weights_bytes")) return 1;
    if (!bytes) { set_error("soar_unet_weights_bytes: NULL bytes"); return 1; }
    const Plan P = make_plan(*cfg);
    *bytes = align_up(P.total * sizeof(float));
    if (count) *count = P.count();
    if (floats) *floats = P.floats;
    return 0;
}

int soar_unet_pack_weights(const SoarUnetConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                           size_t packed_bytes, void *stream_)
{
    const char *me = "soar_unet_pack_weights";
    if (!check_cfg(cfg, me)) return 1;
    const Plan P = make_plan(*cfg);
    if (!sizes) { set_error("%s: NULL sizes", me); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    std::vector<int> conv_of(P.count(), -1);
    for (size_t j = 0; j < P.convs.size(); j++) conv_of[P.convs[j].idx] = (int)j;
    return pack_weights(P, tensors, sizes, count, packed, packed_bytes, stream, me, [&](int i, const float *src, float *dst) -> int {
        const Repack *r = conv_of[i] >= 0 ? &P.convs[conv_of[i]] : nullptr;
        if (P.half && P.mat[i])                                  // a product's B operand: 16-bit, a linear layer's matrix as one long row
            return r ? launch_conv_pack16(src, dst, r->Cout, r->Cin, r->Cinp, 9, cfg->precision, stream)
                     : launch_conv_pack16(src, dst, 1, (int)P.n[i], (int)P.n[i], 1, cfg->precision, stream);
        if (!r) return PACK_COPY;
        hipLaunchKernelGGL(unet_pack_pad_kernel, dim3(blocks((int64_t)r->Cout * 9 * r->Cinp)), dim3(256), 0, stream, src, dst, r->Cout, r->Cin, r->Cinp, 9);
        SOAR_LAUNCH_OK("unet_pack_pad", stream, 0);
        return 0;
    });
}

int soar_unet_workspace_bytes(const SoarUnetConfig *cfg, int32_t N, int32_t H, int32_t W, int32_t T, int32_t ip_tokens, size_t *bytes)
{
    const char *me = "soar_unet_workspace_bytes";
    if (!check_cfg(cfg, me)) return 1;
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (!check_sizes(*cfg, N, H, W, T, ip_tokens, me)) return 1;
    *bytes = carve(*cfg, make_plan(*cfg), N, H, W, T, ip_tokens, nullptr, nullptr);
    return 0;
}

int soar_unet_forward(const SoarUnetConfig *cfg, const void *packed, const SoarUnetArgs *args, void *workspace, size_t workspace_bytes,
                      void *stream_)
{
    const char *me = "soar_unet_forward";
    if (!check_cfg(cfg, me)) return 1;
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarUnetConfig &c = *cfg;
    const SoarUnetArgs &a = *args;
    if (!check_sizes(c, a.N, a.H, a.W, a.T, a.n_ip, me)) return 1;
    if (a.n_probes < 0 || a.n_probes > SOAR_UNET_MAX_PROBES) { set_error("%s: %d probes: at most %d", me, a.n_probes, SOAR_UNET_MAX_PROBES); return 1; }
    if (a.N == 0) return 0;
    if (!packed || !a.x || !a.t || !a.context || !a.eps || (!a.ip_tokens != !a.n_ip)) {
        set_error("%s: NULL packed weights, x, t, context or eps, or image tokens without their count", me);
        return 1;
    }
    if (a.camera && !c.camera_dim) { set_error("%s: a camera, but the weights have no camera_embed", me); return 1; }
    if (!a.camera && c.camera_dim) { set_error("%s: the weights have camera_embed, but no camera is given", me); return 1; }
    for (int i = 0; i < a.n_probes; i++)
        if (!a.probe_dst[i]) { set_error("%s: probe %d has no destination", me, i); return 1; }
    const Plan P = make_plan(c);
    if (!workspace_ok(me, workspace, workspace_bytes, carve(c, P, a.N, a.H, a.W, a.T, a.n_ip, nullptr, nullptr), "soar_unet_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const float *base = static_cast<const float *>(packed);
    auto Wt = [&](int i) { return base + P.off[i]; };
    Ws w;
    carve(c, P, a.N, a.H, a.W, a.T, a.n_ip, workspace, &w);
    const int N = a.N, mc = c.model_channels, E = 4 * mc, ctx = c.context_dim, wt = c.precision;

    auto probe = [&](int code, const float *src, size_t floats) -> int {
        for (int i = 0; i < a.n_probes; i++)
            if (a.probe_code[i] == code) SOAR_HIP_OK(hipMemcpyAsync(a.probe_dst[i], src, floats * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return 0;
    };
    auto silu_of = [&](const float *x, float *y, int64_t total) -> int {
        hipLaunchKernelGGL(unet_silu_kernel, dim3(blocks(total)), dim3(256), 0, stream, x, y, total);
        SOAR_LAUNCH_OK("unet_silu", stream, 0);
        return 0;
    };
    auto group_norm = [&](const float *x, const float *add, int64_t hw, int C, const float *gamma, const float *beta, float eps, int act, float *y) -> int {
        hipLaunchKernelGGL(unet_gn_stats_kernel, dim3(GN_GROUPS, (unsigned)N), dim3(256), 0, stream, x, add, w.stats, hw, C, eps);
        SOAR_LAUNCH_OK("unet_gn_stats", stream, 0);
        const int64_t total = (int64_t)N * hw * C;
        hipLaunchKernelGGL(unet_gn_apply_kernel, dim3(blocks(total)), dim3(256), 0, stream, x, add, w.stats, gamma, beta, y, total, hw, C, act);
        SOAR_LAUNCH_OK("unet_gn_apply", stream, 0);
        return 0;
    };

    // ---- the embedding
    hipLaunchKernelGGL(unet_time_kernel, dim3(blocks((int64_t)N * mc)), dim3(256), 0, stream, a.t, w.temb, N, mc / 2);
    SOAR_LAUNCH_OK("unet_time", stream, 0);
    if (gemm(w.temb, mc, Wt(P.time0), mc, E, Wt(P.time0 + 1), nullptr, w.e1, E, N, stream, ACT_NONE, wt)) return 1;
    if (silu_of(w.e1, w.e1, (int64_t)N * E)) return 1;
    if (gemm(w.e1, E, Wt(P.time0 + 2), E, E, Wt(P.time0 + 3), nullptr, w.emb, E, N, stream, ACT_NONE, wt)) return 1;
    if (a.camera) {
        if (gemm(a.camera, c.camera_dim, Wt(P.cam0), c.camera_dim, E, Wt(P.cam0 + 1), nullptr, w.e1, E, N, stream, ACT_NONE, wt)) return 1;
        if (silu_of(w.e1, w.e1, (int64_t)N * E)) return 1;
        if (gemm(w.e1, E, Wt(P.cam0 + 2), E, E, Wt(P.cam0 + 3), w.emb, w.emb, E, N, stream, ACT_NONE, wt)) return 1;
    }
    if (probe(SOAR_UNET_PROBE_EMB, w.emb, (size_t)N * E)) return 1;
    if (silu_of(w.emb, w.semb, (int64_t)N * E)) return 1;

    // ---- the blocks' parts.  H, W: the level's size
    auto res_block = [&](int t0, const float *x, int cin, int cout, int H, int W, float *y) -> int {
        const int64_t hw = (int64_t)H * W;
        if (group_norm(x, nullptr, hw, cin, Wt(t0), Wt(t0 + 1), 1e-5f, 1, w.tmp)) return 1;
        if (conv3x3(w.tmp, cin, Wt(t0 + 2), Wt(t0 + 3), nullptr, w.h1, cout, N, H, W, 1, w.part, wt, stream)) return 1;
        if (gemm(w.semb, E, Wt(t0 + 4), E, cout, Wt(t0 + 5), nullptr, w.eo, cout, N, stream, ACT_NONE, wt)) return 1;
        if (group_norm(w.h1, w.eo, hw, cout, Wt(t0 + 6), Wt(t0 + 7), 1e-5f, 1, w.tmp)) return 1;
        const float *skip = x;
        if (cin != cout) {
            if (gemm(x, cin, Wt(t0 + 10), cin, cout, Wt(t0 + 11), nullptr, y, cout, (int64_t)N * hw, stream, ACT_NONE, wt)) return 1;
            skip = y;
        }
        return conv3x3(w.tmp, cout, Wt(t0 + 8), Wt(t0 + 9), skip, y, cout, N, H, W, 1, w.part, wt, stream);
    };
    // in place on x [N][H W][C]
    auto transformer = [&](int t0, float *x, int C, int H, int W, int code) -> int {
        const int64_t hw = (int64_t)H * W, M = (int64_t)N * hw;
        const int heads = C / c.head_channels, hd = c.head_channels, o = t0 + P.tr_tail;
        const float scale = 1.f / sqrtf((float)hd);
        if (group_norm(x, nullptr, hw, C, Wt(t0), Wt(t0 + 1), 1e-6f, 0, w.tmp)) return 1;
        if (gemm(w.tmp, C, Wt(t0 + 2), C, C, Wt(t0 + 3), nullptr, w.tx, C, M, stream, ACT_NONE, wt)) return 1;
        // attn1 over the tokens of all the views of a group: q | k | v from the three weights, which lie one behind the other
        if (layer_norm(w.tx, Wt(t0 + 4), Wt(t0 + 5), w.tn, M, C, 1e-5f, ACT_NONE, stream)) return 1;
        if (gemm(w.tn, C, Wt(t0 + 6), C, 3 * C, nullptr, nullptr, w.qkv, 3 * C, M, stream, ACT_NONE, wt)) return 1;
        SoarUnetAttnArgs s{};
        s.q = w.qkv; s.k = w.qkv + C; s.v = w.qkv + 2 * C; s.out = w.ao;
        s.ldq = s.ldk = s.ldv = 3 * C; s.ldo = C;
        s.B = N / c.n_view; s.Lq = s.Lk = (int)(c.n_view * hw); s.heads = heads; s.hd = hd; s.scale = scale;
        if (launch_attention(s, c.attn_precision, 64, false, "unet attention", stream)) return 1;
        if (gemm(w.ao, C, Wt(t0 + 9), C, C, Wt(t0 + 10), w.tx, w.tx, C, M, stream, ACT_NONE, wt)) return 1;
        if (probe(code + 1, w.tx, (size_t)M * C)) return 1;
        // attn2 per view: the text tokens, and the image tokens as a second key set
        if (layer_norm(w.tx, Wt(t0 + 11), Wt(t0 + 12), w.tn, M, C, 1e-5f, ACT_NONE, stream)) return 1;
        if (gemm(w.tn, C, Wt(t0 + 13), C, C, nullptr, nullptr, w.qkv, C, M, stream, ACT_NONE, wt)) return 1;
        if (gemm(a.context, ctx, Wt(t0 + 14), ctx, 2 * C, nullptr, nullptr, w.kv, 2 * C, (int64_t)N * a.T, stream, ACT_NONE, wt)) return 1;
        SoarUnetAttnArgs x2{};
        x2.q = w.qkv; x2.k = w.kv; x2.v = w.kv + C; x2.out = w.ao;
        x2.ldq = C; x2.ldk = x2.ldv = 2 * C; x2.ldo = C;
        x2.B = N; x2.Lq = (int)hw; x2.Lk = a.T; x2.heads = heads; x2.hd = hd; x2.scale = scale;
        if (a.ip_tokens) {
            if (gemm(a.ip_tokens, ctx, Wt(t0 + 16), ctx, 2 * C, nullptr, nullptr, w.kvip, 2 * C, (int64_t)N * a.n_ip, stream, ACT_NONE, wt)) return 1;
            x2.k2 = w.kvip; x2.v2 = w.kvip + C; x2.ldk2 = x2.ldv2 = 2 * C; x2.Lk2 = a.n_ip; x2.w2 = a.ip_weight;
        }
        if (launch_attention(x2, c.attn_precision, 64, false, "unet attention", stream)) return 1;
        if (gemm(w.ao, C, Wt(o), C, C, Wt(o + 1), w.tx, w.tx, C, M, stream, ACT_NONE, wt)) return 1;
        if (probe(code + 2, w.tx, (size_t)M * C)) return 1;
        // GEGLU feed-forward
        if (layer_norm(w.tx, Wt(o + 2), Wt(o + 3), w.tn, M, C, 1e-5f, ACT_NONE, stream)) return 1;
        if (gemm(w.tn, C, Wt(o + 4), C, 8 * C, Wt(o + 5), nullptr, w.ff, 8 * C, M, stream, ACT_NONE, wt)) return 1;
        hipLaunchKernelGGL(unet_geglu_kernel, dim3(blocks(M * 4 * C)), dim3(256), 0, stream, w.ff, w.gg, M * 4 * C, 4 * C);
        SOAR_LAUNCH_OK("unet_geglu", stream, 0);
        if (gemm(w.gg, 4 * C, Wt(o + 6), 4 * C, C, Wt(o + 7), w.tx, w.tx, C, M, stream, ACT_NONE, wt)) return 1;
        if (probe(code + 3, w.tx, (size_t)M * C)) return 1;
        if (gemm(w.tx, C, Wt(o + 8), C, C, Wt(o + 9), x, x, C, M, stream, ACT_NONE, wt)) return 1;
        return probe(code + 4, x, (size_t)M * C);
    };

    // ---- down
    {
        const int64_t total = (int64_t)N * a.H * a.W * CIN0;
        hipLaunchKernelGGL(unet_stage_kernel, dim3(blocks(total)), dim3(256), 0, stream, a.x, a.x_stride[0], a.x_stride[1], a.x_stride[2],
                           a.x_stride[3], w.x0, total, c.in_channels, a.H, a.W);
        SOAR_LAUNCH_OK("unet_stage", stream, 0);
    }
    float *cur = nullptr;
    int code = 0;
    for (size_t bi = 0; bi < P.in.size(); bi++, code += 8) {
        const Blk &b = P.in[bi];
        const int H = a.H >> b.level, W = a.W >> b.level;
        float *y = w.skips[bi];
        size_t floats = (size_t)N * H * W * b.cout;
        if (bi == 0) {
            if (conv3x3(w.x0, CIN0, Wt(b.conv), Wt(b.conv + 1), nullptr, y, b.cout, N, H, W, 1, w.part, wt, stream)) return 1;
        } else if (b.down) {
            if (conv3x3(cur, b.cin, Wt(b.conv), Wt(b.conv + 1), nullptr, y, b.cout, N, H, W, 2, w.part, wt, stream)) return 1;
            floats /= 4;
        } else {
            if (res_block(b.res, cur, b.cin, b.cout, H, W, y)) return 1;
        }
        if (probe(code, y, floats)) return 1;
        if (b.tr >= 0 && transformer(b.tr, y, b.cout, H, W, code)) return 1;
        cur = y;
    }
    // ---- middle
    {
        const Blk &b = P.mid;
        const int H = a.H >> b.level, W = a.W >> b.level;
        const size_t floats = (size_t)N * H * W * b.cout;
        if (res_block(b.res, cur, b.cin, b.cout, H, W, w.act[0])) return 1;
        if (probe(code, w.act[0], floats)) return 1;
        if (transformer(b.tr, w.act[0], b.cout, H, W, code)) return 1;
        if (res_block(b.res2, w.act[0], b.cout, b.cout, H, W, w.act[1])) return 1;
        if (probe(code + 7, w.act[1], floats)) return 1;
        cur = w.act[1];
        code += 8;
    }
    // ---- up
    int flip = 0;                                               // cur is act[1 - flip] from here on
    for (size_t bi = 0; bi < P.out.size(); bi++, code += 8) {
        const Blk &b = P.out[bi];
        const int H = a.H >> b.level, W = a.W >> b.level;
        const int64_t rows = (int64_t)N * H * W;
        const int ch = b.cin - b.skip_ch;
        const float *skip = w.skips[P.in.size() - 1 - bi];
        hipLaunchKernelGGL(unet_cat_kernel, dim3(blocks(rows * b.cin / 4)), dim3(256), 0, stream, cur, ch, skip, b.skip_ch, w.cat, rows * b.cin / 4);
        SOAR_LAUNCH_OK("unet_cat", stream, 0);
        if (probe(code + 6, w.cat, (size_t)rows * b.cin)) return 1;
        float *y = w.act[flip];
        if (res_block(b.res, w.cat, b.cin, b.cout, H, W, y)) return 1;
        if (probe(code, y, (size_t)rows * b.cout)) return 1;
        if (b.tr >= 0 && transformer(b.tr, y, b.cout, H, W, code)) return 1;
        cur = y;
        flip ^= 1;
        if (b.up) {
            const int64_t total4 = rows * 4 * b.cout / 4;
            hipLaunchKernelGGL(unet_up_kernel, dim3(blocks(total4)), dim3(256), 0, stream, cur, w.up, total4, H, W, b.cout);
            SOAR_LAUNCH_OK("unet_up", stream, 0);
            y = w.act[flip];
            if (conv3x3(w.up, b.cout, Wt(b.conv), Wt(b.conv + 1), nullptr, y, b.cout, N, 2 * H, 2 * W, 1, w.part, wt, stream)) return 1;
            if (probe(code + 5, y, (size_t)rows * 4 * b.cout)) return 1;
            cur = y;
            flip ^= 1;
        }
    }
    // ---- out
    if (group_norm(cur, nullptr, (int64_t)a.H * a.W, mc * c.channel_mult[0], Wt(P.out0), Wt(P.out0 + 1), 1e-5f, 1, w.tmp)) return 1;
    return conv3x3(w.tmp, mc * c.channel_mult[0], Wt(P.out0 + 2), Wt(P.out0 + 3), nullptr, a.eps, c.out_channels, N, a.H, a.W, 1, w.part, wt, stream);
}

int soar_unet_attention(const SoarUnetAttnArgs *args, void *stream_)
{
    if (!args) { set_error("soar_unet_attention: NULL args"); return 1; }
    return launch_kv_attention(*args, 64, false, "unet attention", static_cast<hipStream_t>(stream_));
}

}  // extern "C"
