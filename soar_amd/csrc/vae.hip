// vae.hip -- the Stable-Diffusion-2.1 VAE encoder (ldm AutoencoderKL, encoder + quant_conv) and the SDS guidance's loss tail
// (soar_amd/sds.py), as include/soar_hip.h and DESIGN.md 9f state them.
//
//   (conv_pack_kernel      conv_gemm.hip: torch [Cout][Cin][kk] -> [Cout][tap][Cin] (forward) and, spatially flipped and transposed,
//                          [Cin][tap][Cout] (data gradient))
//   (conv_gemm_kernel      conv_gemm.hip: every convolution with Cin >= 128 and the attention's products, as the shared implicit GEMM
//                          with M = output pixels of one image, in 64 x 64 tiles.  Taps: 1 x 1, 3 x 3 pad 1, 3 x 3 stride 2 (ldm's
//                          Downsample: pad right / bottom by one), and the data gradient of the latter as a 3 x 3 convolution over
//                          the zero-dilated output gradient (never materialised: odd dilated coordinates load zeros).  B may be per
//                          image (attention).  Epilogue: y = alpha acc + bias + res)
//   vae_first_kernel       conv_in with the bilinear resize (align_corners=False, torch's source-index arithmetic) and x * 2 - 1 on
//                          load, reading the caller's strides
//   vae_gn_partial_kernel  GroupNorm (32 groups) sums per image and chunk of 256 pixels in double; forward: sum x, sum x^2; backward:
//                          sum dxhat, sum dxhat xhat
//   vae_gn_final_kernel    the chunks of one (image, group) in a fixed order -> mean, rstd (forward) / the two means (backward)
//   vae_gn_apply_kernel    y = silu?((x - mean) rstd gamma + beta)
//   vae_gn_bwd_kernel      dx = rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)) (+ a residual gradient)
//   vae_softmax_kernel     one wave per query row; the padded keys / queries get 0
//   vae_softmax_bwd_kernel dS = alpha P (dP - rowsum(dP P))
//   vae_transpose_kernel   [B][R][ld] column slice -> [B][C][R] (the attention's per-image B operands)
//   vae_conv_out_kernel    norm_out's 512 channels -> 8, one wave per latent pixel; vae_conv_out_bwd_kernel its data gradient
//   vae_head_kernel        quant_conv, chunk, logvar clamp, std, latents = s (mean + std eps); keeps d latents / d logvar
//   vae_head_bwd_kernel    the gradient of latents (times g_scale) through the sampling and quant_conv
//   vae_first_bwd_kernel   conv_in's data gradient (x 2) at the resized pixels
//   vae_resize_bwd_kernel  the resize's data gradient as a gather over the resized pixels that read an input pixel (no atomics),
//                          times grad_scale, written through the caller's strides
//   sds_q_sample_kernel    x_t = sqrt(ac[t]) latents + sqrt(1 - ac[t]) noise into both halves of the UNet input
//   sds_loss_kernel        one workgroup: CFG, x0 reconstruction, the per-group std rescale, loss, grad_norm and d loss / d latents
//                          (recon mode), or w(t) (eps - noise) clipped and nan_to_num'ed (SDS mode); sums in double, fixed order
//
// Precision (soar_vae_*16): 0 is all of the above in float32.  1 (bf16) / 2 (f16) run exactly the products whose B
// operand is a weight tensor on conv_gemm16_kernel: the packed forward and data-gradient forms are 16-bit values, A is rounded as it
// is loaded, the sums and every activation in memory stay float32.  conv_in, conv_out, quant_conv, the attention's products of two
// activations, softmax, GroupNorm, the resize and the loss tail stay float32.  The backward then keeps *g_scale away from the 16-bit
// products: it multiplies at conv_in's data gradient, and f16 runs on g_latents 2^10 and divides there as well.
//
// No atomics: every value and gradient has one fixed order of summation, independent of N (bitwise reproducible, N = 4 equals four
// N = 1 calls).  No host synchronisation, no allocation.  Offsets are size_t.
#include "conv_gemm.h"
#include "workspace.h"

namespace soar {

namespace {

constexpr int CH = 128;
constexpr int ZC = 4;                  // z_channels
constexpr int GROUPS = 32;
constexpr float GN_EPS = 1e-6f;
constexpr int NLEV = 4;
const int LEVC[NLEV] = {128, 256, 512, 512};
constexpr int CMID = 512;
constexpr int CHUNK = 256;             // GroupNorm pixels per partial sum
constexpr int64_t MAX_PIX = int64_t(1) << 28;

// ---- the raw weights: one flat float array, ldm's tensors in a fixed order (include/soar_hip.h) ----
struct RB {
    int cin, cout;
    size_t n1g, n1b, c1w, c1b, n2g, n2b, c2w, c2b, ninw, ninb;      // raw offsets
    size_t c1f, c1r, c2f, c2r, ninf, ninr;                            // packed: forward / data-gradient forms
};
struct Layout {
    size_t cin_w, cin_b;
    RB rb[NLEV][2];
    size_t dw[3], db[3], df[3], dr[3];                                // downsample convs
    RB mid1, mid2;
    size_t an_g, an_b, q_w, q_b, k_w, k_b, v_w, v_b, p_w, p_b;      // attention (raw)
    size_t qkv_f, qkv_b, qkv_r, p_f, p_r;                             // packed: [3C][C], bias [3C], [C][3C], [C][C] x 2
    size_t no_g, no_b, co_w, co_b, qc_w, qc_b;
    size_t raw_total;                                                 // floats
    size_t total;                                                     // floats of the packed form (raw copy first)
};
// prec != 0: the forward / data-gradient forms are 16-bit values, two to a float; their offsets still count floats, every region
// 256-byte aligned.  The raw copy, the biases and the norm affines are float32 at every precision.
Layout layout(int prec = 0)
{
    Layout L{};
    size_t off = 0;
    auto raw = [&](size_t n) { const size_t o = off; off += n; return o; };
    auto rb_raw = [&](RB &b, int cin, int cout) {
        b.cin = cin; b.cout = cout;
        b.n1g = raw(cin); b.n1b = raw(cin);
        b.c1w = raw((size_t)cout * cin * 9); b.c1b = raw(cout);
        b.n2g = raw(cout); b.n2b = raw(cout);
        b.c2w = raw((size_t)cout * cout * 9); b.c2b = raw(cout);
        if (cin != cout) { b.ninw = raw((size_t)cout * cin); b.ninb = raw(cout); }
    };
    L.cin_w = raw((size_t)CH * 3 * 9); L.cin_b = raw(CH);
    int c = CH;
    for (int l = 0; l < NLEV; l++) {
        for (int j = 0; j < 2; j++) { rb_raw(L.rb[l][j], c, LEVC[l]); c = LEVC[l]; }
        if (l < 3) { L.dw[l] = raw((size_t)c * c * 9); L.db[l] = raw(c); }
    }
    rb_raw(L.mid1, CMID, CMID);
    L.an_g = raw(CMID); L.an_b = raw(CMID);
    L.q_w = raw((size_t)CMID * CMID); L.q_b = raw(CMID);
    L.k_w = raw((size_t)CMID * CMID); L.k_b = raw(CMID);
    L.v_w = raw((size_t)CMID * CMID); L.v_b = raw(CMID);
    L.p_w = raw((size_t)CMID * CMID); L.p_b = raw(CMID);
    rb_raw(L.mid2, CMID, CMID);
    L.no_g = raw(CMID); L.no_b = raw(CMID);
    L.co_w = raw((size_t)2 * ZC * CMID * 9); L.co_b = raw(2 * ZC);
    L.qc_w = raw((size_t)2 * ZC * 2 * ZC); L.qc_b = raw(2 * ZC);
    L.raw_total = off;
    // packed regions, every one 256-byte aligned
    Carver pk;
    pk.float_offset(L.raw_total);       // behind the raw copy
    auto wmat = [&](size_t n) { return pk.float_offset(prec ? (n + 1) / 2 : n); };      // a B operand of n elements
    auto rb_pack = [&](RB &b) {
        b.c1f = wmat((size_t)b.cout * b.cin * 9); b.c1r = wmat((size_t)b.cout * b.cin * 9);
        b.c2f = wmat((size_t)b.cout * b.cout * 9); b.c2r = wmat((size_t)b.cout * b.cout * 9);
        if (b.cin != b.cout) { b.ninf = wmat((size_t)b.cout * b.cin); b.ninr = wmat((size_t)b.cout * b.cin); }
    };
    for (int l = 0; l < NLEV; l++) {
        for (int j = 0; j < 2; j++) rb_pack(L.rb[l][j]);
        if (l < 3) { L.df[l] = wmat((size_t)LEVC[l] * LEVC[l] * 9); L.dr[l] = wmat((size_t)LEVC[l] * LEVC[l] * 9); }
    }
    rb_pack(L.mid1);
    rb_pack(L.mid2);
    L.qkv_f = wmat((size_t)3 * CMID * CMID); L.qkv_b = pk.float_offset(3 * CMID); L.qkv_r = wmat((size_t)3 * CMID * CMID);
    L.p_f = wmat((size_t)CMID * CMID); L.p_r = wmat((size_t)CMID * CMID);
    L.total = pk.bytes() / sizeof(float);
    return L;
}

// ---- the workspace ----
struct Dims {
    int N, S[NLEV];
    int T, Tp;                         // attention tokens, padded to a multiple of 64
    int64_t pix(int l) const { return (int64_t)N * S[l] * S[l]; }
};
Dims dims_of(int N, int image_size)
{
    Dims d{};
    d.N = N;
    for (int l = 0; l < NLEV; l++) d.S[l] = image_size >> l;
    d.T = d.S[3] * d.S[3];
    d.Tp = (d.T + 63) / 64 * 64;
    return d;
}
struct RBws { size_t x, h1, st1, st2; };      // the block's input (kept), conv1's output, the two GroupNorms' statistics
struct WsLayout {
    size_t t_in;                      // conv_in's output
    RBws rb[NLEV][2];
    size_t rb_out[NLEV][2];           // each block's output
    size_t down[3];                   // the downsamples' outputs
    RBws mid1, mid2;
    size_t mid1_out, an_st, qkv, P, vT, O, attn_out, mid2_out, no_st, m8, dlv;
    size_t tmp, part;                 // silu(gn(.)) of the current layer; the GroupNorm partial sums (double)
    // backward
    size_t g[3], dO, dOT, dP, XT, dqkv, g8, gxr;
    size_t total;
};
WsLayout ws_layout(const Dims &d)
{
    WsLayout L{};
    Carver ws;
    const int64_t st = (int64_t)d.N * GROUPS * 2;
    int c = CH;
    L.t_in = ws.offset<float>(d.pix(0) * CH);
    for (int l = 0; l < NLEV; l++) {
        for (int j = 0; j < 2; j++) {
            L.rb[l][j].h1 = ws.offset<float>(d.pix(l) * LEVC[l]);
            L.rb[l][j].st1 = ws.offset<float>(st);
            L.rb[l][j].st2 = ws.offset<float>(st);
            L.rb_out[l][j] = ws.offset<float>(d.pix(l) * LEVC[l]);
            c = LEVC[l];
        }
        if (l < 3) L.down[l] = ws.offset<float>(d.pix(l + 1) * c);
    }
    for (RBws *b : {&L.mid1, &L.mid2}) {
        b->h1 = ws.offset<float>(d.pix(3) * CMID);
        b->st1 = ws.offset<float>(st);
        b->st2 = ws.offset<float>(st);
    }
    L.mid1_out = ws.offset<float>(d.pix(3) * CMID);
    L.an_st = ws.offset<float>(st);
    const int64_t NT = (int64_t)d.N * d.Tp;
    L.qkv = ws.offset<float>(NT * 3 * CMID);
    L.P = ws.offset<float>(NT * d.Tp);
    L.vT = ws.offset<float>(NT * CMID);
    L.O = ws.offset<float>(NT * CMID);
    L.attn_out = ws.offset<float>(d.pix(3) * CMID);
    L.mid2_out = ws.offset<float>(d.pix(3) * CMID);
    L.no_st = ws.offset<float>(st);
    L.m8 = ws.offset<float>(d.pix(3) * 2 * ZC);
    L.dlv = ws.offset<float>(d.pix(3) * ZC);
    L.tmp = ws.offset<float>(d.pix(0) * CH);
    const int64_t nchunk = (int64_t)(d.S[0] * d.S[0] + CHUNK - 1) / CHUNK;
    L.part = ws.offset<float>((int64_t)d.N * nchunk * GROUPS * 2 * 2 + (int64_t)d.N * GROUPS * 2);   // the doubles, then the backward's two means
    for (int i = 0; i < 3; i++) L.g[i] = ws.offset<float>(d.pix(0) * CH);
    L.dO = ws.offset<float>(NT * CMID);
    L.dOT = ws.offset<float>(NT * CMID);
    L.dP = ws.offset<float>(NT * d.Tp);
    L.XT = ws.offset<float>(NT * d.Tp);
    L.dqkv = ws.offset<float>(NT * 3 * CMID);
    L.g8 = ws.offset<float>(d.pix(3) * 2 * ZC);
    L.gxr = ws.offset<float>(d.pix(0) * 4);
    // the blocks' inputs are the outputs in front of them
    L.rb[0][0].x = L.t_in;
    L.rb[0][1].x = L.rb_out[0][0];
    for (int l = 1; l < NLEV; l++) {
        L.rb[l][0].x = L.down[l - 1];
        L.rb[l][1].x = L.rb_out[l][0];
    }
    L.mid1.x = L.rb_out[3][1];
    L.mid2.x = L.attn_out;
    L.total = ws.bytes() == 0 ? ALIGN : ws.bytes();
    return L;
}

// ---- GroupNorm ----
struct GnK {
    const float *x;        // [N][HW][C]
    const float *dy;       // backward: gradient of the output
    const float *res;      // backward: added to dx, or NULL
    float *y;              // forward: silu?(gn(x)); backward: dx
    const float *gamma, *beta;
    float *stats;          // [N][32][2]: mean, rstd
    float *bstats;         // backward: [N][32][2]: mean(dxhat), mean(dxhat xhat)
    double *part;          // [N][nchunk][32][2]
    int64_t hw;
    int C, nchunk, silu, bwd;
};
__device__ __forceinline__ float sigm(float z) { return 1.f / (1.f + expf(-z)); }

// grid (nchunk, N); thread t: channel quad t % (C / 4), pixel row t / (C / 4)
__global__ void __launch_bounds__(256) vae_gn_partial_kernel(GnK k)
{
    __shared__ double sh[256][2];
    const int t = threadIdx.x, n = blockIdx.y, chunk = blockIdx.x;
    const int c4 = k.C / 4, rows = 256 / c4;
    const int cq = t % c4, pr = t / c4;
    const int cpg = k.C / GROUPS, g = cq * 4 / cpg;
    const int64_t p0 = (int64_t)chunk * CHUNK, p1 = min(p0 + CHUNK, k.hw);
    double s0 = 0.0, s1 = 0.0;
    float mean = 0.f, rstd = 0.f;
    float ga[4], be[4];
    if (k.bwd) {
        mean = k.stats[((size_t)n * GROUPS + g) * 2];
        rstd = k.stats[((size_t)n * GROUPS + g) * 2 + 1];
#pragma unroll
        for (int j = 0; j < 4; j++) { ga[j] = k.gamma[cq * 4 + j]; be[j] = k.beta[cq * 4 + j]; }
    }
    if (pr < rows) {
        for (int64_t p = p0 + pr; p < p1; p += rows) {
            const size_t idx = ((size_t)n * k.hw + p) * k.C + cq * 4;
            const float4 xv = *reinterpret_cast<const float4 *>(k.x + idx);
            const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
            if (!k.bwd) {
#pragma unroll
                for (int j = 0; j < 4; j++) { s0 += (double)xs[j]; s1 += (double)xs[j] * (double)xs[j]; }
            } else {
                const float4 dv = *reinterpret_cast<const float4 *>(k.dy + idx);
                const float ds[4] = {dv.x, dv.y, dv.z, dv.w};
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const float xh = (xs[j] - mean) * rstd;
                    float dz = ds[j];
                    if (k.silu) {
                        const float z = fmaf(xh, ga[j], be[j]);
                        const float sg = sigm(z);
                        dz *= sg * (1.f + z * (1.f - sg));
                    }
                    const float dxh = dz * ga[j];
                    s0 += (double)dxh;
                    s1 += (double)dxh * (double)xh;
                }
            }
        }
    }
    sh[t][0] = s0;
    sh[t][1] = s1;
    __syncthreads();
    if (t < GROUPS) {
        // group t: quads t cpg / 4 .. (t + 1) cpg / 4 - 1 of every pixel row, rows outer, in a fixed order
        const int q0 = t * cpg / 4, q1 = (t + 1) * cpg / 4;
        double a = 0.0, b = 0.0;
        for (int r = 0; r < rows; r++)
            for (int q = q0; q < q1; q++) { a += sh[r * c4 + q][0]; b += sh[r * c4 + q][1]; }
        double *o = k.part + (((size_t)n * k.nchunk + chunk) * GROUPS + t) * 2;
        o[0] = a;
        o[1] = b;
    }
}

// thread = (image, group)
__global__ void __launch_bounds__(256) vae_gn_final_kernel(GnK k, int N)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N * GROUPS) return;
    const int n = e / GROUPS, g = e - n * GROUPS;
    double a = 0.0, b = 0.0;
    for (int c = 0; c < k.nchunk; c++) {
        const double *p = k.part + (((size_t)n * k.nchunk + c) * GROUPS + g) * 2;
        a += p[0];
        b += p[1];
    }
    const double cnt = (double)k.hw * (k.C / GROUPS);
    if (!k.bwd) {
        const double m = a / cnt;
        const double var = fmax(b / cnt - m * m, 0.0);
        k.stats[(size_t)e * 2] = (float)m;
        k.stats[(size_t)e * 2 + 1] = (float)(1.0 / sqrt(var + (double)GN_EPS));
    } else {
        k.bstats[(size_t)e * 2] = (float)(a / cnt);
        k.bstats[(size_t)e * 2 + 1] = (float)(b / cnt);
    }
}

__global__ void __launch_bounds__(256) vae_gn_apply_kernel(GnK k, int64_t n4)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const int c4 = k.C / 4;
    const int cq = (int)(e % c4);
    const int64_t n = e / c4 / k.hw;
    const int g = cq * 4 / (k.C / GROUPS);
    const float mean = k.stats[((size_t)n * GROUPS + g) * 2], rstd = k.stats[((size_t)n * GROUPS + g) * 2 + 1];
    const float4 xv = reinterpret_cast<const float4 *>(k.x)[e];
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float z = fmaf((xs[j] - mean) * rstd, k.gamma[cq * 4 + j], k.beta[cq * 4 + j]);
        o[j] = k.silu ? z * sigm(z) : z;
    }
    reinterpret_cast<float4 *>(k.y)[e] = make_float4(o[0], o[1], o[2], o[3]);
}

__global__ void __launch_bounds__(256) vae_gn_bwd_kernel(GnK k, int64_t n4)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n4) return;
    const int c4 = k.C / 4;
    const int cq = (int)(e % c4);
    const int64_t n = e / c4 / k.hw;
    const int g = cq * 4 / (k.C / GROUPS);
    const size_t si = ((size_t)n * GROUPS + g) * 2;
    const float mean = k.stats[si], rstd = k.stats[si + 1], ma = k.bstats[si], mb = k.bstats[si + 1];
    const float4 xv = reinterpret_cast<const float4 *>(k.x)[e];
    const float4 dv = reinterpret_cast<const float4 *>(k.dy)[e];
    const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ds[4] = {dv.x, dv.y, dv.z, dv.w};
    float rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (k.res) {
        const float4 rv = reinterpret_cast<const float4 *>(k.res)[e];
        rs[0] = rv.x; rs[1] = rv.y; rs[2] = rv.z; rs[3] = rv.w;
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float ga = k.gamma[cq * 4 + j];
        const float xh = (xs[j] - mean) * rstd;
        float dz = ds[j];
        if (k.silu) {
            const float z = fmaf(xh, ga, k.beta[cq * 4 + j]);
            const float sg = sigm(z);
            dz *= sg * (1.f + z * (1.f - sg));
        }
        o[j] = rstd * (dz * ga - ma - xh * mb) + rs[j];
    }
    reinterpret_cast<float4 *>(k.y)[e] = make_float4(o[0], o[1], o[2], o[3]);
}

// ---- attention helpers ----
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
struct SmK {
    const float *s;        // [N][Tp][Tp] scores (forward) / P (backward)
    const float *dp;       // backward: [N][Tp][Tp]
    float *out;            // P / dS
    int64_t rows;          // N Tp
    int T, Tp;
    float alpha;
};
// one wave per row; lanes stride the keys, the wave's sums in a fixed butterfly order
__global__ void __launch_bounds__(256) vae_softmax_kernel(SmK k)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= k.rows) return;
    const bool valid = (int)(row % k.Tp) < k.T;
    const float *s = k.s + (size_t)row * k.Tp;
    float *o = k.out + (size_t)row * k.Tp;
    if (!valid) {
        for (int j = lane; j < k.Tp; j += 64) o[j] = 0.f;
        return;
    }
    float m = -INFINITY;
    for (int j = lane; j < k.T; j += 64) m = fmaxf(m, s[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (int j = lane; j < k.T; j += 64) sum += expf(s[j] - m);
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int j = lane; j < k.Tp; j += 64) o[j] = j < k.T ? expf(s[j] - m) * inv : 0.f;
}
__global__ void __launch_bounds__(256) vae_softmax_bwd_kernel(SmK k)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= k.rows) return;
    const float *p = k.s + (size_t)row * k.Tp, *dp = k.dp + (size_t)row * k.Tp;
    float *o = k.out + (size_t)row * k.Tp;
    float d = 0.f;
    for (int j = lane; j < k.Tp; j += 64) d += p[j] * dp[j];
    d = wave_sum(d);
    for (int j = lane; j < k.Tp; j += 64) o[j] = k.alpha * (p[j] * (dp[j] - d));
}

struct TrK {
    const float *x;        // [B][R][ld], columns c0 .. c0 + C - 1
    float *y;              // [B][C][R]
    int64_t ld;
    int B, R, C, c0;
};
__global__ void __launch_bounds__(256) vae_transpose_kernel(TrK k)
{
    __shared__ float t[32][33];
    const int b = blockIdx.z, cb = blockIdx.x * 32, rb = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;       // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int rr = rb + r, cc = cb + tx;
        t[r][tx] = (rr < k.R && cc < k.C) ? k.x[((size_t)b * k.R + rr) * k.ld + k.c0 + cc] : 0.f;
    }
    __syncthreads();
    for (int c = ty; c < 32; c += 8) {
        const int cc = cb + c, rr = rb + tx;
        if (cc < k.C && rr < k.R) k.y[((size_t)b * k.C + cc) * k.R + rr] = t[tx][c];
    }
}

// ---- conv_in with the resize and x * 2 - 1 on load ----
struct Src1 { int i0, i1; float l0, l1; };
// torch's upsample_bilinear2d (align_corners=False, no scale factor): scale = in / out, src = max(scale (d + 0.5) - 0.5, 0)
__device__ __forceinline__ Src1 src_index(int d, int in, int out)
{
    const float scale = (float)in / (float)out;
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    Src1 r;
    r.i0 = (int)s;
    r.i1 = r.i0 + (r.i0 < in - 1 ? 1 : 0);
    r.l1 = s - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}
struct FirstK {
    const float *x;        // [N][3][H][W] at xs
    int64_t xs[4];
    int H, W, S;           // input and resized size
    const float *w, *bias; // torch [128][3][3][3]
    float *y;              // [N][S][S][128]
    const float *gpre;     // backward: [N][S][S][128]
    float *gxr;            // backward: [N][S][S][4] (3 used) gradient of the resized image (of x, before the * 2)
    const float *g_scale;  // backward, 16-bit precisions: the device scalar that multiplies here instead of at the head, or NULL
    float post;            // backward, 16-bit precisions: times this (undoes the head's pre-scale); 0: float32, neither is applied
    int64_t npix;          // N S S
};
// thread = (pixel, 32 output channels)
__global__ void __launch_bounds__(256) vae_first_kernel(FirstK k)
{
    __shared__ float Ws[CH * 27], Bs[CH];
    for (int e = threadIdx.x; e < CH * 27; e += 256) Ws[e] = k.w[e];
    if (threadIdx.x < CH) Bs[threadIdx.x] = k.bias[threadIdx.x];
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t p = t >> 2;
    const int co0 = (int)(t & 3) * 32;
    if (p >= k.npix) return;
    const int64_t ss = (int64_t)k.S * k.S;
    const int64_t n = p / ss;
    const int q = (int)(p - n * ss), y = q / k.S, x = q - y * k.S;
    float in[27];
#pragma unroll
    for (int t9 = 0; t9 < 9; t9++) {
        const int yy = y + t9 / 3 - 1, xx = x + t9 % 3 - 1;
        if (yy < 0 || yy >= k.S || xx < 0 || xx >= k.S) {            // zero padding of the resized, shifted image
#pragma unroll
            for (int c = 0; c < 3; c++) in[c * 9 + t9] = 0.f;
            continue;
        }
        const Src1 sy = src_index(yy, k.H, k.S), sx = src_index(xx, k.W, k.S);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float *b = k.x + n * k.xs[0] + c * k.xs[1];
            const float v00 = b[sy.i0 * k.xs[2] + sx.i0 * k.xs[3]], v01 = b[sy.i0 * k.xs[2] + sx.i1 * k.xs[3]];
            const float v10 = b[sy.i1 * k.xs[2] + sx.i0 * k.xs[3]], v11 = b[sy.i1 * k.xs[2] + sx.i1 * k.xs[3]];
            const float v = sy.l0 * (sx.l0 * v00 + sx.l1 * v01) + sy.l1 * (sx.l0 * v10 + sx.l1 * v11);
            in[c * 9 + t9] = v * 2.f - 1.f;
        }
    }
    float *out = k.y + (size_t)p * CH + co0;
    for (int o4 = 0; o4 < 8; o4++) {
        float acc[4];
#pragma unroll
        for (int o = 0; o < 4; o++) {
            const int co = co0 + o4 * 4 + o;
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 27; j++) a = fmaf(in[j], Ws[co * 27 + j], a);
            acc[o] = a + Bs[co];
        }
        *reinterpret_cast<float4 *>(out + o4 * 4) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
}

// thread = resized pixel: g[c] = 2 sum over the taps and 128 channels of gpre at the output pixel that reads it
__global__ void __launch_bounds__(256) vae_first_bwd_kernel(FirstK k)
{
    __shared__ float Ws[CH * 27];
    for (int e = threadIdx.x; e < CH * 27; e += 256) Ws[e] = k.w[e];
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= k.npix) return;
    const int64_t ss = (int64_t)k.S * k.S;
    const int64_t n = p / ss;
    const int q = (int)(p - n * ss), y = q / k.S, x = q - y * k.S;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int t9 = 0; t9 < 9; t9++) {
        const int oy = y - (t9 / 3 - 1), ox = x - (t9 % 3 - 1);
        if (oy < 0 || oy >= k.S || ox < 0 || ox >= k.S) continue;
        const float4 *g4 = reinterpret_cast<const float4 *>(k.gpre + ((size_t)n * ss + (size_t)oy * k.S + ox) * CH);
        for (int c4 = 0; c4 < CH / 4; c4++) {
            const float4 gv = g4[c4];
            const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
            for (int o = 0; o < 4; o++) {
                const int co = c4 * 4 + o;
#pragma unroll
                for (int ci = 0; ci < 3; ci++) acc[ci] = fmaf(gg[o], Ws[co * 27 + ci * 9 + t9], acc[ci]);
            }
        }
    }
    float o[3] = {2.f * acc[0], 2.f * acc[1], 2.f * acc[2]};
    if (k.post != 0.f) {
        // behind the last 16-bit product: the loss weight and the power of two are one exact factor, so one rounding each
        const float f = (k.g_scale ? k.g_scale[0] : 1.f) * k.post;
#pragma unroll
        for (int c = 0; c < 3; c++) o[c] *= f;
    }
    *reinterpret_cast<float4 *>(k.gxr + (size_t)p * 4) = make_float4(o[0], o[1], o[2], 0.f);
}

struct ResizeBwdK {
    const float *gxr;      // [N][S][S][4]
    float *g;              // [N][3][H][W] at gs
    int64_t gs[4];
    const float *scale;    // [N][H][W] at ss, or NULL
    int64_t ss[3];
    int H, W, S;
    int64_t npix;          // N H W
};
// the resized pixels that read input row i: src(d) within [i - 1, i + 1); the candidate window is widened by one on each side
// and every candidate is tested with the forward's own arithmetic
__device__ __forceinline__ void out_range(int i, int in, int out, int &lo, int &hi)
{
    const double sc = (double)out / (double)in;
    lo = max(0, (int)floor((i - 1 + 0.5) * sc - 0.5) - 1);
    hi = min(out - 1, (int)ceil((i + 1 + 0.5) * sc - 0.5) + 1);
}
__device__ __forceinline__ float weight_at(const Src1 &s, int i) { return (s.i0 == i ? s.l0 : 0.f) + (s.i1 == i ? s.l1 : 0.f); }
__global__ void __launch_bounds__(256) vae_resize_bwd_kernel(ResizeBwdK k)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= k.npix) return;
    const int64_t hw = (int64_t)k.H * k.W;
    const int64_t n = p / hw;
    const int q = (int)(p - n * hw), iy = q / k.W, ix = q - iy * k.W;
    int ylo, yhi, xlo, xhi;
    out_range(iy, k.H, k.S, ylo, yhi);
    out_range(ix, k.W, k.S, xlo, xhi);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int oy = ylo; oy <= yhi; oy++) {
        const float wy = weight_at(src_index(oy, k.H, k.S), iy);
        if (wy == 0.f) continue;
        for (int ox = xlo; ox <= xhi; ox++) {
            const float wx = weight_at(src_index(ox, k.W, k.S), ix);
            if (wx == 0.f) continue;
            const float4 gv = *reinterpret_cast<const float4 *>(k.gxr + (((size_t)n * k.S + oy) * k.S + ox) * 4);
            const float wgt = wy * wx;
            acc[0] = fmaf(wgt, gv.x, acc[0]);
            acc[1] = fmaf(wgt, gv.y, acc[1]);
            acc[2] = fmaf(wgt, gv.z, acc[2]);
        }
    }
    const float sc = k.scale ? k.scale[n * k.ss[0] + iy * k.ss[1] + ix * k.ss[2]] : 1.f;
#pragma unroll
    for (int c = 0; c < 3; c++) k.g[n * k.gs[0] + c * k.gs[1] + iy * k.gs[2] + ix * k.gs[3]] = k.scale ? acc[c] * sc : acc[c];
}

// ---- the head ----
struct HeadK {
    const float *xs;       // [N][h][w][512]: silu(norm_out(.))
    const float *cw, *cb;  // conv_out torch [8][512][3][3], [8]
    const float *qw, *qb;  // quant_conv [8][8], [8]
    float *m8;             // [N][h][w][8] conv_out's output / backward: its gradient
    const float *eps;      // [N][4][h][w]
    float *mean, *logvar, *lat, *dlv;   // [N][4][h][w]
    const float *g_lat, *g_scale;
    float pre;             // backward, 16-bit precisions: multiplies g_lat in place of *g_scale (1, or 2^10 at f16); 0: float32
    float *gx;             // backward: [N][h][w][512]
    float sf;
    int s;                 // h = w
    int64_t npix;          // N h w
};
// one wave per latent pixel: lane j holds channels j + 64 m
__global__ void __launch_bounds__(256) vae_conv_out_kernel(HeadK k)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= k.npix) return;
    const int64_t ss = (int64_t)k.s * k.s;
    const int64_t n = p / ss;
    const int q = (int)(p - n * ss), y = q / k.s, x = q - y * k.s;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t9 = 0; t9 < 9; t9++) {
        const int yy = y + t9 / 3 - 1, xx = x + t9 % 3 - 1;
        if (yy < 0 || yy >= k.s || xx < 0 || xx >= k.s) continue;
        const float *src = k.xs + ((size_t)n * ss + (size_t)yy * k.s + xx) * CMID;
#pragma unroll
        for (int m = 0; m < CMID / 64; m++) {
            const int ci = m * 64 + lane;
            const float v = src[ci];
#pragma unroll
            for (int o = 0; o < 8; o++) acc[o] = fmaf(v, k.cw[((size_t)o * CMID + ci) * 9 + t9], acc[o]);
        }
    }
#pragma unroll
    for (int o = 0; o < 8; o++) acc[o] = wave_sum(acc[o]);
    if (lane < 8) {
        float v = acc[0];
#pragma unroll
        for (int o = 1; o < 8; o++) v = lane == o ? acc[o] : v;
        k.m8[(size_t)p * 8 + lane] = v + k.cb[lane];
    }
}
// thread = (pixel, channel): g[ci] = sum over the taps and 8 outputs
__global__ void __launch_bounds__(256) vae_conv_out_bwd_kernel(HeadK k)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= k.npix * CMID) return;
    const int ci = (int)(e % CMID);
    const int64_t p = e / CMID;
    const int64_t ss = (int64_t)k.s * k.s;
    const int64_t n = p / ss;
    const int q = (int)(p - n * ss), y = q / k.s, x = q - y * k.s;
    float acc = 0.f;
    for (int t9 = 0; t9 < 9; t9++) {
        const int oy = y - (t9 / 3 - 1), ox = x - (t9 % 3 - 1);
        if (oy < 0 || oy >= k.s || ox < 0 || ox >= k.s) continue;
        const float *g = k.m8 + ((size_t)n * ss + (size_t)oy * k.s + ox) * 8;
#pragma unroll
        for (int o = 0; o < 8; o++) acc = fmaf(g[o], k.cw[((size_t)o * CMID + ci) * 9 + t9], acc);
    }
    k.gx[e] = acc;
}
// thread = latent pixel
__global__ void __launch_bounds__(256) vae_head_kernel(HeadK k)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= k.npix) return;
    const int64_t ss = (int64_t)k.s * k.s;
    const int64_t n = p / ss, q = p - n * ss;
    float m[8], mo[8];
#pragma unroll
    for (int j = 0; j < 8; j++) m[j] = k.m8[(size_t)p * 8 + j];
#pragma unroll
    for (int o = 0; o < 8; o++) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; j++) a = fmaf(k.qw[o * 8 + j], m[j], a);
        mo[o] = a + k.qb[o];
    }
#pragma unroll
    for (int c = 0; c < ZC; c++) {
        const size_t idx = ((size_t)n * ZC + c) * ss + q;
        const float lv = mo[ZC + c];
        const float lvc = fminf(fmaxf(lv, -30.f), 20.f);
        const float sd = expf(0.5f * lvc);
        if (k.mean) k.mean[idx] = mo[c];
        if (k.logvar) k.logvar[idx] = lvc;
        if (k.lat) {
            const float e = k.eps[idx];
            k.lat[idx] = k.sf * (mo[c] + sd * e);
            // torch's clamp passes the gradient at the bounds
            k.dlv[idx] = (lv >= -30.f && lv <= 20.f) ? k.sf * e * (0.5f * sd) : 0.f;
        }
    }
}
__global__ void __launch_bounds__(256) vae_head_bwd_kernel(HeadK k)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= k.npix) return;
    const int64_t ss = (int64_t)k.s * k.s;
    const int64_t n = p / ss, q = p - n * ss;
    const float gs = k.pre != 0.f ? k.pre : k.g_scale ? k.g_scale[0] : 1.f;
    float dmo[8];
#pragma unroll
    for (int c = 0; c < ZC; c++) {
        const size_t idx = ((size_t)n * ZC + c) * ss + q;
        const float gl = k.g_lat[idx] * gs;
        dmo[c] = k.sf * gl;
        dmo[ZC + c] = k.dlv[idx] * gl;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        float a = 0.f;
#pragma unroll
        for (int o = 0; o < 8; o++) a = fmaf(k.qw[o * 8 + j], dmo[o], a);
        k.m8[(size_t)p * 8 + j] = a;
    }
}

// ---- the loss tail ----
struct SdsK {
    SoarSdsArgs a;
    int64_t per;           // 4 h w
};
__device__ __forceinline__ int t_of(const SdsK &k)
{
    int64_t t = k.a.t[0];
    return (int)(t < 0 ? 0 : t >= k.a.n_timesteps ? k.a.n_timesteps - 1 : t);
}
// x_t = sqrt_ac[t] x0 + sqrt_1m_ac[t] noise: the one formula both kernels use
__device__ __forceinline__ float q_sample(const SdsK &k, int t, size_t i)
{
    return fmaf(k.a.tables[t], k.a.latents[i], k.a.tables[k.a.n_timesteps + t] * k.a.noise[i]);
}
__global__ void __launch_bounds__(256) sds_q_sample_kernel(SdsK k)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)k.a.B * k.per;
    if (i >= n) return;
    const float v = q_sample(k, t_of(k), (size_t)i);
    k.a.x_in[i] = v;
    k.a.x_in[n + i] = v;
}
constexpr int LOSS_THREADS = 1024;
__device__ double block_sum(double v, double *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int m = LOSS_THREADS / 2; m >= 1; m >>= 1) {
        if (t < m) sh[t] += sh[t + m];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}
// the x0 reconstructions of element i: recon (CFG) and, for the rescale, recon_nocfg (the text branch alone)
__device__ __forceinline__ void recon_of(const SdsK &k, int t, size_t i, float &rc, float &rt)
{
    const int64_t n = (int64_t)k.a.B * k.per;
    const float xt = q_sample(k, t, i);
    const float et = k.a.eps_pred[i], eu = k.a.eps_pred[n + i];
    const float e = eu + k.a.guidance_scale * (et - eu);
    const float sr = k.a.tables[2 * k.a.n_timesteps + t], srm = k.a.tables[3 * k.a.n_timesteps + t];
    rc = sr * xt - srm * e;
    rt = sr * xt - srm * et;
}
__global__ void __launch_bounds__(LOSS_THREADS) sds_loss_kernel(SdsK k)
{
    __shared__ double sh[LOSS_THREADS];
    const int tid = threadIdx.x;
    const int t = t_of(k);
    const int64_t n = (int64_t)k.a.B * k.per;
    const float invB = 1.f / (float)k.a.B;
    double l2 = 0.0;                       // sum of the per-element gradient's squares (before / B)
    if (k.a.mode == SOAR_SDS_RECON) {
        const bool rescale = k.a.recon_std_rescale > 0.f;
        const int ng = rescale ? k.a.B / k.a.n_view : 1;
        const int64_t gsz = rescale ? (int64_t)k.a.n_view * k.per : n;
        const float r = k.a.recon_std_rescale;
        for (int g = 0; g < ng; g++) {
            const int64_t e0 = (int64_t)g * gsz;
            float factor = 1.f;
            if (rescale) {
                // torch.std (unbiased) of recon_nocfg and recon over the group's n_view x 4 x h x w elements, two passes in double
                double s_c = 0.0, s_t = 0.0;
                for (int64_t i = e0 + tid; i < e0 + gsz; i += LOSS_THREADS) {
                    float rc, rt;
                    recon_of(k, t, (size_t)i, rc, rt);
                    s_c += rc; s_t += rt;
                }
                const double m_c = block_sum(s_c, sh) / (double)gsz, m_t = block_sum(s_t, sh) / (double)gsz;
                double v_c = 0.0, v_t = 0.0;
                for (int64_t i = e0 + tid; i < e0 + gsz; i += LOSS_THREADS) {
                    float rc, rt;
                    recon_of(k, t, (size_t)i, rc, rt);
                    v_c += (rc - m_c) * (rc - m_c);
                    v_t += (rt - m_t) * (rt - m_t);
                }
                const double d = (double)(gsz > 1 ? gsz - 1 : 1);
                const float sd_c = (float)sqrt(block_sum(v_c, sh) / d), sd_t = (float)sqrt(block_sum(v_t, sh) / d);
                factor = (sd_t + 1e-8f) / (sd_c + 1e-8f);
            }
            double acc = 0.0;
            for (int64_t i = e0 + tid; i < e0 + gsz; i += LOSS_THREADS) {
                float rc, rt;
                recon_of(k, t, (size_t)i, rc, rt);
                if (rescale) rc = r * (rc * factor) + (1.f - r) * rc;
                const float diff = k.a.latents[i] - rc;
                k.a.g_lat[i] = diff * invB;
                acc += (double)diff * (double)diff;
            }
            l2 += block_sum(acc, sh);
        }
        if (tid == 0) {
            k.a.loss[0] = (float)(0.5 * l2 / (double)k.a.B);
            k.a.grad_norm[0] = (float)(sqrt(l2) / (double)k.a.B);
        }
    } else {
        const float w = 1.f - k.a.tables[4 * k.a.n_timesteps + t];
        double acc = 0.0;
        for (int64_t i = tid; i < n; i += LOSS_THREADS) {
            const float et = k.a.eps_pred[i], eu = k.a.eps_pred[n + i];
            const float e = eu + k.a.guidance_scale * (et - eu);
            float g = w * (e - k.a.noise[i]);
            if (k.a.grad_clip > 0.f) g = fminf(fmaxf(g, -k.a.grad_clip), k.a.grad_clip);
            if (isnan(g)) g = 0.f;
            else if (isinf(g)) g = g > 0.f ? 3.402823466e38f : -3.402823466e38f;
            k.a.g_lat[i] = g * invB;
            acc += (double)g * (double)g;
        }
        l2 = block_sum(acc, sh);
        if (tid == 0) {
            k.a.loss[0] = (float)(0.5 * l2 / (double)k.a.B);
            k.a.grad_norm[0] = (float)sqrt(l2);
        }
    }
}

// ---- host side ----
struct Ctx {
    Dims d;
    WsLayout L;
    Layout W;
    const float *P;
    char *ws;
    hipStream_t stream;
    int wt;                // WT_*: what the packed B operands hold
    float *F(size_t off) const { return reinterpret_cast<float *>(ws + off); }
    const float *R(size_t off) const { return P + off; }
};

// conv over NHWC activations: side x side taps at offset off (3 x 3 pad 1: off = -1), stride 1, at level lev
ConvGemm conv_k(const Ctx &c, int lev, const float *x, int Cin, const float *w, int Cout, int side, int off, const float *bias,
                const float *res, float *y)
{
    ConvGemm k{};
    const int S = c.d.S[lev];
    k.x = x; k.ldx = Cin; k.xim = (int64_t)S * S;
    k.bias = bias; k.res = res; k.y = y; k.ldy = Cout; k.yim = (int64_t)S * S;
    k.alpha = 1.f;
    k.N = c.d.N; k.Hin = S; k.Win = S; k.Hg = S; k.Wg = S; k.Wout = S; k.os = 1; k.Cin = Cin; k.Cout = Cout;
    k.stride = 1; k.dil = 1; k.per_image = 1; k.nph = 1;
    square_taps(k.ph[0], w, (int64_t)side * side * Cin, side, off);
    return k;
}

// a product whose B operand is a packed weight tensor: at the context's operand type
int launch_w(const Ctx &c, ConvGemm k)
{
    k.wtype = c.wt;
    return launch_conv_gemm(k, c.stream);
}

int gn_forward(const Ctx &c, const float *x, int64_t hw, int C, const float *gamma, const float *beta, float *stats, float *y, int silu)
{
    GnK k{};
    k.x = x; k.y = y; k.gamma = gamma; k.beta = beta; k.stats = stats;
    k.part = reinterpret_cast<double *>(c.ws + c.L.part);
    k.hw = hw; k.C = C; k.nchunk = (int)((hw + CHUNK - 1) / CHUNK); k.silu = silu; k.bwd = 0;
    hipLaunchKernelGGL(vae_gn_partial_kernel, dim3((unsigned)k.nchunk, (unsigned)c.d.N), dim3(256), 0, c.stream, k);
    SOAR_LAUNCH_OK("vae_gn_partial", c.stream, 0);
    hipLaunchKernelGGL(vae_gn_final_kernel, dim3(blocks((int64_t)c.d.N * GROUPS)), dim3(256), 0, c.stream, k, c.d.N);
    SOAR_LAUNCH_OK("vae_gn_final", c.stream, 0);
    const int64_t n4 = (int64_t)c.d.N * hw * C / 4;
    hipLaunchKernelGGL(vae_gn_apply_kernel, dim3(blocks(n4)), dim3(256), 0, c.stream, k, n4);
    SOAR_LAUNCH_OK("vae_gn_apply", c.stream, 0);
    return 0;
}
// dx = GroupNorm(+SiLU)'s data gradient of dy, + res; dx may alias dy
int gn_backward(const Ctx &c, const float *x, int64_t hw, int C, const float *gamma, const float *beta, const float *stats,
                const float *dy, const float *res, float *dx, int silu)
{
    GnK k{};
    const int nchunk = (int)((hw + CHUNK - 1) / CHUNK);
    float *bst = c.F(c.L.part) + (size_t)c.d.N * nchunk * GROUPS * 2 * 2;     // the two means go behind the partial sums
    k.x = x; k.dy = dy; k.res = res; k.y = dx; k.gamma = gamma; k.beta = beta; k.stats = const_cast<float *>(stats);
    k.bstats = bst;
    k.part = reinterpret_cast<double *>(c.ws + c.L.part);
    k.hw = hw; k.C = C; k.nchunk = nchunk; k.silu = silu; k.bwd = 1;
    hipLaunchKernelGGL(vae_gn_partial_kernel, dim3((unsigned)k.nchunk, (unsigned)c.d.N), dim3(256), 0, c.stream, k);
    SOAR_LAUNCH_OK("vae_gn_partial", c.stream, 0);
    hipLaunchKernelGGL(vae_gn_final_kernel, dim3(blocks((int64_t)c.d.N * GROUPS)), dim3(256), 0, c.stream, k, c.d.N);
    SOAR_LAUNCH_OK("vae_gn_final", c.stream, 0);
    const int64_t n4 = (int64_t)c.d.N * hw * C / 4;
    hipLaunchKernelGGL(vae_gn_bwd_kernel, dim3(blocks(n4)), dim3(256), 0, c.stream, k, n4);
    SOAR_LAUNCH_OK("vae_gn_bwd", c.stream, 0);
    return 0;
}

int rb_forward(const Ctx &c, int lev, const RB &b, const RBws &s, float *out)
{
    const int64_t hw = (int64_t)c.d.S[lev] * c.d.S[lev];
    const float *x = c.F(s.x);
    float *tmp = c.F(c.L.tmp), *h1 = c.F(s.h1);
    if (gn_forward(c, x, hw, b.cin, c.R(b.n1g), c.R(b.n1b), c.F(s.st1), tmp, 1)) return 1;
    if (launch_w(c, conv_k(c, lev, tmp, b.cin, c.R(b.c1f), b.cout, 3, -1, c.R(b.c1b), nullptr, h1))) return 1;
    if (gn_forward(c, h1, hw, b.cout, c.R(b.n2g), c.R(b.n2b), c.F(s.st2), tmp, 1)) return 1;
    const float *res = x;
    if (b.cin != b.cout) {
        ConvGemm k = conv_k(c, lev, x, b.cin, c.R(b.ninf), b.cout, 1, 0, c.R(b.ninb), nullptr, out);
        if (launch_w(c, k)) return 1;
        res = out;
    }
    return launch_w(c, conv_k(c, lev, tmp, b.cout, c.R(b.c2f), b.cout, 3, -1, c.R(b.c2b), res, out));
}
// g: gradient of the block's output (kept); writes the gradient of its input into gx.  t1 / t2: scratch at the level's size
int rb_backward(const Ctx &c, int lev, const RB &b, const RBws &s, const float *g, float *gx, float *t1, float *t2)
{
    const int64_t hw = (int64_t)c.d.S[lev] * c.d.S[lev];
    if (launch_w(c, conv_k(c, lev, g, b.cout, c.R(b.c2r), b.cout, 3, -1, nullptr, nullptr, t1))) return 1;
    if (gn_backward(c, c.F(s.h1), hw, b.cout, c.R(b.n2g), c.R(b.n2b), c.F(s.st2), t1, nullptr, t1, 1)) return 1;
    if (launch_w(c, conv_k(c, lev, t1, b.cout, c.R(b.c1r), b.cin, 3, -1, nullptr, nullptr, t2))) return 1;
    const float *res = g;
    if (b.cin != b.cout) {
        ConvGemm k = conv_k(c, lev, g, b.cout, c.R(b.ninr), b.cin, 1, 0, nullptr, nullptr, t1);
        if (launch_w(c, k)) return 1;
        res = t1;
    }
    return gn_backward(c, c.F(s.x), hw, b.cin, c.R(b.n1g), c.R(b.n1b), c.F(s.st1), t2, res, gx, 1);
}

int transpose(const Ctx &c, const float *x, int64_t ld, int R, int C, int c0, float *y)
{
    TrK k{};
    k.x = x; k.y = y; k.ld = ld; k.B = c.d.N; k.R = R; k.C = C; k.c0 = c0;
    hipLaunchKernelGGL(vae_transpose_kernel, dim3((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32), (unsigned)c.d.N), dim3(256), 0,
                       c.stream, k);
    SOAR_LAUNCH_OK("vae_transpose", c.stream, 0);
    return 0;
}
// a product of per-image row-major operands: y[i] (rows M, ldy) = alpha x[i] (M x K, ldx) B[i]^T with B[i] rows Cout x K at ldw
ConvGemm mm_k(const Ctx &c, const float *x, int64_t ldx, int64_t xim, int M, int K, const float *w, int64_t ldw, int64_t wbat, int Cout,
              float *y, int64_t ldy, int64_t yim)
{
    ConvGemm k{};
    k.x = x; k.ldx = ldx; k.xim = xim; k.wbat = wbat;
    k.y = y; k.ldy = ldy; k.yim = yim; k.alpha = 1.f;
    k.N = c.d.N; k.Hin = 1; k.Win = M; k.Hg = 1; k.Wg = M; k.Wout = M; k.os = 1; k.Cin = K; k.Cout = Cout;
    k.stride = 1; k.dil = 1; k.per_image = 1; k.nph = 1;
    square_taps(k.ph[0], w, ldw, 1, 0);
    return k;
}

int attn_forward(const Ctx &c)
{
    const Dims &d = c.d;
    const int T = d.T, Tp = d.Tp, C3 = 3 * CMID;
    const float *x = c.F(c.L.mid1_out);
    float *tmp = c.F(c.L.tmp), *qkv = c.F(c.L.qkv), *P = c.F(c.L.P), *vT = c.F(c.L.vT), *O = c.F(c.L.O);
    if (gn_forward(c, x, T, CMID, c.R(c.W.an_g), c.R(c.W.an_b), c.F(c.L.an_st), tmp, 0)) return 1;
    if (Tp != T) SOAR_HIP_OK(hipMemsetAsync(qkv, 0, (size_t)d.N * Tp * C3 * sizeof(float), c.stream));
    ConvGemm k = mm_k(c, tmp, CMID, T, T, CMID, c.R(c.W.qkv_f), CMID, 0, C3, qkv, C3, Tp);
    k.bias = c.R(c.W.qkv_b);
    if (launch_w(c, k)) return 1;
    // scores into the dP buffer, then P
    float *Sc = c.F(c.L.dP);
    k = mm_k(c, qkv, C3, Tp, Tp, CMID, qkv + CMID, C3, (int64_t)Tp * C3, Tp, Sc, Tp, Tp);
    k.alpha = 1.f / sqrtf((float)CMID);
    if (launch_conv_gemm(k, c.stream)) return 1;
    SmK sm{};
    sm.s = Sc; sm.out = P; sm.rows = (int64_t)d.N * Tp; sm.T = T; sm.Tp = Tp;
    hipLaunchKernelGGL(vae_softmax_kernel, dim3((unsigned)((sm.rows + 3) / 4)), dim3(256), 0, c.stream, sm);
    SOAR_LAUNCH_OK("vae_softmax", c.stream, 0);
    if (transpose(c, qkv, C3, Tp, CMID, 2 * CMID, vT)) return 1;
    if (launch_conv_gemm(mm_k(c, P, Tp, Tp, Tp, Tp, vT, Tp, (int64_t)CMID * Tp, CMID, O, CMID, Tp), c.stream)) return 1;
    k = mm_k(c, O, CMID, Tp, T, CMID, c.R(c.W.p_f), CMID, 0, CMID, c.F(c.L.attn_out), CMID, T);
    k.bias = c.R(c.W.p_b);
    k.res = x;
    return launch_w(c, k);
}
// g: gradient of the attention block's output; writes the gradient of its input into gx (t: scratch)
int attn_backward(const Ctx &c, const float *g, float *gx, float *t)
{
    const Dims &d = c.d;
    const int T = d.T, Tp = d.Tp, C3 = 3 * CMID;
    const float *qkv = c.F(c.L.qkv), *P = c.F(c.L.P);
    float *dO = c.F(c.L.dO), *dOT = c.F(c.L.dOT), *dP = c.F(c.L.dP), *XT = c.F(c.L.XT), *dqkv = c.F(c.L.dqkv);
    if (Tp != T) SOAR_HIP_OK(hipMemsetAsync(dO, 0, (size_t)d.N * Tp * CMID * sizeof(float), c.stream));
    if (launch_w(c, mm_k(c, g, CMID, T, T, CMID, c.R(c.W.p_r), CMID, 0, CMID, dO, CMID, Tp))) return 1;
    // dV = P^T dO
    if (transpose(c, P, Tp, Tp, Tp, 0, XT)) return 1;
    if (transpose(c, dO, CMID, Tp, CMID, 0, dOT)) return 1;
    if (launch_conv_gemm(mm_k(c, XT, Tp, Tp, Tp, Tp, dOT, Tp, (int64_t)CMID * Tp, CMID, dqkv + 2 * CMID, C3, Tp), c.stream)) return 1;
    // dP = dO V^T, dS in place
    if (launch_conv_gemm(mm_k(c, dO, CMID, Tp, Tp, CMID, qkv + 2 * CMID, C3, (int64_t)Tp * C3, Tp, dP, Tp, Tp), c.stream)) return 1;
    SmK sm{};
    sm.s = P; sm.dp = dP; sm.out = dP; sm.rows = (int64_t)d.N * Tp; sm.T = T; sm.Tp = Tp; sm.alpha = 1.f / sqrtf((float)CMID);
    hipLaunchKernelGGL(vae_softmax_bwd_kernel, dim3((unsigned)((sm.rows + 3) / 4)), dim3(256), 0, c.stream, sm);
    SOAR_LAUNCH_OK("vae_softmax_bwd", c.stream, 0);
    // dQ = dS K, dK = dS^T Q
    if (transpose(c, qkv, C3, Tp, CMID, CMID, dOT)) return 1;
    if (launch_conv_gemm(mm_k(c, dP, Tp, Tp, Tp, Tp, dOT, Tp, (int64_t)CMID * Tp, CMID, dqkv, C3, Tp), c.stream)) return 1;
    if (transpose(c, dP, Tp, Tp, Tp, 0, XT)) return 1;
    if (transpose(c, qkv, C3, Tp, CMID, 0, dOT)) return 1;
    if (launch_conv_gemm(mm_k(c, XT, Tp, Tp, Tp, Tp, dOT, Tp, (int64_t)CMID * Tp, CMID, dqkv + CMID, C3, Tp), c.stream)) return 1;
    // d(normed input) = [dQ dK dV] [Wq; Wk; Wv], then the GroupNorm (no SiLU) + the residual
    if (launch_w(c, mm_k(c, dqkv, C3, Tp, T, C3, c.R(c.W.qkv_r), C3, 0, CMID, t, CMID, T))) return 1;
    return gn_backward(c, c.F(c.L.mid1_out), T, CMID, c.R(c.W.an_g), c.R(c.W.an_b), c.F(c.L.an_st), t, g, gx, 0);
}

bool check_size(const char *what, int32_t N, int32_t H, int32_t W, int32_t S)
{
    if (N < 0) { set_error("%s: N must be >= 0 (got %d)", what, N); return false; }
    if (H <= 0 || W <= 0) { set_error("%s: H and W must be positive (got H=%d, W=%d)", what, H, W); return false; }
    if (S < 8 || S % 8) { set_error("%s: image_size must be a positive multiple of 8 (got %d)", what, S); return false; }
    if ((int64_t)N * S * S > MAX_PIX || (int64_t)N * H * W > MAX_PIX) {
        set_error("%s: need N * image_size^2 and N * H * W <= 2^28 (N=%d, H=%d, W=%d, image_size=%d)", what, N, H, W, S);
        return false;
    }
    return true;
}
bool check_args(const char *what, const SoarVaeArgs *a, const void *ws, size_t ws_bytes)
{
    if (!a) { set_error("%s: NULL args", what); return false; }
    if (!check_size(what, a->N, a->H, a->W, a->image_size)) return false;
    if (a->N == 0) return true;
    if (!a->weights) { set_error("%s: NULL weights", what); return false; }
    if ((uintptr_t)a->weights & (ALIGN - 1)) { set_error("%s: the packed weights must be 256-byte aligned", what); return false; }
    return workspace_ok(what, ws, ws_bytes, ws_layout(dims_of(a->N, a->image_size)).total, "soar_vae_workspace_bytes");
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" int soar_vae_weights_floats(size_t *floats)
{
    if (!floats) { set_error("soar_vae_weights_floats: NULL floats"); return 1; }
    *floats = layout().raw_total;
    return 0;
}

extern "C" int soar_vae_weights_bytes(size_t *bytes)
{
    if (!bytes) { set_error("soar_vae_weights_bytes: NULL bytes"); return 1; }
    *bytes = layout().total * sizeof(float);
    return 0;
}

static bool check_precision(const char *what, int32_t precision)
{
    if (precision >= WT_F32 && precision <= WT_F16) return true;
    set_error("%s: precision must be 0 (f32), 1 (bf16) or 2 (f16) (got %d)", what, precision);
    return false;
}

extern "C" int soar_vae_weights_bytes16(int32_t precision, size_t *bytes)
{
    if (!bytes) { set_error("soar_vae_weights_bytes16: NULL bytes"); return 1; }
    if (!check_precision("soar_vae_weights_bytes16", precision)) return 1;
    *bytes = layout(precision).total * sizeof(float);
    return 0;
}

// exact: the packed buffer must be exactly the precision's size (soar_vae_pack_weights16), or at least it (soar_vae_pack_weights)
static int vae_pack_weights(const char *me, const float *raw, size_t raw_floats, void *packed, size_t packed_bytes, int prec, bool exact,
                            void *stream_)
{
    const Layout L = layout(prec);
    if (!raw || raw_floats != L.raw_total) {
        set_error("%s: raw must hold %zu floats (got %zu%s)", me, L.raw_total, raw_floats, raw ? "" : ", NULL");
        return 1;
    }
    const size_t need = L.total * sizeof(float);
    if (!packed || (exact ? packed_bytes != need : packed_bytes < need) || ((uintptr_t)packed & (ALIGN - 1))) {
        if (exact) set_error("%s: packed must be %zu bytes at precision %d, 256-byte aligned (got %zu)", me, need, prec, packed_bytes);
        else set_error("%s: packed must be %zu bytes, 256-byte aligned (got %zu)", me, need, packed_bytes);
        return 1;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    float *P = static_cast<float *>(packed);
    SOAR_HIP_OK(hipMemcpyAsync(P, raw, L.raw_total * sizeof(float), hipMemcpyDeviceToDevice, stream));
    // fwd, bwd: the regions' offsets in floats; fcol, bcol: where inside them this tensor starts, in elements
    auto pack_at = [&](size_t src, size_t fwd, size_t fcol, size_t bwd, size_t bcol, int Cout, int Cin, int kk, int64_t ldb) -> int {
        if (!prec) return launch_conv_pack(raw + src, P + fwd + fcol, P + bwd + bcol, Cout, Cin, kk, ldb, stream);
        uint16_t *f16 = reinterpret_cast<uint16_t *>(P + fwd) + fcol, *b16 = reinterpret_cast<uint16_t *>(P + bwd) + bcol;
        if (launch_conv_pack16(raw + src, f16, Cout, Cin, Cin, kk, prec, stream)) return 1;
        return launch_conv_pack16_bwd(raw + src, b16, Cout, Cin, kk, ldb, Cout, prec, stream);
    };
    auto pack = [&](size_t src, size_t fwd, size_t bwd, int Cout, int Cin, int kk, int64_t ldb) {
        return pack_at(src, fwd, 0, bwd, 0, Cout, Cin, kk, ldb);
    };
    auto pack_rb = [&](const RB &b) -> int {
        if (pack(b.c1w, b.c1f, b.c1r, b.cout, b.cin, 9, b.cout)) return 1;
        if (pack(b.c2w, b.c2f, b.c2r, b.cout, b.cout, 9, b.cout)) return 1;
        if (b.cin != b.cout && pack(b.ninw, b.ninf, b.ninr, b.cout, b.cin, 1, b.cout)) return 1;
        return 0;
    };
    for (int l = 0; l < NLEV; l++) {
        for (int j = 0; j < 2; j++)
            if (pack_rb(L.rb[l][j])) return 1;
        if (l < 3 && pack(L.dw[l], L.df[l], L.dr[l], LEVC[l], LEVC[l], 9, LEVC[l])) return 1;
    }
    if (pack_rb(L.mid1) || pack_rb(L.mid2)) return 1;
    const size_t qkvw[3] = {L.q_w, L.k_w, L.v_w}, qkvb[3] = {L.q_b, L.k_b, L.v_b};
    for (int j = 0; j < 3; j++) {
        // forward rows j C .. of [3C][C]; data gradient columns j C .. of [C][3C]
        if (pack_at(qkvw[j], L.qkv_f, (size_t)j * CMID * CMID, L.qkv_r, (size_t)j * CMID, CMID, CMID, 1, 3 * CMID)) return 1;
        SOAR_HIP_OK(hipMemcpyAsync(P + L.qkv_b + (size_t)j * CMID, raw + qkvb[j], CMID * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    return pack(L.p_w, L.p_f, L.p_r, CMID, CMID, 1, CMID);
}

extern "C" int soar_vae_pack_weights(const float *raw, size_t raw_floats, void *packed, size_t packed_bytes, void *stream_)
{
    return vae_pack_weights("soar_vae_pack_weights", raw, raw_floats, packed, packed_bytes, WT_F32, false, stream_);
}

extern "C" int soar_vae_pack_weights16(const float *raw, size_t raw_floats, void *packed, size_t packed_bytes, int32_t precision,
                                       void *stream_)
{
    if (!check_precision("soar_vae_pack_weights16", precision)) return 1;
    return vae_pack_weights("soar_vae_pack_weights16", raw, raw_floats, packed, packed_bytes, precision, true, stream_);
}

extern "C" int soar_vae_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t image_size, size_t *bytes)
{
    if (!bytes) { set_error("soar_vae_workspace_bytes: NULL bytes"); return 1; }
    if (!check_size("soar_vae_workspace_bytes", N, H, W, image_size)) return 1;
    *bytes = ws_layout(dims_of(N, image_size)).total;
    return 0;
}

static int vae_forward(const char *me, const SoarVaeArgs *a, int prec, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_args(me, a, workspace, workspace_bytes)) return 1;
    if (a->N == 0) return 0;
    if (!a->x) { set_error("%s: NULL x", me); return 1; }
    if (a->latents && !a->eps) { set_error("%s: latents need eps (the posterior noise)", me); return 1; }
    if (!a->latents && !a->mean && !a->logvar) { set_error("%s: no output (latents, mean, logvar all NULL)", me); return 1; }
    Ctx c{};
    c.d = dims_of(a->N, a->image_size);
    c.L = ws_layout(c.d);
    c.W = layout(prec);
    c.wt = prec;
    c.P = static_cast<const float *>(a->weights);
    c.ws = static_cast<char *>(workspace);
    c.stream = static_cast<hipStream_t>(stream_);
    const Dims &d = c.d;

    FirstK fk{};
    fk.x = a->x;
    for (int j = 0; j < 4; j++) fk.xs[j] = a->x_stride[j];
    fk.H = a->H; fk.W = a->W; fk.S = d.S[0];
    fk.w = c.R(c.W.cin_w); fk.bias = c.R(c.W.cin_b); fk.y = c.F(c.L.t_in); fk.npix = d.pix(0);
    hipLaunchKernelGGL(vae_first_kernel, dim3(blocks(fk.npix * 4)), dim3(256), 0, c.stream, fk);
    SOAR_LAUNCH_OK("vae_first", c.stream, 0);
    for (int l = 0; l < NLEV; l++) {
        for (int j = 0; j < 2; j++)
            if (rb_forward(c, l, c.W.rb[l][j], c.L.rb[l][j], c.F(c.L.rb_out[l][j]))) return 1;
        if (l == 3) break;
        ConvGemm k = conv_k(c, l, c.F(c.L.rb_out[l][1]), LEVC[l], c.R(c.W.df[l]), LEVC[l], 3, 0, c.R(c.W.db[l]), nullptr, c.F(c.L.down[l]));
        k.Hg = k.Wg = k.Wout = d.S[l + 1]; k.yim = (int64_t)d.S[l + 1] * d.S[l + 1];
        k.stride = 2;                                 // taps at 0 .. 2: pad right / bottom by one, the bounds check loads the zeros
        if (launch_w(c, k)) return 1;
    }
    if (rb_forward(c, 3, c.W.mid1, c.L.mid1, c.F(c.L.mid1_out))) return 1;
    if (attn_forward(c)) return 1;
    if (rb_forward(c, 3, c.W.mid2, c.L.mid2, c.F(c.L.mid2_out))) return 1;
    const int64_t hw3 = (int64_t)d.S[3] * d.S[3];
    if (gn_forward(c, c.F(c.L.mid2_out), hw3, CMID, c.R(c.W.no_g), c.R(c.W.no_b), c.F(c.L.no_st), c.F(c.L.tmp), 1)) return 1;
    HeadK hk{};
    hk.xs = c.F(c.L.tmp); hk.cw = c.R(c.W.co_w); hk.cb = c.R(c.W.co_b); hk.qw = c.R(c.W.qc_w); hk.qb = c.R(c.W.qc_b);
    hk.m8 = c.F(c.L.m8); hk.eps = a->eps; hk.mean = a->mean; hk.logvar = a->logvar; hk.lat = a->latents; hk.dlv = c.F(c.L.dlv);
    hk.sf = a->scale_factor; hk.s = d.S[3]; hk.npix = d.pix(3);
    hipLaunchKernelGGL(vae_conv_out_kernel, dim3((unsigned)((hk.npix + 3) / 4)), dim3(256), 0, c.stream, hk);
    SOAR_LAUNCH_OK("vae_conv_out", c.stream, 0);
    hipLaunchKernelGGL(vae_head_kernel, dim3(blocks(hk.npix)), dim3(256), 0, c.stream, hk);
    SOAR_LAUNCH_OK("vae_head", c.stream, 0);
    return 0;
}

extern "C" int soar_vae_forward(const SoarVaeArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    return vae_forward("soar_vae_forward", a, WT_F32, workspace, workspace_bytes, stream_);
}

extern "C" int soar_vae_forward16(const SoarVaeArgs *a, int32_t precision, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_precision("soar_vae_forward16", precision)) return 1;
    return vae_forward("soar_vae_forward16", a, precision, workspace, workspace_bytes, stream_);
}

static int vae_backward(const char *me, const SoarVaeArgs *a, int prec, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_args(me, a, workspace, workspace_bytes)) return 1;
    if (a->N == 0) return 0;
    if (!a->g_latents || !a->g_x) { set_error("%s: NULL g_latents / g_x", me); return 1; }
    Ctx c{};
    c.d = dims_of(a->N, a->image_size);
    c.L = ws_layout(c.d);
    c.W = layout(prec);
    c.wt = prec;
    // 16-bit operands: the incoming weight (1e-4 in the shipped configs) would push the gradient below the types' range, so it
    // multiplies behind the last such product instead (the chain is linear); f16 also runs on g_latents 2^10.  Both powers are exact.
    const float pre = prec == WT_F16 ? 1024.f : 1.f;
    c.P = static_cast<const float *>(a->weights);
    c.ws = static_cast<char *>(workspace);
    c.stream = static_cast<hipStream_t>(stream_);
    const Dims &d = c.d;
    float *G[3] = {c.F(c.L.g[0]), c.F(c.L.g[1]), c.F(c.L.g[2])};

    HeadK hk{};
    hk.cw = c.R(c.W.co_w); hk.qw = c.R(c.W.qc_w); hk.m8 = c.F(c.L.g8); hk.dlv = c.F(c.L.dlv);
    hk.g_lat = a->g_latents; hk.g_scale = a->g_scale; hk.gx = G[0];
    if (prec) hk.pre = pre;
    hk.sf = a->scale_factor; hk.s = d.S[3]; hk.npix = d.pix(3);
    hipLaunchKernelGGL(vae_head_bwd_kernel, dim3(blocks(hk.npix)), dim3(256), 0, c.stream, hk);
    SOAR_LAUNCH_OK("vae_head_bwd", c.stream, 0);
    hipLaunchKernelGGL(vae_conv_out_bwd_kernel, dim3(blocks(hk.npix * CMID)), dim3(256), 0, c.stream, hk);
    SOAR_LAUNCH_OK("vae_conv_out_bwd", c.stream, 0);
    const int64_t hw3 = (int64_t)d.S[3] * d.S[3];
    // G[0]: the gradient of the current tensor; G[1], G[2]: scratch
    auto rot = [&]() { float *t = G[0]; G[0] = G[1]; G[1] = t; };
    if (gn_backward(c, c.F(c.L.mid2_out), hw3, CMID, c.R(c.W.no_g), c.R(c.W.no_b), c.F(c.L.no_st), G[0], nullptr, G[1], 1)) return 1;
    rot();
    if (rb_backward(c, 3, c.W.mid2, c.L.mid2, G[0], G[1], G[1], G[2])) return 1;
    rot();
    if (attn_backward(c, G[0], G[1], G[2])) return 1;
    rot();
    if (rb_backward(c, 3, c.W.mid1, c.L.mid1, G[0], G[1], G[1], G[2])) return 1;
    rot();
    for (int l = NLEV - 1; l >= 0; l--) {
        if (l < 3) {
            // the downsample's data gradient: a 3 x 3 pad-2-top-left convolution over the zero-dilated gradient (the padded row and
            // column are never produced)
            ConvGemm k = conv_k(c, l, G[0], LEVC[l], c.R(c.W.dr[l]), LEVC[l], 3, -2, nullptr, nullptr, G[1]);
            k.Hin = k.Win = d.S[l + 1]; k.xim = (int64_t)d.S[l + 1] * d.S[l + 1];
            k.dil = 2;
            if (launch_w(c, k)) return 1;
            rot();
        }
        for (int j = 1; j >= 0; j--) {
            if (rb_backward(c, l, c.W.rb[l][j], c.L.rb[l][j], G[0], G[1], G[1], G[2])) return 1;
            rot();
        }
    }
    FirstK fk{};
    fk.H = a->H; fk.W = a->W; fk.S = d.S[0];
    fk.w = c.R(c.W.cin_w); fk.gpre = G[0]; fk.gxr = c.F(c.L.gxr); fk.npix = d.pix(0);
    if (prec) { fk.g_scale = a->g_scale; fk.post = 1.f / pre; }
    hipLaunchKernelGGL(vae_first_bwd_kernel, dim3(blocks(fk.npix)), dim3(256), 0, c.stream, fk);
    SOAR_LAUNCH_OK("vae_first_bwd", c.stream, 0);
    ResizeBwdK rk{};
    rk.gxr = c.F(c.L.gxr); rk.g = a->g_x;
    for (int j = 0; j < 4; j++) rk.gs[j] = a->g_x_stride[j];
    rk.scale = a->grad_scale;
    for (int j = 0; j < 3; j++) rk.ss[j] = a->grad_scale_stride[j];
    rk.H = a->H; rk.W = a->W; rk.S = d.S[0]; rk.npix = (int64_t)a->N * a->H * a->W;
    hipLaunchKernelGGL(vae_resize_bwd_kernel, dim3(blocks(rk.npix)), dim3(256), 0, c.stream, rk);
    SOAR_LAUNCH_OK("vae_resize_bwd", c.stream, 0);
    return 0;
}

extern "C" int soar_vae_backward(const SoarVaeArgs *a, void *workspace, size_t workspace_bytes, void *stream_)
{
    return vae_backward("soar_vae_backward", a, WT_F32, workspace, workspace_bytes, stream_);
}

extern "C" int soar_vae_backward16(const SoarVaeArgs *a, int32_t precision, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!check_precision("soar_vae_backward16", precision)) return 1;
    return vae_backward("soar_vae_backward16", a, precision, workspace, workspace_bytes, stream_);
}

static bool check_sds(const char *what, const SoarSdsArgs *a)
{
    if (!a) { set_error("%s: NULL args", what); return false; }
    if (a->B < 0 || a->h < 0 || a->w < 0) { set_error("%s: B, h, w must be >= 0 (got %d, %d, %d)", what, a->B, a->h, a->w); return false; }
    if (a->n_timesteps <= 0) { set_error("%s: n_timesteps must be > 0 (got %d)", what, a->n_timesteps); return false; }
    if (a->B == 0) return true;
    if (!a->t || !a->tables || !a->latents || !a->noise) { set_error("%s: NULL t / tables / latents / noise", what); return false; }
    return true;
}

extern "C" int soar_sds_q_sample(const SoarSdsArgs *a, void *stream_)
{
    if (!check_sds("soar_sds_q_sample", a)) return 1;
    if (a->B == 0) return 0;
    if (!a->x_in) { set_error("soar_sds_q_sample: NULL x_in"); return 1; }
    SdsK k{};
    k.a = *a;
    k.per = (int64_t)ZC * a->h * a->w;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(sds_q_sample_kernel, dim3(blocks((int64_t)a->B * k.per)), dim3(256), 0, stream, k);
    SOAR_LAUNCH_OK("sds_q_sample", stream, 0);
    return 0;
}

extern "C" int soar_sds_loss(const SoarSdsArgs *a, void *stream_)
{
    if (!check_sds("soar_sds_loss", a)) return 1;
    if (a->mode != SOAR_SDS_RECON && a->mode != SOAR_SDS_PLAIN) { set_error("soar_sds_loss: mode must be 0 (SDS) or 1 (recon) (got %d)", a->mode); return 1; }
    if (a->mode == SOAR_SDS_RECON && a->recon_std_rescale > 0.f && (a->n_view <= 0 || a->B % a->n_view)) {
        set_error("soar_sds_loss: B must be a multiple of n_view for the std rescale (B=%d, n_view=%d)", a->B, a->n_view);
        return 1;
    }
    if (a->B == 0) return 0;
    if (!a->eps_pred || !a->loss || !a->grad_norm || !a->g_lat) { set_error("soar_sds_loss: NULL eps_pred / loss / grad_norm / g_lat"); return 1; }
    SdsK k{};
    k.a = *a;
    k.per = (int64_t)ZC * a->h * a->w;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(sds_loss_kernel, dim3(1), dim3(LOSS_THREADS), 0, stream, k);
    SOAR_LAUNCH_OK("sds_loss", stream, 0);
    return 0;
}
