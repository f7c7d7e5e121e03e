// sam.hip -- SAM (Segment Anything) for point prompts, forward only, float32 (soar_amd/sam.py).
//
//   sam_attn_kernel        (attention.hip) multi-head attention with the decomposed relative-position bias, windows and whole grids alike
//   ln_rows_kernel         (layer_norm.h) LayerNorm over the last axis (tokens, and the channels of an NHWC map), optionally GELU behind it
//   the rest               pre- and post-processing, Fourier features, the decoder's small attentions, the transposed convolutions
//                          and the hyper-network product: plain VALU kernels
// Every matrix product (linear layers, patch embedding, the neck's convolutions) is launch_conv_gemm (conv_gemm.h: gemm()).
// No atomics; no sum's order depends on the batch: a frame's result does not depend on its neighbours or its place among them.
#include "attention.h"
#include "layer_norm.h"
#include "net_weights.h"
#include "workspace.h"

namespace soar {
namespace {

constexpr int TOK_MAX = 64;            // decoder tokens per frame

// ---- the packed weights -----------------------------------------------------------------------------------------------------------
// tensors in the order of soar_amd.sam.tensor_keys
struct Layout : WeightPlan {
    size_t image_pe = 0;               // behind the tensors: the dense positional encoding, computed by the packer
    int enc_block0 = 3, neck0 = 0, prompt0 = 0, dec0 = 0, dec_layer0 = 0, final0 = 0, up0 = 0, hyper0 = 0, iou0 = 0;
};
constexpr int ENC_BLOCK_TENSORS = 14, DEC_LAYER_TENSORS = 36;

Layout make_layout(const SoarSamConfig &c)
{
    Layout L;
    auto add = [&](size_t n) { L.add(n); };
    const size_t g2 = (size_t)c.grid * c.grid, C = c.embed, P = c.out_chans, pp3 = (size_t)3 * c.patch * c.patch;
    add(g2 * C); add(C * pp3); add(C);
    for (int b = 0; b < c.depth; b++) {
        const size_t S = c.window[b] ? c.window[b] : c.grid;
        add(C); add(C); add(3 * C * C); add(3 * C); add((2 * S - 1) * c.head_dim); add((2 * S - 1) * c.head_dim);
        add(C * C); add(C); add(C); add(C); add((size_t)c.mlp * C); add(c.mlp); add((size_t)c.mlp * C); add(C);
    }
    L.neck0 = (int)L.off.size();
    add(P * C); add(P); add(P); add(P * P * 9); add(P); add(P);
    L.prompt0 = (int)L.off.size();
    add(P); add(P); add(P); add(P); add(P);                      // gaussian [2][P / 2], point_embeddings 0 and 1, not_a_point, no_mask
    L.dec0 = (int)L.off.size();
    add(P); add((size_t)c.mask_tokens * P);
    L.dec_layer0 = (int)L.off.size();
    auto attn = [&](size_t I) { for (int i = 0; i < 3; i++) { add(I * P); add(I); } add(P * I); add(P); };
    const size_t I = P / c.dec_down;
    for (int l = 0; l < c.dec_layers; l++) {
        attn(P); add(P); add(P);
        attn(I); add(P); add(P);
        add((size_t)c.dec_mlp * P); add(c.dec_mlp); add((size_t)c.dec_mlp * P); add(P); add(P); add(P);
        add(P); add(P); attn(I);
    }
    L.final0 = (int)L.off.size();
    attn(I); add(P); add(P);
    L.up0 = (int)L.off.size();
    add(P * (P / 4) * 4); add(P / 4); add(P / 4); add(P / 4); add((P / 4) * (P / 8) * 4); add(P / 8);
    L.hyper0 = (int)L.off.size();
    for (int m = 0; m < c.mask_tokens; m++)
        for (int l = 0; l < c.hyper_depth; l++) { const size_t o = l == c.hyper_depth - 1 ? P / 8 : P; add(o * P); add(o); }
    L.iou0 = (int)L.off.size();
    for (int l = 0; l < c.iou_depth; l++) {
        const size_t i = l == 0 ? P : (size_t)c.iou_hidden, o = l == c.iou_depth - 1 ? (size_t)c.mask_tokens : (size_t)c.iou_hidden;
        add(o * i); add(o);
    }
    L.image_pe = L.total;
    L.total += g2 * P;
    return L;
}

bool check_cfg(const SoarSamConfig *cp, const char *me)
{
    if (!cp) { set_error("%s: NULL cfg", me); return false; }
    const SoarSamConfig &c = *cp;
    bool ok = c.image_size >= 1 && c.patch >= 1 && c.grid >= 1 && c.grid <= ATTN_SIDE && (int64_t)c.grid * c.patch == c.image_size && c.embed >= 8 &&
              c.embed % 8 == 0 && c.depth >= 1 && c.depth <= SOAR_SAM_MAX_DEPTH && c.heads >= 1 && c.head_dim >= 4 && c.head_dim <= 96 &&
              c.head_dim % 4 == 0 && (int64_t)c.heads * c.head_dim == c.embed && c.mlp >= 8 && c.mlp % 8 == 0 && c.out_chans >= 8 &&
              c.out_chans % 8 == 0 && (3 * c.patch * c.patch) % 8 == 0 && c.dec_layers >= 1 && c.dec_layers <= 8 && c.dec_heads >= 1 &&
              c.dec_down >= 1 && c.out_chans % c.dec_down == 0 && (c.out_chans / c.dec_down) % 8 == 0 &&
              (c.out_chans / c.dec_down) % c.dec_heads == 0 && c.out_chans % c.dec_heads == 0 && c.out_chans / c.dec_heads <= 64 &&
              c.dec_mlp >= 8 && c.dec_mlp % 8 == 0 && c.mask_tokens >= 2 && c.mask_tokens <= 8 && c.hyper_depth >= 2 && c.hyper_depth <= 8 &&
              c.iou_depth >= 2 && c.iou_depth <= 8 && c.iou_hidden >= 8 && c.iou_hidden % 8 == 0;
    for (int b = 0; ok && b < c.depth; b++) ok = c.window[b] >= 0 && c.window[b] <= ATTN_SIDE;
    if (!ok)
        set_error("%s: a configuration the kernels cannot run (image_size=%d, patch=%d, grid=%d <= 64, embed=%d = heads %d x head_dim %d "
                  "<= 96, mlp=%d, out_chans=%d, decoder %d layers %d heads down %d mlp %d, mask_tokens=%d, hyper_depth=%d, iou %d x %d; "
                  "widths multiples of 8, head_dim of 4, windows 0 .. 64)", me, c.image_size, c.patch, c.grid, c.embed, c.heads, c.head_dim,
                  c.mlp, c.out_chans, c.dec_layers, c.dec_heads, c.dec_down, c.dec_mlp, c.mask_tokens, c.hyper_depth, c.iou_depth, c.iou_hidden);
    return ok;
}

// ---- small pieces ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) preprocess_kernel(const uint8_t *__restrict__ img, float *__restrict__ patches, int64_t total, int nh,
                                                         int nw, int grid, int patch)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int pp = patch * patch, K = 3 * pp;
    const int k = (int)(e % K);
    const int64_t tk = e / K;
    const int t = (int)(tk % (grid * grid)), b = (int)(tk / (grid * grid));
    const int ci = k / pp, ky = (k - ci * pp) / patch, kx = k - ci * pp - ky * patch;
    const int y = (t / grid) * patch + ky, x = (t % grid) * patch + kx;
    const float mean = ci == 0 ? 123.675f : ci == 1 ? 116.28f : 103.53f, sd = ci == 0 ? 58.395f : ci == 1 ? 57.12f : 57.375f;
    float v = 0.f;
    if (y < nh && x < nw) v = ((float)img[(((size_t)b * nh + y) * nw + x) * 3 + ci] - mean) / sd;
    patches[e] = v;
}

// y[e] = a[e] + b[e % period]
__global__ void __launch_bounds__(256) add_kernel(const float *__restrict__ a, const float *__restrict__ b, float *y, int64_t total, int64_t period)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) y[e] = a[e] + b[e % period];
}
int add(const float *a, const float *b, float *y, int64_t total, int64_t period, hipStream_t stream)
{
    if (total == 0) return 0;
    hipLaunchKernelGGL(add_kernel, dim3(blocks(total)), dim3(256), 0, stream, a, b, y, total, period);
    SOAR_LAUNCH_OK("sam_add", stream, 0);
    return 0;
}

// sin | cos of 2 pi ((2 x - 1, 2 y - 1) . G), G [2][half]
__device__ __forceinline__ float fourier(const float *__restrict__ G, int half, int d, float x, float y)
{
    const int f = d < half ? d : d - half;
    const float arg = 6.283185307179586f * ((2.f * x - 1.f) * G[f] + (2.f * y - 1.f) * G[half + f]);
    return d < half ? sinf(arg) : cosf(arg);
}
__global__ void __launch_bounds__(256) image_pe_kernel(const float *__restrict__ G, float *__restrict__ pe, int grid, int P)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= grid * grid * P) return;
    const int d = e % P, t = e / P;
    pe[e] = fourier(G, P / 2, d, ((float)(t % grid) + 0.5f) / (float)grid, ((float)(t / grid) + 0.5f) / (float)grid);
}
// tokens [B][T][P]: iou token, mask tokens, the frame's points, the padding point; zeros behind
__global__ void __launch_bounds__(256) tokens_kernel(const float *__restrict__ G, const float *__restrict__ pt_emb0, const float *__restrict__ pt_emb1,
                                                     const float *__restrict__ not_a_point, const float *__restrict__ iou_token,
                                                     const float *__restrict__ mask_tokens, const float *__restrict__ points,
                                                     const int32_t *__restrict__ labels, const int32_t *__restrict__ counts, float *tokens, int B,
                                                     int T, int P, int nm, int M, float sx, float sy, float image_size)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * T * P) return;
    const int d = e % P, t = (e / P) % T, b = e / (P * T);
    const int n = min(max(counts[b], 0), M), p = t - 1 - nm;
    float v = 0.f;
    if (t == 0) v = iou_token[d];
    else if (t <= nm) v = mask_tokens[(t - 1) * P + d];
    else if (p < n) {
        const float x = (points[((size_t)b * M + p) * 2] * sx + 0.5f) / image_size, y = (points[((size_t)b * M + p) * 2 + 1] * sy + 0.5f) / image_size;
        v = fourier(G, P / 2, d, x, y) + (labels[(size_t)b * M + p] ? pt_emb1[d] : pt_emb0[d]);
    } else if (p == n) v = not_a_point[d];
    tokens[e] = v;
}

// The decoder's attentions: q [B][Nq][I], k, v [B][Nk][I], heads of hd = I / heads <= 64 channels; a wave per (query, head, frame).
// With counts: frame b has 1 + nm + counts[b] + 1 tokens on the token side (qtok: the queries are tokens; ktok: the keys are).
__global__ void __launch_bounds__(64) small_attn_kernel(const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
                                                        float *__restrict__ out, int Nq, int Nk, int I, int hd, const int32_t *__restrict__ counts,
                                                        int extra, int M, int qtok, int ktok, float scale)
{
    const int qi = blockIdx.x, head = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
    const int ntok = extra + min(max(counts[b], 0), M);
    if (qtok && qi >= ntok) return;
    const int nk = ktok ? ntok : Nk;
    __shared__ float qs[64];
    if (lane < hd) qs[lane] = q[((size_t)b * Nq + qi) * I + head * hd + lane] * scale;
    __syncthreads();
    const float *kb = k + (size_t)b * Nk * I + head * hd, *vb = v + (size_t)b * Nk * I + head * hd;
    float mx = -INFINITY;
    for (int j = lane; j < nk; j += 64) {
        float s = 0.f;
        for (int d = 0; d < hd; d++) s += qs[d] * kb[(size_t)j * I + d];
        mx = fmaxf(mx, s);
    }
    for (int d = 32; d; d >>= 1) mx = fmaxf(mx, __shfl_xor(mx, d));
    float sum = 0.f, acc[64];
#pragma unroll
    for (int d = 0; d < 64; d++) acc[d] = 0.f;
    for (int j = lane; j < nk; j += 64) {
        float s = 0.f;
        for (int d = 0; d < hd; d++) s += qs[d] * kb[(size_t)j * I + d];
        const float p = expf(s - mx);
        sum += p;
#pragma unroll
        for (int d = 0; d < 64; d++)
            if (d < hd) acc[d] += p * vb[(size_t)j * I + d];
    }
    for (int d = 32; d; d >>= 1) sum += __shfl_xor(sum, d);
#pragma unroll
    for (int d = 0; d < 64; d++) {
        if (d < hd) {
            float t = acc[d];
            for (int x = 32; x; x >>= 1) t += __shfl_xor(t, x);
            if (lane == 0) out[((size_t)b * Nq + qi) * I + head * hd + d] = t / sum;
        }
    }
}

// ConvTranspose2d 2 x 2 stride 2 on NHWC: x [B][g][g][Cin] -> y [B][2 g][2 g][Cout]; w [ky kx][Cout][Cin] (packed)
__global__ void __launch_bounds__(256) convt_kernel(const float *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias,
                                                    float *__restrict__ y, int64_t total, int g, int Cin, int Cout, int act)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int co = (int)(e % Cout);
    const int64_t pix = e / Cout;
    const int ox = (int)(pix % (2 * g)), oy = (int)((pix / (2 * g)) % (2 * g)), b = (int)(pix / ((int64_t)4 * g * g));
    const float *xr = x + (((size_t)b * g + (oy >> 1)) * g + (ox >> 1)) * Cin;
    const float *wr = w + ((size_t)((oy & 1) * 2 + (ox & 1)) * Cout + co) * Cin;
    float s = 0.f;
    for (int ci = 0; ci < Cin; ci++) s += xr[ci] * wr[ci];
    s += bias[co];
    y[e] = act == ACT_GELU ? gelu_erf(s) : s;
}
// torch [Cin][Cout][2][2] -> [ky kx][Cout][Cin]
__global__ void __launch_bounds__(256) convt_pack_kernel(const float *__restrict__ w, float *__restrict__ out, int Cin, int Cout)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Cin * Cout * 4) return;
    const int t = e & 3, co = (e >> 2) % Cout, ci = (e >> 2) / Cout;
    out[((size_t)t * Cout + co) * Cin + ci] = w[e];
}
// masks [B][nm - 1][L L] = hyper [B][nm][Cu] (rows 1 ..) . up [B][L L][Cu]
__global__ void __launch_bounds__(256) hyper_kernel(const float *__restrict__ hyper, const float *__restrict__ up, float *__restrict__ masks,
                                                    int64_t total, int LL, int nm, int Cu)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int pix = (int)(e % LL), mk = (int)((e / LL) % (nm - 1)), b = (int)(e / ((int64_t)LL * (nm - 1)));
    const float *hr = hyper + ((size_t)b * nm + mk + 1) * Cu, *ur = up + ((size_t)b * LL + pix) * Cu;
    float s = 0.f;
    for (int c = 0; c < Cu; c++) s += hr[c] * ur[c];
    masks[e] = s;
}
// rows [B][row stride] of `n` floats gathered to [B][n] (the mask tokens' outputs of the IoU head)
__global__ void __launch_bounds__(256) gather_kernel(const float *__restrict__ src, float *__restrict__ dst, int B, int n, int stride, int first)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < B * n) dst[e] = src[(size_t)(e / n) * stride + first + e % n];
}

// F.interpolate(mode = "bilinear", align_corners = False): source coordinate and weights of output o
__device__ __forceinline__ void lerp_at(int o, float scale, int n, int &i0, int &i1, float &w1)
{
    float s = scale * ((float)o + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = min((int)s, n - 1);
    i1 = min(i0 + 1, n - 1);
    w1 = s - (float)i0;
}
__device__ __forceinline__ float bilerp(const float *__restrict__ p, int n, int y0, int y1, float wy, int x0, int x1, float wx)
{
    const float a = p[(size_t)y0 * n + x0], b = p[(size_t)y0 * n + x1], c = p[(size_t)y1 * n + x0], d = p[(size_t)y1 * n + x1];
    return (1.f - wy) * ((1.f - wx) * a + wx * b) + wy * ((1.f - wx) * c + wx * d);
}
// both interpolations at once: an output pixel takes four pixels of the image_size-squared map, each four of the low-resolution one
__global__ void __launch_bounds__(256) postprocess_kernel(const float *__restrict__ low, float *__restrict__ logits, uint8_t *__restrict__ masks,
                                                          int64_t total, int L, int S, int nh, int nw, int H, int W)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int x = (int)(e % W), y = (int)((e / W) % H);
    const float *p = low + (e / ((int64_t)W * H)) * L * L;
    int Y[2], X[2];
    float wy, wx;
    lerp_at(y, (float)nh / (float)H, nh, Y[0], Y[1], wy);
    lerp_at(x, (float)nw / (float)W, nw, X[0], X[1], wx);
    float v[2][2];
    const float s1 = (float)L / (float)S;
#pragma unroll
    for (int iy = 0; iy < 2; iy++)
#pragma unroll
        for (int ix = 0; ix < 2; ix++) {
            int y0, y1, x0, x1;
            float fy, fx;
            lerp_at(Y[iy], s1, L, y0, y1, fy);
            lerp_at(X[ix], s1, L, x0, x1, fx);
            v[iy][ix] = bilerp(p, L, y0, y1, fy, x0, x1, fx);
        }
    const float r = (1.f - wy) * ((1.f - wx) * v[0][0] + wx * v[0][1]) + wy * ((1.f - wx) * v[1][0] + wx * v[1][1]);
    if (logits) logits[e] = r;
    if (masks) masks[e] = r > 0.f ? 1 : 0;
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------
struct EncWs { float *x, *t, *qkv, *h, *n1, *n2; };
struct DecWs { float *q, *q0, *qpe, *keys, *kpe, *qp, *kp, *vp, *ao, *hid, *up1, *up2, *hy1, *hy2, *hin, *io1, *io2; };
size_t carve_enc(const SoarSamConfig &c, int B, void *base, EncWs *w)
{
    Carver cv(base);
    const size_t M = (size_t)B * c.grid * c.grid;
    EncWs e;
    e.x = cv.take<float>(M * c.embed); e.t = cv.take<float>(M * c.embed); e.qkv = cv.take<float>(M * 3 * c.embed); e.h = cv.take<float>(M * c.mlp);
    e.n1 = cv.take<float>(M * c.out_chans); e.n2 = cv.take<float>(M * c.out_chans);
    if (w) *w = e;
    return cv.bytes();
}
size_t carve_dec(const SoarSamConfig &c, int B, int T, void *base, DecWs *w)
{
    Carver cv(base);
    const size_t P = c.out_chans, HW = (size_t)c.grid * c.grid, R = HW > (size_t)T ? HW : (size_t)T, BT = (size_t)B * T;
    DecWs d;
    d.q = cv.take<float>(BT * P); d.q0 = cv.take<float>(BT * P); d.qpe = cv.take<float>(BT * P); d.keys = cv.take<float>(B * HW * P); d.kpe = cv.take<float>(B * HW * P);
    d.qp = cv.take<float>(B * R * P); d.kp = cv.take<float>(B * R * P); d.vp = cv.take<float>(B * R * P); d.ao = cv.take<float>(B * R * P); d.hid = cv.take<float>(BT * c.dec_mlp);
    d.up1 = cv.take<float>(B * HW * 4 * (P / 4)); d.up2 = cv.take<float>(B * HW * 16 * (P / 8));
    d.hy1 = cv.take<float>((size_t)B * c.mask_tokens * P); d.hy2 = cv.take<float>((size_t)B * c.mask_tokens * P); d.hin = cv.take<float>((size_t)B * c.mask_tokens * (P / 8));
    const size_t iw = (size_t)(c.iou_hidden > c.mask_tokens ? c.iou_hidden : c.mask_tokens);
    d.io1 = cv.take<float>(B * iw); d.io2 = cv.take<float>(B * iw);
    if (w) *w = d;
    return cv.bytes();
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_sam_weights_bytes(const SoarSamConfig *cfg, size_t *bytes, int32_t *count)
{
    if (!check_cfg(cfg, "soar_sam_weights_bytes")) return 1;
    if (!bytes) { set_error("soar_sam_weights_bytes: NULL bytes"); return 1; }
    const Layout L = make_layout(*cfg);
    *bytes = align_up(L.total * sizeof(float));
    if (count) *count = L.count();
    return 0;
}

int soar_sam_pack_weights(const SoarSamConfig *cfg, const float *const *tensors, int32_t count, void *packed, size_t packed_bytes, void *stream_)
{
    const char *me = "soar_sam_pack_weights";
    if (!check_cfg(cfg, me)) return 1;
    const SoarSamConfig &c = *cfg;
    const Layout L = make_layout(c);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int P = c.out_chans;
    const int neck_conv = L.neck0 + 3, upa = L.up0, upb = L.up0 + 4;
    auto special = [&](int i, const float *src, float *dst) -> int {
        if (i == neck_conv) return launch_conv_pack(src, dst, nullptr, P, P, 9, 0, stream);
        if (i != upa && i != upb) return PACK_COPY;
        const int Cin = i == upa ? P : P / 4, Cout = i == upa ? P / 4 : P / 8;
        hipLaunchKernelGGL(convt_pack_kernel, dim3(blocks((int64_t)Cin * Cout * 4)), dim3(256), 0, stream, src, dst, Cin, Cout);
        SOAR_LAUNCH_OK("sam_convt_pack", stream, 0);
        return 0;
    };
    if (pack_weights(L, tensors, nullptr, count, packed, packed_bytes, stream, me, special)) return 1;
    float *base = static_cast<float *>(packed);
    hipLaunchKernelGGL(image_pe_kernel, dim3(blocks((int64_t)c.grid * c.grid * P)), dim3(256), 0, stream, base + L.off[L.prompt0], base + L.image_pe, c.grid, P);
    SOAR_LAUNCH_OK("sam_image_pe", stream, 0);
    return 0;
}

int soar_sam_workspace_bytes(const SoarSamConfig *cfg, int32_t B, int32_t max_points, size_t *bytes)
{
    const char *me = "soar_sam_workspace_bytes";
    if (!check_cfg(cfg, me)) return 1;
    const int T = 1 + cfg->mask_tokens + max_points + 1;
    if (!bytes || B < 0 || B > 4096 || max_points < 0 || T > TOK_MAX) {
        set_error("%s: need bytes, 0 <= B <= 4096 and at most %d points a frame (B=%d, max_points=%d)", me, TOK_MAX - 2 - cfg->mask_tokens, B, max_points);
        return 1;
    }
    const size_t e = carve_enc(*cfg, B, nullptr, nullptr), d = carve_dec(*cfg, B, T, nullptr, nullptr);
    *bytes = e > d ? e : d;
    return 0;
}

int soar_sam_preprocess(const SoarSamConfig *cfg, int32_t B, int32_t nh, int32_t nw, const uint8_t *resized, float *patches, void *stream_)
{
    const char *me = "soar_sam_preprocess";
    if (!check_cfg(cfg, me)) return 1;
    if (B < 0 || B > 4096 || nh < 1 || nw < 1 || nh > cfg->image_size || nw > cfg->image_size) {
        set_error("%s: need 0 <= B <= 4096 and a resized frame of 1 .. image_size a side (B=%d, %d x %d, image_size=%d)", me, B, nh, nw, cfg->image_size);
        return 1;
    }
    if (B == 0) return 0;
    if (!resized || !patches) { set_error("%s: NULL resized or patches", me); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t total = (int64_t)B * cfg->image_size * cfg->image_size * 3;
    hipLaunchKernelGGL(preprocess_kernel, dim3(blocks(total)), dim3(256), 0, stream, resized, patches, total, nh, nw, cfg->grid, cfg->patch);
    SOAR_LAUNCH_OK("sam_preprocess", stream, 0);
    return 0;
}

int soar_sam_encode(const SoarSamConfig *cfg, const void *packed, const SoarSamEncodeArgs *args, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *me = "soar_sam_encode";
    if (!check_cfg(cfg, me)) return 1;
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarSamConfig &c = *cfg;
    const SoarSamEncodeArgs &a = *args;
    if (a.B < 0 || a.B > 4096 || a.block_begin < 0 || a.block_end < a.block_begin || a.block_end > c.depth) {
        set_error("%s: need 0 <= B <= 4096 and 0 <= block_begin <= block_end <= depth (B=%d, blocks %d .. %d of %d)", me, a.B, a.block_begin, a.block_end, c.depth);
        return 1;
    }
    if (a.B == 0) return 0;
    if (!packed || (!a.patches == !a.tokens_in) || (!a.tokens_out && !a.embeddings)) {
        set_error("%s: need packed weights, exactly one of patches and tokens_in, and tokens_out or embeddings", me);
        return 1;
    }
    if (!workspace_ok(me, workspace, workspace_bytes, carve_enc(c, a.B, nullptr, nullptr), "soar_sam_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Layout L = make_layout(c);
    const float *base = static_cast<const float *>(packed);
    auto W = [&](int i) { return base + L.off[i]; };
    EncWs w;
    carve_enc(c, a.B, workspace, &w);
    const int C = c.embed, g2 = c.grid * c.grid;
    const int64_t M = (int64_t)a.B * g2;
    if (a.patches) {
        const int K = 3 * c.patch * c.patch;
        for (int b = 0; b < a.B; b++)                            // pos_embed rides as the residual: one product per frame
            if (gemm(a.patches + (size_t)b * g2 * K, K, W(1), K, C, W(2), W(0), w.x + (size_t)b * g2 * C, C, g2, stream)) return 1;
    } else {
        SOAR_HIP_OK(hipMemcpyAsync(w.x, a.tokens_in, M * C * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    const float scale = 1.f / sqrtf((float)c.head_dim);
    for (int blk = a.block_begin; blk < a.block_end; blk++) {
        const int t0 = L.enc_block0 + ENC_BLOCK_TENSORS * blk;
        if (layer_norm(w.x, W(t0), W(t0 + 1), w.t, M, C, 1e-6f, ACT_NONE, stream)) return 1;
        if (gemm(w.t, C, W(t0 + 2), C, 3 * C, W(t0 + 3), nullptr, w.qkv, 3 * C, M, stream)) return 1;
        if (launch_sam_attention(w.qkv, W(t0 + 3), W(t0 + 4), W(t0 + 5), w.t, a.B, c.grid, c.grid, c.heads, c.head_dim, c.window[blk], scale, stream)) return 1;
        if (gemm(w.t, C, W(t0 + 6), C, C, W(t0 + 7), w.x, w.x, C, M, stream)) return 1;
        if (layer_norm(w.x, W(t0 + 8), W(t0 + 9), w.t, M, C, 1e-6f, ACT_NONE, stream)) return 1;
        if (gemm(w.t, C, W(t0 + 10), C, c.mlp, W(t0 + 11), nullptr, w.h, c.mlp, M, stream, ACT_GELU)) return 1;
        if (gemm(w.h, c.mlp, W(t0 + 12), c.mlp, C, W(t0 + 13), w.x, w.x, C, M, stream)) return 1;
    }
    if (a.tokens_out) SOAR_HIP_OK(hipMemcpyAsync(a.tokens_out, w.x, M * C * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (a.embeddings) {
        const int P = c.out_chans, n0 = L.neck0;
        if (gemm(w.x, C, W(n0), C, P, nullptr, nullptr, w.n1, P, M, stream)) return 1;
        if (layer_norm(w.n1, W(n0 + 1), W(n0 + 2), w.n1, M, P, 1e-6f, ACT_NONE, stream)) return 1;
        ConvGemm k{};
        k.x = w.n1; k.ldx = P; k.xim = g2; k.y = w.n2; k.ldy = P; k.yim = g2; k.alpha = 1.f;
        k.N = a.B; k.Hg = k.Wg = k.Hin = k.Win = k.Wout = c.grid; k.Cin = k.Cout = P; k.stride = 1; k.dil = 1; k.os = 1; k.nph = 1;
        square_taps(k.ph[0], W(n0 + 3), (int64_t)9 * P, 3, -1);
        if (launch_conv_gemm(k, stream)) return 1;
        if (layer_norm(w.n2, W(n0 + 4), W(n0 + 5), a.embeddings, M, P, 1e-6f, ACT_NONE, stream)) return 1;
    }
    return 0;
}

int soar_sam_decode(const SoarSamConfig *cfg, const void *packed, const SoarSamDecodeArgs *args, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *me = "soar_sam_decode";
    if (!check_cfg(cfg, me)) return 1;
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarSamConfig &c = *cfg;
    const SoarSamDecodeArgs &a = *args;
    const int nm = c.mask_tokens, Mp = a.max_points, T = 1 + nm + Mp + 1;
    if (a.B < 0 || a.B > 4096 || Mp < 0 || T > TOK_MAX) {
        set_error("%s: need 0 <= B <= 4096 and at most %d points a frame (B=%d, max_points=%d)", me, TOK_MAX - 2 - nm, a.B, Mp);
        return 1;
    }
    if (a.B == 0) return 0;
    if (!packed || !a.embeddings || !a.counts || (Mp && (!a.points || !a.labels)) || !a.low_res || !a.iou) {
        set_error("%s: NULL packed weights, embeddings, counts, points, labels, low_res or iou", me);
        return 1;
    }
    if (!workspace_ok(me, workspace, workspace_bytes, carve_dec(c, a.B, T, nullptr, nullptr), "soar_sam_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Layout L = make_layout(c);
    const float *base = static_cast<const float *>(packed);
    auto W = [&](int i) { return base + L.off[i]; };
    DecWs w;
    carve_dec(c, a.B, T, workspace, &w);
    const int P = c.out_chans, B = a.B, HW = c.grid * c.grid, I2 = P / c.dec_down, extra = 2 + nm;
    const int64_t BT = (int64_t)B * T, BHW = (int64_t)B * HW;
    const float *image_pe = base + L.image_pe;

    hipLaunchKernelGGL(tokens_kernel, dim3(blocks(BT * P)), dim3(256), 0, stream, W(L.prompt0), W(L.prompt0 + 1), W(L.prompt0 + 2), W(L.prompt0 + 3),
                       W(L.dec0), W(L.dec0 + 1), a.points, a.labels, a.counts, w.q, B, T, P, nm, Mp, a.scale_x, a.scale_y, (float)c.image_size);
    SOAR_LAUNCH_OK("sam_tokens", stream, 0);
    SOAR_HIP_OK(hipMemcpyAsync(w.q0, w.q, BT * P * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (a.prompt_tokens) SOAR_HIP_OK(hipMemcpyAsync(a.prompt_tokens, w.q, BT * P * sizeof(float), hipMemcpyDeviceToDevice, stream));
    if (add(a.embeddings, W(L.prompt0 + 4), w.keys, BHW * P, P, stream)) return 1;       // + no_mask_embed

    // one attention module: projections, the small attention, the output projection with `res` added (NULL: replaces)
    auto attention = [&](int t0, int I, const float *qin, int64_t nq, const float *kin, const float *vin, int64_t nkv, bool qtok, bool ktok,
                         const float *res, float *out) -> int {
        const int Nq = qtok ? T : HW, Nk = ktok ? T : HW, hd = I / c.dec_heads;
        if (gemm(qin, P, W(t0), P, I, W(t0 + 1), nullptr, w.qp, I, nq, stream)) return 1;
        if (gemm(kin, P, W(t0 + 2), P, I, W(t0 + 3), nullptr, w.kp, I, nkv, stream)) return 1;
        if (gemm(vin, P, W(t0 + 4), P, I, W(t0 + 5), nullptr, w.vp, I, nkv, stream)) return 1;
        hipLaunchKernelGGL(small_attn_kernel, dim3((unsigned)Nq, (unsigned)c.dec_heads, (unsigned)B), dim3(64), 0, stream, w.qp, w.kp, w.vp, w.ao, Nq, Nk,
                           I, hd, a.counts, extra, Mp, qtok ? 1 : 0, ktok ? 1 : 0, 1.f / sqrtf((float)hd));
        SOAR_LAUNCH_OK("sam_small_attn", stream, 0);
        return gemm(w.ao, I, W(t0 + 6), I, P, W(t0 + 7), res, out, P, nq, stream);
    };
    // (rows of w.ao that no query wrote -- unused token slots -- hold whatever was there; they feed only their own rows)
    SOAR_HIP_OK(hipMemsetAsync(w.ao, 0, (size_t)B * (HW > T ? HW : T) * P * sizeof(float), stream));
    for (int l = 0; l < c.dec_layers; l++) {
        const int t0 = L.dec_layer0 + DEC_LAYER_TENSORS * l;
        if (l == 0) {
            if (attention(t0, P, w.q, BT, w.q, w.q, BT, true, true, nullptr, w.q)) return 1;
        } else {
            if (add(w.q, w.q0, w.qpe, BT * P, BT * P, stream)) return 1;
            if (attention(t0, P, w.qpe, BT, w.qpe, w.q, BT, true, true, w.q, w.q)) return 1;
        }
        if (layer_norm(w.q, W(t0 + 8), W(t0 + 9), w.q, BT, P, 1e-5f, ACT_NONE, stream)) return 1;
        if (add(w.q, w.q0, w.qpe, BT * P, BT * P, stream)) return 1;
        if (add(w.keys, image_pe, w.kpe, BHW * P, (int64_t)HW * P, stream)) return 1;
        if (attention(t0 + 10, I2, w.qpe, BT, w.kpe, w.keys, BHW, true, false, w.q, w.q)) return 1;
        if (layer_norm(w.q, W(t0 + 18), W(t0 + 19), w.q, BT, P, 1e-5f, ACT_NONE, stream)) return 1;
        if (gemm(w.q, P, W(t0 + 20), P, c.dec_mlp, W(t0 + 21), nullptr, w.hid, c.dec_mlp, BT, stream, ACT_RELU)) return 1;
        if (gemm(w.hid, c.dec_mlp, W(t0 + 22), c.dec_mlp, P, W(t0 + 23), w.q, w.q, P, BT, stream)) return 1;
        if (layer_norm(w.q, W(t0 + 24), W(t0 + 25), w.q, BT, P, 1e-5f, ACT_NONE, stream)) return 1;
        if (add(w.q, w.q0, w.qpe, BT * P, BT * P, stream)) return 1;
        if (attention(t0 + 28, I2, w.kpe, BHW, w.qpe, w.q, BT, false, true, w.keys, w.keys)) return 1;
        if (layer_norm(w.keys, W(t0 + 26), W(t0 + 27), w.keys, BHW, P, 1e-5f, ACT_NONE, stream)) return 1;
    }
    if (add(w.q, w.q0, w.qpe, BT * P, BT * P, stream)) return 1;
    if (add(w.keys, image_pe, w.kpe, BHW * P, (int64_t)HW * P, stream)) return 1;
    if (attention(L.final0, I2, w.qpe, BT, w.kpe, w.keys, BHW, true, false, w.q, w.q)) return 1;
    if (layer_norm(w.q, W(L.final0 + 8), W(L.final0 + 9), w.q, BT, P, 1e-5f, ACT_NONE, stream)) return 1;
    if (a.tokens_out) SOAR_HIP_OK(hipMemcpyAsync(a.tokens_out, w.q, BT * P * sizeof(float), hipMemcpyDeviceToDevice, stream));

    // up-scaling
    const int C4 = P / 4, C8 = P / 8, g = c.grid;
    hipLaunchKernelGGL(convt_kernel, dim3(blocks(BHW * 4 * C4)), dim3(256), 0, stream, w.keys, W(L.up0), W(L.up0 + 1), w.up1, BHW * 4 * C4, g, P, C4, ACT_NONE);
    SOAR_LAUNCH_OK("sam_convt1", stream, 0);
    if (layer_norm(w.up1, W(L.up0 + 2), W(L.up0 + 3), w.up1, BHW * 4, C4, 1e-6f, ACT_GELU, stream)) return 1;
    hipLaunchKernelGGL(convt_kernel, dim3(blocks(BHW * 16 * C8)), dim3(256), 0, stream, w.up1, W(L.up0 + 4), W(L.up0 + 5), w.up2, BHW * 16 * C8, 2 * g, C4, C8, ACT_GELU);
    SOAR_LAUNCH_OK("sam_convt2", stream, 0);
    // hyper-networks: mask token m's row of every frame through its own MLP
    for (int mk = 0; mk < nm; mk++) {
        const float *x = w.q + (size_t)(1 + mk) * P;
        int64_t ldx = (int64_t)T * P;
        float *bufs[2] = {w.hy1 + (size_t)mk * P, w.hy2 + (size_t)mk * P};
        for (int l = 0; l < c.hyper_depth; l++) {
            const int t0 = L.hyper0 + 2 * (mk * c.hyper_depth + l);
            const bool last = l == c.hyper_depth - 1;
            float *y = last ? w.hin + (size_t)mk * C8 : bufs[l & 1];
            const int64_t ldy = last ? (int64_t)nm * C8 : (int64_t)nm * P;
            if (gemm(x, ldx, W(t0), P, last ? C8 : P, W(t0 + 1), nullptr, y, ldy, B, stream, last ? ACT_NONE : ACT_RELU)) return 1;
            x = y; ldx = ldy;
        }
    }
    const int64_t LL = (int64_t)16 * HW, total = (int64_t)B * (nm - 1) * LL;
    hipLaunchKernelGGL(hyper_kernel, dim3(blocks(total)), dim3(256), 0, stream, w.hin, w.up2, a.low_res, total, (int)LL, nm, C8);
    SOAR_LAUNCH_OK("sam_hyper", stream, 0);
    // IoU head on the iou token's row
    {
        const float *x = w.q;
        int64_t ldx = (int64_t)T * P;
        int K = P;
        float *bufs[2] = {w.io1, w.io2};
        const int iw = c.iou_hidden > nm ? c.iou_hidden : nm;
        for (int l = 0; l < c.iou_depth; l++) {
            const bool last = l == c.iou_depth - 1;
            const int N = last ? nm : c.iou_hidden;
            if (gemm(x, ldx, W(L.iou0 + 2 * l), K, N, W(L.iou0 + 2 * l + 1), nullptr, bufs[l & 1], iw, B, stream, last ? ACT_NONE : ACT_RELU)) return 1;
            x = bufs[l & 1]; ldx = iw; K = N;
        }
        hipLaunchKernelGGL(gather_kernel, dim3(blocks((int64_t)B * (nm - 1))), dim3(256), 0, stream, x, a.iou, B, nm - 1, iw, 1);
        SOAR_LAUNCH_OK("sam_iou_gather", stream, 0);
    }
    return 0;
}

int soar_sam_postprocess(int32_t B, int32_t K, int32_t L, int32_t image_size, int32_t nh, int32_t nw, int32_t H, int32_t W, const float *low_res,
                         float *logits, uint8_t *masks, void *stream_)
{
    const char *me = "soar_sam_postprocess";
    if (B < 0 || K < 1 || L < 1 || image_size < 1 || nh < 1 || nw < 1 || nh > image_size || nw > image_size || H < 1 || W < 1 || H > 65535 || W > 65535 ||
        B > 4096 || K > 64) {
        set_error("%s: bad sizes (B=%d, K=%d, L=%d, image_size=%d, resized %d x %d, frame %d x %d)", me, B, K, L, image_size, nh, nw, H, W);
        return 1;
    }
    if (B == 0) return 0;
    if (!low_res || (!logits && !masks)) { set_error("%s: NULL low_res, or neither logits nor masks", me); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int64_t total = (int64_t)B * K * H * W;
    hipLaunchKernelGGL(postprocess_kernel, dim3(blocks(total)), dim3(256), 0, stream, low_res, logits, masks, total, L, image_size, nh, nw, H, W);
    SOAR_LAUNCH_OK("sam_postprocess", stream, 0);
    return 0;
}

int soar_sam_attention(const float *qkv, const float *bias, const float *rel_h, const float *rel_w, float *out, int32_t B, int32_t gh, int32_t gw,
                       int32_t heads, int32_t hd, int32_t window, float scale, void *stream_)
{
    return launch_sam_attention(qkv, bias, rel_h, rel_w, out, B, gh, gw, heads, hd, window, scale, static_cast<hipStream_t>(stream_));
}

}  // extern "C"
