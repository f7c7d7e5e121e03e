// clip.hip -- the SDS guidance's conditioning, forward only, float32 (soar_amd/clip.py): the CLIP text and image
// encoders (one pre-LN transformer tower, causal for text) and IP-Adapter's image-token Resampler.
//
//   kv_attn_kernel         (attention.hip) the towers' self-attention -- causal for text, head dimension up to 96 -- and the Resampler's
//                          attention of a few queries over n + n_q keys
//   ln_rows_kernel         (layer_norm.h)
//   clip_embed_kernel      token embedding gather + position embedding
//   clip_patches_kernel    bytes -> (x / 255 - mean) / std, unfolded into the patch product's rows (K = 3 p^2 padded to a multiple of 8)
//   clip_class_pos_kernel  the class row and the position embedding, in place on the tokens
//   clip_repeat_kernel     the Resampler's latents, once per batch entry
// Every linear layer is launch_conv_gemm (conv_gemm.h: gemm()): bias, the erf GELU and the residual are its epilogue.  Tokens are
// [B][L][width].  precision 1 (bf16) or 2 (f16) in either configuration: the products' weights are packed as 16-bit values and every
// product runs on the 16-bit matrix core, its A operand rounded on load (conv_gemm16_kernel); attn_precision 1 or 2,
// independently: the attention runs as kv_attn16_kernel (attention.h's contract).  Everything in memory stays float32.
// No atomics; nothing depends on the batch: a sequence's result is the same bits alone and in any batch.
#include "attention.h"
#include "layer_norm.h"
#include "net_weights.h"
#include "workspace.h"

namespace soar {
namespace {

constexpr float LN_EPS = 1e-5f;
constexpr int BLOCK_TENSORS = 12;      // ln_1 w b, in_proj w b, out_proj w b, ln_2 w b, c_fc w b, c_proj w b
constexpr int LAYER_TENSORS = 11;      // norm1 w b, norm2 w b, to_q, to_kv, to_out, ff norm w b, ff in, ff out

// ---- where the tensors lie in the packed buffer --------------------------------------------------------------------------------------
struct Plan : WeightPlan {
    int pad_idx = -1, pad_rows = 0, pad_k = 0, pad_kp = 0;     // the patch convolution: rows of pad_k floats laid pad_kp apart
    int tok = 0, pos = 0, cls = -1, pre = -1, blocks = 0, fin = 0;
};

int patch_k(const SoarClipConfig &c) { return 3 * c.patch * c.patch; }
int patch_kp(const SoarClipConfig &c) { return (patch_k(c) + 7) / 8 * 8; }

Plan clip_plan(const SoarClipConfig &c)
{
    Plan P;
    const size_t W = c.width, M = c.mlp;
    P.half = c.precision != WT_F32;    // a product's B operand as 16-bit values
    auto mat = [&](size_t n) { return P.add(n, 0, true); };
    if (c.kind == SOAR_CLIP_TEXT) {
        P.tok = P.add((size_t)c.vocab * W);
        P.pos = P.add((size_t)c.tokens * W);
    } else {
        P.tok = P.pad_idx = P.add(W * patch_k(c), W * patch_kp(c), true);
        P.pad_rows = c.width; P.pad_k = patch_k(c); P.pad_kp = patch_kp(c);
        P.cls = P.add(W);
        P.pos = P.add((size_t)c.tokens * W);
        P.pre = P.add(W); P.add(W);
    }
    P.blocks = (int)P.off.size();
    for (int l = 0; l < c.layers; l++) {
        P.add(W); P.add(W); mat(3 * W * W); P.add(3 * W); mat(W * W); P.add(W);
        P.add(W); P.add(W); mat(M * W); P.add(M); mat(W * M); P.add(W);
    }
    P.fin = P.add(W); P.add(W);
    return P;
}

Plan resampler_plan(const SoarResamplerConfig &c)
{
    Plan P;
    const size_t D = c.dim, I = (size_t)c.heads * c.dim_head, F = c.ff;
    P.half = c.precision != WT_F32;
    auto mat = [&](size_t n) { return P.add(n, 0, true); };
    P.add((size_t)c.queries * D);                                // latents
    mat(D * c.emb); P.add(D);                                    // proj_in
    mat((size_t)c.out * D); P.add(c.out);                        // proj_out
    P.add(c.out); P.add(c.out);                                  // norm_out
    P.blocks = (int)P.off.size();
    for (int l = 0; l < c.depth; l++) {
        P.add(D); P.add(D); P.add(D); P.add(D); mat(I * D); mat(2 * I * D); mat(D * I);
        P.add(D); P.add(D); mat(F * D); mat(D * F);
    }
    return P;
}

bool check_precisions(int precision, int attn_precision, const char *me)
{
    if (precision < WT_F32 || precision > WT_F16) { set_error("%s: precision = %d: 0 f32, 1 bf16 or 2 f16", me, precision); return false; }
    if (attn_precision < WT_F32 || attn_precision > WT_F16) { set_error("%s: attn_precision = %d: 0 f32, 1 bf16 or 2 f16", me, attn_precision); return false; }
    return true;
}
bool check_clip(const SoarClipConfig *cp, const char *me)
{
    if (!cp) { set_error("%s: NULL cfg", me); return false; }
    const SoarClipConfig &c = *cp;
    if (c.kind != SOAR_CLIP_TEXT && c.kind != SOAR_CLIP_VISION) { set_error("%s: kind = %d is neither text (0) nor vision (1)", me, c.kind); return false; }
    if (c.width < 8 || c.width > 16384 || c.width % 8 || c.mlp < 8 || c.mlp > 65536 || c.mlp % 8) {
        set_error("%s: width = %d and mlp = %d must be multiples of 8 (the matrix products' k)", me, c.width, c.mlp);
        return false;
    }
    if (c.heads < 1 || c.width % c.heads) { set_error("%s: width = %d is no multiple of heads = %d", me, c.width, c.heads); return false; }
    const int hd = c.width / c.heads;
    if (hd % 4 || hd > 96) { set_error("%s: head_dim = %d: the attention kernel runs multiples of 4 up to 96", me, hd); return false; }
    if (c.layers < 0 || c.layers > SOAR_CLIP_MAX_LAYERS || c.tokens < 1 || c.tokens > 65535) {
        set_error("%s: need 0 .. %d layers and 1 .. 65535 tokens (layers=%d, tokens=%d)", me, SOAR_CLIP_MAX_LAYERS, c.layers, c.tokens);
        return false;
    }
    if (c.kind == SOAR_CLIP_TEXT && c.vocab < 1) { set_error("%s: vocab = %d below 1", me, c.vocab); return false; }
    if (c.kind == SOAR_CLIP_VISION && (c.patch < 1 || c.patch > 64 || c.grid < 1 || c.grid > 255 || c.tokens != 1 + c.grid * c.grid)) {
        set_error("%s: need patch in 1 .. 64, grid in 1 .. 255 and tokens = 1 + grid^2 (patch=%d, grid=%d, tokens=%d)", me, c.patch, c.grid, c.tokens);
        return false;
    }
    return check_precisions(c.precision, c.attn_precision, me);
}
bool check_clip_sizes(const SoarClipConfig &c, int B, int L, const char *me)
{
    if (B < 0 || B > 65535 || L < 1 || L > c.tokens || (c.kind == SOAR_CLIP_VISION && L != c.tokens)) {
        set_error("%s: need 0 <= B <= 65535 and %s (B=%d, L=%d)", me, c.kind == SOAR_CLIP_TEXT ? "1 <= L <= the context length" : "L = 1 + grid^2", B, L);
        return false;
    }
    return true;
}
bool check_resampler(const SoarResamplerConfig *cp, const char *me)
{
    if (!cp) { set_error("%s: NULL cfg", me); return false; }
    const SoarResamplerConfig &c = *cp;
    if (c.dim < 8 || c.dim % 8 || c.emb < 8 || c.emb % 8 || c.ff < 8 || c.ff % 8 || c.dim > 16384 || c.emb > 16384 || c.ff > 65536) {
        set_error("%s: dim = %d, emb = %d and ff = %d must be multiples of 8 (the matrix products' k)", me, c.dim, c.emb, c.ff);
        return false;
    }
    if (c.dim_head < 4 || c.dim_head % 4 || c.dim_head > 96) { set_error("%s: dim_head = %d: the attention kernel runs multiples of 4 up to 96", me, c.dim_head); return false; }
    if (c.heads < 1 || c.heads > 4096 || (c.heads * c.dim_head) % 8) { set_error("%s: heads dim_head = %d x %d must be a multiple of 8", me, c.heads, c.dim_head); return false; }
    if (c.depth < 0 || c.depth > SOAR_CLIP_MAX_LAYERS || c.queries < 1 || c.queries > 65535 || c.out < 1 || c.out > 16384) {
        set_error("%s: need 0 .. %d layers, 1 .. 65535 queries and out from 1 (depth=%d, queries=%d, out=%d)", me, SOAR_CLIP_MAX_LAYERS, c.depth, c.queries, c.out);
        return false;
    }
    return check_precisions(c.precision, c.attn_precision, me);
}

// a linear layer on contiguous rows: y [M][Cout] = act(x [M][K] w[Cout][K]^T + bias) + res
int linear(const float *x, const float *w, int K, int Cout, const float *bias, const float *res, float *y, int64_t M, int act, int wtype, hipStream_t stream)
{
    return gemm(x, K, w, K, Cout, bias, res, y, Cout, M, stream, act, wtype);
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
// x [B L][W] = tok[ids] + pos[l], four channels a thread; an id outside the table is clamped (soar_amd/clip.py refuses it first)
__global__ void __launch_bounds__(256) clip_embed_kernel(const int32_t *__restrict__ ids, const float *__restrict__ tok, const float *__restrict__ pos,
                                                         float *__restrict__ x, int64_t total4, int L, int W, int vocab)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total4) return;
    const int q = W / 4, c = (int)(e % q);
    const int64_t row = e / q;
    const int id = min(max(ids[row], 0), vocab - 1), l = (int)(row % L);
    const float4 a = reinterpret_cast<const float4 *>(tok)[(size_t)id * q + c], b = reinterpret_cast<const float4 *>(pos)[(size_t)l * q + c];
    reinterpret_cast<float4 *>(x)[e] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
// img [B][S][S][3] bytes -> rows [B][g g][Kp]: element (ch p + py) p + px of token (ty, tx) is pixel (ty p + py, tx p + px)'s
// (byte / 255 - mean) / std, in that order of operations; elements K .. Kp - 1 are zeros
__global__ void __launch_bounds__(256) clip_patches_kernel(const uint8_t *__restrict__ img, float *__restrict__ rows, int64_t total, int g, int p, int Kp)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const float mean[3] = {0.48145466f, 0.4578275f, 0.40821073f}, sd[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    const int k = (int)(e % Kp);
    const int64_t t = e / Kp;
    if (k >= 3 * p * p) { rows[e] = 0.f; return; }
    const int px = k % p, py = (k / p) % p, ch = k / (p * p);
    const int tx = (int)(t % g), ty = (int)((t / g) % g);
    const int64_t b = t / ((int64_t)g * g);
    const int S = g * p;
    const float v = (float)img[((b * S + ty * p + py) * S + tx * p + px) * 3 + ch] / 255.f;
    rows[e] = (v - mean[ch]) / sd[ch];
}
// x [B][T][W]: row 0 = cls + pos[0]; row t = x + pos[t] (rows 1 .. T - 1 hold the patch product), four channels a thread
__global__ void __launch_bounds__(256) clip_class_pos_kernel(float *x, const float *__restrict__ cls, const float *__restrict__ pos, int64_t total4, int T, int W)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total4) return;
    const int q = W / 4, c = (int)(e % q), t = (int)((e / q) % T);
    const float4 a = t ? reinterpret_cast<const float4 *>(x)[e] : reinterpret_cast<const float4 *>(cls)[c];
    const float4 b = reinterpret_cast<const float4 *>(pos)[(size_t)t * q + c];
    reinterpret_cast<float4 *>(x)[e] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
// y [B][per] = src [per], four floats a thread
__global__ void __launch_bounds__(256) clip_repeat_kernel(const float *__restrict__ src, float *__restrict__ y, int64_t total4, int64_t per4)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total4) reinterpret_cast<float4 *>(y)[e] = reinterpret_cast<const float4 *>(src)[e % per4];
}

int attention(const float *q, const float *k, const float *v, float *out, int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int B, int Lq, int Lk,
              int heads, int hd, float scale, bool causal, int type, const char *me, hipStream_t stream)
{
    SoarUnetAttnArgs s{};
    s.q = q; s.k = k; s.v = v; s.out = out; s.ldq = ldq; s.ldk = ldk; s.ldv = ldv; s.ldo = ldo;
    s.B = B; s.Lq = Lq; s.Lk = Lk; s.heads = heads; s.hd = hd; s.scale = scale;
    return launch_attention(s, type, 96, causal, me, stream);
}

// ---- packing and probes, the same for the three networks ---------------------------------------------------------------------------
int pack(const Plan &P, int wtype, const float *const *tensors, const int64_t *sizes, int count, void *packed, size_t packed_bytes, void *stream_,
         const char *me)
{
    if (!sizes) { set_error("%s: NULL sizes", me); return 1; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    return pack_weights(P, tensors, sizes, count, packed, packed_bytes, stream, me, [&](int i, const float *src, float *dst) -> int {
        if (P.half && P.mat[i])                                  // a product's B operand: 16-bit, a matrix as one long row; the patch rows padded
            return i == P.pad_idx ? launch_conv_pack16(src, dst, P.pad_rows, P.pad_k, P.pad_kp, 1, wtype, stream)
                                  : launch_conv_pack16(src, dst, 1, (int)P.n[i], (int)P.n[i], 1, wtype, stream);
        if (i != P.pad_idx || P.pad_kp == P.pad_k) return PACK_COPY;
        SOAR_HIP_OK(hipMemsetAsync(dst, 0, (size_t)P.pad_rows * P.pad_kp * sizeof(float), stream));    // rows of K floats, laid Kp apart behind zeros
        SOAR_HIP_OK(hipMemcpy2DAsync(dst, P.pad_kp * sizeof(float), src, P.pad_k * sizeof(float), P.pad_k * sizeof(float), P.pad_rows,
                                     hipMemcpyDeviceToDevice, stream));
        return 0;
    });
}
bool check_probes(int n, const float *const *dst, const char *me)
{
    if (n < 0 || n > SOAR_CLIP_MAX_PROBES) { set_error("%s: %d probes: at most %d", me, n, SOAR_CLIP_MAX_PROBES); return false; }
    for (int i = 0; i < n; i++)
        if (!dst[i]) { set_error("%s: probe %d has no destination", me, i); return false; }
    return true;
}

struct ClipWs { float *x, *tn, *qkv, *ao, *ff; };
size_t clip_carve(const SoarClipConfig &c, int B, int L, void *base, ClipWs *out)
{
    Carver cv(base);
    ClipWs w;
    const size_t M = (size_t)B * L;
    w.x = cv.take<float>(M * c.width); w.tn = cv.take<float>(M * c.width); w.qkv = cv.take<float>(3 * M * c.width);
    w.ao = cv.take<float>(M * c.width); w.ff = cv.take<float>(M * c.mlp);
    if (out) *out = w;
    return cv.bytes();
}
struct ResWs { float *xp, *xn, *lat, *ln, *q, *kv, *ao, *ff, *po; };
size_t resampler_carve(const SoarResamplerConfig &c, int B, int n, void *base, ResWs *out)
{
    Carver cv(base);
    ResWs w;
    const size_t Mx = (size_t)B * n, Ml = (size_t)B * c.queries, I = (size_t)c.heads * c.dim_head;
    w.xp = cv.take<float>(Mx * c.dim); w.xn = cv.take<float>(Mx * c.dim); w.lat = cv.take<float>(Ml * c.dim); w.ln = cv.take<float>(Ml * c.dim);
    w.q = cv.take<float>(Ml * I); w.kv = cv.take<float>((Mx + Ml) * 2 * I); w.ao = cv.take<float>(Ml * I); w.ff = cv.take<float>(Ml * c.ff);
    w.po = cv.take<float>(Ml * c.out);
    if (out) *out = w;
    return cv.bytes();
}

}  // namespace
}  // namespace soar

using namespace soar;

extern "C" {

int soar_clip_weights_bytes(const SoarClipConfig *cfg, size_t *bytes, int32_t *count, size_t *floats)
{
    if (!check_clip(cfg, "soar_clip_weights_bytes")) return 1;
    if (!bytes) { set_error("soar_clip_weights_bytes: NULL bytes"); return 1; }
    const Plan P = clip_plan(*cfg);
    *bytes = align_up(P.total * sizeof(float));
    if (count) *count = P.count();
    if (floats) *floats = P.floats;
    return 0;
}

int soar_clip_pack_weights(const SoarClipConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                           size_t packed_bytes, void *stream)
{
    if (!check_clip(cfg, "soar_clip_pack_weights")) return 1;
    return pack(clip_plan(*cfg), cfg->precision, tensors, sizes, count, packed, packed_bytes, stream, "soar_clip_pack_weights");
}

int soar_clip_workspace_bytes(const SoarClipConfig *cfg, int32_t B, int32_t L, size_t *bytes)
{
    const char *me = "soar_clip_workspace_bytes";
    if (!check_clip(cfg, me)) return 1;
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (!check_clip_sizes(*cfg, B, L, me)) return 1;
    *bytes = clip_carve(*cfg, B, L, nullptr, nullptr);
    return 0;
}

int soar_clip_preprocess(const SoarClipConfig *cfg, int32_t B, const uint8_t *images, float *rows, void *stream_)
{
    const char *me = "soar_clip_preprocess";
    if (!check_clip(cfg, me)) return 1;
    if (cfg->kind != SOAR_CLIP_VISION || B < 0 || B > 65535) { set_error("%s: need a vision configuration and 0 <= B <= 65535 (B=%d)", me, B); return 1; }
    if (B == 0) return 0;
    if (!images || !rows) { set_error("%s: NULL images or rows", me); return 1; }
    const int64_t total = (int64_t)B * cfg->grid * cfg->grid * patch_kp(*cfg);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    hipLaunchKernelGGL(clip_patches_kernel, dim3(blocks(total)), dim3(256), 0, stream, images, rows, total, cfg->grid, cfg->patch, patch_kp(*cfg));
    SOAR_LAUNCH_OK("clip_patches", stream, 0);
    return 0;
}

int soar_clip_forward(const SoarClipConfig *cfg, const void *packed, const SoarClipArgs *args, void *workspace, size_t workspace_bytes, void *stream_)
{
    const char *me = "soar_clip_forward";
    if (!check_clip(cfg, me)) return 1;
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarClipConfig &c = *cfg;
    const SoarClipArgs &a = *args;
    if (!check_clip_sizes(c, a.B, a.L, me)) return 1;
    if (a.run_layers < 0 || a.run_layers > c.layers) { set_error("%s: run_layers = %d outside 0 .. %d", me, a.run_layers, c.layers); return 1; }
    if (!check_probes(a.n_probes, a.probe_dst, me)) return 1;
    if (a.B == 0) return 0;
    const bool text = c.kind == SOAR_CLIP_TEXT;
    if (!packed || !a.out || (text ? !a.ids : !a.patches)) { set_error("%s: NULL packed weights, out, or %s", me, text ? "ids" : "patches"); return 1; }
    if (!workspace_ok(me, workspace, workspace_bytes, clip_carve(c, a.B, a.L, nullptr, nullptr), "soar_clip_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Plan P = clip_plan(c);
    const float *base = static_cast<const float *>(packed);
    auto Wt = [&](int i) { return base + P.off[i]; };
    ClipWs w;
    clip_carve(c, a.B, a.L, workspace, &w);
    const int B = a.B, L = a.L, W = c.width, hd = W / c.heads, wt = c.precision;
    const int64_t M = (int64_t)B * L;
    auto probe = [&](int code, const float *src) -> int {
        for (int i = 0; i < a.n_probes; i++)
            if (a.probe_code[i] == code) SOAR_HIP_OK(hipMemcpyAsync(a.probe_dst[i], src, (size_t)M * W * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return 0;
    };

    if (text) {
        hipLaunchKernelGGL(clip_embed_kernel, dim3(blocks(M * W / 4)), dim3(256), 0, stream, a.ids, Wt(P.tok), Wt(P.pos), w.x, M * W / 4, L, W, c.vocab);
        SOAR_LAUNCH_OK("clip_embed", stream, 0);
        if (probe(SOAR_CLIP_PROBE_EMBED, w.x)) return 1;
    } else {
        // the patch product writes rows 1 .. of every image's tokens; the class row has no product row
        if (gemm(a.patches, P.pad_kp, Wt(P.tok), P.pad_kp, W, nullptr, nullptr, w.x + W, W, L - 1, stream, ACT_NONE, wt, B, L - 1, L)) return 1;
        hipLaunchKernelGGL(clip_class_pos_kernel, dim3(blocks(M * W / 4)), dim3(256), 0, stream, w.x, Wt(P.cls), Wt(P.pos), M * W / 4, L, W);
        SOAR_LAUNCH_OK("clip_class_pos", stream, 0);
        if (probe(SOAR_CLIP_PROBE_EMBED, w.x)) return 1;
        if (layer_norm(w.x, Wt(P.pre), Wt(P.pre + 1), w.x, M, W, LN_EPS, ACT_NONE, stream)) return 1;
        if (probe(SOAR_CLIP_PROBE_PRE, w.x)) return 1;
    }
    const float scale = 1.f / sqrtf((float)hd);
    for (int l = 0; l < a.run_layers; l++) {
        const int t0 = P.blocks + l * BLOCK_TENSORS;
        if (layer_norm(w.x, Wt(t0), Wt(t0 + 1), w.tn, M, W, LN_EPS, ACT_NONE, stream)) return 1;
        if (linear(w.tn, Wt(t0 + 2), W, 3 * W, Wt(t0 + 3), nullptr, w.qkv, M, ACT_NONE, wt, stream)) return 1;
        if (attention(w.qkv, w.qkv + W, w.qkv + 2 * W, w.ao, 3 * W, 3 * W, 3 * W, W, B, L, L, c.heads, hd, scale, text, c.attn_precision, "clip attention", stream)) return 1;
        if (linear(w.ao, Wt(t0 + 4), W, W, Wt(t0 + 5), w.x, w.x, M, ACT_NONE, wt, stream)) return 1;
        if (probe(2 * l, w.x)) return 1;
        if (layer_norm(w.x, Wt(t0 + 6), Wt(t0 + 7), w.tn, M, W, LN_EPS, ACT_NONE, stream)) return 1;
        if (linear(w.tn, Wt(t0 + 8), W, c.mlp, Wt(t0 + 9), nullptr, w.ff, M, ACT_GELU, wt, stream)) return 1;
        if (linear(w.ff, Wt(t0 + 10), c.mlp, W, Wt(t0 + 11), w.x, w.x, M, ACT_NONE, wt, stream)) return 1;
        if (probe(2 * l + 1, w.x)) return 1;
    }
    if (a.final_norm) return layer_norm(w.x, Wt(P.fin), Wt(P.fin + 1), a.out, M, W, LN_EPS, ACT_NONE, stream);
    SOAR_HIP_OK(hipMemcpyAsync(a.out, w.x, (size_t)M * W * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

int soar_clip_attention(const SoarClipAttnArgs *a, void *stream)
{
    if (!a) { set_error("soar_clip_attention: NULL args"); return 1; }
    return attention(a->q, a->k, a->v, a->out, a->ldq, a->ldk, a->ldv, a->ldo, a->B, a->Lq, a->Lk, a->heads, a->hd, a->scale, a->causal != 0,
                     WT_F32, "soar_clip_attention", static_cast<hipStream_t>(stream));
}

int soar_resampler_weights_bytes(const SoarResamplerConfig *cfg, size_t *bytes, int32_t *count, size_t *floats)
{
    if (!check_resampler(cfg, "soar_resampler_weights_bytes")) return 1;
    if (!bytes) { set_error("soar_resampler_weights_bytes: NULL bytes"); return 1; }
    const Plan P = resampler_plan(*cfg);
    *bytes = align_up(P.total * sizeof(float));
    if (count) *count = P.count();
    if (floats) *floats = P.floats;
    return 0;
}

int soar_resampler_pack_weights(const SoarResamplerConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                                size_t packed_bytes, void *stream)
{
    if (!check_resampler(cfg, "soar_resampler_pack_weights")) return 1;
    return pack(resampler_plan(*cfg), cfg->precision, tensors, sizes, count, packed, packed_bytes, stream, "soar_resampler_pack_weights");
}

int soar_resampler_workspace_bytes(const SoarResamplerConfig *cfg, int32_t B, int32_t n, size_t *bytes)
{
    const char *me = "soar_resampler_workspace_bytes";
    if (!check_resampler(cfg, me)) return 1;
    if (!bytes) { set_error("%s: NULL bytes", me); return 1; }
    if (B < 0 || B > 65535 || n < 1 || n > 65535) { set_error("%s: need 0 <= B <= 65535 and 1 <= n <= 65535 (B=%d, n=%d)", me, B, n); return 1; }
    *bytes = resampler_carve(*cfg, B, n, nullptr, nullptr);
    return 0;
}

int soar_resampler_forward(const SoarResamplerConfig *cfg, const void *packed, const SoarResamplerArgs *args, void *workspace, size_t workspace_bytes,
                           void *stream_)
{
    const char *me = "soar_resampler_forward";
    if (!check_resampler(cfg, me)) return 1;
    if (!args) { set_error("%s: NULL args", me); return 1; }
    const SoarResamplerConfig &c = *cfg;
    const SoarResamplerArgs &a = *args;
    if (a.B < 0 || a.B > 65535 || a.n < 1 || a.n > 65535) { set_error("%s: need 0 <= B <= 65535 and 1 <= n <= 65535 (B=%d, n=%d)", me, a.B, a.n); return 1; }
    if (!check_probes(a.n_probes, a.probe_dst, me)) return 1;
    if (a.B == 0) return 0;
    if (!packed || !a.x || !a.out) { set_error("%s: NULL packed weights, x or out", me); return 1; }
    if (!workspace_ok(me, workspace, workspace_bytes, resampler_carve(c, a.B, a.n, nullptr, nullptr), "soar_resampler_workspace_bytes")) return 1;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Plan P = resampler_plan(c);
    const float *base = static_cast<const float *>(packed);
    auto Wt = [&](int i) { return base + P.off[i]; };
    ResWs w;
    resampler_carve(c, a.B, a.n, workspace, &w);
    const int B = a.B, n = a.n, nq = c.queries, D = c.dim, I = c.heads * c.dim_head, keys = n + nq, wt = c.precision;
    const int64_t Mx = (int64_t)B * n, Ml = (int64_t)B * nq;
    auto probe = [&](int code, const float *src) -> int {
        for (int i = 0; i < a.n_probes; i++)
            if (a.probe_code[i] == code) SOAR_HIP_OK(hipMemcpyAsync(a.probe_dst[i], src, (size_t)Ml * D * sizeof(float), hipMemcpyDeviceToDevice, stream));
        return 0;
    };
    hipLaunchKernelGGL(clip_repeat_kernel, dim3(blocks(Ml * D / 4)), dim3(256), 0, stream, Wt(0), w.lat, Ml * D / 4, (int64_t)nq * D / 4);
    SOAR_LAUNCH_OK("clip_repeat", stream, 0);
    if (linear(a.x, Wt(1), c.emb, D, Wt(2), nullptr, w.xp, Mx, ACT_NONE, wt, stream)) return 1;
    // q and k are each scaled by dim_head^-0.25 in the definition; here the query carries both factors
    const float s = 1.f / sqrtf(sqrtf((float)c.dim_head));
    for (int l = 0; l < c.depth; l++) {
        const int t0 = P.blocks + l * LAYER_TENSORS;
        if (layer_norm(w.xp, Wt(t0), Wt(t0 + 1), w.xn, Mx, D, LN_EPS, ACT_NONE, stream)) return 1;
        if (layer_norm(w.lat, Wt(t0 + 2), Wt(t0 + 3), w.ln, Ml, D, LN_EPS, ACT_NONE, stream)) return 1;
        if (linear(w.ln, Wt(t0 + 4), D, I, nullptr, nullptr, w.q, Ml, ACT_NONE, wt, stream)) return 1;
        // k | v of the image tokens and of the latents into one buffer [B][n + nq][2 I]: one joint softmax, no concatenation
        if (gemm(w.xn, D, Wt(t0 + 5), D, 2 * I, nullptr, nullptr, w.kv, 2 * I, n, stream, ACT_NONE, wt, B, n, keys)) return 1;
        if (gemm(w.ln, D, Wt(t0 + 5), D, 2 * I, nullptr, nullptr, w.kv + (size_t)n * 2 * I, 2 * I, nq, stream, ACT_NONE, wt, B, nq, keys)) return 1;
        if (attention(w.q, w.kv, w.kv + I, w.ao, I, 2 * I, 2 * I, I, B, nq, keys, c.heads, c.dim_head, s * s, false, c.attn_precision, "resampler attention", stream)) return 1;
        if (linear(w.ao, Wt(t0 + 6), I, D, nullptr, w.lat, w.lat, Ml, ACT_NONE, wt, stream)) return 1;
        if (probe(2 * l, w.lat)) return 1;
        if (layer_norm(w.lat, Wt(t0 + 7), Wt(t0 + 8), w.ln, Ml, D, LN_EPS, ACT_NONE, stream)) return 1;
        if (linear(w.ln, Wt(t0 + 9), D, c.ff, nullptr, nullptr, w.ff, Ml, ACT_GELU, wt, stream)) return 1;
        if (linear(w.ff, Wt(t0 + 10), c.ff, D, nullptr, w.lat, w.lat, Ml, ACT_NONE, wt, stream)) return 1;
        if (probe(2 * l + 1, w.lat)) return 1;
    }
    if (linear(w.lat, Wt(3), D, c.out, Wt(4), nullptr, w.po, Ml, ACT_NONE, wt, stream)) return 1;
    return layer_norm(w.po, Wt(5), Wt(6), a.out, Ml, c.out, LN_EPS, ACT_NONE, stream);
}

}  // extern "C"
