"""The restatement of tests/clip_ref.py with 16-bit matrix products and / or the 16-bit attention (soar_amd/clip.py ``precision`` /
``attention_precision`` = ``"bf16"`` / ``"f16"``), in float64: with a 16-bit ``precision`` both operands of every
matrix product are rounded to the type (through float32, to nearest even, as the kernels round a float32 activation and the packer a
float32 weight); with a 16-bit ``attention_precision`` the attention is tests/unet_attn_half_ref.py's ``attention16``.  Everything else
-- embeddings, biases, norms, GELU, residuals -- is clip_ref's own float64 arithmetic, and with both at ``"f32"`` these functions are
clip_ref's."""
import math

import torch

import clip_ref as R
from unet_attn_half_ref import DTYPES, attention16, rounded

F64 = torch.float64


class _Ops:
    def __init__(self, precision, attention_precision):
        self.prec, self.attn = precision, attention_precision

    def mm(self, x, w):
        """x w^T"""
        if self.prec == "f32":
            return x @ w.T
        return rounded(x, DTYPES[self.prec]) @ rounded(w, DTYPES[self.prec]).T

    def attention(self, q, k, v, heads, scale=None, causal=False):
        if self.attn == "f32":
            return R.attention(q, k, v, heads, scale=scale, causal=causal)
        return attention16(q, k, v, heads, scale=scale, causal=causal, precision=self.attn)


def tower(ops, sd, pre, x, heads, layers, causal, stages):
    W = x.shape[-1]
    for i in range(layers):
        l1w, l1b, iw, ib, ow, ob, l2w, l2b, fw, fb, pw, pb = R._block_weights(sd, pre, i, F64)
        qkv = ops.mm(R.layer_norm(x, l1w, l1b), iw) + ib
        x = x + ops.mm(ops.attention(qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:], heads, causal=causal), ow) + ob
        stages[(i, "attn")] = x
        x = x + ops.mm(R.gelu(ops.mm(R.layer_norm(x, l2w, l2b), fw) + fb), pw) + pb
        stages[(i, "block")] = x
    return x


def text_forward(sd, cfg, ids, precision="f32", attention_precision="f32", skip_last=0, pre=""):
    """clip_ref.text_forward in float64 with the roundings"""
    ops = _Ops(precision, attention_precision)
    tok = R._first(sd, pre + "embeddings.token_embedding.weight", pre + "token_embedding.weight").to(F64)
    pos = R._first(sd, pre + "embeddings.position_embedding.weight", pre + "positional_embedding").to(F64)
    x = tok[ids.long()] + pos[:ids.shape[1]]
    stages = {("embed", ""): x}
    x = tower(ops, sd, pre, x, cfg["heads"], cfg["layers"] - skip_last, True, stages)
    w, b = R._first(sd, pre + "final_layer_norm.weight", pre + "ln_final.weight"), R._first(sd, pre + "final_layer_norm.bias", pre + "ln_final.bias")
    return R.layer_norm(x, w.to(F64), b.to(F64)), stages


def vision_forward(sd, cfg, pixels, precision="f32", attention_precision="f32", skip_last=0, post_norm=False, pre=""):
    """clip_ref.vision_forward in float64 with the roundings (the patch product is a product like the others)"""
    ops = _Ops(precision, attention_precision)
    g = lambda *keys: R._first(sd, *[pre + k for k in keys]).to(F64)
    conv = g("embeddings.patch_embedding.weight", "conv1.weight")
    W, p = conv.shape[0], cfg["patch"]
    B, gr = pixels.shape[0], cfg["image"] // cfg["patch"]
    rows = pixels.to(F64).reshape(B, 3, gr, p, gr, p).permute(0, 2, 4, 1, 3, 5).reshape(B, gr * gr, 3 * p * p)
    x = ops.mm(rows, conv.reshape(W, -1))
    cls = g("embeddings.class_embedding", "class_embedding")
    x = torch.cat([cls.expand(B, 1, W), x], dim=1) + g("embeddings.position_embedding.weight", "positional_embedding")
    stages = {("embed", ""): x}
    x = R.layer_norm(x, g("pre_layrnorm.weight", "ln_pre.weight"), g("pre_layrnorm.bias", "ln_pre.bias"))
    stages[("pre", "")] = x
    x = tower(ops, sd, pre, x, cfg["heads"], cfg["layers"] - skip_last, False, stages)
    if post_norm:
        x = R.layer_norm(x, g("post_layernorm.weight", "ln_post.weight"), g("post_layernorm.bias", "ln_post.bias"))
    return x, stages


def resampler_forward(sd, cfg, x, precision="f32", attention_precision="f32", pre=""):
    """clip_ref.resampler_forward in float64 with the roundings.  The 16-bit attention takes the query times dim_head^-0.5 and the keys
    as they are -- where its two roundings fall in the kernel -- instead of dim_head^-0.25 on each."""
    ops = _Ops(precision, attention_precision)
    g = lambda k: sd[pre + k].to(F64)
    x = x.to(F64)
    B, heads = x.shape[0], cfg["heads"]
    lat = g("latents").repeat(B, 1, 1)
    x = ops.mm(x, g("proj_in.weight")) + g("proj_in.bias")
    scale = 1 / math.sqrt(math.sqrt(cfg["dim_head"]))
    stages = {}
    for i in range(cfg["depth"]):
        p = f"layers.{i}."
        xn = R.layer_norm(x, g(p + "0.norm1.weight"), g(p + "0.norm1.bias"))
        ln = R.layer_norm(lat, g(p + "0.norm2.weight"), g(p + "0.norm2.bias"))
        q = ops.mm(ln, g(p + "0.to_q.weight"))
        k, v = ops.mm(torch.cat([xn, ln], dim=1), g(p + "0.to_kv.weight")).chunk(2, dim=-1)
        if attention_precision == "f32":
            a = R.attention(q * scale, k * scale, v, heads, scale=1.0)
        else:
            a = ops.attention(q, k, v, heads, scale=scale * scale)
        lat = lat + ops.mm(a, g(p + "0.to_out.weight"))
        stages[(i, "attn")] = lat
        h = R.layer_norm(lat, g(p + "1.0.weight"), g(p + "1.0.bias"))
        lat = lat + ops.mm(R.gelu(ops.mm(h, g(p + "1.1.weight"))), g(p + "1.3.weight"))
        stages[(i, "ff")] = lat
    out = ops.mm(lat, g("proj_out.weight")) + g("proj_out.bias")
    return R.layer_norm(out, g("norm_out.weight"), g("norm_out.bias")), stages
