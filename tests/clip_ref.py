"""Plain-torch restatement, in any dtype, of what soar_amd/clip.py computes: CLIP's text and image towers in transformers'
and open_clip's key layouts, IP-Adapter's Resampler, and the image preprocessing on top of jpeg_decode_ref's Pillow resize.  Also the
tiny configurations of the tests and seeded state dicts for them.

The two towers are checked against transformers' CLIPTextModel / CLIPVisionModel in float64 (tests/golden/clip_tiny.npz, written by
tests/tools/make_clip_golden.py, and live in tests/test_clip_cpu.py).  The Resampler has no independent implementation on the machine
this was written on: its restatement is the definition.
"""
import math

import numpy as np
import torch

import jpeg_decode_ref

# the smallest sizes at which the kernels can still go wrong (tests/test_clip_gpu.py says which path each one takes)
TEXT_A = dict(width=64, heads=2, layers=2, mlp=128, context=13, vocab=50)
TEXT_B = dict(width=128, heads=2, layers=3, mlp=256, context=150, vocab=50)
VISION_A = dict(width=160, heads=2, layers=2, mlp=320, patch=14, image=70)
VISION_B = dict(width=64, heads=2, layers=3, mlp=128, patch=14, image=168)
RESAMPLER_A = dict(dim=64, heads=2, dim_head=32, depth=2, queries=5, emb=160, out=48, ff=256)
RESAMPLER_B = dict(dim=128, heads=2, dim_head=64, depth=1, queries=16, emb=64, out=40, ff=512)
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def tokens_of(cfg):
    return 1 + (cfg["image"] // cfg["patch"]) ** 2


# ---- state dicts (transformers' bare keys, as CLIPTextModel / CLIPVisionModel save them) -----------------------------------------------
def _block_shapes(p, W, mlp):
    out = {}
    for n in ("layer_norm1", "layer_norm2"):
        out[p + n + ".weight"] = out[p + n + ".bias"] = (W,)
    for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
        out[p + "self_attn." + n + ".weight"] = (W, W)
        out[p + "self_attn." + n + ".bias"] = (W,)
    out[p + "mlp.fc1.weight"], out[p + "mlp.fc1.bias"] = (mlp, W), (mlp,)
    out[p + "mlp.fc2.weight"], out[p + "mlp.fc2.bias"] = (W, mlp), (W,)
    return out


def text_shapes(cfg):
    W = cfg["width"]
    out = {"embeddings.token_embedding.weight": (cfg["vocab"], W), "embeddings.position_embedding.weight": (cfg["context"], W)}
    for i in range(cfg["layers"]):
        out.update(_block_shapes(f"encoder.layers.{i}.", W, cfg["mlp"]))
    out["final_layer_norm.weight"] = out["final_layer_norm.bias"] = (W,)
    return out


def vision_shapes(cfg):
    W, p = cfg["width"], cfg["patch"]
    out = {"embeddings.class_embedding": (W,), "embeddings.patch_embedding.weight": (W, 3, p, p),
           "embeddings.position_embedding.weight": (tokens_of(cfg), W), "pre_layrnorm.weight": (W,), "pre_layrnorm.bias": (W,)}
    for i in range(cfg["layers"]):
        out.update(_block_shapes(f"encoder.layers.{i}.", W, cfg["mlp"]))
    out["post_layernorm.weight"] = out["post_layernorm.bias"] = (W,)
    return out


def resampler_shapes(cfg):
    D, I, F = cfg["dim"], cfg["heads"] * cfg["dim_head"], cfg["ff"]
    out = {"latents": (1, cfg["queries"], D), "proj_in.weight": (D, cfg["emb"]), "proj_in.bias": (D,), "proj_out.weight": (cfg["out"], D),
           "proj_out.bias": (cfg["out"],), "norm_out.weight": (cfg["out"],), "norm_out.bias": (cfg["out"],)}
    for i in range(cfg["depth"]):
        p = f"layers.{i}."
        for n in ("0.norm1", "0.norm2", "1.0"):
            out[p + n + ".weight"] = out[p + n + ".bias"] = (D,)
        out[p + "0.to_q.weight"], out[p + "0.to_kv.weight"], out[p + "0.to_out.weight"] = (I, D), (2 * I, D), (D, I)
        out[p + "1.1.weight"], out[p + "1.3.weight"] = (F, D), (D, F)
    return out


def tiny_state_dict(shapes, seed=0):
    """Random float32 weights that keep activations of order one: matrices ~ N(0, 1 / fan_in), norm gains near 1, small biases,
    embeddings of order one."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, s in shapes.items():
        norm = "norm" in k or k.endswith(("1.0.weight", "1.0.bias"))
        if k.endswith("bias"):
            sd[k] = 0.1 * torch.randn(s, generator=g)
        elif norm:
            sd[k] = 1.0 + 0.1 * torch.randn(s, generator=g)
        elif "embedding" in k and len(s) <= 2 or k == "latents":
            sd[k] = torch.randn(s, generator=g) * (0.5 if "position" in k else 1.0)
        else:
            sd[k] = torch.randn(s, generator=g) / math.sqrt(float(np.prod(s[1:])))
    return sd


def _rename_blocks(sd, out, src, dst, layers):
    names = {"layer_norm1": "ln_1", "layer_norm2": "ln_2", "self_attn.out_proj": "attn.out_proj", "mlp.fc1": "mlp.c_fc", "mlp.fc2": "mlp.c_proj"}
    for i in range(layers):
        a, b = f"{src}encoder.layers.{i}.", f"{dst}transformer.resblocks.{i}."
        for hf, oc in names.items():
            for kind in ("weight", "bias"):
                out[f"{b}{oc}.{kind}"] = sd[f"{a}{hf}.{kind}"]
        for kind in ("weight", "bias"):
            out[f"{b}attn.in_proj_{kind}"] = torch.cat([sd[f"{a}self_attn.{x}_proj.{kind}"] for x in "qkv"])


def to_open_clip_text(sd, cfg, prefix=""):
    """transformers' text keys -> open_clip's, q | k | v concatenated"""
    out = {prefix + "token_embedding.weight": sd["embeddings.token_embedding.weight"],
           prefix + "positional_embedding": sd["embeddings.position_embedding.weight"],
           prefix + "ln_final.weight": sd["final_layer_norm.weight"], prefix + "ln_final.bias": sd["final_layer_norm.bias"]}
    _rename_blocks(sd, out, "", prefix, cfg["layers"])
    return out


def to_open_clip_vision(sd, cfg, prefix=""):
    v = prefix + "visual."
    out = {v + "conv1.weight": sd["embeddings.patch_embedding.weight"], v + "class_embedding": sd["embeddings.class_embedding"],
           v + "positional_embedding": sd["embeddings.position_embedding.weight"], v + "ln_pre.weight": sd["pre_layrnorm.weight"],
           v + "ln_pre.bias": sd["pre_layrnorm.bias"], v + "ln_post.weight": sd["post_layernorm.weight"], v + "ln_post.bias": sd["post_layernorm.bias"]}
    _rename_blocks(sd, out, "", v, cfg["layers"])
    return out


# ---- the pieces -------------------------------------------------------------------------------------------------------------------------
def layer_norm(x, w, b, eps=1e-5):
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * w + b


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v, heads, scale=None, causal=False):
    """q [B,Lq,heads hd], k, v [B,Lk,heads hd] -> softmax(scale q k^T (+ causal mask)) v per head"""
    B, Lq, C = q.shape
    Lk, hd = k.shape[1], C // heads
    scale = hd ** -0.5 if scale is None else scale
    qh, kh, vh = (t.reshape(B, -1, heads, hd).transpose(1, 2) for t in (q, k, v))
    s = (qh * scale) @ kh.transpose(-1, -2)
    if causal:
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, dim=-1) @ vh).transpose(1, 2).reshape(B, Lq, C)


def _block_weights(sd, pre, i, dtype):
    """(ln_1 w b, in_proj w b, out_proj w b, ln_2 w b, c_fc w b, c_proj w b) of block i from either layout"""
    g = lambda k: sd[k].to(dtype)
    p = f"{pre}encoder.layers.{i}."
    if p + "layer_norm1.weight" in sd:
        cat = lambda kind: torch.cat([g(f"{p}self_attn.{x}_proj.{kind}") for x in "qkv"])
        return (g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"), cat("weight"), cat("bias"), g(p + "self_attn.out_proj.weight"),
                g(p + "self_attn.out_proj.bias"), g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"), g(p + "mlp.fc1.weight"),
                g(p + "mlp.fc1.bias"), g(p + "mlp.fc2.weight"), g(p + "mlp.fc2.bias"))
    p = f"{pre}transformer.resblocks.{i}."
    return tuple(g(p + n) for n in ("ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                                    "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight",
                                    "mlp.c_proj.bias"))


def tower(sd, pre, x, heads, layers, causal, dtype, stages):
    W = x.shape[-1]
    for i in range(layers):
        l1w, l1b, iw, ib, ow, ob, l2w, l2b, fw, fb, pw, pb = _block_weights(sd, pre, i, dtype)
        qkv = layer_norm(x, l1w, l1b) @ iw.T + ib
        x = x + attention(qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:], heads, causal=causal) @ ow.T + ob
        stages[(i, "attn")] = x
        x = x + gelu(layer_norm(x, l2w, l2b) @ fw.T + fb) @ pw.T + pb
        stages[(i, "block")] = x
    return x


def _first(sd, *keys):
    for k in keys:
        if k in sd:
            return sd[k]
    raise KeyError(keys)


def text_forward(sd, cfg, ids, dtype, skip_last=0, pre=""):
    """-> (final-normed tokens [B,L,W], stages: ("embed", ""), (i, "attn"), (i, "block"))"""
    tok = _first(sd, pre + "embeddings.token_embedding.weight", pre + "token_embedding.weight").to(dtype)
    pos = _first(sd, pre + "embeddings.position_embedding.weight", pre + "positional_embedding").to(dtype)
    x = tok[ids.long()] + pos[:ids.shape[1]]
    stages = {("embed", ""): x}
    x = tower(sd, pre, x, cfg["heads"], cfg["layers"] - skip_last, True, dtype, stages)
    w, b = _first(sd, pre + "final_layer_norm.weight", pre + "ln_final.weight"), _first(sd, pre + "final_layer_norm.bias", pre + "ln_final.bias")
    return layer_norm(x, w.to(dtype), b.to(dtype)), stages


def vision_forward(sd, cfg, pixels, dtype, skip_last=0, post_norm=False, pre=""):
    """pixels [B,3,S,S] (normalised) -> (tokens [B,1 + g g,W], stages: ("embed", ""), ("pre", ""), (i, "attn"), (i, "block"))"""
    g = lambda *keys: _first(sd, *[pre + k for k in keys]).to(dtype)
    conv = g("embeddings.patch_embedding.weight", "conv1.weight")
    W, p = conv.shape[0], cfg["patch"]
    B, gr = pixels.shape[0], cfg["image"] // cfg["patch"]
    rows = pixels.to(dtype).reshape(B, 3, gr, p, gr, p).permute(0, 2, 4, 1, 3, 5).reshape(B, gr * gr, 3 * p * p)
    x = rows @ conv.reshape(W, -1).T
    cls = g("embeddings.class_embedding", "class_embedding")
    x = torch.cat([cls.expand(B, 1, W), x], dim=1) + g("embeddings.position_embedding.weight", "positional_embedding")
    stages = {("embed", ""): x}
    x = layer_norm(x, g("pre_layrnorm.weight", "ln_pre.weight"), g("pre_layrnorm.bias", "ln_pre.bias"))
    stages[("pre", "")] = x
    x = tower(sd, pre, x, cfg["heads"], cfg["layers"] - skip_last, False, dtype, stages)
    if post_norm:
        x = layer_norm(x, g("post_layernorm.weight", "ln_post.weight"), g("post_layernorm.bias", "ln_post.bias"))
    return x, stages


def resampler_forward(sd, cfg, x, dtype, pre=""):
    """IP-Adapter's Resampler.forward: x [B,n,emb] -> (tokens [B,queries,out], stages: (i, "attn"), (i, "ff"))"""
    g = lambda k: sd[pre + k].to(dtype)
    x = x.to(dtype)
    B, heads = x.shape[0], cfg["heads"]
    lat = g("latents").repeat(B, 1, 1)
    x = x @ g("proj_in.weight").T + g("proj_in.bias")
    scale = 1 / math.sqrt(math.sqrt(cfg["dim_head"]))
    stages = {}
    for i in range(cfg["depth"]):
        p = f"layers.{i}."
        xn = layer_norm(x, g(p + "0.norm1.weight"), g(p + "0.norm1.bias"))
        ln = layer_norm(lat, g(p + "0.norm2.weight"), g(p + "0.norm2.bias"))
        q = ln @ g(p + "0.to_q.weight").T
        k, v = (torch.cat([xn, ln], dim=1) @ g(p + "0.to_kv.weight").T).chunk(2, dim=-1)
        # softmax((q scale) (k scale)^T) v: q and k each carry dim_head^-0.25
        lat = lat + attention(q * scale, k * scale, v, heads, scale=1.0) @ g(p + "0.to_out.weight").T
        stages[(i, "attn")] = lat
        h = layer_norm(lat, g(p + "1.0.weight"), g(p + "1.0.bias"))
        lat = lat + gelu(h @ g(p + "1.1.weight").T) @ g(p + "1.3.weight").T
        stages[(i, "ff")] = lat
    out = lat @ g("proj_out.weight").T + g("proj_out.bias")
    return layer_norm(out, g("norm_out.weight"), g("norm_out.bias")), stages


# ---- preprocessing ------------------------------------------------------------------------------------------------------------------------
def to_bytes(images):
    """to_pil_image: a float image times 255, truncated to a byte; [H,W,3] or [B,H,W,3] -> uint8 [B,H,W,3]"""
    x = images[None] if images.dim() == 3 else images
    return x if x.dtype == torch.uint8 else x.mul(255).to(torch.uint8)


def resized(images, S):
    """-> uint8 [B,S,S,3]: Resize((S, S), BICUBIC) of to_bytes(images), Pillow's bytes"""
    return torch.from_numpy(np.stack([jpeg_decode_ref.resize_bicubic(im.numpy(), S, S) for im in to_bytes(images)]))


def normalized(u8, dtype=torch.float32):
    """uint8 [B,S,S,3] -> [B,3,S,S]: to_tensor's x / 255 and Normalize's (x - mean) / std, each one operation in dtype"""
    x = u8.permute(0, 3, 1, 2).to(dtype) / 255
    return (x - torch.tensor(MEAN, dtype=dtype, device=x.device).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype, device=x.device).view(1, 3, 1, 1)


def patch_rows(pixels, patch):
    """[B,3,S,S] -> [B,g g,Kp]: a token's (channel, y, x) window, padded from 3 patch^2 to a multiple of 8 with zeros"""
    B, _, S, _ = pixels.shape
    g = S // patch
    rows = pixels.reshape(B, 3, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(B, g * g, 3 * patch * patch)
    return torch.nn.functional.pad(rows, (0, (-rows.shape[2]) % 8))


def sample_image(H, W, seed=0, as_float=False):
    """a smooth image with noise on it: uint8 [H,W,3], or float32 in 0 .. 1"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    img = torch.stack([xx, yy, 0.5 + 0.5 * torch.sin(6 * xx + 4 * yy)], dim=-1) * 0.8 + 0.2 * torch.rand(H, W, 3, generator=g)
    return img.clamp(0, 1) if as_float else (img.clamp(0, 1) * 255).to(torch.uint8)


# ---- tests/golden/clip_tiny.npz (tests/tools/make_clip_golden.py) ---------------------------------------------------------------------
def golden_values(grid):
    """{key: (int8 array, scale)} -> the float64 tensors the stored integers stand for; a norm's gain is 1 + that"""
    return {k: torch.from_numpy(q.astype(np.float64) * s + (1.0 if "norm" in k and k.endswith("weight") else 0.0)) for k, (q, s) in grid.items()}


def load_golden(path):
    """-> (text state dict, vision state dict, the other arrays), float64"""
    z = np.load(path)
    sds = {"text": {}, "vision": {}}
    rest = {}
    for k in z.files:
        name, kind, *key = k.split(".", 2)
        if kind == "q":
            sds[name][key[0]] = (z[k], float(z[f"{name}.s.{key[0]}"]))
        elif kind != "s":
            rest[k] = torch.from_numpy(z[k])
    return golden_values(sds["text"]), golden_values(sds["vision"]), rest
