"""Time the SDS guidance's conditioning (soar_amd/clip.py, csrc/clip.hip, csrc/attention.hip) at the shipped shapes with seeded random
weights (no checkpoint needed) against the same networks composed from torch-float32 operations (tests/clip_ref.py, its attention
replaced by ``F.scaled_dot_product_attention``) on the same GPU -> profiles/clip_time.json.

Reported: the ViT-H/14 image encoder (width 1280, 16 heads of 80, 32 blocks, 257 tokens) at 1 and 4 images of 224 x 224; the Resampler
(dim 1024, depth 4, 12 heads of 64, 16 queries) on one image's 257 tokens; ``ImageTokens`` end to end from a 1080 x 1920 float frame
(what a training step calls); the text encoder (width 1024, 16 heads of 64, 23 blocks) at 2 x 77 tokens.  Medians of device-event times
with the fastest and slowest call beside them.  The torch side of ``ImageTokens`` uses the library's Pillow-exact resize too: torch has
no equivalent of it.
"""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import clip_ref as R  # noqa: E402
from soar_amd import clip  # noqa: E402

VISION = dict(width=1280, heads=16, layers=32, mlp=5120, patch=14, image=224)
TEXT = dict(width=1024, heads=16, layers=23, mlp=4096, context=77, vocab=49408)
RESAMPLER = dict(dim=1024, heads=12, dim_head=64, depth=4, queries=16, emb=1280, out=1024, ff=4096)


def device_weights(shapes, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for key, shape in shapes.items():
        t = torch.randn(shape, generator=g, device="cuda")
        if len(shape) == 1 and ("norm" in key or key.endswith(("1.0.weight", "1.0.bias"))):
            sd[key] = (1.0 if key.endswith("weight") else 0.0) + 0.1 * t
        elif len(shape) == 1 or "embedding" in key and len(shape) == 2 or key == "latents":
            sd[key] = 0.1 * t if key.endswith("bias") else t
        else:
            sd[key] = t / float(np.prod(shape[1:])) ** 0.5
    return sd


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def sdpa_attention(q, k, v, heads, scale=None, causal=False):
    B, Lq, C = q.shape
    sp = lambda t: t.reshape(B, -1, heads, C // heads).transpose(1, 2)
    return F.scaled_dot_product_attention(sp(q), sp(k), sp(v), scale=scale, is_causal=causal).transpose(1, 2).reshape(B, Lq, C)


def distance(a, b):
    return ((a - b).abs().max() / b.pow(2).mean().sqrt()).item()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_time.json"))
    args = ap.parse_args()
    assert args.iters >= 5
    vsd, tsd, rsd = device_weights(R.vision_shapes(VISION), 0), device_weights(R.text_shapes(TEXT), 1), device_weights(R.resampler_shapes(RESAMPLER), 2)
    vnet = clip.ClipImageEncoder(vsd).to("cuda")
    tnet = clip.ClipTextEncoder(tsd).to("cuda")
    rnet = clip.Resampler(rsd).to("cuda")
    tokens = clip.ImageTokens(vnet, rnet)
    assert vnet.cfg["head_dim"] == 80 and vnet.cfg["tokens"] == 257 and tnet.cfg["head_dim"] == 64 and rnet.cfg["heads"] == 12
    g = torch.Generator(device="cuda").manual_seed(3)
    images = (torch.rand(4, 224, 224, 3, device="cuda", generator=g) * 255).to(torch.uint8)
    frame = torch.rand(1080, 1920, 3, device="cuda", generator=g)
    ids = torch.randint(0, TEXT["vocab"], (2, 77), device="cuda", generator=g)
    x = torch.randn(1, 257, 1280, device="cuda", generator=g)
    res = {"device": torch.cuda.get_device_name(0), "config": "ViT-H/14, SD-2.1's text encoder and ImageDream's Resampler: shapes only, random weights",
           "warmup": args.warmup, "iters": args.iters, "unit": "ms per call (median, min, max of device events)",
           "torch": "tests/clip_ref.py in float32 with F.scaled_dot_product_attention; ImageTokens' resize is the library's on both sides"}
    R.attention = sdpa_attention

    def t_vision(u8):
        return R.vision_forward(vsd, VISION, R.normalized(u8, torch.float32), torch.float32)[0]

    def t_tokens(img):
        u8 = vnet.resized(img)
        return R.resampler_forward(rsd, RESAMPLER, t_vision(u8), torch.float32)[0][0]

    gc.collect()
    gc.freeze()
    gc.disable()
    with torch.no_grad():
        for n in (1, 4):
            res[f"image_encoder_{n}"] = {"hip": timed(lambda: vnet(images[:n]), args.warmup, args.iters),
                                         "torch_f32_sdpa": timed(lambda: t_vision(images[:n]), args.warmup, args.iters)}
        res["image_encoder_1"]["distance_hip_to_torch_f32_worst_over_rms"] = distance(vnet(images[:1]), t_vision(images[:1]))
        res["resampler"] = {"hip": timed(lambda: rnet(x), args.warmup, args.iters),
                            "torch_f32_sdpa": timed(lambda: R.resampler_forward(rsd, RESAMPLER, x, torch.float32)[0], args.warmup, args.iters)}
        res["image_tokens_1080x1920"] = {"hip": timed(lambda: tokens(frame), args.warmup, args.iters),
                                         "torch_f32_sdpa": timed(lambda: t_tokens(frame), args.warmup, args.iters)}
        res["image_tokens_1080x1920"]["distance_hip_to_torch_f32_worst_over_rms"] = distance(tokens(frame)[0], t_tokens(frame))
        res["text_encoder_2x77"] = {"hip": timed(lambda: tnet(ids), args.warmup, args.iters),
                                    "torch_f32_sdpa": timed(lambda: R.text_forward(tsd, TEXT, ids, torch.float32)[0], args.warmup, args.iters)}
        res["text_encoder_2x77"]["distance_hip_to_torch_f32_worst_over_rms"] = distance(tnet(ids), R.text_forward(tsd, TEXT, ids, torch.float32)[0])
    for k, v in res.items():
        if isinstance(v, dict) and "hip" in v:
            v["hip_over_torch"] = v["hip"]["median"] / v["torch_f32_sdpa"]["median"]
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
