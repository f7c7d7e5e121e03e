"""Time SAM (soar_amd/sam.py, csrc/sam.hip) at ViT-H's shapes with seeded random weights (no checkpoint needed) on 1080 x 1920
frames, batches of 1 and 4, against the same network composed from torch-float32 operations (tests/sam_ref.py) on the same GPU
-> profiles/sam_time.json.

Stages: ``embed`` (resize, normalisation, image encoder), ``decode`` (prompt encoder, mask decoder; 25 points a frame) and the whole
``masks.segment_sequence`` chunk (upload, embed, decode, post-processing, clean-up).  The torch side's attention is
``F.scaled_dot_product_attention`` with the relative-position bias as its additive mask, and, as a second figure, the explicit product;
its ``embed`` starts from the pre-processed image (the resize is not part of it), and its ``decode`` and post-processing are the
restatement's one-frame functions in a Python loop over the frames: an unbatched baseline.  The encoder is also reported in TFLOP/s against the
157.3 TFLOP/s f32 MFMA peak; its FLOPs are derived from the layer sizes (2 per multiply-add, padded windows counted as computed).
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

import sam_ref as R  # noqa: E402
from soar_amd import masks, sam  # noqa: E402

PEAK = 157.3e12
VIT_H = dict(image_size=1024, patch=16, embed=1280, depth=32, heads=16, window=14, global_blocks=(7, 15, 23, 31), mlp=5120, out_chans=256,
             dec_layers=2, dec_heads=8, dec_down=2, dec_mlp=2048, mask_tokens=4, hyper_depth=3, iou_depth=3, iou_hidden=256)
H, W, POINTS = 1080, 1920, 25


def device_weights(cfg, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for key, shape in R.state_dict_shapes(cfg).items():
        t = torch.randn(shape, generator=g, device="cuda")
        if key.endswith(".bias") or "rel_pos" in key or key.endswith("pos_embed"):
            t = 0.1 * t
        elif len(shape) == 1:
            t = 1.0 + 0.1 * t
        elif len(shape) >= 2 and "gaussian" not in key and shape[0] > 1 and "tokens" not in key:
            t = t / (float(np.prod(shape[1:])) if "upscaling" not in key else float(shape[0])) ** 0.5
        sd[key] = t
    return sd


def encoder_flops(cfg, B):
    g, C, P, hd = R.grid_of(cfg), cfg["embed"], cfg["out_chans"], cfg["embed"] // cfg["heads"]
    M = B * g * g
    f = 2.0 * M * 3 * cfg["patch"] ** 2 * C
    for i in range(cfg["depth"]):
        f += 2.0 * M * C * (4 * C + 2 * cfg["mlp"])
        if i in cfg["global_blocks"]:
            f += 4.0 * B * cfg["heads"] * hd * (g * g) ** 2
        else:
            nw = -(-g // cfg["window"]) ** 2
            f += 4.0 * B * nw * cfg["heads"] * hd * cfg["window"] ** 4
    return f + 2.0 * M * (C * P + 9 * P * P)


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
    return sorted(ts)[len(ts) // 2]


def sdpa_rel_attention(q, k, v, rel_h, rel_w, Sh, Sw, scale):
    """tests/sam_ref.py rel_attention with the bias as scaled_dot_product_attention's additive mask"""
    ih = torch.arange(Sh)[:, None] - torch.arange(Sh)[None, :] + Sh - 1
    iw = torch.arange(Sw)[:, None] - torch.arange(Sw)[None, :] + Sw - 1
    r = q.reshape(q.shape[0], q.shape[1], Sh, Sw, -1)
    bh = torch.einsum("nahwc,hkc->nahwk", r, rel_h[ih])
    bw = torch.einsum("nahwc,wkc->nahwk", r, rel_w[iw])
    bias = (bh[..., :, None] + bw[..., None, :]).reshape(q.shape[0], q.shape[1], Sh * Sw, Sh * Sw)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=scale)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_time.json"))
    args = ap.parse_args()
    cfg = VIT_H
    sd = device_weights(cfg)
    seg = sam.SamSegmenter(sd).to("cuda")
    assert {k: v for k, v in seg.cfg.items()} == cfg, "the sizes read from the state dict are not ViT-H's"
    res = {"device": torch.cuda.get_device_name(0), "config": "ViT-H shapes, random weights", "frame": [H, W], "points": POINTS, "warmup": args.warmup,
           "iters": args.iters, "unit": "ms per call (median)", "f32_mfma_peak_tflops": PEAK / 1e12, "batches": {}}
    gc.collect()
    gc.freeze()
    gc.disable()
    rng = np.random.default_rng(0)
    explicit = R.rel_attention
    for B in (1, 4):
        frames = [R.synthetic_frame(H, W, i) for i in range(B)]
        images = torch.from_numpy(np.stack(frames)).cuda()
        pts = torch.from_numpy(rng.uniform([0.3 * W, 0.1 * H], [0.7 * W, 0.9 * H], (B, POINTS, 2)).astype(np.float32)).cuda()
        kp = np.concatenate([pts.cpu().numpy(), np.ones((B, POINTS, 1), np.float32)], -1)
        row = {"encoder_gflop": encoder_flops(cfg, B) / 1e9}
        with torch.no_grad():
            row["hip_embed"] = timed(lambda: seg.embed(images), args.warmup, args.iters)
            patches, _ = seg.patches(images)
            row["hip_encoder_only"] = timed(lambda: seg.encode(patches=patches), args.warmup, args.iters)
            row["hip_encoder_tflops"] = encoder_flops(cfg, B) / (row["hip_encoder_only"] * 1e-3) / 1e12
            row["hip_encoder_peak_share"] = row["hip_encoder_tflops"] * 1e12 / PEAK
            emb = seg.embed(images)
            row["hip_decode"] = timed(lambda: seg.decode(emb, pts, None, (H, W)), args.warmup, args.iters)
            low, _ = seg.decode(emb, pts, None, (H, W))
            row["hip_postprocess"] = timed(lambda: seg.postprocess(low, (H, W)), args.warmup, args.iters)
            row["hip_segment_sequence_chunk"] = timed(lambda: masks.segment_sequence(seg, frames, kp, chunk=B), args.warmup, args.iters)

            x = seg.preprocessed(images)
            new_hw = R.resized_hw(H, W, cfg["image_size"])
            for name, fn in (("sdpa", sdpa_rel_attention), ("explicit", explicit)):
                R.rel_attention = fn
                row[f"torch_f32_encoder_{name}"] = timed(lambda: R.encode(sd, cfg, x), 1, max(3, args.iters // 2))
            row["torch_f32_encoder_tflops"] = encoder_flops(cfg, B) / (min(row["torch_f32_encoder_sdpa"], row["torch_f32_encoder_explicit"]) * 1e-3) / 1e12
            R.rel_attention = sdpa_rel_attention
            t_emb = R.encode(sd, cfg, x)
            R.rel_attention = explicit

            def torch_decode():
                out = []
                for b in range(B):
                    sparse = R.prompt_tokens(sd, cfg, pts[b], [1] * POINTS, (H, W), new_hw)
                    out.append(R.decode(sd, cfg, t_emb[b], sparse)[0])
                return torch.stack(out)
            row["torch_f32_decode"] = timed(torch_decode, args.warmup, args.iters)
            t_low = torch_decode()
            row["torch_f32_postprocess"] = timed(lambda: [R.postprocess(t_low[b], cfg, new_hw, (H, W)) for b in range(B)], args.warmup, args.iters)
            rms = lambda t: t.pow(2).mean().sqrt().item()
            row["distance_hip_to_torch_f32"] = {"embedding_worst_over_rms": ((emb - t_emb).abs().max() / rms(t_emb)).item(),
                                                "low_res_worst_over_rms": ((low - t_low).abs().max() / rms(t_low)).item()}
        res["batches"][str(B)] = row
        print(B, json.dumps(row), flush=True)
        del x, t_emb, emb, patches
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
