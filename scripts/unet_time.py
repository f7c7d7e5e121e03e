"""Time the multi-view diffusion UNet (soar_amd/unet.py, csrc/unet.hip, csrc/attention.hip) at the shipped model's shapes with seeded
random weights (no checkpoint needed): N = 8 latents of 32 x 32 (text and unconditional halves of 4 views), 77 text and 16 image
tokens, against the same network composed from torch-float32 operations (tests/unet_ref.py) on the same GPU -> profiles/unet_time.json.

Reported: one ``forward``, and the attention kernel alone at level 0 (2 groups x 4096 tokens, 5 heads of 64).  The torch side's
attention is ``F.scaled_dot_product_attention`` and, as a second figure, the restatement's explicit product.  Medians of device-event
times with the fastest and slowest call beside them.  FLOPs are derived from the layer sizes (2 per multiply-add) and set against the
157.3 TFLOP/s f32 MFMA peak.
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

import unet_ref as R  # noqa: E402
from soar_amd import unet  # noqa: E402

PEAK = 157.3e12
SHIPPED = dict(in_channels=4, out_channels=4, model_channels=320, channel_mult=(1, 2, 4, 4), num_res_blocks=2, attention=(True, True, True, False),
               context_dim=1024, camera_dim=16, with_ip=True, num_head_channels=64, ip_dim=16, ip_weight=1.0, n_view=4, N=8, h=32, w=32, T=77)


def device_weights(cfg, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for key, shape in R.state_dict_shapes(cfg).items():
        t = torch.randn(shape, generator=g, device="cuda")
        sd[key] = ((1.0 if key.endswith("weight") else 0.0) + 0.1 * t) if len(shape) == 1 else t / float(np.prod(shape[1:])) ** 0.5
    return sd


def forward_flops(cfg):
    """multiply-adds x 2 of the convolutions, linear layers and attention products of one forward"""
    N, hw0, ctx, E = cfg["N"], cfg["h"] * cfg["w"], cfg["context_dim"], 4 * cfg["model_channels"]
    Tk = cfg["T"] + cfg["ip_dim"]
    ins, mid_ch, outs = R.layout(cfg)
    f = 0.0

    def res(cin, cout, rows):
        return 2.0 * rows * 9 * (cin * cout + cout * cout) + 2.0 * N * E * cout + (2.0 * rows * cin * cout if cin != cout else 0.0)

    def tr(C, rows):
        L = cfg["n_view"] * rows // N
        return 2.0 * rows * C * C * (2 + 4 + 2 + 12) + 2.0 * N * Tk * ctx * 2 * C + 4.0 * (N // cfg["n_view"]) * L * L * C + 4.0 * rows * Tk * C

    for b in ins + outs:
        rows = N * hw0 >> (2 * b["level"])
        if b["kind"] == "conv":
            f += 2.0 * rows * 9 * b["cin"] * b["cout"]
        elif b["kind"] == "down":
            f += 2.0 * (rows // 4) * 9 * b["cin"] * b["cout"]
        else:
            f += res(b["cin"], b["cout"], rows) + (tr(b["cout"], rows) if b["attn"] else 0.0)
            if b.get("up"):
                f += 2.0 * 4 * rows * 9 * b["cout"] * b["cout"]
    rows = N * hw0 >> (2 * (len(cfg["channel_mult"]) - 1))
    f += 2 * res(mid_ch, mid_ch, rows) + tr(mid_ch, rows)
    return f + 2.0 * N * hw0 * 9 * cfg["model_channels"] * cfg["out_channels"]


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


def sdpa_attention(q, k, v, heads, scale=None):
    B, Lq, C = q.shape
    sp = lambda t: t.reshape(B, -1, heads, C // heads).transpose(1, 2)
    return F.scaled_dot_product_attention(sp(q), sp(k), sp(v), scale=scale).transpose(1, 2).reshape(B, Lq, C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_time.json"))
    args = ap.parse_args()
    cfg = SHIPPED
    sd = device_weights(cfg)
    net = unet.MultiviewUNet(sd, num_head_channels=64, ip_dim=16, n_view=4).to("cuda")
    assert all(net.cfg[k] == cfg[k] for k in net.cfg), "the sizes read from the state dict are not the shipped model's"
    x, t, ctx, cam, ip = (v.cuda() for v in R.inputs(cfg, 0))
    t = t[::4].repeat_interleave(4)
    gflop = forward_flops(cfg) / 1e9
    res = {"device": torch.cuda.get_device_name(0), "config": "sd-v2.1-base-4view-ipmv shapes, random weights", "N": cfg["N"], "latents": [cfg["h"], cfg["w"]],
           "context_tokens": [cfg["T"], cfg["ip_dim"]], "warmup": args.warmup, "iters": args.iters, "unit": "ms per call (median, min, max of device events)",
           "f32_mfma_peak_tflops": PEAK / 1e12, "forward_gflop": gflop}
    gc.collect()
    gc.freeze()
    gc.disable()
    explicit = R.attention
    with torch.no_grad():
        res["hip_forward"] = timed(lambda: net(x, t, ctx, camera=cam, ip_tokens=ip), args.warmup, args.iters)
        res["hip_forward_tflops"] = gflop / res["hip_forward"]["median"]
        eps = net(x, t, ctx, camera=cam, ip_tokens=ip)
        for name, fn in (("sdpa", sdpa_attention), ("explicit", explicit)):
            R.attention = fn
            res[f"torch_f32_forward_{name}"] = timed(lambda: R.forward(sd, cfg, x, t, ctx, cam, ip, dtype=torch.float32)[0], 1, max(3, args.iters // 2))
        R.attention = explicit
        t_eps = R.forward(sd, cfg, x, t, ctx, cam, ip, dtype=torch.float32)[0]
        best = min(res["torch_f32_forward_sdpa"]["median"], res["torch_f32_forward_explicit"]["median"])
        res["torch_f32_forward_tflops"] = gflop / best
        res["hip_over_torch_forward"] = res["hip_forward"]["median"] / best
        res["distance_hip_to_torch_f32_worst_over_rms"] = ((eps - t_eps).abs().max() / t_eps.pow(2).mean().sqrt()).item()
        del t_eps
        torch.cuda.empty_cache()
        # the attention kernel alone at level 0: q | k | v as the slices of one product
        B, L, heads, hd = cfg["N"] // cfg["n_view"], cfg["n_view"] * cfg["h"] * cfg["w"], cfg["model_channels"] // 64, 64
        qkv = torch.randn(B, L, 3 * heads * hd, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        q, k, v = qkv.chunk(3, dim=-1)
        a_gflop = 4.0 * B * heads * hd * L * L / 1e9
        res["attention_level0"] = {"B": B, "L": L, "heads": heads, "hd": hd, "gflop": a_gflop,
                                   "hip": timed(lambda: unet.attention(q, k, v, heads), args.warmup, args.iters),
                                   "torch_f32_sdpa": timed(lambda: sdpa_attention(q, k, v, heads), args.warmup, args.iters),
                                   "torch_f32_explicit": timed(lambda: explicit(q, k, v, heads), args.warmup, args.iters)}
        a = res["attention_level0"]
        a["hip_tflops"] = a_gflop / a["hip"]["median"]
        a["hip_over_torch"] = a["hip"]["median"] / min(a["torch_f32_sdpa"]["median"], a["torch_f32_explicit"]["median"])
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
