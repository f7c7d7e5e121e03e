"""Time the multi-view diffusion UNet with 16-bit matrix products (soar_amd/unet.py ``precision``) at the shipped
model's shapes of scripts/unet_time.py with seeded random weights -> profiles/unet_half_time.json.

Reported, all in one process:
  * one ``forward`` at f32, bf16 and f16, the three alternating call by call;
  * the same network composed from torch operations (tests/unet_ref.py with ``F.scaled_dot_product_attention``) in float32, after
    ``.to(torch.bfloat16)`` and after ``.half()``;
  * the shared GEMM alone (soar_selftest_conv_gemm / _conv_gemm16) at the four largest products of the model, at the three operand
    types: TFLOP/s and the fraction of the 2.5 PFLOP/s 16-bit matrix peak (157.3 TFLOP/s for float32 operands).
Medians of device-event times with the fastest and slowest call beside them.

``--root TREE`` imports ``soar_amd`` from another checkout (built there) and times what that tree has: with a tree from before the
``precision`` argument, its float32 ``forward`` alone -- the yardstick.  ``--parent FILE...`` copies such runs' results into the
output as ``parent_f32_forward``.
"""
import argparse
import ctypes as C
import gc
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--root", default=ROOT, help="the checkout whose soar_amd is timed")
    ap.add_argument("--parent", nargs="*", default=[], help="results of --root runs over the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unet_half_time.json"))
    return ap.parse_args()


ARGS = _args()
sys.path[:0] = [os.path.abspath(ARGS.root), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402

import conv_gemm_ref as G  # noqa: E402
import unet_ref as R  # noqa: E402
from soar_amd import hip_lib, unet  # noqa: E402
from unet_time import SHIPPED, device_weights, forward_flops, sdpa_attention  # noqa: E402

PEAK16, PEAK32 = 2.5e15, 157.3e12
TYPES = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}


def stats(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def once(fn, reps=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def alternating(fns, warmup, iters, reps=1):
    """{name: fn} -> {name: stats}: every round times each fn once, so a drift of the machine falls on all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ts[k].append(once(fn, reps))
    return {k: stats(v) for k, v in ts.items()}


def gemm_alone(name, d, warmup, iters):
    """the descriptor over unguarded random buffers at the three operand types"""
    lib = hip_lib.lib()
    g = torch.Generator(device="cuda").manual_seed(3)
    d.ldx, d.xim, d.ldy, d.yim = d.Cin, d.Hin * d.Win, d.Cout, d.Hout * d.Wout
    K = d.ph[0].ntaps * d.Cin
    d.ph[0].ldw = K
    x = torch.randn(d.N * d.xim * d.ldx, device="cuda", generator=g)
    w = torch.randn(d.Cout * K, device="cuda", generator=g) / K ** 0.5
    bias = torch.randn(d.Cout, device="cuda", generator=g)
    y = torch.empty(d.N * d.yim * d.ldy, device="cuda")
    ws = {"f32": w, "bf16": w.to(torch.bfloat16), "f16": w.to(torch.float16)}
    tile = C.c_int32(0)
    stream = torch.cuda.current_stream().cuda_stream
    fns = {}
    for p, (wtype, _) in TYPES.items():
        a = G.c_args(d, x.data_ptr(), ws[p].data_ptr(), bias.data_ptr(), None, y.data_ptr())
        if wtype:
            fns[p] = lambda a=a, wtype=wtype: hip_lib.check(lib.soar_selftest_conv_gemm16(C.byref(a), wtype, C.byref(tile), stream), "conv_gemm16")
        else:
            fns[p] = lambda a=a: hip_lib.check(lib.soar_selftest_conv_gemm(C.byref(a), C.byref(tile), stream), "conv_gemm")
    M = d.N * d.Hg * d.Wg
    gflop = 2.0 * M * K * d.Cout / 1e9
    out = {"name": name, "M": M, "K": K, "Cout": d.Cout, "gflop": gflop, "ms": alternating(fns, warmup, iters, reps=10)}
    fns["f32"]()
    out["tile"] = tile.value
    for p in TYPES:
        tf = gflop / out["ms"][p]["median"]
        out[p + "_tflops"] = tf
        out[p + "_fraction_of_peak"] = tf * 1e12 / (PEAK32 if p == "f32" else PEAK16)
    return out


def main():
    args = ARGS
    cfg = SHIPPED
    has_precision = "precision" in inspect.signature(unet.MultiviewUNet.__init__).parameters
    sd = device_weights(cfg)
    kw = dict(num_head_channels=64, ip_dim=16, n_view=4)
    nets = {"f32": unet.MultiviewUNet(sd, **kw).to("cuda")}
    if has_precision:
        for p in ("bf16", "f16"):
            nets[p] = unet.MultiviewUNet(sd, precision=p, **kw).to("cuda")
    x, t, ctx, cam, ip = (v.cuda() for v in R.inputs(cfg, 0))
    t = t[::4].repeat_interleave(4)
    gflop = forward_flops(cfg) / 1e9
    res = {"device": torch.cuda.get_device_name(0), "config": "sd-v2.1-base-4view-ipmv shapes, random weights", "N": cfg["N"],
           "latents": [cfg["h"], cfg["w"]], "context_tokens": [cfg["T"], cfg["ip_dim"]], "warmup": args.warmup, "iters": args.iters,
           "unit": "ms per call (median, min, max of device events)", "forward_gflop": gflop, "peak_16bit_tflops": PEAK16 / 1e12,
           "peak_f32_tflops": PEAK32 / 1e12, "tree": "this" if os.path.abspath(args.root) == ROOT else "--root"}
    gc.collect()
    gc.freeze()
    gc.disable()
    with torch.no_grad():
        fwd = alternating({p: (lambda n=n: n(x, t, ctx, camera=cam, ip_tokens=ip)) for p, n in nets.items()}, args.warmup, args.iters)
        res["hip_forward"] = fwd
        res["hip_forward_tflops"] = {p: gflop / v["median"] for p, v in fwd.items()}
        if not has_precision:
            print(json.dumps(res), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            json.dump(res, open(args.out, "w"), indent=1)
            return
        res["hip_16bit_over_f32_forward"] = {p: fwd[p]["median"] / fwd["f32"]["median"] for p in ("bf16", "f16")}
        eps = {p: n(x, t, ctx, camera=cam, ip_tokens=ip) for p, n in nets.items()}
        rms = eps["f32"].pow(2).mean().sqrt()
        res["distance_to_hip_f32_worst_over_rms"] = {p: ((eps[p] - eps["f32"]).abs().max() / rms).item() for p in ("bf16", "f16")}
        del eps
        torch.cuda.empty_cache()
        # torch: the same composition, its tensors converted
        explicit = R.attention
        R.attention = sdpa_attention
        try:
            tor = {}
            for p, (_, dt) in TYPES.items():
                sdp = {k: v.to(dt) for k, v in sd.items()}
                tor[p] = stats([once(lambda: R.forward(sdp, cfg, x, t, ctx, cam, ip, dtype=dt)[0]) for _ in range(2 + max(5, args.iters // 2))][2:])
                del sdp
                torch.cuda.empty_cache()
        finally:
            R.attention = explicit
        res["torch_forward_sdpa"] = tor
        res["hip_over_torch_forward"] = {p: fwd[p]["median"] / tor[p]["median"] for p in TYPES}
        # the GEMM alone: the four largest products (3 x 3 convolutions of an output block at levels 0 and 1, a ResBlock's at level
        # 0, GEGLU's projection at level 0)
        N, h, w, mc = cfg["N"], cfg["h"], cfg["w"], cfg["model_channels"]
        res["gemm_alone"] = [
            gemm_alone("conv3x3 640 -> 320 at 32 x 32", G.conv3x3(N, h, w, 2 * mc, mc), args.warmup, args.iters),
            gemm_alone("conv3x3 1280 -> 640 at 16 x 16", G.conv3x3(N, h // 2, w // 2, 4 * mc, 2 * mc), args.warmup, args.iters),
            gemm_alone("conv3x3 320 -> 320 at 32 x 32", G.conv3x3(N, h, w, mc, mc), args.warmup, args.iters),
            gemm_alone("linear 320 -> 2560 over 8192 tokens", G.conv1x1(1, 1, N * h * w, mc, 8 * mc), args.warmup, args.iters),
        ]
    for f in args.parent:
        res.setdefault("parent_f32_forward", []).append(json.load(open(f))["hip_forward"]["f32"])
    if "parent_f32_forward" in res:
        best = min(v["median"] for v in res["parent_f32_forward"])
        res["hip_over_parent_f32_forward"] = {p: fwd[p]["median"] / best for p in TYPES}
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
