"""Time the environment-map background (soar_amd/background.py) against the float32 torch restatement (tests/envmap_ref.py:
the SH basis as torch ops, three F.linear layers, sigmoid, and the renderer's composite), on one GPU, in one process after
warm-up, with device events.

    python scripts/background_time.py [--iters 50] [--out profiles/background_time.json] [--hip-only]

Shapes: the configuration's (B = 5 rows of 512 x 512: 4 SDS views and the video frame's row, 4 composited) and a larger one
(B = 5 at 1024 x 1024).  Two workloads each: the forward (background and composite) and the forward plus the backward with
upstream gradients on the composite and on the last row (comp_bg), as the SDS step gives them."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import envmap_ref as R  # noqa: E402
from soar_amd.background import NeuralEnvironmentMapBackground  # noqa: E402


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="time only the HIP module (for a kernel-trace run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    env = NeuralEnvironmentMapBackground({"random_aug": False}).to(dev)
    ref = R.RefBackground(env).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters}
    for B, NC, H, W in ((5, 4, 512, 512), (5, 4, 1024, 1024)):
        g = torch.Generator().manual_seed(1)
        dirs = torch.nn.functional.normalize(torch.randn(B, H, W, 3, generator=g), dim=-1).to(dev)
        renders = torch.rand(NC, 3, H, W, generator=g).to(dev).requires_grad_(True)
        masks = torch.rand(NC, 1, H, W, generator=g).to(dev).requires_grad_(True)
        G = torch.randn(NC, H, W, 3, generator=g).to(dev)
        Gb = torch.randn(1, H, W, 3, generator=g).to(dev)

        def hip(backward):
            def run():
                env.zero_grad(set_to_none=True)
                with torch.set_grad_enabled(backward):
                    comp, bg = env.composite(dirs, renders, masks, NC)
                    if backward:
                        torch.autograd.backward([comp, bg[[-1]]], [G, Gb])
            return run

        def torch_form(backward):
            def run():
                ref.zero_grad(set_to_none=True)
                with torch.set_grad_enabled(backward):
                    bg = ref(dirs)
                    comp = (renders + (1 - masks) * bg[:NC].permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
                    if backward:
                        torch.autograd.backward([comp, bg[[-1]]], [G, Gb])
            return run

        key = f"B{B}_{H}x{W}"
        subjects = (("hip", hip),) if args.hip_only else (("hip", hip), ("torch_fp32", torch_form))
        for name, make in subjects:
            res[f"{name}_{key}_forward_ms"], res[f"{name}_{key}_forward_min_ms"] = timed(make(False), args.iters)
            res[f"{name}_{key}_fwd_bwd_ms"], res[f"{name}_{key}_fwd_bwd_min_ms"] = timed(make(True), args.iters)
        if not args.hip_only:
            res[f"speedup_{key}_forward"] = res[f"torch_fp32_{key}_forward_ms"] / res[f"hip_{key}_forward_ms"]
            res[f"speedup_{key}_fwd_bwd"] = res[f"torch_fp32_{key}_fwd_bwd_ms"] / res[f"hip_{key}_fwd_bwd_ms"]
        print(json.dumps({k: v for k, v in res.items() if key in k}), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
