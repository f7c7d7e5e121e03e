"""Time the attribute field (soar_amd/field.py) against the float32 torch restatement of nerfstudio's fallback
(tests/field_ref.py: all levels at once, eight gathers by advanced indexing, F.linear heads), at P surfels with the default
configuration, on one GPU, in one process after warm-up, with device events.

    python scripts/field_time.py [--points 100000] [--iters 50] [--out profiles/field_time.json]

Two workloads each: the forward; the forward plus the backward with the renderer's upstream gradients (shs, scales, offsets:
TS/renderer/diff_gaussian_rasterizer.py:225-243), which reach the `encoding` table and three heads.  Both for the surfels in
the generator's random order and in Morton order (synthetic.sort_surfels_spatially: a model initialised from the SMPL-X
vertices is in such an order), since the scatter's in-wave combining depends on it.  With SOAR_HIP_LIB set to a variant
(scripts/variant.py) the HIP numbers are that variant's."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import field_ref as R  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402
from soar_amd.field import HashMLPField  # noqa: E402


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
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="time only the HIP field (for a kernel-trace run)")
    ap.add_argument("--order", choices=("random", "spatial", "both"), default="both")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    surf = syn.make_surfels(args.points, 0)
    aabb = torch.stack([surf.xyz.min(0)[0], surf.xyz.max(0)[0]])
    c = aabb.mean(0)
    aabb = (aabb - c) * 1.5 + c
    torch.manual_seed(0)
    field = HashMLPField(aabb).to(dev)
    ref = R.RefField(field).to(dev)
    orders = {"random": surf.xyz, "spatial": syn.sort_surfels_spatially(surf).xyz}
    g = torch.Generator().manual_seed(1)
    up = {h: torch.randn(args.points, o, generator=g).to(dev) for h, o in (("shs", 3), ("scales", 1), ("offsets", 3))}

    def fwd(f, xyz):
        def run():
            with torch.no_grad():
                f(xyz)
        return run

    def fwd_bwd(f, xyz):
        def run():
            f.zero_grad(set_to_none=True)
            out = f(xyz)
            torch.autograd.backward([out[h] for h in up], [up[h] for h in up])
        return run

    res = {"points": args.points, "device": torch.cuda.get_device_name(0), "library": os.environ.get("SOAR_HIP_LIB", "in-tree")}
    subjects = (("hip", field),) if args.hip_only else (("hip", field), ("torch_fp32", ref))
    for order in (("random", "spatial") if args.order == "both" else (args.order,)):
        xyz = orders[order].to(dev).contiguous()
        for name, f in subjects:
            res[f"{name}_{order}_forward_ms"], res[f"{name}_{order}_forward_min_ms"] = timed(fwd(f, xyz), args.iters)
            res[f"{name}_{order}_fwd_bwd_ms"], res[f"{name}_{order}_fwd_bwd_min_ms"] = timed(fwd_bwd(f, xyz), args.iters)
        if not args.hip_only:
            res[f"speedup_{order}_forward"] = res[f"torch_fp32_{order}_forward_ms"] / res[f"hip_{order}_forward_ms"]
            res[f"speedup_{order}_fwd_bwd"] = res[f"torch_fp32_{order}_fwd_bwd_ms"] / res[f"hip_{order}_fwd_bwd_ms"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
