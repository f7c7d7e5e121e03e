"""Time the geometry model's two per-surfel passes and its one-launch Adam (soar_amd/geometry.py, csrc/geometry.hip) against the
torch composition of the same expressions (tests/geometry_ref.py, float32), at P surfels on one GPU, in one process after warm-up.

    python scripts/geometry_time.py [--points 100000] [--iters 30] [--reps 20] [--out profiles/geometry_time.json]

A timed region is ``reps`` repetitions between two device events (one call is a few microseconds of device work: a region of one
call would time the event pair); the figure is the median over ``iters`` regions divided by ``reps``, HIP and torch alternating.
Workloads: the five activations forward + backward; the five regularizers forward + backward (all weights on); one Adam step
over all groups of a model (27 tensors) against ``torch.optim.Adam(foreach=True)`` over the same groups."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import geometry_ref as R  # noqa: E402
from soar_amd import geometry as G  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps           # microseconds per call


def compare(fns, iters, reps, warmup=3):
    for fn in fns.values():
        for _ in range(warmup):
            region(fn, reps)
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():                   # alternating: both see the same neighbours on the machine
            ts[k].append(region(fn, reps))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--hip-only", action="store_true", help="run only the HIP passes (for a kernel-trace run)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    P = args.points
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    raw = [r(P, 4), r(P, 1), r(P, 1), r(P, 1), r(P, 3)]
    ups = [r(*t.shape) for t in raw]
    leaves = [t.clone().requires_grad_(True) for t in raw]

    def act(f):
        def run():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(list(f(*leaves)), ups)
        return run

    xyz, pos = r(P, 3).requires_grad_(True), r(P, 3)
    scaling, opacity, scales = torch.exp(r(P, 1)), torch.sigmoid(r(P, 1)).requires_grad_(True), (torch.sigmoid(r(P, 1)) * 2e-2).requires_grad_(True)
    lam = {k: 0.5 for k in G.LAMBDAS}

    def reg(f):
        def run():
            xyz.grad = opacity.grad = scales.grad = None
            f(xyz, pos, scaling, opacity, scales, lam)[0].backward()
        return run

    res = {"points": P, "device": torch.cuda.get_device_name(0), "reps_per_region": args.reps, "regions": args.iters, "unit": "us per call"}
    subjects = {"hip": (G.surfel_activations, G.surfel_regularizers)}
    if not args.hip_only:
        subjects["torch_fp32"] = (R.activations, R.regularizers)
    for name, k in (("activations_fwd_bwd", 0), ("regularizers_fwd_bwd", 1)):
        out = compare({s: (act if k == 0 else reg)(f[k]) for s, f in subjects.items()}, args.iters, args.reps)
        for s, (med, lo) in out.items():
            res[f"{s}_{name}_us"], res[f"{s}_{name}_min_us"] = med, lo
        if "torch_fp32" in out:
            res[f"speedup_{name}"] = out["torch_fp32"][0] / out["hip"][0]
    # the optimizer: a model of P surfels from the synthetic body, every group with a gradient
    surf = syn.make_surfels(P, 0)
    m = G.GaussianSurfelModel({})
    m.create_from_pcd(surf.xyz, surf.colors.clamp(0.02, 0.98), 10)
    m.training_setup()
    ours = [p for grp in m.optimizer.param_groups for p in grp["params"]]
    ref = [p.detach().clone().requires_grad_(True) for p in ours]
    it = iter(ref)
    tadam = torch.optim.Adam([{"params": [next(it) for _ in grp["params"]], "lr": grp["lr"]} for grp in m.optimizer.param_groups], lr=0.0,
                             eps=1e-15, foreach=True)
    for a, b in zip(ours, ref):
        a.grad = torch.randn(a.shape, device=dev) * 0.01
        b.grad = a.grad.clone()
    fns = {"hip": m.optimizer.step}
    if not args.hip_only:
        fns["torch_foreach"] = tadam.step
    out = compare(fns, args.iters, args.reps)
    res["adam_tensors"], res["adam_floats"] = len(ours), sum(p.numel() for p in ours)
    for s, (med, lo) in out.items():
        res[f"{s}_adam_step_us"], res[f"{s}_adam_step_min_us"] = med, lo
    if "torch_foreach" in out:
        res["speedup_adam_step"] = out["torch_foreach"][0] / out["hip"][0]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
