"""Time the avatar initialisation (soar_amd/body.py, csrc/body.hip) on one GPU, in one process after warm-up.

    python scripts/body_time.py [--iters 30] [--reps 10] [--out profiles/body_time.json]

* ``soar_smplx_vertices`` (with the joint-chain launch in front of it, as ``body.smplx_vertices`` runs it) at V = 10475 for
  B in {1, 4, 64, 512}, against the torch float32 composition of the same formula on the same device (tests/body_ref.py).
* Two levels of subdivision plus vertex normals and frames on a 10 242-vertex closed mesh, against nothing: there is no other path.

A timed region is ``reps`` calls between two device events; the figure is the median over ``iters`` regions divided by ``reps``,
HIP and torch alternating.  All figures are WARM: the same 61 MB of posedirs are read again by every call and fit the 256 MiB
Infinity Cache, so the B = 1 figure is not an HBM-streaming time (the byte floor is stated beside it for scale)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import body_ref as R  # noqa: E402
from soar_amd import body as B  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402

HBM_BYTES_PER_S = 6.3e12       # achievable float4-copy rate of the device


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
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    body = syn.make_body_model(0)
    dbody = type(body)(*[getattr(body, f).to(dev) for f in ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")])
    g = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "V": int(body.v_template.shape[0]), "reps_per_region": args.reps, "regions": args.iters,
           "unit": "us per call", "regime": "warm (repeated calls on the same arrays; posedirs fits the Infinity Cache)",
           "posedirs_bytes": int(body.posedirs.numel() * 4),
           "posedirs_hbm_floor_us": body.posedirs.numel() * 4 / HBM_BYTES_PER_S * 1e6}
    for nb in (1, 4, 64, 512):
        pose = (torch.randn(nb, 165, generator=g) * 0.4).to(dev)
        betas = (torch.randn(nb, 20, generator=g) * 0.7).to(dev)
        transl = torch.randn(nb, 3, generator=g).to(dev)
        out = compare({"hip": lambda: B.smplx_vertices(dbody, betas, pose, transl),
                       "torch_fp32": lambda: R.lbs_vertices(dbody, betas, pose, transl, torch.float32, dev)}, args.iters, args.reps)
        for s, (med, lo) in out.items():
            res[f"{s}_vertices_B{nb}_us"], res[f"{s}_vertices_B{nb}_min_us"] = med, lo
        res[f"speedup_vertices_B{nb}"] = out["torch_fp32"][0] / out["hip"][0]
    v, f = R.icosphere(5)
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    rd = torch.randn(tv.shape[0] + 30720 + 122880, 3, generator=g).to(dev)

    def init():
        sv, sf = B.subdivide(tv, tf, levels=2)
        return B.surfel_frames(B.vertex_normals(sv, sf), rd)

    assert init().shape[0] == rd.shape[0]
    out = compare({"hip": init}, args.iters, args.reps)
    res["mesh_vertices_in"], res["mesh_points_out"] = int(tv.shape[0]), int(rd.shape[0])
    res["hip_subdivide2_normals_frames_us"], res["hip_subdivide2_normals_frames_min_us"] = out["hip"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
