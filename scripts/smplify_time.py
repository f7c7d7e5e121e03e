"""Time the SMPL-X keypoint fitting (soar_amd/smplify.py, csrc/smplify.hip) on one GPU, in one process after warm-up.

    python scripts/smplify_time.py [--iters 20] [--reps 5] [--frames 64 256] [--out profiles/smplify_time.json]

* one closure evaluation (``smplify_objective``: the three losses and the gradient of their sum) for N frames of
  ``synthetic.make_body_model()`` (V = 10475), against the torch float32 composition of what the reference's closure does on the
  same device: the full-vertex ``lbs`` with the rotmat -> rotvec -> Rodrigues detour, through autograd (tests/smplify_ref.py);
* a whole ``SMPLify.fit`` with the reference's defaults (20 + 40 L-BFGS steps of at most 20 iterations), the same optimiser driven
  by the HIP closure and by the torch one, once each.  L-BFGS stops a step early when it has converged, so the two fits do not
  evaluate their closure equally often: the number of evaluations is given beside each time.

The synthetic body has no faces, landmarks or keypoint tables: 51 + 17 landmark triangles, 21 selected vertices and a one-to-one
table of the first 137 model points are drawn with a seed.  A timed region is ``reps`` calls between two device events; the figure
is the median over ``iters`` regions divided by ``reps``, HIP and torch alternating."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import smplify_ref as R  # noqa: E402
from soar_amd import smplify as S  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402

LOSSES = ("kp", "preserve", "smooth")


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps           # microseconds per call


def compare(fns, iters, reps, warmup=2):
    for fn in fns.values():
        for _ in range(warmup):
            region(fn, reps)
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():                   # alternating: both see the same neighbours on the machine
            ts[k].append(region(fn, reps))
    return {k: (statistics.median(v), min(v)) for k, v in ts.items()}


def make_model(dev):
    body = syn.make_body_model(0)
    g = torch.Generator().manual_seed(5)
    V = body.v_template.shape[0]
    faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(400)])
    bary = torch.rand(68, 3, generator=g) + 0.05
    m = types.SimpleNamespace(**{f: getattr(body, f).to(dev) for f in ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights")},
                              parents=body.parents, faces_tensor=faces, lmk_faces_idx=torch.randint(0, 400, (68,), generator=g),
                              lmk_bary_coords=bary / bary.sum(1, keepdim=True), extra_joints_idxs=torch.randperm(V, generator=g)[:21])
    m.vertex_joint_selector = types.SimpleNamespace(extra_joints_idxs=m.extra_joints_idxs)
    tables = (list(range(137)), list(range(137)), torch.ones(137))
    return m, tables


def make_inputs(m, tables, N, dev):
    g = torch.Generator().manual_seed(100 + N)
    seq = syn.make_pose_sequence(N, 0)
    fp = seq["full_pose"]
    true = {"global_orient": fp[:, :3], "body_pose": fp[:, 3:66], "jaw_pose": fp[:, 66:69], "leye_pose": fp[:, 69:72], "reye_pose": fp[:, 72:75],
            "left_hand_pose": fp[:, 75:120], "right_hand_pose": fp[:, 120:165], "betas": seq["betas"].expand(N, -1),
            "expression": seq["expression"], "transl": seq["transl"]}
    start = {k: (v + (0.05 if k in R.POSE_KEYS else 0.02) * torch.randn(v.shape, generator=g) if k in R.GRAD_KEYS else v.clone())
             for k, v in true.items()}
    six = lambda d: {k: (S.rotation_6d_from_rotvec(v.reshape(N, -1, 3)) if k in R.POSE_KEYS else (v[:1] if k == "betas" else v)).to(dev)
                     for k, v in d.items()}
    img_wh = (1080, 1920)
    Ks = torch.tensor([[1500.0, 0.0, 540.0], [0.0, 1500.0, 960.0], [0.0, 0.0, 1.0]]).repeat(N, 1, 1).to(dev)
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.0, 0.1, 3.5])
    w2c = w2c.to(dev)
    with torch.no_grad():
        uv = R.keypoints(m, tables, six(true), Ks, w2c)
    conf = 0.4 + 0.6 * torch.rand(N, 137, 1, generator=g)
    target = torch.cat([(uv.cpu() + 2.0 * torch.randn(N, 137, 2, generator=g)) / torch.tensor(img_wh, dtype=torch.float32), conf], -1).to(dev)
    return start, six(start), Ks, w2c, img_wh, target


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--no-fit", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    m, tables = make_model(dev)
    rig = S.KeypointRig.from_body_model(m, *tables, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "V": int(m.v_template.shape[0]), "gathered_vertices": rig.VS, "points": rig.P,
           "reps_per_region": args.reps, "regions": args.iters, "unit": "us per closure evaluation, s per fit",
           "torch": "float32 full-vertex lbs with the rotvec detour, autograd, same device (tests/smplify_ref.py)"}

    def torch_objective(_rig, params, init, Ks, w2c, img_wh, tk, scales, weights=(100.0, 60.0, 10000.0), sigma=100.0, ignore_hands=False):
        ls, gr = R.objective(m, tables, params, init, Ks, w2c, img_wh, tk, scales, dtype=torch.float32, device=dev, weights=weights, sigma=sigma,
                             ignore_hands=ignore_hands, detour=True)
        return types.SimpleNamespace(losses=torch.stack([ls[k] for k in LOSSES]), grads=gr)

    for N in args.frames:
        start, p6, Ks, w2c, img_wh, target = make_inputs(m, tables, N, dev)
        scales = S.target_scales(target, img_wh)
        a, b = S.smplify_objective(rig, p6, p6, Ks, w2c, img_wh, target, scales), torch_objective(rig, p6, p6, Ks, w2c, img_wh, target, scales)
        res[f"closure_N{N}_loss_hip"], res[f"closure_N{N}_loss_torch"] = float(a.losses.sum()), float(b.losses.sum())
        out = compare({"hip": lambda: S.smplify_objective(rig, p6, p6, Ks, w2c, img_wh, target, scales),
                       "torch_fp32": lambda: torch_objective(rig, p6, p6, Ks, w2c, img_wh, target, scales)}, args.iters, args.reps)
        for s, (med, lo) in out.items():
            res[f"{s}_closure_N{N}_us"], res[f"{s}_closure_N{N}_min_us"] = med, lo
        res[f"speedup_closure_N{N}"] = out["torch_fp32"][0] / out["hip"][0]
        if args.no_fit:
            continue
        for name, fit in (("hip", S.SMPLify(rig)), ("torch_fp32", S.SMPLify(rig, objective=torch_objective))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fit.fit(start, Ks, w2c, img_wh, target)
            torch.cuda.synchronize()
            res[f"{name}_fit_N{N}_s"], res[f"{name}_fit_N{N}_evaluations"] = time.perf_counter() - t0, fit.evaluations
            res[f"{name}_fit_N{N}_final_losses"] = fit.loss_dict
        res[f"speedup_fit_N{N}"] = res[f"torch_fp32_fit_N{N}_s"] / res[f"hip_fit_N{N}_s"]
        print(json.dumps({k: v for k, v in res.items() if f"N{N}" in k}), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
