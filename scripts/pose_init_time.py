"""Time the initialisation from keypoints (soar_amd/pose_init.py, csrc/pose_init.hip) on one GPU, in one process after warm-up.

    python scripts/pose_init_time.py [--runs 9] [--frames 256] [--parent-lib PATH] [--out profiles/pose_init_time.json]

* ``search`` and ``viterbi_path`` for N frames and S = 2 base poses x 24 yaws x 3 pitches = 144 states on the 10 475-vertex
  synthetic body of ``scripts/smplify_time.py`` (137 one-to-one mapped points), each against the NumPy / torch float64 restatement
  of tests/pose_init_ref.py on the host, and the whole ``init_from_keypoints``.  A HIP figure is a region of ``reps`` calls
  between two device events divided by ``reps``; ``init_from_keypoints`` and the host restatements are wall-clock around one call
  that ends in a synchronise.  Every figure is the median of ``runs`` (at least 7) with the smallest and the largest beside it.
* ``--parent-lib``: the existing objective's closure (``scripts/smplify_time.py``'s, N = 64 and 256) with this tree's library and
  with another build of it (the parent commit's) loaded as a second library and driven through the same Python call, the two
  alternating in this process: csrc/smplify.hip gained a kernel, and the kernels it had must not have moved.

The scene: frame n shows base pose (n // 64) % 2 at yaw index (n // 8) % 24 of the middle pitch, 2 px of noise on the targets."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import pose_init_ref as PR  # noqa: E402
import smplify_time as ST  # noqa: E402
from soar_amd import hip_lib  # noqa: E402
from soar_amd import pose_init as PI  # noqa: E402
from soar_amd import smplify as S  # noqa: E402


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": len(v)}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


class Swap:
    """The library handle with the named entry points taken from another build."""

    def __init__(self, base, other, names):
        self.base, self.other, self.names = base, other, names

    def __getattr__(self, n):
        return getattr(self.other if n in self.names else self.base, n)


def closure_ab(parent_path, runs, res):
    dev = torch.device("cuda:0")
    m, tables = ST.make_model(dev)
    rig = S.KeypointRig.from_body_model(m, *tables, device=dev)
    base = hip_lib.lib()
    other = C.CDLL(os.path.abspath(parent_path))
    for name in ("soar_smplify_objective", "soar_last_error"):
        getattr(other, name).restype, getattr(other, name).argtypes = hip_lib.SIGNATURES[name]
    swapped = Swap(base, other, {"soar_smplify_objective"})
    for N in (64, 256):
        start, p6, Ks, w2c, img_wh, target = ST.make_inputs(m, tables, N, dev)
        scales = S.target_scales(target, img_wh)
        call = lambda: S.smplify_objective(rig, p6, p6, Ks, w2c, img_wh, target, scales)
        a = call()
        hip_lib._lib = swapped
        b = call()
        hip_lib._lib = base
        res[f"closure_N{N}_same_bits"] = bool(torch.equal(a.losses, b.losses) and all(torch.equal(a.grads[k], b.grads[k]) for k in a.grads))
        ts = {"this": [], "parent": []}
        for r in range(runs + 1):
            for name in (("this", "parent") if r % 2 == 0 else ("parent", "this")):           # alternating order
                hip_lib._lib = swapped if name == "parent" else base
                regions = [ST.region(call, 5) for _ in range(20)]
                if r:                                                                           # run 0 warms up
                    ts[name].append(statistics.median(regions))
            hip_lib._lib = base
        for name, v in ts.items():
            res[f"closure_N{N}_{name}_us"] = stats(v)
            res[f"closure_N{N}_{name}_us_all"] = v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.runs < 7:
        ap.error("--runs must be at least 7")
    dev = torch.device("cuda:0")
    N, wh = args.frames, (1080, 1920)
    m, tables = ST.make_model(dev)
    rig = S.KeypointRig.from_body_model(m, *tables, device=dev)
    R = PI.rotation_bank(24, (-0.3, 0.0, 0.3), device=dev)
    poses = PI.base_poses(rig)
    B, H = poses.shape[0], R.shape[0]
    res = {"device": torch.cuda.get_device_name(0), "V": int(m.v_template.shape[0]), "gathered_vertices": rig.VS, "model_points": rig.PA,
           "frames": N, "states": B * H, "runs": args.runs, "reps_per_region": args.reps, "unit": "us per call",
           "host": "tests/pose_init_ref.py: NumPy / torch float64 on the CPU"}
    pts = S.model_points(rig, PI._base_params(rig, poses, 10))
    Ks = torch.tensor([[1500.0, 0.0, 540.0], [0.0, 1500.0, 960.0], [0.0, 0.0, 1.0]]).repeat(N, 1, 1)
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.0, 0.1, 3.5])
    n = np.arange(N)
    b_true, h_true = (n // 64) % 2, 24 + (n // 8) % 24
    g = torch.Generator().manual_seed(3)
    cam_t = np.stack([0.2 * np.sin(n / 40.0), 0.1 + 0 * n, 3.5 + 0.5 * np.cos(n / 60.0)], 1)
    tab = (tables[0], tables[1], tables[2].cpu())
    tgt = PR.plant(pts.cpu(), pts[:, 0].cpu(), R.cpu()[h_true], b_true, cam_t, tab, Ks, torch.eye(4), wh, 0.4 + 0.6 * torch.rand(N, 137, generator=g))
    tgt[..., :2] += 2.0 * torch.randn(N, 137, 2, generator=g, dtype=torch.float64) / torch.tensor(wh, dtype=torch.float64)
    # (planted with an identity rotation in w2c: cam_t is the camera-space translation either way)
    target = tgt.float().to(dev)
    Kd, wd = Ks.to(dev), w2c.to(dev)
    scales = S.target_scales(target, wh)
    T = PI.transition_cost(R, B)

    search = lambda: PI.search(pts, pts[:, 0], R, rig, target, Kd, wd, wh, scales)
    sr_ = search()
    path = lambda: PI.viterbi_path(sr_.cost, T, sr_.transl, sr_.valid)
    init = lambda: PI.init_from_keypoints(rig, target, wh, Kd, wd, rotations=R, poses=poses)
    vit = path()
    res["frames_at_the_planted_state"] = float((vit.path.cpu().numpy() == b_true * H + h_true).mean())
    res["frames_valid"] = int(sr_.valid.sum())
    host_search = lambda: PR.search(pts.cpu(), pts[:, 0].cpu(), R.cpu(), tab, target.cpu(), Ks, w2c, wh, scales.cpu())
    U, Tn = sr_.cost.cpu().numpy(), T.cpu().numpy()
    tr, vd = sr_.transl.cpu().numpy(), sr_.valid.cpu().numpy()
    host_path = lambda: PR.fill(tr, PR.viterbi(U, Tn)[0], vd)
    ref = host_search()
    res["search_cost_worst_vs_float64"] = PR.sr.worst(np.where(np.isfinite(ref["cost"]), sr_.cost.cpu().numpy(), 0), np.where(np.isfinite(ref["cost"]), ref["cost"], 0))
    res["path_equals_host"] = bool((PR.viterbi(U, Tn)[0] == vit.path.cpu().numpy()).all())
    for fn in (search, path, init):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in ("search_hip", "viterbi_hip", "init_from_keypoints", "search_host", "viterbi_host")}
    for _ in range(args.runs):
        ts["search_hip"].append(ST.region(search, args.reps))
        ts["viterbi_hip"].append(ST.region(path, args.reps))
        ts["init_from_keypoints"].append(wall(init))
        t0 = time.perf_counter()
        host_search()
        ts["search_host"].append((time.perf_counter() - t0) * 1e6)
        t0 = time.perf_counter()
        host_path()
        ts["viterbi_host"].append((time.perf_counter() - t0) * 1e6)
    for k, v in ts.items():
        res[k + "_us"] = stats(v)
    res["search_host_over_hip"] = res["search_host_us"]["median"] / res["search_hip_us"]["median"]
    res["viterbi_host_over_hip"] = res["viterbi_host_us"]["median"] / res["viterbi_hip_us"]["median"]
    print(json.dumps(res), flush=True)
    if args.parent_lib:
        closure_ab(args.parent_lib, max(args.runs // 2, 3), res)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
