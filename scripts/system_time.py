"""One training step of each stage through `SurfelMVDreamSystem`, timed against the same step composed by hand.

The shapes are the shipped configs' (TS/configs/gaussiansurfel_imagedream_s{0,1}.yaml): four SDS views at 512 x 512, one video frame
at 1080 x 1920, two normal views at 512 x 512, P = 100k surfels, `use_explicit: false`.  The UNet is not part of this package: the
guidance is `MultiviewSDS` over a `LatentEncoder` with random weights at `image_size` 64 and a linear stand-in for the UNet, the
LPIPS network has random weights -- the scene, the guidance and the composed step are those of the tests (tests/system_scene.py) at
other sizes.  The composed step stops in front of the optimizer, so the system is timed the same way.

    python scripts/system_time.py [--steps 20] [--warmup 5] [--out profiles/system_time.json] [--small]

`--small`: the tests' sizes (what tests/test_system_gpu.py runs this script at).  Per stage: the median over `--steps` steps of the
wall time of a step with one synchronisation at its end, and of the time the host needs to issue it.  Median, not mean: the first
steps after a resolution change allocate.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import torch  # noqa: E402

import system_scene as T  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, issue = [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        wall.append(t2 - t0)
        issue.append(t1 - t0)
    return {"wall_ms_median": 1e3 * statistics.median(wall), "issue_ms_median": 1e3 * statistics.median(issue),
            "wall_ms_min": 1e3 * min(wall), "wall_ms_max": 1e3 * max(wall), "steps": steps}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "system_time.json"))
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args(argv)
    sz = T.SMALL if a.small else T.CONFIG
    w = T.make_world(sz)
    res = {"shapes": {"P": sz.P, "sds_views": [4, sz.VIEW, sz.VIEW], "frame": [sz.H, sz.W], "normal_views": [2, sz.RES, sz.RES]},
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "stages": {}}
    for stage in (0, 1):
        it = 600                                              # beyond sds_start in both stages: every term of the step is on
        system = T.build(w, stage)
        composed = T.build(w, stage)

        def system_step():
            geo = system.geometry
            system.global_step = it
            T.seeded()
            geo.invalidate()                                  # (no optimizer step lies between two repeats: a fresh activation node)
            batch = dict(w.batch)
            system.logged = {}
            out, gt_out = system.forward(batch, head_flag=False)
            loss_sds, loss = system.compute_losses(batch, out, gt_out)
            loss_sds.backward(retain_graph=True)
            loss.backward()
            geo.optimizer.zero_grad(set_to_none=True)

        res["stages"][str(stage)] = {"system": timed(system_step, a.steps, a.warmup),
                                     "composed_by_hand": timed(lambda: T.compose_reference_step(composed, w.batch, it), a.steps, a.warmup)}
        print(json.dumps({str(stage): res["stages"][str(stage)]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")
    return res


if __name__ == "__main__":
    main()
