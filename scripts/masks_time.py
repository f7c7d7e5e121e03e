"""Time the mask clean-up (soar_amd/masks.py, csrc/masks.hip) on one GPU, in one process after warm-up.

    python scripts/masks_time.py [--frames 16] [--size 1080 1920] [--iters 20] [--reps 3] [--out profiles/masks_time.json]

The scene: ``frames`` frames of blobs (a Gaussian-filtered noise field above zero, sigma 12, plus 1 % salt noise), each split into
K = 3 candidates, as uint8 and as float32 logits.  ``clean_masks`` (the whole pipeline: 7 launches and 2 memsets per chunk) is timed
between device events; the figure is the median over ``iters`` regions of ``reps`` calls.  Next to it, where scipy imports, the host
path: the device-to-host copy of the candidates, then per frame ``scipy.ndimage`` erosion / dilation with the same border values,
``label`` with the 3 x 3 structure and the largest component, and the copy back of the masks.

The split of the HIP path by launch comes from one traced call under ``torch.profiler`` (device time per kernel name); the entry
points ``open_close`` and ``largest_component`` are timed with events as well.  ``union_read_GBps`` is the bytes of the candidates
over the time of the one launch that reads them (masks_pack_morph_kernel)."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from soar_amd import hip_lib, masks  # noqa: E402
import masks_ref as R  # noqa: E402


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps           # microseconds per call


def median_us(fn, iters, reps, warmup=3):
    for _ in range(warmup):
        region(fn, reps)
    ts = [region(fn, reps) for _ in range(iters)]
    return statistics.median(ts), min(ts)


def launches(fn):
    """device microseconds per kernel name of one call, in the order of the first launch"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        if getattr(ev, "device_type", None) is not None and "cuda" in str(ev.device_type).lower():
            name = ev.name.replace("(anonymous namespace)::", "").replace("void ", "").replace("soar::", "").split("(")[0].split("<")[0].strip()
            d = out.setdefault(name, {"launches": 0, "us": 0.0})
            d["launches"] += 1
            d["us"] += float(getattr(ev, "device_time", 0.0) or getattr(ev, "cuda_time", 0.0))
    return out


def host_path(cand_dev):
    """-> (seconds for copy down, scipy and copy up; masks) -- None where scipy is missing"""
    try:
        from scipy import ndimage as ndi
    except ImportError:
        return None
    box, eight = np.ones((5, 5), bool), np.ones((3, 3), bool)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cand = cand_dev.cpu().numpy()
    t1 = time.perf_counter()
    out = np.zeros((cand.shape[0],) + cand.shape[2:], np.uint8)
    for i, c in enumerate(cand):
        m = (c > 0).any(0)
        m = ndi.binary_dilation(ndi.binary_erosion(m, box, border_value=1), box, border_value=0)
        m = ndi.binary_erosion(ndi.binary_dilation(m, box, border_value=0), box, border_value=1)
        lab, n = ndi.label(m, structure=eight)
        if n:
            out[i] = lab == (np.argmax(np.bincount(lab.reshape(-1))[1:]) + 1)
    t2 = time.perf_counter()
    back = torch.from_numpy(out).to(cand_dev.device)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    return {"copy_down_ms": (t1 - t0) * 1e3, "scipy_ms": (t2 - t1) * 1e3, "copy_up_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t0) * 1e3}, back


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, nargs=2, default=[1080, 1920])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, (H, W), K = args.frames, args.size, 3
    base = R.blobs(H, W, 12.0, 0, salt=0.01)
    frames = [np.roll(base, (37 * i, 101 * i), axis=(0, 1)) for i in range(N)]               # N different frames of one field
    u8 = torch.from_numpy(np.stack([R.split_candidates(f, K, i) for i, f in enumerate(frames)])).to(dev)
    f32 = torch.where(u8 != 0, 3.0, -3.0).to(torch.float32)
    res = {"device": torch.cuda.get_device_name(0), "frames": N, "K": K, "size": [H, W], "reps_per_region": args.reps, "regions": args.iters,
           "unit": "us per call (median, min)", "library": os.path.basename(hip_lib.LIB_PATH),
           "workspace_bytes": masks.workspace_bytes(N, H, W), "launch_split_source": "torch.profiler, one traced call"}
    ref, ref_stats = masks.clean_masks(u8, return_stats=True)
    res["stats_frame0"] = dict(zip(masks.STATS, ref_stats[0].tolist()))
    gc.collect()
    gc.freeze()
    gc.disable()
    for name, cand in (("uint8", u8), ("float32", f32)):
        assert torch.equal(masks.clean_masks(cand), ref)
        t_clean = median_us(lambda: masks.clean_masks(cand), args.iters, args.reps)
        t_oc = median_us(lambda: masks.open_close(cand), args.iters, args.reps)
        r = {"clean_masks_us": t_clean[0], "clean_masks_min_us": t_clean[1], "clean_masks_us_per_frame": t_clean[0] / N,
             "open_close_us": t_oc[0], "open_close_min_us": t_oc[1], "candidate_bytes": cand.numel() * cand.element_size()}
        try:
            split = launches(lambda: masks.clean_masks(cand))
            r["launches"] = split
            pack = [v for k, v in split.items() if "pack_morph" in k]
            if pack and pack[0]["us"] > 0:
                r["union_read_GBps"] = r["candidate_bytes"] / (pack[0]["us"] * 1e-6) / 1e9
        except Exception as e:                                   # the tracer is the profiler's, not this project's
            r["launches"] = f"torch.profiler failed: {type(e).__name__}: {e}"
        res[name] = r
        print(json.dumps({name: r}), flush=True)
    t_lc = median_us(lambda: masks.largest_component(ref), args.iters, args.reps)
    res["largest_component_us"], res["largest_component_min_us"] = t_lc
    host = host_path(u8)
    if host is None:
        res["host_path"] = "scipy is not installed"
    else:
        host_path(u8)                                            # the second run is the one reported
        res["host_path"], back = host_path(u8)
        res["host_path"]["equal_to_hip"] = bool(torch.equal(back, ref))
        res["host_over_hip"] = res["host_path"]["total_ms"] * 1e3 / res["uint8"]["clean_masks_us"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
