"""Time the test-split evaluation (soar_amd/evaluate.py) of one 1080 x 1920 frame, on one GPU, in one process after warm-up.

    python scripts/eval_time.py [--iters 20] [--out profiles/eval_time.json]

  * the launch alone (soar_eval_image_metrics: the tile kernel and the small reduction behind it), by device events, with and without
    the byte image; its bytes (read and written) over its time are printed next to the 8 TB/s roofline;
  * `image_metrics` with LPIPS (seeded random VGG weights: the time does not depend on their values), wall clock;
  * the reference's path on the same box: three device-to-host copies, then the white target, PSNR and the float32
    `scipy.ndimage.uniform_filter` SSIM of tests/eval_ref.py, which is what skimage runs (skimage itself is not installed here, and
    the reference's LPIPS on the CPU is left out: the figure is a lower bound of the reference's time)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import eval_ref as R  # noqa: E402
import lpips_ref as LR  # noqa: E402
from soar_amd import evaluate as E  # noqa: E402
from soar_amd import hip_lib  # noqa: E402
from soar_amd.lpips import LPIPSVGG  # noqa: E402

HBM_ROOFLINE = 8.0e12


def wall(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def events(fn, iters, warmup=3):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W = 1080, 1920
    pred_h, gt_h, mask_h = R.make_case(1, H, W, "smooth", noise=0.05, mask="blob", seed=0)
    pred, gt, mask = (torch.from_numpy(a).to(dev) for a in (pred_h, gt_h, mask_h))
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "iters": args.iters}

    # the launch alone: the same argument block issued 20 times between two events
    L, stream, REPEAT = hip_lib.lib(), torch.cuda.current_stream(dev).cuda_stream, 20
    nb = ctypes.c_size_t(0)
    hip_lib.check(L.soar_eval_scratch_bytes(1, H, W, ctypes.byref(nb)), "soar_eval_scratch_bytes")
    scratch = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    out = torch.empty((3, 1, H, W, 3), device=dev)
    metrics = torch.empty((1, 3), dtype=torch.float64, device=dev)
    grid = torch.empty((1, H, 2 * W, 3), dtype=torch.uint8, device=dev)
    a = hip_lib.SoarEvalArgs()
    a.N, a.H, a.W = 1, H, W
    a.pred, a.gt_rgb, a.gt_mask = pred.data_ptr(), gt.data_ptr(), mask.data_ptr()
    for i in range(4):
        a.pred_stride[i], a.gt_stride[i] = pred.stride(i), gt.stride(i)
    for i in range(3):
        a.mask_stride[i] = mask.stride(i)
    a.gt_white, a.pred2, a.gt2, a.metrics = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), metrics.data_ptr()

    def relaunch():
        for _ in range(REPEAT):
            hip_lib.check(L.soar_eval_image_metrics(ctypes.byref(a), scratch.data_ptr(), nb.value, stream), "soar_eval_image_metrics")

    pix = H * W
    read, written = 4 * (3 * pix + 3 * pix + pix), 4 * 3 * 3 * pix
    for name, g, extra in (("launch", None, 0), ("launch_with_grid", grid.data_ptr(), 2 * 3 * pix)):
        a.grid = g
        med, low = events(relaunch, args.iters)
        res[name + "_ms"], res[name + "_min_ms"] = med / REPEAT, low / REPEAT
        res[name + "_bytes_read"], res[name + "_bytes_written"] = read, written + extra
        res[name + "_bytes_per_s"] = (read + written + extra) / (res[name + "_ms"] * 1e-3)
        res[name + "_share_of_8TBs_roofline"] = res[name + "_bytes_per_s"] / HBM_ROOFLINE
    res["scratch_bytes"] = nb.value

    res["image_metrics_ms"], _ = wall(lambda: E.image_metrics(pred, gt, mask), args.iters)
    model = LPIPSVGG(LR.lpips_state_dict(LR.random_weights())).to(dev)
    res["image_metrics_with_lpips_ms"], res["image_metrics_with_lpips_min_ms"] = wall(lambda: E.image_metrics(pred, gt, mask, lpips=model), args.iters)

    # the reference's path, without its LPIPS: copies to the host, then skimage's arithmetic in NumPy / scipy
    def reference_frame():
        p, g, m = pred[0].cpu().numpy(), gt[0].cpu().numpy(), mask[0].cpu().numpy()
        gw = R.white_target(g, m)
        return R.psnr(p, gw), R.ssim7_filter(p, gw, np.float32)

    res["reference_host_psnr_ssim_ms"], res["reference_host_psnr_ssim_min_ms"] = wall(reference_frame, max(3, args.iters // 5), warmup=1)
    res["speedup_psnr_ssim"] = res["reference_host_psnr_ssim_ms"] / res["image_metrics_ms"]
    m = E.image_metrics(pred, gt, mask)
    psnr_ref, ssim_ref = reference_frame()
    res["psnr"], res["ssim"] = m["psnr"].item(), m["ssim"].item()
    res["ssim_minus_float32_scipy"], res["psnr_minus_host"] = res["ssim"] - ssim_ref, res["psnr"] - psnr_ref
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
