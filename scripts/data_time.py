"""Time the training data module (soar_amd/data.py) against the reference's path, on one GPU, in one process after warm-up.

    python scripts/data_time.py [--frames 64] [--iters 30] [--out profiles/data_time.json]

A synthetic 64-frame 1080 x 1920 sequence, the configuration's 4 views at 512 x 512.
  * `collate()` of the device-resident dataset (one launch; wall clock to the end of the launch, and the launch alone by device
    events) against the reference's path: the torch-CPU restatement of `collate` (tests/data_ref.py: the float32 video on the
    host, the rays built in torch-CPU) followed by `.to(device)` of every tensor from pageable memory, which is what Lightning does.
  * `soar_data_crops` over the sequence against `F.grid_sample` on the device (float frames already resident: torch's best case).
The launch's bytes (read + written) over its time are printed next to the 8 TB/s roofline."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import data_ref as R  # noqa: E402
from soar_amd import data as D  # noqa: E402

HBM_ROOFLINE = 8.0e12


def wall(fn, iters, warmup=5):
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


def events(fn, iters, warmup=5):
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
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W, B, RES = args.frames, 1080, 1920, 4, 512
    seq = R.synthetic_sequence(N, H, W, seed=0)
    cfg = dict(height=RES, width=RES, batch_size=B, n_view=4, smpl_type="smplx", rays_d_normalize=False, elevation_range=(0, 30),
               camera_distance_range=(0.8, 1.0), fovy_range=(15, 60))
    res = {"device": torch.cuda.get_device_name(0), "frames": N, "video": [H, W], "views": [B, RES, RES], "iters": args.iters}

    t0 = time.perf_counter()
    store = D.FrameStore.from_arrays(**seq, device=dev)
    torch.cuda.synchronize()
    res["store_construction_s"] = time.perf_counter() - t0
    ds = D.RandomMultiviewCameraDataset(cfg, store, "train")
    torch.manual_seed(0)
    random.seed(0)
    res["collate_ms"], res["collate_min_ms"] = wall(lambda: ds.collate(None), args.iters)
    t0 = time.perf_counter()
    for _ in range(args.iters):
        ds._draw()
    res["collate_host_draw_ms"] = (time.perf_counter() - t0) * 1e3 / args.iters
    # the launch alone: the last step's argument block issued again, 20 times between two events (the host keeps ahead of the device)
    import ctypes
    from soar_amd import hip_lib
    last, stream, REPEAT = ds._last_args, torch.cuda.current_stream(dev).cuda_stream, 20

    def relaunch():
        for _ in range(REPEAT):
            hip_lib.check(hip_lib.lib().soar_data_step_batch(ctypes.byref(last), stream), "soar_data_step_batch")

    med, low = events(relaunch, args.iters)
    res["collate_launch_ms"], res["collate_launch_min_ms"] = med / REPEAT, low / REPEAT
    # the launch's traffic: every output written once; the frame's bytes, its crops' rows read once
    pix, crop = H * W, D.CROP * D.CROP
    written = 4 * (2 * B * RES * RES * 3 + 2 * crop * 3 + pix * 3 + pix + 2 * crop * 3 + crop + crop * 3 + crop)
    read = pix * 3 + pix + 2 * crop * 3 + crop + 4 * (crop * 3 + crop)
    res["launch_bytes_written"], res["launch_bytes_read"] = written, read
    res["launch_bytes_per_s"] = (written + read) / (res["collate_launch_ms"] * 1e-3)
    res["launch_share_of_8TBs_roofline"] = res["launch_bytes_per_s"] / HBM_ROOFLINE

    # the reference's path on the same box: torch-CPU collate, then every tensor to the device from pageable memory
    state = R.make_state(cfg, **seq, with_crops=False)
    state.frames_img_crop, state.frames_mask_crop = store.rgb_crop.cpu(), store.mask_crop.cpu()

    def to_device(x):
        if torch.is_tensor(x):
            return x.to(dev)
        return {k: to_device(v) for k, v in x.items()} if isinstance(x, dict) else x

    def reference_step():
        return to_device(R.collate(state))

    res["reference_collate_and_copy_ms"], res["reference_collate_and_copy_min_ms"] = wall(reference_step, args.iters)
    t0 = time.perf_counter()
    for _ in range(args.iters):
        R.collate(state)
    res["reference_collate_cpu_ms"] = (time.perf_counter() - t0) * 1e3 / args.iters
    res["speedup_collate"] = res["reference_collate_and_copy_ms"] / res["collate_ms"]
    del state

    # crops: one launch over the byte video against F.grid_sample over float frames already on the device, 8 frames at a time
    res["crops_ms"], res["crops_min_ms"] = events(lambda: D.crops(store.images, store.masks, store.boxes), max(5, args.iters // 3), warmup=2)
    imgs, masks = R.float_frames(seq["images"][:8], seq["masks"][:8])
    grids = torch.cat([R.crop_grid(R.mask_bbox(m), H, W)[0] for m in masks]).to(dev)
    imgs_d, masks_d = imgs.permute(0, 3, 1, 2).contiguous().to(dev), masks[:, None].contiguous().to(dev)

    def torch_crops():
        F.grid_sample(imgs_d, grids, mode="bilinear", align_corners=False)
        F.grid_sample(masks_d, grids, mode="bilinear", align_corners=False)

    t8, _ = events(torch_crops, max(5, args.iters // 3), warmup=2)
    res["grid_sample_device_ms_scaled_to_all_frames"] = t8 * N / 8
    res["speedup_crops"] = res["grid_sample_device_ms_scaled_to_all_frames"] / res["crops_ms"]
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
