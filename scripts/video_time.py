"""Time the MJPEG video output (soar_amd/video.py) on the playback timing script's workload: 36 turntable frames at 1080 x 1920 of a
100k-surfel avatar, on one GPU, in one process after warm-up.

    python scripts/video_time.py [--iters 5] [--out profiles/video_time.json]

  * `AvatarPlayer.play` with PNGs only (the code path before the video output existed);
  * `AvatarPlayer.play(..., video=True)`: the same PNGs and the three `video.avi` files;
  * the encode stage alone on the 36 finished `rgb` frames, which are on the device: `write_video` (JPEG on the device, the compressed
    bytes copied to the host, the AVI file written) against the equal-bytes baseline on the host: the same frames copied to the host
    and saved with Pillow's JPEG encoder at the same quality, subsampling and restart interval into memory.  The two produce the same
    scan bytes, which the script checks;
  * the encoder alone by device events: `encode_jpeg` of a chunk of 8 frames into a buffer of its own (no synchronisation inside).
The three host-clock paths alternate within every iteration, so that whatever else the host is doing falls on all of them; medians,
minima and every sample are kept."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from playback_time import events, make_player  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402
from soar_amd import video  # noqa: E402
from soar_amd.renderer import cameras  # noqa: E402

QUALITY, SUBSAMPLING = 90, "420"


def scan_of(jpeg: bytes) -> bytes:
    """what lies between the end of SOS and EOI"""
    i = 2
    while True:
        n = (jpeg[i + 2] << 8) | jpeg[i + 3]
        if jpeg[i + 1] == 0xDA:
            return jpeg[i + 2 + n:-2]
        i += 2 + n


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--surfels", type=int, default=100000)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, F, P = args.height, args.width, args.frames, args.surfels
    player = make_player(P, 4, dev)
    spec = syn.make_camera(W, H, distance=3.0, elevation=0.1, azimuth=0.4)
    cam = cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(dev), image_width=W, image_height=H,
                         world_view_transform=spec.world_view_transform.to(dev), full_proj_transform=spec.full_proj_transform.to(dev),
                         prcppoint=spec.prcppoint.to(dev))
    bg = torch.ones(3, device=dev)
    poses = player.turntable(n=F, frame=0)
    ri = video.DEFAULT_RESTART_INTERVAL[SUBSAMPLING]
    opts = dict(fps=25, quality=QUALITY, subsampling=SUBSAMPLING)
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "frames": F, "surfels": P, "chunk": 8, "iters": args.iters,
           "quality": QUALITY, "subsampling": SUBSAMPLING, "restart_interval": ri}
    frames = player.render(poses, cam, bg=bg, chunk=8)["rgb"]                  # [F,H,W,4] on the device: what the encode stage is timed on
    tmp = tempfile.mkdtemp(prefix="video_time_")
    state = {}

    def play_png():
        player.play(poses, cam, os.path.join(tmp, "png"), bg=bg, chunk=8)

    def play_video():
        player.play(poses, cam, os.path.join(tmp, "video"), bg=bg, chunk=8, video=opts)

    def encode_device():
        state["writer"] = video.write_video(os.path.join(tmp, "clip.avi"), frames, chunk=8, **opts)

    def encode_host():
        host = frames.cpu().numpy()                                            # 4 bytes a pixel cross to the host
        out = []
        for i in range(F):
            b = io.BytesIO()
            Image.fromarray(host[i, :, :, :3]).save(b, "JPEG", quality=QUALITY, subsampling=2, optimize=False, restart_marker_blocks=ri)
            out.append(b.getvalue())
        state["pillow"] = out

    paths = {"play_png": play_png, "play_png_video": play_video, "encode_device": encode_device, "encode_host_pillow": encode_host}
    for fn in paths.values():                                                  # warm-up: every shape of the timed window
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    for _ in range(args.iters):
        for k, fn in paths.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    for k in paths:
        res[k + "_ms"], res[k + "_min_ms"], res[k + "_all_ms"] = statistics.median(ts[k]), min(ts[k]), ts[k]
    res["video_cost_in_play_ms"] = res["play_png_video_ms"] - res["play_png_ms"]
    res["ratio_host_pillow_over_device"] = res["encode_host_pillow_ms"] / res["encode_device_ms"]

    # the same bytes: the device's scan bytes are Pillow's, frame by frame
    ours = video.read_mjpeg_avi(os.path.join(tmp, "clip.avi"))
    res["scan_bytes_equal_to_pillow"] = len(ours) == F and all(scan_of(a) == scan_of(b) for a, b in zip(ours, state["pillow"]))
    res["bytes_to_host_device_path"] = state["writer"].bytes_to_host
    res["compressed_bytes"] = sum(len(f) for f in ours)
    res["bytes_to_host_host_path"] = frames.numel()
    res["avi_bytes"] = os.path.getsize(os.path.join(tmp, "clip.avi"))

    # the encoder alone: 8 frames into a buffer of its own
    chunk = frames[:8]
    data, offsets = video.encode_jpeg(chunk, quality=QUALITY, subsampling=SUBSAMPLING)
    out = torch.empty(data.numel() + 1024, dtype=torch.uint8, device=dev)
    med, low = events(lambda: video.encode_jpeg(chunk, quality=QUALITY, subsampling=SUBSAMPLING, out=out), 20)
    res["encode_8_frames_ms"], res["encode_8_frames_min_ms"] = med, low
    res["encode_8_frames_pixels_per_s"] = 8 * H * W / (med * 1e-3)
    res["encode_8_frames_compressed_bytes"] = int(offsets[-1])
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
