"""Time the PNG output on the device (soar_amd/png.py) on the video timing script's workload: 36 turntable frames at 1080 x 1920 of a
100k-surfel avatar, on one GPU, in one process after warm-up.

    python scripts/png_time.py [--iters 3] [--out profiles/png_time.json]

  * `AvatarPlayer.play` as it was (raw images copied to the host, `PIL.Image.save` once per image) against
    `AvatarPlayer.play(..., device_png=True)`; the two alternate within every iteration, so that whatever else the host is doing falls
    on both; medians, minima and every sample are kept;
  * where the device path's time goes: `render` alone, `write_png_files` on the four finished outputs (encode, copy, write), and the
    writing of the same bytes from host memory alone;
  * the encoder alone by device events: `encode_png` of 8 RGBA frames into a buffer of its own (no synchronisation inside), at pieces
    of 16 KiB, 32 KiB and 65535 bytes -- the measurement behind `DEFAULT_PIECE_BYTES`;
  * bytes copied to the host on either path, and the files' total bytes against Pillow's for the same images at its default level
    (what `play` writes without `device_png`) and at `compress_level=1`.
Every file of the device path is opened with Pillow and compared with the image it was made from."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from playback_time import events, make_player  # noqa: E402
from soar_amd import png  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402
from soar_amd.renderer import cameras  # noqa: E402

KEYS = ("rgb", "normal", "occ", "mask")


def folder_bytes(folder: str) -> int:
    return sum(os.path.getsize(os.path.join(folder, k, n)) for k in KEYS for n in os.listdir(os.path.join(folder, k)))


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
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
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "frames": F, "surfels": P, "chunk": 8, "iters": args.iters,
           "piece_bytes": png.DEFAULT_PIECE_BYTES}
    tmp = tempfile.mkdtemp(prefix="png_time_")
    state = {}

    def play_host():
        player.play(poses, cam, os.path.join(tmp, "host"), bg=bg, chunk=8)

    def play_device():
        player.play(poses, cam, os.path.join(tmp, "device"), bg=bg, chunk=8, device_png=True)

    def render_only():
        state["res"] = player.render(poses, cam, bg=bg, chunk=8)

    def write_only():
        state["copied"] = sum(png.write_png_files([os.path.join(tmp, "write", f"{k}{i:05d}.png") for i in range(F)], state["res"][k], chunk=8)
                              for k in KEYS)

    def files_only():
        for i, b in enumerate(state["blobs"]):
            with open(os.path.join(tmp, "files", f"{i:05d}.png"), "wb") as fh:
                fh.write(b)

    os.makedirs(os.path.join(tmp, "write"))
    os.makedirs(os.path.join(tmp, "files"))
    render_only()
    write_only()
    state["blobs"] = [open(os.path.join(tmp, "write", n), "rb").read() for n in sorted(os.listdir(os.path.join(tmp, "write")))]
    paths = {"play_host_png": play_host, "play_device_png": play_device, "render": render_only, "write_png_files": write_only,
             "file_writes": files_only}
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
    res["ratio_host_over_device"] = res["play_host_png_ms"] / res["play_device_png_ms"]

    # bytes: what crosses to the host, and the files against Pillow's
    out = state["res"]
    res["bytes_to_host_device_path"] = state["copied"]
    res["bytes_to_host_host_path"] = sum(out[k].numel() for k in KEYS)
    res["file_bytes_device"] = folder_bytes(os.path.join(tmp, "device"))
    res["file_bytes_pillow_default"] = folder_bytes(os.path.join(tmp, "host"))
    level1, same = 0, True
    for k in KEYS:
        host = out[k].cpu().numpy()
        for i in range(F):
            b = io.BytesIO()
            Image.fromarray(host[i]).save(b, "PNG", compress_level=1)
            level1 += len(b.getvalue())
            back = Image.open(os.path.join(tmp, "device", k, f"{i:05d}.png"))
            same = same and back.mode == ("L" if k == "mask" else "RGBA") and np.array_equal(np.asarray(back), host[i])
    res["file_bytes_pillow_level_1"] = level1
    res["device_files_decode_to_the_images"] = bool(same)

    # the encoder alone: 8 RGBA frames into a buffer of its own, at three piece sizes
    chunk = out["rgb"][:8]
    buf = torch.empty(8 * png.png_bound(H, W, 4, 16384), dtype=torch.uint8, device=dev)
    res["encode_8_frames"] = {}
    for piece in (16384, 32768, 65535):
        _, offsets = png.encode_png(chunk, piece_bytes=piece, out=buf)
        med, low = events(lambda: png.encode_png(chunk, piece_bytes=piece, out=buf), 20)
        res["encode_8_frames"][str(piece)] = {"ms": med, "min_ms": low, "pixels_per_s": 8 * H * W / (med * 1e-3),
                                              "compressed_bytes": int(offsets[-1])}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
