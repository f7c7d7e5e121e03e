"""Time the PNG input on the device (soar_amd/png.py, csrc/png_decode.hip) on a synthetic sequence directory: 36 frames of 1080 x 1920
(images/, masks/, and normal_F/ and normal_B/ at 512 x 512), on one GPU, in one process after warm-up.

    python scripts/png_decode_time.py [--iters 3] [--out profiles/png_decode_time.json]

The directory is written twice: (a) by Pillow at its default level -- one serial deflate stream per file, what ffmpeg's and Pillow's
files are -- and (b) by the device writers (soar_amd.png.write_png_files), whose files are independent pieces.
  * `FrameStore.from_dataroot` as it was (one `PIL.Image.open` per file on the host, raw arrays uploaded) against
    `from_dataroot(..., device_png=True)`, on (a) and on (b); the paths alternate within every iteration, after one warm-up pass;
  * `decode_png` alone by device events: 32 files of images/ already on the device, for (a) and for (b); and the segments it found;
  * the bytes uploaded on each path;
  * images/ alone at N = 1 .. 36 files, `read_png_files` against the Pillow loop: where the two cross.
The two stores of a directory are compared tensor by tensor."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from playback_time import events  # noqa: E402
from soar_amd import png  # noqa: E402
from soar_amd.data import CROP, FrameStore  # noqa: E402

FOLDERS = ("images", "masks", "normal_F", "normal_B")


def synthetic(N, H, W, dev):
    """an avatar-like sequence: a shaded body with 2-level noise on white, its mask, and smooth normal maps inside a disc"""
    g = torch.Generator(device=dev).manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    images, masks = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev), torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    for n in range(N):
        cx, cy = W * (0.45 + 0.1 * np.sin(n / 6.0)), H * 0.52
        inside = ((xx - cx) / (0.16 * W)) ** 2 + ((yy - cy) / (0.42 * H)) ** 2 <= 1.0
        shade = 90 + 100 * (xx - cx + 0.16 * W) / (0.32 * W) + 30 * torch.sin(yy / 37.0)
        body = torch.stack([shade, 0.8 * shade + 20, 0.6 * shade + 40], dim=-1) + torch.randint(0, 2, (H, W, 3), generator=g, device=dev)
        images[n] = torch.where(inside[..., None], body.clamp(0, 255), torch.full_like(body, 255.0)).to(torch.uint8)
        masks[n] = inside.to(torch.uint8) * 255
    u = torch.linspace(-1, 1, CROP, device=dev)
    ny, nx = torch.meshgrid(u, u, indexing="ij")
    disc = nx * nx + ny * ny <= 0.8
    nz = torch.sqrt((1 - nx * nx - ny * ny).clamp_min(0))
    normal = ((torch.stack([nx, ny, nz], dim=-1) * 0.5 + 0.5) * 255).to(torch.uint8) * disc[..., None]
    nF = torch.cat([normal, (disc.to(torch.uint8) * 255)[..., None]], dim=-1)[None].repeat(N, 1, 1, 1)
    for n in range(N):
        nF[n, :, :, 0] = nF[n, :, :, 0].roll(n, dims=1)
    nB = nF[..., :3].flip(2).contiguous()
    return dict(images=images, masks=masks, normal_F=nF, normal_B=nB)


def write_root(root, seq, device_writers):
    from PIL import Image
    N = seq["images"].shape[0]
    for d in FOLDERS + ("smplx",):
        os.makedirs(os.path.join(root, d))
    for d in FOLDERS:
        paths = [os.path.join(root, d, f"{i:05d}.png") for i in range(N)]
        if device_writers:
            png.write_png_files(paths, seq[d])
        else:
            for p, im in zip(paths, seq[d].cpu().numpy()):
                Image.fromarray(im).save(p)
    K = torch.tensor([[1500.0, 0.0, 960.0], [0.0, 1500.0, 540.0], [0.0, 0.0, 1.0]]).repeat(N, 1, 1)
    torch.save(dict(w2c=torch.eye(4), Ks=K, normal_Ks=K.clone(), betas=torch.zeros(10), body_pose=torch.zeros(N, 63),
                    global_orient=torch.zeros(N, 3), transl=torch.zeros(N, 3) + torch.tensor([0.0, 0.0, 6.0])), os.path.join(root, "smplx", "params.pth"))


def folder_bytes(root):
    return {d: sum(os.path.getsize(os.path.join(root, d, n)) for n in os.listdir(os.path.join(root, d))) for d in FOLDERS}


def same_store(x, y):
    keys = ("images", "masks", "normal_F", "normal_B", "normal_mask", "boxes", "rgb_crop", "mask_crop")
    return all(torch.equal(getattr(x, k), getattr(y, k)) for k in keys)


def wall(fn):
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W = args.frames, args.height, args.width
    seq = synthetic(N, H, W, dev)
    tmp = tempfile.mkdtemp(prefix="png_decode_time_")
    roots = {"pillow": os.path.join(tmp, "a"), "device_writers": os.path.join(tmp, "b")}
    write_root(roots["pillow"], seq, False)
    write_root(roots["device_writers"], seq, True)
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "normal_maps": [CROP, CROP], "frames": N, "iters": args.iters, "chunk": 32}
    raw = sum(seq[d].numel() for d in FOLDERS)
    for name, root in roots.items():
        paths = {"host": lambda root=root: FrameStore.from_dataroot(root, "smplx", device=dev),
                 "device_png": lambda root=root: FrameStore.from_dataroot(root, "smplx", device=dev, device_png=True)}
        stores = {k: wall(fn)[1] for k, fn in paths.items()}                       # the warm-up pass
        ts = {k: [] for k in paths}
        for _ in range(args.iters):
            for k, fn in paths.items():
                ts[k].append(wall(fn)[0])
        r = res[name] = {"file_bytes": folder_bytes(root), "stores_equal": bool(same_store(stores["host"], stores["device_png"]))}
        for k in paths:
            r[f"from_dataroot_{k}_ms"], r[f"from_dataroot_{k}_min_ms"], r[f"from_dataroot_{k}_all_ms"] = statistics.median(ts[k]), min(ts[k]), ts[k]
        r["ratio_host_over_device"] = r["from_dataroot_host_ms"] / r["from_dataroot_device_png_ms"]
        r["bytes_uploaded_host_path"] = raw
        r["bytes_uploaded_device_path"] = sum(r["file_bytes"].values())
        del stores

        # the decoder alone: 32 files of images/, already on the device
        names = sorted(os.listdir(os.path.join(root, "images")))[:32]
        blobs = [open(os.path.join(root, "images", n), "rb").read() for n in names]
        off = np.cumsum([0] + [len(b) for b in blobs]).astype(np.int64)
        data, offsets = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).to(dev), torch.from_numpy(off).to(dev)
        out = torch.empty((len(blobs), H, W, 3), dtype=torch.uint8, device=dev)
        _, status, segments = png.decode_png(data, offsets, H, W, 3, strict=False, out=out, return_info=True)
        med, low = events(lambda: png.decode_png(data, offsets, H, W, 3, strict=False, out=out), 5, warmup=1)
        r["decode_png_images"] = {"files": len(blobs), "ms": med, "min_ms": low, "pixels_per_s": len(blobs) * H * W / (med * 1e-3),
                                  "compressed_bytes": int(off[-1]), "segments_per_file": sorted(set(segments.tolist())),
                                  "all_ok": bool((status == 0).all()), "equal_to_the_source": bool(torch.equal(out, seq["images"][:len(blobs)]))}

        # images/ alone at growing N: where the two paths cross
        cross = r["images_folder_by_n"] = {}
        all_paths = [os.path.join(root, "images", n) for n in sorted(os.listdir(os.path.join(root, "images")))]
        for n in (1, 2, 4, 8, 16, N):
            if n > N:
                continue
            host = lambda: torch.from_numpy(np.stack([np.array(Image.open(p)) for p in all_paths[:n]])).to(dev)
            device = lambda: png.read_png_files(all_paths[:n], dev)
            wall(host), wall(device)
            th, td = [], []
            for _ in range(args.iters):
                th.append(wall(host)[0])
                td.append(wall(device)[0])
            cross[str(n)] = {"pillow_ms": statistics.median(th), "read_png_files_ms": statistics.median(td)}
        faster = [int(n) for n, v in cross.items() if v["read_png_files_ms"] < v["pillow_ms"]]
        r["device_path_faster_from_n"] = min(faster) if faster else None
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
