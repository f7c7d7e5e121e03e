"""Time the JPEG input on the device (soar_amd/jpeg.py, csrc/jpeg_decode.hip) and frame extraction (soar_amd/frames.py): 36 frames of
1080 x 1920 at quality 90, on one GPU, in one process after warm-up.

    python scripts/jpeg_decode_time.py [--iters 3] [--out profiles/jpeg_decode_time.json]

The frames are coded twice: (a) by the project's own encoder at 4:2:0 (restart markers every 4 MCUs: thousands of intervals per
file, decoded in parallel) and (b) by Pillow (no restart markers: one interval per file, one lane's serial work).
  * `decode_jpeg` alone by device events, the files' bytes already on the device, for (a) and for (b), and the intervals it found;
  * the whole device path (bytes uploaded, decoded) against Pillow decoding on the host plus the upload of the pixels -- the same
    bytes out, which is checked -- at N = 1 .. 36 files, the two alternating, every sample kept: where the two cross, if they do;
    and the device path alone call after call (alternating, it starts on a device that the host path has left idle for a while);
  * `extract_frames` end to end from an `.avi` written by `MjpegWriter`, at the frames' own size and scaled to a height of 540."""
import argparse
import io
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from playback_time import events  # noqa: E402
from png_decode_time import synthetic, wall  # noqa: E402
from soar_amd import codec_io, jpeg  # noqa: E402
from soar_amd.frames import extract_frames  # noqa: E402
from soar_amd.video import MjpegWriter, encode_jpeg  # noqa: E402


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
    frames = synthetic(N, H, W, dev)["images"]
    data, offsets = encode_jpeg(frames, quality=90, subsampling="420")
    host, off = data.cpu().numpy().tobytes(), offsets.tolist()
    files = {"own_420_restart_4": [host[off[b]:off[b + 1]] for b in range(N)], "pillow_420_no_restart": []}
    for im in frames.cpu().numpy():
        buf = io.BytesIO()
        Image.fromarray(im).save(buf, "JPEG", quality=90)
        files["pillow_420_no_restart"].append(buf.getvalue())
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "frames": N, "quality": 90, "iters": args.iters, "chunk": N}

    def pillow_path(blobs):
        return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(b))) for b in blobs])).to(dev)

    def device_path(blobs):
        return jpeg.decode_blobs(blobs, H, W, 3, dev)[0]

    for name, blobs in files.items():
        r = res[name] = {"compressed_bytes": sum(len(b) for b in blobs), "raw_bytes": N * H * W * 3}
        d, o = codec_io.upload(blobs, dev)
        out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
        _, status, intervals = jpeg.decode_jpeg(d, o, H, W, 3, strict=False, out=out, return_info=True)
        med, low = events(lambda: jpeg.decode_jpeg(d, o, H, W, 3, strict=False, out=out), 5, warmup=1)
        r["decode_jpeg"] = {"files": N, "ms": med, "min_ms": low, "pixels_per_s": N * H * W / (med * 1e-3),
                            "intervals_per_file": sorted(set(intervals.tolist())), "all_ok": bool((status == 0).all()),
                            "equal_to_pillow": bool(torch.equal(out, pillow_path(blobs)))}
        one = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)
        d1, o1 = codec_io.upload(blobs[:1], dev)
        med, low = events(lambda: jpeg.decode_jpeg(d1, o1, H, W, 3, strict=False, out=one), 5, warmup=1)
        r["decode_jpeg_one_file"] = {"ms": med, "min_ms": low}
        cross = r["by_n"] = {}
        for n in (1, 2, 4, 8, 16, N):
            if n > N:
                continue
            paths = {"pillow_decode_and_upload_ms": lambda n=n: pillow_path(blobs[:n]), "upload_and_decode_jpeg_ms": lambda n=n: device_path(blobs[:n])}
            for fn in paths.values():
                wall(fn)
            ts = {k: [] for k in paths}
            for _ in range(args.iters):
                for k, fn in paths.items():
                    ts[k].append(wall(fn)[0])
            cross[str(n)] = {k: statistics.median(v) for k, v in ts.items()}
            cross[str(n)].update({k.replace("_ms", "_all_ms"): v for k, v in ts.items()})
            # ... and the device path alone, call after call: alternating, it starts on a device the host path has left idle
            cross[str(n)]["upload_and_decode_jpeg_back_to_back_ms"] = statistics.median(wall(paths["upload_and_decode_jpeg_ms"])[0] for _ in range(args.iters))
        faster = [int(n) for n, v in cross.items() if v["upload_and_decode_jpeg_ms"] < v["pillow_decode_and_upload_ms"]]
        r["device_path_faster_from_n"] = min(faster) if faster else None

    # frame extraction end to end: video in, folder of PNGs out
    tmp = tempfile.mkdtemp(prefix="jpeg_decode_time_")
    video = os.path.join(tmp, "clip.avi")
    with MjpegWriter(video, H, W, fps=30, quality=90) as w:
        for i in range(0, N, 8):
            w.write(frames[i:i + 8])
    r = res["extract_frames"] = {"video_bytes": os.path.getsize(video)}
    for label, height in (("same_size", -1), ("height_540", 540)):
        ts = []
        for it in range(args.iters + 1):                          # the first pass warms up
            root = os.path.join(tmp, f"{label}_{it}")
            ts.append(wall(lambda: extract_frames(video, root, height=height))[0])
            r[f"{label}_png_bytes"] = sum(os.path.getsize(os.path.join(root, "clip", "images", f)) for f in os.listdir(os.path.join(root, "clip", "images")))
            shutil.rmtree(root, ignore_errors=True)
        r[f"{label}_ms"], r[f"{label}_all_ms"] = statistics.median(ts[1:]), ts[1:]
    shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
