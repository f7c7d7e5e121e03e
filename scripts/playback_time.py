"""Time avatar playback (soar_amd/playback.py): 36 turntable frames at 1080 x 1920 of a 100k-surfel avatar, on one GPU, in one
process after warm-up.

    python scripts/playback_time.py [--iters 5] [--out profiles/playback_time.json]

  * `AvatarPlayer.render` (field and blend weights once, the joint chain of all frames in one launch, chunks of 8 frames through the
    batched path, one soar_playback_finish launch per chunk), then the four byte tensors copied to the host;
  * the baseline on the same box, in the same process: the same frames rendered one plugin `forward()` per frame under `no_grad`
    (field, blend-weight cache, joint chain and the per-view path every frame), torch's conversion
    `x.mul(255).add_(0.5).clamp_(0, 255).to(uint8)` on the device, the byte images copied to the host per frame;
  * the two kernels alone, by device events: soar_motion_resample for the 36 frames, soar_playback_finish for a chunk of 8 frames with
    its bytes over its time next to the 8 TB/s roofline.
The avatar is synthetic (soar_amd.synthetic) with a seeded attribute field of the reference's size."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from soar_amd import playback as pb  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402
from soar_amd.field import HashMLPField  # noqa: E402
from soar_amd.renderer import cameras  # noqa: E402
from soar_amd.smpl_guidance import SMPLGuidance  # noqa: E402

HBM_ROOFLINE = 8.0e12


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


def make_player(P, n_keys, dev):
    surf = syn.make_surfels(P, 0)
    fp = syn.make_pose_sequence(n_keys, 0)
    full = fp["full_pose"]
    parms = {"betas": fp["betas"], "expression": fp["expression"], "global_orient": full[:, :3], "body_pose": full[:, 3:66],
             "jaw_pose": full[:, 66:69], "leye_pose": full[:, 69:72], "reye_pose": full[:, 72:75], "left_hand_pose": full[:, 75:120],
             "right_hand_pose": full[:, 120:165], "transl": fp["transl"]}
    guide = SMPLGuidance(syn.make_body_model(0), parms, device=dev)
    torch.manual_seed(11)
    lo, hi = surf.xyz.min(0)[0], surf.xyz.max(0)[0]
    c = (lo + hi) / 2
    field = HashMLPField(torch.stack([(lo - c) * 1.5 + c, (hi - c) * 1.5 + c]))
    sd = {"geometry._xyz": surf.xyz, "geometry._rotation": surf.rot, "geometry._colors": torch.logit(surf.colors.clamp(0.02, 0.98)),
          "geometry._occ": torch.logit(torch.rand(P, 1).clamp(0.02, 0.98)), "geometry._scaling": torch.log(surf.scales[:, :1])}
    sd.update({"geometry.attribute_field." + k: v for k, v in field.state_dict().items()})
    return pb.AvatarPlayer.from_checkpoint({"state_dict": sd}, guide)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--surfels", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, W, F, P = 1080, 1920, args.frames, args.surfels
    player = make_player(P, 4, dev)
    spec = syn.make_camera(W, H, distance=3.0, elevation=0.1, azimuth=0.4)
    cam = cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(dev), image_width=W, image_height=H,
                         world_view_transform=spec.world_view_transform.to(dev), full_proj_transform=spec.full_proj_transform.to(dev),
                         prcppoint=spec.prcppoint.to(dev))
    bg = torch.ones(3, device=dev)
    poses = player.turntable(n=F, frame=0)
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "frames": F, "surfels": P, "chunk": 8, "iters": args.iters}

    def playback():
        return {k: v.cpu() for k, v in player.render(poses, cam, bg=bg, chunk=8).items()}

    to_bytes = lambda x: x.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)

    def per_frame():
        out = {"rgb": [], "normal": [], "occ": [], "mask": []}
        with torch.no_grad():
            for i in range(F):
                o = player.renderer.forward(cam, bg, gt=True, gt_a_smpl=player.frame_pose(poses, i))
                for k, src in (("rgb", "render"), ("normal", "normal"), ("occ", "occ")):
                    out[k].append(to_bytes(torch.cat([o[src], o["mask"]], dim=0)).permute(1, 2, 0).cpu())
                out["mask"].append(to_bytes(o["mask"].clone())[0].cpu())
        return {k: torch.stack(v) for k, v in out.items()}

    # the two paths alternate, so that whatever else the host is doing falls on both
    for fn in (playback, per_frame, playback, per_frame):
        fn()
    torch.cuda.synchronize()
    ts = {playback: [], per_frame: []}
    for _ in range(args.iters):
        for fn in (playback, per_frame):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[fn].append((time.perf_counter() - t0) * 1e3)
    res["playback_ms"], res["playback_min_ms"] = statistics.median(ts[playback]), min(ts[playback])
    res["per_frame_forward_ms"], res["per_frame_forward_min_ms"] = statistics.median(ts[per_frame]), min(ts[per_frame])
    res["playback_all_ms"], res["per_frame_forward_all_ms"] = ts[playback], ts[per_frame]
    res["playback_ms_per_frame"] = res["playback_ms"] / F
    res["per_frame_forward_ms_per_frame"] = res["per_frame_forward_ms"] / F
    res["ratio_per_frame_over_playback"] = res["per_frame_forward_ms"] / res["playback_ms"]
    a, b = playback(), per_frame()
    res["bytes_equal_to_per_frame_path"] = all(torch.equal(a[k], b[k]) for k in a)
    res["mask_coverage"] = float((a["mask"] > 127).float().mean())

    # the kernels alone
    g = player.guidance.smpl_parms
    keys = player._keys_of(g)
    t = torch.linspace(0, keys[0].shape[0] - 1, F, device=dev)
    med, low = events(lambda: pb.motion_resample(keys[0], keys[1], keys[2], t), 20)
    res["motion_resample_ms"], res["motion_resample_min_ms"] = med, low
    B = 8
    imgs = [torch.rand(B, c, H, W, device=dev) for c in (3, 3, 1, 3)]
    out = pb.playback_finish(*imgs)
    REPEAT = 10

    def relaunch():
        for _ in range(REPEAT):
            pb.playback_finish(*imgs, out=out)

    med, low = events(relaunch, 20)
    nbytes = B * H * W * (40 + 13)
    res["finish_8_frames_ms"], res["finish_8_frames_min_ms"] = med / REPEAT, low / REPEAT
    res["finish_bytes"] = nbytes
    res["finish_bytes_per_s"] = nbytes / (res["finish_8_frames_ms"] * 1e-3)
    res["finish_share_of_8TBs_roofline"] = res["finish_bytes_per_s"] / HBM_ROOFLINE
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
