"""Time the hand and face keypoint stage (soar_amd/pose_parts.py, csrc/pose_parts.hip) at the released shapes (VGG-19's front widths,
6 stages, 22 / 71 maps, crops of 368 x 368) with seeded random weights on 8 frames of 1080 x 1920 -> profiles/pose_parts_time.json.

* ``CpmNet.forward`` on 16 hand crops and on 8 face crops against the same networks in torch float32 on the same GPU
  (tests/pose_parts_ref.py's module with one ``F.conv2d`` per layer, MIOpen convolutions).
* The rectangle, crop and keypoint launches against the NumPy restatement on the host (tests/pose_parts_ref.py).
* ``pose.detect_sequence`` with the part networks against the same call without them (the BODY_25 network at its shipped shapes).

Medians of ``--iters`` (at least 7) with the spread (min, max); device events round each device call.
"""
import argparse
import gc
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pose_parts_ref as R  # noqa: E402
import pose_ref  # noqa: E402
from pose_time import device_weights as body_weights, host_timed, timed  # noqa: E402
from soar_amd import pose, pose_parts  # noqa: E402


def device_weights(cfg, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for name, shape in pose_parts.layer_keys(cfg):
        fan_in = shape[1] * shape[2] * shape[3]
        sd[f"{name}.weight"] = torch.randn(shape, generator=g, device="cuda") * math.sqrt(2.0 / fan_in)
        sd[f"{name}.bias"] = torch.randn(shape[0], generator=g, device="cuda") * 0.1
    return sd


def wall_timed(fn, iters):
    """host wall clock round a call that ends with a copy to the host -> dict(median, min, max) in ms"""
    fn()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def standing_people(B, H, W):
    """one person per frame, arms and head where the rules accept them, shifted from frame to frame"""
    J = np.zeros((25, 3), np.float32)
    for j, xy in {1: (960, 330), 0: (960, 240), 15: (930, 220), 16: (990, 220), 17: (900, 235), 18: (1020, 235), 2: (820, 340), 3: (760, 520),
                  4: (730, 690), 5: (1100, 340), 6: (1160, 520), 7: (1190, 690)}.items():
        J[j] = (*xy, 0.9)
    people = np.zeros((B, 8, 25, 3), np.float32)
    people[:, 0] = J
    people[:, 0, :, 0] += 40 * np.arange(B, dtype=np.float32)[:, None]
    return torch.from_numpy(people).cuda(), torch.ones(B, dtype=torch.int32).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_parts_time.json"))
    args = ap.parse_args()
    if args.iters < 7:
        ap.error("--iters must be at least 7")
    B, H, W, S = 8, 1080, 1920, 368
    res = {"device": torch.cuda.get_device_name(0), "frames": [B, H, W], "net_side": S, "warmup": args.warmup, "iters": args.iters,
           "unit": "ms per call: median, min, max", "networks": {}}
    gc.collect()
    gc.freeze()
    gc.disable()
    g = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    people, n_people = standing_people(B, H, W)
    nets = {}
    with torch.no_grad():
        boxes = pose_parts.part_boxes(people, n_people)
        xh, xf = pose_parts.crop_parts(img, boxes, S)
        assert bool(boxes[..., 3].all())
        for name, cfg, x in (("hand", R.SHIPPED_HAND, xh), ("face", R.SHIPPED_FACE, xf)):
            sd = device_weights(cfg)
            net = nets[name] = pose_parts.CpmNet(sd).to("cuda")
            ref = R.RefCpmNet(sd, rowwise=False).to("cuda")
            row = {"crops": x.shape[0], "config": {k: cfg[k] for k in ("n_stages", "n_maps")},
                   "forward": timed(lambda: net(x), args.warmup, args.iters),
                   "torch_f32_forward": timed(lambda: ref(x), args.warmup, args.iters)}
            heat, t_heat = net(x), ref(x)[1][-1].permute(0, 2, 3, 1)
            row["distance_hip_to_torch_f32"] = {"worst_element": (heat - t_heat).abs().max().item(),
                                                "relative_l2": (torch.norm(heat - t_heat) / torch.norm(t_heat)).item()}
            row["forward_slower_than_torch"] = row["forward"]["median"] > row["torch_f32_forward"]["median"]
            res["networks"][name] = row
            print(name, json.dumps(row), flush=True)
            del ref, t_heat
        # the three part launches against the restatement on the host
        heat_h, heat_f = nets["hand"](xh), nets["face"](xf)
        dev = {"part_boxes": timed(lambda: pose_parts.part_boxes(people, n_people), args.warmup, args.iters),
               "crop_parts": timed(lambda: pose_parts.crop_parts(img, boxes, S), args.warmup, args.iters),
               "part_keypoints_hands": timed(lambda: pose_parts.part_keypoints(heat_h, boxes, "hands", S), args.warmup, args.iters),
               "part_keypoints_face": timed(lambda: pose_parts.part_keypoints(heat_f, boxes, "face", S), args.warmup, args.iters)}
        p_np, n_np, img_np, b_np = people.cpu().numpy(), n_people.cpu().numpy(), img.cpu().numpy(), boxes.cpu().numpy()
        hh_np, hf_np = heat_h.cpu().numpy(), heat_f.cpu().numpy()
        host = {}
        host["part_boxes"], b_ref = host_timed(lambda: R.boxes_ref(p_np, n_np), args.host_iters)
        host["crop_parts"], (ch_ref, cf_ref) = host_timed(lambda: R.crop_ref(img_np, b_np, S), args.host_iters)
        host["part_keypoints_hands"], kh_ref = host_timed(lambda: R.keypoints_ref(hh_np, b_np, "hands"), args.host_iters)
        host["part_keypoints_face"], kf_ref = host_timed(lambda: R.keypoints_ref(hf_np, b_np, "face"), args.host_iters)
        same = lambda a, b: bool(np.array_equal(a.cpu().numpy().view(np.int32), b.view(np.int32)))
        res["part_launches"] = {"device": dev, "host_numpy": host, "bit_equal": {
            "part_boxes": same(boxes, b_ref), "crop_parts": same(xh, ch_ref) and same(xf, cf_ref),
            "part_keypoints_hands": same(pose_parts.part_keypoints(heat_h, boxes, "hands", S), kh_ref),
            "part_keypoints_face": same(pose_parts.part_keypoints(heat_f, boxes, "face", S), kf_ref)}}
        print("part launches", json.dumps(res["part_launches"]), flush=True)
        del heat_h, heat_f, xh, xf
        # the sequence with and without the part networks
        body = pose.PoseNet(body_weights(pose_ref.SHIPPED)).to("cuda")
        seq = {"body_only": wall_timed(lambda: pose.detect_sequence(body, img, chunk=B), args.iters),
               "with_hand_and_face": wall_timed(lambda: pose.detect_sequence(body, img, chunk=B, hand_net=nets["hand"], face_net=nets["face"]),
                                                args.iters)}
        seq["added_ms_per_frame"] = (seq["with_hand_and_face"]["median"] - seq["body_only"]["median"]) / B
        seq["note"] = "host wall clock round the call, the copy of the result to the host included; a random body net finds whom it finds"
        res["detect_sequence_8_frames"] = seq
        print("sequence", json.dumps(seq), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
