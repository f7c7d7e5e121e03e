"""Time the body keypoint stage (soar_amd/pose.py, csrc/pose.hip) at the shipped BODY_25 shapes with seeded random weights on
1080 x 1920 frames (net input 368 x 656), one frame and a chunk of 8 -> profiles/pose_time.json.

* ``preprocess``, ``forward``, ``pose_peaks``, ``pose_assemble`` and the whole ``detect``: medians of ``--iters`` (at least 7) with the
  spread (min, max), device events round each call.
* ``forward`` against the same network in torch float32 on the same GPU (tests/pose_ref.py's module, MIOpen convolutions).
* The post-processing against the restatement on the host (NumPy, tests/pose_ref.py): on the random net's maps, which fill every
  part's 32 peak slots (the worst case), and on a constructed scene of two people at the same map size (what a frame looks like).
* How far a frame fills the chip: the workgroups of every stage convolution at one frame and at eight (the launcher's tile rule
  restated), and the measured time per frame of ``forward`` at both.
* ``--slope-ab parent.json new.json [parent2.json new2.json ...]``: what ``scripts/normals_time.py`` measured in the same session with
  the parent commit's library and with this one (the ``slope`` field of the shared GEMM's descriptor must cost its callers nothing):
  both numbers per shape and the session's spread, copied into the same JSON.  ``--ab-only`` takes the pairs into the JSON that
  is already there (a second session of A/B runs; the one before is kept under ``..._earlier``) and measures nothing else.
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

import pose_ref as R  # noqa: E402
from soar_amd import pose  # noqa: E402

CUS = 256


def device_weights(cfg, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sd = {}
    for conv, prelu, shape in pose.layer_keys(cfg):
        fan_in = shape[1] * shape[2] * shape[3]
        sd[f"{conv}.weight"] = torch.randn(shape, generator=g, device="cuda") * math.sqrt(2.0 / fan_in)
        sd[f"{conv}.bias"] = torch.randn(shape[0], generator=g, device="cuda") * 0.1
        if prelu:
            sd[f"{prelu}.weight"] = torch.rand(shape[0], generator=g, device="cuda") * 0.8 - 0.2
    return sd


def timed(fn, warmup, iters):
    """-> dict(median, min, max) in ms"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def host_timed(fn, iters):
    """-> (dict(median, min, max, iters) in ms, what the last call returned)"""
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "iters": iters}, out


def workgroups(rows, cout):
    """csrc/conv_gemm.hip conv_gemm_tile, restated: 128 x 128 tiles where those still fill the chip, else 64 x 64 -> (tile, workgroups)"""
    big = math.ceil(rows / 128) * math.ceil(cout / 128)
    if big >= 256 and cout >= 128:
        return 128, big
    return 64, math.ceil(rows / 64) * math.ceil(cout / 64)


def fill_table(cfg, h, w):
    out = {}
    for B in (1, 8):
        rows = B * h * w
        table = {}
        for name, cout in (("block 3x3, stage 0", cfg["w0"]), ("block 3x3, later stages", cfg["w1"]), ("1x1, stage 0", cfg["m0"]),
                           ("1x1, later stages", cfg["m1"]), ("maps: PAF", 56), ("maps: heat", 32)):
            tile, n = workgroups(rows, cout)
            table[name] = {"tile": tile, "workgroups": n, "per_compute_unit": n / CUS}
        out[f"B={B}"] = {"rows": rows, "row_tiles_of_64": math.ceil(rows / 64), "convolutions": table}
    return out


def post_processing(heat, paf, warmup, iters, host_iters):
    """GPU and host times of the two post-processing steps over maps [B,h,w,*] on the device"""
    peaks, counts = pose.pose_peaks(heat)
    row = {"peaks_found_per_part_mean": float(counts[:, :25].float().mean()), "peaks_kept_per_part_mean": float(counts[:, :25].clamp(max=32).float().mean()),
           "pose_peaks": timed(lambda: pose.pose_peaks(heat), warmup, iters),
           "pose_assemble": timed(lambda: pose.pose_assemble(peaks, counts, paf), warmup, iters)}
    row["n_people"] = pose.pose_assemble(peaks, counts, paf)[1].tolist()
    if host_iters:
        h0, f0 = heat[0].cpu().numpy(), paf[0].cpu().numpy()
        t_peaks, (p0, c0) = host_timed(lambda: R.peaks_ref(h0), host_iters)
        t_asm, (a0, _) = host_timed(lambda: R.assemble_ref(p0, c0, f0), host_iters)
        got = pose.pose_assemble(peaks[:1], counts[:1], paf[:1])
        row["host_one_frame"] = {"peaks_ref": t_peaks, "assemble_ref": t_asm,
                                 "bit_equal": bool(np.array_equal(peaks[0].cpu().numpy().view(np.int32), p0.view(np.int32))
                                                   and np.array_equal(got[0][0].cpu().numpy().view(np.int32), a0.view(np.int32)))}
    return row


def slope_ab(pairs, note):
    runs = [(json.load(open(a)), json.load(open(b))) for a, b in zip(pairs[::2], pairs[1::2])]
    ab = {"script": "scripts/normals_time.py", "unit": "ms per call of both generators (median of its iterations); one entry per run of the session",
          "order_of_runs": note, "shapes": {}}
    for shape in runs[0][0]["shapes"]:
        parent = [r[0]["shapes"][shape]["hip"] for r in runs]
        new = [r[1]["shapes"][shape]["hip"] for r in runs]
        spread = max(max(parent) - min(parent), max(new) - min(new))
        diff = sum(new) / len(new) - sum(parent) / len(parent)
        ab["shapes"][shape] = {"parent_library": parent, "this_library": new, "session_spread": spread, "difference_of_means": diff,
                               "unchanged_within_spread": abs(diff) <= spread}
    return ab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--slope-ab", nargs="*", default=[])
    ap.add_argument("--ab-only", action="store_true")
    ap.add_argument("--ab-order", default="parent, then this library, in every round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_time.json"))
    args = ap.parse_args()
    if args.iters < 7:
        ap.error("--iters must be at least 7")
    if len(args.slope_ab) % 2:
        ap.error("--slope-ab takes pairs: parent.json new.json ...")
    if args.ab_only:
        res = json.load(open(args.out))
        if "shared_gemm_slope_field_ab" in res:
            res["shared_gemm_slope_field_ab_earlier"] = res["shared_gemm_slope_field_ab"]
        res["shared_gemm_slope_field_ab"] = slope_ab(args.slope_ab, args.ab_order)
        json.dump(res, open(args.out, "w"), indent=1)
        return
    cfg = R.SHIPPED
    sd = device_weights(cfg)
    net = pose.PoseNet(sd).to("cuda")
    ref = R.RefNet(sd).to("cuda")
    H, W = 1080, 1920
    nh, nw = pose.net_size(H, W, 368)
    h, w = nh // 8, nw // 8
    res = {"device": torch.cuda.get_device_name(0), "config": cfg, "frames": [H, W], "net_input": [nh, nw], "maps": [h, w],
           "warmup": args.warmup, "iters": args.iters, "unit": "ms per call: median, min, max", "compute_units": CUS,
           "chip_fill": fill_table(cfg, h, w), "shapes": {}}
    gc.collect()
    gc.freeze()
    gc.disable()
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for B in (1, 8):
            img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
            x = net.preprocess(img, 368)
            heat, paf = net(x)
            row = {"preprocess": timed(lambda: net.preprocess(img, 368), args.warmup, args.iters),
                   "forward": timed(lambda: net(x), args.warmup, args.iters),
                   "detect": timed(lambda: pose.detect(net, img), args.warmup, args.iters)}
            xc = x.contiguous()
            row["torch_f32_forward"] = timed(lambda: ref(xc), args.warmup, args.iters)
            _, stages = ref(xc)
            t_heat = stages[-1].permute(0, 2, 3, 1)
            row["distance_hip_to_torch_f32"] = {"worst_element": (heat - t_heat).abs().max().item(),
                                                "relative_l2": (torch.norm(heat - t_heat) / torch.norm(t_heat)).item()}
            row["forward_ms_per_frame"] = row["forward"]["median"] / B
            row["forward_slower_than_torch"] = row["forward"]["median"] > row["torch_f32_forward"]["median"]
            row["random_maps"] = post_processing(heat, paf, args.warmup, args.iters, 1 if B == 1 else 0)     # (the host takes seconds here)
            people = [R.person(200.4, 180.6, {k: (1.8 * dx, 1.8 * dy) for k, (dx, dy) in R.TEMPLATE.items()}),
                      R.person(420.7, 190.3, {k: (1.8 * dx, 1.8 * dy) for k, (dx, dy) in R.TEMPLATE.items()})]
            s_heat, s_paf, _ = R.scene(h, w, people)
            row["two_person_scene"] = post_processing(torch.from_numpy(s_heat).cuda()[None].expand(B, -1, -1, -1).contiguous(),
                                                      torch.from_numpy(s_paf).cuda()[None].expand(B, -1, -1, -1).contiguous(),
                                                      args.warmup, args.iters, args.host_iters if B == 1 else 0)
            res["shapes"][f"B={B}"] = row
            print(B, json.dumps(row), flush=True)
    one, eight = res["shapes"]["B=1"]["forward_ms_per_frame"], res["shapes"]["B=8"]["forward_ms_per_frame"]
    res["forward_per_frame_one_over_eight"] = one / eight
    if args.slope_ab:
        res["shared_gemm_slope_field_ab"] = slope_ab(args.slope_ab, args.ab_order)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
