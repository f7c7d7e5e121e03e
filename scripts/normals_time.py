"""Time the normal networks (soar_amd/normals.py, csrc/normalnet.hip) at the shipped configuration (ngf 64, 4 levels, 9 blocks) with
random He-scaled weights at 512 x 512, N = 1 and N = 4, against the same network composed from torch-float32 (tests/normalnet_ref.py,
MIOpen convolutions) on the same GPU -> profiles/normals_time.json.

Per layer group (first layer, downs, trunk, ups, last layer): the torch path is timed with device events between the groups; the HIP
path is one C call, so its kernels' times are read from a torch.profiler trace and attributed by their order in the call.  The trunk
is also timed without a profiler, as the difference between the network with 9 and with 0 residual blocks, and reported in TFLOP/s
against the 157.3 TFLOP/s f32 MFMA peak.  Both generators run in every figure.
"""
import argparse
import gc
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import normalnet_ref as R  # noqa: E402
from soar_amd import normals  # noqa: E402

PEAK = 157.3e12
NGF, N_DOWN, N_BLOCKS = 64, 4, 9
GROUPS = ("first", "downs", "trunk", "ups", "last")


def device_weights(seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    layers = normals.layer_keys(NGF, N_DOWN, N_BLOCKS)
    first_up = 1 + N_DOWN + 2 * N_BLOCKS
    sd = {}
    for key, shape in normals.state_dict_layout(NGF, N_DOWN, N_BLOCKS).items():
        if key.endswith(".weight"):
            idx = [k for k, _ in layers].index(key.split(".model.")[1][:-len(".weight")])
            fan_in = shape[0] * 9 / 4.0 if first_up <= idx < first_up + N_DOWN else shape[1] * shape[2] * shape[3]
            sd[key] = torch.randn(shape, generator=g, device="cuda") * math.sqrt(2.0 / fan_in)
        else:
            sd[key] = torch.randn(shape, generator=g, device="cuda") * 0.1
    return sd


def without_trunk(sd):
    """the same checkpoint for n_blocks = 0: the layers behind the trunk move up by 9 indices"""
    out = {}
    for k, v in sd.items():
        net, rest = k.split(".model.")
        i = int(rest.split(".")[0])
        if 4 + 3 * N_DOWN <= i < 4 + 3 * N_DOWN + N_BLOCKS:
            continue
        j = i - N_BLOCKS if i >= 4 + 3 * N_DOWN + N_BLOCKS else i
        out[f"{net}.model.{j}.{rest.split('.', 1)[1]}"] = v
    return out


def flops(N, H, W):
    """FLOPs per group of ONE generator (2 per multiply-add)"""
    px = N * H * W
    f = {"first": 2.0 * px * 49 * 6 * NGF, "last": 2.0 * px * 49 * NGF * 3, "downs": 0.0, "ups": 0.0}
    for d in range(N_DOWN):
        c = NGF << d
        f["downs"] += 2.0 * (px >> (2 * (d + 1))) * 9 * c * 2 * c
        f["ups"] += 2.0 * (px >> (2 * (d + 1))) * 9 * 2 * c * c        # 9 taps per input pixel = 9 / 4 per output pixel
    ct = NGF << N_DOWN
    f["trunk"] = 2.0 * (px >> (2 * N_DOWN)) * 9 * ct * ct * 2 * N_BLOCKS
    return f


def timed(fn, warmup, iters):
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
    return sorted(ts)[len(ts) // 2]


def torch_groups(x, sd, net, marks):
    """ref.generator with an event after every group"""
    layers = normals.layer_keys(NGF, N_DOWN, N_BLOCKS)
    get = lambda i, what: sd[f"{net}.model.{layers[i][0]}.{what}"]
    inorm = lambda t: F.instance_norm(t, eps=1e-5)
    mark = lambda: marks.append(torch.cuda.Event(enable_timing=True)) or marks[-1].record()
    li = 0
    mark()
    x = F.relu(inorm(F.conv2d(F.pad(x, (3, 3, 3, 3), mode="reflect"), get(li, "weight"), get(li, "bias"))))
    li += 1
    mark()
    for _ in range(N_DOWN):
        x = F.relu(inorm(F.conv2d(x, get(li, "weight"), get(li, "bias"), stride=2, padding=1)))
        li += 1
    mark()
    for _ in range(N_BLOCKS):
        y = F.relu(inorm(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), get(li, "weight"), get(li, "bias"))))
        x = x + inorm(F.conv2d(F.pad(y, (1, 1, 1, 1), mode="reflect"), get(li + 1, "weight"), get(li + 1, "bias")))
        li += 2
    mark()
    for _ in range(N_DOWN):
        x = F.relu(inorm(F.conv_transpose2d(x, get(li, "weight"), get(li, "bias"), stride=2, padding=1, output_padding=1)))
        li += 1
    mark()
    x = torch.tanh(F.conv2d(F.pad(x, (3, 3, 3, 3), mode="reflect"), get(li, "weight"), get(li, "bias")))
    mark()
    return x


def hip_kernel_groups(net, inputs, iters):
    """ms per group and call from a profiler trace: the kernels of one generator come as first, 3 IN, then per convolution the GEMM
    and 3 IN launches, last"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            net(*inputs)
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    evs = [e for e in evs if any(k in e.name for k in ("nn_first", "conv_gemm_kernel", "nn_in_", "nn_last"))]
    evs.sort(key=lambda e: e.time_range.start)
    per_gen = 1 + 3 + 4 * (2 * N_DOWN + 2 * N_BLOCKS) + 1
    if len(evs) != per_gen * 2 * iters:
        return {"error": f"expected {per_gen * 2 * iters} kernel records, the trace holds {len(evs)}"}
    order = ["first"] * 4 + ["downs"] * (4 * N_DOWN) + ["trunk"] * (8 * N_BLOCKS) + ["ups"] * (4 * N_DOWN) + ["last"]
    out = {g: 0.0 for g in GROUPS}
    out["trunk_gemm_only"] = 0.0
    for i, e in enumerate(evs):
        dur = (e.time_range.end - e.time_range.start) * 1e-3 / iters
        out[order[i % per_gen]] += dur
        if order[i % per_gen] == "trunk" and "conv_gemm_kernel" in e.name:
            out["trunk_gemm_only"] += dur
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_time.json"))
    args = ap.parse_args()
    sd = device_weights()
    net = normals.NormalNet(sd, NGF, N_DOWN, N_BLOCKS).to("cuda")
    net0 = normals.NormalNet(without_trunk(sd), NGF, N_DOWN, 0).to("cuda")
    res = {"device": torch.cuda.get_device_name(0), "config": [NGF, N_DOWN, N_BLOCKS], "warmup": args.warmup, "iters": args.iters,
           "unit": "ms per call of both generators (median)", "f32_mfma_peak_tflops": PEAK / 1e12, "shapes": {}}
    gc.collect()
    gc.freeze()
    gc.disable()
    for N in (1, 4):
        inputs = [t.cuda() for t in R.make_inputs(N, 512, 512, 7)]
        fl = flops(N, 512, 512)
        row = {"gflop_per_generator": {g: fl[g] / 1e9 for g in GROUPS}}
        with torch.no_grad():
            row["hip"] = timed(lambda: net(*inputs), args.warmup, args.iters)
            row["hip_without_trunk"] = timed(lambda: net0(*inputs), args.warmup, args.iters)
            row["hip_trunk_by_difference"] = row["hip"] - row["hip_without_trunk"]
            row["hip_trunk_tflops"] = 2 * fl["trunk"] / (row["hip_trunk_by_difference"] * 1e-3) / 1e12
            row["hip_trunk_peak_share"] = row["hip_trunk_tflops"] * 1e12 / PEAK
            row["hip_groups"] = hip_kernel_groups(net, inputs, 3)
            if "trunk_gemm_only" in row["hip_groups"]:
                row["hip_trunk_gemm_tflops"] = 2 * fl["trunk"] / (row["hip_groups"]["trunk_gemm_only"] * 1e-3) / 1e12

            def t32():
                marks = []
                a = torch_groups(torch.cat([inputs[0], inputs[1]], 1), sd, "netF", marks)
                b = torch_groups(torch.cat([inputs[0], inputs[2]], 1), sd, "netB", marks)
                return a, b, marks
            row["torch_f32"] = timed(t32, args.warmup, args.iters)
            acc = {g: [] for g in GROUPS}
            for _ in range(args.iters):
                _, _, marks = t32()
                torch.cuda.synchronize()
                for gi, g in enumerate(GROUPS):
                    acc[g].append(marks[gi].elapsed_time(marks[gi + 1]) + marks[6 + gi].elapsed_time(marks[7 + gi]))
            row["torch_f32_groups"] = {g: sorted(v)[len(v) // 2] for g, v in acc.items()}
            row["torch_f32_trunk_tflops"] = 2 * fl["trunk"] / (row["torch_f32_groups"]["trunk"] * 1e-3) / 1e12
            hF, hB = net(*inputs)
            tF, tB, _, _ = R.normalnet(*inputs, sd, NGF, N_DOWN, N_BLOCKS, dtype=torch.float32)
            row["distance_hip_to_torch_f32"] = {"worst_element": max((hF - tF).abs().max().item(), (hB - tB).abs().max().item()),
                                                "relative_l2": (torch.norm(hF - tF) / torch.norm(tF)).item()}
        res["shapes"][f"[{N},3,512,512]"] = row
        print(N, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
