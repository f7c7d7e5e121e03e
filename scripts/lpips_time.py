"""Time LPIPS-VGG (soar_amd/lpips.py) against the float32 torch restatement (tests/lpips_ref.py, MIOpen convolutions) on the same
GPU: [1,3,512,512] and [2,3,512,512], forward only and forward + backward with respect to in0, device events after warm-up.
-> profiles/lpips_time.json.

``--trace CSV`` instead reads a rocprofv3 kernel trace of ``--trace-run`` (N = 1 at 512 x 512, forward + backward, repeated) and
reports every convolution launch's time and achieved TFLOP/s, FLOPs from the shapes, against the 157.3 TFLOP/s f32 MFMA peak:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o lpips -- python scripts/lpips_time.py --trace-run
    python scripts/lpips_time.py --trace OUT/.../lpips_kernel_trace.csv
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import lpips_ref as R  # noqa: E402

PEAK = 157.3e12
LEVEL = [0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]


def conv_flops(N, H, W):
    """FLOPs of the 13 convolutions (2 per multiply-add) at N x H x W"""
    out = []
    for i, (cin, cout) in enumerate(R.CONV_CH):
        h, w = H, W
        for _ in range(LEVEL[i]):
            h, w = h // 2, w // 2
        out.append(2.0 * N * h * w * 9 * cin * cout)
    return out


def model():
    from soar_amd.lpips import LPIPSVGG
    return LPIPSVGG(R.lpips_state_dict(R.random_weights(0))).to("cuda")


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def run_times(warmup, iters):
    m = model()
    w32 = R.weights_of(m, torch.float32)
    res = {"device": torch.cuda.get_device_name(0), "warmup": warmup, "iters": iters, "unit": "ms per call", "shapes": {}}
    for N in (1, 2):
        a = R.normal_images(N, 512, 512, 1).cuda()
        b = (a + 0.3 * R.normal_images(N, 512, 512, 2).cuda()).clamp(-1, 1)
        x = a.clone().requires_grad_(True)

        def hip_fwd():
            with torch.no_grad():
                m(a, b)

        def hip_fb():
            x.grad = None
            m(x, b).sum().backward()

        def t32_fwd():
            with torch.no_grad():
                R.lpips(a, b, w32)

        def t32_fb():
            x.grad = None
            R.lpips(x, b, w32).sum().backward()

        row = {k: timed(f, warmup, iters) for k, f in
               (("hip_forward", hip_fwd), ("torch_f32_forward", t32_fwd), ("hip_forward_backward", hip_fb),
                ("torch_f32_forward_backward", t32_fb))}
        fl = sum(conv_flops(N, 512, 512))
        row["conv_gflop_forward_both_inputs"] = 2 * fl / 1e9
        row["conv_gflop_forward_backward"] = (2 * fl + fl) / 1e9
        row["hip_forward_tflops"] = 2 * fl / (row["hip_forward"] * 1e-3) / 1e12
        row["hip_forward_backward_tflops"] = 3 * fl / (row["hip_forward_backward"] * 1e-3) / 1e12
        res["shapes"][f"[{N},3,512,512]"] = row
        print(N, json.dumps(row), flush=True)
    return res


def trace_run(iters=6):
    m = model()
    a = R.normal_images(1, 512, 512, 1).cuda()
    b = (a + 0.3 * R.normal_images(1, 512, 512, 2).cuda()).clamp(-1, 1)
    for _ in range(iters):
        x = a.clone().requires_grad_(True)
        m(x, b).sum().backward()
    torch.cuda.synchronize()


def read_trace(path):
    """conv launches of trace_run in order: per iteration 24 forward (layers 1..12, in0 then in1) and 12 backward (12..1)"""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "lpips_conv_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = 36
    n_it = len(rows) // per
    fl = conv_flops(1, 512, 512)
    out = []
    for j in range(per):
        layer = 1 + j // 2 if j < 24 else 12 - (j - 24)
        ts = [(int(rows[it * per + j]["End_Timestamp"]) - int(rows[it * per + j]["Start_Timestamp"])) * 1e-9 for it in range(1, n_it)]
        t = sorted(ts)[len(ts) // 2]
        kind = "forward" if j < 24 else "data-gradient"
        out.append({"launch": j, "layer": layer, "kind": kind, "K": 9 * (R.CONV_CH[layer][0] if kind == "forward" else R.CONV_CH[layer][1]),
                    "us": t * 1e6, "tflops": fl[layer] / t / 1e12, "peak_share": fl[layer] / t / PEAK,
                    "kernel": rows[j]["Kernel_Name"][:60]})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_time.json"))
    args = ap.parse_args()
    if args.trace_run:
        trace_run()
        return
    if args.trace:
        convs = read_trace(args.trace)
        for c in convs:
            print(json.dumps(c))
        d = json.load(open(args.out)) if os.path.exists(args.out) else {}
        d["conv_launches_1x512x512"] = convs
        json.dump(d, open(args.out, "w"), indent=1)
        return
    res = run_times(args.warmup, args.iters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
