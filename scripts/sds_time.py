"""Time the SDS guidance's encoder and loss tail (soar_amd/sds.py) against the float32 torch restatement (tests/vae_ref.py, MIOpen
convolutions) on the same GPU at the workload's shape, [4,3,512,512] -> 256: the encoder's forward alone, and forward + backward
through MultiviewSDS with a trivial eps_fn (torch: the same chain through autograd), device events after warm-up.
-> profiles/sds_time.json.

``--trace CSV`` instead reads a rocprofv3 kernel trace of ``--trace-run`` (one forward + backward, repeated) and reports every
GEMM launch's time and achieved TFLOP/s, FLOPs from the shapes, against the 157.3 TFLOP/s f32 MFMA peak:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o sds -- python scripts/sds_time.py --trace-run
    python scripts/sds_time.py --trace OUT/.../sds_kernel_trace.csv
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import vae_ref as R  # noqa: E402

PEAK = 157.3e12
N, HW, S = 4, 512, 256


def gemm_flops(N, S):
    """(name, FLOPs) of the encoder's GEMM launches in forward order (2 per multiply-add), as vae.hip issues them"""
    out = []
    c, lev = 128, [S, S // 2, S // 4, S // 8]
    for i, m in enumerate(R.CH_MULT):
        s = lev[i]
        for j in range(2):
            co = 128 * m
            out.append((f"down{i}.block{j}.conv1", 2.0 * N * s * s * 9 * c * co))
            if c != co:
                out.append((f"down{i}.block{j}.nin", 2.0 * N * s * s * c * co))
            out.append((f"down{i}.block{j}.conv2", 2.0 * N * s * s * 9 * co * co))
            c = co
        if i < 3:
            out.append((f"down{i}.downsample", 2.0 * N * (s // 2) ** 2 * 9 * c * c))
    s, T = lev[3], lev[3] ** 2
    for b in ("mid.block_1",):
        out += [(b + ".conv1", 2.0 * N * T * 9 * c * c), (b + ".conv2", 2.0 * N * T * 9 * c * c)]
    out += [("attn.qkv", 2.0 * N * T * c * 3 * c), ("attn.qk", 2.0 * N * T * T * c), ("attn.pv", 2.0 * N * T * T * c),
            ("attn.proj", 2.0 * N * T * c * c)]
    out += [("mid.block_2.conv1", 2.0 * N * T * 9 * c * c), ("mid.block_2.conv2", 2.0 * N * T * 9 * c * c)]
    return out


def setup():
    from soar_amd import sds
    weights = R.random_weights(0)
    enc = sds.LatentEncoder(weights).to("cuda")
    m = sds.MultiviewSDS(enc, image_size=S).to("cuda")
    rgb = R.images(N, HW, HW, 1).cuda().permute(0, 2, 3, 1).contiguous()
    return weights, enc, m, rgb


def trivial_eps(x, t):
    return x * 0.9


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
    weights, enc, m, rgb = setup()
    w32 = R.cast(weights, torch.float32, "cuda")
    tb = {k: v.cuda() for k, v in R.tables(R.ldm_alphas_cumprod()).items()}
    x = rgb.clone().requires_grad_(True)
    eps = torch.randn(N, 4, S // 8, S // 8, device="cuda")
    noise = torch.randn_like(eps)
    t = torch.tensor([300], device="cuda")

    def hip_fwd():
        with torch.no_grad():
            enc(rgb.permute(0, 3, 1, 2), S, posterior_noise=eps)

    def t32_fwd():
        with torch.no_grad():
            R.latents(rgb.permute(0, 3, 1, 2), w32, S, eps)

    def hip_fb():
        x.grad = None
        m(x, trivial_eps, t=t, noise=noise, posterior_noise=eps)["loss_sds"].backward()

    def t32_fb():
        x.grad = None
        lat = R.latents(x.permute(0, 3, 1, 2), w32, S, eps)
        with torch.no_grad():
            x_in = R.q_sample(lat, t, noise, tb)
            e = trivial_eps(torch.cat([x_in, x_in]), t)
        _, _, dlat = R.loss_tail(lat, noise, e, t, tb, 5.0, 4, True, 0.2)
        lat.backward(dlat)

    res = {"device": torch.cuda.get_device_name(0), "shape": f"[{N},3,{HW},{HW}] -> {S}", "warmup": warmup, "iters": iters,
           "unit": "ms per call"}
    for k, f in (("hip_forward", hip_fwd), ("torch_f32_forward", t32_fwd), ("hip_forward_backward", hip_fb),
                 ("torch_f32_forward_backward", t32_fb)):
        res[k] = timed(f, warmup, iters)
        print(k, res[k], flush=True)
    fl = sum(f for _, f in gemm_flops(N, S))
    res["gemm_gflop_forward"] = fl / 1e9
    res["hip_forward_tflops"] = fl / (res["hip_forward"] * 1e-3) / 1e12
    res["hip_forward_backward_tflops"] = 2 * fl / (res["hip_forward_backward"] * 1e-3) / 1e12
    return res


def trace_run(iters=4):
    _, _, m, rgb = setup()
    for _ in range(iters):
        x = rgb.clone().requires_grad_(True)
        m(x, trivial_eps, t=torch.tensor([300], device="cuda"))["loss_sds"].backward()
    torch.cuda.synchronize()


def read_trace(path):
    """the forward GEMM launches of every iteration of trace_run, matched in order to gemm_flops"""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "conv_gemm_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = gemm_flops(N, S)
    nf = len(names)
    per = len(rows) // 4                       # forward + backward launches of one iteration
    out = []
    for j, (name, fl) in enumerate(names):
        ts = [(int(rows[it * per + j]["End_Timestamp"]) - int(rows[it * per + j]["Start_Timestamp"])) * 1e-9 for it in range(1, 4)]
        t = sorted(ts)[len(ts) // 2]
        out.append({"launch": j, "gemm": name, "us": t * 1e6, "tflops": fl / t / 1e12, "peak_share": fl / t / PEAK})
    total = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-9 for r in rows[per:2 * per]]
    return out, {"gemm_launches_per_iteration": per, "forward_gemms": nf, "gemm_ms_per_iteration": sum(total) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sds_time.json"))
    args = ap.parse_args()
    if args.trace_run:
        trace_run()
        return
    if args.trace:
        convs, summary = read_trace(args.trace)
        for c in convs:
            print(json.dumps(c))
        print(json.dumps(summary))
        d = json.load(open(args.out)) if os.path.exists(args.out) else {}
        d["gemm_launches_forward"] = convs
        d["trace_summary"] = summary
        json.dump(d, open(args.out, "w"), indent=1)
        return
    res = run_times(args.warmup, args.iters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
