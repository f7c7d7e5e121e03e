"""Time the SDS guidance's VAE encoder at its three precisions (soar_amd/sds.py LatentEncoder(precision=...)) at the
workload's shape, [4,3,512,512] -> 256: the encoder's forward alone, and forward + backward through MultiviewSDS with a trivial
eps_fn.  The precisions alternate call by call in one process, every call between its own pair of device events after a warm-up;
reported: the median of ``--iters`` (at least 7) calls with the fastest and the slowest.  Beside them the torch network
(tests/vae_ref.py on the device, MIOpen / hipBLASLt) in float32 and converted with ``.to(torch.bfloat16)`` / ``.half()``, weights
and activations alike, timed the same way.  -> profiles/sds_half_time.json.

``--tree DIR --only f32`` times another checkout of the project (the parent commit, which has no ``precision`` argument) through
this same script and stores it under ``"parent"``:

    python scripts/sds_half_time.py
    python scripts/sds_half_time.py --tree ../parent --only f32 --key parent

``--trace-run PREC`` is the program for one rocprofv3 kernel trace (forward + backward at one precision, repeated); ``--trace CSV
--key trace_PREC`` reads it and splits the device time of one iteration into the GEMM launches, GroupNorm and the rest:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o sds -- python scripts/sds_half_time.py --trace-run bf16
    python scripts/sds_half_time.py --trace OUT/.../sds_kernel_trace.csv --key trace_bf16
"""
import argparse
import csv
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HW, S = 4, 512, 256
PRECISIONS = ("f32", "bf16", "f16")
TRACE_ITERS = 4


def _tree():
    """--tree DIR, read before soar_amd is imported: the checkout whose package and restatement are timed"""
    for i, a in enumerate(sys.argv):
        if a == "--tree" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
    return HERE


ROOT = _tree()
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import vae_ref as R  # noqa: E402


def trivial_eps(x, t):
    return x * 0.9


def encoder(weights, precision):
    from soar_amd import sds
    # (a checkout from before the argument existed is float32 only)
    enc = sds.LatentEncoder(weights) if precision == "f32" else sds.LatentEncoder(weights, precision=precision)
    return enc.to("cuda")


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def alternate(fns, warmup, iters):
    """{name: fn} -> {name: {median, min, max}} in ms: the names in turn, call by call, ``iters`` rounds after ``warmup``"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            ms[k].append(event_ms(f))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}


def run_times(precisions, warmup, iters, with_torch):
    from soar_amd import sds
    weights = R.random_weights(0)
    rgb = R.images(N, HW, HW, 1).cuda().permute(0, 2, 3, 1).contiguous()
    eps = torch.randn(N, 4, S // 8, S // 8, device="cuda")
    noise = torch.randn_like(eps)
    t = torch.tensor([300], device="cuda")
    tb = {k: v.cuda() for k, v in R.tables(R.ldm_alphas_cumprod()).items()}
    x = rgb.clone().requires_grad_(True)
    fwd, fb, skipped = {}, {}, {}
    for p in precisions:
        enc = encoder(weights, p)
        m = sds.MultiviewSDS(enc, image_size=S).to("cuda")

        def hip_fwd(enc=enc):
            with torch.no_grad():
                enc(rgb.permute(0, 3, 1, 2), S, posterior_noise=eps)

        def hip_fb(m=m):
            x.grad = None
            m(x, trivial_eps, t=t, noise=noise, posterior_noise=eps)["loss_sds"].backward()

        fwd["hip_" + p], fb["hip_" + p] = hip_fwd, hip_fb
    if with_torch:
        for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
            w = R.cast(weights, dt, "cuda")
            xin, e_dt, n_dt = rgb.to(dt), eps.to(dt), noise.to(dt)
            xg = xin.clone().requires_grad_(True)
            tbd = {k: v.to(dt) for k, v in tb.items()}

            def t_fwd(w=w, xin=xin, e_dt=e_dt):
                with torch.no_grad():
                    R.latents(xin.permute(0, 3, 1, 2), w, S, e_dt)

            def t_fb(w=w, xg=xg, e_dt=e_dt, n_dt=n_dt, tbd=tbd):
                xg.grad = None
                lat = R.latents(xg.permute(0, 3, 1, 2), w, S, e_dt)
                with torch.no_grad():
                    x_in = R.q_sample(lat, t, n_dt, tbd)
                    e = trivial_eps(torch.cat([x_in, x_in]), t)
                _, _, dlat = R.loss_tail(lat, n_dt, e, t, tbd, 5.0, 4, True, 0.2)
                lat.backward(dlat)

            try:                                   # a type torch cannot run this chain in is reported, not fatal
                t_fwd()
                t_fb()
                torch.cuda.synchronize()
            except Exception as ex:  # noqa: BLE001
                skipped["torch_" + name] = f"{type(ex).__name__}: {ex}"[:300]
                continue
            print("torch_" + name, "ready", flush=True)
            fwd["torch_" + name], fb["torch_" + name] = t_fwd, t_fb
    res = {"device": torch.cuda.get_device_name(0), "shape": f"[{N},3,{HW},{HW}] -> {S}", "warmup": warmup, "iters": iters,
           "unit": "ms per call: median, min, max of device events; the entries of a block alternate call by call in one process"}
    if skipped:
        res["not_run"] = skipped
    res["forward"] = alternate(fwd, warmup, iters)
    res["forward_backward"] = alternate(fb, warmup, iters)
    for k in res["forward"]:
        print(k, "forward", res["forward"][k], "forward+backward", res["forward_backward"][k], flush=True)
    return res


def trace_run(precision):
    from soar_amd import sds
    weights = R.random_weights(0)
    m = sds.MultiviewSDS(encoder(weights, precision), image_size=S).to("cuda")
    rgb = R.images(N, HW, HW, 1).cuda().permute(0, 2, 3, 1).contiguous()
    for _ in range(TRACE_ITERS):
        x = rgb.clone().requires_grad_(True)
        m(x, trivial_eps, t=torch.tensor([300], device="cuda"))["loss_sds"].backward()
    torch.cuda.synchronize()


def read_trace(path):
    """the kernels of the last iteration of trace_run (from its vae_first_kernel on), summed by kind, in ms"""
    with open(path) as f:
        rows = [r for r in csv.DictReader(f)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "vae_first_kernel" in r["Kernel_Name"]]
    assert len(starts) >= TRACE_ITERS, f"expected {TRACE_ITERS} iterations in the trace, found {len(starts)}"
    it = rows[starts[-1]:]
    kinds = {"gemm_16bit": 0.0, "gemm_f32": 0.0, "groupnorm": 0.0, "rest": 0.0}
    counts = dict.fromkeys(kinds, 0)
    per_kernel = {}
    for r in it:
        name = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        kind = ("gemm_16bit" if "conv_gemm16_kernel" in name else "gemm_f32" if "conv_gemm_kernel" in name
                else "groupnorm" if "vae_gn_" in name else "rest")
        kinds[kind] += ms
        counts[kind] += 1
        short = name.replace("soar::(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
        per_kernel[short] = per_kernel.get(short, 0.0) + ms
    return {"unit": "ms of device time in one forward + backward, kernels summed (no gaps)", "by_kind_ms": kinds, "launches": counts,
            "total_ms": sum(kinds.values()), "by_kernel_ms": dict(sorted(per_kernel.items(), key=lambda kv: -kv[1]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--only", help="comma-separated precisions (default: all three and the torch network)")
    ap.add_argument("--key", help="store the result under this key of --out instead of replacing the file")
    ap.add_argument("--trace-run", metavar="PREC")
    ap.add_argument("--trace", metavar="CSV")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "sds_half_time.json"))
    args = ap.parse_args()
    if args.trace_run:
        trace_run(args.trace_run)
        return
    if args.iters < 7:
        ap.error("--iters must be at least 7")
    if args.trace:
        res = read_trace(args.trace)
    else:
        precisions = tuple(args.only.split(",")) if args.only else PRECISIONS
        res = run_times(precisions, args.warmup, args.iters, with_torch=not args.only)
    if args.key:
        d = json.load(open(args.out)) if os.path.exists(args.out) else {}
        d[args.key] = res
        res = d
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res if not args.key else res[args.key], indent=1))


if __name__ == "__main__":
    main()
