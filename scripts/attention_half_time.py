"""Time the 16-bit matrix-core attention (csrc/attention.hip kv_attn16_kernel) and the networks that can switch it on,
at the shipped shapes with seeded random weights -> profiles/attention_half_time.json.

Reported, the variants of a table alternating call by call in one process, medians of 15 device-event times with the fastest and
slowest beside them:
  * the kernel alone at float32 / bf16 / f16 -- the UNet's level-0 self-attention (2 x 4096 tokens, 5 heads of 64), its cross-attention
    (8 x 1024 queries over 77 + 16 tokens) and ViT-H/14's 257 tokens at 16 heads of 80 -- each against torch's
    ``scaled_dot_product_attention`` on tensors of the same dtype, with TFLOP/s (4 Lq Lk hd per head and batch entry);
  * one UNet ``forward`` at (precision, attention_precision) = (f32, f32), (bf16, f32), (bf16, bf16);
  * ``ImageTokens``, the ViT-H/14 encoder at one and four images and the text encoder at 2 x 77 at the same three pairs, against the
    torch composition of tests/clip_ref.py converted with ``.to(torch.bfloat16)``.

``--root TREE`` imports ``soar_amd`` from another checkout (built there) and times what that tree has -- with the parent commit's tree
the UNet at (f32, f32) and (bf16, f32) and the conditioning at f32 -- into ``--out``; ``--parent FILE...`` copies such runs' results
into the output.  ``--yardstick`` times this tree exactly as a ``--root`` run times the parent (the same configurations alternating in
a process of their own: how many networks share the caches moves a median by more than the code does) and ``--this FILE...`` copies
those in too, so that the default path can be held against the parent's like for like in one session.
"""
import argparse
import gc
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--root", default=ROOT, help="the checkout whose soar_amd is timed")
    ap.add_argument("--parent", nargs="*", default=[], help="results of --root runs over the parent commit")
    ap.add_argument("--yardstick", action="store_true", help="time only what the parent commit has, as a --root run of it does")
    ap.add_argument("--this", nargs="*", default=[], help="results of --yardstick runs of this tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_half_time.json"))
    return ap.parse_args()


ARGS = _args()
sys.path[:0] = [os.path.abspath(ARGS.root), os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import clip_ref as CR  # noqa: E402
import unet_ref as UR  # noqa: E402
from soar_amd import clip, unet  # noqa: E402
import clip_time as CT  # noqa: E402
from unet_time import SHIPPED, device_weights  # noqa: E402

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
PAIRS = [("f32", "f32"), ("bf16", "f32"), ("bf16", "bf16")]
HAS16 = "attention_precision" in inspect.signature(unet.MultiviewUNet.__init__).parameters and not ARGS.yardstick
CLIP16 = "precision" in inspect.signature(clip.ClipImageEncoder.__init__).parameters and not ARGS.yardstick


def stats(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def once(fn, reps=1):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def alternating(fns, warmup, iters, reps=1):
    """{name: fn} -> {name: stats}: every round times each fn once, so a drift of the machine falls on all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ts[k].append(once(fn, reps))
    return {k: stats(v) for k, v in ts.items()}


def label(p, a):
    return f"{p}/{a}"


def kernel_alone(name, B, Lq, Lk, heads, hd, Lk2, fn, warmup, iters):
    g = torch.Generator(device="cuda").manual_seed(Lq + Lk)
    C = heads * hd
    q, k, v = (torch.randn(B, L, C, device="cuda", generator=g) for L in (Lq, Lk, Lk))
    extra = {}
    if Lk2:
        extra = dict(k2=torch.randn(B, Lk2, C, device="cuda", generator=g), v2=torch.randn(B, Lk2, C, device="cuda", generator=g), w2=1.0)
    sp = lambda t, dt: t.to(dt).reshape(B, -1, heads, hd).transpose(1, 2).contiguous()
    fns = {p: (lambda p=p: fn(q, k, v, heads, precision=p, **extra)) for p in DTYPES}
    for p, dt in DTYPES.items():
        qs, ks, vs = sp(q, dt), sp(k, dt), sp(v, dt)
        if Lk2:
            k2s, v2s = sp(extra["k2"], dt), sp(extra["v2"], dt)
            fns["torch_sdpa_" + p] = lambda qs=qs, ks=ks, vs=vs, k2s=k2s, v2s=v2s: (F.scaled_dot_product_attention(qs, ks, vs) +
                                                                                   F.scaled_dot_product_attention(qs, k2s, v2s))
        else:
            fns["torch_sdpa_" + p] = lambda qs=qs, ks=ks, vs=vs: F.scaled_dot_product_attention(qs, ks, vs)
    gflop = 4.0 * B * heads * Lq * (Lk + Lk2) * hd / 1e9
    ms = alternating(fns, warmup, iters, reps=10)
    out = {"name": name, "B": B, "Lq": Lq, "Lk": Lk, "Lk2": Lk2, "heads": heads, "hd": hd, "gflop": gflop, "ms": ms,
           "tflops": {k_: gflop / v_["median"] for k_, v_ in ms.items()}}
    ref = fns["f32"]()
    rms = ref.pow(2).mean().sqrt()
    out["distance_to_hip_f32_worst_over_rms"] = {p: ((fns[p]() - ref).abs().max() / rms).item() for p in ("bf16", "f16")}
    return out


def unet_section(res, warmup, iters):
    cfg = SHIPPED
    sd = device_weights(cfg)
    kw = dict(num_head_channels=64, ip_dim=16, n_view=4)
    pairs = PAIRS if HAS16 else PAIRS[:2]
    nets = {label(p, a): unet.MultiviewUNet(sd, precision=p, **(dict(attention_precision=a) if HAS16 else {}), **kw).to("cuda") for p, a in pairs}
    x, t, ctx, cam, ip = (v.cuda() for v in UR.inputs(cfg, 0))
    t = t[::4].repeat_interleave(4)
    fwd = alternating({k: (lambda n=n: n(x, t, ctx, camera=cam, ip_tokens=ip)) for k, n in nets.items()}, warmup, iters)
    res["unet_forward"] = fwd
    if HAS16:
        eps = {k: n(x, t, ctx, camera=cam, ip_tokens=ip) for k, n in nets.items()}
        rms = eps["f32/f32"].pow(2).mean().sqrt()
        res["unet_distance_to_f32_worst_over_rms"] = {k: ((e - eps["f32/f32"]).abs().max() / rms).item() for k, e in eps.items() if k != "f32/f32"}
    del nets, sd
    torch.cuda.empty_cache()


def clip_section(res, warmup, iters):
    vsd, tsd, rsd = (CT.device_weights(CR.vision_shapes(CT.VISION), 0), CT.device_weights(CR.text_shapes(CT.TEXT), 1),
                     CT.device_weights(CR.resampler_shapes(CT.RESAMPLER), 2))
    pairs = PAIRS if CLIP16 else PAIRS[:1]
    kw = lambda p, a: dict(precision=p, attention_precision=a) if CLIP16 else {}
    g = torch.Generator(device="cuda").manual_seed(3)
    images = (torch.rand(4, 224, 224, 3, device="cuda", generator=g) * 255).to(torch.uint8)
    frame = torch.rand(1080, 1920, 3, device="cuda", generator=g)
    ids = torch.randint(0, CT.TEXT["vocab"], (2, 77), device="cuda", generator=g)
    vnets = {label(p, a): clip.ClipImageEncoder(vsd, **kw(p, a)).to("cuda") for p, a in pairs}
    rnets = {label(p, a): clip.Resampler(rsd, **kw(p, a)).to("cuda") for p, a in pairs}
    tnets = {label(p, a): clip.ClipTextEncoder(tsd, **kw(p, a)).to("cuda") for p, a in pairs}
    tokens = {k: clip.ImageTokens(vnets[k], rnets[k]) for k in vnets}
    tables = {"image_encoder_1": {k: (lambda n=n: n(images[:1])) for k, n in vnets.items()},
              "image_encoder_4": {k: (lambda n=n: n(images)) for k, n in vnets.items()},
              "image_tokens_1080x1920": {k: (lambda n=n: n(frame)) for k, n in tokens.items()},
              "text_encoder_2x77": {k: (lambda n=n: n(ids)) for k, n in tnets.items()}}
    if CLIP16:                                                   # torch: the same composition, its tensors converted
        CR.attention = CT.sdpa_attention
        bf = torch.bfloat16
        vb, tb, rb = ({k: v.to(bf) for k, v in sd.items()} for sd in (vsd, tsd, rsd))
        t_vision = lambda u8: CR.vision_forward(vb, CT.VISION, CR.normalized(u8, bf), bf)[0]
        any_vnet = next(iter(vnets.values()))
        tables["image_encoder_1"]["torch_bf16_sdpa"] = lambda: t_vision(images[:1])
        tables["image_encoder_4"]["torch_bf16_sdpa"] = lambda: t_vision(images)
        tables["image_tokens_1080x1920"]["torch_bf16_sdpa"] = lambda: CR.resampler_forward(rb, CT.RESAMPLER, t_vision(any_vnet.resized(frame)), bf)[0][0]
        tables["text_encoder_2x77"]["torch_bf16_sdpa"] = lambda: CR.text_forward(tb, CT.TEXT, ids, bf)[0]
    for name, fns in tables.items():
        res[name] = alternating(fns, warmup, iters)
    if CLIP16:
        ref = tokens["f32/f32"](frame)[0]
        rms = ref.pow(2).mean().sqrt()
        res["image_tokens_distance_to_f32_worst_over_rms"] = {k: ((n(frame)[0] - ref).abs().max() / rms).item() for k, n in tokens.items() if k != "f32/f32"}


def main():
    args = ARGS
    assert args.iters >= 5
    res = {"device": torch.cuda.get_device_name(0), "warmup": args.warmup, "iters": args.iters,
           "unit": "ms per call (median, min, max of device events); the kernel alone: 10 calls per event pair",
           "configs": "(precision, attention_precision); shipped shapes, random weights",
           "tree": ("this, as the parent is timed" if args.yardstick else "this") if os.path.abspath(args.root) == ROOT else "--root"}
    gc.collect()
    gc.freeze()
    gc.disable()
    with torch.no_grad():
        if HAS16:
            res["kernel_alone"] = [
                kernel_alone("UNet level-0 self-attention", 2, 4096, 4096, 5, 64, 0, unet.attention, args.warmup, args.iters),
                kernel_alone("UNet level-0 cross-attention, 77 + 16 tokens", 8, 1024, 77, 5, 64, 16, unet.attention, args.warmup, args.iters),
                kernel_alone("ViT-H/14, 257 tokens", 1, 257, 257, 16, 80, 0, clip.attention, args.warmup, args.iters),
            ]
        unet_section(res, args.warmup, args.iters)
        clip_section(res, args.warmup, args.iters)
    keep = ("unet_forward", "image_encoder_1", "image_encoder_4", "image_tokens_1080x1920", "text_encoder_2x77")
    for key, files in (("parent", args.parent), ("this_as_the_parent_is_timed", args.this)):
        for f in files:
            p = json.load(open(f))
            res.setdefault(key, []).append({k: p[k] for k in keep if k in p})
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
