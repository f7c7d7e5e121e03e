"""The SDS guidance's conditioning with 16-bit products and / or the 16-bit attention (soar_amd/clip.py ``precision`` /
``attention_precision``; csrc/clip.hip, csrc/conv_gemm.hip conv_gemm16_kernel, csrc/attention.hip kv_attn16_kernel)
against the restatements of tests/clip_ref.py (float64) and tests/clip_half_ref.py (float64 with the same roundings), on the tiny towers
of tests/test_clip_gpu.py.

Tolerance, measured not fixed (tests/test_unet_half_gpu.py): ``e16`` is the distance of the rounded restatement from plain float64,
worst element over the float64 tensor's RMS, and the kernels must lie within ``4 e16`` of float64.  A stage no rounding reaches (the
embedding of the text tower: a float32 sum) has ``e16`` = 0 and is held to the float32 bar of tests/test_clip_gpu.py instead."""
import pytest
import torch

import clip_half_ref as H
import clip_ref as R
from test_clip_gpu import ids_of, image_of
from test_unet_half_gpu import rel, within

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAIRS = [("bf16", "f32"), ("bf16", "bf16"), ("f16", "f16")]
TEXT = {"A": R.TEXT_A, "B": R.TEXT_B}
VISION = {"A": R.VISION_A, "B": R.VISION_B}
RESAMPLER = {"A": R.RESAMPLER_A, "B": R.RESAMPLER_B}
_nets = {}


def text(name, prec="f32", attn="f32"):
    from soar_amd import clip
    cfg = TEXT[name]
    sd = R.tiny_state_dict(R.text_shapes(cfg), 10)
    if ("text", name, prec, attn) not in _nets:
        _nets["text", name, prec, attn] = clip.ClipTextEncoder(sd, heads=cfg["heads"], precision=prec, attention_precision=attn).to(DEV)
    return cfg, sd, _nets["text", name, prec, attn]


def vision(name, prec="f32", attn="f32"):
    from soar_amd import clip
    cfg = VISION[name]
    sd = R.tiny_state_dict(R.vision_shapes(cfg), 20)
    if ("vision", name, prec, attn) not in _nets:
        _nets["vision", name, prec, attn] = clip.ClipImageEncoder(sd, heads=cfg["heads"], precision=prec, attention_precision=attn).to(DEV)
    return cfg, sd, _nets["vision", name, prec, attn]


def resampler(name, prec="f32", attn="f32"):
    from soar_amd import clip
    cfg = RESAMPLER[name]
    sd = R.tiny_state_dict(R.resampler_shapes(cfg), 30)
    if ("resampler", name, prec, attn) not in _nets:
        _nets["resampler", name, prec, attn] = clip.Resampler(sd, dim_head=cfg["dim_head"], precision=prec, attention_precision=attn).to(DEV)
    return cfg, sd, _nets["resampler", name, prec, attn]


def held(label, taps, out, s64, o64, s16, o16, probes, s32=None):
    """every probe and the output within 4 e16; a probe no rounding reaches (e16 = 0) within 4 e32 (s32: the float32 restatement's)"""
    ratios = []
    for key in probes:
        if rel(s16[key], s64[key]) > 0:
            ratios.append(within(f"{label} {key}", taps[key], s64[key], s16[key]))
        else:
            e32, err = rel(s32[key], s64[key]), rel(taps[key], s64[key])
            print(f"{label} {key}: no rounding in front of it: err {err:.3g}  e32 {e32:.3g}")
            assert err <= 4.0 * e32
    ratios.append(within(f"{label} out", out, o64, o16))
    print(f"{label}: largest ratio {max(ratios):.2f}")


@pytest.mark.parametrize("prec,attn", PAIRS)
@pytest.mark.parametrize("name,L", [("A", 13), ("B", 77), ("B", 150)])
def test_text_stage_by_stage(name, L, prec, attn):
    cfg, sd, net = text(name, prec, attn)
    ids = ids_of(cfg, 2, L)
    probes = [("embed", ""), (0, "attn"), (0, "block"), (cfg["layers"] - 1, "attn"), (cfg["layers"] - 1, "block")]
    out, taps = net(ids.to(DEV), probes=probes)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32
    o64, s64 = R.text_forward(sd, cfg, ids, torch.float64)
    o16, s16 = H.text_forward(sd, cfg, ids, prec, attn)
    held(f"text {name} L={L} {prec}/{attn}", taps, out, s64, o64, s16, o16, probes, R.text_forward(sd, cfg, ids, torch.float32)[1])


@pytest.mark.parametrize("prec,attn", PAIRS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_vision_stage_by_stage(name, prec, attn):
    cfg, sd, net = vision(name, prec, attn)
    img = image_of(cfg, 3, B=2)
    probes = [("embed", ""), ("pre", ""), (0, "attn"), (0, "block"), (cfg["layers"] - 1, "block")]
    out, taps = net(img.to(DEV), probes=probes)
    torch.cuda.synchronize()
    px = R.normalized(R.resized(img, cfg["image"]), torch.float64)
    o64, s64 = R.vision_forward(sd, cfg, px, torch.float64)
    o16, s16 = H.vision_forward(sd, cfg, px, prec, attn)
    assert out.shape == (2, R.tokens_of(cfg), cfg["width"])
    held(f"vision {name} {prec}/{attn}", taps, out, s64, o64, s16, o16, probes)


@pytest.mark.parametrize("prec,attn", PAIRS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_resampler_stage_by_stage(name, prec, attn):
    cfg, sd, net = resampler(name, prec, attn)
    n = {"A": 26, "B": 145}[name]
    x = torch.randn(2, n, cfg["emb"], generator=torch.Generator().manual_seed(n))
    probes = [(i, s) for i in range(cfg["depth"]) for s in ("attn", "ff")]
    out, taps = net(x.to(DEV), probes=probes)
    torch.cuda.synchronize()
    o64, s64 = R.resampler_forward(sd, cfg, x, torch.float64)
    o16, s16 = H.resampler_forward(sd, cfg, x, prec, attn)
    held(f"resampler {name} {prec}/{attn}", taps, out, s64, o64, s16, o16, probes)


def test_the_restatement_without_roundings_is_clip_ref():
    """the harness: at f32 / f32 tests/clip_half_ref.py computes what tests/clip_ref.py does (no GPU involved)"""
    cfg, sd, _ = text("A")
    ids = ids_of(cfg, 2, 13)
    assert rel(H.text_forward(sd, cfg, ids)[0], R.text_forward(sd, cfg, ids, torch.float64)[0]) < 1e-12
    vcfg, vsd, _ = vision("A")
    px = R.normalized(R.resized(image_of(vcfg, 3), vcfg["image"]), torch.float64)
    assert rel(H.vision_forward(vsd, vcfg, px)[0], R.vision_forward(vsd, vcfg, px, torch.float64)[0]) < 1e-12
    rcfg, rsd, _ = resampler("A")
    x = torch.randn(1, 26, rcfg["emb"], generator=torch.Generator().manual_seed(2))
    assert rel(H.resampler_forward(rsd, rcfg, x)[0], R.resampler_forward(rsd, rcfg, x, torch.float64)[0]) < 1e-12


@pytest.mark.parametrize("prec,attn", PAIRS)
@pytest.mark.parametrize("p", [31, 32, 76])
def test_causality_is_exact(p, prec, attn):
    """changing the tokens behind position p leaves the rows up to p bit-equal (tests/test_clip_gpu.py's test at 16 bits)"""
    cfg, sd, net = text("B", prec, attn)
    ids = ids_of(cfg, 1, 150)
    other = ids.clone()
    other[:, p + 1:] = (ids[:, p + 1:] + 1 + torch.arange(150 - p - 1) % 7) % cfg["vocab"]
    a, b = net(ids.to(DEV)), net(other.to(DEV))
    assert torch.equal(a[:, :p + 1], b[:, :p + 1])
    assert not torch.equal(a[:, p + 1], b[:, p + 1])


@pytest.mark.parametrize("prec,attn", PAIRS)
def test_batch_independence_and_repeatability(prec, attn):
    cfg, sd, net = text("B", prec, attn)
    ids = ids_of(cfg, 3, 77).to(DEV)
    both = net(ids)
    assert torch.equal(both, net(ids))
    for b in range(3):
        assert torch.equal(net(ids[b:b + 1]), both[b:b + 1]), b
    vcfg, _, vnet = vision("B", prec, attn)
    img = image_of(vcfg, 7, B=3).to(DEV)
    vboth = vnet(img)
    assert torch.equal(vboth, vnet(img))
    for b in range(3):
        assert torch.equal(vnet(img[b]), vboth[b:b + 1]), b
    rcfg, _, rnet = resampler("B", prec, attn)
    x = torch.randn(3, 145, rcfg["emb"], generator=torch.Generator().manual_seed(1)).to(DEV)
    rboth = rnet(x)
    assert torch.equal(rboth, rnet(x))
    for b in range(3):
        assert torch.equal(rnet(x[b:b + 1]), rboth[b:b + 1]), b


def test_defaults_give_the_bits_of_the_modules_without_the_arguments():
    from soar_amd import clip
    cfg, sd, named = text("A")
    ids = ids_of(cfg, 2, 13).to(DEV)
    plain = clip.ClipTextEncoder(sd, heads=cfg["heads"]).to(DEV)
    assert plain.precision == plain.attention_precision == "f32" and plain._packed_bytes == named._packed_bytes
    want = plain(ids)
    assert torch.equal(named(ids), want)
    _, _, half = text("A", "bf16", "bf16")
    assert not torch.equal(half(ids), want) and half._packed_bytes < plain._packed_bytes
    assert half._pack.packed is not plain._pack.packed and torch.equal(half.weights, plain.weights)
    assert torch.equal(plain(ids), want)                         # ... whose packed weights are their own
    vcfg, vsd, vnamed = vision("A")
    img = image_of(vcfg, 3, B=2).to(DEV)
    assert torch.equal(vnamed(img), clip.ClipImageEncoder(vsd, heads=vcfg["heads"]).to(DEV)(img))
    assert not torch.equal(vision("A", "f32", "f16")[2](img), vnamed(img))
    rcfg, rsd, rnamed = resampler("A")
    x = torch.randn(2, 26, rcfg["emb"], generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(rnamed(x), clip.Resampler(rsd, dim_head=rcfg["dim_head"]).to(DEV)(x))
    assert not torch.equal(resampler("A", "f32", "bf16")[2](x), rnamed(x))


@pytest.mark.parametrize("prec,attn", PAIRS)
def test_image_tokens_run_end_to_end(prec, attn):
    from soar_amd import clip
    vcfg, vsd, vnet = vision("A", prec, attn)
    rcfg, rsd, rnet = resampler("A", prec, attn)
    tokens = clip.ImageTokens(vnet, rnet)
    ref_rgb = R.sample_image(37, 83, 13, as_float=True)
    cond, uncond = tokens(ref_rgb.to(DEV))
    torch.cuda.synchronize()
    assert cond.shape == (rcfg["queries"], rcfg["out"]) and cond.dtype == torch.float32 and float(uncond.abs().max()) == 0
    px = R.normalized(R.resized(ref_rgb, vcfg["image"]), torch.float64)
    t64 = R.resampler_forward(rsd, rcfg, R.vision_forward(vsd, vcfg, px, torch.float64)[0], torch.float64)[0][0]
    t16 = H.resampler_forward(rsd, rcfg, H.vision_forward(vsd, vcfg, px, prec, attn)[0], prec, attn)[0][0]
    within(f"ImageTokens {prec}/{attn}", cond, t64, t16)
