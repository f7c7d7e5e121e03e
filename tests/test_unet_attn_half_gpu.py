"""The multi-view diffusion UNet with its attentions on the 16-bit matrix core (soar_amd/unet.py ``attention_precision="bf16"`` /
``"f16"``, csrc/attention.hip kv_attn16_kernel), alone and together with the 16-bit products of 9y, against the
restatements of tests/unet_ref.py (float64) and tests/unet_attn_half_ref.py (float64 with the same roundings).

Tolerance, measured not fixed (tests/test_unet_half_gpu.py): ``e16`` is the distance of the rounded restatement from plain float64,
worst element over the float64 tensor's RMS, and the kernels must lie within ``4 e16`` of float64.  Where no attention lies in front of
a stage and the products are float32, ``e16`` is 0 and the stage is held to the float32 bar of tests/test_unet_gpu.py instead."""
import pytest
import torch

import unet_attn_half_ref as A
import unet_ref as R
from test_unet_half_gpu import CFGS, PROBES, on_dev, rel, run, within
from test_unet_half_gpu import setup as load

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAIRS = [("f32", "bf16"), ("bf16", "bf16"), ("f16", "f16")]
_nets = {}
_r32 = {}


def net_of(name, prec, attn):
    if (name, prec, attn) not in _nets:
        from soar_amd import unet
        cfg = CFGS[name]
        _nets[name, prec, attn] = unet.MultiviewUNet(R.tiny_state_dict(cfg, 0), num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"],
                                                     ip_weight=cfg["ip_weight"], n_view=cfg["n_view"], precision=prec, attention_precision=attn).to(DEV)
    return _nets[name, prec, attn]


def float32_restatement(name):
    if name not in _r32:
        cfg, sd, inp, _ = load(name)
        _r32[name] = R.forward(sd, cfg, *inp, dtype=torch.float32)
    return _r32[name]


def held(label, got, ref64, ref16, ref32):
    """within 4 e16; a stage the roundings do not reach (e16 = 0) within 4 e32, the float32 path's own bar"""
    if rel(ref16, ref64) > 0:
        return within(label, got, ref64, ref16)
    e32, err = rel(ref32, ref64), rel(got, ref64)
    print(f"{label}: no rounding in front of it: err {err:.3g}  e32 {e32:.3g}")
    assert err <= 4.0 * e32
    return 0.0


@pytest.mark.parametrize("prec,attn", PAIRS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_stage_by_stage(name, prec, attn):
    cfg, sd, inp, (eps64, st64) = load(name)
    eps16, st16 = A.forward(sd, cfg, *inp, precision=prec, attention_precision=attn)
    eps32, st32 = float32_restatement(name)
    eps, taps = run(net_of(name, prec, attn), on_dev(inp), probes=PROBES[name])
    torch.cuda.synchronize()
    assert eps.shape == eps64.shape and eps.dtype == torch.float32
    ratios = []
    for key in PROBES[name]:
        assert taps[key].shape == st64[key].shape and taps[key].dtype == torch.float32
        ratios.append(held(f"{name} {prec}/{attn} {key[0]} {key[1]}", taps[key], st64[key], st16[key], st32[key]))
    ratios.append(held(f"{name} {prec}/{attn} eps", eps, eps64, eps16, eps32))
    print(f"{name} {prec}/{attn}: largest ratio {max(ratios):.2f}")


@pytest.mark.parametrize("prec,attn", PAIRS)
def test_groups_and_runs_are_bit_equal(prec, attn):
    cfg, sd, inp, _ = load("A")
    net = net_of("A", prec, attn)
    d = on_dev(inp)
    both = run(net, d)
    assert torch.equal(both, run(net, d))                        # two runs
    f = cfg["n_view"]
    for g0 in (0, f):                                            # each group alone
        one = run(net, tuple(v[g0:g0 + f] for v in d))
        assert torch.equal(one, both[g0:g0 + f]), g0


def test_the_default_is_the_float32_attention_and_the_16_bit_one_is_another():
    from soar_amd import unet
    cfg, sd, inp, (eps64, _) = load("A")
    kw = dict(num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"], ip_weight=cfg["ip_weight"], n_view=cfg["n_view"])
    d = on_dev(inp)
    for prec in ("f32", "bf16"):
        omitted = unet.MultiviewUNet(sd, precision=prec, **kw).to(DEV)
        named = net_of("A", prec, "f32")
        assert omitted.attention_precision == named.attention_precision == "f32"
        assert omitted._packed_bytes == named._packed_bytes == net_of("A", prec, "bf16")._packed_bytes
        e_omitted, e_named = run(omitted, d), run(named, d)
        assert torch.equal(e_omitted, e_named)
        assert not torch.equal(run(net_of("A", prec, "bf16"), d), e_named)


def test_guidance_runs_with_16_bit_attention():
    """sds.MultiviewGuidance with a (bf16, bf16) UNet at the tiny configuration: loss and image gradient lie within 4 e16 of MultiviewSDS
    with the float64 restatement as its eps_fn, e16 taken with the rounded restatement as eps_fn (tests/test_unet_half_gpu.py's test)."""
    import vae_ref
    from soar_amd import sds
    cfg, sd, _, _ = load("A")
    net = net_of("A", "bf16", "bf16")
    Bn, S = 4, 64
    g = torch.Generator().manual_seed(11)
    enc = sds.LatentEncoder(vae_ref.random_weights(0)).to(DEV)
    rgb = torch.rand(Bn, 40, 48, 3, generator=g).to(DEV)
    text = torch.randn(2, cfg["T"], cfg["context_dim"], generator=g).to(DEV)
    tokens = torch.randn(cfg["ip_dim"], cfg["context_dim"], generator=g).to(DEV)
    c2w = torch.randn(Bn, 4, 4, generator=g).to(DEV)
    ref_rgb = torch.rand(3, 32, 32, generator=g).to(DEV)
    noise, post = (torch.randn(Bn, 4, S // 8, S // 8, generator=g).to(DEV) for _ in range(2))
    t = torch.tensor([431], device=DEV)
    args = dict(guidance_scale=5.0, n_view=4, recon_loss=True, recon_std_rescale=0.2, image_size=S)
    guide = sds.MultiviewGuidance(enc, net, text, image_tokens=lambda img: (tokens, torch.zeros_like(tokens)), **args).to(DEV)
    cam = c2w.clone()
    cam[:, :3, 3] = c2w[:, :3, 3] / (c2w[:, :3, 3].norm(dim=1, keepdim=True) + 1e-8)
    ctx = torch.cat([text[0:1].expand(Bn, -1, -1), text[1:2].expand(Bn, -1, -1)])
    cam2 = cam.reshape(Bn, 16).repeat(2, 1)
    ip = torch.cat([tokens[None].expand(Bn, -1, -1), torch.zeros_like(tokens)[None].expand(Bn, -1, -1)])

    def result(fn):
        x = rgb.clone().requires_grad_(True)
        out = fn(x)
        out["loss_sds"].backward()
        torch.cuda.synchronize()
        return out["loss_sds"].detach().reshape(1), x.grad

    def restated(fwd):
        plain = sds.MultiviewSDS(enc, **args).to(DEV)
        eps_fn = lambda x_in, tt: fwd(sd, cfg, x_in.cpu(), tt.cpu(), ctx.cpu(), cam2.cpu(), ip.cpu())[0].to(DEV)
        return result(lambda x: plain(x, eps_fn, t=t, noise=noise, posterior_noise=post))

    loss, grad = result(lambda x: guide(x, c2w=c2w, ref_rgb=ref_rgb, t=t, noise=noise, posterior_noise=post, elevation=None))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    l64, g64 = restated(lambda *a: R.forward(*a, dtype=torch.float64))
    l16, g16 = restated(lambda *a: A.forward(*a, precision="bf16", attention_precision="bf16"))
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    within("guidance bf16/bf16 loss_sds", loss, l64.double(), l16)
    within("guidance bf16/bf16 image gradient", grad, g64.double(), g16)
