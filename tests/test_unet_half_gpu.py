"""The multi-view diffusion UNet with 16-bit matrix products (soar_amd/unet.py ``precision="bf16"`` / ``"f16"``, csrc/unet.hip,
csrc/conv_gemm.hip conv_gemm16_kernel) against the restatements of tests/unet_ref.py (float64) and
tests/unet_half_ref.py (float64 with every product operand rounded to the type).

Tolerance, measured not fixed: for every compared tensor ``e16`` is the distance of the rounded restatement from plain float64 (worst
element over the float64 tensor's RMS: ``rel`` of tests/test_unet_gpu.py), and the kernels must lie within ``4 e16`` of float64.  4 is
the factor of all the project's networks; it covers the order of accumulation and an operand that rounds the other way on the device
because the float32 activations in front of it differ in their last bits."""
import pytest
import torch

import unet_half_ref as H
import unet_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FACTOR = 4.0
CFGS = {"A": R.CONFIG_A, "B": R.CONFIG_B}
PRECS = ["bf16", "f16"]
# the probe lists of tests/test_unet_gpu.py
PROBES = {
    "A": [("emb", ""), ("input_blocks.0", "res"), ("input_blocks.1", "res"), ("input_blocks.1", "attn1"), ("input_blocks.1", "attn2"),
          ("input_blocks.1", "ff"), ("input_blocks.1", "transformer"), ("input_blocks.2", "res"), ("middle_block", "res2"),
          ("output_blocks.1", "cat"), ("output_blocks.1", "res"), ("output_blocks.1", "up")],
    "B": [("emb", ""), ("input_blocks.0", "res"), ("input_blocks.1", "res"), ("input_blocks.3", "res"), ("input_blocks.4", "res"),
          ("input_blocks.4", "attn1"), ("input_blocks.4", "attn2"), ("input_blocks.4", "ff"), ("input_blocks.4", "transformer"),
          ("middle_block", "res2"), ("output_blocks.2", "cat"), ("output_blocks.2", "res"), ("output_blocks.2", "up"),
          ("output_blocks.5", "up")],
}
_cache = {}
_nets = {}


def rel(a, b):
    """worst element of a - b over b's RMS (b: float64)"""
    return float((a.double().cpu() - b.cpu()).abs().max() / b.cpu().pow(2).mean().sqrt())


def within(name, got, ref64, ref16):
    e16 = rel(ref16, ref64)
    err = rel(got, ref64)
    print(f"{name}: err {err:.3g}  e16 {e16:.3g}  ratio {err / e16 if e16 else float('inf' if err else 0):.2f}")
    if e16 == 0:
        assert torch.equal(got.double().cpu(), ref64.cpu()), f"{name}: the rounded restatement is exact, the kernels are not"
    assert err <= FACTOR * e16, f"{name}: {err:.3g} from float64, rounded restatement {e16:.3g}: ratio {err / e16 if e16 else float('inf'):.2f} > {FACTOR}"
    return err / e16 if e16 else 0.0


def net_of(name, prec):
    if (name, prec) not in _nets:
        from soar_amd import unet
        cfg = CFGS[name]
        _nets[name, prec] = unet.MultiviewUNet(R.tiny_state_dict(cfg, 0), num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"],
                                               ip_weight=cfg["ip_weight"], n_view=cfg["n_view"], precision=prec).to(DEV)
    return _nets[name, prec]


def setup(name):
    """The state dict, the inputs and the float64 restatement (computed once, on the CPU)."""
    if name not in _cache:
        cfg = CFGS[name]
        sd = R.tiny_state_dict(cfg, 0)
        inp = R.inputs(cfg, 0)
        _cache[name] = (cfg, sd, inp, R.forward(sd, cfg, *inp, dtype=torch.float64))
    return _cache[name]


def on_dev(inp):
    return tuple(None if v is None else v.to(DEV) for v in inp)


def run(net, inp, **kw):
    x, t, ctx, cam, ip = inp
    return net(x, t, ctx, camera=cam, ip_tokens=ip, **kw)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_stage_by_stage(name, prec):
    cfg, sd, inp, (eps64, st64) = setup(name)
    eps16, st16 = H.forward(sd, cfg, *inp, precision=prec)
    eps, taps = run(net_of(name, prec), on_dev(inp), probes=PROBES[name])
    torch.cuda.synchronize()
    assert eps.shape == eps64.shape and eps.dtype == torch.float32
    ratios = []
    for key in PROBES[name]:
        assert taps[key].shape == st64[key].shape and taps[key].dtype == torch.float32
        ratios.append(within(f"{name} {prec} {key[0]} {key[1]}", taps[key], st64[key], st16[key]))
    ratios.append(within(f"{name} {prec} eps", eps, eps64, eps16))
    print(f"{name} {prec}: largest ratio {max(ratios):.2f}")


def test_the_16_bit_path_is_another():
    cfg, sd, inp, (eps64, _) = setup("A")
    d = on_dev(inp)
    e32, e16 = run(net_of("A", "f32"), d), run(net_of("A", "bf16"), d)
    assert not torch.equal(e16, e32)
    assert rel(e16, eps64) > rel(e32, eps64)


@pytest.mark.parametrize("prec", PRECS)
def test_groups_runs_and_strides_are_bit_equal(prec):
    cfg, sd, inp, _ = setup("A")
    net = net_of("A", prec)
    d = on_dev(inp)
    both = run(net, d)
    assert torch.equal(both, run(net, d))                        # two runs
    f = cfg["n_view"]
    for g0 in (0, f):                                            # each group alone
        one = run(net, tuple(v[g0:g0 + f] for v in d))
        assert torch.equal(one, both[g0:g0 + f]), g0
    x = d[0]
    strided = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)[:, :, :, :]
    assert not strided.is_contiguous() and torch.equal(strided, x)
    assert torch.equal(run(net, (strided,) + d[1:]), both)
    wide = torch.zeros(x.shape[0], x.shape[1], x.shape[2], 2 * x.shape[3], device=DEV)
    wide[..., ::2] = x
    assert torch.equal(run(net, (wide[..., ::2],) + d[1:]), both)


def test_two_precisions_of_one_state_dict_keep_their_own_packed_weights():
    from soar_amd import unet
    cfg, sd, inp, _ = setup("A")
    kw = dict(num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"], ip_weight=cfg["ip_weight"], n_view=cfg["n_view"])
    n32 = unet.MultiviewUNet(sd, **kw).to(DEV)
    n16 = unet.MultiviewUNet(sd, precision="bf16", **kw).to(DEV)
    assert n32.precision == "f32" and n16.precision == "bf16"
    assert n16.weights.dtype == torch.float32 and torch.equal(n16.weights, n32.weights)
    d = on_dev(inp)
    before = run(n32, d).clone()
    half = run(n16, d)
    assert n32._pack.packed is not n16._pack.packed and n32._pack.packed.data_ptr() != n16._pack.packed.data_ptr()
    assert n16._packed_bytes < n32._packed_bytes
    assert torch.equal(run(n32, d), before)
    assert not torch.equal(half, before)


def test_guidance_runs_with_a_bf16_unet():
    """sds.MultiviewGuidance with a bf16 UNet at the tiny configuration: loss and image gradient are finite and lie within 4 e16 of
    MultiviewSDS with the float64 restatement as its eps_fn, e16 taken with the rounded restatement as eps_fn."""
    import vae_ref
    from soar_amd import sds
    cfg, sd, _, _ = setup("A")
    net = net_of("A", "bf16")
    B, S = 4, 64
    g = torch.Generator().manual_seed(11)
    enc = sds.LatentEncoder(vae_ref.random_weights(0)).to(DEV)
    rgb = torch.rand(B, 40, 48, 3, generator=g).to(DEV)
    text = torch.randn(2, cfg["T"], cfg["context_dim"], generator=g).to(DEV)
    tokens = torch.randn(cfg["ip_dim"], cfg["context_dim"], generator=g).to(DEV)
    c2w = torch.randn(B, 4, 4, generator=g).to(DEV)
    ref_rgb = torch.rand(3, 32, 32, generator=g).to(DEV)
    noise, post = (torch.randn(B, 4, S // 8, S // 8, generator=g).to(DEV) for _ in range(2))
    t = torch.tensor([431], device=DEV)
    args = dict(guidance_scale=5.0, n_view=4, recon_loss=True, recon_std_rescale=0.2, image_size=S)
    guide = sds.MultiviewGuidance(enc, net, text, image_tokens=lambda img: (tokens, torch.zeros_like(tokens)), **args).to(DEV)
    cam = c2w.clone()
    cam[:, :3, 3] = c2w[:, :3, 3] / (c2w[:, :3, 3].norm(dim=1, keepdim=True) + 1e-8)
    ctx = torch.cat([text[0:1].expand(B, -1, -1), text[1:2].expand(B, -1, -1)])
    cam2 = cam.reshape(B, 16).repeat(2, 1)
    ip = torch.cat([tokens[None].expand(B, -1, -1), torch.zeros_like(tokens)[None].expand(B, -1, -1)])

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
    l16, g16 = restated(lambda *a: H.forward(*a, precision="bf16"))
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    within("guidance bf16 loss_sds", loss, l64.double(), l16)
    within("guidance bf16 image gradient", grad, g64.double(), g16)
