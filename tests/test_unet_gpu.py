"""The multi-view diffusion UNet on the device (soar_amd/unet.py, csrc/unet.hip, csrc/attention.hip) against the
plain-torch restatement of tests/unet_ref.py in float64.

Tolerance, measured not fixed (the bar of tests/test_sam_gpu.py): for every compared tensor ``e32`` is the distance of the restatement
run in float32 from the restatement run in float64 (worst element over the float64 tensor's RMS), and the kernels must lie within
``4 e32`` of float64: the factor covers another order of accumulation over the same float32 operands.  Both configurations are tiny
(tests/unet_ref.py).
"""
import pytest
import torch

import unet_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FACTOR = 4.0
CFGS = {"A": R.CONFIG_A, "B": R.CONFIG_B}
# embedding, first convolution, a ResBlock, a transformer block after attn1 / attn2 / ff and whole, a down-sampling, the concatenated
# input and its ResBlock, an up-sampling (B: one at .1.conv and one at .2.conv), the middle block's end
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


def rel(a, b):
    """worst element of a - b over b's RMS (b: float64)"""
    return float((a.double().cpu() - b.cpu()).abs().max() / b.cpu().pow(2).mean().sqrt())


def within(name, got, ref64, ref32):
    e32 = rel(ref32, ref64)
    err = rel(got, ref64)
    print(f"{name}: err {err:.3g}  e32 {e32:.3g}  ratio {err / e32 if e32 else float('inf' if err else 0):.2f}")
    assert err <= FACTOR * e32, f"{name}: {err:.3g} from float64, float32 restatement {e32:.3g}: ratio {err / e32 if e32 else float('inf'):.2f} > {FACTOR}"


def setup(name):
    """The module, the inputs, and the restatement's eps and stages in float64 and float32 (computed once, on the CPU)."""
    if name not in _cache:
        from soar_amd import unet
        cfg = CFGS[name]
        sd = R.tiny_state_dict(cfg, 0)
        net = unet.MultiviewUNet(sd, num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"], ip_weight=cfg["ip_weight"],
                                 n_view=cfg["n_view"]).to(DEV)
        inp = R.inputs(cfg, 0)
        r64 = R.forward(sd, cfg, *inp, dtype=torch.float64)
        r32 = R.forward(sd, cfg, *inp, dtype=torch.float32)
        _cache[name] = (cfg, sd, net, inp, r64, r32)
    return _cache[name]


def on_dev(inp):
    return tuple(None if v is None else v.to(DEV) for v in inp)


def run(net, inp, **kw):
    x, t, ctx, cam, ip = inp
    return net(x, t, ctx, camera=cam, ip_tokens=ip, **kw)


@pytest.mark.parametrize("name", ["A", "B"])
def test_stage_by_stage(name):
    cfg, sd, net, inp, (eps64, st64), (eps32, st32) = setup(name)
    eps, taps = run(net, on_dev(inp), probes=PROBES[name])
    torch.cuda.synchronize()
    assert eps.shape == eps64.shape
    for key in PROBES[name]:
        assert taps[key].shape == st64[key].shape, (key, taps[key].shape, st64[key].shape)
        within(f"{name} {key[0]} {key[1]}", taps[key], st64[key], st32[key])
    within(f"{name} eps", eps, eps64, eps32)


ATTN_CASES = [(1, 1, 64, 1, 0), (64, 7, 16, 2, 0), (200, 93, 64, 3, 0), (130, 130, 32, 2, 0), (256, 256, 64, 5, 0), (200, 77, 64, 3, 16)]


@pytest.mark.parametrize("Lq,Lk,hd,heads,Lk2", ATTN_CASES)
def test_attention_kernel_alone(Lq, Lk, hd, heads, Lk2):
    """the key tail, a query tile's tail, a padded head, more than one key tile; a second key set with weight 0.5.  The sources
    are slices of wider rows (q | k | v of one product), so every pointer has its own pitch."""
    from soar_amd import unet
    B, C = 2, heads * hd
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q = torch.randn(B, Lq, C, generator=g) * 1.5
    kv = torch.randn(B, Lk, 2 * C + 4, generator=g)
    k, v = kv[..., :C], kv[..., C:2 * C]
    ref = lambda dt: R.attention(q.to(dt), k.to(dt), v.to(dt), heads)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    kvd = kv.to(DEV)
    args = dict()
    if Lk2:
        kv2 = torch.randn(B, Lk2, 2 * C, generator=g)
        k2, v2 = kv2[..., :C], kv2[..., C:]
        ref2 = lambda dt: R.attention(q.to(dt), k2.to(dt), v2.to(dt), heads)
        r64, r32 = r64 + 0.5 * ref2(torch.float64), r32 + 0.5 * ref2(torch.float32)
        kv2d = kv2.to(DEV)
        args = dict(k2=kv2d[..., :C], v2=kv2d[..., C:], w2=0.5)
    out = unet.attention(q.to(DEV), kvd[..., :C], kvd[..., C:2 * C], heads, **args)
    again = unet.attention(q.to(DEV), kvd[..., :C], kvd[..., C:2 * C], heads, **args)
    torch.cuda.synchronize()
    assert torch.equal(out, again)
    within(f"attention Lq={Lq} Lk={Lk} hd={hd} heads={heads} Lk2={Lk2}", out, r64, r32)


def test_groups_runs_and_strides_are_bit_equal():
    cfg, sd, net, inp, _, _ = setup("A")
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


def test_refusals():
    from soar_amd import hip_lib
    cfg, sd, net, inp, _, _ = setup("A")
    x, t, ctx, cam, ip = on_dev(inp)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        net(x.cpu(), t, ctx, camera=cam, ip_tokens=ip)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        net(x, t, ctx.cpu(), camera=cam, ip_tokens=ip)
    with pytest.raises(ValueError, match="multiple of n_view"):
        net(x[:6], t[:6], ctx[:6], camera=cam[:6], ip_tokens=ip[:6])
    with pytest.raises(ValueError, match="level 0 is 7 x 8"):
        net(x[:, :, :7], t, ctx, camera=cam, ip_tokens=ip)
    with pytest.raises(ValueError, match="context must be"):
        net(x, t, ctx[..., :32], camera=cam, ip_tokens=ip)
    with pytest.raises(ValueError, match="no camera is given"):
        net(x, t, ctx, ip_tokens=ip)
    with pytest.raises(hip_lib.SoarHipError, match=r"workspace of 1024 bytes, need \d+ \(soar_unet_workspace_bytes\)"):
        net(x, t, ctx, camera=cam, ip_tokens=ip, workspace=hip_lib._workspace(1024, DEV))
    cfgb, _, netb, inpb, _, _ = setup("B")
    xb, tb, ctxb, _, _ = on_dev(inpb)
    with pytest.raises(ValueError, match="no camera_embed"):
        netb(xb, tb, ctxb, camera=torch.zeros(3, 16, device=DEV))
    with pytest.raises(ValueError, match="no attn2.to_k_ip"):
        netb(xb, tb, ctxb, ip_tokens=torch.zeros(3, 16, 40, device=DEV))
    with pytest.raises(ValueError, match="level 1 is 4 x 5"):
        netb(xb[..., :10], tb, ctxb)
    # the C entry refuses the same by itself
    import ctypes as C
    nb = C.c_size_t(0)
    assert hip_lib.lib().soar_unet_workspace_bytes(C.byref(netb._c), 3, 8, 10, 7, 0, C.byref(nb)) == 1 and "level 1 is 4 x 5" in hip_lib.last_error()
    assert hip_lib.lib().soar_unet_workspace_bytes(C.byref(net._c), 6, 8, 8, 7, 3, C.byref(nb)) == 1 and "multiple of n_view" in hip_lib.last_error()


def test_guidance_matches_the_restatement_as_eps_fn():
    """MultiviewGuidance (encoder, UNet and loss tail in HIP) against MultiviewSDS with the float64 restatement as its eps_fn; the
    float32 restatement as eps_fn gives e32"""
    import vae_ref
    from soar_amd import sds
    cfg, sd, net, _, _, _ = setup("A")
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
    seen = []

    def image_tokens(img):
        seen.append(img)
        return tokens, torch.zeros_like(tokens)

    args = dict(guidance_scale=5.0, n_view=4, recon_loss=True, recon_std_rescale=0.2, image_size=S)
    guide = sds.MultiviewGuidance(enc, net, text, image_tokens=image_tokens, **args).to(DEV)
    # the context, built here: text rows per view, cameras for both halves, image tokens and zeros
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

    def restated(dtype):
        plain = sds.MultiviewSDS(enc, **args).to(DEV)
        eps_fn = lambda x_in, tt: R.forward(sd, cfg, x_in.cpu(), tt.cpu(), ctx.cpu(), cam2.cpu(), ip.cpu(), dtype=dtype)[0].to(DEV)
        return result(lambda x: plain(x, eps_fn, t=t, noise=noise, posterior_noise=post))

    loss, grad = result(lambda x: guide(x, c2w=c2w, ref_rgb=ref_rgb, t=t, noise=noise, posterior_noise=post, elevation=None))
    assert len(seen) == 1 and seen[0] is ref_rgb
    l64, g64 = restated(torch.float64)
    l32, g32 = restated(torch.float32)
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    within("guidance loss_sds", loss, l64.double(), l32)
    within("guidance image gradient", grad, g64.double(), g32)
