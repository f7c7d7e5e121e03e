"""The SDS guidance's conditioning on the device (soar_amd/clip.py, csrc/clip.hip, csrc/attention.hip) against the
plain-torch restatement of tests/clip_ref.py in float64.

Tolerance, measured not fixed (the bar of tests/test_sam_gpu.py and tests/test_unet_gpu.py): for every compared tensor ``e32`` is the
distance of the restatement run in float32 from the restatement run in float64 (worst element over the float64 tensor's RMS), and the
kernels must lie within ``4 e32`` of float64: the factor covers another order of accumulation over the same float32 operands.  Where
``e32`` is 0, equality is required.  The towers' restatement is held against transformers' CLIP in tests/test_clip_cpu.py; the
Resampler's has no independent implementation to be held against.

The configurations (tests/clip_ref.py) are the smallest at which the kernels can still go wrong.  Text A: a head dimension padded to 32,
one key tile, L = 13 and 5.  Text B: L = 77 is three key tiles, the last partial, with the causal diagonal inside tiles; L = 150 puts
the mask across the boundary of the 128-query tile.  Vision A: head dimension 80 (the 96-wide instantiation), 26 tokens, K = 588 padded
to 592.  Vision B: 145 tokens, a full query tile and a tail.  Resampler A: 5 queries over 31 keys; B: 16 queries over 161 keys, a
partial last tile.
"""
import pytest
import torch

import clip_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FACTOR = 4.0
_cache = {}


def rel(a, b):
    """worst element of a - b over b's RMS (b: float64)"""
    return float((a.double().cpu() - b.cpu()).abs().max() / b.cpu().pow(2).mean().sqrt())


def within(name, got, ref64, ref32):
    e32 = rel(ref32, ref64)
    err = rel(got, ref64)
    print(f"{name}: err {err:.3g}  e32 {e32:.3g}  ratio {err / e32 if e32 else float('inf' if err else 0):.2f}")
    assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
    assert err <= FACTOR * e32, f"{name}: {err:.3g} from float64, float32 restatement {e32:.3g}: ratio {err / e32 if e32 else float('inf'):.2f} > {FACTOR}"


def text(name):
    if ("text", name) not in _cache:
        from soar_amd import clip
        cfg = {"A": R.TEXT_A, "B": R.TEXT_B}[name]
        sd = R.tiny_state_dict(R.text_shapes(cfg), 10)
        _cache[("text", name)] = (cfg, sd, clip.ClipTextEncoder(sd, heads=cfg["heads"]).to(DEV))
    return _cache[("text", name)]


def vision(name):
    if ("vision", name) not in _cache:
        from soar_amd import clip
        cfg = {"A": R.VISION_A, "B": R.VISION_B}[name]
        sd = R.tiny_state_dict(R.vision_shapes(cfg), 20)
        _cache[("vision", name)] = (cfg, sd, clip.ClipImageEncoder(sd, heads=cfg["heads"]).to(DEV))
    return _cache[("vision", name)]


def resampler(name):
    if ("resampler", name) not in _cache:
        from soar_amd import clip
        cfg = {"A": R.RESAMPLER_A, "B": R.RESAMPLER_B}[name]
        sd = R.tiny_state_dict(R.resampler_shapes(cfg), 30)
        _cache[("resampler", name)] = (cfg, sd, clip.Resampler(sd, dim_head=cfg["dim_head"]).to(DEV))
    return _cache[("resampler", name)]


def ids_of(cfg, B, L, seed=0):
    return torch.randint(0, cfg["vocab"], (B, L), generator=torch.Generator().manual_seed(100 * L + seed))


@pytest.mark.parametrize("name,L", [("A", 13), ("A", 5), ("B", 77), ("B", 150)])
def test_text_stage_by_stage(name, L):
    cfg, sd, net = text(name)
    ids = ids_of(cfg, 2, L)
    probes = [("embed", ""), (0, "attn"), (0, "block"), (cfg["layers"] - 1, "attn"), (cfg["layers"] - 1, "block")]
    out, taps = net(ids.to(DEV), probes=probes)
    torch.cuda.synchronize()
    o64, s64 = R.text_forward(sd, cfg, ids, torch.float64)
    o32, s32 = R.text_forward(sd, cfg, ids, torch.float32)
    for key in probes:
        within(f"text {name} L={L} {key}", taps[key], s64[key], s32[key])
    within(f"text {name} L={L} out", out, o64, o32)


def test_text_skip_last_and_open_clip_layout():
    """the open_clip layout's default leaves the last block out; the same weights in either layout give the same bits"""
    from soar_amd import clip
    cfg, sd, net = text("A")
    ids = ids_of(cfg, 2, 13)
    oc = clip.ClipTextEncoder(R.to_open_clip_text(sd, cfg, "cond_stage_model.model."), heads=cfg["heads"]).to(DEV)
    assert oc.skip_last == 1
    out = oc(ids.to(DEV))
    within("text A penultimate", out, R.text_forward(sd, cfg, ids, torch.float64, skip_last=1)[0], R.text_forward(sd, cfg, ids, torch.float32, skip_last=1)[0])
    assert torch.equal(out, clip.ClipTextEncoder(sd, heads=cfg["heads"], skip_last=1).to(DEV)(ids.to(DEV)))
    both = clip.encode_prompts(net, ids[0].to(DEV), ids[1:2].to(DEV))
    assert both.shape == (2, 13, cfg["width"]) and torch.equal(both, net(ids.to(DEV)))


def image_of(cfg, seed=0, B=1):
    """uint8 [B, 41, 59, 3]: both sides are resized, by different factors"""
    return torch.stack([R.sample_image(41, 59, seed + b) for b in range(B)])


@pytest.mark.parametrize("name", ["A", "B"])
def test_vision_stage_by_stage(name):
    cfg, sd, net = vision(name)
    img = image_of(cfg, 3, B=2)
    probes = [("embed", ""), ("pre", ""), (0, "attn"), (0, "block"), (cfg["layers"] - 1, "block")]
    out, taps = net(img.to(DEV), probes=probes)
    torch.cuda.synchronize()
    u8 = R.resized(img, cfg["image"])
    o64, s64 = R.vision_forward(sd, cfg, R.normalized(u8, torch.float64), torch.float64)
    o32, s32 = R.vision_forward(sd, cfg, R.normalized(u8, torch.float32), torch.float32)
    assert out.shape == (2, R.tokens_of(cfg), cfg["width"])
    for key in probes:
        within(f"vision {name} {key}", taps[key], s64[key], s32[key])
    within(f"vision {name} out", out, o64, o32)


def test_vision_skip_last_and_post_norm():
    from soar_amd import clip
    cfg, sd, _ = vision("A")
    img = image_of(cfg, 5)
    u8 = R.resized(img, cfg["image"])
    net = clip.ClipImageEncoder(R.to_open_clip_vision(sd, cfg, "model."), skip_last=1, post_norm=True, heads=cfg["heads"]).to(DEV)
    ref = lambda dt: R.vision_forward(sd, cfg, R.normalized(u8, dt), dt, skip_last=1, post_norm=True)[0]
    within("vision A skip_last=1 post_norm", net(img.to(DEV)), ref(torch.float64), ref(torch.float32))


@pytest.mark.parametrize("name", ["A", "B"])
def test_resampler_stage_by_stage(name):
    cfg, sd, net = resampler(name)
    n = {"A": 26, "B": 145}[name]
    x = torch.randn(2, n, cfg["emb"], generator=torch.Generator().manual_seed(n))
    probes = [(i, s) for i in range(cfg["depth"]) for s in ("attn", "ff")]
    out, taps = net(x.to(DEV), probes=probes)
    torch.cuda.synchronize()
    o64, s64 = R.resampler_forward(sd, cfg, x, torch.float64)
    o32, s32 = R.resampler_forward(sd, cfg, x, torch.float32)
    for key in probes:
        within(f"resampler {name} {key}", taps[key], s64[key], s32[key])
    within(f"resampler {name} norm_out", out, o64, o32)


ATTN_CASES = [(1, 1, 80, 1, False), (5, 5, 32, 2, True), (77, 77, 64, 3, True), (150, 150, 64, 2, True), (26, 26, 80, 2, False),
              (257, 257, 80, 2, False), (16, 273, 64, 3, False), (5, 31, 32, 2, False)]


@pytest.mark.parametrize("Lq,Lk,hd,heads,causal", ATTN_CASES)
def test_attention_kernel_alone(Lq, Lk, hd, heads, causal):
    """one key, a causal tile, the diagonal inside tiles and across the query tile's boundary, head dimension 80 with one and with
    several query tiles, a few queries over many keys.  The sources are slices of wider rows, so every pointer has its own pitch."""
    from soar_amd import clip
    B, C = 2, heads * hd
    g = torch.Generator().manual_seed(Lq * 1000 + Lk)
    q = torch.randn(B, Lq, C, generator=g) * 1.5
    kv = torch.randn(B, Lk, 2 * C + 4, generator=g)
    k, v = kv[..., :C], kv[..., C:2 * C]
    ref = lambda dt: R.attention(q.to(dt), k.to(dt), v.to(dt), heads, causal=causal)
    kvd = kv.to(DEV)
    out = clip.attention(q.to(DEV), kvd[..., :C], kvd[..., C:2 * C], heads, causal=causal)
    again = clip.attention(q.to(DEV), kvd[..., :C], kvd[..., C:2 * C], heads, causal=causal)
    torch.cuda.synchronize()
    assert torch.equal(out, again)
    within(f"attention Lq={Lq} Lk={Lk} hd={hd} heads={heads} causal={causal}", out, ref(torch.float64), ref(torch.float32))


@pytest.mark.parametrize("p", [31, 32, 76])
def test_causality_is_exact(p):
    """changing the tokens behind position p leaves the rows up to p bit-equal: a mask that is off by one at a tile's edge fails here,
    where a tolerance could hide it"""
    cfg, sd, net = text("B")
    ids = ids_of(cfg, 1, 150)
    other = ids.clone()
    other[:, p + 1:] = (ids[:, p + 1:] + 1 + torch.arange(150 - p - 1) % 7) % cfg["vocab"]
    assert not torch.equal(ids[:, p + 1:], other[:, p + 1:])
    a, b = net(ids.to(DEV)), net(other.to(DEV))
    assert torch.equal(a[:, :p + 1], b[:, :p + 1])
    assert not torch.equal(a[:, p + 1], b[:, p + 1])


def test_batch_independence_and_repeatability():
    cfg, sd, net = text("B")
    ids = ids_of(cfg, 3, 77).to(DEV)
    both = net(ids)
    assert torch.equal(both, net(ids))
    for b in range(3):
        assert torch.equal(net(ids[b:b + 1]), both[b:b + 1]), b
    for name in ("A", "B"):
        vcfg, _, vnet = vision(name)
        img = image_of(vcfg, 7, B=3).to(DEV)
        vboth = vnet(img)
        assert torch.equal(vboth, vnet(img))
        for b in range(3):
            assert torch.equal(vnet(img[b]), vboth[b:b + 1]), (name, b)
    for name, n in (("A", 26), ("B", 145)):
        rcfg, _, rnet = resampler(name)
        x = torch.randn(3, n, rcfg["emb"], generator=torch.Generator().manual_seed(1)).to(DEV)
        rboth = rnet(x)
        assert torch.equal(rboth, rnet(x))
        for b in range(3):
            assert torch.equal(rnet(x[b:b + 1]), rboth[b:b + 1]), (name, b)


@pytest.mark.parametrize("as_float", [True, False])
def test_preprocessing_is_exact(as_float):
    """37 x 83 -> 70 x 70: the device's patch rows equal the restatement's (to_pil_image's truncation, Pillow's bicubic bytes, to_tensor
    and Normalize in float32, the patch windows, the zero padding) bit for bit"""
    cfg, _, net = vision("A")
    img = R.sample_image(37, 83, 9, as_float=as_float)
    u8 = net.resized(img.to(DEV))
    want_u8 = R.resized(img, 70)
    assert torch.equal(u8.cpu(), want_u8)
    rows = net.preprocess(img.to(DEV))
    assert rows.shape == (1, 25, 592)
    assert torch.equal(rows.cpu(), R.patch_rows(R.normalized(want_u8), 14))


def test_refusals_on_the_device():
    from soar_amd import clip, hip_lib
    cfg, _, net = text("A")
    ids = ids_of(cfg, 1, 13).to(DEV)
    with pytest.raises(hip_lib.SoarHipError, match=r"workspace of 1024 bytes, need \d+ \(soar_clip_workspace_bytes\)"):
        net(ids, workspace=hip_lib._workspace(1024, DEV))
    _, _, rnet = resampler("A")
    with pytest.raises(hip_lib.SoarHipError, match=r"workspace of 1024 bytes, need \d+ \(soar_resampler_workspace_bytes\)"):
        rnet(torch.zeros(1, 26, 160, device=DEV), workspace=hip_lib._workspace(1024, DEV))
    with pytest.raises(ValueError, match=r"x must be float \[B, n, 160\]"):
        rnet(torch.zeros(1, 26, 64, device=DEV))
    q = torch.zeros(1, 5, 64, device=DEV)
    with pytest.raises(hip_lib.SoarHipError, match="a causal mask needs one key set and Lq = Lk"):
        clip.attention(q, torch.zeros(1, 7, 64, device=DEV), torch.zeros(1, 7, 64, device=DEV), 2, causal=True)
    with pytest.raises(RuntimeError, match="move the module"):
        clip.ClipTextEncoder(R.tiny_state_dict(R.text_shapes(cfg), 0), heads=2)(ids)


def test_guidance_with_the_conditioning_in_the_library():
    """MultiviewGuidance fed by ImageTokens and encode_prompts against the same guidance fed the float64 restatement's embeddings and
    tokens; the float32 restatement's give e32.  The text width and the Resampler's output are the tiny UNet's context_dim."""
    import unet_ref
    import vae_ref
    from soar_amd import clip, sds, unet
    ucfg = unet_ref.CONFIG_A
    ctx = ucfg["context_dim"]
    net = unet.MultiviewUNet(unet_ref.tiny_state_dict(ucfg, 0), num_head_channels=ucfg["num_head_channels"], ip_dim=ucfg["ip_dim"],
                             ip_weight=ucfg["ip_weight"], n_view=ucfg["n_view"]).to(DEV)
    tcfg = dict(width=ctx, heads=2, layers=1, mlp=2 * ctx, context=ucfg["T"], vocab=50)
    tsd = R.tiny_state_dict(R.text_shapes(tcfg), 40)
    vcfg, vsd, vnet = vision("A")
    rcfg = dict(R.RESAMPLER_A, depth=1, queries=ucfg["ip_dim"], out=ctx)
    rsd = R.tiny_state_dict(R.resampler_shapes(rcfg), 41)
    tnet = clip.ClipTextEncoder(tsd, heads=2).to(DEV)
    tokens = clip.ImageTokens(vnet, clip.Resampler(rsd, dim_head=rcfg["dim_head"]).to(DEV))

    B, S = 4, 64
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(0, 50, (2, ucfg["T"]), generator=g)
    ref_rgb = R.sample_image(37, 83, 13, as_float=True)
    enc = sds.LatentEncoder(vae_ref.random_weights(0)).to(DEV)
    rgb = torch.rand(B, 40, 48, 3, generator=g).to(DEV)
    c2w = torch.randn(B, 4, 4, generator=g).to(DEV)
    noise, post = (torch.randn(B, 4, S // 8, S // 8, generator=g).to(DEV) for _ in range(2))
    t = torch.tensor([431], device=DEV)
    args = dict(guidance_scale=5.0, n_view=4, recon_loss=True, recon_std_rescale=0.2, image_size=S)

    cond, uncond = tokens(ref_rgb.to(DEV))
    assert cond.shape == (ucfg["ip_dim"], ctx) and uncond.shape == cond.shape and float(uncond.abs().max()) == 0 and float(cond.abs().max()) > 0

    def result(guide):
        x = rgb.clone().requires_grad_(True)
        out = guide(x, c2w=c2w, ref_rgb=ref_rgb.to(DEV), t=t, noise=noise, posterior_noise=post)
        out["loss_sds"].backward()
        torch.cuda.synchronize()
        return out["loss_sds"].detach().reshape(1), x.grad

    def restated(dtype):
        emb = R.text_forward(tsd, tcfg, ids, dtype)[0]
        px = R.normalized(R.resized(ref_rgb, vcfg["image"]), dtype)
        tok = R.resampler_forward(rsd, rcfg, R.vision_forward(vsd, vcfg, px, dtype)[0], dtype)[0][0].to(torch.float32).to(DEV)
        return result(sds.MultiviewGuidance(enc, net, emb.to(torch.float32).to(DEV), image_tokens=lambda img: (tok, torch.zeros_like(tok)), **args).to(DEV))

    text_embeddings = clip.encode_prompts(tnet, ids[0].to(DEV), ids[1].to(DEV))
    loss, grad = result(sds.MultiviewGuidance(enc, net, text_embeddings, image_tokens=tokens, **args).to(DEV))
    l64, g64 = restated(torch.float64)
    l32, g32 = restated(torch.float32)
    assert float(l64) > 0 and float(g64.abs().max()) > 0
    within("guidance loss_sds", loss, l64.double(), l32)
    within("guidance image gradient", grad, g64.double(), g32)
