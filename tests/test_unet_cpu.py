"""CPU tests of the multi-view diffusion UNet's restatement (tests/unet_ref.py) and of soar_amd/unet.py's host side: the pieces of
the restatement against torch.nn.functional, the multi-view properties of the definition, the size inference and the refusals."""
import math

import pytest
import torch
import torch.nn.functional as F

import unet_ref as R

CFGS = {"A": R.CONFIG_A, "B": R.CONFIG_B}


def _close(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def test_restated_pieces_agree_with_torch_functional_in_float64():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 96, 5, 7, generator=g, dtype=torch.float64) * 2 + 0.5
    w, b = torch.randn(96, generator=g, dtype=torch.float64), torch.randn(96, generator=g, dtype=torch.float64)
    for eps in (1e-5, 1e-6):
        _close(R.group_norm(x, w, b, eps), F.group_norm(x, 32, w, b, eps))
    tok = torch.randn(2, 11, 96, generator=g, dtype=torch.float64)
    _close(R.layer_norm(tok, w, b), F.layer_norm(tok, (96,), w, b, 1e-5))
    _close(R.silu(tok), F.silu(tok))
    _close(R.gelu_erf(tok), F.gelu(tok))
    a, gate = tok.chunk(2, dim=-1)
    _close(R.geglu(tok), a * F.gelu(gate))
    q, k, v = (torch.randn(2, n, 96, generator=g, dtype=torch.float64) for n in (11, 5, 5))
    heads = 3
    sp = lambda t: t.reshape(2, -1, heads, 32).transpose(1, 2)
    ref = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).transpose(1, 2).reshape(2, 11, 96)
    _close(R.attention(q, k, v, heads), ref)
    t = torch.tensor([0, 1, 500, 999])
    e = R.time_embedding(t, 32, torch.float64)
    assert e.shape == (4, 32) and torch.equal(e[0], torch.cat([torch.ones(16), torch.zeros(16)]).double())
    assert abs(float(e[3, 15]) - math.cos(999 * math.exp(-math.log(10000.0) * 15 / 16))) < 1e-12


@pytest.fixture(scope="module")
def case_a():
    cfg = R.CONFIG_A
    sd = R.tiny_state_dict(cfg, 0)
    x, t, ctx, cam, ip = R.inputs(cfg, 0)
    # the views of a group share t, as in the guidance
    t = t[:: cfg["n_view"]].repeat_interleave(cfg["n_view"])
    return cfg, sd, x, t, ctx, cam, ip


def test_permuting_the_views_of_a_group_permutes_eps(case_a):
    cfg, sd, x, t, ctx, cam, ip = case_a
    eps, _ = R.forward(sd, cfg, x, t, ctx, cam, ip)
    perm = torch.tensor([2, 0, 3, 1, 4, 5, 6, 7])                # inside the first group only
    eps_p, _ = R.forward(sd, cfg, x[perm], t[perm], ctx[perm], cam[perm], ip[perm])
    _close(eps_p, eps[perm], 1e-10)
    assert float((eps_p - eps).abs().max()) > 1e-3               # and the views do differ


def test_zero_to_v_ip_equals_no_image_tokens(case_a):
    cfg, sd, x, t, ctx, cam, ip = case_a
    zeroed = {k: (torch.zeros_like(v) if k.endswith("to_v_ip.weight") else v) for k, v in sd.items()}
    a, _ = R.forward(zeroed, cfg, x, t, ctx, cam, ip)
    b, _ = R.forward(sd, cfg, x, t, ctx, cam, None)
    c, _ = R.forward(sd, cfg, x, t, ctx, cam, ip)
    _close(a, b, 1e-12)
    assert float((c - b).abs().max()) > 1e-4


def test_one_view_is_the_plain_sd_path():
    """n_view = 1: every latent is its own group, so a batch is its samples one by one"""
    cfg = R.CONFIG_B
    sd = R.tiny_state_dict(cfg, 1)
    x, t, ctx, cam, ip = R.inputs(cfg, 1)
    assert cam is None and ip is None
    eps, st = R.forward(sd, cfg, x, t, ctx)
    assert eps.shape == x.shape and st[("output_blocks.2", "up")].shape == (3, 128, 4, 6) and ("output_blocks.2", "attn1") not in st
    assert "output_blocks.2.1.conv.weight" in sd and "output_blocks.5.2.conv.weight" in sd
    for n in range(cfg["N"]):
        one, _ = R.forward(sd, cfg, x[n:n + 1], t[n:n + 1], ctx[n:n + 1])
        _close(one, eps[n:n + 1], 1e-11)


def test_concatenation_straddles_groups_in_a():
    cfg = R.CONFIG_A
    ins, mid, outs = R.layout(cfg)
    assert [b["cin"] for b in outs] == [128, 96, 96, 64] and outs[1]["cin"] // 32 == 3 and 64 % 3 != 0


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("prefix", ["", "model.diffusion_model."])
def test_size_inference(name, prefix):
    from soar_amd import unet
    cfg = CFGS[name]
    sd = {prefix + k: v for k, v in R.tiny_state_dict(cfg, 2).items()}
    sd["first_stage_model.encoder.conv_in.weight"] = torch.zeros(3)
    sd[prefix + "image_embed.latents"] = torch.zeros(3)
    got = unet.infer_config(unet.strip_prefix(sd))
    for k in ("in_channels", "out_channels", "model_channels", "channel_mult", "num_res_blocks", "attention", "context_dim", "camera_dim", "with_ip"):
        assert got[k] == cfg[k], (k, got[k], cfg[k])
    m = unet.MultiviewUNet(sd, num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"], n_view=cfg["n_view"])
    shapes = R.state_dict_shapes(cfg)
    keys = unet.tensor_keys(m.cfg)
    assert {k for k, _ in keys} == set(shapes) and all(tuple(s) == shapes[k] for k, s in keys)
    assert m.weights.numel() == sum(math.prod(s) for s in shapes.values())
    ins, _, outs = R.layout(cfg)
    assert m.blocks == [f"input_blocks.{i}" for i in range(len(ins))] + ["middle_block"] + [f"output_blocks.{i}" for i in range(len(outs))]


@pytest.mark.parametrize("name", ["A", "B"])
def test_missing_or_misshapen_keys_are_refused_by_name(name):
    from soar_amd import unet
    cfg = CFGS[name]
    sd = R.tiny_state_dict(cfg, 3)
    for key in ("time_embed.2.bias", "input_blocks.1.0.in_layers.2.weight", "middle_block.1.transformer_blocks.0.attn2.to_v.weight",
                "output_blocks.1.0.emb_layers.1.weight", "out.2.weight", "middle_block.1.transformer_blocks.0.ff.net.2.weight"):
        bad = dict(sd)
        del bad[key]
        with pytest.raises(KeyError, match=key.replace(".", r"\.")):
            unet.MultiviewUNet(bad, num_head_channels=cfg["num_head_channels"], n_view=cfg["n_view"])
        bad = dict(sd)
        bad[key] = torch.zeros(tuple(sd[key].shape) + (1,)) if sd[key].dim() == 1 else sd[key][..., :-1]
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            unet.MultiviewUNet(bad, num_head_channels=cfg["num_head_channels"], n_view=cfg["n_view"])
    with pytest.raises(KeyError, match="input_blocks"):
        unet.MultiviewUNet({})


def test_head_channels_must_divide_the_widths():
    from soar_amd import hip_lib, unet
    with pytest.raises(hip_lib.SoarHipError, match="head_channels"):
        unet.MultiviewUNet(R.tiny_state_dict(R.CONFIG_A, 0), num_head_channels=24)


def test_normalize_camera_is_its_formula():
    from soar_amd import unet
    g = torch.Generator().manual_seed(4)
    c2w = torch.randn(5, 4, 4, generator=g)
    got = unet.normalize_camera(c2w)
    assert got.shape == (5, 16)
    for b in range(5):
        want = c2w[b].clone()
        want[:3, 3] = c2w[b, :3, 3] / (torch.sqrt((c2w[b, :3, 3] ** 2).sum()) + 1e-8)
        assert torch.allclose(got[b], want.reshape(16), rtol=1e-6, atol=0)
    assert torch.equal(unet.normalize_camera(torch.zeros(1, 4, 4)), torch.zeros(1, 16))
    assert torch.equal(c2w, torch.randn(5, 4, 4, generator=torch.Generator().manual_seed(4)))    # the input is left alone


def test_cpu_tensors_are_refused():
    from soar_amd import sds, unet
    import vae_ref
    cfg = R.CONFIG_A
    m = unet.MultiviewUNet(R.tiny_state_dict(cfg, 0), num_head_channels=16, ip_dim=3)
    x, t, ctx, cam, ip = R.inputs(cfg, 0)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        m(x, t, ctx, camera=cam, ip_tokens=ip)
    g = sds.MultiviewGuidance(sds.LatentEncoder(vae_ref.random_weights(0)), m, torch.zeros(2, 7, 40), image_size=64)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        g(torch.zeros(4, 64, 64, 3), c2w=torch.eye(4).repeat(4, 1, 1))
    g.set_step_range(0.1, 0.5)
    assert (g.sds.min_step, g.sds.max_step) == (100, 500)
    with pytest.raises(ValueError, match="text_embeddings"):
        sds.MultiviewGuidance(sds.LatentEncoder(vae_ref.random_weights(0)), m, torch.zeros(2, 7, 48))
