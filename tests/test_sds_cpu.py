"""CPU tests of the SDS guidance's encoder and loss tail (soar_amd/sds.py, csrc/vae.hip): the float64 restatement
(tests/vae_ref.py) against autograd's numerical gradient at a narrow width, the state-dict checks, the schedule, and the refusals of
the C ABI (no kernel launches: there is no GPU in this container)."""
import ctypes as C

import pytest
import torch

import vae_ref as R
from soar_amd import sds


def test_restatement_gradient_passes_gradcheck():
    w = R.cast(R.random_weights(0, ch=32), torch.float64)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(1, 3, 16, 16, generator=g, dtype=torch.float64, requires_grad=True)
    eps = torch.randn(1, 4, 2, 2, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda v: R.latents(v, w, 16, eps), (x,), fast_mode=True)
    # through a non-integer resize too
    x2 = torch.rand(1, 3, 13, 19, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda v: R.latents(v, w, 16, eps), (x2,), fast_mode=True)


def test_restatement_gradient_passes_gradcheck_off_grid_with_a_peaked_attention():
    """the oracle of the GPU suite's off-grid cases at T = 9 (11 x 9 -> 24: upsampling both ways), with the attention gain that suite
    uses at this size; the softmax it exposes is the one the network applies"""
    w = R.cast(R.random_weights(0, ch=32, attn_gain=1.5), torch.float64)
    plain = R.random_weights(0, ch=32)
    for k, v in R.random_weights(0, ch=32, attn_gain=1.5).items():
        gain = 1.5 if k in ("encoder.mid.attn_1.q.weight", "encoder.mid.attn_1.k.weight") else 1.0
        assert torch.equal(v, plain[k] * gain), k
    g = torch.Generator().manual_seed(2)
    x = torch.rand(2, 3, 11, 9, generator=g, dtype=torch.float64, requires_grad=True)
    eps = torch.randn(2, 4, 3, 3, generator=g, dtype=torch.float64)
    assert torch.autograd.gradcheck(lambda v: R.latents(v, w, 24, eps), (x,), fast_mode=True)
    with torch.no_grad():
        P = R.attention_probs(x, w, 24)
        Pp = R.attention_probs(x, R.cast(plain, torch.float64), 24)
    assert P.shape == (2, 9, 9) and torch.allclose(P.sum(2), torch.ones(2, 9, dtype=torch.float64), atol=1e-12)
    assert float(P.max(2).values.mean()) > float(Pp.max(2).values.mean())


def test_restatement_activations_stay_order_one():
    w = R.cast(R.random_weights(0), torch.float64)
    x = R.images(1, 64, 64, 3).double()
    mean, logvar = R.moments(x, w, 64)
    assert mean.shape == (1, 4, 8, 8)
    assert 0.05 < float(mean.abs().mean()) < 20 and float(logvar.abs().max()) < 20


def test_the_key_list_matches_the_library_order():
    assert [(k, tuple(s)) for k, s in sds.WEIGHT_ORDER] == [(k, tuple(s)) for k, s in R.keys(128)]
    n3 = sum(1 for k, s in sds.WEIGHT_ORDER if len(s) == 4 and s[2] == 3)
    n1 = sum(1 for k, s in sds.WEIGHT_ORDER if len(s) == 4 and s[2] == 1)
    assert (n3, n1) == (25, 7)


def test_state_dict_prefix_is_accepted_and_extra_keys_ignored():
    sd = R.random_weights(2)
    m1 = sds.LatentEncoder(sd)
    pre = {"first_stage_model." + k: v for k, v in sd.items()}
    pre["first_stage_model.decoder.conv_in.weight"] = torch.zeros(3)
    pre["model.diffusion_model.out.0.weight"] = torch.zeros(2)
    m2 = sds.LatentEncoder(pre)
    assert torch.equal(m1.weights, m2.weights) and m1.weights.dtype == torch.float32
    assert m1.weights.numel() == sum(v.numel() for v in sd.values())
    assert torch.equal(m1.weights[:128 * 27], sd["encoder.conv_in.weight"].reshape(-1))
    assert m1.scale_factor == pytest.approx(0.18215) and not m1.training


def test_missing_or_misshapen_keys_are_refused_by_name():
    sd = R.random_weights(3)
    bad = dict(sd)
    del bad["encoder.mid.attn_1.k.bias"]
    with pytest.raises(KeyError, match=r"encoder\.mid\.attn_1\.k\.bias"):
        sds.LatentEncoder(bad)
    bad = {"first_stage_model." + k: v for k, v in sd.items()}
    del bad["first_stage_model.quant_conv.weight"]
    with pytest.raises(KeyError, match=r"first_stage_model\.quant_conv\.weight"):
        sds.LatentEncoder(bad)
    bad = dict(sd)
    bad["encoder.down.1.block.0.nin_shortcut.weight"] = torch.zeros(256, 128, 3, 3)
    with pytest.raises(ValueError, match=r"encoder\.down\.1\.block\.0\.nin_shortcut\.weight"):
        sds.LatentEncoder(bad)
    with pytest.raises(KeyError, match=r"encoder\.conv_in\.weight"):
        sds.LatentEncoder({})


def test_schedule_is_ldms():
    ac = sds.ldm_schedule()
    assert ac.dtype == torch.float64 and ac.shape == (1000,)
    betas = 1 - ac / torch.cat([torch.ones(1, dtype=torch.float64), ac[:-1]])
    assert float(betas[0]) == pytest.approx(0.00085, rel=1e-9) and float(betas[-1]) == pytest.approx(0.012, rel=1e-9)
    tb = sds.schedule_tables(ac)
    ref = R.tables(R.ldm_alphas_cumprod())
    for i, k in enumerate(("sqrt_ac", "sqrt_1m_ac", "sqrt_recip_ac", "sqrt_recipm1_ac", "ac")):
        assert torch.equal(tb[i], ref[k]), k
    m = sds.MultiviewSDS(sds.LatentEncoder(R.random_weights(0)))
    assert (m.min_step, m.max_step) == (20, 750)
    m.set_step_range(0.02, 0.5)
    assert m.max_step == 500


def test_inputs_are_refused_before_anything_runs():
    enc = sds.LatentEncoder(R.random_weights(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(1, 3, 64, 64))
    with pytest.raises(ValueError, match="N, 3, H, W"):
        enc(torch.zeros(1, 4, 64, 64))
    m = sds.MultiviewSDS(enc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(4, 64, 64, 3), lambda x, t: x)
    with pytest.raises(ValueError, match="B, H, W, 3"):
        m(torch.zeros(4, 3, 64, 64), lambda x, t: x)


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_workspace_sizing_refuses_bad_sizes_and_grows(lib):
    from soar_amd import hip_lib
    n = C.c_size_t(0)
    assert lib.soar_vae_workspace_bytes(-1, 64, 64, 64, C.byref(n)) != 0 and "N must be >= 0" in hip_lib.last_error()
    assert lib.soar_vae_workspace_bytes(1, 64, 64, 60, C.byref(n)) != 0 and "multiple of 8" in hip_lib.last_error()
    assert lib.soar_vae_workspace_bytes(1, 64, 64, 0, C.byref(n)) != 0 and "multiple of 8" in hip_lib.last_error()
    assert lib.soar_vae_workspace_bytes(1, 0, 64, 64, C.byref(n)) != 0 and "positive" in hip_lib.last_error()
    assert lib.soar_vae_workspace_bytes(1, 64, 64, 64, None) != 0 and "NULL" in hip_lib.last_error()
    sizes = {}
    for N, S in [(1, 64), (2, 64), (1, 256), (4, 256)]:
        assert lib.soar_vae_workspace_bytes(N, 300, 260, S, C.byref(n)) == 0
        assert n.value % 256 == 0
        sizes[N, S] = n.value
    assert sizes[2, 64] > sizes[1, 64] and sizes[1, 256] > sizes[1, 64] and sizes[4, 256] > 3 * sizes[1, 256]
    # the forward keeps every activation of level 0 (5 x 128 channels) plus three gradient buffers
    assert sizes[1, 256] > 4 * 8 * 128 * 256 * 256
    assert lib.soar_vae_workspace_bytes(0, 64, 64, 64, C.byref(n)) == 0 and n.value >= 256
    # image_size 72 has 81 attention tokens, padded to 128: its size lies strictly between those of 64 and 80 ...
    by_size = {}
    for S in (64, 72, 80, 88):
        assert lib.soar_vae_workspace_bytes(2, 50, 90, S, C.byref(n)) == 0
        by_size[S] = n.value
    assert by_size[64] < by_size[72] < by_size[80] < by_size[88]
    # ... and the padded attention buffers are counted with T_pad, not T.  Everything else grows linearly with the pixel count (72
    # and 88 share T_pad = 128 and give the slope); what is left of 72 over 64 is the step of ten [T_pad][512] and three
    # [T_pad][T_pad] buffers from T_pad = 64 to 128 (2.9 MB at N = 2; 0.8 MB if T were counted), up to the 256-byte roundings
    slope = (by_size[88] - by_size[72]) / (88 ** 2 - 72 ** 2)
    step = (by_size[72] - slope * 72 ** 2) - (by_size[64] - slope * 64 ** 2)
    attn_bytes = lambda tp: 2 * 4 * (10 * tp * 512 + 3 * tp * tp)
    assert abs(step - (attn_bytes(128) - attn_bytes(64))) < 64 * 1024, step
    assert lib.soar_vae_weights_floats(C.byref(n)) == 0
    assert n.value == sum(int(torch.tensor(s).prod()) for _, s in R.keys(128)) == 34163664
    assert lib.soar_vae_weights_bytes(C.byref(n)) == 0 and n.value > 4 * 34163664 and n.value % 256 == 0


def test_entries_refuse_bad_arguments_without_touching_the_gpu(lib):
    from soar_amd import hip_lib
    assert lib.soar_vae_forward(None, None, 0, None) != 0 and "NULL args" in hip_lib.last_error()
    a = hip_lib.SoarVaeArgs()
    a.N, a.H, a.W, a.image_size = 1, 64, 64, 64
    assert lib.soar_vae_forward(C.byref(a), None, 0, None) != 0 and "NULL weights" in hip_lib.last_error()
    a.weights = 0x100000
    assert lib.soar_vae_forward(C.byref(a), None, 0, None) != 0 and "workspace" in hip_lib.last_error()
    assert lib.soar_vae_backward(C.byref(a), 0x100000, 8, None) != 0 and "workspace" in hip_lib.last_error()
    # one byte short at a size with a padded attention: refused by both entries, by size, before any device call
    n = C.c_size_t(0)
    a.N, a.H, a.W, a.image_size = 2, 50, 90, 72
    assert lib.soar_vae_workspace_bytes(2, 50, 90, 72, C.byref(n)) == 0
    for entry in (lib.soar_vae_forward, lib.soar_vae_backward):
        assert entry(C.byref(a), 0x100000, n.value - 1, None) != 0
        assert f"workspace of {n.value - 1} bytes, need {n.value} (soar_vae_workspace_bytes)" in hip_lib.last_error()
    assert lib.soar_vae_forward(C.byref(a), 0x100000, n.value, None) != 0 and "NULL x" in hip_lib.last_error()
    a.N, a.H, a.W, a.image_size = 1, 64, 64, 64
    a.image_size = 36
    assert lib.soar_vae_forward(C.byref(a), None, 0, None) != 0 and "multiple of 8" in hip_lib.last_error()
    a.image_size, a.N = 64, -2
    assert lib.soar_vae_backward(C.byref(a), None, 0, None) != 0 and "N must be >= 0" in hip_lib.last_error()
    a.N = 1
    assert lib.soar_vae_forward(C.byref(a), 0x100000, 1 << 40, None) != 0 and "NULL x" in hip_lib.last_error()
    a.x = 0x100000
    a.latents = 0x100000
    assert lib.soar_vae_forward(C.byref(a), 0x100000, 1 << 40, None) != 0 and "eps" in hip_lib.last_error()
    assert lib.soar_vae_backward(C.byref(a), 0x100000, 1 << 40, None) != 0 and "g_latents" in hip_lib.last_error()
    a.N = 0
    assert lib.soar_vae_forward(C.byref(a), None, 0, None) == 0 and lib.soar_vae_backward(C.byref(a), None, 0, None) == 0
    # the packer checks the raw size first
    assert lib.soar_vae_pack_weights(0x100000, 5, 0x100000, 1 << 40, None) != 0 and "floats" in hip_lib.last_error()
    assert lib.soar_vae_pack_weights(None, 34163664, 0x100000, 1 << 40, None) != 0 and "NULL" in hip_lib.last_error()
    assert lib.soar_vae_pack_weights(0x100000, 34163664, 0x100000, 16, None) != 0 and "packed" in hip_lib.last_error()


def test_loss_tail_entries_refuse_bad_arguments_without_touching_the_gpu(lib):
    from soar_amd import hip_lib
    assert lib.soar_sds_loss(None, None) != 0 and "NULL args" in hip_lib.last_error()
    s = hip_lib.SoarSdsArgs()
    s.B, s.n_view, s.h, s.w, s.mode, s.n_timesteps = 4, 4, 32, 32, hip_lib.SDS_RECON, 1000
    s.recon_std_rescale = 0.2
    assert lib.soar_sds_loss(C.byref(s), None) != 0 and "NULL t" in hip_lib.last_error()
    s.t = s.tables = s.latents = s.noise = 0x100000
    assert lib.soar_sds_q_sample(C.byref(s), None) != 0 and "x_in" in hip_lib.last_error()
    assert lib.soar_sds_loss(C.byref(s), None) != 0 and "eps_pred" in hip_lib.last_error()
    s.B = 6
    assert lib.soar_sds_loss(C.byref(s), None) != 0 and "multiple of n_view" in hip_lib.last_error()
    s.B, s.mode = 4, 7
    assert lib.soar_sds_loss(C.byref(s), None) != 0 and "mode" in hip_lib.last_error()
    s.mode, s.n_timesteps = hip_lib.SDS_PLAIN, 0
    assert lib.soar_sds_loss(C.byref(s), None) != 0 and "n_timesteps" in hip_lib.last_error()
    s.n_timesteps, s.B = 1000, -1
    assert lib.soar_sds_q_sample(C.byref(s), None) != 0 and "B, h, w" in hip_lib.last_error()
    s.B = 0
    assert lib.soar_sds_loss(C.byref(s), None) == 0 and lib.soar_sds_q_sample(C.byref(s), None) == 0
