"""CPU tests of the environment-map background (soar_amd/background.py): the float64 restatement (tests/envmap_ref.py) against
the specification, the module's config, parameters and draws, and argument checks of the C entries that stop before any GPU work."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

import envmap_ref as R
from soar_amd.background import NeuralEnvironmentMapBackground as Env
from soar_amd.renderer import registry

SOAR_CFG = {"color_activation": "sigmoid", "random_aug": True, "share_aug_bg": True, "random_aug_prob": 0.5}


def test_basis_is_orthonormal_on_the_sphere():
    n_t, n_p = 64, 128
    t, wt = np.polynomial.legendre.leggauss(n_t)                 # cos(theta), exact for the degree-4 products
    phi = (np.arange(n_p) + 0.5) * 2 * np.pi / n_p
    ct = torch.tensor(t, dtype=torch.float64)[:, None].expand(n_t, n_p)
    st = torch.sqrt(1 - ct ** 2)
    ph = torch.tensor(phi, dtype=torch.float64)[None, :].expand(n_t, n_p)
    v = torch.stack([st * torch.cos(ph), st * torch.sin(ph), ct], -1)
    Y = R.basis(v).reshape(-1, 9)
    w = (torch.tensor(wt, dtype=torch.float64)[:, None] * (2 * np.pi / n_p)).expand(n_t, n_p).reshape(-1, 1)
    G = (Y * w).T @ Y
    assert (G - torch.eye(9, dtype=torch.float64)).abs().max() < 1e-6


def test_basis_closed_forms_at_axes_and_fixed_directions():
    s = 1 / math.sqrt(3)
    pts = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (s, s, s), (0.6, -0.8, 0.0), (0.3, 0.4, -0.5)]  # the last is not unit
    for x, y, z in pts:
        want = [0.28209479177387814, -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
                1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999,
                -1.0925484305920792 * x * z, 0.54627421529603959 * (x * x - y * y)]
        got = R.basis(torch.tensor([x, y, z], dtype=torch.float64))
        assert np.allclose(got.numpy(), want, atol=1e-15, rtol=0)
    # the z^2 form differs from the rasterizer's 2z^2 - x^2 - y^2 form off the sphere
    v = torch.tensor([0.3, 0.4, -0.5], dtype=torch.float64)
    alt = 0.31539156525251999 * (2 * v[2] ** 2 - v[0] ** 2 - v[1] ** 2)
    assert abs(float(R.basis(v)[6] - alt)) > 1e-3


def test_round_trip_is_followed():
    d = torch.tensor([[1e-8, -3e-9, 0.3], [0.1, 0.7, -0.999999]], dtype=torch.float32)
    x = R.round_trip(d)
    u = (d + 1.0) / 2.0
    assert torch.equal(x, u * 2.0 - 1.0)
    assert x[0, 0] == 0 and x[0, 1] == 0 and not torch.equal(x, d)
    e = R.encode(d)
    assert e.dtype == torch.float64 and torch.equal(e, R.basis(x.double()))


def test_config_defaults_and_registration():
    assert registry.find("gaussiandreamer-background") is Env
    m = Env()
    c = m.cfg
    assert (c.n_output_dims, c.color_activation, c.random_aug, c.random_aug_prob, c.eval_color, c.share_aug_bg) == \
        (3, "sigmoid", False, 0.5, None, False)
    assert c.dir_encoding_config == {"otype": "SphericalHarmonics", "degree": 3}
    assert c.mlp_network_config == {"otype": "VanillaMLP", "activation": "ReLU", "n_neurons": 16, "n_hidden_layers": 2}
    assert Env(SOAR_CFG).cfg.share_aug_bg is True
    assert isinstance(m, torch.nn.Module)


@pytest.mark.parametrize("cfg,key", [
    ({"n_output_dims": 4}, "n_output_dims"),
    ({"color_activation": "relu"}, "color_activation"),
    ({"dir_encoding_config": {"otype": "HashGrid", "degree": 3}}, "dir_encoding_config.otype"),
    ({"dir_encoding_config": {"otype": "SphericalHarmonics", "degree": 4}}, "dir_encoding_config.degree"),
    ({"dir_encoding_config": {"otype": "SphericalHarmonics", "degree": 3, "include_xyz": True}}, "include_xyz"),
    ({"mlp_network_config": {"otype": "VanillaMLP", "activation": "ReLU", "n_neurons": 32, "n_hidden_layers": 2}}, "n_neurons"),
    ({"mlp_network_config": {"otype": "VanillaMLP", "activation": "ReLU", "n_neurons": 16, "n_hidden_layers": 3}}, "n_hidden_layers"),
    ({"mlp_network_config": {"otype": "VanillaMLP", "activation": "SiLU", "n_neurons": 16, "n_hidden_layers": 2}}, "activation"),
    ({"mlp_network_config": {"otype": "FullyFusedMLP", "activation": "ReLU", "n_neurons": 16, "n_hidden_layers": 2}}, "otype"),
])
def test_unsupported_configs_are_refused_by_name(cfg, key):
    with pytest.raises(NotImplementedError, match=key):
        Env(cfg)


def test_unknown_config_key_is_refused():
    with pytest.raises(ValueError):
        Env({"not_a_key": 1})


def test_parameters_and_reference_state_dict():
    torch.manual_seed(3)
    m = Env(SOAR_CFG)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert shapes == {"network.layers.0.weight": (16, 9), "network.layers.2.weight": (16, 16), "network.layers.4.weight": (3, 16)}
    assert sum(p.numel() for p in m.parameters()) == 448
    g = torch.Generator().manual_seed(9)
    sd = {"network.layers.0.weight": torch.randn(16, 9, generator=g), "network.layers.2.weight": torch.randn(16, 16, generator=g),
          "network.layers.4.weight": torch.randn(3, 16, generator=g),
          "encoding.encoding.encoding.params": torch.zeros(0)}         # tiny-cuda-nn's (empty) parameter of the SH encoding
    m.load_state_dict(sd)
    for k in (0, 2, 4):
        assert torch.equal(m.network.layers[k].weight, sd[f"network.layers.{k}.weight"])
    # as the background of a whole system's checkpoint: the `background.` keys
    outer = torch.nn.Module()
    outer.background = Env(SOAR_CFG)
    outer.load_state_dict({"background." + k: v for k, v in sd.items()})
    assert torch.equal(outer.background.network.layers[4].weight, sd["network.layers.4.weight"])


def test_seeded_construction_is_deterministic_and_draws_like_the_reference_layers():
    torch.manual_seed(11)
    a = Env(SOAR_CFG)
    torch.manual_seed(11)
    b = Env(SOAR_CFG)
    torch.manual_seed(11)
    ref = [torch.nn.Linear(9, 16, bias=False), torch.nn.Linear(16, 16, bias=False), torch.nn.Linear(16, 3, bias=False)]
    for k, lin in zip((0, 2, 4), ref):
        assert torch.equal(a.network.layers[k].weight, b.network.layers[k].weight)
        assert torch.equal(a.network.layers[k].weight, lin.weight)


def _reference_draws(training, random_aug, prob, share, B):
    """the reference forward's draws (TS/background/gaussian_mvdream_background.py:49-72) -> the constant or None"""
    if training and random_aug and random.random() < prob:
        n_color = 1 if share else B
        value = random.random() < 0.5
        return torch.randn(n_color, 1, 1, 3) * value
    return None


@pytest.mark.parametrize("share", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_draws_follow_the_reference_order(monkeypatch, share, training):
    from soar_amd import background as BG
    moved = []
    monkeypatch.setattr(BG._color_ring, "to_device", lambda v, dev: (moved.append(v.clone()), v.reshape(-1))[1])
    m = Env({**SOAR_CFG, "share_aug_bg": share})
    m.train(training)
    B = 5
    for seed in range(12):
        random.seed(seed)
        torch.manual_seed(100 + seed)
        want = _reference_draws(training, True, 0.5, share, B)
        py_state, th_state = random.getstate(), torch.get_rng_state()
        random.seed(seed)
        torch.manual_seed(100 + seed)
        got = m.draw_color(B, "cpu")
        assert random.getstate() == py_state and torch.equal(torch.get_rng_state(), th_state)
        if want is None:
            assert got is None
        else:
            assert got.shape == (3 * (1 if share else B),)
            assert torch.equal(got, (torch.zeros_like(want) + want).reshape(-1))      # color * 0 + randn * value
            assert not torch.signbit(got[got == 0]).any()


def test_eval_color_and_no_aug_make_no_draws():
    m = Env({**SOAR_CFG, "eval_color": (0.1, 0.2, 0.3)})
    m.eval()
    random.seed(0)
    s = random.getstate()
    assert torch.equal(m.draw_color(4, "cpu"), torch.tensor([0.1, 0.2, 0.3]))
    assert random.getstate() == s
    m = Env({"random_aug": False})
    assert m.draw_color(4, "cpu") is None and random.getstate() == s


def test_cpu_tensors_and_grad_dirs_are_refused():
    m = Env(SOAR_CFG)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 2, 2, 3))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 2, 3))
    with pytest.raises(NotImplementedError, match="dirs"):
        m(torch.zeros(1, 2, 2, 3, requires_grad=True))


def test_image_stride_refuses_overlapping_images():
    from soar_amd.background import _image_stride
    H, W = 8, 8
    assert _image_stride(torch.zeros(3, 3, H, W), 3, H, W) == 3 * H * W
    assert _image_stride(torch.zeros(3, 5, H, W)[:, 1:4], 3, H, W) == 5 * H * W          # views of a larger buffer
    assert _image_stride(torch.ones(1, 1, H, W).expand(4, 1, H, W), 1, H, W) is None      # stride 0: one image
    assert _image_stride(torch.ones(1, 3, H, W).expand(4, 3, H, W), 3, H, W) is None
    assert _image_stride(torch.zeros(4 * H * W + 3 * H * W).as_strided((4, 3, H, W), (H * W, H * W, W, 1)), 3, H, W) is None
    assert _image_stride(torch.ones(1, 1, H, W).expand(1, 1, H, W), 1, H, W) == H * W
    assert _image_stride(torch.zeros(2, 3, W, H).transpose(2, 3), 3, H, W) is None


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_c_entries_check_arguments(lib):
    from soar_amd import hip_lib
    n = C.c_size_t(0)
    assert lib.soar_envmap_workspace_bytes(5, 512, 512, C.byref(n)) == 0 and n.value >= 448 * 8 and n.value % 256 == 0
    assert lib.soar_envmap_workspace_bytes(0, 512, 512, C.byref(n)) == 0 and n.value % 256 == 0
    assert lib.soar_envmap_workspace_bytes(-1, 4, 4, C.byref(n)) != 0 and "negative" in hip_lib.last_error()
    assert lib.soar_envmap_workspace_bytes(4096, 1024, 1024, C.byref(n)) != 0 and "2^30" in hip_lib.last_error()
    assert lib.soar_envmap_forward(None, None) != 0 and "NULL args" in hip_lib.last_error()
    a = hip_lib.SoarEnvmapArgs()
    a.B, a.H, a.W = 2, 4, 4
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "NULL dirs" in hip_lib.last_error()
    a.dirs = 0x1000
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "NULL weight" in hip_lib.last_error()
    a.w1 = a.w2 = a.w3 = 0x1000
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "NULL bg" in hip_lib.last_error()
    a.n_comp = 3
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "n_comp" in hip_lib.last_error()
    a.n_comp = 1
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "NULL mask" in hip_lib.last_error()
    a.mask, a.mask_stride, a.render_stride = 0x1000, 16, 16
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "strides" in hip_lib.last_error()
    a.render_stride, a.bg = 48, 0x1000
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "render / comp" in hip_lib.last_error()
    a.color, a.color_rows = 0x1000, 3
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "color_rows" in hip_lib.last_error()
    a.color, a.W = None, -1
    assert lib.soar_envmap_forward(C.byref(a), None) != 0 and "negative" in hip_lib.last_error()
    a.W = 4
    assert lib.soar_envmap_backward(C.byref(a), None, 0, None) != 0 and "workspace" in hip_lib.last_error()
    lib.soar_envmap_workspace_bytes(2, 4, 4, C.byref(n))
    assert lib.soar_envmap_backward(C.byref(a), 0x1010, n.value, None) != 0 and "aligned" in hip_lib.last_error()
    a.d_w1 = 0x1000
    assert lib.soar_envmap_backward(C.byref(a), 0x1000, n.value, None) != 0 and "together" in hip_lib.last_error()
