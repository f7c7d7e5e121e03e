"""CPU tests of the training system (soar_amd/system.py) and of the oracle of its image terms (tests/step_terms_ref.py): the schedule
rule, the step's constants, config parsing, closed-form cases of the oracle, and the refusal of CPU tensors."""
import json
import math
import os

import pytest
import torch

import step_terms_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = json.load(open(os.path.join(ROOT, "tests", "golden", "system_configs.json")))


def test_schedule_rule():
    from soar_amd.system import C
    assert C(0.5, 0, 10) == 0.5 and C(3, 7, 10) == 3
    # three values: a leading 0
    assert C([1.0, 2.0, 100], 0, 0) == 1.0 and C([1.0, 2.0, 100], 0, 50) == 1.5 and C([1.0, 2.0, 100], 0, 100) == 2.0
    # four values, linear, clamped at both ends
    s = [100, 1.0, 3.0, 200]
    assert C(s, 0, 0) == 1.0 and C(s, 0, 100) == 1.0 and C(s, 0, 150) == 2.0 and C(s, 0, 200) == 3.0 and C(s, 0, 10 ** 6) == 3.0
    # an integer end_step runs on global_step, a float one on the epoch
    assert C([0, 0.0, 1.0, 10], 5, 2) == pytest.approx(0.2) and C([0, 0.0, 1.0, 10.0], 5, 2) == pytest.approx(0.5)
    assert C((0, 0.0, 1.0, 10), 0, 5) == pytest.approx(0.5)                      # a tuple is a list
    for bad in ("0.5", None, {"a": 1}, [1.0, 2.0], [0, 1, 2, 3, 4], [0, "a", 1, 2]):
        with pytest.raises(TypeError):
            C(bad, 0, 0)
    # the shipped max_step_percent schedule
    m = [0, 0.75, 0.25, 1000]
    assert [C(m, 0, t) for t in (0, 500, 1000, 2000)] == [0.75, 0.5, 0.25, 0.25]


def test_step_constants():
    from soar_amd.system import consistency_weight, sds_start_of
    assert sds_start_of(1) == 0 and sds_start_of(0) == 500
    for it, want in ((0, 0.01), (500, 0.01 + 0.05), (5000, 0.01 + 0.1)):
        assert consistency_weight(0.01, it) == pytest.approx(want, abs=1e-15)
        assert consistency_weight(0.01, it) == R.consistency_weight(0.01, it)


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_the_shipped_configs_parse(name):
    from soar_amd.renderer import registry
    import soar_amd.renderer  # noqa: F401
    cfg = CONFIGS[name]
    needs_lpips = any(cfg["loss"][k] > 0 for k in ("lambda_normal_F", "lambda_normal_B", "lambda_vgg"))
    cls = registry.find("gaussiansurfel-mvdream-system")
    if needs_lpips:
        with pytest.raises(ValueError, match="lpips"):
            cls(cfg)
    s = cls(cfg, lpips=object())
    assert s.training_stage == cfg["training_stage"] and s.sds_start == (0 if cfg["training_stage"] == 1 else 500)
    assert s.loss_cfg == cfg["loss"] and s.use_explicit is False and s.global_step == 0
    s.global_step = 1000
    from soar_amd.system import C
    assert s.step_range() == (C(cfg["guidance"]["min_step_percent"], 0, 1000), C(cfg["guidance"]["max_step_percent"], 0, 1000))
    if name == "gaussiansurfel_imagedream_s0":
        assert s.step_range() == (0.02, 0.5)                        # [0, 0.75, 0.25, 2000] half way
    assert s._weight("lambda_sds") == cfg["loss"]["lambda_sds"]


def test_unbuilt_terms_are_refused():
    from soar_amd.system import SurfelMVDreamSystem, parse_loss
    base = dict(CONFIGS["gaussiansurfel_imagedream_s0"]["loss"])
    parse_loss(base)
    for key in ("lambda_tv_loss", "lambda_depth_tv_loss"):
        with pytest.raises(NotImplementedError, match=key):
            SurfelMVDreamSystem({"loss": dict(base, **{key: 0.1})}, lpips=object())
    with pytest.raises(NotImplementedError, match="lambda_tv_loss"):
        parse_loss(dict(base, lambda_tv_loss=[0, 0.0, 1.0, 100]))
    with pytest.raises(TypeError):
        parse_loss(dict(base, lambda_curv="much"))
    with pytest.raises(ValueError, match="training_stage"):
        SurfelMVDreamSystem({"training_stage": 2})


# ---- the oracle, on closed forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_cos_loss(dtype):
    # identical unit normals: cos = 1 everywhere, nothing is below cos(pi / 10000): an empty selection, NaN
    n = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]])
    img = ((n + 1) / 2).reshape(1, 1, 3, 3)
    assert torch.isnan(R.cos_loss(img, img, None, math.pi / 10000, 1.0, dtype))
    # a one-pixel image: normals at 60 degrees, 1 - cos = 0.5
    a = ((torch.tensor([1.0, 0.0, 0.0]) + 1) / 2).reshape(1, 1, 1, 3)
    b = ((torch.tensor([0.5, math.sqrt(0.75), 0.0]) + 1) / 2).reshape(1, 1, 1, 3)
    assert R.cos_loss(a, b, None, 0.0, 1.0, dtype).item() == pytest.approx(0.5, abs=1e-6)
    assert R.cos_loss(a, b, torch.ones(1, 1, 1, dtype=torch.bool), 0.0, 1.0, dtype).item() == pytest.approx(0.5, abs=1e-6)
    # an all-zero mask: NaN
    assert torch.isnan(R.cos_loss(a, b, torch.zeros(1, 1, 1, dtype=torch.bool), 0.0, 1.0, dtype))
    # opposite normals, weight 2: 1 - (-2) = 3
    assert R.cos_loss(a, 1 - a, None, 0.0, 2.0, dtype).item() == pytest.approx(3.0, abs=1e-6)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_frame_terms(dtype):
    occ = torch.tensor([0.25, 0.5, 0.75]).reshape(1, 1, 1, 3)
    assert R.loss_occ(occ, torch.ones(1, 1, 1), dtype).item() == pytest.approx(0.5)
    assert torch.isnan(R.loss_occ(occ, torch.zeros(1, 1, 1), dtype))
    two = torch.cat([occ, torch.zeros(1, 1, 1, 3)], 2)                          # the second pixel lies outside the mask
    assert R.loss_occ(two, torch.tensor([[[0.3, 0.0]]]), dtype).item() == pytest.approx(0.5)
    rgb, bg = torch.full((1, 1, 2, 3), 0.8), torch.tensor([0.2, 0.4, 0.6])
    out = R.blended(rgb, torch.tensor([[[1.0, 0.25]]]), bg, dtype)
    assert torch.allclose(out[0, 0, 0], torch.full((3,), 0.8, dtype=dtype))
    assert torch.allclose(out[0, 0, 1], (0.8 * 0.25 + bg * 0.75).to(dtype))
    assert R.abs_mean(torch.tensor([-2.0, 0.0, 1.0, 0.0]), dtype).item() == 0.75


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_normal_views(dtype):
    g = torch.Generator().manual_seed(0)
    cn, gF, gB = torch.rand(2, 4, 4, 3, generator=g), torch.rand(1, 4, 4, 3, generator=g), torch.rand(1, 4, 4, 3, generator=g)
    cm = torch.rand(2, 4, 4, 1, generator=g)
    gm = torch.tensor([0.0, 5e-6, 0.3, 1.0]).repeat(4).reshape(1, 4, 4)
    lp = R.lpips_inputs(cn, gF, gB, gm, dtype)
    assert lp.shape == (4, 3, 4, 4)
    # the front view sees the float mask, the back view its binarisation
    x = cn.to(dtype).permute(0, 3, 1, 2)
    assert torch.equal(lp[0, :, 0, 2], (x[0, :, 0, 2] * torch.tensor(0.3).to(dtype) - 0.5) * 2) and torch.equal(lp[1, :, 0, 2], (x[1, :, 0, 2] - 0.5) * 2)
    assert torch.equal(lp[1, :, 0, 1], torch.full((3,), -1.0, dtype=dtype)) and not torch.equal(lp[0, :, 0, 1], torch.full((3,), -1.0, dtype=dtype))
    assert R.lpips_inputs(cn, gF, None, gm, dtype).shape == (2, 3, 4, 4)
    v = R.normal_view_values(cn, cm, gF, gB, gm, dtype)
    sel = gm > 1e-5
    assert int(sel.sum()) == 8
    assert v["cos_F"].item() == pytest.approx(0.2 * R.cos_loss(cn[[0]], gF, sel, 0.0, 1.0, dtype).item())
    assert v["mask_l1"].item() == pytest.approx((cm[0, ..., 0] - gm[0]).abs().mean().item(), rel=1e-6)
    assert R.normal_view_values(cn, cm, gF, None, gm, dtype)["cos_B"] is None


# ---- import and refusal ---------------------------------------------------------------------------------------------------------
def test_modules_import_without_a_gpu_and_refuse_cpu_tensors():
    import soar_amd
    from soar_amd import step_losses as S
    from soar_amd import system  # noqa: F401
    assert soar_amd.SurfelMVDreamSystem is system.SurfelMVDreamSystem
    z = torch.zeros(1, 4, 4, 3)
    for call in (lambda: S.consistency_loss(z, z), lambda: S.abs_mean(z), lambda: S.frame_extra_terms(z, z, z[..., 0], z[0, 0, 0]),
                 lambda: S.normal_view_terms(z, z[..., :1], z, None, z[..., 0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
