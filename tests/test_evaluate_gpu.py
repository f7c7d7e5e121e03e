"""GPU tests of the test-split evaluation (csrc/eval.hip, soar_amd/evaluate.py) against the NumPy restatement (tests/eval_ref.py):
PSNR / MSE / SSIM on one window, off the tile grid, over several tiles and images and on long thin images, under every kind of mask;
the per-pixel outputs bit for bit; strided inputs; reproducibility; LPIPS through the module; TestEvaluator over a test split.

The bars are derived, not measured: the inputs are float32 widened exactly and their products are exact in float64, a sum
of 49 (or 3 H W) float64 terms carries a relative error below 1e-13, and the SSIM denominators are at least C1 C2, which leaves four
orders of margin to 1e-9; the two host restatements themselves differ by 2e-14."""
import math

import numpy as np
import pytest
import torch

import eval_ref as R
import lpips_ref as LR
from soar_amd import data as D
from soar_amd import evaluate as E
from soar_amd.lpips import LPIPSVGG
from test_lpips_gpu import VALUE_REL            # the bar tests/test_lpips_gpu.py holds LPIPSVGG to against the float64 restatement

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SSIM_ABS, MSE_REL, PSNR_DB = 1e-9, 1e-12, 1e-9

# 7x7: one window; 8x9; 23x37: off the 16x64 tile grid; 3x64x80: several tiles, the batch index in every address; 40x200 and 200x40:
# long thin images, the halo on one axis only
SHAPES = [(1, 7, 7), (1, 8, 9), (1, 23, 37), (3, 64, 80), (1, 40, 200), (1, 200, 40)]
MASKS = ["inside", "outside", "checker", "half"]
KINDS = {"inside": "random", "outside": "smooth", "checker": "white", "half": "random"}
_cache = {}


def _case(shape, mask):
    """inputs and their restated values, made once per (shape, mask) and left unchanged"""
    key = (shape, mask)
    if key not in _cache:
        N, H, W = shape
        pred, gt, m = R.make_case(N, H, W, KINDS[mask], noise=0.05, mask=mask, seed=H * 1000 + W + MASKS.index(mask))
        _cache[key] = (pred, gt, m, [R.image_metrics(pred[n], gt[n], m[n]) for n in range(N)])
    return _cache[key]


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _compare(out, want, N, label):
    psnr, ssim, mse = out["psnr"].cpu().numpy(), out["ssim"].cpu().numpy(), out["mse"].cpu().numpy()
    assert psnr.dtype == ssim.dtype == mse.dtype == np.float64 and psnr.shape == ssim.shape == mse.shape == (N,)
    for n in range(N):
        w = want[n]
        e_ssim, e_mse, e_psnr = abs(ssim[n] - w["ssim"]), abs(mse[n] - w["mse"]) / w["mse"], abs(psnr[n] - w["psnr"])
        print(f"\n{label} image {n}: ssim {w['ssim']:.6f} err {e_ssim:.1e}  mse {w['mse']:.3e} rel {e_mse:.1e}  psnr {w['psnr']:.3f} err {e_psnr:.1e}")
        assert e_ssim <= SSIM_ABS and e_mse <= MSE_REL and e_psnr <= PSNR_DB
        assert np.array_equal(out["gt_white"][n].cpu().numpy(), w["gt_white"])
        assert np.array_equal(out["pred2"][n].cpu().numpy(), w["pred2"]) and np.array_equal(out["gt2"][n].cpu().numpy(), w["gt2"])
        assert np.array_equal(out["grid"][n].cpu().numpy(), w["grid"])


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics_and_pixel_outputs_match_the_restatement(shape, mask):
    N, H, W = shape
    pred, gt, m, want = _case(shape, mask)
    assert pred.max() > 1.0 or pred.min() < 0.0                  # pred = target + noise leaves [0, 1] a little: the bytes must clamp
    if mask == "half":
        assert (m == 0.5).any() and (want[0]["gt_white"][m[0] == 0.5] == 1.0).all()      # exactly 0.5 counts as outside
    out = E.image_metrics(_dev(pred), _dev(gt), _dev(m), grid=True)
    assert out["lpips"] is None and out["grid"].dtype == torch.uint8 and out["grid"].shape == (N, H, 2 * W, 3)
    assert out["gt_white"].is_contiguous() and out["pred2"].is_contiguous() and out["gt2"].is_contiguous()
    _compare(out, want, N, f"{N}x{H}x{W} {mask}")
    # a second call on the same inputs: the same bits, with or without the byte image
    again = E.image_metrics(_dev(pred), _dev(gt), _dev(m[..., None]))
    assert again["grid"] is None
    for k in ("psnr", "ssim", "mse", "gt_white", "pred2", "gt2"):
        assert torch.equal(out[k], again[k]), k


@pytest.mark.parametrize("shape", [(1, 23, 37), (3, 64, 80)], ids=lambda s: "x".join(map(str, s)))
def test_strided_inputs_go_in_without_a_copy(shape):
    N, H, W = shape
    pred, gt, m, want = _case(shape, "checker")
    # every other column of a tensor twice as wide
    wide = torch.full((N, H, 2 * W, 3), 7.0, device=DEV)
    wide[:, :, ::2] = _dev(pred)
    sliced = wide[:, :, ::2]
    # an NCHW tensor, permuted
    nchw = _dev(pred).permute(0, 3, 1, 2).contiguous()
    view = nchw.permute(0, 2, 3, 1)
    gt_wide = torch.full((N, H, 2 * W, 3), -3.0, device=DEV)
    gt_wide[:, :, 1::2] = _dev(gt)
    m_tall = torch.full((N, 2 * H, W), 9.0, device=DEV)
    m_tall[:, ::2] = _dev(m)
    assert not sliced.is_contiguous() and not view.is_contiguous()
    _compare(E.image_metrics(sliced, _dev(gt), _dev(m), grid=True), want, N, "sliced pred")
    _compare(E.image_metrics(view, gt_wide[:, :, 1::2], m_tall[:, ::2], grid=True), want, N, "permuted pred, sliced target and mask")


def test_equal_images_and_constants():
    pred, gt, m, _ = _case((1, 23, 37), "checker")
    gw = _dev(R.white_target(gt, m))
    out = E.image_metrics(gw, _dev(gt), _dev(m))
    assert out["ssim"].item() == 1.0 and out["mse"].item() == 0.0 and out["psnr"].item() == math.inf
    a, b = 0.25, 0.75
    out = E.image_metrics(torch.full((2, 20, 70, 3), a, device=DEV), torch.full((2, 20, 70, 3), b, device=DEV), torch.ones(2, 20, 70, device=DEV))
    want_ssim = (2 * a * b + R.C1) / (a * a + b * b + R.C1)
    assert (out["ssim"].cpu() - want_ssim).abs().max().item() <= 1e-12
    assert (out["psnr"].cpu() + 10 * math.log10((b - a) ** 2)).abs().max().item() <= 1e-12


def test_refusals_on_the_device():
    x, m = torch.zeros(1, 16, 16, 3, device=DEV), torch.ones(1, 16, 16, device=DEV)
    with pytest.raises(TypeError, match="float32"):
        E.image_metrics(x.double(), x.double(), m.double())
    with pytest.raises(TypeError, match="float32"):
        E.image_metrics(x, x, m > 0)
    with pytest.raises(ValueError, match="7x7"):
        E.image_metrics(x[:, :6], x[:, :6], m[:, :6])
    with pytest.raises(ValueError, match="empty batch"):
        E.image_metrics(x[:0], x[:0], m[:0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.image_metrics(x, x.cpu(), m)


# ---- LPIPS -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return LPIPSVGG(LR.lpips_state_dict(LR.random_weights())).to(DEV)


@pytest.mark.parametrize("shape", [(1, 16, 16), (2, 23, 37)], ids=lambda s: "x".join(map(str, s)))
def test_lpips_is_the_modules_value_on_the_kernels_inputs(model, shape):
    N, H, W = shape
    pred, gt, m, want = _case(shape, "checker")
    out = E.image_metrics(_dev(pred), _dev(gt), _dev(m), lpips=model)
    assert out["lpips"].shape == (N,) and out["lpips"].dtype == torch.float32 and not out["lpips"].requires_grad
    with torch.no_grad():
        direct = model(out["pred2"].permute(0, 3, 1, 2), out["gt2"].permute(0, 3, 1, 2)).view(-1)
    assert torch.equal(out["lpips"], direct)
    # ... and within the module's own bar of the float64 restatement on 2 pred - 1, 2 gt_white - 1
    w64 = LR.weights_of(model, torch.float64)
    p64 = 2 * _dev(pred).double().permute(0, 3, 1, 2) - 1
    g64 = 2 * _dev(np.stack([w["gt_white"] for w in want])).double().permute(0, 3, 1, 2) - 1
    v64 = LR.lpips(p64, g64, w64, f32_ties=True).view(-1)
    err = float((out["lpips"].double() - v64).abs().max() / v64.abs().max())
    print(f"\n{N}x{H}x{W} lpips {v64.tolist()} rel err {err:.2e}")
    assert float(v64.min()) > 0 and err <= VALUE_REL
    # gradients are not this path's business: an input that requires them changes nothing
    again = E.image_metrics(_dev(pred).requires_grad_(True), _dev(gt), _dev(m), lpips=model)
    assert torch.equal(again["lpips"], out["lpips"]) and not again["lpips"].requires_grad


# ---- TestEvaluator over a test split -----------------------------------------------------------------------------------------------
def test_evaluator_over_the_test_split(model, monkeypatch):
    """Five test frames through collate().  The reference's split keeps one frame in ten for testing (half of every fifth), so that a
    sequence of 5 frames has an EMPTY test split: 50 frames is the shortest sequence with five test frames."""
    import data_ref
    Nf, H, W = 50, 36, 52
    assert D.split_indices(5, "test") == [] and D.split_indices(Nf, "test") == [2, 7, 12, 17, 22]
    store = D.FrameStore.from_arrays(**data_ref.synthetic_sequence(Nf, H, W, seed=4), device=DEV)
    ds = D.RandomMultiviewCameraDataset(dict(height=64, width=64, batch_size=4, n_view=4, smpl_type="smplx"), store, "test")
    assert len(ds) == 5
    render = lambda b: b["gt_rgb"] * 0.9                    # noqa: E731
    ev = E.evaluate_split(render, ds, E.TestEvaluator(model, capacity=len(ds), keep_images=True))
    assert ev.count == 5 and ev.gt_indices == [2, 7, 12, 17, 22] and ev.buffer.is_cuda and ev.buffer.dtype == torch.float64
    with pytest.raises(RuntimeError, match="capacity"):
        ev.add(render(ds[0]), ds[0])

    # finish(): exactly one device-to-host transfer, of the metrics buffer
    moved = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (moved.append(t), real_cpu(t, *a, **k))[1])
    for name in ("item", "tolist", "numpy"):
        real = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, lambda t, *a, _real=real, _name=name, **k: (moved.append(_name) if t.is_cuda else None, _real(t, *a, **k))[1])
    res = ev.finish()
    monkeypatch.undo()
    assert len(moved) == 1 and moved[0] is ev.buffer

    assert res["gt_indices"] == [2, 7, 12, 17, 22] and res["psnrs"].shape == res["ssims"].shape == res["lpips"].shape == (5,)
    for k in range(5):
        b = ds[k]
        m = E.image_metrics(render(b), b["gt_rgb"], b["gt_mask"], lpips=model, grid=True)
        assert res["psnrs"][k] == m["psnr"].item() and res["ssims"][k] == m["ssim"].item() and res["lpips"][k] == m["lpips"].item()
        assert torch.equal(ev.images[k], m["grid"][0])
        # ... which are the restatement's
        w = R.image_metrics(render(b)[0].cpu().numpy(), b["gt_rgb"][0].cpu().numpy(), b["gt_mask"][0].cpu().numpy())
        assert abs(res["ssims"][k] - w["ssim"]) <= SSIM_ABS and abs(res["psnrs"][k] - w["psnr"]) <= PSNR_DB
    assert res["psnr"] == res["psnrs"].mean() and res["ssim"] == res["ssims"].mean() and res["lpips_mean"] == res["lpips"].mean()
    assert np.isfinite(res["psnrs"]).all() and (res["lpips"] > 0).all()
