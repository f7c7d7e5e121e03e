"""CPU tests of the test-split evaluation (soar_amd/evaluate.py, csrc/eval.hip): the two NumPy restatements of skimage's SSIM agree, how
far skimage's float32 arithmetic lies from the float64 definition, the closed forms, the refusals of the C ABI and of the Python
surface (no launch, no device) and the files TestEvaluator.finish writes."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import eval_ref as R

# (H, W, target, noise, mask) of make_case, seed = position
CASES = [(7, 7, "random", 0.05, "inside"), (8, 9, "smooth", 0.01, "blob"), (23, 37, "random", 0.1, "checker"),
         (23, 37, "white", 0.02, "inside"), (40, 200, "smooth", 0.05, "half"), (200, 40, "white", 0.1, "blob"),
         (64, 80, "random", 0.03, "blob")]
# the largest distance of the float32 uniform_filter form from the float64 value over CASES, as measured (2.5e-9 .. 2.63e-7: the
# smooth and the mostly white targets, whose window variances are small, lie furthest); the bar is four times that, which covers
# another summation order inside scipy's filter
FLOAT32_MEASURED = 2.63e-7
FLOAT32_BAR = 4 * FLOAT32_MEASURED


def _case(i):
    H, W, kind, noise, mask = CASES[i]
    pred, gt, m = R.make_case(1, H, W, kind, noise, mask, seed=i)
    return pred[0], R.white_target(gt[0], m[0])


@pytest.fixture(scope="module")
def values():
    """per case: the direct float64 SSIM, the float64 and the float32 uniform_filter forms"""
    out = []
    for i in range(len(CASES)):
        pred, gw = _case(i)
        out.append((R.ssim7(pred, gw), R.ssim7_filter(pred, gw, np.float64), R.ssim7_filter(pred, gw, np.float32)))
    return out


def test_the_two_float64_restatements_agree(values):
    worst = max(abs(a - b) for a, b, _ in values)
    print(f"\ndirect window sums against uniform_filter, float64: {worst:.2e}")
    assert worst <= 1e-12


def test_distance_from_skimages_float32_arithmetic(values):
    d = [abs(a - c) for a, _, c in values]
    print("\nfloat32 uniform_filter form against float64, per case:", " ".join(f"{v:.2e}" for v in d))
    assert max(d) <= FLOAT32_BAR
    assert max(d) > 0                           # float32 does round: a zero would mean that the float32 path ran in float64


@pytest.mark.parametrize("a,b", [(0.25, 0.75), (0.9, 0.1), (0.3, 0.3000001), (1.0, 0.0)])
def test_constant_images_have_closed_forms(a, b):
    pred, gt = np.full((9, 11, 3), a, np.float32), np.full((9, 11, 3), b, np.float32)
    a64, b64 = float(np.float32(a)), float(np.float32(b))
    want_ssim = (2 * a64 * b64 + R.C1) / (a64 * a64 + b64 * b64 + R.C1)
    # a constant's window variance is 0 up to the rounding of uxx - ux ux (1e-16), against C2 = 9e-4
    assert abs(R.ssim7(pred, gt) - want_ssim) <= 1e-12
    d = float(np.float32(b) - np.float32(a))
    d2 = float(np.float32(d) * np.float32(d))
    assert abs(R.psnr(pred, gt) - (-10 * math.log10(d2))) <= 1e-12


def test_equal_images_give_exactly_one_and_infinity():
    for i in (0, 2, 6):
        _, gw = _case(i)
        assert R.ssim7(gw, gw) == 1.0
        assert R.ssim7_filter(gw, gw, np.float64) == 1.0
        assert R.mse(gw, gw) == 0.0 and R.psnr(gw, gw) == math.inf


def test_white_target_and_bytes():
    gt = np.array([[[0.2, 0.4, 0.6], [0.1, 0.1, 0.1], [0.3, 0.3, 0.3]]], np.float32)
    m = np.array([[1.0, 0.5, 0.50001]], np.float32)
    gw = R.white_target(gt, m)
    assert gw[0, 0].tolist() == gt[0, 0].tolist() and gw[0, 1].tolist() == [1.0, 1.0, 1.0] and gw[0, 2].tolist() == gt[0, 2].tolist()
    pred = np.array([[[-0.1, 0.999, 1.2], [0.5, 1.0, 0.0], [254.9 / 255, 0.25, 0.75]]], np.float32)
    g = R.byte_grid(pred, gw)
    assert g.shape == (1, 6, 3) and g.dtype == np.uint8
    assert g[0, 0].tolist() == [0, 254, 255] and g[0, 1].tolist() == [127, 255, 0] and g[0, 4].tolist() == [255, 255, 255]


# ---- the C ABI: every refusal comes before any launch -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_scratch_sizing_and_its_refusals(lib):
    from soar_amd import hip_lib
    n = C.c_size_t(0)
    assert lib.soar_eval_scratch_bytes(1, 1080, 1920, C.byref(n)) == 0
    assert 0 < n.value <= 1 << 20 and n.value % 256 == 0 and n.value % 32 == 0
    one = n.value
    assert lib.soar_eval_scratch_bytes(3, 1080, 1920, C.byref(n)) == 0 and 3 * one - 2 * 256 <= n.value <= 3 * one
    assert lib.soar_eval_scratch_bytes(1, 7, 7, C.byref(n)) == 0 and n.value >= 32
    for N, H, W in ((0, 64, 64), (-1, 64, 64), (1, 6, 64), (1, 64, 6), (1, 0, 0), (70000, 8, 8), (4, 32768, 32768)):
        assert lib.soar_eval_scratch_bytes(N, H, W, C.byref(n)) != 0, (N, H, W)
        assert "bad arguments" in hip_lib.last_error()
    assert lib.soar_eval_scratch_bytes(1, 64, 64, None) != 0


def test_image_metrics_refuses_bad_arguments_before_any_launch(lib):
    from soar_amd import hip_lib
    one = C.c_double(0.0)
    p = C.cast(C.pointer(one), C.c_void_p).value           # any non-NULL address: nothing reads it before the checks fail
    assert lib.soar_eval_image_metrics(None, p, 1 << 20, None) != 0 and "NULL args" in hip_lib.last_error()

    def args(**kw):
        a = hip_lib.SoarEvalArgs()
        a.N, a.H, a.W = 1, 16, 16
        for name in ("pred", "gt_rgb", "gt_mask", "gt_white", "pred2", "gt2", "metrics"):
            setattr(a, name, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, word in ((dict(H=6), "7x7"), (dict(W=6), "7x7"), (dict(N=0), "bad arguments"), (dict(N=-2), "bad arguments")):
        assert lib.soar_eval_image_metrics(C.byref(args(**kw)), p, 1 << 20, None) != 0
        assert word in hip_lib.last_error(), (kw, hip_lib.last_error())
    for name in ("pred", "gt_rgb", "gt_mask", "gt_white", "pred2", "gt2", "metrics"):
        assert lib.soar_eval_image_metrics(C.byref(args(**{name: None})), p, 1 << 20, None) != 0
        assert "NULL" in hip_lib.last_error() and name in hip_lib.last_error()
    n = C.c_size_t(0)
    assert lib.soar_eval_scratch_bytes(1, 16, 16, C.byref(n)) == 0
    assert lib.soar_eval_image_metrics(C.byref(args()), None, n.value, None) != 0 and "NULL workspace" in hip_lib.last_error()
    assert lib.soar_eval_image_metrics(C.byref(args()), 0x1000, n.value - 1, None) != 0
    assert f"workspace of {n.value - 1} bytes, need {n.value} (soar_eval_scratch_bytes)" in hip_lib.last_error()


def test_python_surface_refuses_cpu_tensors_dtypes_and_shapes():
    from soar_amd import evaluate as E
    x, m = torch.zeros(1, 16, 16, 3), torch.ones(1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.image_metrics(x, x, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.image_metrics(x, x, m[..., None])
    with pytest.raises(ValueError, match=r"N, H, W, 3"):
        E.image_metrics(x.permute(0, 3, 1, 2), x, m)
    with pytest.raises(ValueError, match="gt_mask"):
        E.image_metrics(x, x, torch.ones(1, 16, 16, 3))
    with pytest.raises(ValueError, match="agree"):
        E.image_metrics(x, x, torch.ones(1, 16, 15))
    with pytest.raises(ValueError, match="agree"):
        E.image_metrics(x, torch.zeros(2, 16, 16, 3), m)
    # (the dtype and size checks come behind the device check: on the device they are exercised by tests/test_evaluate_gpu.py)
    with pytest.raises(ValueError, match="capacity"):
        E.TestEvaluator(None, 0)
    ev = E.TestEvaluator(None, 2)
    with pytest.raises(ValueError, match="one frame per call"):
        ev.add(torch.zeros(2, 16, 16, 3), {})
    with pytest.raises(RuntimeError, match="no frame"):
        ev.finish()


def test_finish_writes_the_references_files(tmp_path):
    from soar_amd import evaluate as E
    rng = np.random.default_rng(3)
    psnrs, ssims = 20 + 15 * rng.random(5), rng.random(5)
    lp = rng.random(5).astype(np.float32)
    ev = E.TestEvaluator(None, capacity=8, keep_images=True)
    # a buffer built on the host stands in for the device's: finish() treats it the same way (one .cpu(), then NumPy)
    ev.buffer = torch.full((8, 3), float("nan"), dtype=torch.float64)
    ev.buffer[:5] = torch.from_numpy(np.stack([psnrs, ssims, lp.astype(np.float64)], axis=1))
    ev.count, ev.gt_indices = 5, [2, 7, 12, 17, 22]
    imgs = rng.integers(0, 256, (5, 9, 20, 3), dtype=np.uint8)
    ev.images = [torch.from_numpy(i) for i in imgs]
    res = ev.finish(save_dir=str(tmp_path / "save"), step=1200)
    assert np.array_equal(res["psnrs"], psnrs) and np.array_equal(res["ssims"], ssims) and np.array_equal(res["lpips"], lp)
    assert res["lpips"].dtype == np.float32 and res["gt_indices"] == [2, 7, 12, 17, 22]
    assert res["psnr"] == psnrs.mean() and res["ssim"] == ssims.mean() and res["lpips_mean"] == lp.mean()
    save = tmp_path / "save"
    assert np.array_equal(np.loadtxt(save / "psnrs.txt"), psnrs)            # savetxt's default %.18e round-trips a float64
    assert np.array_equal(np.loadtxt(save / "ssims.txt"), ssims)
    assert np.array_equal(np.loadtxt(save / "lpips.txt").astype(np.float32), lp)
    text = (save / "average.txt").read_text()
    assert text == f"{psnrs.mean()} {ssims.mean()} {lp.mean()}"
    assert [float(t) for t in text.split()] == [float(psnrs.mean()), float(ssims.mean()), float(lp.mean())]
    from PIL import Image
    for i, img in zip(ev.gt_indices, imgs):
        assert np.array_equal(np.array(Image.open(save / "it1200-test" / f"{i}.png")), img)
    # without save_dir nothing is written
    ev.finish()
    assert sorted(p.name for p in save.iterdir()) == ["average.txt", "it1200-test", "lpips.txt", "psnrs.txt", "ssims.txt"]
