"""NumPy restatement of the test-split metrics, the oracle of tests/test_evaluate_*.py.  It states what the reference's
test_step (TS/system/gaussian_surfel_mvdream.py:527-589) gets from skimage, whose package is not installed here:
``peak_signal_noise_ratio(gt, pred)`` on float32 images of data range 1 and ``structural_similarity(pred, gt, channel_axis=-1,
data_range=1)`` (7x7 uniform window, sample covariance, the border of 3 cropped), and threestudio's byte conversion.

* ``ssim7`` sums every window directly in float64: the definition.
* ``ssim7_filter(dtype)`` is skimage's own way, ``scipy.ndimage.uniform_filter(size=7)`` and ``crop(S, 3)``: with float64 it must agree
  with ``ssim7`` to rounding, with float32 it is the arithmetic skimage itself runs on float32 images."""
import numpy as np

C1, C2 = 0.01 ** 2, 0.03 ** 2            # (K1 data_range)^2, (K2 data_range)^2
WIN = 7
COV_NORM = WIN * WIN / (WIN * WIN - 1)   # use_sample_covariance=True


def white_target(gt_rgb, gt_mask):
    """gt[~(mask > 0.5)] = 1.0: float32 [..., H, W, 3]"""
    gt_rgb, gt_mask = np.asarray(gt_rgb, np.float32), np.asarray(gt_mask, np.float32)
    return np.where(gt_mask[..., None] > 0.5, gt_rgb, np.float32(1.0)).astype(np.float32)


def mse(pred, gt_white):
    """skimage's mean_squared_error on float32 images: the difference and its square in float32, the mean in float64"""
    pred, gt_white = np.asarray(pred, np.float32), np.asarray(gt_white, np.float32)
    d = gt_white - pred
    return float(np.mean(d * d, dtype=np.float64))


def psnr(pred, gt_white):
    with np.errstate(divide="ignore"):
        return float(10 * np.log10(np.float64(1.0) / mse(pred, gt_white)))


def _ssim_of_means(ux, uy, uxx, uyy, uxy):
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def _window_sums(a):
    """[H, W] float64 -> [H - 6, W - 6]: the sum of every 7x7 window wholly inside, added tap by tap"""
    H, W = a.shape
    out = np.zeros((H - WIN + 1, W - WIN + 1), np.float64)
    for dy in range(WIN):
        for dx in range(WIN):
            out += a[dy:dy + H - WIN + 1, dx:dx + W - WIN + 1]
    return out


def ssim7(pred, gt_white):
    """[H, W, 3] float32 images -> the float64 mean over the channels of the mean of S over the windows"""
    pred, gt_white = np.asarray(pred, np.float32), np.asarray(gt_white, np.float32)
    assert pred.shape == gt_white.shape and pred.ndim == 3 and min(pred.shape[:2]) >= WIN
    per_channel = []
    for c in range(pred.shape[2]):
        x, y = pred[..., c].astype(np.float64), gt_white[..., c].astype(np.float64)
        n = float(WIN * WIN)
        S = _ssim_of_means(_window_sums(x) / n, _window_sums(y) / n, _window_sums(x * x) / n, _window_sums(y * y) / n,
                           _window_sums(x * y) / n)
        per_channel.append(S.mean(dtype=np.float64))
    return float(np.mean(per_channel))


def ssim7_filter(pred, gt_white, dtype=np.float64):
    """skimage's structural_similarity: uniform_filter(size=7) per channel in `dtype`, crop(S, 3).mean(dtype=float64)"""
    from scipy.ndimage import uniform_filter
    pred, gt_white = np.asarray(pred, np.float32), np.asarray(gt_white, np.float32)
    pad = (WIN - 1) // 2
    per_channel = []
    for c in range(pred.shape[2]):
        x, y = pred[..., c].astype(dtype), gt_white[..., c].astype(dtype)
        f = lambda a: uniform_filter(a, size=WIN)                      # noqa: E731
        S = _ssim_of_means(f(x), f(y), f(x * x), f(y * y), f(x * y))
        H, W = S.shape
        per_channel.append(S[pad:H - pad, pad:W - pad].mean(dtype=np.float64))
    return float(np.mean(per_channel))


def byte_grid(pred, gt_white):
    """pred | gt_white side by side as threestudio's save_image_grid converts them: clip(0, 1) * 255 in float32, astype(uint8)"""
    both = np.concatenate([np.asarray(pred, np.float32), np.asarray(gt_white, np.float32)], axis=-2)
    return (both.clip(0, 1) * np.float32(255.0)).astype(np.uint8)


def lpips_inputs(pred, gt_white):
    """x * 2 - 1 in float32, as the reference feeds its LPIPS network"""
    return (np.asarray(pred, np.float32) * np.float32(2) - np.float32(1)), (np.asarray(gt_white, np.float32) * np.float32(2) - np.float32(1))


def image_metrics(pred, gt_rgb, gt_mask):
    """one image [H, W, 3] -> dict of the restated values"""
    gw = white_target(gt_rgb, gt_mask)
    p2, g2 = lpips_inputs(pred, gw)
    return {"gt_white": gw, "mse": mse(pred, gw), "psnr": psnr(pred, gw), "ssim": ssim7(pred, gw), "pred2": p2, "gt2": g2,
            "grid": byte_grid(pred, gw)}


def make_case(N, H, W, kind="random", noise=0.05, mask="blob", seed=0):
    """Seeded float32 inputs -> pred [N,H,W,3], gt_rgb [N,H,W,3], gt_mask [N,H,W].  kind: "random" (uniform noise target), "smooth"
    (a low-frequency target) or "white" (a target that is mostly 1.0); pred = gt_white + noise * normal, which leaves [0, 1] a little.
    mask: "inside" (all ones), "outside" (all zeros), "checker" (5x5 cells), "half" (inside, but a band holds exactly 0.5, which
    counts as outside) or "blob" (an ellipse)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    if kind == "random":
        gt = rng.random((N, H, W, 3))
    elif kind == "smooth":
        ph = rng.random((N, 1, 1, 3)) * 6.0
        gt = 0.5 + 0.4 * np.sin(0.21 * xx[None, ..., None] + 0.13 * yy[None, ..., None] + ph)
    elif kind == "white":
        gt = np.where(rng.random((N, H, W, 1)) < 0.9, 1.0, rng.random((N, H, W, 3)))
    else:
        raise ValueError(kind)
    if mask == "inside":
        m = np.ones((N, H, W))
    elif mask == "outside":
        m = np.zeros((N, H, W))
    elif mask == "checker":
        m = np.broadcast_to((((yy // 5) + (xx // 5)) % 2), (N, H, W)).copy()
    elif mask == "half":
        m = np.ones((N, H, W))
        m[:, H // 3:, : max(1, W // 2)] = 0.5
    elif mask == "blob":
        m = np.broadcast_to((((yy - 0.5 * H) / (0.4 * H)) ** 2 + ((xx - 0.45 * W) / (0.35 * W)) ** 2 <= 1.0), (N, H, W)).astype(np.float64)
    else:
        raise ValueError(mask)
    gt, m = gt.astype(np.float32), m.astype(np.float32)
    pred = (white_target(gt, m) + noise * rng.standard_normal((N, H, W, 3))).astype(np.float32)
    return pred, gt, m
