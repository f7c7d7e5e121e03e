"""NumPy restatement of csrc/fitviz.hip, written from the formulas of include/soar_hip.h: integers for coverage (Python
ints: no width to overflow), ``np.float32`` for the blends and the byte rules, ``np.rint`` for the rounding.  Whole images are painted
primitive by primitive in drawing order -- the plain meaning of "the last writer wins" -- with none of the kernel's tiles or culling."""
import numpy as np

F32 = np.float32
COORD_LIMIT = 1 << 20


def centres(px, kp_mask):
    """``px [K,2]`` float32 -> list of ``(cx, cy)`` or None: truncation toward zero, drawn iff masked in, finite, |coord| < 2^20 and
    both integers >= 1."""
    out = []
    for k in range(px.shape[0]):
        x, y = float(px[k, 0]), float(px[k, 1])
        ok = bool(kp_mask[k]) and np.isfinite(x) and np.isfinite(y) and abs(x) < COORD_LIMIT and abs(y) < COORD_LIMIT
        c = (int(x), int(y)) if ok else None                    # int() truncates toward zero
        out.append(c if c is not None and c[0] >= 1 and c[1] >= 1 else None)
    return out


def disc_covers(px, py, c, r):
    dx, dy = px - c[0], py - c[1]
    return dx * dx + dy * dy <= r * r + 1


def limb_covers(px, py, a, b, t):
    dx, dy = b[0] - a[0], b[1] - a[1]
    qx, qy = px - a[0], py - a[1]
    L2, s = dx * dx + dy * dy, qx * dx + qy * dy
    if 0 < s < L2:
        cr = qx * dy - qy * dx
        return 4 * cr * cr <= t * t * L2
    ex, ey = (qx, qy) if s <= 0 else (px - b[0], py - b[1])
    return 4 * (ex * ex + ey * ey) <= t * t


def paint_disc(img, c, r, rgb):
    H, W = img.shape[:2]
    for py in range(max(c[1] - r, 0), min(c[1] + r, H - 1) + 1):
        for px in range(max(c[0] - r, 0), min(c[0] + r, W - 1) + 1):
            if disc_covers(px, py, c, r):
                img[py, px] = rgb


def paint_limb(img, a, b, t, rgb):
    H, W = img.shape[:2]
    g = (t + 1) // 2
    for py in range(max(min(a[1], b[1]) - g, 0), min(max(a[1], b[1]) + g, H - 1) + 1):
        for px in range(max(min(a[0], b[0]) - g, 0), min(max(a[0], b[0]) + g, W - 1) + 1):
            if limb_covers(px, py, a, b, t):
                img[py, px] = rgb


def keypoint_panel(H, W, target_px, fit_px, kp_mask, limbs=None, limb_rgb=None, radius=3, thickness=4, target_rgb=(0, 255, 0),
                   fit_rgb=(255, 0, 0)):
    """Panel 0 before the blend: black, the target set's limbs, its discs, the fit set's limbs, its discs."""
    img = np.zeros((H, W, 3), np.uint8)
    for px, rgb in ((target_px, target_rgb), (fit_px, fit_rgb)):
        cs = centres(px, kp_mask)
        if limbs is not None:
            for (ia, ib), lrgb in zip(np.asarray(limbs).tolist(), np.asarray(limb_rgb).tolist()):
                if cs[ia] is not None and cs[ib] is not None:
                    paint_limb(img, cs[ia], cs[ib], thickness, lrgb)
        for c in cs:
            if c is not None:
                paint_disc(img, c, radius, rgb)
    return img


def blend(c, img):
    """rint(0.6f c + 0.4f img): float32 products and sum, half to even, clamped."""
    v = F32(0.6) * c.astype(F32) + F32(0.4) * img.astype(F32)
    assert v.dtype == F32
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def normal_bytes(prior, mask):
    """``prior [3,H,W]`` float32, ``mask [H,W]`` -> ``[H,W,3]`` uint8: (uint8)((n * 0.5f + 0.5f) * 255.0f) on the body, 0 off it."""
    v = (prior.astype(F32) * F32(0.5) + F32(0.5)) * F32(255.0)
    assert v.dtype == F32
    b = np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8)          # the cast truncates
    return np.where((mask != 0)[None], b, 0).astype(np.uint8).transpose(1, 2, 0)


def halve(strip):
    """``[H,S,3]`` -> ``[H//2,S//2,3]``: (a + b + c + d + 2) >> 2 of every 2 x 2 block; an odd last row or column is dropped."""
    H, S = strip.shape[0] // 2 * 2, strip.shape[1] // 2 * 2
    s = strip[:H, :S].astype(np.int64)
    return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def strips(target_px, fit_px, kp_mask, prior, mask, imgs=None, limbs=None, limb_rgb=None, radius=3, thickness=4, half=False,
           target_rgb=(0, 255, 0), fit_rgb=(255, 0, 0)):
    """``prior [N,3,2,3,H,W]``, ``mask [N,3,2,H,W]`` (host arrays) -> ``[N,H,5W,3]`` or its halved form."""
    N = target_px.shape[0]
    H, W = prior.shape[-2:]
    prior, mask = prior.reshape(N, 3, 2, 3, H, W), mask.reshape(N, 3, 2, H, W)
    out = []
    for n in range(N):
        p0 = keypoint_panel(H, W, target_px[n], fit_px[n], kp_mask, limbs, limb_rgb, radius, thickness, target_rgb, fit_rgb)
        views = [normal_bytes(prior[n, k, 0], mask[n, k, 0]) for k in range(3)]
        p1 = views[0]
        if imgs is not None:
            p0, p1 = blend(p0, imgs[n]), blend(p1, imgs[n])
        s = np.concatenate([p0, p1] + views, axis=1)
        out.append(halve(s) if half else s)
    return np.stack(out)


def yaw_views(verts, pivot, R):
    """``verts [N,V,3]``, ``pivot [N,3]``, ``R [n_views,3,3]`` float32 (R[0] is not used) -> ``[N,n_views,V,3]`` in float32, every
    operation rounded once, in the header's order."""
    verts, pivot, R = verts.astype(F32), pivot.astype(F32), R.astype(F32)
    out = np.empty((verts.shape[0], R.shape[0]) + verts.shape[1:], F32)
    out[:, 0] = verts
    d = verts - pivot[:, None]
    for k in range(1, R.shape[0]):
        for i in range(3):
            out[:, k, :, i] = ((R[k, i, 0] * d[..., 0] + R[k, i, 1] * d[..., 1]) + R[k, i, 2] * d[..., 2]) + pivot[:, None, i]
    assert out.dtype == F32
    return out


def yaw_views64(verts, pivot, R):
    v, p = verts.astype(np.float64), pivot.astype(np.float64)[:, None]
    return np.stack([np.einsum("ij,nvj->nvi", R[k].astype(np.float64), v - p) + p for k in range(R.shape[0])], axis=1)


def residuals(fit_px, target_px, conf, kp_mask, thresh=0.3):
    """``[N,3]`` float32 by the kernel's order of additions: lane l of 64 takes keypoints l, l + 64, ...; then x[l] += x[l ^ off]."""
    N, K = fit_px.shape[:2]
    out = np.zeros((N, 3), F32)
    lanes = np.arange(64)
    for n in range(N):
        f, t = fit_px[n].astype(F32), target_px[n].astype(F32)
        ok = (np.asarray(kp_mask) != 0) & (conf[n].astype(F32) > F32(thresh)) & np.isfinite(f).all(1) & np.isfinite(t).all(1)
        with np.errstate(invalid="ignore", over="ignore"):
            dx, dy = f[:, 0] - t[:, 0], f[:, 1] - t[:, 1]
            d = np.where(ok, np.sqrt(dx * dx + dy * dy), F32(0)).astype(F32)
        s, m = np.zeros(64, F32), np.zeros(64, F32)
        for k in range(K):
            s[k % 64] = s[k % 64] + d[k]
            m[k % 64] = max(m[k % 64], d[k])
        for off in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ off]
            m = np.maximum(m, m[lanes ^ off])
        cnt = int(ok.sum())
        if cnt:
            out[n] = (F32(cnt), s[0] / F32(cnt), m[0])
    return out


def residuals64(fit_px, target_px, conf, kp_mask, thresh=0.3):
    N = fit_px.shape[0]
    out = np.zeros((N, 3))
    for n in range(N):
        f, t = fit_px[n].astype(np.float64), target_px[n].astype(np.float64)
        ok = (np.asarray(kp_mask) != 0) & (conf[n].astype(F32) > F32(thresh)) & np.isfinite(f).all(1) & np.isfinite(t).all(1)
        if ok.any():
            d = np.sqrt(((f[ok] - t[ok]) ** 2).sum(1))
            out[n] = (ok.sum(), d.mean(), d.max())
    return out
