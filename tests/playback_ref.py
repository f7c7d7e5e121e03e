"""NumPy restatement of csrc/playback.hip, written from the formulas of include/soar_hip.h.

``motion_resample(..., dtype)`` follows the kernel's operations in their order in ``dtype``: float32 is the kernel's own arithmetic
(only sin / cos / arccos / arctan2 differ from the device's by a few ulp), float64 the same formulas at a precision where rounding
does not matter -- the difference between the two is what float32 costs.  ``playback_finish`` restates the output stage.
"""
from __future__ import annotations

import numpy as np

JOINTS = 55
SMALL_ANGLE = 1e-3       # playback.hip: SMALL_ANGLE
LERP_DOT = 0.999999      # playback.hip: LERP_DOT


def quat_of_axis_angle(a: np.ndarray) -> np.ndarray:
    """a [..., 3] -> (w, x, y, z) [..., 4] in a's dtype"""
    dt = a.dtype.type
    ax, ay, az = a[..., 0], a[..., 1], a[..., 2]
    t2 = ax * ax + ay * ay + az * az
    t = np.sqrt(t2)
    h = dt(0.5) * t
    small = t < dt(np.float32(SMALL_ANGLE))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(small, dt(0.5) - t2 / dt(48.0), np.sin(h) / t)
    return np.stack([np.cos(h), s * ax, s * ay, s * az], axis=-1)


def normalised(q: np.ndarray) -> np.ndarray:
    w, x, y, z = (q[..., i] for i in range(4))
    n = np.sqrt(w * w + x * x + y * y + z * z)
    return q / n[..., None]


def slerp(q: np.ndarray, r: np.ndarray, u) -> np.ndarray:
    """q, r [..., 4], u broadcastable to [...]: the kernel's slerp (flip, lerp branch above LERP_DOT, normalisation)"""
    dt = q.dtype.type
    u = np.broadcast_to(np.asarray(u, q.dtype), q.shape[:-1])
    dot = q[..., 0] * r[..., 0] + q[..., 1] * r[..., 1] + q[..., 2] * r[..., 2] + q[..., 3] * r[..., 3]
    flip = dot < 0
    r = np.where(flip[..., None], -r, r)
    dot = np.where(flip, -dot, dot)
    lerp = dot > dt(np.float32(LERP_DOT))
    with np.errstate(divide="ignore", invalid="ignore"):
        th = np.arccos(np.minimum(dot, dt(1.0)))
        sn = np.sin(th)
        a = np.where(lerp, dt(1.0) - u, np.sin((dt(1.0) - u) * th) / sn)
        b = np.where(lerp, u, np.sin(u * th) / sn)
    return normalised(a[..., None] * q + b[..., None] * r)


def times_yaw(q: np.ndarray, yaw: np.ndarray) -> np.ndarray:
    """q (x) (cos(yaw / 2), 0, sin(yaw / 2), 0): R <- R Ry(yaw)"""
    dt = q.dtype.type
    c, s = np.cos(dt(0.5) * yaw), np.sin(dt(0.5) * yaw)
    w, x, y, z = (q[..., i] for i in range(4))
    return np.stack([w * c - y * s, x * c - z * s, y * c + w * s, z * c + x * s], axis=-1)


def axis_angle_of_quat(q: np.ndarray) -> np.ndarray:
    dt = q.dtype.type
    q = np.where((q[..., 0] < 0)[..., None], -q, q)
    w, x, y, z = (q[..., i] for i in range(4))
    n2 = x * x + y * y + z * z
    n = np.sqrt(n2)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(n < dt(np.float32(SMALL_ANGLE)), dt(2.0) + n2 / dt(3.0), (dt(2.0) * np.arctan2(n, w)) / n)
    return k[..., None] * q[..., 1:]


def motion_resample(key_pose, key_transl, key_expr, t, yaw=None, dtype=np.float64):
    """key_pose [K,55,3], key_transl [K,3], key_expr [K,E], t [F], yaw [F] or None (float32 arrays, as the kernel gets them)
    -> pose [F,55,3], transl [F,3], expr [F,E] in ``dtype``."""
    kp, kt, ke = (np.asarray(x, np.float32).astype(dtype) for x in (key_pose, key_transl, key_expr))
    K = kp.shape[0]
    t32 = np.asarray(t, np.float32)
    tc32 = np.fmin(np.fmax(t32, np.float32(0)), np.float32(K - 1))       # (fmaxf: a NaN time samples key 0)
    i0 = np.floor(tc32).astype(np.int64)
    i1 = np.minimum(i0 + 1, K - 1)
    u32 = tc32 - i0.astype(np.float32)                    # exact in float32 (Sterbenz), so the same number in either dtype
    u = u32.astype(dtype)
    F = t32.shape[0]
    yw = np.zeros((F, JOINTS), dtype)
    if yaw is not None:
        yw[:, 0] = np.asarray(yaw, np.float32).astype(dtype)
    p0, p1 = kp[i0], kp[i1]                               # [F,55,3]
    q = quat_of_axis_angle(p0)
    on_key = (u == 0)[:, None]
    q = np.where(on_key[..., None], q, slerp(q, quat_of_axis_angle(p1), u[:, None]))
    turned = yw != 0
    q = np.where(turned[..., None], times_yaw(q, yw), q)
    pose = np.where((on_key & ~turned)[..., None], p0, axis_angle_of_quat(q))
    one = np.dtype(dtype).type(1.0)
    lin = lambda v: np.where((u == 0)[:, None], v[i0], (one - u)[:, None] * v[i0] + u[:, None] * v[i1])
    return pose, lin(kt), lin(ke)


def rotation_matrices(a: np.ndarray) -> np.ndarray:
    """axis-angle [..., 3] -> [..., 3, 3] in float64 (Rodrigues with the quaternion's terms: exact at every angle)"""
    q = normalised(quat_of_axis_angle(np.asarray(a, np.float64)))
    w, x, y, z = (q[..., i] for i in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1)
    return R.reshape(a.shape[:-1] + (3, 3))


def rot_y(angle) -> np.ndarray:
    """Ry(angle) [..., 3, 3] in float64: euler2mat(angle, 0, 0, "syxz")"""
    angle = np.asarray(angle, np.float64)
    c, s, o, z = np.cos(angle), np.sin(angle), np.ones_like(angle), np.zeros_like(angle)
    return np.stack([c, z, s, z, o, z, -s, z, c], axis=-1).reshape(angle.shape + (3, 3))


def to_byte(x: np.ndarray) -> np.ndarray:
    """torchvision's save_image conversion in float32: multiply, add, clamp, truncate; NaN -> 0"""
    s = np.asarray(x, np.float32) * np.float32(255.0) + np.float32(0.5)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(s), np.float32(0), np.minimum(np.maximum(s, np.float32(0)), np.float32(255)))
    return s.astype(np.int32).astype(np.uint8)


def playback_finish(render, normal, mask, occ=None, normal_as_rgb=False):
    """render, normal, occ [B,3,H,W], mask [B,1,H,W] float32 -> rgb, normal, occ (or None) [B,H,W,4] and mask [B,H,W], uint8"""
    render, normal, mask = (np.asarray(x, np.float32) for x in (render, normal, mask))
    if normal_as_rgb:
        normal = normal * np.float32(0.5) + np.float32(0.5)
    a = to_byte(mask)                                                     # [B,1,H,W]
    rgba = lambda img: np.ascontiguousarray(np.concatenate([to_byte(img), a], axis=1).transpose(0, 2, 3, 1))
    return rgba(render), rgba(normal), None if occ is None else rgba(np.asarray(occ, np.float32)), a[:, 0]


def crafted_values() -> np.ndarray:
    """float32 values where the conversion can go wrong: every k / 255 and its two float32 neighbours, every (k + 0.5) / 255 (where
    the truncation steps) and its neighbours, values below 0 and above 1, infinities, NaN"""
    k = np.arange(256, dtype=np.float64)
    vals = []
    for base in (k / 255.0, (k + 0.5) / 255.0):
        b = base.astype(np.float32)
        vals += [b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))]
    extra = np.array([-1.0, -1e-3, -1e-8, -0.0, 0.0, 1e-8, 1.0 + 1e-6, 1.002, 1.5, 2.0, 300.0, 1e30, -1e30, np.inf, -np.inf, np.nan],
                     np.float32)
    return np.concatenate(vals + [extra]).astype(np.float32)


def motion_case():
    """The inputs of the motion tests: K = 3 keys, E = 10, F = 9 times.  Among the 55 joints: joint 3 has two identical keys (the lerp
    branch), joint 4 a pair of keys whose quaternions have a negative dot (the flip), joint 5 a rotation 5e-4 short of pi, joint 6 is
    zero in every key, joint 7 zero in the last key.  -> key_pose [3,55,3], key_transl [3,3], key_expr [3,10], t [9], yaw [9]."""
    rng = np.random.default_rng(0)
    K, E = 3, 10
    kp = rng.normal(0, 0.6, (K, JOINTS, 3)).astype(np.float32)
    kp[1, 3] = kp[0, 3]
    kp[0, 4] = (0.0, 0.0, 0.4)
    kp[1, 4] = (0.0, 0.0, 2 * np.pi - 1.0)
    kp[1, 5] = (np.array([1.0, 2.0, 2.0]) / 3.0 * (np.pi - 5e-4)).astype(np.float32)
    kp[:, 6] = 0.0
    kp[2, 7] = 0.0
    kt = rng.normal(0, 1, (K, 3)).astype(np.float32)
    ke = rng.normal(0, 1, (K, E)).astype(np.float32)
    t = np.array([0.0, K - 1, 1.0, 0.5, 1e-4, 1 - 1e-4, 1.5, 1 + 1e-4, 2 - 1e-4], np.float32)
    yaw = np.array([0.0, 0.0, 0.0, 0.7, 0.0, 3.0, 6.1, 0.0, -2.0], np.float32)
    return kp, kt, ke, t, yaw
