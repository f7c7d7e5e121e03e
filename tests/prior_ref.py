"""The normal-prior renderer's definition restated in NumPy: integer coverage, float64 everywhere else, and a float32
mode of the same restatement (the same operations in the same order in np.float32).  One frame at a time.

    vertex_setup(verts, faces, w2c, K, dtype)            -> dict(xy, snapped, valid, inv_z, normals, well)
    rasterize(snapped, inv_z, normals, faces, H, W, ...) -> dict(face, mask, prior, q, q2) per view (0 front, 1 rear)
    near_ties(res)                                       -> bool [2,H,W]

``q2`` is the runner-up's depth among the faces that are not the winner's vertex triple again: an exact copy of a face has the same
``q`` bit for bit in any precision, so its tie is decided by the index rule -- which the tests check, not excuse.
"""
import numpy as np

SUB = 256
INVALID = -(1 << 31)
GUARD = float(1 << 20)
FLOOR = 1e-6


def csr(faces, V):
    """(offsets [V+1], corners [3F]): per vertex the corners 3 face + corner that name it, ascending -- by a plain loop."""
    rows = [[] for _ in range(V)]
    for f, tri in enumerate(np.asarray(faces).tolist()):
        for c, v in enumerate(tri):
            rows[v].append(3 * f + c)
    off = np.zeros(V + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.array([c for r in rows for c in r], np.int64)


def normalize(x, dt):
    n = np.sqrt((x * x).sum(-1, keepdims=True).astype(dt)).astype(dt)
    return (x / np.maximum(n, dt(1e-12))).astype(dt)


def vertex_setup(verts, faces, w2c, K, dtype=np.float64):
    dt = np.dtype(dtype).type
    v, M, K = np.asarray(verts).astype(dt), np.asarray(w2c).astype(dt), np.asarray(K).astype(dt)
    faces = np.asarray(faces, np.int64)
    rot = lambda a: np.stack([M[r, 0] * a[:, 0] + M[r, 1] * a[:, 1] + M[r, 2] * a[:, 2] for r in range(3)], -1).astype(dt)
    p = (rot(v) + M[None, :3, 3]).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        x = K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2]
        y = K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]
        valid = (p[:, 2] > dt(1e-6)) & (np.abs(x) <= dt(GUARD)) & (np.abs(y) <= dt(GUARD))
        xy = np.stack([x, y], -1)
        snapped = np.where(valid[:, None], np.rint(np.where(valid[:, None], xy, 0) * dt(SUB)), INVALID).astype(np.int64)
        inv_z = np.where(valid, dt(1) / p[:, 2], dt(0)).astype(dt)
    acc, scale = np.zeros((v.shape[0], 3), dt), np.zeros(v.shape[0], np.float64)
    if faces.shape[0]:
        a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
        e1, e2 = b - a, c - a
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], -1).astype(dt)
        np.add.at(acc, faces.reshape(-1), np.repeat(cr, 3, axis=0))          # unbuffered, in ascending (face, corner) order
        np.add.at(scale, faces.reshape(-1), np.repeat(np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1), 3))
    # a normal is well-conditioned when its sum is exactly zero (no face, a repeated vertex) or keeps 1e-3 of its terms' scale
    # |e1| |e2|: the cross product of a collinear face is rounding noise, which normalisation blows up to a unit vector of any direction
    length = np.linalg.norm(acc.astype(np.float64), axis=1)
    well = (length == 0) | (length >= 1e-3 * scale)
    return dict(xy=xy, snapped=snapped, valid=valid, inv_z=inv_z, normals=rot(normalize(acc, dt)), well=well)


def _owns(dx, dy):
    return (dy > 0) | ((dy == 0) & (dx > 0))


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def face_samples(snapped, tri, H, W):
    """The pixels face ``tri`` owns: (rows, cols, e [3,n] int64, area, (i0, i1, i2) as oriented) or None."""
    i0, i1, i2 = (int(t) for t in tri)
    P = [snapped[i] for i in (i0, i1, i2)]
    if any(int(p[0]) == INVALID for p in P):
        return None
    (x0, y0), (x1, y1), (x2, y2) = [(int(p[0]), int(p[1])) for p in P]
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if area < 0:
        i1, i2, x1, y1, x2, y2, area = i2, i1, x2, y2, x1, y1, -area
    if area == 0:
        return None
    fl = lambda a: (a - 128) // SUB                          # floor division, negative coordinates included
    jx0, jx1 = max(0, -fl(-min(x0, x1, x2) + 256)), min(W - 1, fl(max(x0, x1, x2)))      # ceil((m - 128) / 256) = -floor((128 - m) / 256)
    jy0, jy1 = max(0, -fl(-min(y0, y1, y2) + 256)), min(H - 1, fl(max(y0, y1, y2)))
    if jx0 > jx1 or jy0 > jy1:
        return None
    jj, ii = np.meshgrid(np.arange(jx0, jx1 + 1, dtype=np.int64), np.arange(jy0, jy1 + 1, dtype=np.int64))
    px, py = SUB * jj + 128, SUB * ii + 128
    e = [_edge(x1, y1, x2, y2, px, py), _edge(x2, y2, x0, y0, px, py), _edge(x0, y0, x1, y1, px, py)]
    o = [_owns(np.int64(x2 - x1), np.int64(y2 - y1)), _owns(np.int64(x0 - x2), np.int64(y0 - y2)), _owns(np.int64(x1 - x0), np.int64(y1 - y0))]
    inside = np.ones(px.shape, bool)
    for ek, ok in zip(e, o):
        inside &= (ek > 0) | ((ek == 0) & ok)
    if not inside.any():
        return None
    return ii[inside], jj[inside], np.stack([ek[inside] for ek in e]), area, (i0, i1, i2)


def face_boxes(snapped, faces):
    """int64 [F,4]: first / last pixel column and first / last row whose sample 256 j + 128 the face's snapped bounding box holds,
    clamped to int16; (32767, -32768, 32767, -32768) for a face that draws nothing (an invalid vertex, zero area, no sample)."""
    out = np.tile(np.array([32767, -32768, 32767, -32768], np.int64), (len(faces), 1))
    for f, tri in enumerate(np.asarray(faces).tolist()):
        P = [[int(x) for x in snapped[i]] for i in tri]
        if any(p[0] == INVALID for p in P):
            continue
        (x0, y0), (x1, y1), (x2, y2) = P
        if (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) == 0:
            continue
        b = [-((128 - min(x0, x1, x2)) // SUB), (max(x0, x1, x2) - 128) // SUB, -((128 - min(y0, y1, y2)) // SUB), (max(y0, y1, y2) - 128) // SUB]
        if b[0] <= b[1] and b[2] <= b[3]:
            out[f] = np.clip(b, -32768, 32767)
    return out


def rasterize(snapped, inv_z, normals, faces, H, W, dtype=np.float64, space="opengl"):
    """Both views.  ``face`` / ``mask`` / ``prior`` as the kernel's; ``q`` the winner's depth and ``q2`` the runner-up's (see the
    module docstring), NaN where there is none."""
    dt = np.dtype(dtype).type
    snapped, faces = np.asarray(snapped, np.int64), np.asarray(faces, np.int64)
    iz, nr = np.asarray(inv_z).astype(dt), np.asarray(normals).astype(dt)
    face = np.full((2, H, W), -1, np.int64)
    q = np.full((2, H, W), np.nan, dt)
    q2 = np.full((2, H, W), np.nan, dt)
    acc = np.zeros((2, H, W, 3), dt)
    rows = {}
    canon = np.array([rows.setdefault(tuple(t), f) for f, t in enumerate(faces.tolist())], np.int64)
    win_canon = np.full((2, H, W), -1, np.int64)
    kept = []
    for f in range(faces.shape[0]):
        s = face_samples(snapped, faces[f], H, W)
        if s is None:
            continue
        ii, jj, e, area, idx = s
        A = dt(area)
        w = [(e[k].astype(dt) / A * iz[idx[k]]).astype(dt) for k in range(3)]
        qf = sum_in_order(w, dt)
        n = sum_in_order([w[k][:, None] * nr[idx[k]][None, :] for k in range(3)], dt)
        kept.append((f, ii, jj, qf))
        for view, sign in ((0, 1), (1, -1)):
            better = (face[view, ii, jj] < 0) | (sign * qf > sign * q[view, ii, jj])     # strict: among equal q the smaller index stays
            bi, bj = ii[better], jj[better]
            q[view, bi, bj], face[view, bi, bj], win_canon[view, bi, bj], acc[view, bi, bj] = qf[better], f, canon[f], n[better]
    for f, ii, jj, qf in kept:                                                             # the runner-up, once the winners are known
        for view, sign in ((0, 1), (1, -1)):
            cur2 = q2[view, ii, jj]
            cand = (win_canon[view, ii, jj] != canon[f]) & (np.isnan(cur2) | (sign * qf > sign * cur2))
            q2[view, ii[cand], jj[cand]] = qf[cand]
    mask = (face >= 0)
    nrm = normalize(acc, dt)
    if space == "opengl":
        nrm = nrm * np.array([1, -1, -1], dt)
    prior = np.where(mask[..., None], nrm, dt(0)).transpose(0, 3, 1, 2)
    return dict(face=face, mask=mask.astype(np.uint8), prior=prior, q=q, q2=q2)


def sum_in_order(terms, dt):
    out = terms[0].astype(dt)
    for t in terms[1:]:
        out = (out + t.astype(dt)).astype(dt)
    return out


def near_ties(res, rel=1e-5):
    """bool [2,H,W]: covered pixels whose best and second-best q lie within ``rel`` relative."""
    q, q2 = res["q"].astype(np.float64), res["q2"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (res["face"] >= 0) & ~np.isnan(q2) & (np.abs(q - q2) <= rel * np.abs(q))


def worst(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)) if a.size else 0.0


def bar_check(name, hip, f32, f64, report=None):
    """HIP against float64 at most 4 x (float32 restatement against float64), floor 1e-6 of the largest magnitude: the worst
    element.  The float32 yardstick itself is capped at 1e-4 so that a broken restatement fails.  Prints before it asserts."""
    w_hip, w_t = worst(hip, f64), worst(f32, f64)
    line = f"{name}: worst hip {w_hip:.3e} f32 {w_t:.3e} bar {max(4 * w_t, FLOOR):.3e}"
    print(line)
    if report is not None:
        report.append(line)
    assert np.isfinite(np.asarray(hip, np.float64)).all(), name
    assert w_t <= 1e-4, (name, w_t)
    assert w_hip <= max(4 * w_t, FLOOR), (name, w_hip, w_t)
