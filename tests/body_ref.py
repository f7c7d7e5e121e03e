"""Restatements for soar_amd/body.py (csrc/body.hip): the body model's vertex forward in torch (any dtype: float64 is the
yardstick, float32 the composition a user without the kernel would run), and midpoint subdivision, vertex normals and surfel
frames in numpy.  Also the small test meshes."""
import numpy as np
import torch

from soar_amd import smplx_joints as sj

FLOOR = 1e-6          # of the largest magnitude


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def worst(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def bar_check(name, hip, f32, f64, report=None):
    """HIP against float64 may be at most 4 x (float32 against float64), floor 1e-6: relative L2 and worst element over the largest
    magnitude.  The float32 yardstick itself is capped at 1e-4 so that a broken restatement fails.  Prints before it asserts."""
    hip, f32, f64 = (np.asarray(torch.as_tensor(x).detach().cpu().numpy() if isinstance(x, torch.Tensor) else x) for x in (hip, f32, f64))
    d_hip, d_t, w_hip, w_t = rel_l2(hip, f64), rel_l2(f32, f64), worst(hip, f64), worst(f32, f64)
    line = f"{name}: rel-L2 hip {d_hip:.3e} f32 {d_t:.3e} | worst hip {w_hip:.3e} f32 {w_t:.3e}"
    print(line)
    if report is not None:
        report.append(line)
    assert np.isfinite(hip).all(), name
    assert d_t <= 1e-4 and w_t <= 1e-4, (name, d_t, w_t)
    assert d_hip <= max(4 * d_t, FLOOR), (name, d_hip, d_t)
    assert w_hip <= max(4 * w_t, FLOOR), (name, w_hip, w_t)


# ---- the body model ----------------------------------------------------------------------------------------------------------

def posedirs_from_factors(U, Wt):
    """posedirs = U @ Wt, float32, as a fixed sequence of rank-1 updates in float64 (the same bits on every machine)."""
    U, Wt = np.asarray(U, np.float64), np.asarray(Wt, np.float64)
    acc = np.zeros((U.shape[0], Wt.shape[1]), np.float64)
    for r in range(U.shape[1]):
        acc += U[:, r:r + 1] * Wt[r:r + 1, :]
    return acc.astype(np.float32)


def lbs_vertices(m, betas, pose, transl=None, dtype=torch.float64, device="cpu"):
    """lbs() of the body model plus transl: template + shape blend + pose correctives, skinned.  -> [B,V,3] in ``dtype``."""
    c = lambda x: torch.as_tensor(x).to(device=device, dtype=dtype)
    vt, sd, pd, Jr, W = c(m.v_template), c(m.shapedirs), c(m.posedirs), c(m.J_regressor), c(m.lbs_weights)
    parents = torch.as_tensor(m.parents).long()
    betas, pose = c(betas), c(pose)
    B = pose.shape[0]
    betas = betas.expand(B, -1)
    v_shaped = vt[None] + torch.einsum("bl,mkl->bmk", betas, sd)
    J = torch.einsum("ji,bik->bjk", Jr, v_shaped)
    R = sj.batch_rodrigues(pose.reshape(-1, 3)).view(B, -1, 3, 3)
    feat = (R[:, 1:] - torch.eye(3, dtype=dtype, device=device)).reshape(B, -1)
    v_posed = v_shaped + torch.matmul(feat, pd).view(B, -1, 3)
    A = sj.rigid_transforms(R, J, parents.to(device))
    T = torch.matmul(W, A.view(B, -1, 16)).view(B, -1, 4, 4)
    v = torch.einsum("bvxy,bvy->bvx", T[..., :3, :3], v_posed) + T[..., :3, 3]
    if transl is not None:
        v = v + c(transl)[:, None]
    return v


# ---- meshes ------------------------------------------------------------------------------------------------------------------

def subdivide_np(verts, faces):
    """One midpoint subdivision.  New vertices in ascending order of the key (min << 32) | max; children of (a, b, c) at rows
    4 f .. 4 f + 3: (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca).  Midpoints in the dtype of ``verts``."""
    verts, faces = np.asarray(verts), np.asarray(faces, np.int64)
    V, F = verts.shape[0], faces.shape[0]
    e = np.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], axis=1).reshape(-1, 2)       # [3F,2]: ab, bc, ca per face
    key = (e.min(1).astype(np.uint64) << np.uint64(32)) | e.max(1).astype(np.uint64)
    uniq, inv = np.unique(key, return_inverse=True)
    a, b = (uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xffffffff)).astype(np.int64)
    mid = ((verts[a] + verts[b]) * verts.dtype.type(0.5)).astype(verts.dtype)
    m = V + inv.reshape(F, 3)
    ab, bc, ca = m[:, 0], m[:, 1], m[:, 2]
    A, B, C = faces[:, 0], faces[:, 1], faces[:, 2]
    ch = np.stack([A, ab, ca, ab, B, bc, ca, bc, C, ab, bc, ca], axis=1).reshape(4 * F, 3)
    return np.concatenate([verts, mid]).astype(verts.dtype), ch.astype(np.int32)


def _normalize(x, eps=1e-12):
    n = np.sqrt((x * x).sum(-1, keepdims=True))
    return x / np.maximum(n, x.dtype.type(eps))


def vertex_normals_np(verts, faces, weighting="angle", dtype=np.float64):
    """normalize(sum over a vertex's face corners of weight * unit face normal); normalize = x / max(|x|, 1e-12)."""
    v, f = np.asarray(verts).astype(dtype), np.asarray(faces, np.int64)
    p = v[f]                                                           # [F,3,3]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.sqrt((n * n).sum(-1))
    unit = n / np.maximum(ln, dtype(1e-12))[:, None]
    out = np.zeros_like(v)
    for c in range(3):
        if weighting == "area":
            w = dtype(0.5) * ln
        elif weighting == "uniform":
            w = np.ones_like(ln)
        else:
            u, q = p[:, (c + 1) % 3] - p[:, c], p[:, (c + 2) % 3] - p[:, c]
            x = np.cross(u, q)
            w = np.arctan2(np.sqrt((x * x).sum(-1)), (u * q).sum(-1))
        np.add.at(out, f[:, c], (w[:, None] * unit).astype(dtype))
    return _normalize(out)


def frames_np(normals, rand_dir, dtype=np.float64):
    """[P,3,3] with columns (ux, uy, uz): ux = normalize(uz x rand), uy = normalize(uz x ux)."""
    uz, rd = np.asarray(normals).astype(dtype), np.asarray(rand_dir).astype(dtype)
    ux = _normalize(np.cross(uz, rd))
    uy = _normalize(np.cross(uz, ux))
    return np.stack([ux, uy, uz], axis=-1)


def quat_to_mat_np(q):
    q = np.asarray(q, np.float64)
    r, i, j, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    s = 2.0 / (q * q).sum(-1)
    m = np.stack([1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r),
                  s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r),
                  s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)], axis=-1)
    return m.reshape(-1, 3, 3)


def icosahedron():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], np.int32)
    return v / np.linalg.norm(v, axis=1, keepdims=True), f


def icosphere(levels, dtype=np.float32):
    """Unit icosphere, outward-facing: 10 * 4^levels + 2 vertices (levels = 5: 10 242)."""
    v, f = icosahedron()
    for _ in range(levels):
        v, f = subdivide_np(v, f)
        v = v / np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(dtype), f


def open_strip(n=40, seed=3, dtype=np.float32):
    """An open triangle strip of 2 n vertices with jittered heights, plus two vertices that no face uses."""
    rng = np.random.default_rng(seed)
    x = np.arange(n, dtype=np.float64)
    v = np.concatenate([np.stack([x, np.zeros(n), 0.2 * rng.standard_normal(n)], 1),
                        np.stack([x + 0.5, np.ones(n), 0.2 * rng.standard_normal(n)], 1), [[-5.0, 3.0, 1.0], [7.0, -4.0, 2.0]]])
    f = []
    for i in range(n - 1):
        f += [[i, i + 1, n + i], [i + 1, n + i + 1, n + i]]
    return v.astype(dtype), np.array(f, np.int32)


def nonmanifold(dtype=np.float32):
    """Three triangles around the edge (0, 1) -- a non-manifold edge -- next to a strip that shares vertex 1."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, -0.3, 1], [0.5, -0.8, -0.7], [2, 0.2, 0.1], [1.6, 1.1, -0.2]], np.float64)
    f = np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4], [1, 5, 6], [1, 6, 2]], np.int32)
    return v.astype(dtype), f


def mesh_stats(verts, faces):
    """(V, E, F, total area, unit normals [F,3]) in float64."""
    v, f = np.asarray(verts, np.float64), np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    E = np.unique(e, axis=0).shape[0]
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    ln = np.linalg.norm(n, axis=1)
    return v.shape[0], E, f.shape[0], 0.5 * ln.sum(), n / np.maximum(ln, 1e-300)[:, None]
