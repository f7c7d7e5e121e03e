"""CPU restatements for the mesh-export tests (soar_amd/mesh.py, csrc/mesh.hip): a pure-Python marching cubes driven by the
generated case table, mesh-topology checks, the TSDF integration in float64 and analytic signed-distance fields."""
from __future__ import annotations

import importlib.util
import os
import re
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "soar_amd", "csrc")


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mcubes_table", os.path.join(CSRC, "gen_mcubes_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_table():
    """(edge lower corners [12], triangles per case [256] of (e0, e1, e2)) parsed from the committed mcubes_table.h"""
    text = open(os.path.join(CSRC, "mcubes_table.h")).read()
    nums = lambda s: [int(x) for x in re.findall(r"-?\d+", s)]
    mt = int(re.search(r"#define SOAR_MC_MAX_TRIS (\d+)", text).group(1))
    corner = nums(re.search(r"kMcEdgeCorner\[12\] = \{([^}]*)\}", text).group(1))
    ntri = nums(re.search(r"kMcNumTris\[256\] = \{([^}]*)\}", text).group(1))
    body = text[text.index("kMcTris[256]"):]
    rows = re.findall(r"\{([-\d, ]+)\}", body)
    assert len(corner) == 12 and len(ntri) == 256 and len(rows) == 256
    tris = []
    for c in range(256):
        r = nums(rows[c])
        assert len(r) == 3 * mt
        tris.append([tuple(r[3 * t:3 * t + 3]) for t in range(ntri[c])])
        assert all(v == -1 for v in r[3 * ntri[c]:])
    return corner, tris


_TABLE = None


def table():
    global _TABLE
    if _TABLE is None:
        _TABLE = load_table()
    return _TABLE


def marching_cubes(values: np.ndarray, level: float = 0.0, valid=None):
    """The kernel's algorithm, restated: vertex ids by (voxel, axis), triangles by (cell, table order); float32 placement."""
    corner, tris = table()
    f = np.asarray(values, dtype=np.float32)
    X, Y, Z = f.shape
    lev = np.float32(level)
    ok = np.ones(f.shape, bool) if valid is None else np.asarray(valid, bool)
    inside = f < lev
    vid = {}
    verts = []
    for x in range(X):
        for y in range(Y):
            for z in range(Z):
                if not ok[x, y, z]:
                    continue
                for ax in range(3):
                    j = [x, y, z]
                    j[ax] += 1
                    if j[ax] >= f.shape[ax] or not ok[tuple(j)] or inside[x, y, z] == inside[tuple(j)]:
                        continue
                    f0, f1 = f[x, y, z], f[tuple(j)]
                    t = np.float32(np.float32(lev - f0) / np.float32(f1 - f0))
                    p = [np.float32(x), np.float32(y), np.float32(z)]
                    p[ax] = np.float32(p[ax] + t)
                    vid[(x, y, z, ax)] = len(verts)
                    verts.append(p)
    faces = []
    for x in range(X - 1):
        for y in range(Y - 1):
            for z in range(Z - 1):
                cs = [(x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1)) for c in range(8)]
                if not all(ok[c] for c in cs):
                    continue
                case = sum(int(inside[cs[c]]) << c for c in range(8))
                for tri in tris[case]:
                    face = []
                    for e in tri:
                        c = cs[corner[e]]
                        face.append(vid[(c[0], c[1], c[2], e >> 2)])
                    faces.append(face)
    return np.array(verts, np.float32).reshape(-1, 3), np.array(faces, np.int32).reshape(-1, 3)


def check_closed_manifold(verts, faces, dims=None):
    """Every edge not on the grid's border lies in exactly two faces, once in each direction.  `dims`: the grid, whose border
    planes (index coordinate 0 or dim - 1) may carry open edges; None: the mesh must be closed everywhere."""
    verts = np.asarray(verts)
    directed = Counter()
    for a, b, c in np.asarray(faces).tolist():
        assert len({a, b, c}) == 3, "degenerate face"
        for u, v in ((a, b), (b, c), (c, a)):
            directed[(u, v)] += 1

    def on_border(u, v):
        if dims is None:
            return False
        for k in range(3):
            for plane in (0.0, float(dims[k] - 1)):
                if verts[u, k] == plane and verts[v, k] == plane:
                    return True
        return False

    for (u, v), n in directed.items():
        if on_border(u, v):
            continue
        assert n == 1, f"edge {(u, v)} used {n} times in one direction"
        assert directed.get((v, u), 0) == 1, f"edge {(u, v)} has no opposite half-edge"


def check_vertices_on_crossings(verts, values, level=0.0, valid=None):
    """Every vertex lies on a sign-changing edge between valid corners, and every such edge carries exactly one vertex."""
    f = np.asarray(values, np.float32)
    ok = np.ones(f.shape, bool) if valid is None else np.asarray(valid, bool)
    inside = f < np.float32(level)
    seen = set()
    for p in np.asarray(verts, np.float32):
        frac = [k for k in range(3) if p[k] != np.floor(p[k])]
        assert len(frac) == 1, f"vertex {p} not strictly inside one grid edge"
        ax = frac[0]
        lo = [int(np.floor(p[k])) for k in range(3)]
        hi = list(lo)
        hi[ax] += 1
        lo, hi = tuple(lo), tuple(hi)
        assert ok[lo] and ok[hi] and inside[lo] != inside[hi], f"vertex {p} on an edge without a crossing"
        assert (lo, ax) not in seen, f"two vertices on edge {lo}, axis {ax}"
        seen.add((lo, ax))
    n_cross = 0
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(0, -1), slice(1, None)
        a, b = tuple(a), tuple(b)
        n_cross += int((ok[a] & ok[b] & (inside[a] != inside[b])).sum())
    assert len(seen) == n_cross


def euler_characteristic(verts, faces):
    faces = np.asarray(faces, np.int64)
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    e.sort(axis=1)
    E = len(np.unique(e, axis=0))
    V = len(np.unique(faces))
    return V - E + len(faces)


def enclosed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def n_components(n_verts, faces):
    parent = list(range(n_verts))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces).tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    used = np.unique(np.asarray(faces))
    return len({find(int(u)) for u in used})


def table_face_count(values, level=0.0, valid=None):
    """The number of triangles the case table gives a field: the sum, over the cells with 8 valid corners, of the case's count."""
    _, tris = table()
    ntri = np.array([len(t) for t in tris])
    f = np.asarray(values, np.float32)
    if min(f.shape) < 2:
        return 0
    ok = np.ones(f.shape, bool) if valid is None else np.asarray(valid, bool)
    inside = f < np.float32(level)
    case = np.zeros(tuple(d - 1 for d in f.shape), np.int64)
    whole = np.ones(case.shape, bool)
    for c in range(8):
        sl = tuple(slice(o, o + d - 1) for o, d in zip((c & 1, (c >> 1) & 1, (c >> 2) & 1), f.shape))
        case |= inside[sl].astype(np.int64) << c
        whole &= ok[sl]
    return int(ntri[case[whole]].sum())


def component_stats(verts, faces):
    """The components of a mesh over its faces' edges, each labelled by its least vertex id -> (label [V], used [V] bool,
    labs [C] ascending, n_faces [C], lo [C,3], hi [C,3], glo [3], ghi [3]): the boxes (float32 coordinates, exact) over the
    vertices that a face uses, per component and of the whole mesh."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3)
    parent = list(range(len(verts)))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]              # halving: the roots are what they are without it, the walks are short
            x = parent[x]
        return x

    for a, b, c in faces.tolist():
        for u, v in ((a, b), (b, c)):
            ru, rv = find(u), find(v)
            parent[max(ru, rv)] = min(ru, rv)
    label = np.array([find(v) for v in range(len(verts))], np.int64)
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    labs, inv = np.unique(label[used], return_inverse=True)
    lo, hi = np.full((len(labs), 3), np.inf, np.float32), np.full((len(labs), 3), -np.inf, np.float32)
    np.minimum.at(lo, inv, verts[used])
    np.maximum.at(hi, inv, verts[used])
    n_faces = np.bincount(np.searchsorted(labs, label[faces[:, 0]]), minlength=len(labs))
    return label, used, labs, n_faces, lo, hi, verts[used].min(0), verts[used].max(0)


def box_diag64(lo, hi):
    d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def box_diag32(lo, hi):
    """the kernel's box_diag: float32 differences, squares and sums in the order written, sqrtf"""
    d = np.asarray(hi, np.float32) - np.asarray(lo, np.float32)
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=np.float32)


def filter_components(verts, faces, min_faces, min_diag_frac, diag=box_diag64):
    """soar_mesh_filter_components restated: a component (labelled by its least vertex id, as n_components finds it) stays when
    it has >= min_faces faces and its bounding-box diagonal is not below min_diag_frac times the diagonal over all vertices
    that a face uses; kept vertices and faces keep their input order.  The diagonals are float64 here, float32 there
    (diag=box_diag32 restates those: tests/test_mesh_cases_cpu.py holds the two together on every case)."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3)
    label, used, labs, n_faces, lo, hi, glo, ghi = component_stats(verts, faces)
    frac = np.float32(min_diag_frac) if diag is box_diag32 else min_diag_frac
    keep_c = (n_faces >= min_faces) & ~(diag(lo, hi) < frac * diag(glo, ghi))
    keep_v = np.zeros(len(verts), bool)
    keep_v[used] = keep_c[np.searchsorted(labs, label[used])]
    new_id = np.cumsum(keep_v) - 1
    return verts[keep_v], new_id[faces[keep_v[faces[:, 0]]]].astype(np.int32).reshape(-1, 3)


def tsdf_reference(depth, opac, viewm, projm, prcp, origin, voxel, dims, trunc, znear=0.2, min_opac=0.5, acc=None, eps_px=1e-3):
    """float64 restatement of soar_tsdf_integrate (torch tensors on the CPU) -> (sum, weight, ambiguous) where `ambiguous`
    flags voxels whose projection lies within eps_px of a pixel-rounding boundary (or on another decision boundary) in a view.
    Non-finite pixels: a NaN opacity, or an opacity >= min_opac with a NaN depth, is no observation; +inf depth gives s = 1,
    -inf depth is hidden, +inf opacity is opaque, -inf opacity is free space -- the arithmetic as written."""
    import torch
    X, Y, Z = dims
    d = torch.float64
    g = torch.stack(torch.meshgrid(torch.arange(X, dtype=d), torch.arange(Y, dtype=d), torch.arange(Z, dtype=d), indexing="ij"), -1)
    # voxel positions as the kernel forms them (float32 multiply, then add), the rest in float64
    p = (g.reshape(-1, 3).float() * torch.tensor(voxel, dtype=torch.float32) + torch.tensor(origin, dtype=torch.float32)).to(d)
    ph = torch.cat([p, torch.ones(len(p), 1, dtype=d)], 1)
    s_acc = torch.zeros(len(p), dtype=d) if acc is None else acc[0].reshape(-1).to(d).clone()
    w_acc = torch.zeros(len(p), dtype=d) if acc is None else acc[1].reshape(-1).to(d).clone()
    amb = torch.zeros(len(p), dtype=torch.bool)
    N, H, W = depth.shape
    for k in range(N):
        V = viewm[k].reshape(4, 4).to(d)
        P = projm[k].reshape(4, 4).to(d)
        zc = (ph @ V)[:, 2]
        h = ph @ P
        ndc = h[:, :2] / h[:, 3:4]
        pix_x = ((ndc[:, 0] + 1.0) * W - 1.0) * 0.5 + W * (float(prcp[k][0]) - 0.5)
        pix_y = ((ndc[:, 1] + 1.0) * H - 1.0) * 0.5 + H * (float(prcp[k][1]) - 0.5)
        ux, uy = pix_x + 0.5, pix_y + 0.5
        fi, fj = torch.floor(ux), torch.floor(uy)
        near = lambda u: (u - torch.round(u)).abs() < eps_px
        seen = (zc > znear) & (fi >= 0) & (fi < W) & (fj >= 0) & (fj < H)
        amb |= (zc - znear).abs() < 1e-5
        amb |= (zc > znear) & (near(ux) | near(uy)) & (ux > -1) & (ux < W + 1) & (uy > -1) & (uy < H + 1)
        ii = fi.clamp(0, W - 1).long()
        jj = fj.clamp(0, H - 1).long()
        o = opac[k].to(d)[jj, ii]
        dep = depth[k].to(d)[jj, ii]
        eta = dep - zc
        free = o < min_opac
        amb |= seen & ((o - min_opac).abs() < 1e-6)
        amb |= seen & ~free & ((eta + trunc).abs() < 1e-5)
        # a NaN opacity, or an opaque pixel with a NaN depth (eta >= -trunc is false), is no observation
        use = seen & ~o.isnan() & (free | (eta >= -trunc))
        s = torch.where(free, torch.ones_like(eta), torch.clamp(eta / trunc, max=1.0))
        s_acc += torch.where(use, s, torch.zeros_like(s))
        w_acc += use.to(d)
    return s_acc.reshape(X, Y, Z), w_acc.reshape(X, Y, Z), amb.reshape(X, Y, Z)


def capsule_sdf(points, capsules):
    """min_i(dist(p, segment_i) - r_i) for points [n,3] (torch) and capsules [(a, b, r)]"""
    import torch
    best = None
    for a, b, r in capsules:
        a = torch.tensor(a, dtype=points.dtype, device=points.device)
        b = torch.tensor(b, dtype=points.dtype, device=points.device)
        ab = b - a
        t = (((points - a) @ ab) / (ab @ ab)).clamp(0, 1)
        d = (points - (a + t[:, None] * ab)).norm(dim=1) - r
        best = d if best is None else torch.minimum(best, d)
    return best


def check_closed_fast(faces, n_verts):
    """Vectorised check_closed_manifold(dims=None) for large meshes: every directed edge once, its opposite once."""
    f = np.asarray(faces, np.int64)
    u = np.concatenate([f[:, 0], f[:, 1], f[:, 2]])
    v = np.concatenate([f[:, 1], f[:, 2], f[:, 0]])
    key = u * n_verts + v
    uniq, cnt = np.unique(key, return_counts=True)
    assert (cnt == 1).all(), f"{int((cnt > 1).sum())} directed edges used more than once"
    rev = v * n_verts + u
    assert np.isin(rev, uniq).all(), "edges without an opposite half-edge"


def n_components_torch(n_verts, faces):
    """Connected components over the faces' edges by min-label propagation (torch, on the faces' device); unused vertices
    are not counted."""
    import torch
    f = faces.long()
    lab = torch.arange(n_verts, device=f.device)
    while True:
        m = lab[f].min(1).values
        new = lab.clone()
        new.scatter_reduce_(0, f.reshape(-1), m.repeat_interleave(3), reduce="amin")
        new = new[new]
        if torch.equal(new, lab):
            break
        lab = new
    return int(torch.unique(lab[f.reshape(-1)]).numel())
