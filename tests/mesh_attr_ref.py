"""NumPy float64 restatement of csrc/mesh_attr.hip (soar_amd/mesh.py: vertex_attributes, adjacency, smooth, prune_by_quality) and the
fixtures of tests/test_mesh_attr_cpu.py / test_mesh_attr_gpu.py.  Everything is generated in code from fixed seeds.

The contract ("Colour, smoothing, skinning"):
  * neighbours: the k nearest surfel centres of a vertex by squared distance, nearest first, ties to the lower index;
  * colour: the mean of their colours added in that order, clamped to [0,1]; quality: the squared distance to the nearest;
  * adjacency: row i = for every face at vertex i its two other corners, ascending (a neighbour across an edge of m faces stands m
    times); border[i] = some neighbour stands exactly once;
  * smoothing step: P' = (P + S) / (n + 1), S the sum of the row's positions -- of a border vertex only those that stand once --,
    n the number of terms, n = 0 keeps P;
  * pruning: vertices with quality > thresh go, faces that touch one go, the rest keep their order, keep[new] = old."""
from typing import NamedTuple

import numpy as np

GAP = 1e-5            # relative gap between consecutive neighbour distances below which float32 could order them differently


class Fixture(NamedTuple):
    name: str
    verts: np.ndarray        # [V,3] float32
    faces: np.ndarray        # [F,3] int32


# ---- fixtures --------------------------------------------------------------------------------------------------------------------

def icosahedron():
    """unit icosahedron -> (verts [12,3] float64, faces [20,3])"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], dtype=np.float64)
    v /= np.linalg.norm(v[0])
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], dtype=np.int32)
    return v, f


def icosphere(levels):
    v, f = icosahedron()
    v = [tuple(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = (np.array(v[a]) + np.array(v[b])) / 2.0
                mid[key] = len(v)
                v.append(tuple(p / np.linalg.norm(p)))
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [[a, ab, ca], [ab, b, bc], [ca, bc, c], [ab, bc, ca]]
        f = np.array(nf, dtype=np.int32)
    return np.array(v, dtype=np.float64), f


def open_grid(n):
    """n x n vertices in the plane z = 0 over [-0.5, 0.5]^2, every cell split along the same diagonal; vertex id = i * n + j"""
    a = np.linspace(-0.5, 0.5, n)
    v = np.stack([np.repeat(a, n), np.tile(a, n), np.zeros(n * n)], 1)
    f = []
    for i in range(n - 1):
        for j in range(n - 1):
            p = i * n + j
            f += [[p, p + n, p + n + 1], [p, p + n + 1, p + 1]]
    return v, np.array(f, dtype=np.int32)


def disc(rim, seed):
    """an open fan: a centre (vertex 0, `rim` faces) and `rim` rim vertices, heights from `seed`: rim + 1 vertices"""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(rim) / rim
    r = 0.45 + 0.05 * rng.random(rim)
    v = np.concatenate([[[0.0, 0.0, 0.1]], np.stack([r * np.cos(ang), r * np.sin(ang), 0.1 * rng.standard_normal(rim)], 1)])
    f = np.array([[0, 1 + k, 1 + (k + 1) % rim] for k in range(rim)], dtype=np.int32)
    return v, f


def _fx(name, v, f):
    return Fixture(name, np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3))


def fixtures():
    v, f = icosphere(2)
    out = [_fx("icosphere2", 0.5 * v, f)]
    v, f = open_grid(9)
    out.append(_fx("grid9", v, f))
    # three faces on the edge (0, 1)
    out.append(_fx("fan3", [[0, 0, -0.3], [0, 0, 0.3], [0.4, 0, 0], [-0.2, 0.35, 0.05], [-0.2, -0.35, -0.05]],
                   [[0, 1, 2], [0, 1, 3], [0, 1, 4]]))
    # a tetrahedron and a vertex no face uses
    out.append(_fx("isolated", [[0.3, 0.3, 0.3], [-0.3, -0.3, 0.3], [-0.3, 0.3, -0.3], [0.3, -0.3, -0.3], [0.1, 0.2, 0.45]],
                   [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]))
    out.append(_fx("single", [[0.1, -0.2, 0.3]], np.zeros((0, 3))))
    v, f = disc(64, 3)
    out.append(_fx("disc65", v, f))            # one vertex past a wavefront
    v, f = disc(256, 4)
    out.append(_fx("disc257", v, f))           # one vertex past a workgroup; a row of 512 entries
    return out


N_SURFELS, SURFEL_SEED = 300, 7


def surfels():
    """-> (centres [300,3] float32 in [-0.6, 0.6]^3, colours [300,3] float32 in [-0.5, 1.5]: the clamp has work to do)"""
    rng = np.random.default_rng(SURFEL_SEED)
    pts = (1.2 * rng.random((N_SURFELS, 3)) - 0.6).astype(np.float32)
    col = (2.0 * rng.random((N_SURFELS, 3)) - 0.5).astype(np.float32)
    return pts, col


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def knn(verts, pts, k):
    """-> (idx [V,k] int32, d2 [V,k] float64): the k nearest points, nearest first, ties to the lower index"""
    v, p = np.asarray(verts, np.float64), np.asarray(pts, np.float64)
    d2 = ((v[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    order = np.lexsort((np.broadcast_to(np.arange(len(p)), d2.shape), d2), axis=1)[:, :k]
    return order.astype(np.int32), np.take_along_axis(d2, order, 1)


def min_relative_gap(verts, pts, k):
    """the least (d_{r+1} - d_r) / d_{r+1} over every vertex and the ranks r = 0 .. k-1 (the last one is the gap between the k-th
    neighbour and the first one left out)"""
    _, d2 = knn(verts, pts, k + 1)
    return float(((d2[:, 1:] - d2[:, :-1]) / d2[:, 1:]).min())


def transfer(verts, pts, colors, k):
    """-> (idx, color [V,3] float64, quality [V] float64, d2 [V,k] float64)"""
    idx, d2 = knn(verts, pts, k)
    c = np.asarray(colors, np.float64)[idx].mean(1)
    return idx, np.clip(c, 0.0, 1.0), d2[:, 0], d2


def color_float32(colors, idx):
    """the kernel's arithmetic: float32 adds in rank order, one float32 division, the clamp"""
    c = np.asarray(colors, np.float32)
    acc = np.zeros((idx.shape[0], 3), np.float32)
    for r in range(idx.shape[1]):
        acc = (acc + c[idx[:, r]]).astype(np.float32)
    return np.clip((acc / np.float32(idx.shape[1])).astype(np.float32), np.float32(0), np.float32(1))


def adjacency(V, faces):
    """-> (row_start [V+1] int32, nbr [6F] int32, border [V] bool)"""
    rows = [[] for _ in range(V)]
    for a, b, c in np.asarray(faces).tolist():
        rows[a] += [b, c]
        rows[b] += [c, a]
        rows[c] += [a, b]
    rows = [sorted(r) for r in rows]
    row_start = np.zeros(V + 1, np.int32)
    row_start[1:] = np.cumsum([len(r) for r in rows])
    nbr = np.array([j for r in rows for j in r], dtype=np.int32)
    border = np.array([any(r.count(j) == 1 for j in r) for r in rows], dtype=bool)
    return row_start, nbr, border


def smooth_step(verts, row_start, nbr, border):
    v = np.asarray(verts, np.float64)
    out = v.copy()
    for i in range(len(v)):
        row = nbr[row_start[i]:row_start[i + 1]].tolist()
        if border[i]:
            row = [j for j in row if row.count(j) == 1]
        if row:
            out[i] = (v[i] + v[row].sum(0)) / (len(row) + 1)
    return out


def smooth(verts, faces, steps):
    v = np.asarray(verts, np.float64)
    adj = adjacency(len(v), faces)
    for _ in range(steps):
        v = smooth_step(v, *adj)
    return v


def max_terms(V, faces):
    """the longest row: the largest n_i any smoothing sum can have"""
    row_start, _, _ = adjacency(V, faces)
    return int(np.diff(row_start).max()) if V else 0


def prune(verts, faces, quality, thresh):
    """-> (verts', faces', keep [V'] int32)"""
    q = np.asarray(quality)
    kv = ~(q > thresh)
    faces = np.asarray(faces).reshape(-1, 3)
    kf = kv[faces].all(1) if len(faces) else np.zeros(0, bool)
    new = np.cumsum(kv) - 1
    keep = np.nonzero(kv)[0].astype(np.int32)
    return np.asarray(verts)[kv], new[faces[kf]].astype(np.int32).reshape(-1, 3), keep


# ---- parsers for the writers' tests --------------------------------------------------------------------------------------------

def parse_obj(path):
    """-> (v [V,3 or 6] float64, f [F,3] int64 zero-based)"""
    v, f = [], []
    for line in open(path).read().splitlines():
        t = line.split()
        if t[0] == "v":
            v.append([float(x) for x in t[1:]])
        elif t[0] == "f":
            f.append([int(x) - 1 for x in t[1:]])
        else:
            raise ValueError(line)
    return np.array(v, np.float64).reshape(len(v), -1), np.array(f, np.int64).reshape(-1, 3)


def parse_ply(path):
    """a binary_little_endian PLY with scalar vertex properties and triangles -> (dict name -> array [V], faces [F,3] int32)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    kinds = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    counts, props, cur = {}, {"vertex": [], "face": []}, None
    for ln in lines[2:-1]:
        t = ln.split()
        if t[0] == "element":
            cur = t[1]
            counts[cur] = int(t[2])
        elif t[0] == "property" and t[1] == "list":
            assert cur == "face" and t[2:] == ["uchar", "int", "vertex_indices"], ln
        elif t[0] == "property":
            props[cur].append((t[2], kinds[t[1]]))
        else:
            raise ValueError(ln)
    vt = np.dtype(props["vertex"])
    V, F = counts["vertex"], counts["face"]
    rec = np.frombuffer(raw, vt, V, end)
    ft = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    fr = np.frombuffer(raw, ft, F, end + V * vt.itemsize)
    assert end + V * vt.itemsize + F * ft.itemsize == len(raw)
    assert (fr["n"] == 3).all()
    return {name: rec[name] for name, _ in props["vertex"]}, fr["v"].astype(np.int32).reshape(-1, 3)
