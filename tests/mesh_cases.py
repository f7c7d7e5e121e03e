"""Seeded mesh-extraction cases for tests/test_mesh_cases_cpu.py and tests/test_mesh_gpu.py (soar_amd/mesh.py, csrc/mesh.hip).
CPU only, procedural, no fixture files.

* Fusion (``fusion_case``): the camera recipe of test_fuse_depth_matches_float64_restatement -- fov 55 degrees,
  ``make_c2w(dist, el, az)`` drawn from generator seed 11, prcp in [0.4, 0.6], depth in [2.4, 3.6], opacity 0.1 / 0.9 -- on grids
  that are no cubes, centred on the origin with a longest extent of 2.  ``plant_nonfinite`` writes NaN and +-inf into known pixel
  columns of both planes.
* Marching cubes (``mc_field`` and friends): one random field seen through the three cyclic axis orders, grids of 255 / 256 / 257
  voxels, grids with a dimension of 1, fields of exact ties.
* Component filter: fans of 1..130 faces under a seeded permutation, boxes that sit on the diagonal threshold exactly and one ulp
  either side, vertices no face uses, strips that make the deepest union-find forests, and meshes of a given (V, F).
  Each filter case is a namespace with verts [V,3] float32, faces [F,3] int32, the filter's arguments and, where the case is
  built for a decision, keep_v [V] / keep_f [F]: what must stay."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

# ---- fusion ---------------------------------------------------------------------------------------------------------------------

FOV_DEG, ZNEAR, MIN_OPACITY, AMBIGUOUS_CAP = 55.0, 0.2, 0.5, 0.05
NEAR_DIST = 0.3                                      # `inside`: every second camera this far from the origin, depth in [0.2, 0.8]
FUSION_CASES = {                                     # name -> (views, H, W, dims, every second camera inside the grid)
    "offcube": (5, 31, 45, (37, 5, 66), False),      # three different strides, N = 12210 is no multiple of 256
    "thin": (3, 17, 23, (1, 129, 3), False),         # a dimension of 1
    "inside": (6, 31, 45, (21, 34, 13), True),       # voxels behind a camera and nearer to it than znear
}
CHUNK_CASE = (130, 9, 12, (6, 10, 7), False)         # more views than one call takes (64): fuse_depth's second and third chunk
CHUNK_VIEW = 100                                     # the view of the second chunk that is held against the restatement alone


def centred_grid(dims):
    """-> (origin, voxel): the grid centred on the origin whose longest extent is 2"""
    voxel = 2.0 / (max(dims) - 1)
    return tuple(-0.5 * (d - 1) * voxel for d in dims), voxel


def make_fusion(n, H, W, dims, inside=False, seed=11):
    from soar_amd import synthetic as syn
    gen = torch.Generator().manual_seed(seed)
    fovx = math.radians(FOV_DEG)
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    views, projs, prcps = [], [], []
    for k in range(n):
        el, az = float(torch.rand(1, generator=gen)) * 2 - 1, float(torch.rand(1, generator=gen)) * 6.28
        dist = NEAR_DIST if inside and k % 2 == 1 else 3.0
        wv, full, _ = syn.camera_from_c2w(syn.make_c2w(dist, el, az, target=(0.0, 0.0, 0.0)), fovx, fovy, znear=ZNEAR)
        views.append(wv)
        projs.append(full)
        prcps.append(0.4 + 0.2 * torch.rand(2, generator=gen))
    depth = 2.4 + 1.2 * torch.rand(n, H, W, generator=gen)
    opac = torch.where(torch.rand(n, H, W, generator=gen) < 0.3, 0.1, 0.9)
    if inside:
        depth[1::2] = 0.2 + 0.6 * torch.rand(len(depth[1::2]), H, W, generator=gen)
    origin, voxel = centred_grid(dims)
    return SimpleNamespace(n=n, H=H, W=W, dims=tuple(dims), depth=depth, opac=opac, viewm=torch.stack(views), projm=torch.stack(projs),
                           prcp=torch.stack(prcps), origin=origin, voxel=voxel, trunc=3 * voxel, near_views=list(range(1, n, 2)) if inside else [])


@functools.lru_cache(maxsize=None)
def fusion_case(name):
    return make_fusion(*(CHUNK_CASE if name == "chunk" else FUSION_CASES[name]))


def one_view(case, k):
    """view k of a case as a case of its own"""
    return SimpleNamespace(**{**vars(case), "n": 1, "depth": case.depth[k:k + 1], "opac": case.opac[k:k + 1], "viewm": case.viewm[k:k + 1],
                              "projm": case.projm[k:k + 1], "prcp": case.prcp[k:k + 1], "near_views": []})


def reference(case, R):
    """tests/mesh_ref.tsdf_reference on a case -> (sum, weight, ambiguous), float64"""
    return R.tsdf_reference(case.depth, case.opac, case.viewm, case.projm, case.prcp, case.origin, case.voxel, case.dims, case.trunc,
                            znear=ZNEAR, min_opac=MIN_OPACITY)


def view_z(case):
    """[n, X*Y*Z] float64: the view-space z of every voxel in every view"""
    X, Y, Z = case.dims
    d = torch.float64
    g = torch.stack(torch.meshgrid(torch.arange(X, dtype=d), torch.arange(Y, dtype=d), torch.arange(Z, dtype=d), indexing="ij"), -1)
    p = g.reshape(-1, 3) * case.voxel + torch.tensor(case.origin, dtype=d)
    ph = torch.cat([p, torch.ones(len(p), 1, dtype=d)], 1)
    return torch.stack([(ph @ case.viewm[k].to(d))[:, 2] for k in range(case.n)])


# what is planted, in every view: (kind, plane, value, first column).  A kind fills one whole pixel column, shifted by the view's
# number, so that voxels project into it whatever the camera's elevation; the six columns are three apart
NONFINITE_KINDS = (("depth nan", "depth", float("nan"), 12), ("depth +inf", "depth", float("inf"), 15), ("depth -inf", "depth", float("-inf"), 18),
                   ("opac nan", "opac", float("nan"), 21), ("opac +inf", "opac", float("inf"), 24), ("opac -inf", "opac", float("-inf"), 27))


def plant_nonfinite(case, kinds=None):
    """A copy of the case with the named kinds (default: all) planted; the drawn opacities stay, so a planted depth column crosses
    free-space pixels (opacity 0.1: the depth is not read) and opaque ones."""
    out = SimpleNamespace(**vars(case))
    out.depth, out.opac = case.depth.clone(), case.opac.clone()
    for name, plane, value, col in NONFINITE_KINDS:
        if kinds is None or name in kinds:
            for k in range(case.n):
                getattr(out, plane)[k, :, col + k] = value
    return out


# ---- marching cubes -------------------------------------------------------------------------------------------------------------

MC_BASE = (5, 33, 70)
MC_AXES = {"xyz": (0, 1, 2), "zxy": (2, 0, 1), "yzx": (1, 2, 0)}          # shapes (5, 33, 70), (70, 5, 33), (33, 70, 5)
MC_SIZE_GRIDS = [(3, 5, 17), (4, 8, 8), (1, 1, 257)]                      # 255, 256 and 257 voxels
MC_FLAT_GRIDS = [(1, 40, 40), (40, 1, 40), (40, 40, 1), (1, 1, 40), (1, 40, 1), (40, 1, 1)]
MC_TIE_GRID = (9, 14, 11)


@functools.lru_cache(maxsize=None)
def _mc_base():
    rng = np.random.default_rng(300)
    return rng.standard_normal(MC_BASE).astype(np.float32), rng.uniform(size=MC_BASE) > 0.1


def mc_field(order):
    """-> (field, valid): the one random-normal field (and its 10 % invalid mask) with its axes in the given order, contiguous"""
    f, m = _mc_base()
    return np.ascontiguousarray(np.transpose(f, MC_AXES[order])), np.ascontiguousarray(np.transpose(m, MC_AXES[order]))


def mc_unpermute(verts, order):
    """vertices of mc_field(order)'s mesh with their columns put back into the base field's axis order"""
    out = np.empty_like(verts)
    for i, a in enumerate(MC_AXES[order]):
        out[:, a] = verts[:, i]
    return out


def sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]


def mc_random(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def mc_ties(negative_zeros):
    """A field drawn from {-1, 0, 1}: at level 0 every crossing edge with a 0 end has t = 0 or t = 1 exactly, the vertex sits on a
    grid point and triangles of zero area appear.  negative_zeros: every second 0 is -0.0 (not inside either: -0.0 < 0 is false)."""
    rng = np.random.default_rng(310)
    f = rng.integers(-1, 2, MC_TIE_GRID).astype(np.float32)
    if negative_zeros:
        flat = f.reshape(-1)
        zeros = np.flatnonzero(flat == 0)
        flat[zeros[::2]] = -0.0
    return f


# ---- the component filter -------------------------------------------------------------------------------------------------------

def _permuted(verts, faces, vert_tag, face_tag, seed):
    """vertex ids and face order under a seeded permutation; the tags (per vertex / per face) travel along"""
    rng = np.random.default_rng(seed)
    where = rng.permutation(len(verts))                  # vertex i goes to row where[i]
    order = rng.permutation(len(faces))
    v, vt = np.empty_like(verts), np.empty_like(vert_tag)
    v[where], vt[where] = verts, vert_tag
    return v, where[faces][order].astype(np.int32), vt, face_tag[order]


FAN_MIN_FACES = (1, 63, 64, 65, 131)


@functools.lru_cache(maxsize=None)
def fans():
    """Open fans of k triangles (k + 2 vertices) for k = 1..130, two of each, 10 apart on a grid, vertex ids and face order permuted:
    most waves of faces and of vertices hold several components -> (verts, faces, k of each vertex's fan, k of each face's fan).
    With min_diag_frac = 0 the filter keeps exactly the fans with k >= min_faces."""
    verts, faces, vk, fk = [], [], [], []
    for c, k in enumerate(k for k in range(1, 131) for _ in range(2)):
        base = len(verts)
        cx, cy = 10.0 * (c % 20), -10.0 * (c // 20)
        verts.append((cx, cy, 0.5))
        ang = np.arange(k + 1) * 2 * np.pi / (k + 2)
        verts += [(cx + 3 * np.cos(a), cy + 3 * np.sin(a), 0.0) for a in ang]
        faces += [(base, base + 1 + i, base + 2 + i) for i in range(k)]
        vk += [k] * (k + 2)
        fk += [k] * k
    return _permuted(np.array(verts, np.float32), np.array(faces, np.int64), np.array(vk), np.array(fk), 61)


def fans_case(min_faces):
    verts, faces, vk, fk = fans()
    return SimpleNamespace(verts=verts, faces=faces, min_faces=min_faces, min_diag_frac=0.0, keep_v=vk >= min_faces, keep_f=fk >= min_faces)


def tie_case(permute=False, strays=False):
    """Boxes on the diagonal threshold.  Every z is -2; the faces' vertices span x in [-6, 6], y in [-8, 8]: the whole-mesh diagonal
    is 20 from (12, 16, 0), and min_diag_frac = 0.25 (exact in float32) puts the threshold at 5 in float32 and float64 alike.

      two triangles with a 3 x 4 box      diagonal 5 exactly, not below the threshold: stay
      `shorter`                            a 3 x 4 box between y = -8 and y = -4 whose y = -8 corner is one float32 ulp (2^-21)
                                           nearer: dy = 4 - 2^-21 exactly, dy^2 rounds to 16 - 2^-18, the sum 25 - 2^-18 is a
                                           float32 and its root rounds to 5 - 2^-21 < 5: goes, in float32 as in float64.  (An ulp
                                           taken off a corner at 3 or 4 instead is lost in float32: the sum is 25 or 25 - 2^-19 and
                                           its root rounds to 5.  The filter compares float32 diagonals, so the corner that moves is
                                           the one whose ulp survives.)
      `longer`                             a box from x = 0 to the float32 after 3, 4 high: stays in both
      a unit triangle                      goes
      a strip of 100 triangles             102 vertices with consecutive ids (whole waves in one component when not permuted),
                                           diagonal about 6.4: stays
    strays: three vertices that no face uses, at distance 1000, inserted among the others: they must not count for the whole-mesh
    box (if they did, the threshold would be near 500 and nothing would stay)."""
    up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))
    parts = [([(-6, -8), (-3, -8), (-6, -4)], True), ([(6, 8), (3, 8), (6, 4)], True),
             ([(0, up(-8)), (3, -4), (0, -4)], False), ([(0, -4), (up(3), 0), (0, 0)], True), ([(1, 1), (2, 1), (1, 2)], False)]
    verts, faces, vkeep, fkeep = [], [], [], []
    for pts, keep in parts:
        faces.append((len(verts), len(verts) + 1, len(verts) + 2))
        verts += [(x, y, -2.0) for x, y in pts]
        vkeep += [keep] * 3
        fkeep.append(keep)
    base = len(verts)
    verts += [(-6 + 0.0625 * p, 2.0 + p % 2, -2.0) for p in range(102)]
    faces += [(base + i, base + i + 1, base + i + 2) for i in range(100)]
    vkeep += [True] * 102
    fkeep += [True] * 100
    verts, faces, vkeep, fkeep = np.array(verts, np.float32), np.array(faces, np.int64), np.array(vkeep), np.array(fkeep)
    if permute:
        verts, faces, vkeep, fkeep = _permuted(verts, faces, vkeep, fkeep, 62)
    if strays:
        at = [5, 60, len(verts)]                          # rows of the strays in the new numbering, ascending
        far = np.array([(1000, 0, -2), (0, -1000, -2), (0, 0, 1000)], np.float32)
        new_id = np.arange(len(verts)) + np.searchsorted(np.array(at) - np.arange(3), np.arange(len(verts)), side="right")
        v2 = np.zeros((len(verts) + 3, 3), np.float32)
        k2 = np.zeros(len(verts) + 3, bool)
        v2[new_id], k2[new_id] = verts, vkeep
        for row, p in zip(at, far):
            v2[row] = p
        verts, vkeep, faces = v2, k2, new_id[faces]
    return SimpleNamespace(verts=verts, faces=faces.astype(np.int32), min_faces=1, min_diag_frac=0.25, keep_v=vkeep, keep_f=fkeep)


def strip_case(shuffled, n=20000):
    """A strip of n triangles (i, i+1, i+2 along the strip), one component.  not shuffled: the vertex ids descend along the strip, so
    every hook puts a vertex under its successor and the forest is one chain of depth n.  shuffled: ids and face order permuted.
    The filter's defaults keep all of it, vertices and faces in input order: the output is the input."""
    V = n + 2
    p = np.arange(V)
    verts = np.stack([0.01 * p, p % 2, np.zeros(V)], 1).astype(np.float32)
    faces = np.stack([p[:-2], p[1:-1], p[2:]], 1)
    if shuffled:
        verts, faces, _, _ = _permuted(verts, faces, p, p[:-2], 63)
    else:
        verts, faces = verts[::-1].copy(), (V - 1 - faces)
    return SimpleNamespace(verts=verts, faces=faces.astype(np.int32), min_faces=64, min_diag_frac=0.2, keep_v=np.ones(V, bool), keep_f=np.ones(n, bool))


def single_triangle():
    verts = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float32)
    return SimpleNamespace(verts=verts, faces=np.array([(2, 0, 1)], np.int32), min_faces=1, min_diag_frac=0.2, keep_v=np.ones(3, bool),
                           keep_f=np.ones(1, bool))


SIZED_CASES = [(255, 255, 70), (256, 256, 71), (257, 257, 72), (255, 257, 73), (257, 255, 74), (256, 1, 75), (3, 256, 76),
               (5000, 40, 77), (40, 5000, 78)]      # (V, F, seed): both block edges, V >> F, F >> V


def sized_case(V, F, seed):
    """A mesh of exactly V vertices and F faces: the vertices in clumps of 3..12 (a clump's radius between 0.02 and 0.6, its centre
    in [-1, 1]^3), every face inside one clump, one face in twenty naming a vertex twice, ids permuted.  Clumps without a face are
    vertices no face uses.  min_faces = 4 and min_diag_frac = 0.15 cut through both criteria; what stays is the restatement's to say."""
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < V:
        sizes.append(min(int(rng.integers(3, 13)), V - sum(sizes)))
    start = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    sizes = np.array(sizes)
    clump = np.repeat(np.arange(len(sizes)), sizes)
    verts = (rng.uniform(-1, 1, (len(sizes), 3))[clump] + rng.uniform(0.02, 0.6, len(sizes))[clump, None] * rng.uniform(-1, 1, (V, 3)))
    can = np.flatnonzero(sizes >= 3)
    share = sizes[can] * rng.uniform(0.05, 1, len(can)) ** 3            # some clumps get a few faces only
    pick = rng.choice(can, F, p=share / share.sum())
    faces = np.stack([start[g] + rng.choice(sizes[g], 3, replace=False) for g in pick])
    twice = rng.uniform(size=F) < 0.05
    faces[twice, 1] = faces[twice, 0]
    where = rng.permutation(V)
    out = np.empty((V, 3), np.float32)
    out[where] = verts
    return SimpleNamespace(verts=out, faces=where[faces].astype(np.int32), min_faces=4, min_diag_frac=0.15, twice=int(twice.sum()))
