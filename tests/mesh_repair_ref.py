"""NumPy restatement of csrc/mesh_repair.hip (soar_amd/mesh.py: repair_manifold, manifold_report) and the fixtures of
tests/test_mesh_repair_cpu.py / test_mesh_repair_gpu.py.  Everything is generated in code.

The definition ("Repairing non-manifold edges and vertices"; MeshLab's two repair filters made order-free):
  1. a face that names a vertex outside [0, V) is refused; a face with two equal corners (a null face) is dropped;
  2. an undirected edge is (min, max) of two consecutive corners.  a2 of a face = (n.x n.x + n.y n.y) + n.z n.z with
     n = (b - a) x (c - a), every operation rounded to float32.  On an edge with k > 2 live faces the k - 2 faces that come first in
     ascending (a2's bits as uint32, face index) are marked; every marked face goes, in ONE pass;
  3. over the corners 3 f + c of the surviving faces: for every edge with exactly two surviving faces the two faces' corners at each
     end of the edge are joined, whatever the faces' directions.  A fan is a connected set of corners, its id its least corner.  Per
     vertex the fan of least id keeps the vertex; every other fan gets a copy at the same coordinates;
  4. output: the input vertices that a surviving face names, in input order, then the copies in ascending fan id; the surviving faces
     in their order and winding; source[v'] = the input vertex v' came from;
  5. the nine counts, COUNT_NAMES."""
import functools
from typing import NamedTuple

import numpy as np

import mesh_holes_ref as H
import mesh_simplify_ref as S
from mesh_attr_ref import disc, open_grid

COUNT_NAMES = ("vertices", "faces", "non_manifold_edges", "faces_removed", "null_faces", "vertex_copies", "unreferenced_vertices",
               "same_direction_edges", "border_edges")


class Repaired(NamedTuple):
    verts: np.ndarray        # [V',3] float32
    faces: np.ndarray        # [F',3] int32
    source: np.ndarray       # [V'] int32
    counts: tuple            # the nine counts, in COUNT_NAMES' order


class Fixture(NamedTuple):
    name: str
    verts: np.ndarray        # [V,3] float32
    faces: np.ndarray        # [F,3] int32


# ---- the restatement -----------------------------------------------------------------------------------------------------------

def area_bits(verts, faces):
    """[F] uint32: the bits of a2, float32 operation by operation (rows of `faces` must be in range)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
        nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
        ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
        nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
        a2 = (nx * nx + ny * ny) + nz * nz
    assert a2.dtype == np.float32
    return np.ascontiguousarray(a2).view(np.uint32)


def _edges(f, alive):
    """-> dict (lo, hi) -> [half-edges 3 f + c of the faces with alive[f], ascending]"""
    out = {}
    for i in np.nonzero(alive)[0].tolist():
        t = f[i].tolist()
        for c in range(3):
            a, b = t[c], t[(c + 1) % 3]
            out.setdefault((a, b) if a < b else (b, a), []).append(3 * i + c)
    return out


def repair(verts, faces) -> Repaired:
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    V, F = len(v), len(f)
    n_bad = int(((f < 0) | (f >= V)).any(1).sum())
    if n_bad:
        raise ValueError(f"{n_bad} faces name a vertex outside [0, {V})")
    # 1. null faces
    live = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2]) if F else np.zeros(0, bool)
    # 2. edges with more than two faces lose their smallest
    bits = area_bits(v, f).tolist() if F else []
    marked = np.zeros(F, bool)
    many = 0
    for hs in _edges(f, live).values():
        if len(hs) > 2:
            many += 1
            order = sorted((bits[h // 3], h // 3) for h in hs)
            for _, i in order[:len(hs) - 2]:
                marked[i] = True
    alive = live & ~marked
    # 3. fans: union-find over the corners, every set named by its least corner
    parent = list(range(3 * F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)

    nxt = lambda h: h - 2 if h % 3 == 2 else h + 1
    flat = f.reshape(-1).tolist()
    same = border = 0
    for hs in _edges(f, alive).values():
        assert len(hs) <= 2                                   # one pass is enough
        if len(hs) == 1:
            border += 1
            continue
        h0, h1 = hs
        if flat[h0] == flat[h1]:                              # both run from the same end: inconsistent winding, joined all the same
            same += 1
            union(h0, h1)
            union(nxt(h0), nxt(h1))
        else:
            union(h0, nxt(h1))
            union(nxt(h0), h1)
    corners = [h for i in np.nonzero(alive)[0].tolist() for h in (3 * i, 3 * i + 1, 3 * i + 2)]
    fan = {h: find(h) for h in corners}
    least = {}
    for h in corners:
        least[flat[h]] = min(least.get(flat[h], fan[h]), fan[h])
    # 4. output
    kept = sorted(least)
    new_id = {old: k for k, old in enumerate(kept)}
    copies = sorted({r for h, r in fan.items() if r != least[flat[h]]})
    copy_id = {r: len(kept) + k for k, r in enumerate(copies)}
    source = np.array(kept + [flat[r] for r in copies], np.int32).reshape(-1)
    fo = np.array([[new_id[flat[h]] if fan[h] == least[flat[h]] else copy_id[fan[h]] for h in (3 * i, 3 * i + 1, 3 * i + 2)]
                   for i in np.nonzero(alive)[0].tolist()], np.int32).reshape(-1, 3)
    vo = v[source]
    n_null = int(F - live.sum())
    counts = (len(vo), len(fo), many, int(marked.sum()), n_null, len(copies), V - len(kept), same, border)
    return Repaired(vo, fo, source, counts)


def non_manifold_edges(faces):
    """edges with more than two faces, over the faces without a repeated corner"""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    live = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return sum(1 for hs in _edges(f, live).values() if len(hs) > 2)


# ---- fixtures --------------------------------------------------------------------------------------------------------------------

def _fx(name, v, f):
    return Fixture(name, np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3), np.ascontiguousarray(f, dtype=np.int32).reshape(-1, 3))


def pages(apexes):
    """faces (0, 1, 2 + i) on the edge 0 -> 1 = (0,0,0) -> (1,0,0), one per apex; the directions alternate"""
    v = [[0, 0, 0], [1, 0, 0]] + [list(a) for a in apexes]
    f = [[0, 1, 2 + i] if i % 2 == 0 else [1, 0, 2 + i] for i in range(len(apexes))]
    return v, f


def pages70():
    """70 pages on one edge, heights in a scrambled order with six ties: a run wider than a wavefront"""
    k = np.arange(70)
    ang = 2.0 * np.pi * k / 70.0
    height = 0.25 + ((k * 37) % 64) / 16.0                    # 64 distinct values: 6 of the 70 repeat an earlier one
    return pages(np.stack([np.full(70, 0.5), height * np.cos(ang), height * np.sin(ang)], 1))


def tetrahedron(ids, pts):
    """an outward-facing tetrahedron over four vertex ids with positions pts (positively oriented: det(p1-p0, p2-p0, p3-p0) > 0)"""
    a, b, c, d = ids
    p = np.asarray(pts, np.float64)
    assert np.linalg.det(np.stack([p[1] - p[0], p[2] - p[0], p[3] - p[0]])) > 0
    return [[a, c, b], [a, b, d], [b, c, d], [c, a, d]]


def two_tetrahedra_on_an_edge():
    """vertices 0, 1 are the shared edge (k = 4 there); the second tetrahedron is smaller, so both of its faces at the edge go"""
    v = [[0, 0, 0], [0, 0, 1], [1, 0.2, 0.5], [0.3, 1, 0.5], [-0.5, -0.1, 0.5], [-0.2, -0.6, 0.5]]
    f = tetrahedron((0, 1, 2, 3), [v[0], v[1], v[2], v[3]]) + tetrahedron((0, 1, 4, 5), [v[0], v[1], v[4], v[5]])
    return v, f


def marked_twice():
    """face 0 = (0, 1, 2) is the smallest on its edges 0-1 and 1-2, each of which has two larger pages besides"""
    v = [[0, 0, 0], [1, 0, 0], [1, 0.5, 0], [0.5, 0, 2], [0.5, 0, -2], [1, 0.25, 2], [1, 0.25, -2]]
    f = [[0, 1, 2], [0, 1, 3], [1, 0, 4], [1, 2, 5], [2, 1, 6]]
    return v, f


def lone_apex_first():
    """the smallest of three pages on the edge 1-2 has vertex 0 for its apex, and nothing else names vertex 0: it is dropped and
    every id shifts"""
    v = [[0.5, 0.1, 0], [0, 0, 0], [1, 0, 0], [0.5, 0, 1.5], [0.5, -2, 0]]
    f = [[1, 2, 3], [2, 1, 0], [1, 2, 4]]
    return v, f


def two_tetrahedra_on_a_vertex():
    v = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]
    f = tetrahedron((0, 1, 2, 3), [v[0], v[1], v[2], v[3]]) + tetrahedron((0, 5, 4, 6), [v[0], v[5], v[4], v[6]])
    return v, f


def three_fans():
    """vertex 3 (not the first) carries a closed fan (a tetrahedron), an open fan of two faces and a lone triangle, in an order in
    which the fan of least id is not the first face's alone"""
    v = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0], [-1, 0, 0], [-1, -1, 0], [0, -1, 0], [0, 0, -1], [0.5, 0, -1]]
    f = [[4, 5, 3]] + tetrahedron((3, 0, 1, 2), [v[3], v[0], v[1], v[2]]) + [[3, 5, 6], [7, 8, 3]]
    return v, f


def lone_triangles(n=70):
    """n lone triangles around vertex 0, which stands at another corner in each: n - 1 copies, ordered by fan id"""
    ang = 2.0 * np.pi * np.arange(2 * n) / (2 * n)
    v = [[0, 0, 0]] + np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], 1).tolist()
    f = []
    for i in range(n):
        t = [0, 1 + 2 * i, 2 + 2 * i]
        f.append(t[-(i % 3):] + t[:-(i % 3)] if i % 3 else t)
    return v, f


def two_half_discs():
    """two open fans of three faces each at vertex 0, on opposite sides"""
    v = [[0, 0, 0], [1, 0, 0], [0.7, 0.7, 0], [0, 1, 0], [-0.7, 0.7, 0.1], [-1, 0, 0], [-0.7, -0.7, 0], [0, -1, 0], [0.7, -0.7, 0.1]]
    f = [[0, 1, 2], [0, 5, 6], [0, 2, 3], [0, 6, 7], [0, 3, 4], [0, 7, 8]]
    return v, f


def with_null_faces():
    """the 5 x 5 grid with three faces that name a vertex twice in between, one of them naming one vertex three times; vertex 25 is
    named by null faces alone"""
    v, f = open_grid(5)
    v = np.concatenate([v, [[2.0, 2.0, 2.0]]])
    f = f.tolist()
    f = f[:3] + [[7, 7, 8]] + f[3:10] + [[25, 3, 25]] + f[10:] + [[4, 4, 4]]
    return v, f


@functools.lru_cache(maxsize=None)
def two_sheets(level, inner, R):
    """two nested icospheres of scale 1 and `inner`, clustered at cell_for(v, R) by the restatement of simplify: where both sheets
    pass through one cell the result has edges with more than two faces"""
    v0, f0 = S.icosphere(level, scale=1.0)
    v1, f1 = S.icosphere(level, scale=inner)
    v, f = np.concatenate([v0, v1]), np.concatenate([f0, f1 + len(v0)])
    return v, f, S.cell_for(v, R)


@functools.lru_cache(maxsize=None)
def clustered_two_sheets():
    v, f, cell = two_sheets(3, 0.9, 7)
    r = S.simplify(v, f, cell)
    return r.vertices, r.faces


@functools.lru_cache(maxsize=None)
def fixtures():
    out = [_fx("pages3_distinct", *pages([[0.5, 2, 0], [0.5, -0.5, 0.1], [0.5, 0, 1]]))]
    # faces 1 and 2 have the same a2 (mirror images), the least: face 1 goes
    out.append(_fx("pages3_tie", *pages([[0.5, 0, 2], [0.5, 1, 0], [0.5, -1, 0]])))
    out.append(_fx("pages5", *pages([[0.5, 1, 0], [0.5, 0, 3], [0.5, -0.25, 0], [0.5, 0, -0.5], [0.5, 2, 2]])))
    out.append(_fx("pages70", *pages70()))
    out.append(_fx("tetrahedra_on_an_edge", *two_tetrahedra_on_an_edge()))
    out.append(_fx("marked_twice", *marked_twice()))
    out.append(_fx("lone_apex_first", *lone_apex_first()))
    out.append(_fx("tetrahedra_on_a_vertex", *two_tetrahedra_on_a_vertex()))
    out.append(_fx("three_fans", *three_fans()))
    out.append(_fx("lone_triangles70", *lone_triangles(70)))
    out.append(_fx("two_half_discs", *two_half_discs()))
    out.append(_fx("same_direction", H.fixture("g_same_way").verts, H.fixture("g_same_way").faces))
    out.append(_fx("null_faces", *with_null_faces()))
    out.append(_fx("no_faces", [[0.1, -0.2, 0.3], [0.5, 0.5, 0.5]], np.zeros((0, 3))))
    out.append(_fx("grid9_touching_holes", H.fixture("d_grid9").verts, H.fixture("d_grid9").faces))
    out.append(_fx("clustered_two_sheets", *clustered_two_sheets()))
    out += list(manifold_fixtures())
    return tuple(out)


@functools.lru_cache(maxsize=None)
def manifold_fixtures():
    """inputs that need nothing: they come back with equal bits"""
    v, f = S.icosphere(2)
    return _fx("icosphere2", v, f), _strip(), _fx("tube12_13", *H.tube(12, 13)), _fx("disc7", *disc(7, 5))


def _strip():
    """an open strip of 16 triangles between two rows of 9 vertices, every vertex named"""
    n = 9
    v = [[k / (n - 1), 0.0, 0.1 * (k % 2)] for k in range(n)] + [[k / (n - 1), 0.3, 0.0] for k in range(n)]
    f = []
    for k in range(n - 1):
        f += [[k, k + 1, n + k], [k + 1, n + k + 1, n + k]]
    return _fx("open_strip", v, f)


def fixture(name):
    return next(fx for fx in fixtures() if fx.name == name)


@functools.lru_cache(maxsize=None)
def wanted(name) -> Repaired:
    """the restatement's result for a fixture, computed once and shared (treat as read-only)"""
    fx = fixture(name)
    r = repair(fx.verts, fx.faces)
    for a in r[:3]:
        a.setflags(write=False)
    return r
