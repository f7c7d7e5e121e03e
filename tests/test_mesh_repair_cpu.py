"""CPU tests of the repair of non-manifold edges and vertices: the NumPy restatement tests/mesh_repair_ref.py and its fixtures, held
to the definition ("Repairing non-manifold edges and vertices") by a brute-force check that shares no code with it,
and what soar_mesh_repair_workspace_size / _count / soar_mesh_repair refuse before any launch.  No kernel runs here."""
import ctypes as C

import numpy as np
import pytest

import mesh_holes_ref as H
import mesh_repair_ref as R

FIXTURES = R.fixtures()


# ---- a check written apart from the restatement: dictionaries over edges, a flood fill per vertex --------------------------------

def faces_per_edge(faces):
    n = {}
    for t in np.asarray(faces).reshape(-1, 3).tolist():
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            n[frozenset((a, b))] = n.get(frozenset((a, b)), 0) + 1
    return n


def fans_per_vertex(V, faces):
    """[V] the number of groups the faces at a vertex fall into when two of them hang together through an edge at that vertex"""
    f = np.asarray(faces).reshape(-1, 3).tolist()
    at = [[] for _ in range(V)]
    for i, t in enumerate(f):
        for a in set(t):
            at[a].append(i)
    out = []
    for v in range(V):
        todo, groups = set(at[v]), 0
        while todo:
            groups += 1
            stack = [todo.pop()]
            while stack:
                i = stack.pop()
                for j in [j for j in todo if len((set(f[i]) & set(f[j])) - {v}) >= 1]:
                    todo.discard(j)
                    stack.append(j)
        out.append(groups)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f.name)
def test_the_restatement_gives_a_manifold_and_is_idempotent(fx):
    r = R.wanted(fx.name)
    V, F = len(r.verts), len(r.faces)
    assert r.verts.dtype == np.float32 and r.faces.dtype == np.int32 and r.source.dtype == np.int32
    assert r.counts[:2] == (V, F) and r.source.shape == (V,)
    if F:
        assert r.faces.min() >= 0 and r.faces.max() < V
        assert (r.faces[:, 0] != r.faces[:, 1]).all() and (r.faces[:, 1] != r.faces[:, 2]).all() and (r.faces[:, 0] != r.faces[:, 2]).all()
    per_edge = faces_per_edge(r.faces)
    assert max(per_edge.values(), default=0) <= 2
    assert fans_per_vertex(V, r.faces) == [1] * V              # one fan each, and no vertex without a face
    assert sum(1 for n in per_edge.values() if n == 1) == r.counts[8]
    # source maps coordinates bit for bit, and every surviving face is an input face in the input's order
    assert np.array_equal(bits(r.verts), bits(fx.verts[r.source]))
    back = r.source[r.faces] if F else np.zeros((0, 3), np.int32)
    rows = [t for t in fx.faces.tolist() if len(set(t)) == 3]
    it = iter(rows)
    assert all(any(t == u for u in it) for t in back.tolist())                    # a subsequence of the input's faces
    assert len(rows) - F == r.counts[3] and len(fx.faces) - len(rows) == r.counts[4]
    assert r.counts[5] == V - len(np.unique(r.source)) and r.counts[6] == len(fx.verts) - len(np.unique(r.source))
    # a second application is the identity
    again = R.repair(r.verts, r.faces)
    assert np.array_equal(again.faces, r.faces) and np.array_equal(bits(again.verts), bits(r.verts))
    assert np.array_equal(again.source, np.arange(V, dtype=np.int32))
    assert again.counts == (V, F, 0, 0, 0, 0, 0, r.counts[7], r.counts[8])


def test_what_every_small_fixture_must_give():
    """worked out by hand from the definition"""
    c = lambda name: dict(zip(R.COUNT_NAMES, R.wanted(name).counts))
    # a2 = 4, 0.26, 1 for the three pages: the second goes, its apex with it
    r = R.wanted("pages3_distinct")
    assert r.faces.tolist() == [[0, 1, 2], [0, 1, 3]] and r.source.tolist() == [0, 1, 2, 4]
    assert c("pages3_distinct") == dict(vertices=4, faces=2, non_manifold_edges=1, faces_removed=1, null_faces=0, vertex_copies=0,
                                        unreferenced_vertices=1, same_direction_edges=1, border_edges=4)
    # faces 1 and 2 tie at a2 = 1 below face 0's 4: the lower index goes
    fx = R.fixture("pages3_tie")
    assert R.area_bits(fx.verts, fx.faces).tolist() == bits([4.0, 1.0, 1.0]).tolist()
    assert R.wanted("pages3_tie").faces.tolist() == [[0, 1, 2], [0, 1, 3]] and R.wanted("pages3_tie").source.tolist() == [0, 1, 2, 4]
    assert c("pages3_tie")["same_direction_edges"] == 1
    # a2 = 1, 9, 1/16, 1/4, 8: the faces 0, 2, 3 go
    assert R.wanted("pages5").source.tolist() == [0, 1, 3, 6] and c("pages5")["faces_removed"] == 3
    assert c("pages5")["same_direction_edges"] == 0
    # 70 pages: the two largest stay, and they are the two of height 0.25 + 63 / 16
    fx = R.fixture("pages70")
    a = R.area_bits(fx.verts, fx.faces)
    order = sorted(range(70), key=lambda i: (int(a[i]), i))
    assert len(set(a.tolist())) < 70                           # there are ties in the run
    assert sorted(R.wanted("pages70").source.tolist()) == sorted([0, 1] + [2 + i for i in order[-2:]])
    assert c("pages70") == dict(vertices=4, faces=2, non_manifold_edges=1, faces_removed=68, null_faces=0, vertex_copies=0,
                                unreferenced_vertices=68, same_direction_edges=c("pages70")["same_direction_edges"], border_edges=4)
    # two tetrahedra on an edge: the smaller one loses its two faces there; its other two hang together at 4-5 alone, so at the
    # vertices 0 and 1 they are fans of their own
    assert c("tetrahedra_on_an_edge") == dict(vertices=8, faces=6, non_manifold_edges=1, faces_removed=2, null_faces=0, vertex_copies=2,
                                              unreferenced_vertices=0, same_direction_edges=0, border_edges=4)
    # (its faces 6 = (1, 4, 5) and 7 = (4, 0, 5) are left: the fan at vertex 1 is corner 18, the one at vertex 0 corner 22)
    assert R.wanted("tetrahedra_on_an_edge").source.tolist() == [0, 1, 2, 3, 4, 5, 1, 0]
    assert R.wanted("tetrahedra_on_an_edge").faces[4:].tolist() == [[6, 4, 5], [4, 7, 5]]
    # one face, marked by two edges, goes once
    assert c("marked_twice")["faces_removed"] == 1 and c("marked_twice")["non_manifold_edges"] == 2
    # (without it the pages on 0-1 and those on 1-2 are two fans at vertex 1: the second, from face 3's corner 9, gets the copy)
    assert R.wanted("marked_twice").source.tolist() == [0, 1, 2, 3, 4, 5, 6, 1]
    assert R.wanted("marked_twice").faces.tolist() == [[0, 1, 3], [1, 0, 4], [7, 2, 5], [2, 7, 6]]
    # vertex 0 goes with its face: every id shifts by one
    assert R.wanted("lone_apex_first").source.tolist() == [1, 2, 3, 4] and R.wanted("lone_apex_first").faces.tolist() == [[0, 1, 2], [0, 1, 3]]
    assert c("tetrahedra_on_a_vertex") == dict(vertices=8, faces=8, non_manifold_edges=0, faces_removed=0, null_faces=0, vertex_copies=1,
                                               unreferenced_vertices=0, same_direction_edges=0, border_edges=0)
    assert H.is_closed_and_oriented(R.wanted("tetrahedra_on_a_vertex").faces)
    assert R.wanted("tetrahedra_on_a_vertex").faces[4:].max() == 7 and R.wanted("tetrahedra_on_a_vertex").faces[:4].max() == 3
    # three fans at vertex 3: the lone first face keeps it (corner 2), the tetrahedron (corner 3) and the last face get copies; the
    # face (3, 5, 6) hangs on to the first through the edge 3-5
    r = R.wanted("three_fans")
    assert c("three_fans")["vertex_copies"] == 2 and r.source.tolist() == list(range(9)) + [3, 3]
    assert r.faces[0].tolist() == [4, 5, 3] and r.faces[5].tolist() == [3, 5, 6] and r.faces[6].tolist() == [7, 8, 10]
    assert sorted(set(r.faces[1:5].reshape(-1).tolist())) == [0, 1, 2, 9]
    # 70 lone triangles: the first keeps vertex 0, the others get the copies 141 .. 209 in face order
    r = R.wanted("lone_triangles70")
    assert c("lone_triangles70")["vertex_copies"] == 69 and r.source.tolist() == list(range(141)) + [0] * 69
    assert [int(t[t >= 141][0]) for t in r.faces[1:]] == list(range(141, 210)) and (r.faces[0] < 141).all()
    assert c("two_half_discs")["vertex_copies"] == 1 and R.wanted("two_half_discs").faces[:, 0].tolist() == [0, 9, 0, 9, 0, 9]
    # counted, unchanged
    fx = R.fixture("same_direction")
    assert c("same_direction") == dict(vertices=4, faces=2, non_manifold_edges=0, faces_removed=0, null_faces=0, vertex_copies=0,
                                       unreferenced_vertices=0, same_direction_edges=1, border_edges=4)
    assert np.array_equal(R.wanted("same_direction").faces, fx.faces)
    assert c("null_faces")["null_faces"] == 3 and c("null_faces")["unreferenced_vertices"] == 1 and c("null_faces")["faces"] == 32
    assert R.wanted("no_faces").counts == (0, 0, 0, 0, 0, 0, 2, 0, 0)


@pytest.mark.parametrize("fx", R.manifold_fixtures(), ids=lambda f: f.name)
def test_a_manifold_comes_back_with_equal_bits(fx):
    r = R.wanted(fx.name)
    assert np.array_equal(r.faces, fx.faces) and np.array_equal(bits(r.verts), bits(fx.verts))
    assert np.array_equal(r.source, np.arange(len(fx.verts), dtype=np.int32))
    assert r.counts[2:7] == (0, 0, 0, 0, 0)


def test_a_face_outside_the_mesh_is_refused():
    fx = R.fixture("pages5")
    bad = fx.faces.copy()
    bad[2, 1] = len(fx.verts)
    with pytest.raises(ValueError, match="1 faces name a vertex outside"):
        R.repair(fx.verts, bad)
    bad[3, 0] = -1
    with pytest.raises(ValueError, match="2 faces name a vertex outside"):
        R.repair(fx.verts, bad)


def test_the_clustered_two_sheets_lose_their_non_manifold_edges():
    """two nested icosphere(3) of scale 1.0 / 0.9, clustered at cell_for(v, 7): 218 vertices, 600 faces and 192 edges with more than
    two faces when this was written"""
    fx = R.fixture("clustered_two_sheets")
    before = R.non_manifold_edges(fx.faces)
    r = R.wanted(fx.name)
    print(f"clustered two sheets: {len(fx.verts)} vertices, {len(fx.faces)} faces, {before} edges with more than two faces; "
          f"repaired: {dict(zip(R.COUNT_NAMES, r.counts))}")
    assert before > 0 and before == r.counts[2] == sum(1 for n in faces_per_edge(fx.faces).values() if n > 2)
    assert R.non_manifold_edges(r.faces) == 0 and max(faces_per_edge(r.faces).values()) <= 2
    assert (len(fx.verts), len(fx.faces), before) == (218, 600, 192)


def test_touching_holes_close_once_their_vertex_is_split():
    fx = H.fixture("d_grid9_touching_holes")
    assert H.close_holes(fx.verts, fx.faces, 300).open_left == 6
    r = R.repair(fx.verts, fx.faces)
    assert r.counts[5] == 1 and r.source.tolist() == list(range(81)) + [40] and len(r.faces) == len(fx.faces)
    closed = H.close_holes(r.verts, r.faces, 300)
    assert closed.open_left == 0 and 6 in closed.closed.tolist()
    assert H.is_closed_and_oriented(closed.faces)


# ---- the C calls, before any launch ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


P = 0x7f0000000000                                             # a fake, 256-byte aligned address: nothing reads it before the checks fail
V_, F_ = 81, 126


def _calls(L, need):
    cnt = (C.c_int64 * 9)(*([-5] * 9))
    count = lambda **kw: L.soar_mesh_repair_count(*[kw.get(k, d) for k, d in (
        ("V", V_), ("F", F_), ("verts", P), ("faces", P), ("ws", P), ("nb", need), ("counts", cnt), ("st", None))])
    run = lambda **kw: L.soar_mesh_repair(*[kw.get(k, d) for k, d in (
        ("V", V_), ("F", F_), ("verts", P), ("faces", P), ("ws", P), ("nb", need), ("vo", 2 * P), ("fo", 3 * P), ("src", 4 * P), ("counts", cnt),
        ("st", None))])
    return count, run, cnt


def test_the_workspace_is_checked_before_any_launch(lib):
    from soar_amd import hip_lib
    n = C.c_size_t(0)
    assert lib.soar_mesh_repair_workspace_size(V_, F_, C.byref(n)) == 0 and n.value % 256 == 0
    need = n.value
    # two sorts' keys and values, parents, flags and scans over the 3 F corners
    assert need >= 3 * F_ * (5 * 4 + 2 * 8 + 4 + 2 * 4) + 4 * V_ * 3
    count, run, cnt = _calls(lib, need)

    def refused(rc, *words):
        assert rc != 0 and all(w in hip_lib.last_error() for w in words), (rc, hip_lib.last_error())

    for name, call in (("soar_mesh_repair_count", count), ("soar_mesh_repair", run)):
        refused(call(ws=None), name + ": NULL workspace or workspace not 256-byte aligned")
        refused(call(ws=P + 128), name + ": NULL workspace or workspace not 256-byte aligned")
        refused(call(nb=need - 1), f"{name}: workspace of {need - 1} bytes, need {need} (soar_mesh_repair_workspace_size)")
        refused(call(nb=0), f"need {need}")
        refused(call(verts=None), "NULL argument")
        refused(call(faces=None), "NULL argument")
        refused(call(counts=None), "NULL argument")
        refused(call(V=0), "V=0")
        refused(call(F=-1), "F=-1")
        refused(call(V=(1 << 30) + 1), "2^30")
        refused(call(F=(1 << 28) + 1), "2^28")
    refused(run(vo=None), "NULL argument")
    refused(run(fo=None), "NULL argument")
    refused(run(src=None), "NULL argument")
    refused(run(vo=P), "must not be the inputs")
    refused(run(fo=P), "must not be the inputs")
    assert list(cnt) == [-5] * 9


def test_the_sizing_call(lib):
    from soar_amd import hip_lib
    n, m = C.c_size_t(0), C.c_size_t(0)
    assert lib.soar_mesh_repair_workspace_size(10242, 20480, C.byref(n)) == 0
    assert lib.soar_mesh_repair_workspace_size(10242, 40960, C.byref(m)) == 0 and m.value > n.value
    assert lib.soar_mesh_repair_workspace_size(2, 0, C.byref(n)) == 0 and n.value % 256 == 0 and n.value > 0
    assert lib.soar_mesh_repair_workspace_size(1 << 30, 1 << 28, C.byref(n)) == 0 and n.value > (3 << 28) * 48
    for V, F in ((0, 4), (4, -1), ((1 << 30) + 1, 4), (4, (1 << 28) + 1)):
        assert lib.soar_mesh_repair_workspace_size(V, F, C.byref(n)) != 0 and f"V={V}" in hip_lib.last_error()
    assert lib.soar_mesh_repair_workspace_size(4, 4, None) != 0 and "NULL" in hip_lib.last_error()
    # F = 0: nothing is launched, the counts say that no vertex is named
    need = C.c_size_t(0)
    assert lib.soar_mesh_repair_workspace_size(5, 0, C.byref(need)) == 0
    cnt = (C.c_int64 * 9)(*([-5] * 9))
    assert lib.soar_mesh_repair_count(5, 0, P, None, P, need.value, cnt, None) == 0 and list(cnt) == [0, 0, 0, 0, 0, 0, 5, 0, 0]
    cnt = (C.c_int64 * 9)(*([-5] * 9))
    assert lib.soar_mesh_repair(5, 0, P, None, P, need.value, None, None, None, cnt, None) == 0 and list(cnt) == [0, 0, 0, 0, 0, 0, 5, 0, 0]


def test_python_refuses_cpu_tensors_and_wrong_types():
    import torch
    from soar_amd import mesh
    m = mesh.Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    for call in (mesh.repair_manifold, mesh.manifold_report):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(m)
    assert mesh.REPAIR_COUNTS == R.COUNT_NAMES
