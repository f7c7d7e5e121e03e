"""CPU tests of the yardstick of the hole closing (tests/mesh_holes_ref.py: the restatement test_mesh_holes_gpu.py compares
csrc/mesh_holes.hip with), of its fixtures and of the interface of soar_amd/mesh.py.  No kernel runs here."""
import numpy as np
import pytest
import torch

import mesh_holes_ref as H

FIXTURES = H.fixtures()


def _loop_lengths(fx):
    rings, n_border = H.loops(fx.faces)
    return sorted(len(r) for r in rings), n_border


def test_the_fixtures_are_what_they_claim():
    by = {fx.name[0]: fx for fx in FIXTURES}
    assert sorted(by) == list("abcdefghi")
    for fx in FIXTURES:
        assert fx.verts.dtype == np.float32 and fx.faces.dtype == np.int32 and fx.faces.shape[1:] == (3,)
        if len(fx.faces):
            assert 0 <= fx.faces.min() and fx.faces.max() < len(fx.verts)
            assert (fx.faces[:, 0] != fx.faces[:, 1]).all() and (fx.faces[:, 1] != fx.faces[:, 2]).all() and (fx.faces[:, 0] != fx.faces[:, 2]).all()
    # (a) 162 / 320 less two vertices and 6 + 5 + 1 + 2 faces; the four groups of removed faces share no vertex
    v, f, groups = H.punched_icosphere2()
    full = H.icosphere(2)[1]
    assert len(v) == 160 and len(f) == 320 - 14 and [len(g) for g in groups] == [6, 5, 1, 2]
    sets = [set(full[g].reshape(-1).tolist()) for g in groups]
    assert all(not (sets[i] & sets[j]) for i in range(4) for j in range(i))
    assert _loop_lengths(by["a"]) == ([3, 4, 5, 6], 18)
    # (b) the rim of the 9 x 9 grid
    assert by["b"].verts.shape == (81, 3) and by["b"].faces.shape == (128, 3) and _loop_lengths(by["b"]) == ([32], 32)
    # (c) the tube's two ends
    assert by["c"].verts.shape == (601, 3) and by["c"].faces.shape == (601, 3) and _loop_lengths(by["c"]) == ([300, 301], 601)
    assert all(sorted(u) == [-1, 1] for u in H.edge_uses(by["c"].faces).values() if len(u) != 1)
    # (d) the two holes meet in vertex 40, which two border half-edges leave and two reach: only the rim is a loop
    assert by["d"].faces.shape == (126, 3) and _loop_lengths(by["d"]) == ([32], 38)
    ids, frm, to = H.border_half_edges(by["d"].faces)
    assert sum(frm[h] == 40 for h in ids) == 2 and sum(to[h] == 40 for h in ids) == 2
    # (e) an edge of three faces; (f) one face; (g) two faces that both run 0 -> 1
    assert max(len(u) for u in H.edge_uses(by["e"].faces).values()) == 3 and _loop_lengths(by["e"]) == ([], 6)
    assert _loop_lengths(by["f"]) == ([3], 3)
    assert H.edge_uses(by["g"].faces)[(0, 1)] == [1, 1] and _loop_lengths(by["g"]) == ([], 4)
    # (h) more loops than a workgroup has lanes, each the ring of one vertex
    v, f, removed = H.punched_icosphere5()
    lengths, n_border = _loop_lengths(by["h"])
    print(f"(h): {removed} vertices removed, {len(v)} / {len(f)} left, loops of 5: {lengths.count(5)}, of 6: {lengths.count(6)}")
    assert len(v) == 10242 - removed and removed > 256 and len(lengths) == removed > 256 and set(lengths) <= {5, 6}
    assert len(f) == 20480 - n_border and n_border == sum(lengths)
    # (i) no face at all
    assert by["i"].faces.shape == (0, 3) and len(by["i"].verts) == 2


def test_the_restatement_leaves_what_it_must_not_close():
    for prefix in "def":
        fx = H.fixture(prefix)
        # (d): below its rim's 32 edges nothing may change; (e), (f): nothing at any limit
        for limit in ((3, 31) if prefix == "d" else (3, 31, 32, 300, 65535)):
            got = H.close_holes(fx.verts, fx.faces, limit)
            assert np.array_equal(got.verts, fx.verts) and np.array_equal(got.faces, fx.faces) and len(got.closed) == 0, (fx.name, limit)
            assert got.open_left == H.loops(fx.faces)[1]
    # (d) at the default: the rim is a loop like any other and is capped; the two touching holes stay open, all six edges of them
    fx = H.fixture("d")
    got = H.close_holes(fx.verts, fx.faces)
    assert got.closed.tolist() == [32] and got.open_left == 6
    assert np.array_equal(got.verts[:81], fx.verts) and np.array_equal(got.faces[:126], fx.faces)
    left = sorted(e for e, u in H.edge_uses(got.faces).items() if len(u) == 1)
    assert left == [(30, 39), (30, 40), (39, 40), (40, 49), (40, 50), (49, 50)]
    fx = H.fixture("g")
    got = H.close_holes(fx.verts, fx.faces)
    assert np.array_equal(got.faces, fx.faces) and got.open_left == 4
    fx = H.fixture("i")
    got = H.close_holes(fx.verts, fx.faces)
    assert np.array_equal(got.verts, fx.verts) and got.faces.shape == (0, 3) and got.open_left == 0 and len(got.closed) == 0


@pytest.mark.parametrize("prefix", ["a", "h"])
def test_closing_makes_a_sphere(prefix):
    fx = H.fixture(prefix)
    assert not H.is_closed_and_oriented(fx.faces)
    got = H.wanted(fx.name, H.MAX_HOLE_EDGES)
    V, F = len(fx.verts), len(fx.faces)
    assert np.array_equal(got.verts[:V], fx.verts) and np.array_equal(got.faces[:F], fx.faces)
    assert got.open_left == 0 and H.is_closed_and_oriented(got.faces) and H.euler(got.faces) == 2
    assert len(np.unique(got.faces)) == len(got.verts)
    n4 = got.closed[got.closed >= 4]
    assert len(got.verts) == V + len(n4) and len(got.faces) == F + int(n4.sum()) + int((got.closed == 3).sum())


def test_the_limit_is_inclusive():
    b = H.fixture("b")
    assert H.close_holes(b.verts, b.faces, 32).closed.tolist() == [32]
    assert H.close_holes(b.verts, b.faces, 31).closed.tolist() == []
    c = H.fixture("c")
    got = H.close_holes(c.verts, c.faces, 300)
    assert got.closed.tolist() == [300] and got.open_left == 301
    assert len(got.verts) == 602 and len(got.faces) == 901
    # the ring of 300 is the one at y = 0: its cap's vertex lies there, and every new face has it
    assert got.verts[601, 1] == 0.0 and (got.faces[601:, 2] == 601).all() and got.faces[601:, :2].max() < 300
    assert H.close_holes(c.verts, c.faces, 301).closed.tolist() == [301, 300]       # the strip's first face lies on the ring of 301
    assert H.close_holes(c.verts, c.faces, 299).closed.tolist() == []


def test_the_patches_of_the_punched_sphere():
    """order, shape and orientation of what (a) gains: loops by ascending leader, a triangle for the loop of 3 and a fan for the
    others, every new face turned outward like the sphere's own"""
    fx = H.fixture("a")
    got = H.wanted(fx.name, H.MAX_HOLE_EDGES)
    rings, _ = H.loops(fx.faces)
    assert [r[0] for r in rings] == sorted(r[0] for r in rings) and got.closed.tolist() == [len(r) for r in rings]
    assert sorted(got.closed.tolist()) == [3, 4, 5, 6]
    V, F = len(fx.verts), len(fx.faces)
    assert len(got.verts) == V + 3 and len(got.faces) == F + 1 + 4 + 5 + 6
    p = got.verts.astype(np.float64)[got.faces]
    normal = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert ((normal * p.mean(1)).sum(1) > 0).all()
    # a fan's vertex is the float64 mean of its ring, rounded once
    at, c = F, V
    for ring, n in zip(rings, got.closed.tolist()):
        if n == 3:
            at += 1
            continue
        fan = got.faces[at:at + n]
        assert (fan[:, 2] == c).all() and sorted(fan[:, 0].tolist()) == sorted(fan[:, 1].tolist())
        mean = fx.verts[fan[:, 0]].astype(np.float64).mean(0)
        assert np.abs(got.verts[c].astype(np.float64) - mean).max() <= 2.0 ** -24
        at, c = at + n, c + 1
    # with the limit at 4 only the loops of 3 and 4 close
    assert sorted(H.close_holes(fx.verts, fx.faces, 4).closed.tolist()) == [3, 4]


def test_interface():
    from soar_amd import hip_lib, mesh
    assert mesh.MAX_HOLE_EDGES == 300 == H.MAX_HOLE_EDGES
    fx = H.fixture("b")
    m = mesh.Mesh(torch.from_numpy(fx.verts), torch.from_numpy(fx.faces))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.close_holes(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.open_border_edges(m)
    import inspect
    assert inspect.signature(mesh.close_holes).parameters["max_hole_edges"].default == 300
    assert inspect.signature(mesh.export_avatar).parameters["max_hole_edges"].default is None
    for name in ("soar_mesh_close_holes_bytes", "soar_mesh_close_holes"):
        assert name in hip_lib.SIGNATURES


@pytest.mark.parametrize("bad", [2, 70000, 0, -1])
def test_bad_limits_are_refused(bad):
    """the limit is judged first, before the tensors are looked at"""
    from soar_amd import mesh
    fx = H.fixture("b")
    with pytest.raises(ValueError, match="max_hole_edges"):
        mesh.close_holes(mesh.Mesh(torch.from_numpy(fx.verts), torch.from_numpy(fx.faces)), bad)


def test_the_sizing_call_and_the_checks_before_any_launch():
    import ctypes as C

    from soar_amd import build, hip_lib
    build.build()
    L = hip_lib.lib()
    n = C.c_size_t(0)
    assert L.soar_mesh_close_holes_bytes(10242, 20480, C.byref(n)) == 0
    assert n.value % 256 == 0 and n.value >= 3 * 20480 * (2 * 8 + 11 * 4 + 1) + 10242 * 12
    assert L.soar_mesh_close_holes_bytes(2, 0, C.byref(n)) == 0 and n.value % 256 == 0 and n.value > 0
    for V, F in ((0, 4), (1, -1), ((1 << 30) + 1, 4), (4, (1 << 28) + 1)):
        assert L.soar_mesh_close_holes_bytes(V, F, C.byref(n)) != 0 and f"V={V}" in hip_lib.last_error()
    assert L.soar_mesh_close_holes_bytes(4, 4, None) != 0 and "NULL" in hip_lib.last_error()
    cnt = (C.c_int64 * 4)(-5, -5, -5, -5)
    p = 0x1000                                          # any aligned non-NULL address: nothing reads it before the checks fail
    call = lambda **kw: L.soar_mesh_close_holes(*[kw.get(k, d) for k, d in (
        ("V", 81), ("F", 128), ("verts", p), ("faces", p), ("limit", 300), ("ws", p), ("nb", 0), ("vo", 2 * p), ("fo", 3 * p),
        ("loops", p), ("counts", cnt), ("st", None))])
    for kw, word in ((dict(limit=2), "max_hole_edges=2"), (dict(limit=70000), "max_hole_edges=70000"), (dict(V=0), "V=0"),
                     (dict(verts=None), "NULL"), (dict(fo=None), "NULL"), (dict(counts=None), "NULL"), (dict(vo=p), "must not be"),
                     (dict(ws=None), "workspace"), (dict(ws=p + 64), "aligned"), (dict(), "need")):
        assert call(**kw) != 0 and word in hip_lib.last_error(), (kw, hip_lib.last_error())
    assert list(cnt) == [-5] * 4
