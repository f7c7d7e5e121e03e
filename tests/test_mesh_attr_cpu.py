"""CPU tests of the yardstick of the mesh attributes (tests/mesh_attr_ref.py: the restatement test_mesh_attr_gpu.py compares
csrc/mesh_attr.hip with), of the writers and of the interface of soar_amd/mesh.py.  No kernel runs here."""
import math

import numpy as np
import pytest
import torch

import mesh_attr_ref as A

KS = (1, 4, 8)


def test_fixtures_are_what_they_claim():
    fx = {f.name: f for f in A.fixtures()}
    assert fx["icosphere2"].verts.shape == (162, 3) and fx["icosphere2"].faces.shape == (320, 3)
    assert fx["grid9"].verts.shape == (81, 3) and fx["grid9"].faces.shape == (128, 3)
    assert fx["single"].verts.shape == (1, 3) and fx["single"].faces.shape == (0, 3)
    assert len(fx["disc65"].verts) == 65 and len(fx["disc257"].verts) == 257
    for f in fx.values():
        assert f.verts.dtype == np.float32 and f.faces.dtype == np.int32
        if len(f.faces):
            assert f.faces.min() >= 0 and f.faces.max() < len(f.verts)
            assert (f.faces[:, 0] != f.faces[:, 1]).all() and (f.faces[:, 1] != f.faces[:, 2]).all() and (f.faces[:, 0] != f.faces[:, 2]).all()
    # the closed sphere has no border, the fan's shared edge has three faces, the isolated vertex has an empty row
    rs, nbr, border = A.adjacency(162, fx["icosphere2"].faces)
    assert not border.any() and rs[-1] == 6 * 320
    rs, nbr, border = A.adjacency(5, fx["fan3"].faces)
    assert nbr[rs[0]:rs[1]].tolist() == [1, 1, 1, 2, 3, 4] and border.all()
    rs, nbr, border = A.adjacency(5, fx["isolated"].faces)
    assert rs[5] - rs[4] == 0 and not border.any()
    rs, nbr, border = A.adjacency(81, fx["grid9"].faces)
    n = 9
    want = np.zeros((n, n), bool)
    want[0], want[-1], want[:, 0], want[:, -1] = True, True, True, True
    assert np.array_equal(border.reshape(n, n), want)


def test_one_step_scales_the_icosahedron():
    v, f = A.icosahedron()
    got = A.smooth(v, f, 1)
    s = (1.0 + 2.0 * math.sqrt(5.0)) / 11.0
    assert np.abs(got - s * v).max() < 1e-14
    assert np.abs(A.smooth(v, f, 3) - s ** 3 * v).max() < 1e-14


def test_border_rule_on_the_open_grid():
    n = 9
    v, f = A.open_grid(n)
    v = v.copy()
    rng = np.random.default_rng(0)
    inner = np.ones((n, n), bool)
    inner[0], inner[-1], inner[:, 0], inner[:, -1] = False, False, False, False
    v[inner.ravel(), 2] = rng.standard_normal(int(inner.sum()))           # an interior that pulls out of the plane
    got = A.smooth(v, f, 1).reshape(n, n, 3)
    v3 = v.reshape(n, n, 3)
    for j in range(1, n - 1):                                             # straight borders: on their lines, at the mean of three
        for (a, b, c) in (((0, j), (0, j - 1), (0, j + 1)), ((n - 1, j), (n - 1, j - 1), (n - 1, j + 1)),
                          ((j, 0), (j - 1, 0), (j + 1, 0)), ((j, n - 1), (j - 1, n - 1), (j + 1, n - 1))):
            assert np.abs(got[a] - (v3[a] + v3[b] + v3[c]) / 3.0).max() < 1e-15
            assert got[a][2] == 0.0
    for a, b, c in (((0, 0), (0, 1), (1, 0)), ((0, n - 1), (0, n - 2), (1, n - 1)), ((n - 1, 0), (n - 2, 0), (n - 1, 1)),
                    ((n - 1, n - 1), (n - 1, n - 2), (n - 2, n - 1))):
        assert np.abs(got[a] - (v3[a] + v3[b] + v3[c]) / 3.0).max() < 1e-15   # corners: (P + a + b) / 3, diagonal or not
    # an interior vertex: every neighbour once per adjacent face, twice each here
    i, j = 4, 4
    ring = [(i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1), (i - 1, j - 1), (i + 1, j + 1)]
    want = (v3[i, j] + 2.0 * sum(v3[p] for p in ring)) / 13.0
    assert np.abs(got[i, j] - want).max() < 1e-15
    # a vertex without neighbours stays
    assert np.array_equal(A.smooth(np.array([[1.0, 2.0, 3.0]]), np.zeros((0, 3), np.int32), 3), [[1.0, 2.0, 3.0]])


@pytest.mark.parametrize("k", KS)
def test_neighbour_gap_of_every_fixture(k):
    """float32 distances cannot reorder neighbours whose float64 squared distances differ by more than 1e-5 relative (the float32
    evaluation is off by at most 8 * 2^-24 = 4.8e-7 relative): the exact comparison of indices on the GPU is well defined."""
    pts, _ = A.surfels()
    for f in A.fixtures():
        gap = A.min_relative_gap(f.verts, pts, k)
        assert gap > A.GAP, (f.name, k, gap)


def test_transfer_restatement():
    pts, col = A.surfels()
    v = A.fixtures()[0].verts
    idx, color, quality, d2 = A.transfer(v, pts, col, 4)
    brute = ((v[:, None].astype(np.float64) - pts[None].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(np.sort(brute, 1)[:, :4], d2) and np.array_equal(quality, brute.min(1))
    assert np.array_equal(idx[:, 0], brute.argmin(1))
    assert color.min() >= 0.0 and color.max() <= 1.0
    c32 = A.color_float32(col, idx)
    assert c32.dtype == np.float32 and np.abs(c32 - color).max() <= 4 * 2.0 ** -24
    raw = col.astype(np.float64)[idx].mean(1)
    assert (raw < 0).any() and (raw > 1).any()                           # the clamp is exercised


def test_prune_restatement():
    f = A.fixtures()[1]
    q = np.arange(81, dtype=np.float32)
    v, fc, keep = A.prune(f.verts, f.faces, q, 39.5)
    assert keep.tolist() == list(range(40)) and np.array_equal(v, f.verts[:40])
    assert len(fc) and fc.max() < 40 and np.array_equal(f.verts[:40][fc], f.verts[f.faces[(f.faces < 40).all(1)]])
    v, fc, keep = A.prune(f.verts, f.faces, q, 1e9)
    assert len(v) == 81 and np.array_equal(fc, f.faces) and keep.tolist() == list(range(81))
    v, fc, keep = A.prune(f.verts, f.faces, q, -1.0)
    assert v.shape == (0, 3) and fc.shape == (0, 3) and keep.shape == (0,)


# ---- writers ---------------------------------------------------------------------------------------------------------------------

def _small():
    from soar_amd import mesh
    f = A.fixtures()[3]
    return mesh.Mesh(torch.from_numpy(f.verts), torch.from_numpy(f.faces)), f


def test_save_obj_without_colours_writes_the_bytes_it_always_wrote(tmp_path):
    from soar_amd import mesh
    m, f = _small()
    mesh.save_obj(str(tmp_path / "a.obj"), m)
    want = "".join(f"v {a:.9g} {b:.9g} {c:.9g}\n" for a, b, c in f.verts.tolist())
    want += "".join(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f.faces.tolist())
    assert (tmp_path / "a.obj").read_bytes() == want.encode()
    mesh.save_obj(str(tmp_path / "b.obj"), m, None)
    assert (tmp_path / "b.obj").read_bytes() == want.encode()


def test_obj_with_colours_and_ply_round_trip(tmp_path):
    from soar_amd import mesh
    m, f = _small()
    rng = np.random.default_rng(1)
    V = len(f.verts)
    col = rng.random((V, 3)).astype(np.float32)
    col[0] = [0.0, 1.0, 0.5]
    nrm = rng.standard_normal((V, 3)).astype(np.float32)
    q = rng.random(V).astype(np.float32)
    mesh.save_obj(str(tmp_path / "c.obj"), m, torch.from_numpy(col))
    v, fc = A.parse_obj(str(tmp_path / "c.obj"))
    assert v.shape == (V, 6) and np.array_equal(v[:, :3].astype(np.float32), f.verts) and np.array_equal(v[:, 3:].astype(np.float32), col)
    assert np.array_equal(fc, f.faces)
    with pytest.raises(ValueError):
        mesh.save_obj(str(tmp_path / "d.obj"), m, torch.from_numpy(col[:-1]))

    mesh.save_ply(str(tmp_path / "full.ply"), m, torch.from_numpy(col), torch.from_numpy(nrm), torch.from_numpy(q))
    props, fc = A.parse_ply(str(tmp_path / "full.ply"))
    assert list(props) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "quality"]
    assert np.array_equal(np.stack([props[k] for k in "xyz"], 1), f.verts)
    assert np.array_equal(np.stack([props[k] for k in ("nx", "ny", "nz")], 1), nrm)
    assert np.array_equal(np.stack([props[k] for k in ("red", "green", "blue")], 1), np.floor(col * 255.0 + 0.5).astype(np.uint8))
    assert props["red"][0] == 0 and props["green"][0] == 255 and props["blue"][0] == 128
    assert np.array_equal(props["quality"], q) and np.array_equal(fc, f.faces)
    mesh.save_ply(str(tmp_path / "bare.ply"), m)
    props, fc = A.parse_ply(str(tmp_path / "bare.ply"))
    assert list(props) == ["x", "y", "z"] and np.array_equal(fc, f.faces)
    mesh.save_ply(str(tmp_path / "col.ply"), m, colors=torch.from_numpy(col))
    assert list(A.parse_ply(str(tmp_path / "col.ply"))[0]) == ["x", "y", "z", "red", "green", "blue"]

    w = rng.random((V, 7)).astype(np.float32)
    mesh.save_skinned(str(tmp_path / "s.npz"), m, torch.from_numpy(w), torch.from_numpy(col))
    z = np.load(str(tmp_path / "s.npz"))
    assert sorted(z.files) == ["colors", "faces", "vertices", "weights"]
    assert np.array_equal(z["vertices"], f.verts) and np.array_equal(z["faces"], f.faces) and z["faces"].dtype == np.int32
    assert np.array_equal(z["weights"], w) and np.array_equal(z["colors"], col)
    mesh.save_skinned(str(tmp_path / "t.npz"), m, torch.from_numpy(w), torch.from_numpy(col))
    assert (tmp_path / "s.npz").read_bytes() == (tmp_path / "t.npz").read_bytes()


# ---- interface -------------------------------------------------------------------------------------------------------------------

def test_the_new_names_exist_and_refuse_cpu_tensors():
    from soar_amd import hip_lib, mesh
    m, f = _small()
    V = len(f.verts)
    pts, col = (torch.from_numpy(a) for a in A.surfels())
    no_cpu = pytest.raises(RuntimeError, match="no CPU fallback")
    with no_cpu:
        mesh.vertex_attributes(m.vertices, pts, col, k=4)
    with no_cpu:
        mesh.prune_by_quality(m, torch.zeros(V), 0.5)
    with no_cpu:
        mesh.adjacency(m)
    with no_cpu:
        mesh.smooth(m, steps=3)
    with no_cpu:
        mesh.skin_weights(m, pts, torch.rand(len(pts), 5), K=30)
    with no_cpu:
        mesh.pose_mesh(m, torch.rand(V, 5), torch.eye(4).expand(2, 5, 4, 4))
    with no_cpu:
        mesh.export_avatar((pts, torch.zeros(len(pts), 4), torch.ones(len(pts), 3), torch.ones(len(pts), 1), col), pts,
                           torch.rand(len(pts), 5), resolution=32)
    # shapes are judged before the device: the rasterizer reads scales as [P,3], so [P,1] and [P,2] must never reach it
    P = len(pts)
    for bad in (torch.ones(P, 1), torch.ones(P, 2), torch.ones(P - 1, 3)):
        with pytest.raises(ValueError, match="scales must be"):
            mesh.export_avatar((pts, torch.zeros(P, 4), bad, torch.ones(P, 1), col), pts, torch.rand(P, 5), resolution=32)
    assert mesh.Mesh._fields == ("vertices", "faces")
    for name in ("soar_mesh_attr_transfer", "soar_mesh_adjacency", "soar_mesh_smooth", "soar_mesh_prune"):
        assert name in hip_lib.SIGNATURES and name + "_bytes" in hip_lib.SIGNATURES
