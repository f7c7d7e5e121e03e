"""The yardstick of the mesh decimation, checked itself: tests/mesh_simplify_ref.py against closed forms, the inputs of the GPU
test against the rank threshold's band, and what the C ABI and the Python interface refuse without a device."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_simplify_ref as S


def _case(name):
    return next(c for c in S.cases() if c.name == name)


def test_the_python_interface_exists_and_refuses_cpu_tensors():
    from soar_amd import mesh
    m = mesh.Mesh(torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.simplify(m, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.decimate(m, 1)
    assert mesh.DECIMATE_TARGET == 100_000


def test_cube_corners_edges_and_faces():
    c = _case("cube")
    r = S.result(c)
    on = lambda a: (np.abs(a) <= 1e-12) | (np.abs(a - 1.0) <= 1e-12)           # coordinate on one of the cube's planes
    nplanes = on(r.x64).sum(1)
    # what the cluster's cell says it is: the outer cell layers (index 0 and 3 of 4) hold the cube's planes
    outer = ((r.cell_index == 0) | (r.cell_index == 3)).sum(1)
    assert (outer >= 1).all() and sorted(set(outer.tolist())) == [1, 2, 3]
    assert (outer == 3).sum() == 8 and (outer == 2).sum() == 12 * 2            # one cluster per corner, two more along each edge
    for k in range(3):
        want = np.where(r.cell_index[:, k] == 0, 0.0, 1.0)
        hit = (r.cell_index[:, k] == 0) | (r.cell_index[:, k] == 3)
        assert np.abs(r.x64[hit, k] - want[hit]).max() <= 1e-12                # corner on the corner, edge on the edge, face on the face
    assert (nplanes >= outer).all()
    # along an edge / inside a face the free coordinates are the cluster mean's
    free = ~((r.cell_index == 0) | (r.cell_index == 3))
    assert np.abs(r.x64[free] - r.mean64[free]).max() <= 1e-12
    assert len(r.faces) > 0 and r.faces.max() == len(r.vertices) - 1


def test_flat_grid_projects_the_cluster_means_onto_the_plane():
    c = _case("flat_grid")
    r = S.result(c)
    assert len(r.vertices) == 25 and len(r.faces) == 32                          # 5 x 5 cells, two triangles per cell corner patch
    assert np.abs(r.x64[:, 2] - 0.25).max() <= 1e-12
    assert np.abs(r.x64[:, :2] - r.mean64[:, :2]).max() <= 1e-12
    assert r.ratios.shape == (25, 3) and (np.sort(r.ratios, 1)[:, :2] < 1e-12).all()    # rank 1 everywhere


def test_tetrahedron_both_ways():
    v, f = S.tetrahedron()
    r = S.result(_case("tetrahedron_tiny_cell"))
    assert np.array_equal(r.faces, f) and np.abs(r.x64 - v).max() <= 1e-12      # itself, in its own vertex order
    r = S.result(_case("tetrahedron_huge_cell"))
    assert r.vertices.shape == (0, 3) and r.faces.shape == (0, 3)
    assert S.count(v, f, 10.0) == (0, 0) and S.count(v, f, 0.01) == (4, 4)


def test_degenerate_input():
    r = S.result(_case("degenerate"))
    assert np.array_equal(r.faces, S.DEGENERATE_FACES)
    assert np.abs(r.x64 - S.DEGENERATE_VERTS).max() <= 1e-12
    assert np.array_equal(r.x64[4], [2.0, 0.0, 0.0])                              # vertex 4 sees a zero quadric: its own mean


def test_icosphere_sizes():
    assert S.icosphere(2)[0].shape == (162, 3) and S.icosphere(4)[0].shape == (2562, 3) and S.icosphere(4)[1].shape == (5120, 3)
    c = _case("translated")
    assert np.abs(c.verts.mean(0) - [100.0, -50.0, 3.0]).max() < 0.1


@pytest.mark.parametrize("case", S.cases(), ids=lambda c: c.name)
def test_no_input_of_the_gpu_test_sits_on_the_rank_threshold(case):
    r = S.result(case)
    assert S.ratios_in_band(r.ratios) == 0, np.sort(r.ratios.reshape(-1))[:20]
    n_v, n_f = S.count(case.verts, case.faces, case.cell)
    assert (n_v, n_f) == (len(r.vertices), len(r.faces))
    if len(r.faces):
        assert len(np.unique(r.faces)) == len(r.vertices)                        # no unused vertex
        assert (r.faces[:, 0] != r.faces[:, 1]).all() and (r.faces[:, 1] != r.faces[:, 2]).all() and (r.faces[:, 0] != r.faces[:, 2]).all()
        assert len(np.unique(np.sort(r.faces, 1), axis=0)) == len(r.faces)       # no face twice, whatever its winding


def test_larger_inputs_exercise_more_than_one_workgroup():
    r = S.result(_case("icosphere4_R16"))
    assert len(r.vertices) > 256 and len(r.faces) > 256
    r3 = S.result(_case("icosphere4_R3"))
    assert len(r3.vertices) < 64                                                 # clusters of hundreds of faces: runs of many 64-face rounds


def test_decimate_cells_follows_the_stated_search():
    from soar_amd import mesh
    counts = lambda R: [0, 0, 3, 8, 12, 30, 28, 45, 70, 90, 130][min(R, 10)]    # not monotone at 5 / 6
    for target in (0, 2, 10, 29, 30, 44, 100, 1000):
        for max_cells in (1, 3, 8, 64):
            want = S.decimate_cells(counts, target, max_cells)
            assert mesh._decimate_cells(counts, target, max_cells) == want
            assert counts(want) <= target and want <= max_cells
            assert want == max_cells or counts(want + 1) > target             # stopped by the budget or by max_cells, nothing else
    # worked by hand, target 29: 1, 2, 4 pass, 8 (70) fails; the bisection tries 6 (28: passes) and 7 (45: fails) -> 6, past the 30 at 5
    assert mesh._decimate_cells(counts, 29, 64) == 6 and mesh._decimate_cells(counts, 44, 64) == 6
    assert mesh._decimate_cells(counts, 10, 64) == 3 and mesh._decimate_cells(counts, 2, 64) == 1


def test_c_abi_refuses_bad_arguments_before_any_launch():
    from soar_amd import build, hip_lib
    build.build()
    lib = hip_lib.lib()
    err = hip_lib.last_error
    n = C.c_size_t(0)
    assert lib.soar_mesh_simplify_bytes(0, 10, C.byref(n)) != 0
    assert lib.soar_mesh_simplify_bytes(10, -1, C.byref(n)) != 0
    assert lib.soar_mesh_simplify_bytes(10, 20, None) != 0
    assert lib.soar_mesh_simplify_bytes(2 ** 30 + 1, 20, C.byref(n)) != 0 and lib.soar_mesh_simplify_bytes(10, 2 ** 30 + 1, C.byref(n)) != 0
    assert lib.soar_mesh_simplify_bytes(10, 0, C.byref(n)) == 0 and n.value % 256 == 0
    assert lib.soar_mesh_simplify_bytes(10, 20, C.byref(n)) == 0 and n.value % 256 == 0 and n.value > 0
    need, p, ws = n.value, 0x2000, 0x1000                                        # never dereferenced: every call is refused
    cnt = (C.c_int64 * 2)()
    both = [("count", lambda *a: lib.soar_mesh_simplify_count(*a[:7], cnt if a[7] else None, None)),
            ("full", lambda *a: lib.soar_mesh_simplify(*a[:7], p, p, cnt if a[7] else None, None))]
    for _, call in both:
        assert call(0, 20, p, p, 0.1, ws, need, True) != 0 and "V >= 1" in err()
        assert call(10, -1, p, p, 0.1, ws, need, True) != 0 and "F >= 0" in err()
        assert call(2 ** 30 + 1, 20, p, p, 0.1, ws, need, True) != 0 and "2^30" in err()
        assert call(10, 2 ** 30 + 1, p, p, 0.1, ws, need, True) != 0 and "2^30" in err()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(10, 20, p, p, bad, ws, need, True) != 0 and "cell" in err()
        assert call(10, 20, None, p, 0.1, ws, need, True) != 0 and "NULL" in err()
        assert call(10, 20, p, None, 0.1, ws, need, True) != 0 and "NULL" in err()
        assert call(10, 20, p, p, 0.1, None, need, True) != 0 and "NULL" in err()
        assert call(10, 20, p, p, 0.1, ws, need, False) != 0 and "NULL" in err()
        assert call(10, 20, p, p, 0.1, ws + 1, need, True) != 0 and "aligned" in err()
        assert call(10, 20, p, p, 0.1, ws, need - 1, True) != 0 and "workspace" in err()
    assert lib.soar_mesh_simplify(10, 20, p, p, 0.1, ws, need, None, p, cnt, None) != 0 and "verts_out" in err()
    assert lib.soar_mesh_simplify(10, 20, p, p, 0.1, ws, need, p, None, cnt, None) != 0 and "verts_out" in err()
