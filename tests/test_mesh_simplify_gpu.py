"""GPU tests of the mesh decimation (soar_amd/mesh.py: simplify, decimate, extract_mesh(decimate_target=); csrc/mesh_simplify.hip)
against the NumPy float64 restatement tests/mesh_simplify_ref.py, whose inputs tests/test_mesh_simplify_cpu.py checks."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_simplify_ref as S

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(v, f):
    from soar_amd import mesh
    return mesh.Mesh(torch.as_tensor(v).to(_dev()), torch.as_tensor(f).to(_dev()))


def _raw(lib, fn, v, f, cell, full):
    """the C call itself -> (rc, counts)"""
    from soar_amd import mesh
    V, F = v.shape[0], f.shape[0]
    nb = C.c_size_t(0)
    assert lib.soar_mesh_simplify_bytes(V, F, C.byref(nb)) == 0
    ws = mesh._workspace(nb.value, v.device)
    cnt = (C.c_int64 * 2)()
    st = torch.cuda.current_stream(v.device).cuda_stream
    if full:
        vo, fo = torch.empty(V, 3, device=v.device), torch.empty(max(F, 1), 3, dtype=torch.int32, device=v.device)
        rc = fn(V, F, v.data_ptr(), f.data_ptr(), cell, ws.data_ptr(), nb.value, vo.data_ptr(), fo.data_ptr(), cnt, st)
    else:
        rc = fn(V, F, v.data_ptr(), f.data_ptr(), cell, ws.data_ptr(), nb.value, cnt, st)
    torch.cuda.synchronize()
    return rc, (int(cnt[0]), int(cnt[1]))


@pytest.mark.parametrize("case", S.cases(), ids=lambda c: c.name)
def test_simplify_matches_the_restatement(case):
    """Largest |vertex difference| measured on an MI355X: 0 on every input; the bound is one float32 ulp."""
    from soar_amd import hip_lib, mesh
    want = S.result(case)
    m = _mesh(case.verts, case.faces)
    got = mesh.simplify(m, case.cell)
    gv, gf = _np(got.vertices), _np(got.faces)
    assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
    assert gv.shape == want.vertices.shape and gf.shape == want.faces.shape
    assert np.array_equal(gf, want.faces)
    if len(gv):
        tol = float(np.spacing(np.float32(np.abs(want.vertices).max())))          # one float32 ulp of the largest coordinate
        diff = float(np.abs(gv.astype(np.float64) - want.vertices.astype(np.float64)).max())
        print(f"{case.name}: V {len(gv)} F {len(gf)} max |dv| {diff:.3e} (bound {tol:.3e}), "
              f"bit-equal {int((gv == want.vertices).all(1).sum())} of {len(gv)}")
        assert diff <= tol
    again = mesh.simplify(m, case.cell)
    assert torch.equal(again.vertices, got.vertices) and torch.equal(again.faces, got.faces)   # bit for bit
    lib = hip_lib.lib()
    rc, cnt = _raw(lib, lib.soar_mesh_simplify_count, m.vertices, m.faces, case.cell, False)
    assert rc == 0 and cnt == (len(gv), len(gf))
    rc, cnt = _raw(lib, lib.soar_mesh_simplify, m.vertices, m.faces, case.cell, True)
    assert rc == 0 and cnt == (len(gv), len(gf))


def test_refused_inputs():
    from soar_amd import hip_lib, mesh
    lib = hip_lib.lib()
    err = hip_lib.last_error
    v, f = S.tetrahedron()
    m = _mesh(v, f)
    V, F = 4, 4
    nb = C.c_size_t(0)
    assert lib.soar_mesh_simplify_bytes(V, F, C.byref(nb)) == 0
    ws = mesh._workspace(nb.value, _dev())
    vo, fo = torch.full((V, 3), 7.0, device=_dev()), torch.full((F, 3), 7, dtype=torch.int32, device=_dev())
    cnt = (C.c_int64 * 2)(-1, -1)
    pv, pf, pw = m.vertices.data_ptr(), m.faces.data_ptr(), ws.data_ptr()

    def full(V=V, F=F, pv=pv, pf=pf, cell=0.5, pw=pw, nbytes=nb.value, po=vo.data_ptr(), pfo=fo.data_ptr(), c=cnt):
        return lib.soar_mesh_simplify(V, F, pv, pf, cell, pw, nbytes, po, pfo, c, None)

    def count(V=V, F=F, pv=pv, pf=pf, cell=0.5, pw=pw, nbytes=nb.value, c=cnt):
        return lib.soar_mesh_simplify_count(V, F, pv, pf, cell, pw, nbytes, c, None)

    for call in (full, count):
        assert call(V=0) != 0 and "V >= 1" in err()
        assert call(F=-1) != 0 and "F >= 0" in err()
        assert call(V=2 ** 30 + 1) != 0 and "2^30" in err()
        assert call(F=2 ** 30 + 1) != 0 and "2^30" in err()
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            assert call(cell=bad) != 0 and "cell" in err()
        assert call(pv=None) != 0 and "NULL" in err()
        assert call(pf=None) != 0 and "NULL" in err()
        assert call(pw=None) != 0 and "NULL" in err()
        assert call(c=None) != 0 and "NULL" in err()
        assert call(nbytes=nb.value - 1) != 0 and "workspace" in err()
        assert call(cell=1e-7) != 0 and "cells along axis" in err()               # 1 / 1e-7 cells: more than 2^21
    assert full(po=None) != 0 and "verts_out" in err()
    assert full(pfo=None) != 0 and "verts_out" in err()
    torch.cuda.synchronize()
    assert (vo == 7.0).all() and (fo == 7).all() and tuple(cnt) == (-1, -1)       # nothing was written
    with pytest.raises(ValueError, match="float32"):
        mesh.simplify(mesh.Mesh(m.vertices.double(), m.faces), 0.5)
    with pytest.raises(ValueError, match="int32"):
        mesh.simplify(mesh.Mesh(m.vertices, m.faces.long()), 0.5)
    with pytest.raises(ValueError, match="cell"):
        mesh.simplify(m, 0.0)
    bad = m.faces.clone()
    bad[2, 1] = 4
    with pytest.raises(RuntimeError, match="outside"):
        mesh.simplify(mesh.Mesh(m.vertices, bad), 0.01)
    nan = m.vertices.clone()
    nan[1, 2] = float("nan")
    with pytest.raises(RuntimeError, match="not finite"):
        mesh.simplify(mesh.Mesh(nan, m.faces), 0.01)
    no_faces = mesh.simplify(mesh.Mesh(m.vertices, m.faces[:0]), 0.01)
    assert no_faces.vertices.shape == (0, 3) and no_faces.faces.shape == (0, 3)


@pytest.fixture(scope="module")
def sphere():
    from soar_amd import mesh
    a = torch.arange(24, dtype=torch.float64)
    g = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1)
    field = ((g - torch.tensor([11.3, 11.6, 11.4], dtype=torch.float64)).norm(dim=-1) - 8.5).float()
    v, f = mesh.marching_cubes(field.to(_dev()))
    return mesh.Mesh(v, f)


def test_decimate_meets_the_budget_by_the_stated_search(sphere):
    from soar_amd import mesh
    target = 200
    v, f = _np(sphere.vertices), _np(sphere.faces)
    assert len(f) > 10 * target
    got = mesh.decimate(sphere, target_faces=target)
    gf = _np(got.faces)
    assert 0 < len(gf) <= target
    R = S.decimate_cells(lambda r: S.count(v, f, S.cell_for(v, r))[1], target, 4096)
    assert S.count(v, f, S.cell_for(v, R))[1] <= target < S.count(v, f, S.cell_for(v, R + 1))[1]
    same = mesh.simplify(sphere, float(S.cell_for(v, R)))
    assert torch.equal(got.vertices, same.vertices) and torch.equal(got.faces, same.faces)
    assert (gf[:, 0] != gf[:, 1]).all() and (gf[:, 1] != gf[:, 2]).all() and (gf[:, 0] != gf[:, 2]).all()
    assert len(np.unique(np.sort(gf, 1), axis=0)) == len(gf)
    assert np.array_equal(np.unique(gf), np.arange(len(got.vertices)))
    capped = mesh.decimate(sphere, target_faces=target, max_cells=3)               # the search stops at max_cells
    same = mesh.simplify(sphere, float(S.cell_for(v, 3)))
    assert torch.equal(capped.vertices, same.vertices) and torch.equal(capped.faces, same.faces)


def test_decimate_leaves_a_mesh_within_the_budget_alone(sphere):
    from soar_amd import mesh
    F = sphere.faces.shape[0]
    for target in (F, F + 1, 10 * F):
        got = mesh.decimate(sphere, target_faces=target)
        assert got.vertices is sphere.vertices and got.faces is sphere.faces


def test_extract_mesh_decimate_target():
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    s = syn.make_surfels(20_000)
    args = [t.to(_dev()) for t in (s.xyz, s.rot, s.scales, s.opacity)]
    kw = dict(resolution=64, n_views=16, image_size=256)
    plain = mesh.extract_mesh(*args, **kw)
    none = mesh.extract_mesh(*args, decimate_target=None, **kw)
    assert torch.equal(plain.vertices, none.vertices) and torch.equal(plain.faces, none.faces)
    F = plain.faces.shape[0]
    assert F > 2000
    small = mesh.extract_mesh(*args, decimate_target=500, **kw)
    assert 0 < small.faces.shape[0] <= 500 and small.faces.dtype == torch.int32
    assert int(small.faces.max()) == small.vertices.shape[0] - 1
    lo, hi = plain.vertices.min(0).values, plain.vertices.max(0).values
    _, voxel, _ = mesh.export_grid(args[0], args[2], 64)
    assert (small.vertices >= lo - voxel).all() and (small.vertices <= hi + voxel).all()    # world space, like the plain mesh
    roomy = mesh.extract_mesh(*args, decimate_target=F, **kw)
    assert torch.equal(roomy.vertices, plain.vertices) and torch.equal(roomy.faces, plain.faces)
