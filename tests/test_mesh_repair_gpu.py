"""GPU tests of the repair of non-manifold edges and vertices (soar_amd/mesh.py: repair_manifold, manifold_report and the ``repair``
switches of decimate, extract_mesh and export_avatar; csrc/mesh_repair.hip) against the NumPy restatement tests/mesh_repair_ref.py,
whose fixtures tests/test_mesh_repair_cpu.py checks.  The definition is integer work on the bits of float32 values computed operation
by operation, so every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_holes_ref as H
import mesh_repair_ref as R
import mesh_simplify_ref as S
from workspace_guard import FILLS, guarded

pytestmark = pytest.mark.gpu

FIXTURES = R.fixtures()


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(verts, faces):
    from soar_amd import mesh
    return mesh.Mesh(torch.from_numpy(np.ascontiguousarray(verts, np.float32)).to(_dev()),
                     torch.from_numpy(np.ascontiguousarray(faces, np.int32)).to(_dev()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _equals(got, want: R.Repaired):
    m, source, info = got
    assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and source.dtype == torch.int32
    assert tuple(info) == R.COUNT_NAMES and tuple(info.values()) == want.counts, (info, want.counts)
    assert m.faces.shape == want.faces.shape and np.array_equal(_np(m.faces), want.faces)
    assert np.array_equal(_np(source), want.source)
    assert m.vertices.shape == want.verts.shape and np.array_equal(_bits(_np(m.vertices)), _bits(want.verts))


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f.name)
def test_repair_equals_the_restatement(fx):
    from soar_amd import mesh
    m = _mesh(fx.verts, fx.faces)
    want = R.wanted(fx.name)
    first = mesh.repair_manifold(m)
    _equals(first, want)
    _equals(mesh.repair_manifold(m), want)                               # twice in a row
    assert mesh.manifold_report(m) == first[2] == mesh.manifold_report(m)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=_dev())                                 # and once on a stream of the caller's
    with torch.cuda.stream(s):
        on_stream = mesh.repair_manifold(m)
        report = mesh.manifold_report(m)
    s.synchronize()
    _equals(on_stream, want)
    assert report == first[2]
    # the input is untouched, and the output needs nothing more
    assert np.array_equal(_bits(_np(m.vertices)), _bits(fx.verts)) and np.array_equal(_np(m.faces), fx.faces)
    again, source, info = mesh.repair_manifold(first[0])
    assert torch.equal(again.vertices, first[0].vertices) and torch.equal(again.faces, first[0].faces)
    assert torch.equal(source, torch.arange(len(want.verts), dtype=torch.int32, device=_dev()))
    assert [info[k] for k in ("non_manifold_edges", "faces_removed", "null_faces", "vertex_copies", "unreferenced_vertices")] == [0] * 5


@pytest.mark.parametrize("fx", R.manifold_fixtures(), ids=lambda f: f.name)
def test_a_manifold_comes_back_with_equal_bits(fx):
    from soar_amd import mesh
    m = _mesh(fx.verts, fx.faces)
    got, source, info = mesh.repair_manifold(m)
    assert torch.equal(got.faces, m.faces) and np.array_equal(_bits(_np(got.vertices)), _bits(fx.verts))
    assert torch.equal(source, torch.arange(len(fx.verts), dtype=torch.int32, device=_dev()))
    assert info["vertices"] == len(fx.verts) and info["faces"] == len(fx.faces)


def test_meshes_without_faces_or_vertices_give_empty_results():
    from soar_amd import mesh
    dev = _dev()
    for V in (0, 2):
        m = mesh.Mesh(torch.rand(V, 3, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev))
        got, source, info = mesh.repair_manifold(m)
        assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and source.shape == (0,)
        assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32 and source.dtype == torch.int32
        assert info == mesh.manifold_report(m) == dict(zip(R.COUNT_NAMES, (0, 0, 0, 0, 0, 0, V, 0, 0)))


def test_a_face_outside_the_mesh_is_refused_and_nothing_is_written():
    from soar_amd import hip_lib, mesh
    L = hip_lib.lib()
    dev = _dev()
    fx = R.fixture("tetrahedra_on_an_edge")
    V, F = len(fx.verts), len(fx.faces)
    for value in (V, -1):
        bad = fx.faces.copy()
        bad[3, 1] = value
        m = _mesh(fx.verts, bad)
        for call in (mesh.repair_manifold, mesh.manifold_report):
            with pytest.raises(hip_lib.SoarHipError, match=rf"1 faces name a vertex outside \[0, {V}\)"):
                call(m)
        # the counting call writes nothing but its workspace
        n = C.c_size_t(0)
        assert L.soar_mesh_repair_workspace_size(V, F, C.byref(n)) == 0
        ws = mesh._workspace(n.value, dev)
        cnt = (C.c_int64 * 9)(*([-5] * 9))
        rc = L.soar_mesh_repair_count(V, F, m.vertices.data_ptr(), m.faces.data_ptr(), ws.data_ptr(), n.value, cnt,
                                      torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and "outside" in hip_lib.last_error() and list(cnt) == [-5] * 9
        assert np.array_equal(_np(m.faces), bad)


def test_the_c_call_writes_what_it_reports_and_no_more():
    from soar_amd import hip_lib, mesh
    L = hip_lib.lib()
    dev = _dev()
    fx = R.fixture("three_fans")
    want = R.wanted(fx.name)
    m = _mesh(fx.verts, fx.faces)
    V, F = len(fx.verts), len(fx.faces)
    n = C.c_size_t(0)
    assert L.soar_mesh_repair_workspace_size(V, F, C.byref(n)) == 0
    ws = mesh._workspace(n.value, dev)
    vo = torch.full((3 * F, 3), float("nan"), device=dev)
    fo = torch.full((F, 3), -7, dtype=torch.int32, device=dev)
    so = torch.full((3 * F,), -7, dtype=torch.int32, device=dev)
    cnt = (C.c_int64 * 9)(*([-5] * 9))
    rc = L.soar_mesh_repair(V, F, m.vertices.data_ptr(), m.faces.data_ptr(), ws.data_ptr(), n.value, vo.data_ptr(), fo.data_ptr(),
                            so.data_ptr(), cnt, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip_lib.last_error()
    torch.cuda.synchronize()
    assert tuple(cnt) == want.counts
    nv, nf = want.counts[:2]
    assert np.array_equal(_bits(_np(vo[:nv])), _bits(want.verts)) and np.array_equal(_np(fo[:nf]), want.faces)
    assert np.array_equal(_np(so[:nv]), want.source)
    assert torch.isnan(vo[nv:]).all() and (fo[nf:] == -7).all() and (so[nv:] == -7).all()


# ---- the feature: what could not be reached before -------------------------------------------------------------------------------

def test_clustered_sheets_are_repaired():
    """mesh.simplify of two nested icosphere(4) (scale 1 / 0.93, 14 cells): about 2.9k faces with hundreds of non-manifold edges;
    repair_manifold leaves none, and no vertex with more than one fan"""
    from soar_amd import mesh
    v, f, cell = R.two_sheets(4, 0.93, 14)
    clustered = mesh.simplify(_mesh(v, f), float(cell))
    before = mesh.manifold_report(clustered)
    print(f"clustered: {tuple(clustered.faces.shape)} faces, report {before}")
    assert clustered.faces.shape[0] > 2 * 256 and before["non_manifold_edges"] > 0
    assert before["non_manifold_edges"] == R.non_manifold_edges(_np(clustered.faces))
    got = mesh.repair_manifold(clustered)
    _equals(got, R.repair(_np(clustered.vertices), _np(clustered.faces)))
    after = mesh.manifold_report(got[0])
    assert after["non_manifold_edges"] == 0 and after["vertex_copies"] == 0 and after["faces_removed"] == 0
    assert R.non_manifold_edges(_np(got[0].faces)) == 0


def test_touching_holes_close_after_the_repair():
    from soar_amd import mesh
    fx = H.fixture("d_grid9_touching_holes")
    m = _mesh(fx.verts, fx.faces)
    assert mesh.open_border_edges(mesh.close_holes(m)[0]) == 6
    repaired, source, info = mesh.repair_manifold(m)
    assert info["vertex_copies"] == 1 and int(source[-1]) == 40
    closed, loops = mesh.close_holes(repaired)
    assert mesh.open_border_edges(closed) == 0 and 6 in loops.tolist()
    assert H.is_closed_and_oriented(_np(closed.faces))


# ---- wiring ------------------------------------------------------------------------------------------------------------------------

def test_decimate_repairs_when_asked():
    from soar_amd import mesh
    v, f, _ = R.two_sheets(4, 0.93, 14)
    m = _mesh(v, f)
    target = 3000
    plain = mesh.decimate(m, target)
    off = mesh.decimate(m, target, repair=False)
    assert torch.equal(plain.vertices, off.vertices) and torch.equal(plain.faces, off.faces)
    assert 0 < plain.faces.shape[0] <= target and mesh.manifold_report(plain)["non_manifold_edges"] > 0
    on = mesh.decimate(m, target, repair=True)
    want, _, _ = mesh.repair_manifold(plain)
    assert isinstance(on, mesh.Mesh) and torch.equal(on.vertices, want.vertices) and torch.equal(on.faces, want.faces)
    assert on.faces.shape[0] < plain.faces.shape[0] and mesh.manifold_report(on)["non_manifold_edges"] == 0
    # within the budget: the same tensors without, the repair with
    assert mesh.decimate(plain, target) is plain
    within = mesh.decimate(plain, target, repair=True)
    assert torch.equal(within.vertices, want.vertices) and torch.equal(within.faces, want.faces)


def test_export_avatar_repairs_when_asked():
    from test_mesh_holes_gpu import EXPORT, _open_capsule_surfels
    from soar_amd import body, mesh
    from soar_amd import synthetic as syn
    dev = _dev()
    surf = tuple(t.to(dev) for t in _open_capsule_surfels(2000, 2))
    means3D, rotations, scales, opacities, colors = surf
    bm = syn.make_body_model(V=1024)
    sv, sw = bm.v_template.to(dev), bm.lbs_weights.to(dev)
    kw = dict(EXPORT, decimate_target=600)
    grid = dict(resolution=kw["resolution"], n_views=kw["n_views"], image_size=kw["image_size"], decimate_target=kw["decimate_target"])

    def finish(m):
        m = mesh.smooth(m, mesh.SMOOTH_STEPS)
        color, quality, _ = mesh.vertex_attributes(m.vertices, means3D, colors, mesh.ATTR_K)
        return dict(mesh=m, color=color, quality=quality, normals=body.vertex_normals(m.vertices, m.faces),
                    weights=mesh.skin_weights(m, sv, sw, 30))

    def same(got, wanted_):
        assert torch.equal(got["mesh"].vertices, wanted_["mesh"].vertices) and torch.equal(got["mesh"].faces, wanted_["mesh"].faces)
        for key in ("color", "quality", "normals", "weights"):
            assert torch.equal(got[key], wanted_[key]), key

    def prune(m):
        _, q, _ = mesh.vertex_attributes(m.vertices, means3D, colors, mesh.ATTR_K)
        return mesh.prune_by_quality(m, q, kw["quality_thresh"])[0]

    # repair=False: today's keys and bits, the composition of the public steps without the repair
    raw = mesh.extract_mesh(means3D, rotations, scales, opacities, **grid)
    off = mesh.export_avatar(surf, sv, sw, repair=False, **kw)
    assert sorted(off) == ["color", "mesh", "normals", "quality", "weights"]
    same(off, finish(prune(raw)))
    raw_off = mesh.extract_mesh(means3D, rotations, scales, opacities, repair=False, **grid)
    assert torch.equal(raw_off.vertices, raw.vertices) and torch.equal(raw_off.faces, raw.faces)
    # repair=True: after the extraction and again after the pruning, before the holes are closed
    first, _, info1 = mesh.repair_manifold(raw)
    second, _, info2 = mesh.repair_manifold(prune(first))
    closed, loops = mesh.close_holes(second, 300)
    on = mesh.export_avatar(surf, sv, sw, repair=True, max_hole_edges=300, **kw)
    assert sorted(on) == ["closed", "color", "mesh", "normals", "quality", "repair", "weights"]
    assert on["repair"] == [info1, info2] and torch.equal(on["closed"], loops)
    print(f"export: raw {tuple(raw.faces.shape)}, repairs {on['repair']}")
    same(on, finish(closed))
    report = mesh.manifold_report(on["mesh"])
    assert report["non_manifold_edges"] == 0 and report["vertex_copies"] == 0
    V = int(on["mesh"].vertices.shape[0])
    assert on["color"].shape == (V, 3) and on["weights"].shape == (V, 55)
    # extract_mesh(repair=True) repairs the clustered mesh before it is scaled to world space
    ex = mesh.extract_mesh(means3D, rotations, scales, opacities, repair=True, **grid)
    assert mesh.manifold_report(ex) == dict(mesh.manifold_report(ex), non_manifold_edges=0, vertex_copies=0, faces_removed=0, null_faces=0,
                                            unreferenced_vertices=0)
    assert ex.faces.shape[0] <= raw.faces.shape[0]


# ---- the workspace's contract (the scheme of tests/test_workspace_contract_gpu.py) -------------------------------------------------

def test_the_workspace_is_held_to_its_contract():
    """The workspace between two bands of 0xA5, exactly as large as the sizing call answered, and holding zeros, 0xFF bytes or seeded
    noise beforehand: the outputs are the same bits under all three and outside any guard, and the bands stay intact.  What was read
    in carve_repair before the first run: counts and totals by memsets; vmin for every vertex, fkeep, akeys, ids and parent for every
    face and corner by repair_faces_kernel; ekeys by repair_keys_kernel for every entry, the sorted arrays by the sorts; vkeep and
    cflag for every vertex and corner by repair_flags_kernel; voff / foff / coff by the scans."""
    from soar_amd import mesh
    fx = R.fixture("tetrahedra_on_an_edge")
    want = R.wanted(fx.name)
    m = _mesh(fx.verts, fx.faces)
    runs = {}
    for fill in FILLS:
        with guarded(fill) as g:
            report = mesh.manifold_report(m)
            runs[fill] = mesh.repair_manifold(m)
            assert len(g.buffers) == 2 and all(b[2] == "soar_amd.mesh" for b in g.buffers)
            g.check()
        assert report == runs[fill][2]
    for fill in FILLS:
        _equals(runs[fill], want)
    _equals(mesh.repair_manifold(m), want)
