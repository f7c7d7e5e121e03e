"""GPU tests of the hole closing (soar_amd/mesh.py: close_holes, open_border_edges, export_avatar(max_hole_edges=...);
csrc/mesh_holes.hip) against the NumPy restatement tests/mesh_holes_ref.py, whose fixtures tests/test_mesh_holes_cpu.py checks.
The definition is integer work and one float64 sum in a stated order, so every comparison is bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_holes_ref as H

pytestmark = pytest.mark.gpu

FIXTURES = H.fixtures()
LIMITS = (3, 31, 32, 300)


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(fx):
    from soar_amd import mesh
    return mesh.Mesh(torch.from_numpy(fx.verts).to(_dev()), torch.from_numpy(fx.faces).to(_dev()))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                                                        b.view(np.uint32) if b.dtype == np.float32 else b)


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f.name)
def test_close_holes_equals_the_restatement(fx):
    from soar_amd import mesh
    m = _mesh(fx)
    for limit in LIMITS:
        want = H.wanted(fx.name, limit)
        got, closed = mesh.close_holes(m, limit)
        assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32 and closed.dtype == torch.int32
        assert got.faces.shape == want.faces.shape and np.array_equal(_np(got.faces), want.faces), (fx.name, limit)
        assert np.array_equal(_np(closed), want.closed), (fx.name, limit)
        assert _same_bits(_np(got.vertices), want.verts), (fx.name, limit)
        # the counts: what is left open, and what there was
        assert mesh.open_border_edges(got) == want.open_left, (fx.name, limit)
        again, closed2 = mesh.close_holes(m, limit)                       # two runs, the same bits
        assert torch.equal(again.vertices, got.vertices) and torch.equal(again.faces, got.faces) and torch.equal(closed2, closed)
    assert mesh.open_border_edges(m) == H.loops(fx.faces)[1]
    assert torch.equal(m.vertices, torch.from_numpy(fx.verts).to(_dev())) and torch.equal(m.faces, torch.from_numpy(fx.faces).to(_dev()))
    got, closed = mesh.close_holes(m)                                     # the default is the reference's 300
    assert np.array_equal(_np(got.faces), H.wanted(fx.name, 300).faces)


def test_a_stream_of_the_callers_changes_nothing():
    from soar_amd import mesh
    for prefix in "ach":
        fx = H.fixture(prefix)
        m = _mesh(fx)
        want, wclosed = mesh.close_holes(m)
        torch.cuda.synchronize()
        s = torch.cuda.Stream(device=_dev())
        with torch.cuda.stream(s):
            got, closed = mesh.close_holes(m)
        s.synchronize()
        assert torch.equal(got.vertices, want.vertices) and torch.equal(got.faces, want.faces) and torch.equal(closed, wclosed)


@pytest.mark.parametrize("prefix", ["a", "h"])
def test_the_closed_spheres_have_no_border(prefix):
    from soar_amd import mesh
    fx = H.fixture(prefix)
    m = _mesh(fx)
    assert bool(mesh.adjacency(m)[2].any()) and mesh.open_border_edges(m) > 0
    got, closed = mesh.close_holes(m)
    assert not bool(mesh.adjacency(got)[2].any()) and mesh.open_border_edges(got) == 0
    assert int(closed.sum()) == mesh.open_border_edges(m)


def test_the_c_call():
    from soar_amd import hip_lib, mesh
    L = hip_lib.lib()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    fx = H.fixture("a")
    m = _mesh(fx)
    V, F = len(fx.verts), len(fx.faces)
    n = C.c_size_t(0)
    assert L.soar_mesh_close_holes_bytes(V, F, C.byref(n)) == 0 and n.value % 256 == 0 and n.value > 0
    need = n.value
    ws = mesh._workspace(need + 256, dev)
    vo = torch.full((V + 3 * F // 4, 3), float("nan"), device=dev)
    fo = torch.full((4 * F, 3), -7, dtype=torch.int32, device=dev)
    lo = torch.full((F,), -7, dtype=torch.int32, device=dev)
    cnt = (C.c_int64 * 4)(-5, -5, -5, -5)
    p = lambda t: t.data_ptr()
    call = lambda **kw: L.soar_mesh_close_holes(*[kw.get(k, d) for k, d in (
        ("V", V), ("F", F), ("verts", p(m.vertices)), ("faces", p(m.faces)), ("limit", 300), ("ws", p(ws)), ("nb", need), ("vo", p(vo)),
        ("fo", p(fo)), ("loops", p(lo)), ("counts", cnt), ("st", st))])

    def refused(rc, word):
        assert rc != 0 and word in hip_lib.last_error(), (rc, hip_lib.last_error())

    refused(call(nb=need - 1), "need")
    refused(call(ws=None), "workspace")
    refused(call(ws=p(ws) + 128), "aligned")
    refused(call(vo=None), "NULL")
    refused(call(fo=None), "NULL")
    refused(call(loops=None), "NULL")
    refused(call(counts=None), "NULL")
    refused(call(limit=2), "max_hole_edges")
    refused(call(limit=65536), "max_hole_edges")
    refused(call(F=-1), "F=-1")
    torch.cuda.synchronize()                                              # nothing ran: the outputs hold what they were filled with
    assert torch.isnan(vo).all() and (fo == -7).all() and (lo == -7).all() and list(cnt) == [-5] * 4
    # the call itself, and nothing written past what it reports
    assert call() == 0, hip_lib.last_error()
    want = H.wanted(fx.name, 300)
    nv, nf, nl, left = list(cnt)
    assert (nv, nf, nl, left) == (len(want.verts), len(want.faces), len(want.closed), want.open_left)
    assert _same_bits(_np(vo[:nv]), want.verts) and np.array_equal(_np(fo[:nf]), want.faces) and np.array_equal(_np(lo[:nl]), want.closed)
    assert torch.isnan(vo[nv:]).all() and (fo[nf:] == -7).all() and (lo[nl:] == -7).all()
    # F = 0 copies the vertices; faces and their outputs may be missing
    cnt0 = (C.c_int64 * 4)(-5, -5, -5, -5)
    assert L.soar_mesh_close_holes_bytes(V, 0, C.byref(n)) == 0
    v0 = torch.full((V, 3), float("nan"), device=dev)
    assert L.soar_mesh_close_holes(V, 0, p(m.vertices), None, 300, p(ws), n.value, p(v0), None, None, cnt0, st) == 0, hip_lib.last_error()
    assert list(cnt0) == [V, 0, 0, 0] and torch.equal(v0, m.vertices)
    # refused at the end of the call: a face that names a vertex twice, one that names a vertex the mesh does not have
    for bad_value in (int(m.faces[5, 0]), V):
        bad = m.faces.clone()
        bad[5, 2] = bad_value
        refused(call(faces=p(bad)), "twice")
        with pytest.raises(hip_lib.SoarHipError, match="twice"):
            mesh.close_holes(mesh.Mesh(m.vertices, bad))


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def _open_capsule_surfels(P, seed, r=0.2, half=0.3, cut=0.42):
    """P surfels on a capsule (radius r, axis 2 half along y) without those above y = cut -- a cap of surfels deleted --: centres,
    rotations whose third axis is the normal, flat scales of r / 10, opacities, colours"""
    from soar_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    on_cyl = rng.random(P) < (2 * half) / (2 * half + 2 * r)
    phi = 2 * np.pi * rng.random(P)
    radial = np.stack([np.cos(phi), np.zeros(P), np.sin(phi)], 1)
    cyl = r * radial + np.stack([np.zeros(P), half * (2 * rng.random(P) - 1), np.zeros(P)], 1)
    z = 2 * rng.random(P) - 1
    d = np.sqrt(np.maximum(0, 1 - z * z))[:, None] * radial + z[:, None] * np.array([0.0, 1.0, 0.0])
    cap = r * d + np.where(z > 0, half, -half)[:, None] * np.array([0.0, 1.0, 0.0])
    pts = np.where(on_cyl[:, None], cyl, cap)
    nrm = torch.from_numpy(np.where(on_cyl[:, None], radial, d)).float()
    ux = torch.nn.functional.normalize(torch.linalg.cross(nrm, torch.from_numpy(rng.standard_normal((P, 3))).float(), dim=-1), dim=-1)
    uy = torch.nn.functional.normalize(torch.linalg.cross(nrm, ux, dim=-1), dim=-1)
    rot = syn.rotmat_to_quat(torch.stack([ux, uy, nrm], dim=-1))
    scales = torch.full((P, 3), 0.1 * r)
    scales[:, 2] = -1e10
    col = torch.from_numpy(rng.random((P, 3))).float()
    keep = torch.from_numpy(pts[:, 1] <= cut)
    return tuple(t[keep].contiguous() for t in (torch.from_numpy(pts).float(), rot, scales, torch.ones(P, 1), col))


EXPORT = dict(resolution=32, n_views=8, image_size=128, decimate_target=None, quality_thresh=0.0016)


def test_export_avatar_closes_what_the_pruning_opened():
    """export_avatar(max_hole_edges=300) is the composition of the public steps with close_holes between the pruning and the
    smoothing; without the argument it is the composition without that step, what it was before it had the argument."""
    from soar_amd import body, mesh
    from soar_amd import synthetic as syn
    dev = _dev()
    surf = tuple(t.to(dev) for t in _open_capsule_surfels(2000, 2))
    means3D, rotations, scales, opacities, colors = surf
    bm = syn.make_body_model(V=1024)
    sv, sw = bm.v_template.to(dev), bm.lbs_weights.to(dev)

    raw = mesh.extract_mesh(means3D, rotations, scales, opacities, resolution=EXPORT["resolution"], n_views=EXPORT["n_views"],
                            image_size=EXPORT["image_size"], decimate_target=None)
    _, q, _ = mesh.vertex_attributes(raw.vertices, means3D, colors, mesh.ATTR_K)
    pruned, _ = mesh.prune_by_quality(raw, q, EXPORT["quality_thresh"])
    # not vacuous: the restatement finds a loop to close on the pruned mesh
    want = H.close_holes(_np(pruned.vertices), _np(pruned.faces), 300)
    print(f"export: raw {tuple(raw.faces.shape)}, pruned {tuple(pruned.faces.shape)}, loops closed {want.closed.tolist()}, "
          f"border edges left {want.open_left}")
    assert len(pruned.faces) < len(raw.faces) and len(want.closed) >= 1 and int(want.closed.max()) <= 300

    def finish(m):
        m = mesh.smooth(m, mesh.SMOOTH_STEPS)
        color, quality, _ = mesh.vertex_attributes(m.vertices, means3D, colors, mesh.ATTR_K)
        return dict(mesh=m, color=color, quality=quality, normals=body.vertex_normals(m.vertices, m.faces),
                    weights=mesh.skin_weights(m, sv, sw, 30))

    def same(got, wanted_):
        assert torch.equal(got["mesh"].vertices, wanted_["mesh"].vertices) and torch.equal(got["mesh"].faces, wanted_["mesh"].faces)
        for key in ("color", "quality", "normals", "weights"):
            assert torch.equal(got[key], wanted_[key]), key

    closed_mesh, closed = mesh.close_holes(pruned, 300)
    assert np.array_equal(_np(closed), want.closed) and np.array_equal(_np(closed_mesh.faces), want.faces)
    assert _same_bits(_np(closed_mesh.vertices), want.verts)
    got = mesh.export_avatar(surf, sv, sw, max_hole_edges=300, **EXPORT)
    assert sorted(got) == ["closed", "color", "mesh", "normals", "quality", "weights"]
    assert closed.numel() >= 1 and torch.equal(got["closed"], closed)
    same(got, finish(closed_mesh))
    V = int(got["mesh"].vertices.shape[0])
    assert got["color"].shape == (V, 3) and got["weights"].shape == (V, 55) and V == len(want.verts)
    assert mesh.open_border_edges(got["mesh"]) == want.open_left < mesh.open_border_edges(pruned)
    # without the argument: no key, and the parent's output
    plain = mesh.export_avatar(surf, sv, sw, **EXPORT)
    assert sorted(plain) == ["color", "mesh", "normals", "quality", "weights"]
    same(plain, finish(pruned))
