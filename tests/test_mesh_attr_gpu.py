"""GPU tests of the mesh attributes (soar_amd/mesh.py: vertex_attributes, adjacency, smooth, prune_by_quality, skin_weights,
pose_mesh, export_avatar; csrc/mesh_attr.hip) against the NumPy float64 restatement tests/mesh_attr_ref.py, whose fixtures
tests/test_mesh_attr_cpu.py checks."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mesh_attr_ref as A

pytestmark = pytest.mark.gpu

FIXTURES = A.fixtures()
KS = (1, 4, 8)


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(fx):
    from soar_amd import mesh
    return mesh.Mesh(torch.from_numpy(fx.verts).to(_dev()), torch.from_numpy(fx.faces).to(_dev()))


@pytest.fixture(scope="module")
def surfels():
    pts, col = A.surfels()
    return pts, col, torch.from_numpy(pts).to(_dev()), torch.from_numpy(col).to(_dev())


@pytest.fixture(scope="module")
def wanted(surfels):
    """the restatement's transfer of every fixture and k, computed once"""
    pts, col = surfels[:2]
    return {(fx.name, k): A.transfer(fx.verts, pts, col, k) for fx in FIXTURES for k in KS}


# ---- attribute transfer ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f.name)
def test_vertex_attributes_match_the_restatement(fx, surfels, wanted):
    from soar_amd import hip_lib, mesh
    pts, col, dpts, dcol = surfels
    v = torch.from_numpy(fx.verts).to(_dev())
    V = len(fx.verts)
    for k in KS:
        idx64, _, q64, d64 = wanted[(fx.name, k)]
        color, quality, idx = mesh.vertex_attributes(v, dpts, dcol, k=k)
        assert color.shape == (V, 3) and quality.shape == (V,) and idx.shape == (V, k) and idx.dtype == torch.int32
        # the gap test of test_mesh_attr_cpu.py makes the order unambiguous in float32
        assert np.array_equal(_np(idx), idx64), (fx.name, k)
        want32 = A.color_float32(col, idx64)
        dc = float(np.abs(_np(color).astype(np.float64) - want32.astype(np.float64)).max())
        dq = float((np.abs(_np(quality).astype(np.float64) - q64) / q64).max())
        print(f"{fx.name} k={k}: max |dcolor| {dc:.3e} (bound {4 * 2.0 ** -24:.3e}), max rel |dquality| {dq:.3e} (bound 1e-6)")
        assert dc <= 4 * 2.0 ** -24
        assert _np(color).min() >= 0.0 and _np(color).max() <= 1.0
        assert (np.abs(_np(quality).astype(np.float64) - q64) <= 1e-6 * q64).all()
        # the K squared distances, through the C call
        L = hip_lib.lib()
        nb = C.c_size_t(0)
        assert L.soar_mesh_attr_transfer_bytes(V, k, C.byref(nb)) == 0 and nb.value >= 4 and nb.value % 256 == 0
        ws = mesh._workspace(nb.value, _dev())
        c2, q2, d2 = torch.empty(V, 3, device=_dev()), torch.empty(V, device=_dev()), torch.empty(V, k, device=_dev())
        rc = L.soar_mesh_attr_transfer(V, len(pts), k, v.data_ptr(), dpts.data_ptr(), dcol.data_ptr(), idx.data_ptr(), ws.data_ptr(), nb.value,
                                       c2.data_ptr(), q2.data_ptr(), d2.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, hip_lib.last_error()
        assert torch.equal(c2, color) and torch.equal(q2, quality) and torch.equal(d2[:, 0], quality)
        assert (np.abs(_np(d2).astype(np.float64) - d64) <= 1e-6 * d64).all()


# ---- adjacency, smoothing --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f.name)
def test_adjacency_equals_the_restatement(fx):
    from soar_amd import mesh
    rs, nbr, border = mesh.adjacency(_mesh(fx))
    wrs, wnbr, wborder = A.adjacency(len(fx.verts), fx.faces)
    assert rs.dtype == torch.int32 and nbr.dtype == torch.int32 and border.dtype == torch.bool
    assert np.array_equal(_np(rs), wrs) and np.array_equal(_np(nbr), wnbr) and np.array_equal(_np(border), wborder)


@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f.name)
def test_smoothing_matches_the_restatement(fx):
    """The bound: a step adds n <= 2 maxdeg float32 terms to P (maxdeg = the most faces at one vertex) and divides once; every
    partial sum is at most (n + 1) max|coordinate|, so the sum is off by at most n (n + 1) 2^-24 max|c|, the quotient by
    (n + 1) 2^-24 max|c| after the division; a step is an average, it does not amplify what the step before left, so the errors
    of the steps add."""
    from soar_amd import mesh
    m = _mesh(fx)
    V = len(fx.verts)
    maxdeg = (A.max_terms(V, fx.faces) + 1) // 2
    for steps in (1, 3):
        got = mesh.smooth(m, steps)
        assert got.faces is m.faces or torch.equal(got.faces, m.faces)
        want = A.smooth(fx.verts, fx.faces, steps)
        bound = steps * (2 * maxdeg + 3) * 2.0 ** -23 * float(np.abs(fx.verts).max())
        diff = float(np.abs(_np(got.vertices).astype(np.float64) - want).max())
        print(f"{fx.name} steps={steps}: max |dv| {diff:.3e} (bound {bound:.3e}, maxdeg {maxdeg})")
        assert got.vertices.dtype == torch.float32 and diff <= bound
        again = mesh.smooth(m, steps)
        assert torch.equal(again.vertices, got.vertices)                 # bit for bit
        assert torch.equal(m.vertices, torch.from_numpy(fx.verts).to(_dev()))   # the input is not written
    assert torch.equal(mesh.smooth(m, 0).vertices, m.vertices)


def test_one_step_on_the_icosahedron_is_the_closed_form():
    from soar_amd import mesh
    v, f = A.icosahedron()
    m = mesh.Mesh(torch.from_numpy(v.astype(np.float32)).to(_dev()), torch.from_numpy(f).to(_dev()))
    got = _np(mesh.smooth(m, 1).vertices).astype(np.float64)
    s = (1.0 + 2.0 * math.sqrt(5.0)) / 11.0
    assert np.abs(got - s * v.astype(np.float32).astype(np.float64)).max() <= 13 * 2.0 ** -23


# ---- pruning ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fx", FIXTURES, ids=lambda f: f.name)
def test_pruning_equals_the_restatement(fx, wanted):
    from soar_amd import mesh
    m = _mesh(fx)
    q = wanted[(fx.name, 4)][2].astype(np.float32)
    for thresh in (float(np.median(q)), float(q.max()), float("inf"), -1.0, float(q.min())):
        got, keep = mesh.prune_by_quality(m, torch.from_numpy(q).to(_dev()), thresh)
        wv, wf, wkeep = A.prune(fx.verts, fx.faces, q, np.float32(thresh))
        assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32 and keep.dtype == torch.int32
        assert got.faces.shape == (len(wf), 3)
        assert np.array_equal(_np(got.vertices), wv) and np.array_equal(_np(got.faces), wf) and np.array_equal(_np(keep), wkeep)
    got, keep = mesh.prune_by_quality(m, torch.from_numpy(q).to(_dev()), float("inf"))           # nothing pruned
    assert torch.equal(got.vertices, m.vertices) and torch.equal(got.faces, m.faces) and keep.tolist() == list(range(len(q)))
    got, keep = mesh.prune_by_quality(m, torch.from_numpy(q).to(_dev()), -1.0)                   # everything pruned
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3) and keep.shape == (0,)


# ---- the rig ---------------------------------------------------------------------------------------------------------------------

def test_skin_weights_and_pose_mesh():
    from soar_amd import hip_lib, lbs, mesh
    from soar_amd import synthetic as syn
    dev = _dev()
    bm = syn.make_body_model(V=2048)
    sv, sw = bm.v_template.to(dev), bm.lbs_weights.to(dev).contiguous()
    fx = FIXTURES[0]                                                       # the icosphere: every vertex has faces
    m = _mesh(fx)
    V, J, K = len(fx.verts), sw.shape[1], 30
    w = mesh.skin_weights(m, sv, sw, K=K)
    assert w.shape == (V, J) and w.dtype == torch.float32
    # soar_lbs_knn_weights itself on the same points
    L = hip_lib.lib()
    nb = C.c_size_t(0)
    assert L.soar_lbs_knn_weights_bytes(V, sv.shape[0], C.byref(nb)) == 0
    ws = mesh._workspace(nb.value, dev)
    direct = torch.empty(V, J, device=dev)
    assert L.soar_lbs_knn_weights(m.vertices.data_ptr(), V, sv.data_ptr(), sv.shape[0], sw.data_ptr(), J, K, direct.data_ptr(), None,
                                  ws.data_ptr(), nb.value, torch.cuda.current_stream().cuda_stream) == 0, hip_lib.last_error()
    assert torch.equal(w, direct)

    gen = torch.Generator().manual_seed(5)
    B = 3
    mats = torch.eye(4).repeat(B, J, 1, 1)
    mats[:, :, :3, :] += 0.05 * torch.randn(B, J, 3, 4, generator=gen)
    mats = mats.to(dev)
    pv, pn = mesh.pose_mesh(m, w, mats)
    assert pv.shape == (B, V, 3) and pn.shape == (B, V, 3)
    rot = torch.zeros(V, 4, device=dev)
    rot[:, 0] = 1.0
    for b in range(B):
        want, _ = lbs.lbs_warp(m.vertices, rot, w, mats[b])
        assert torch.equal(pv[b], want), b
    assert float((pn.norm(dim=-1) - 1.0).abs().max()) <= 1e-5
    # the identity pose.  The blended matrix has exact zeros off its diagonal and in its translation, and on the diagonal
    # s = the float32 sum of the J weights: J exact products w_j * 1 and J - 1 adds of partial sums of about 1, so
    # |s - sum_j w_j| <= (J - 1) 2^-24 (1 + small).  Then x' = s x + 0 + 0 + 0 rounds once more: |x' - x| <=
    # (|sum_j w_j - 1| + J 2^-24 (1 + small)) |x|; J + 4 for J (1 + small).  sum_j w_j is taken in float64 from the weights.
    iv, inrm = mesh.pose_mesh(m, w, torch.eye(4, device=dev).repeat(1, J, 1, 1))
    wsum = w.double().sum(1)
    bound = ((wsum - 1.0).abs().max().item() + (J + 4) * 2.0 ** -24) * float(np.abs(fx.verts).max())
    diff = float((iv[0].double() - m.vertices.double()).abs().max())
    print(f"identity pose: max |dv| {diff:.3e} (bound {bound:.3e})")
    assert diff <= bound
    from soar_amd import body
    assert torch.equal(inrm[0], body.vertex_normals(iv[0], m.faces))


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_the_c_abi_refuses_bad_arguments_before_any_launch():
    from soar_amd import hip_lib, mesh
    L = hip_lib.lib()
    dev = _dev()
    st = torch.cuda.current_stream().cuda_stream
    fx = FIXTURES[1]
    m = _mesh(fx)
    V, F, N, k = len(fx.verts), len(fx.faces), A.N_SURFELS, 4
    nan = float("nan")
    fill = {torch.float32: nan, torch.int32: -7, torch.uint8: 249}
    buf = lambda *s, dt=torch.float32: torch.full(s, fill[dt], dtype=dt, device=dev)
    pts, col = torch.rand(N, 3, device=dev), torch.rand(N, 3, device=dev)
    idx = torch.zeros(V, k, dtype=torch.int32, device=dev)
    co, qo = buf(V, 3), buf(V)
    ws = mesh._workspace(1 << 20, dev)
    p = lambda t: t.data_ptr()
    n = C.c_size_t(0)

    def refused(rc, word):
        assert rc != 0 and word in hip_lib.last_error(), (rc, hip_lib.last_error())

    # sizes
    refused(L.soar_mesh_attr_transfer_bytes(V, 0, C.byref(n)), "K")
    refused(L.soar_mesh_attr_transfer_bytes(V, 9, C.byref(n)), "K")
    refused(L.soar_mesh_attr_transfer_bytes(V, 4, None), "soar_mesh_attr_transfer_bytes")
    refused(L.soar_mesh_adjacency_bytes(0, F, C.byref(n)), "V")
    refused(L.soar_mesh_adjacency_bytes(V, -1, C.byref(n)), "F")
    refused(L.soar_mesh_smooth_bytes(0, C.byref(n)), "V")
    refused(L.soar_mesh_prune_bytes(V, F, None), "NULL")
    # transfer
    t = lambda **kw: L.soar_mesh_attr_transfer(*[kw.get(a, d) for a, d in (
        ("V", V), ("N", N), ("K", k), ("verts", p(m.vertices)), ("points", p(pts)), ("colors", p(col)), ("idx", p(idx)), ("ws", p(ws)),
        ("nb", 256), ("color", p(co)), ("quality", p(qo)), ("d2", None), ("st", st))])
    refused(t(K=0), "K=0")
    refused(t(K=9), "K=9")
    refused(t(verts=None), "NULL")
    refused(t(idx=None), "NULL")
    refused(t(quality=None), "NULL")
    refused(t(ws=None), "workspace")
    refused(t(ws=p(ws) + 64), "aligned")
    refused(t(nb=128), "need 256")
    # adjacency
    rs, nb_, bd = buf(V + 1, dt=torch.int32), buf(6 * F, dt=torch.int32), buf(V, dt=torch.uint8)
    assert L.soar_mesh_adjacency_bytes(V, F, C.byref(n)) == 0
    need = n.value
    a = lambda **kw: L.soar_mesh_adjacency(*[kw.get(k_, d) for k_, d in (
        ("V", V), ("F", F), ("faces", p(m.faces)), ("ws", p(ws)), ("nb", need), ("rs", p(rs)), ("nbr", p(nb_)), ("border", p(bd)), ("st", st))])
    refused(a(faces=None), "NULL")
    refused(a(border=None), "NULL")
    refused(a(ws=None), "workspace")
    refused(a(ws=p(ws) + 128), "aligned")
    refused(a(nb=need - 1), "need")
    refused(a(V=0), "V=0")
    # smoothing
    rs_ok, nbr_ok, bd_ok = mesh.adjacency(m)
    bd_ok = bd_ok.to(torch.uint8)
    vo = buf(V, 3)
    assert L.soar_mesh_smooth_bytes(V, C.byref(n)) == 0
    need = n.value
    s = lambda **kw: L.soar_mesh_smooth(*[kw.get(k_, d) for k_, d in (
        ("V", V), ("nnz", 6 * F), ("verts", p(m.vertices)), ("rs", p(rs_ok)), ("nbr", p(nbr_ok)), ("border", p(bd_ok)), ("steps", 3),
        ("ws", p(ws)), ("nb", need), ("out", p(vo)), ("st", st))])
    refused(s(verts=None), "NULL")
    refused(s(nbr=None), "NULL")
    refused(s(out=p(m.vertices)), "verts_out")
    refused(s(steps=-1), "steps")
    refused(s(ws=None), "workspace")
    refused(s(ws=p(ws) + 4), "aligned")
    refused(s(nb=need - 1), "need")
    # pruning
    q = torch.rand(V, device=dev)
    po, fo, ko = buf(V, 3), buf(F, 3, dt=torch.int32), buf(V, dt=torch.int32)
    cnt = (C.c_int64 * 2)(-5, -5)
    assert L.soar_mesh_prune_bytes(V, F, C.byref(n)) == 0
    need = n.value
    r = lambda **kw: L.soar_mesh_prune(*[kw.get(k_, d) for k_, d in (
        ("V", V), ("F", F), ("verts", p(m.vertices)), ("faces", p(m.faces)), ("q", p(q)), ("thresh", 0.5), ("ws", p(ws)), ("nb", need),
        ("vo", p(po)), ("fo", p(fo)), ("keep", p(ko)), ("counts", cnt), ("st", st))])
    refused(r(q=None), "NULL")
    refused(r(faces=None), "NULL")
    refused(r(counts=None), "NULL")
    refused(r(thresh=nan), "threshold")
    refused(r(ws=None), "workspace")
    refused(r(ws=p(ws) + 32), "aligned")
    refused(r(nb=need - 1), "need")
    # nothing ran: every output still holds what it was filled with
    torch.cuda.synchronize()
    for o in (co, qo, vo, po):
        assert torch.isnan(o).all()
    for o in (rs, nb_, fo, ko):
        assert (o == -7).all()
    assert (bd == 249).all() and cnt[0] == -5 and cnt[1] == -5
    # refused after the first launch: an index the points do not have, a face naming a vertex twice
    idx[3, 1] = N
    refused(t(), "outside")
    bad = m.faces.clone()
    bad[5, 2] = bad[5, 0]
    refused(a(faces=p(bad), nb=1 << 20), "twice")


# ---- end to end ------------------------------------------------------------------------------------------------------------------

def _capsule_surfels(P, seed, r=0.2, half=0.3):
    """P surfels on a capsule (radius r, axis 2 half along y): centres, rotations whose third axis is the normal, flat scales of
    r / 10"""
    from soar_amd import synthetic as syn
    rng = np.random.default_rng(seed)
    on_cyl = rng.random(P) < (2 * half) / (2 * half + 2 * r)              # area of the cylinder over the whole area
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
    return torch.from_numpy(pts).float(), rot, scales, torch.ones(P, 1), col


def test_export_avatar_end_to_end(tmp_path):
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    dev = _dev()
    surf = tuple(t.to(dev).contiguous() for t in _capsule_surfels(2000, 2))
    bm = syn.make_body_model(V=1024)

    def run(tag):
        out = mesh.export_avatar(surf, bm.v_template.to(dev), bm.lbs_weights.to(dev), resolution=48, n_views=8, image_size=128,
                                 quality_thresh=0.01)
        paths = [str(tmp_path / f"{tag}.{ext}") for ext in ("obj", "ply", "npz")]
        mesh.save_obj(paths[0], out["mesh"], out["color"])
        mesh.save_ply(paths[1], out["mesh"], out["color"], out["normals"], out["quality"])
        mesh.save_skinned(paths[2], out["mesh"], out["weights"], out["color"])
        return out, paths

    out, paths = run("a")
    m = out["mesh"]
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    print(f"export_avatar: V {V} F {F}, quality max {float(out['quality'].max()):.3e}")
    assert V > 100 and F > 100 and sorted(out) == ["color", "mesh", "normals", "quality", "weights"]
    assert out["color"].shape == (V, 3) and out["quality"].shape == (V,) and out["normals"].shape == (V, 3)
    assert out["weights"].shape == (V, 55)
    assert float(out["color"].min()) >= 0.0 and float(out["color"].max()) <= 1.0
    assert float((out["weights"].sum(1) - 1.0).abs().max()) <= 1e-5          # 30 + 55 float32 roundings of numbers below 1
    # the surface is the capsule's, within the 4 voxels the extractor's own test allows its worst vertex (tests/test_mesh_gpu.py)
    _, voxel, _ = mesh.export_grid(surf[0], surf[2], 48)
    p = m.vertices.double().cpu()
    axis = p.clone()
    axis[:, 0], axis[:, 2] = 0.0, 0.0
    axis[:, 1] = axis[:, 1].clamp(-0.3, 0.3)
    assert float(((p - axis).norm(dim=1) - 0.2).abs().max()) <= 4.0 * voxel
    v, f = A.parse_obj(paths[0])
    assert v.shape == (V, 6) and np.array_equal(f, _np(m.faces)) and np.array_equal(v[:, :3].astype(np.float32), _np(m.vertices))
    assert v[:, 3:].min() >= 0.0 and v[:, 3:].max() <= 1.0
    props, fp = A.parse_ply(paths[1])
    assert list(props) == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "quality"]
    assert np.array_equal(fp, _np(m.faces)) and np.array_equal(props["quality"], _np(out["quality"]))
    z = np.load(paths[2])
    assert z["vertices"].shape == (V, 3) and z["faces"].shape == (F, 3) and z["weights"].shape == (V, 55) and z["colors"].shape == (V, 3)
    # posing the exported asset
    pv, pn = mesh.pose_mesh(m, out["weights"], torch.eye(4, device=dev).repeat(2, 55, 1, 1))
    assert pv.shape == (2, V, 3) and float((pv[0] - m.vertices).abs().max()) <= 1e-5
    _, again = run("b")
    for x, y in zip(paths, again):
        assert open(x, "rb").read() == open(y, "rb").read(), x


# ---- export_avatar on the project's own model -------------------------------------------------------------------------------------

def _capsule_model(P, seed):
    """A GaussianSurfelModel on a capsule of radius 0.1 (the attribute field's scales are sigmoid * 0.02, about 0.01: r / 10 as in
    the tensor test), oriented and opaque, its field's hash tables filled so that colours and scales differ from surfel to surfel,
    and explicit leaves (scale 0.013, the capsule's random colours) that differ from what the field gives."""
    from soar_amd.geometry import GaussianSurfelModel
    dev = _dev()
    pts, rot, _, _, col = _capsule_surfels(P, seed, r=0.1, half=0.15)
    torch.manual_seed(seed)                                                # the field's initial MLP weights
    model = GaussianSurfelModel({})
    model.create_from_pcd(pts, col.clamp(0.02, 0.98), 10)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        model._rotation.copy_(rot.to(dev))
        model._scaling.fill_(math.log(0.013))
        model._opacity.fill_(6.0)
        for enc in (model.attribute_field.encoding, model.attribute_field.quat_encoding):
            enc.hash_table.copy_((torch.rand(enc.hash_table.shape, generator=gen) * 2 - 1).to(dev))
    model.invalidate()
    return model


def test_export_avatar_reads_a_model_as_its_renderer_does():
    """use_explicit false (every SOAR configuration): scales and colours are the attribute field's at the surfel centres, the
    [P,1] scale repeated to three columns with the third at -1e10.  The model path must give, bit for bit, what the tensor path
    gives on the tensors built by that recipe -- and not what the explicit leaves would give."""
    import types

    from soar_amd import mesh
    from soar_amd import synthetic as syn
    dev = _dev()
    model = _capsule_model(2000, 3)
    bm = syn.make_body_model(V=1024)
    sv, sw = bm.v_template.to(dev), bm.lbs_weights.to(dev)
    kw = dict(resolution=48, n_views=8, image_size=128, quality_thresh=0.0025)
    P = model.num_points
    assert model.get_scaling.shape == (P, 1)
    with torch.no_grad():
        fields = model.attribute_field(model.get_xyz.detach())
    fscale, fcol = fields["scales"].detach(), fields["shs"].detach()
    assert fscale.shape == (P, 1) and fcol.shape == (P, 3)
    assert float((fcol - model.get_colors.detach()).abs().max()) > 0.1                      # the two sources differ
    scales = fscale.repeat(1, 3)
    scales[:, 2] = -1e10
    recipe = (model.get_xyz.detach(), model.get_rotation.detach(), scales, model.get_opacity.detach(), fcol)

    got = mesh.export_avatar(model, sv, sw, **kw)
    want = mesh.export_avatar(recipe, sv, sw, **kw)
    V, F = int(got["mesh"].vertices.shape[0]), int(got["mesh"].faces.shape[0])
    print(f"export_avatar(model): V {V} F {F}, field scales {float(fscale.min()):.4f}..{float(fscale.max()):.4f}")
    assert V > 100 and F > 100
    assert torch.equal(got["mesh"].vertices, want["mesh"].vertices) and torch.equal(got["mesh"].faces, want["mesh"].faces)
    for key in ("color", "quality", "normals", "weights"):
        assert torch.equal(got[key], want[key]), key
    # the colours are means of 4 field colours, so inside the field colours' range per channel
    assert (got["color"] >= fcol.min(0).values).all() and (got["color"] <= fcol.max(0).values).all()
    # the tensors of both switches, as the renderer builds them
    t = mesh._surfel_tensors(model, False)
    assert all(torch.equal(a, b) for a, b in zip(t, recipe))
    e = mesh._surfel_tensors(model, True)
    escales = model.get_scaling.detach().repeat(1, 3)
    escales[:, 2] = -1e10
    assert e[2].shape == (P, 3) and torch.equal(e[2], escales) and torch.equal(e[4], model.get_colors)
    assert torch.equal(e[0], recipe[0]) and torch.equal(e[1], recipe[1]) and torch.equal(e[3], recipe[3])

    # refused before anything is launched: a scale that is not [P,1] in a model, not [P,3] in tensors; no field to ask
    leaves = dict(get_xyz=recipe[0], get_rotation=recipe[1], get_opacity=recipe[3], get_colors=fcol, attribute_field=None)
    with pytest.raises(ValueError, match=r"\[2000,1\]"):
        mesh.export_avatar(types.SimpleNamespace(get_scaling=fscale.repeat(1, 2), **leaves), sv, sw, use_explicit=True, **kw)
    with pytest.raises(ValueError, match="attribute_field"):
        mesh.export_avatar(types.SimpleNamespace(get_scaling=fscale, **leaves), sv, sw, **kw)
    for bad in (fscale, fscale.repeat(1, 2), scales[:-1]):
        with pytest.raises(ValueError, match="scales must be"):
            mesh.export_avatar(recipe[:2] + (bad,) + recipe[3:], sv, sw, **kw)
    with pytest.raises(ValueError, match="rotations must be"):
        mesh.export_avatar((recipe[0], recipe[1][:, :3]) + recipe[2:], sv, sw, **kw)
