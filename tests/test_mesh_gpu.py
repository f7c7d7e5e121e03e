"""GPU tests of the mesh export (soar_amd/mesh.py, csrc/mesh.hip): TSDF fusion against a float64 restatement, the depth
convention of the renderer, marching cubes against the Python table driver, analytic fields, the whole path on the bench's
person and the component filter; from section 8 on, the three stages off the cube, at their block edges, ties and thresholds, on
the cases of tests/mesh_cases.py."""
import functools
import math

import numpy as np
import pytest
import torch

import mesh_cases as MC
import mesh_ref as R

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. fusion ----------------------------------------------------------------------------------------------------------

def test_fuse_depth_matches_float64_restatement():
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    H, W, n = 60, 80, 6
    fovx, fovy = math.radians(55.0), 2 * math.atan(math.tan(math.radians(55.0) / 2) * H / W)
    views, projs, prcps = [], [], []
    for k in range(n):
        el, az = float(torch.rand(1, generator=gen)) * 2 - 1, float(torch.rand(1, generator=gen)) * 6.28
        wv, full, _ = syn.camera_from_c2w(syn.make_c2w(3.0, el, az, target=(0.0, 0.0, 0.0)), fovx, fovy, znear=0.2)
        views.append(wv)
        projs.append(full)
        prcps.append(0.4 + 0.2 * torch.rand(2, generator=gen))
    viewm, projm, prcp = torch.stack(views), torch.stack(projs), torch.stack(prcps)
    depth = 2.4 + 1.2 * torch.rand(n, H, W, generator=gen)
    opac = torch.where(torch.rand(n, H, W, generator=gen) < 0.3, 0.1, 0.9)
    origin, voxel, dims = (-1.0, -1.0, -1.0), 2.0 / 63, (64, 64, 64)
    trunc = 3 * voxel
    acc = mesh.fuse_depth(depth[:3].to(dev), opac[:3].to(dev), viewm[:3].to(dev), projm[:3].to(dev), prcp[:3].to(dev), origin, voxel, dims)
    s, w = mesh.fuse_depth(depth[3:].to(dev), opac[3:].to(dev), viewm[3:].to(dev), projm[3:].to(dev), prcp[3:].to(dev), origin, voxel,
                           dims, acc=acc)
    assert s.data_ptr() == acc[0].data_ptr()                      # accumulated in place
    rs, rw, amb = R.tsdf_reference(depth, opac, viewm, projm, prcp, origin, voxel, dims, trunc)
    s, w = s.cpu().double(), w.cpu().double()
    ok = ~amb
    assert amb.float().mean() < 0.05                             # ~ 6 views x 2 axes x 2e-3 px of 1 px
    assert torch.equal(w[ok], rw[ok])
    assert (s[ok] - rs[ok]).abs().max() <= 1e-5
    assert (rw > 0).float().mean() > 0.5 and ((rs / rw.clamp_min(1)).abs() < 1).any()   # the test sees observed band voxels


# ---- 2. depth convention ------------------------------------------------------------------------------------------------

def test_rendered_depth_is_view_space_z_and_fusion_puts_the_wall_there():
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    from soar_amd.rasterizer import GaussianRasterizationSettings, rasterize_views
    dev = _dev()
    S, fov, zw = 128, math.radians(60.0), 2.0
    wv, full, center = syn.camera_from_c2w(torch.eye(4), fov, fov, znear=0.2)     # at the origin, looking along -z
    xs = torch.arange(-1.3, 1.3001, 0.01)
    gx, gy = torch.meshgrid(xs, xs, indexing="ij")
    P = gx.numel()
    means = torch.stack([gx.reshape(-1), gy.reshape(-1), torch.full((P,), -zw)], 1)
    rot = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(P, 1)
    scales = torch.tensor([0.01, 0.01, -1e10]).repeat(P, 1)
    st = GaussianRasterizationSettings(S, S, math.tan(fov / 2), math.tan(fov / 2), torch.zeros(3, device=dev), 1.0, wv.to(dev), full.to(dev),
                                       torch.tensor([0.0, 0.0, S, S], device=dev), torch.tensor([0.5, 0.5], device=dev), 0, center.to(dev),
                                       False, False, False, False, torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev))
    t = lambda a: a.to(dev).contiguous()
    with torch.no_grad():
        out = rasterize_views([st], [dict(means3D=t(means), means2D=torch.zeros(P, 3, device=dev), opacities=torch.ones(P, 1, device=dev),
                                          colors_precomp=torch.zeros(P, 3, device=dev), scales=t(scales), rotations=t(rot))])[0]
    depth, opac = out[2].reshape(S, S), out[3].reshape(S, S)
    assert (opac[16:-16, 16:-16] > 0.99).all()
    assert (depth[16:-16, 16:-16] - zw).abs().max() <= 1e-4
    voxel = 0.01
    origin, dims = (-0.2, -0.2, -zw - 0.3 + 0.0037), (40, 40, 60)
    s, w = mesh.fuse_depth(depth[None], opac[None], wv[None].to(dev), full[None].to(dev), torch.tensor([[0.5, 0.5]], device=dev),
                           origin, voxel, dims)
    valid = w > 0
    field = torch.where(valid, s / w.clamp_min(1), torch.ones_like(s))
    verts, faces = mesh.marching_cubes(field, 0.0, valid)
    assert len(faces) > 1000
    zworld = verts[:, 2].double() * voxel + origin[2]
    assert ((zworld + zw).abs() / voxel).max() <= 0.05


# ---- 3. marching cubes against the table driver -------------------------------------------------------------------------

def _gpu_mc(f, valid=None, level=0.0):
    from soar_amd import mesh
    v, fc = mesh.marching_cubes(torch.as_tensor(f).to(_dev()), level, None if valid is None else torch.as_tensor(valid).to(_dev()))
    return _np(v), _np(fc)


def test_marching_cubes_equals_the_table_driver_on_every_case():
    for case in range(256):
        cube = np.zeros((2, 2, 2), np.float32)
        for c in range(8):
            cube[c & 1, (c >> 1) & 1, (c >> 2) & 1] = (-1.0 if (case >> c) & 1 else 1.0) * (1.0 + 0.1 * c)
        for f in (cube, np.pad(cube, 1, constant_values=1.0)):
            v, fc = _gpu_mc(f)
            rv, rf = R.marching_cubes(f)
            assert np.array_equal(v, rv) and np.array_equal(fc, rf), case


@pytest.mark.parametrize("seed", range(4))
def test_marching_cubes_equals_the_table_driver_on_random_fields(seed):
    rng = np.random.default_rng(100 + seed)
    f = rng.standard_normal((24, 24, 24)).astype(np.float32)
    valid = rng.uniform(size=f.shape) > 0.1 if seed == 3 else None
    level = 0.25 if seed == 2 else 0.0
    v, fc = _gpu_mc(f, valid, level)
    rv, rf = R.marching_cubes(f, level, valid)
    assert np.array_equal(v, rv) and np.array_equal(fc, rf)
    R.check_vertices_on_crossings(v, f, level, valid)
    if valid is None:
        R.check_closed_manifold(v, fc, f.shape)
    v2, fc2 = _gpu_mc(f, valid, level)
    assert np.array_equal(v, v2) and np.array_equal(fc, fc2)


# ---- 4. analytic fields -------------------------------------------------------------------------------------------------

def _grid(n):
    a = torch.arange(n, dtype=torch.float64)
    return torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1)


def test_sphere_and_torus():
    g = _grid(64)
    c, r = torch.tensor([31.7, 32.1, 31.4], dtype=torch.float64), 20.0
    f = ((g - c).norm(dim=-1) - r).float()
    v, fc = _gpu_mc(f)
    R.check_closed_fast(fc, len(v))
    assert R.euler_characteristic(v, fc) == 2
    d = np.linalg.norm(v.astype(np.float64) - c.numpy(), axis=1) - r
    assert np.abs(d).max() <= 0.05
    vol, exact = R.enclosed_volume(v, fc), 4.0 / 3.0 * math.pi * r ** 3
    assert vol > 0 and abs(vol - exact) <= 0.01 * exact
    # torus around z: R = 18, r = 7
    q = g - c
    ft = (torch.sqrt((torch.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - 18.0) ** 2 + q[..., 2] ** 2) - 7.0).float()
    v, fc = _gpu_mc(ft)
    R.check_closed_fast(fc, len(v))
    assert R.euler_characteristic(v, fc) == 0
    assert R.enclosed_volume(v, fc) > 0


# ---- 5. the whole path on the bench's person ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def person():
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    s = syn.make_surfels(100_000)
    dev = _dev()
    args = [t.to(dev) for t in (s.xyz, s.rot, s.scales, s.opacity)]
    m = mesh.extract_mesh(*args, resolution=256)
    _, voxel, _ = mesh.export_grid(args[0], args[2], 256)
    return s, args, m, voxel


def test_extract_mesh_of_the_person(person):
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    s, args, m, voxel = person
    V, F = m.vertices.shape[0], m.faces.shape[0]
    assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and F > 10000
    sdf = R.capsule_sdf(m.vertices.double(), syn._CAPSULES).abs() / voxel
    assert (sdf <= 1.5).float().mean() >= 0.99, float((sdf <= 1.5).float().mean())
    assert sdf.max() <= 4.0, float(sdf.max())
    pts, _ = syn.sample_capsule_surface(40_000, torch.Generator().manual_seed(5))
    pts = pts.double().to(m.vertices.device)
    ext = pts[R.capsule_sdf(pts, syn._CAPSULES) >= -1e-6][:20_000]
    assert len(ext) == 20_000
    near = torch.cat([torch.cdist(ext[i:i + 2000].float(), m.vertices).min(1).values for i in range(0, len(ext), 2000)])
    assert (near <= 2 * voxel).float().mean() >= 0.99, float((near <= 2 * voxel).float().mean())
    assert R.n_components_torch(V, m.faces) == 1
    fc = _np(m.faces)
    R.check_closed_fast(fc, V)
    assert R.euler_characteristic(_np(m.vertices), fc) == 2
    assert len(np.unique(fc)) == V                               # no unused vertex left
    again = mesh.extract_mesh(*args, resolution=256)
    assert torch.equal(again.vertices, m.vertices) and torch.equal(again.faces, m.faces)


# ---- 6. the component filter --------------------------------------------------------------------------------------------

def _clusters(n, gen, keep_away, capsules, lo, hi):
    """n tiny discs of 24 surfels (radius 1 cm) at random places inside [lo, hi], at least `keep_away` from the capsules"""
    from soar_amd import synthetic as syn
    centres = []
    while len(centres) < n:
        c = lo + (hi - lo) * torch.rand(3, generator=gen)
        if float(R.capsule_sdf(c[None].double(), capsules)) >= keep_away:
            centres.append(c)
    xyz, rot = [], []
    for c in centres:
        nrm = torch.nn.functional.normalize(torch.randn(3, generator=gen), dim=0)
        u = torch.nn.functional.normalize(torch.linalg.cross(nrm, torch.randn(3, generator=gen)), dim=0)
        v = torch.linalg.cross(nrm, u)
        a = torch.rand(24, generator=gen) * 6.2832
        rr = 0.01 * torch.sqrt(torch.rand(24, generator=gen))
        xyz.append(c + rr[:, None] * (torch.cos(a)[:, None] * u + torch.sin(a)[:, None] * v))
        rot.append(syn.rotmat_to_quat(torch.stack([u, v, nrm], -1))[None].repeat(24, 1))
    return torch.cat(xyz), torch.cat(rot)


def test_component_filter_removes_small_clusters(person):
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    s, args, m, voxel = person
    dev = _dev()
    gen = torch.Generator().manual_seed(21)
    lo, hi = s.xyz.min(0).values + 0.02, s.xyz.max(0).values - 0.02
    cx, cr = _clusters(50, gen, 0.1, syn._CAPSULES, lo, hi)       # inside the person's box: the grid stays the same
    P = cx.shape[0]
    xyz = torch.cat([s.xyz, cx]).to(dev)
    rot = torch.cat([s.rot, cr]).to(dev)
    scales = torch.cat([s.scales, torch.tensor([0.004, 0.004, -1e10]).repeat(P, 1)]).to(dev)
    opac = torch.ones(xyz.shape[0], 1, device=dev)
    assert mesh.export_grid(xyz, scales, 256) == mesh.export_grid(args[0], args[2], 256)
    with_clusters = mesh.extract_mesh(xyz, rot, scales, opac, resolution=256)
    assert R.n_components_torch(with_clusters.vertices.shape[0], with_clusters.faces) == 1
    d = torch.cdist(cx.to(dev), with_clusters.vertices).min(1).values
    assert (d > 0.05).all()                                      # nothing is left near a cluster
    # the filter alone, bit for bit: the person's mesh with 50 tiny far-away meshes interleaved comes back unchanged
    g = _grid(6)
    blob_v, blob_f = _gpu_mc(((g - 2.5).norm(dim=-1) - 1.6).float())
    assert 0 < len(blob_f) < 64
    V = m.vertices.shape[0]
    pieces_v, pieces_f, base = [], [], 0
    cuts = sorted(torch.randint(0, V, (50,), generator=gen).tolist())
    starts = [0] + cuts
    ends = cuts + [V]
    far = m.vertices.max(0).values + 1.0
    remap = torch.empty(V, dtype=torch.long)
    for i, (a, b) in enumerate(zip(starts, ends)):
        pieces_v.append(m.vertices[a:b])
        remap[a:b] = torch.arange(base, base + b - a)
        base += b - a
        if i < 50:
            off = far + torch.tensor([0.05 * (i % 10), 0.05 * (i // 10), 0.0], device=dev)
            pieces_v.append(torch.as_tensor(blob_v, device=dev) * 0.005 + off)
            pieces_f.append(torch.as_tensor(blob_f, device=dev).long() + base)
            base += len(blob_v)
    big_v = torch.cat(pieces_v)
    person_f = remap.to(dev)[m.faces.long()]
    order = torch.randperm(len(person_f) + sum(len(p) for p in pieces_f), generator=gen)
    all_f = torch.cat([person_f] + pieces_f)[order.to(dev)].int()
    # faces in a shuffled order: the filter keeps the input order, so the person's faces come back in that order
    fv, ff = mesh.filter_components(big_v, all_f)
    keep = order < len(person_f)
    expect_f = m.faces[order[keep].to(dev)]
    assert torch.equal(fv, m.vertices)
    assert torch.equal(ff, expect_f)
    # a component is kept only when it has >= 64 faces AND a diagonal >= 20 % of the whole mesh's
    fv2, ff2 = mesh.filter_components(big_v, all_f, min_faces=1, min_diag_frac=0.0)
    assert len(fv2) == len(big_v) and len(ff2) == len(all_f)


# ---- 7. the component filter at small sizes -----------------------------------------------------------------------------

def _small_filter_mesh(levels, strays, seed):
    """an icosphere of radius 1, a far-away icosahedron of radius 0.005 and `strays` vertices that no face uses; the vertices
    interleaved and the faces shuffled by a seeded permutation -> (verts, faces, which input vertices / faces are the sphere's)"""
    import mesh_attr_ref as A
    sv, sf = A.icosphere(levels)
    iv, jf = A.icosahedron()
    rng = np.random.default_rng(seed)
    v = np.concatenate([sv, 0.005 * iv + 1.5, rng.uniform(-1.0, 1.0, (strays, 3))]).astype(np.float32)
    f = np.concatenate([sf, jf + len(sv)])
    where = rng.permutation(len(v))                     # vertex i goes to row where[i]
    order = rng.permutation(len(f))
    verts = np.empty_like(v)
    verts[where] = v
    faces = where[f][order].astype(np.int32)
    sphere_v = np.zeros(len(v), bool)
    sphere_v[where[:len(sv)]] = True
    return verts, faces, sphere_v, order < len(sf)


# (levels, strays): V = 324 < F = 340 and V = 354 > F = 100; the write kernel runs one grid over max(V, F), two blocks either way
@pytest.mark.parametrize("levels,strays,V,F", [(2, 150, 324, 340), (1, 300, 354, 100)])
def test_component_filter_at_small_sizes(levels, strays, V, F):
    from soar_amd import hip_lib, mesh
    dev = _dev()
    verts, faces, sphere_v, sphere_f = _small_filter_mesh(levels, strays, 40 + levels)
    assert verts.shape == (V, 3) and faces.shape == (F, 3)
    used = np.zeros(V, bool)
    used[faces.reshape(-1)] = True
    # the icosahedron's diagonal is a factor 59 below the threshold of 20 % and the sphere's a factor 4 above it: float32 or
    # float64 diagonals decide alike
    for kw, keep_v, keep_f in ((dict(), sphere_v, sphere_f), (dict(min_faces=1, min_diag_frac=0.0), used, np.ones(F, bool))):
        want_v, want_f = R.filter_components(verts, faces, kw.get("min_faces", mesh.MIN_FACES), kw.get("min_diag_frac", mesh.MIN_DIAG_FRAC))
        assert np.array_equal(want_v, verts[keep_v]) and len(want_f) == int(keep_f.sum())     # the restatement keeps what it should
        got_v, got_f = mesh.filter_components(torch.from_numpy(verts).to(dev), torch.from_numpy(faces).to(dev), **kw)
        assert got_v.dtype == torch.float32 and got_f.dtype == torch.int32
        assert np.array_equal(_np(got_v), want_v) and np.array_equal(_np(got_f), want_f)
    bad = faces.copy()
    bad[F // 2, 1] = V
    with pytest.raises(hip_lib.SoarHipError, match="outside"):
        mesh.filter_components(torch.from_numpy(verts).to(dev), torch.from_numpy(bad).to(dev))


# ---- 8. fusion off the cube (tests/mesh_cases.py; tests/test_mesh_cases_cpu.py checks the cases themselves) -----------------------

def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def _fuse(case, views=slice(None), acc=None):
    from soar_amd import mesh
    t = lambda a: a[views].to(_dev())
    return mesh.fuse_depth(t(case.depth), t(case.opac), t(case.viewm), t(case.projm), t(case.prcp), case.origin, case.voxel, case.dims, acc=acc)


def _holds_against_the_restatement(case, s, w, ref=None):
    """the rules of test_fuse_depth_matches_float64_restatement: at most 5 % of the voxels ambiguous, outside them equal weights and
    sums within 1e-5"""
    rs, rw, amb = MC.reference(case, R) if ref is None else ref
    s, w = s.cpu().double(), w.cpu().double()
    ok = ~amb
    err = float((s[ok] - rs[ok]).abs().max())
    print(f"ambiguous {float(amb.float().mean()):.4f}, weights differing {int((w[ok] != rw[ok]).sum())}, largest sum error {err:.2e}")
    assert amb.float().mean() <= MC.AMBIGUOUS_CAP
    assert torch.equal(w[ok], rw[ok])
    assert err <= 1e-5


@pytest.mark.parametrize("name", list(MC.FUSION_CASES))
def test_fuse_depth_off_the_cube(name):
    case = MC.fusion_case(name)
    s, w = _fuse(case)
    assert s.shape == case.dims and w.shape == case.dims
    _holds_against_the_restatement(case, s, w)


@pytest.mark.parametrize("n", [64, 65, 130])
def test_fuse_depth_chunks_equal_one_call_per_view(n):
    """fuse_depth hands the kernel 64 views per call; the kernel adds in view order, so one call per view gives the same bits"""
    case = MC.fusion_case("chunk")
    s, w = _fuse(case, slice(0, n))
    acc = None
    for k in range(n):
        acc = _fuse(case, slice(k, k + 1), acc)
    assert _same_bits(s, acc[0]) and _same_bits(w, acc[1])
    assert float(w.max()) > 0.75 * n                      # voxels that most views observe: more than one call's 64 at n = 130


def test_fuse_depth_a_view_of_the_second_chunk_alone():
    case = MC.fusion_case("chunk")
    s, w = _fuse(case, slice(MC.CHUNK_VIEW, MC.CHUNK_VIEW + 1))
    _holds_against_the_restatement(MC.one_view(case, MC.CHUNK_VIEW), s, w)


def test_fuse_depth_input_forms():
    from soar_amd import mesh
    case, dev = MC.fusion_case("offcube"), _dev()
    s, w = _fuse(case)

    def strided64(t):                                     # float64, every second element of a buffer twice as wide, NaN between
        wide = torch.full(t.shape[:-1] + (2 * t.shape[-1],), float("nan"), dtype=torch.float64, device=dev)
        wide[..., ::2] = t.to(dev)
        assert not wide[..., ::2].is_contiguous()
        return wide[..., ::2]

    def transposed(t):                                    # the matrices stored column-major
        v = t.to(dev).transpose(1, 2).contiguous().transpose(1, 2)
        assert not v.is_contiguous()
        return v
    s2, w2 = mesh.fuse_depth(strided64(case.depth), strided64(case.opac), transposed(case.viewm), strided64(case.projm), strided64(case.prcp),
                             case.origin, case.voxel, case.dims)
    assert _same_bits(s, s2) and _same_bits(w, w2)
    one = torch.tensor([0.45, 0.55], device=dev).expand(case.n, 2)
    assert one.stride(0) == 0
    args = [t.to(dev) for t in (case.depth, case.opac, case.viewm, case.projm)]
    s3, w3 = mesh.fuse_depth(*args, one, case.origin, case.voxel, case.dims)
    s4, w4 = mesh.fuse_depth(*args, one.contiguous(), case.origin, case.voxel, case.dims)
    assert _same_bits(s3, s4) and _same_bits(w3, w4) and not _same_bits(s3, s)


def test_fuse_depth_nonfinite_pixels():
    """A NaN opacity, or an opaque pixel with a NaN depth, is no observation; +-inf follow the arithmetic (include/soar_hip.h)."""
    case = MC.fusion_case("offcube")
    planted = MC.plant_nonfinite(case)
    s, w = _fuse(planted)
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(w).all())
    _holds_against_the_restatement(planted, s, w)
    clean_w = _fuse(case)[1].cpu().double()
    _, rw, amb = MC.reference(case, R)
    for kind in ("depth nan", "opac nan"):
        only = MC.plant_nonfinite(case, (kind,))
        _, kw, kamb = MC.reference(only, R)
        lost = ~(amb | kamb) & (kw < rw)                  # voxels that project to a planted NaN pixel (test_mesh_cases_cpu: there are some)
        got = _fuse(only)[1].cpu().double()
        assert lost.any() and bool((got < clean_w)[lost].all()), kind


def test_extract_mesh_is_the_same_in_any_grouping():
    from soar_amd import mesh
    from soar_amd import synthetic as syn
    s = syn.make_surfels(4000)
    args = [t.to(_dev()) for t in (s.xyz, s.rot, s.scales, s.opacity)]
    a = mesh.extract_mesh(*args, resolution=48, n_views=10, image_size=128, group=4)
    b = mesh.extract_mesh(*args, resolution=48, n_views=10, image_size=128, group=10)
    assert a.faces.shape[0] > 500
    assert _same_bits(a.vertices, b.vertices) and _same_bits(a.faces, b.faces)


# ---- 9. marching cubes off the cube --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _mc_reference(order, masked, level):
    f, m = MC.mc_field(order)
    return R.marching_cubes(f, level, m if masked else None)


def _mc_equals_the_driver(f, valid=None, level=0.0, ref=None):
    v, fc = _gpu_mc(f, valid, level)
    rv, rf = R.marching_cubes(f, level, valid) if ref is None else ref
    assert v.dtype == np.float32 and fc.dtype == np.int32 and v.shape[1:] == (3,) and fc.shape[1:] == (3,)
    assert _same_bits(v, rv) and _same_bits(fc, rf)
    assert len(fc) == R.table_face_count(f, level, valid)
    return v, fc


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("order", list(MC.MC_AXES))
def test_marching_cubes_equals_the_table_driver_off_the_cube(order, masked, level):
    f, m = MC.mc_field(order)
    valid = m if masked else None
    v, fc = _mc_equals_the_driver(f, valid, level, _mc_reference(order, masked, level))
    assert len(fc) > 5000
    R.check_vertices_on_crossings(v, f, level, valid)
    if not masked:
        R.check_closed_manifold(v, fc, f.shape)


@pytest.mark.parametrize("level", [0.0, 0.25])
@pytest.mark.parametrize("masked", [False, True])
def test_marching_cubes_does_not_depend_on_the_axis_order(masked, level):
    """the same field with its axes in another order: the same vertices (as a set, columns permuted back) and as many faces"""
    base = None
    for order in MC.MC_AXES:
        f, m = MC.mc_field(order)
        v, fc = _gpu_mc(f, m if masked else None, level)
        got = (MC.sorted_rows(MC.mc_unpermute(v, order)), len(fc))
        base = base or got
        assert _same_bits(got[0], base[0]) and got[1] == base[1] > 0, order


@pytest.mark.parametrize("shape", MC.MC_SIZE_GRIDS + MC.MC_FLAT_GRIDS, ids=lambda s: "x".join(map(str, s)))
def test_marching_cubes_at_the_block_edge_and_on_flat_grids(shape):
    f = MC.mc_random(shape, 320)
    v, fc = _mc_equals_the_driver(f)
    assert len(v) > 0
    R.check_vertices_on_crossings(v, f)
    if min(shape) == 1:
        assert fc.shape == (0, 3)                         # vertices but no cell
    else:
        assert len(fc) > 0
        R.check_closed_manifold(v, fc, shape)
    valid = np.random.default_rng(325).uniform(size=shape) > 0.1
    _mc_equals_the_driver(f, valid, 0.25)


def test_marching_cubes_empty_results():
    f = np.abs(MC.mc_random((6, 7, 8), 321)) + 0.5        # no crossing
    one = np.zeros(f.shape, bool)
    one[2, 3, 4] = True
    for field, valid in ((f, None), (MC.mc_random(f.shape, 322), np.zeros(f.shape, bool)), (MC.mc_random(f.shape, 322), one)):
        v, fc = _mc_equals_the_driver(field, valid)
        assert v.shape == (0, 3) and fc.shape == (0, 3)


@pytest.mark.parametrize("negative_zeros", [False, True])
def test_marching_cubes_ties(negative_zeros):
    """values equal to the level: t = 0 or 1 exactly and triangles of zero area; the bits and the table's count are the check"""
    f = MC.mc_ties(negative_zeros)
    v, fc = _mc_equals_the_driver(f)
    assert len(fc) > 0 and (v == np.floor(v)).all(1).any()
    valid = np.random.default_rng(326).uniform(size=f.shape) > 0.1
    _mc_equals_the_driver(f, valid)


def test_marching_cubes_input_forms():
    from soar_amd import mesh
    dev = _dev()
    run = lambda f, valid=None: mesh.marching_cubes(f, 0.25, valid)
    f64 = torch.from_numpy(np.random.default_rng(327).standard_normal(MC.MC_BASE)).to(dev)
    valid = torch.from_numpy(MC.mc_field("xyz")[1]).to(dev)
    for f in (f64, f64.half()):                           # float64 and float16 against their float32 copies
        assert f.dtype != torch.float32
        a, b = run(f, valid), run(f.float(), valid)
        assert len(a[1]) > 5000 and _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    assert not _same_bits(run(f64)[0], run(f64.half())[0])
    view = f64.float().permute(2, 0, 1)                   # not contiguous
    mview = valid.permute(2, 0, 1)
    assert not view.is_contiguous() and not mview.is_contiguous()
    a, b = run(view, mview), run(view.contiguous(), mview.contiguous())
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
    bytes_ = valid.to(torch.uint8) * torch.from_numpy(np.random.default_rng(328).integers(1, 256, MC.MC_BASE).astype(np.uint8)).to(dev)
    assert bytes_.dtype == torch.uint8 and int(bytes_.max()) > 1 and torch.equal(bytes_ != 0, valid)
    a, b = run(f64.float(), bytes_), run(f64.float(), valid)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


# ---- 10. the component filter at its thresholds ----------------------------------------------------------------------------------

def _gpu_filter(case):
    from soar_amd import mesh
    dev = _dev()
    v, f = mesh.filter_components(torch.from_numpy(case.verts).to(dev), torch.from_numpy(case.faces).to(dev), min_faces=case.min_faces,
                                  min_diag_frac=case.min_diag_frac)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return _np(v), _np(f)


def _filter_equals_the_restatement(case):
    want_v, want_f = R.filter_components(case.verts, case.faces, case.min_faces, case.min_diag_frac)
    if hasattr(case, "keep_v"):                           # the restatement keeps what the case is built to keep
        assert np.array_equal(want_v, case.verts[case.keep_v]) and len(want_f) == int(case.keep_f.sum())
    got_v, got_f = _gpu_filter(case)
    assert _same_bits(got_v, want_v) and _same_bits(got_f, want_f)
    return got_v, got_f


@pytest.mark.parametrize("min_faces", MC.FAN_MIN_FACES)
def test_component_filter_counts_faces_under_mixed_waves(min_faces):
    v, f = _filter_equals_the_restatement(MC.fans_case(min_faces))
    assert len(f) == 2 * sum(k for k in range(1, 131) if k >= min_faces)


@pytest.mark.parametrize("permute", [False, True])
def test_component_filter_boxes_at_a_tie_and_unused_vertices(permute):
    v, f = _filter_equals_the_restatement(MC.tie_case(permute, strays=False))
    assert len(f) == 103
    v2, f2 = _filter_equals_the_restatement(MC.tie_case(permute, strays=True))
    assert _same_bits(v, v2) and _same_bits(f, f2)        # vertices that no face uses, 1000 away, change nothing


@pytest.mark.parametrize("shuffled", [False, True])
def test_component_filter_deep_forests(shuffled):
    case = MC.strip_case(shuffled)
    v, f = _filter_equals_the_restatement(case)
    assert _same_bits(v, case.verts) and _same_bits(f, case.faces)


@pytest.mark.parametrize("V,F,seed", MC.SIZED_CASES)
def test_component_filter_sizes(V, F, seed):
    case = MC.sized_case(V, F, seed)
    assert case.verts.shape == (V, 3) and case.faces.shape == (F, 3)
    _filter_equals_the_restatement(case)


def test_component_filter_single_triangle():
    case = MC.single_triangle()
    v, f = _filter_equals_the_restatement(case)
    assert _same_bits(v, case.verts) and np.array_equal(f, case.faces)
