"""GPU tests of the mesh export (soar_amd/mesh.py, csrc/mesh.hip): TSDF fusion against a float64 restatement, the depth
convention of the renderer, marching cubes against the Python table driver, analytic fields, the whole path on the bench's
person and the component filter."""
import math

import numpy as np
import pytest
import torch

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
