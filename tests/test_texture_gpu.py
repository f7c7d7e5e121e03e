"""GPU tests of the texture atlas (soar_amd/texture.py: build_atlas, bake_texture, export_avatar's hook; csrc/mesh_texture.hip) against
the NumPy restatement tests/texture_ref.py, whose invariants tests/test_texture_cpu.py checks.

A texel whose 3-D point is not finite (fixture f's face with the NaN vertex) has no nearest surfel: ``vertex_attributes`` refuses
such a query, so there is no colour of its to compare with.  Those texels are owned, keep their non-finite debug position, and are
black; every other owned texel is compared bit for bit."""
import numpy as np
import pytest
import torch

import texture_ref as R

pytestmark = pytest.mark.gpu

FIXTURES = R.fixtures()
ATLAS_CASES = [(fx, T) for fx in FIXTURES for T in R.SIZES if R.fits(fx, T)]
BAKE_CASES = [(R.fixture(p), T) for p, T in (("c", 64), ("d", 64), ("f", 64), ("g", 64), ("g", 16))]
KS = (1, 4, 8)
ids = lambda cases: [f"{fx.name}-T{T}" for fx, T in cases]


def _dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(fx):
    from soar_amd import mesh
    return mesh.Mesh(torch.from_numpy(fx.verts).to(_dev()), torch.from_numpy(fx.faces).to(_dev()))


def _finite_extent(fx):
    v = fx.verts[np.isfinite(fx.verts).all(1)]
    return v.min(0), v.max(0), float(np.abs(v).max())


def _surfels(fx, n=500, seed=21):
    lo, hi, _ = _finite_extent(fx)
    rng = np.random.default_rng(seed)
    pts = (lo - 0.1 + rng.random((n, 3)) * (hi - lo + 0.2)).astype(np.float32)
    return torch.from_numpy(pts).to(_dev()), torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(_dev())


@pytest.fixture(scope="module")
def wanted():
    """the restatement's atlas of every case, computed once"""
    return {(fx.name, T): R.build_atlas(fx.verts, fx.faces, T) for fx, T in ATLAS_CASES}


@pytest.fixture(scope="module")
def baked():
    """bake_texture(return_debug=True) of a case and k, computed once"""
    from soar_amd import mesh
    cache = {}

    def get(fx, T, k):
        if (fx.name, T, k) not in cache:
            m = _mesh(fx)
            atlas = mesh.build_atlas(m, T)
            pts, col = _surfels(fx)
            cache[(fx.name, T, k)] = (atlas, pts, col) + tuple(mesh.bake_texture(m, atlas, pts, col, k=k, return_debug=True))
        return cache[(fx.name, T, k)]
    return get


# ---- the atlas -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fx,T", ATLAS_CASES, ids=ids(ATLAS_CASES))
def test_build_atlas_equals_the_restatement(fx, T, wanted):
    from soar_amd import mesh
    want = wanted[(fx.name, T)]
    got = mesh.build_atlas(_mesh(fx), T)
    F = len(fx.faces)
    assert isinstance(got, mesh.Atlas) and got.size == T and got.scale_step == want.scale_step
    assert got.uv.shape == (3 * F, 2) and got.uv.dtype == torch.float32
    assert got.uv_faces.shape == (F, 3) and got.uv_faces.dtype == torch.int32 and got.cell.shape == (F, 4) and got.cell.dtype == torch.int32
    assert np.array_equal(_np(got.cell), want.cell), (fx.name, T)
    assert np.array_equal(_np(got.uv_faces), want.uv_faces)
    assert np.array_equal(_np(got.uv), want.uv)                                # ratios of small integers to a power of two: exact
    again = mesh.build_atlas(_mesh(fx), T)
    assert torch.equal(again.cell, got.cell) and torch.equal(again.uv, got.uv) and again.scale_step == got.scale_step


def test_levels_at_the_ladder_thresholds_equal_the_restatement():
    """Fixture (j): faces whose area is within a few ulps of a threshold, where a square root that is one ulp off changes the level
    (tests/test_texture_cpu.py counts them).  The levels the kernel keeps in its workspace, their histogram and the whole atlas
    equal the restatement."""
    import ctypes as C

    from soar_amd import hip_lib, mesh, texture
    fx, T = R.threshold_fixture(), 256
    m = _mesh(fx)
    V, F = len(fx.verts), len(fx.faces)
    want = R.levels(fx.verts, fx.faces)
    L = hip_lib.lib()
    nb = C.c_size_t(0)
    assert L.soar_mesh_atlas_bytes(F, C.byref(nb)) == 0
    ws = mesh._workspace(nb.value, _dev())
    th = texture.ladder().to(_dev())
    hist = (C.c_int64 * (R.LADDER_N + 2))()
    rc = L.soar_mesh_atlas_levels(V, F, m.vertices.data_ptr(), m.faces.data_ptr(), th.data_ptr(), R.LADDER_N, ws.data_ptr(), nb.value, hist,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, hip_lib.last_error()
    got = _np(ws[:4 * F].view(torch.int32)).astype(np.int64)
    down, up = R.levels_if_the_area_were_an_ulp_off(fx.verts, fx.faces)
    print(f"levels: {int((got != want).sum())} of {F} differ; an ulp down would change {int((down != want).sum())}, an ulp up {int((up != want).sum())}")
    assert np.array_equal(got, want)
    assert list(hist) == np.bincount(want, minlength=R.LADDER_N + 1).tolist() + [0]
    ref = R.build_atlas(fx.verts, fx.faces, T)
    atlas = mesh.build_atlas(m, T)
    assert atlas.scale_step == ref.scale_step and np.array_equal(_np(atlas.cell), ref.cell) and np.array_equal(_np(atlas.uv), ref.uv)


def test_too_many_faces_are_refused_with_the_size_that_fits():
    from soar_amd import mesh
    with pytest.raises(ValueError, match="smallest that can is 32"):
        mesh.build_atlas(_mesh(R.fixture("h")), 16)
    assert mesh.build_atlas(_mesh(R.fixture("h")), 32).cell.shape == (33, 4)
    bad = _mesh(R.fixture("c"))
    bad.faces[1, 2] = 99
    with pytest.raises(RuntimeError, match="outside"):
        mesh.build_atlas(bad, 64)


def test_a_mesh_without_faces_bakes_an_empty_texture():
    from soar_amd import mesh
    fx = R.fixture("i")
    atlas = mesh.build_atlas(_mesh(fx), 16)
    pts, col = _surfels(fx)
    tex, dbg = mesh.bake_texture(_mesh(fx), atlas, pts, col, return_debug=True)
    assert tex.shape == (16, 16, 3) and tex.dtype == torch.uint8 and not tex.any() and (dbg["owner"] == -1).all()


# ---- ownership, positions, colours -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fx,T", BAKE_CASES, ids=ids(BAKE_CASES))
def test_ownership_and_positions_match_the_restatement(fx, T, wanted, baked):
    """position: b1, b2, b0 (two roundings), three products and two sums are at most eight float32 roundings per component, each of
    a number of at most max|vertex coordinate| in size (the weights are in [0, 1] and sum to 1): 8 * 2^-24 * max|v|."""
    want = wanted[(fx.name, T)]
    atlas, _, _, tex, dbg = baked(fx, T, 4)
    assert np.array_equal(_np(atlas.cell), want.cell)
    owner, bary64 = R.barycentrics(want.cell, T)
    assert dbg["owner"].dtype == torch.int32 and np.array_equal(_np(dbg["owner"]), owner)
    _, bary32 = R.barycentrics(want.cell, T, np.float32)
    assert np.array_equal(_np(dbg["bary"]), bary32)                             # every operation is a correctly rounded one
    pos = _np(dbg["position"]).astype(np.float64)
    ref = R.positions(fx.verts, fx.faces, owner, bary64)
    compare = owner >= 0
    if fx.name in R.NAN_FACE:
        nan_face = owner == R.NAN_FACE[fx.name]
        assert nan_face.sum() > 0 and not np.isfinite(pos[nan_face]).all(-1).any()
        compare &= ~nan_face
    bound = 8 * 2.0 ** -24 * _finite_extent(fx)[2]
    diff = float(np.abs(pos[compare] - ref[compare]).max())
    print(f"{fx.name} T={T}: {int(compare.sum())} texels, max |dposition| {diff:.3e} (bound {bound:.3e})")
    assert np.isfinite(pos[compare]).all() and diff <= bound
    assert not pos[owner < 0].any() and not _np(dbg["bary"])[owner < 0].any()


@pytest.mark.parametrize("fx,T", BAKE_CASES, ids=ids(BAKE_CASES))
def test_colours_are_vertex_attributes_at_the_texel(fx, T, baked):
    from soar_amd import mesh
    for k in KS:
        atlas, pts, col, tex, dbg = baked(fx, T, k)
        owned = dbg["owner"] >= 0
        finite = owned & torch.isfinite(dbg["position"]).all(-1)
        if fx.name in R.NAN_FACE:
            assert ((dbg["owner"] == R.NAN_FACE[fx.name]) == (owned & ~finite)).all()
        else:
            assert torch.equal(finite, owned)
        want, _, _ = mesh.vertex_attributes(dbg["position"][finite], pts, col, k=k)
        assert torch.equal(dbg["color"][finite], want), (fx.name, T, k)         # bit for bit
        assert torch.equal(tex[finite], torch.floor(want * 255.0 + 0.5).to(torch.uint8))
        assert tex.shape == (T, T, 3) and tex.dtype == torch.uint8
        assert not tex[~finite].any() and not dbg["color"][~finite].any()       # unowned texels, and texels without a point
        plain = mesh.bake_texture(_mesh(fx), atlas, pts, col, k=k)
        assert isinstance(plain, torch.Tensor) and torch.equal(plain, tex)


def test_chunks_repeats_and_views_give_the_same_bytes(baked):
    from soar_amd import mesh
    fx, T = R.fixture("d"), 64
    atlas, pts, col, tex, dbg = baked(fx, T, 4)
    m = _mesh(fx)
    sizes = sorted(set(atlas.cell[:, 2].tolist()))
    assert len(sizes) >= 2 and int((dbg["owner"] >= 0).sum()) > 1000             # chunks of 64 and 1000 end inside cells and rows
    for chunk in (64, 1000):
        got, d2 = mesh.bake_texture(m, atlas, pts, col, chunk_texels=chunk, return_debug=True)
        assert torch.equal(got, tex), chunk
        for key in ("owner", "bary", "position", "color"):
            assert torch.equal(d2[key], dbg[key]), (chunk, key)
    assert torch.equal(mesh.bake_texture(m, atlas, pts, col), tex)               # a second run
    wide = torch.stack([col, 1.0 - col], -1).reshape(len(col), 6)                # colours as every second column
    view = wide[:, ::2]
    assert not view.is_contiguous() and torch.equal(view, col)
    assert torch.equal(mesh.bake_texture(m, atlas, pts, view), tex)
    # an atlas that is not the mesh's, or whose cells lie outside the image, is refused before anything is written
    with pytest.raises(ValueError, match="atlas.cell"):
        mesh.bake_texture(m, atlas._replace(cell=atlas.cell[:-1]), pts, col)
    moved = atlas.cell.clone()
    moved[3, 0] = T
    with pytest.raises(RuntimeError, match="cells"):
        mesh.bake_texture(m, atlas._replace(cell=moved), pts, col)
    with pytest.raises(ValueError, match="k=8"):
        mesh.bake_texture(m, atlas, pts[:5], col[:5], k=8)


def test_a_smooth_colour_field_comes_through():
    """Surfels on a jittered grid around fixture (d), colour an affine function of position, k = 1: a texel has the colour of its
    nearest surfel, which the field's gradient times the distance to it bounds; the byte adds half a step, float32 the rest."""
    from soar_amd import mesh
    fx, T = R.fixture("d"), 64
    m = _mesh(fx)
    lo, hi, _ = _finite_extent(fx)
    rng = np.random.default_rng(33)
    n = 24
    g = np.stack(np.meshgrid(*[np.linspace(lo[k] - 0.2, hi[k] + 0.2, n) for k in range(3)], indexing="ij"), -1).reshape(-1, 3)
    g = g + (rng.random(g.shape) - 0.5) * 0.2 * (hi - lo + 0.4) / (n - 1)
    G = np.array([[0.02, -0.015, 0.02], [-0.025, 0.01, 0.015], [0.01, 0.02, -0.02]])
    pts = torch.from_numpy(g.astype(np.float32)).to(_dev())
    field = lambda p: 0.5 + p.double() @ torch.from_numpy(G).to(_dev()).T
    col = field(pts).float()
    assert 0.0 < float(col.min()) and float(col.max()) < 1.0
    atlas = mesh.build_atlas(m, T)
    tex, dbg = mesh.bake_texture(m, atlas, pts, col, k=1, return_debug=True)
    owned = dbg["owner"] >= 0
    pos = dbg["position"][owned]
    dmax = float(torch.cdist(pos.double(), pts.double()).min(1).values.max())
    bound = torch.from_numpy(np.linalg.norm(G, axis=1)).to(_dev()) * dmax + 1.0 / 255.0
    err = (tex[owned].double() / 255.0 - field(pos)).abs().max(0).values
    print(f"smooth field: {int(owned.sum())} texels, largest nearest-surfel distance {dmax:.3f}, max |dcolour| {err.tolist()} (bounds {bound.tolist()})")
    assert (err <= bound).all()


# ---- the hook --------------------------------------------------------------------------------------------------------------------

def test_export_avatar_bakes_a_texture_on_request(tmp_path):
    from test_mesh_attr_gpu import _capsule_surfels

    from soar_amd import mesh
    from soar_amd import synthetic as syn
    dev = _dev()
    surf = tuple(t.to(dev).contiguous() for t in _capsule_surfels(2000, 2))
    bm = syn.make_body_model(V=1024)
    kw = dict(resolution=48, n_views=8, image_size=128, quality_thresh=0.01)
    plain = mesh.export_avatar(surf, bm.v_template.to(dev), bm.lbs_weights.to(dev), **kw)
    out = mesh.export_avatar(surf, bm.v_template.to(dev), bm.lbs_weights.to(dev), texture_size=256, **kw)
    # without the argument: the keys and tensors of before, bit for bit
    assert sorted(plain) == ["color", "mesh", "normals", "quality", "weights"]
    assert sorted(out) == ["atlas", "color", "mesh", "normals", "quality", "texture", "weights"]
    assert torch.equal(plain["mesh"].vertices, out["mesh"].vertices) and torch.equal(plain["mesh"].faces, out["mesh"].faces)
    for key in ("color", "quality", "normals", "weights"):
        assert torch.equal(plain[key], out[key]), key
    m, atlas, tex = out["mesh"], out["atlas"], out["texture"]
    F = int(m.faces.shape[0])
    assert isinstance(atlas, mesh.Atlas) and atlas.size == 256 and atlas.cell.shape == (F, 4) and tex.shape == (256, 256, 3)
    again, dbg = mesh.bake_texture(m, atlas, surf[0], surf[4], return_debug=True)
    assert torch.equal(again, tex)
    # the texels' points lie on the returned mesh's faces: convex weights of the owner's corners
    owned = dbg["owner"] >= 0
    assert int(owned.sum()) > 16 * F and set(dbg["owner"][owned].unique().tolist()) == set(range(F))
    w = dbg["bary"][owned].double()
    tri = m.vertices.double()[m.faces.long()[dbg["owner"][owned].long()]]                 # [n,3,3]
    assert float(w.min()) >= 0.0 and float((w.sum(1) - 1.0).abs().max()) <= 4 * 2.0 ** -24
    bound = 8 * 2.0 ** -24 * float(m.vertices.abs().max())
    diff = float((dbg["position"][owned].double() - (w[:, :, None] * tri).sum(1)).abs().max())
    print(f"export_avatar(texture_size=256): F {F}, scale_step {atlas.scale_step}, sides {sorted(set(atlas.cell[:, 2].tolist()))}, "
          f"{int(owned.sum())} texels, max |dposition| {diff:.3e} (bound {bound:.3e})")
    assert diff <= bound
    # the colours are the vertex colours' rule: a texel whose point is a corner of its face (the corner texels, and the gutter texels
    # clamped onto a corner) has that vertex's colour (same surfels, same k)
    corner = (dbg["bary"][owned] == 1.0)
    vid = m.faces.long()[dbg["owner"][owned].long()][corner]
    assert corner.sum() >= 3 * F and torch.equal(dbg["color"][owned][corner.any(1)], out["color"][vid])
    # a size too small for the mesh is known only after the export: the error names the size that fits and carries the result
    with pytest.raises(ValueError, match="smallest that can is 256.*result") as info:
        mesh.export_avatar(surf, bm.v_template.to(dev), bm.lbs_weights.to(dev), texture_size=64, **kw)
    kept = info.value.result
    assert sorted(kept) == sorted(plain) and torch.equal(kept["mesh"].vertices, m.vertices) and torch.equal(kept["color"], plain["color"])
    path = tmp_path / "capsule.obj"
    mesh.save_textured_obj(str(path), m, atlas, tex)
    _, _, v, vt, f, ft = R.parse_textured_obj(str(path))
    assert np.array_equal(v.astype(np.float32), _np(m.vertices)) and np.array_equal(f, _np(m.faces)) and vt.shape == (3 * F, 2)
    assert (tmp_path / "capsule.mtl").exists() and (tmp_path / "capsule.png").exists()
