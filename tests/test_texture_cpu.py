"""CPU tests of the texture atlas: the NumPy restatement tests/texture_ref.py satisfies the layout's invariants on every fixture
(conditions, not measurements), the host-side choice of the ladder step in soar_amd/texture.py agrees with it, the writer
round-trips, and the entry points refuse what they must.  The kernels are compared with the restatement in test_texture_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import texture_ref as R

FIXTURES = R.fixtures()
CASES = [(fx, T) for fx in FIXTURES for T in R.SIZES if R.fits(fx, T)]
IDS = [f"{fx.name}-T{T}" for fx, T in CASES]


@pytest.fixture(scope="module")
def atlases():
    return {(fx.name, T): R.build_atlas(fx.verts, fx.faces, T) for fx, T in CASES}


def test_the_fixtures_are_what_they_claim():
    names = [fx.name[0] for fx in FIXTURES]
    assert names == list("abcdefghi")
    assert [len(R.fixture(p).faces) for p in "abcghi"] == [1, 2, 3, 32, 33, 0]
    d = R.fixture("d")
    assert len(d.faces) == 320 and len(set(R.build_atlas(d.verts, d.faces, 64).cell[:, 2].tolist())) >= 2
    e = R.fixture("e")
    area = R.face_areas(e.verts, e.faces)
    assert np.array_equal(area, np.exp2(np.arange(-20.0, 21.0)).astype(np.float32))          # exactly 2^-20 .. 2^20
    for T in (64, 256):                                                                          # both clamps act
        a = R.build_atlas(e.verts, e.faces, T)
        q = np.floor_divide(a.level + a.scale_step, 8)
        assert (q < 2).any() and (q > T.bit_length() - 2).any() and a.cell[:, 2].min() == 4 and a.cell[:, 2].max() == T // 2
    f = R.fixture("f")
    lv = R.levels(f.verts, f.faces)
    assert R.face_areas(f.verts, f.faces)[2] == 0 and np.isnan(R.face_areas(f.verts, f.faces)[R.NAN_FACE[f.name]])
    assert (lv < 0).sum() == 2 and lv[2] < 0 and lv[R.NAN_FACE[f.name]] < 0
    for T in R.SIZES:
        assert (R.build_atlas(f.verts, f.faces, T).cell[lv < 0, 2] == 4).all()
    g = R.build_atlas(R.fixture("g").verts, R.fixture("g").faces, 16)
    assert (g.cell[:, 2] == 4).all() and R.owner_map(g.cell, 16)[1].sum() == 16 * 16                # exactly full
    # every level is a comparison with the table: thresholds themselves count, the float32 below them does not
    th = R.ladder()
    assert th[0] == 2.0 ** -32 and th[-1] == 2.0 ** 32 and th[256] == 1.0 and len(th) == 513
    tri = lambda area: (np.array([[0, 0, 0], [2 * area, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    assert R.levels(*tri(1.0))[0] == 257 and R.levels(*tri(np.nextafter(np.float32(1.0), np.float32(0.0))))[0] == 256


def test_the_threshold_fixture_tells_a_square_root_that_is_an_ulp_off():
    """(j) is what makes the GPU comparison of the levels mean something: for hundreds of its faces the level differs when the
    area is the float32 next to the correctly rounded one, on either side, and the restatement's atlas obeys the layout rules."""
    fx = R.threshold_fixture()
    F = len(fx.faces)
    assert F == 6840 and R.fits(fx, 256)
    lv = R.levels(fx.verts, fx.faces)
    down, up = R.levels_if_the_area_were_an_ulp_off(fx.verts, fx.faces)
    print(f"levels that change with the area one ulp down: {int((down != lv).sum())}, up: {int((up != lv).sum())}")
    assert (lv >= 0).all() and (down != lv).sum() >= 300 and (up != lv).sum() >= 300
    assert (np.bincount(lv[:3840], minlength=R.LADDER_N + 1)[200:321] > 0).all()       # both sides of every threshold 200 .. 319
    a = R.build_atlas(fx.verts, fx.faces, 256)
    owner, claims = R.owner_map(a.cell, 256)
    assert claims.max() == 1 and len(set(a.cell[:, 2].tolist())) >= 2 and len(np.unique(owner[owner >= 0])) == F


def test_refusals_of_the_restatement():
    h = R.fixture("h")
    with pytest.raises(ValueError, match="smallest that can is 32"):
        R.build_atlas(h.verts, h.faces, 16)
    assert R.build_atlas(h.verts, h.faces, 32).cell.shape == (33, 4)
    for fx in FIXTURES:
        for T in fx.raises_at:
            with pytest.raises(ValueError, match="smallest that can"):
                R.build_atlas(fx.verts, fx.faces, T)
    for T in (8, 24, 0, -16, 100, 32768):
        with pytest.raises(ValueError, match="texture_size"):
            R.build_atlas(h.verts, h.faces, T)
    empty = R.build_atlas(R.fixture("i").verts, R.fixture("i").faces, 16)
    assert empty.uv.shape == (0, 2) and empty.cell.shape == (0, 4) and (R.owner_map(empty.cell, 16)[0] == -1).all()


@pytest.mark.parametrize("fx,T", CASES, ids=IDS)
def test_cells_are_inside_aligned_and_disjoint(fx, T, atlases):
    a = atlases[(fx.name, T)]
    x0, y0, s, half = (a.cell[:, k].astype(np.int64) for k in range(4))
    assert ((s >= 4) & (s <= T // 2) & (s & (s - 1) == 0)).all() and np.isin(half, (0, 1)).all()
    assert ((x0 >= 0) & (y0 >= 0) & (x0 + s <= T) & (y0 + s <= T)).all()
    assert (x0 % s == 0).all() and (y0 % s == 0).all()
    # two faces share a cell exactly when they are its two halves; different cells do not overlap
    cells = {}
    for f in range(len(s)):
        cells.setdefault((int(x0[f]), int(y0[f]), int(s[f])), []).append(int(half[f]))
    assert all(sorted(h) in ([0], [0, 1]) for h in cells.values())
    cover = np.zeros((T, T), np.int32)
    for (cx, cy, cs) in cells:
        cover[cy:cy + cs, cx:cx + cs] += 1
    assert cover.max() <= 1
    # ownership: exactly one owner, and the count is the cells' area less the empty halves of odd cells
    owner, claims = R.owner_map(a.cell, T)
    assert claims.max() <= 1 and ((owner >= 0) == (claims == 1)).all()
    want = sum(cs * cs - (cs * (cs - 1) // 2 if h == [0] else 0) for (_, _, cs), h in cells.items())
    assert int((owner >= 0).sum()) == want
    assert np.array_equal(a.uv_faces, np.arange(3 * len(s), dtype=np.int32).reshape(-1, 3))
    # the order: sizes only decrease along the curve, faces of one size in index order
    morton = lambda x, y: sum((((x >> b) & 1) << (2 * b)) | (((y >> b) & 1) << (2 * b + 1)) for b in range(14))
    key = np.array([morton(int(x0[f]) // 4, int(y0[f]) // 4) * 2 + int(half[f]) for f in range(len(s))], np.int64)
    along = np.argsort(key, kind="stable")
    assert (np.diff(s[along]) <= 0).all()
    for size in np.unique(s):
        assert (np.diff(along[s[along] == size]) > 0).all()
    # no gap: the cells fill the curve from its start
    used = sorted((morton(cx // 4, cy // 4), (cs // 4) ** 2) for (cx, cy, cs) in cells)
    at = 0
    for start, n in used:
        assert start == at
        at += n


@pytest.mark.parametrize("fx,T", CASES, ids=IDS)
def test_corners_are_texel_centres_and_no_bilinear_tap_leaves_its_face(fx, T, atlases):
    a = atlases[(fx.name, T)]
    F = len(a.cell)
    owner, _ = R.owner_map(a.cell, T)
    uv = a.uv.astype(np.float64).reshape(F, 3, 2)
    # (u T, (1 - v) T) is the centre of a texel of the face's own cell, owned by the face
    cx, cy = uv[..., 0] * T, (1.0 - uv[..., 1]) * T
    assert (cx - 0.5 == np.floor(cx)).all() and (cy - 0.5 == np.floor(cy)).all()
    px, py = np.floor(cx).astype(np.int64), np.floor(cy).astype(np.int64)
    assert np.array_equal(np.stack([px, py], -1), R.corner_texels(a.cell))
    x0, y0, s = (a.cell[:, k].astype(np.int64)[:, None] for k in range(3))
    assert ((px >= x0) & (px < x0 + s) & (py >= y0) & (py < y0 + s)).all()
    if F:
        assert (owner[py, px] == np.arange(F)[:, None]).all()
    # 64 seeded points in every UV triangle: all four taps of a bilinear lookup are the face's own texels
    rng = np.random.default_rng(5)
    w = rng.dirichlet(np.ones(3), size=(F, 64))                                  # [F,64,3]
    w[:, :3] = np.eye(3)                                                         # the corners themselves
    w[:, 3:6] = 0.5 * (1.0 - np.eye(3))                                          # and the middles of the edges
    tx = (w @ cx[..., None])[..., 0] - 0.5                                       # continuous texel coordinates
    ty = (w @ cy[..., None])[..., 0] - 0.5
    for ix in (np.floor(tx), np.ceil(tx)):
        for iy in (np.floor(ty), np.ceil(ty)):
            ix_, iy_ = ix.astype(np.int64), iy.astype(np.int64)
            assert ((ix_ >= 0) & (ix_ < T) & (iy_ >= 0) & (iy_ < T)).all()
            assert (owner[iy_, ix_] == np.arange(F)[:, None]).all()


@pytest.mark.parametrize("fx,T", CASES, ids=IDS)
def test_the_step_fits_and_the_next_does_not(fx, T, atlases):
    from soar_amd import texture
    a = atlases[(fx.name, T)]
    cap, top_step = (T // 4) ** 2, 8 * (T.bit_length() - 2)
    assert R.units(a.level, a.scale_step, T) <= cap
    assert a.scale_step == top_step or R.units(a.level, a.scale_step + 1, T) > cap
    if a.scale_step == top_step:
        assert (R.sides(a.level, a.scale_step, T)[a.level >= 0] == T // 2).all()
    assert R.J_MIN <= a.scale_step <= top_step
    # the package's host-side choice from the histogram is the same rule
    hist = [int((a.level == e).sum()) for e in range(R.LADDER_N + 1)] + [int((a.level < 0).sum())]
    assert texture.pick_step(hist, T) == a.scale_step
    for step in (a.scale_step, a.scale_step + 1, R.J_MIN, 0):
        assert texture._units(hist, step, T) == R.units(a.level, step, T)


def test_barycentrics_of_the_restatement():
    """corners have unit weights, inner texels the plain ratios, gutter texels are clamped onto the hypotenuse"""
    c = R.fixture("c")
    a = R.build_atlas(c.verts, c.faces, 64)
    owner, w = R.barycentrics(a.cell, 64)
    assert np.allclose(w[owner >= 0].sum(-1), 1.0, atol=1e-15) and (w >= 0).all()
    t = R.corner_texels(a.cell)
    for f in range(3):
        for k in range(3):
            assert np.array_equal(w[t[f, k, 1], t[f, k, 0]], np.eye(3)[k])
    _, w32 = R.barycentrics(a.cell, 64, np.float32)
    assert w32.dtype == np.float32 and np.abs(w32 - w).max() <= 4 * 2.0 ** -24
    pos = R.positions(c.verts, c.faces, owner, w)
    for f in range(3):
        for k in range(3):
            assert np.array_equal(pos[t[f, k, 1], t[f, k, 0]], c.verts[c.faces[f, k]].astype(np.float64))


def test_the_ladder_of_the_package_is_the_restatements():
    from soar_amd import texture
    assert np.array_equal(texture.ladder().numpy(), R.ladder()) and texture.ladder().dtype == torch.float32
    assert (texture.LADDER_N, texture.STEP_MIN, texture.MIN_SIZE, texture.MAX_SIZE) == (R.LADDER_N, R.J_MIN, R.MIN_T, R.MAX_T)
    with pytest.raises(ValueError, match="smallest that can is 32"):
        texture.pick_step([0] * 300 + [33] + [0] * (R.LADDER_N + 1 - 300), 16)


# ---- the writer ------------------------------------------------------------------------------------------------------------------

def test_save_textured_obj_round_trips(tmp_path):
    from PIL import Image

    from soar_amd import mesh
    fx, T = R.fixture("d"), 64
    a = R.build_atlas(fx.verts, fx.faces, T)
    atlas = mesh.Atlas(torch.from_numpy(a.uv), torch.from_numpy(a.uv_faces), torch.from_numpy(a.cell), a.scale_step, T)
    tex = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (T, T, 3), dtype=np.uint8))
    m = mesh.Mesh(torch.from_numpy(fx.verts), torch.from_numpy(fx.faces))
    path = tmp_path / "avatar.obj"
    mesh.save_textured_obj(str(path), m, atlas, tex)
    mtllib, usemtl, v, vt, f, ft = R.parse_textured_obj(str(path))
    F = len(fx.faces)
    assert mtllib == "avatar.mtl" and usemtl is not None
    assert np.array_equal(v.astype(np.float32), fx.verts) and np.array_equal(f, fx.faces)
    assert vt.shape == (3 * F, 2) and np.array_equal(vt.astype(np.float32), a.uv) and np.array_equal(ft, a.uv_faces)
    mtl = (tmp_path / "avatar.mtl").read_text().split("\n")
    assert f"newmtl {usemtl}" in mtl and "map_Kd avatar.png" in mtl
    back = np.asarray(Image.open(tmp_path / "avatar.png"))
    assert back.shape == (T, T, 3) and back.dtype == np.uint8 and np.array_equal(back, tex.numpy())
    # a vt maps through (u T, (1 - v) T) to the centre of the texel the atlas put the corner on
    texel = R.corner_texels(a.cell).reshape(-1, 2)
    assert np.array_equal(vt[:, 0] * T, texel[:, 0] + 0.5) and np.array_equal((1.0 - vt[:, 1]) * T, texel[:, 1] + 0.5)
    # shapes that do not belong together are refused
    with pytest.raises(ValueError, match="texture must be"):
        mesh.save_textured_obj(str(path), m, atlas, tex[:32])
    with pytest.raises(ValueError, match="atlas.uv"):
        mesh.save_textured_obj(str(path), mesh.Mesh(m.vertices, m.faces[:5]), atlas, tex)


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_python_api_refuses_cpu_tensors_and_bad_arguments():
    from soar_amd import mesh, texture
    assert mesh.build_atlas is texture.build_atlas and mesh.bake_texture is texture.bake_texture
    assert mesh.Atlas._fields == ("uv", "uv_faces", "cell", "scale_step", "size")
    fx = R.fixture("c")
    m = mesh.Mesh(torch.from_numpy(fx.verts), torch.from_numpy(fx.faces))
    for T in (8, 24, 100, 0, -64, 32768, 64.0, None):
        with pytest.raises(ValueError, match="texture_size"):
            mesh.build_atlas(m, T)
    with pytest.raises(RuntimeError, match="vertices.*no CPU fallback"):
        mesh.build_atlas(m, 64)
    a = R.build_atlas(fx.verts, fx.faces, 64)
    atlas = mesh.Atlas(torch.from_numpy(a.uv), torch.from_numpy(a.uv_faces), torch.from_numpy(a.cell), a.scale_step, 64)
    pts, col = torch.rand(20, 3), torch.rand(20, 3)
    for k in (0, 9, -1):
        with pytest.raises(ValueError, match=f"k={k}"):
            mesh.bake_texture(m, atlas, pts, col, k=k)
    with pytest.raises(ValueError, match="chunk_texels=0"):
        mesh.bake_texture(m, atlas, pts, col, chunk_texels=0)
    with pytest.raises(ValueError, match="texture_size"):
        mesh.bake_texture(m, atlas._replace(size=48), pts, col)
    with pytest.raises(TypeError, match="atlas"):
        mesh.bake_texture(m, tuple(atlas), pts, col)
    with pytest.raises(RuntimeError, match="vertices.*no CPU fallback"):
        mesh.bake_texture(m, atlas, pts, col)
    # export_avatar judges texture_size before it exports anything
    with pytest.raises(ValueError, match="texture_size"):
        mesh.export_avatar((pts, torch.rand(20, 4), torch.rand(20, 3), torch.rand(20, 1), col), pts, torch.rand(20, 55), texture_size=100)


def test_the_c_abi_refuses_bad_arguments_without_a_launch():
    from soar_amd import build, hip_lib
    build.build()
    L = hip_lib.lib()
    n = C.c_size_t(0)
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)                  # any non-NULL address: nothing reads it before the checks fail
    hist = (C.c_int64 * (R.LADDER_N + 2))()
    total = C.c_int64(0)

    def refused(rc, word):
        assert rc != 0 and word in hip_lib.last_error(), (rc, hip_lib.last_error())

    assert L.soar_mesh_atlas_bytes(100000, C.byref(n)) == 0 and n.value >= 5 * 4 * 100000 and n.value % 256 == 0
    assert L.soar_mesh_texels_bytes(100000, C.byref(n)) == 0 and n.value >= 2 * 8 * 100001 and n.value % 256 == 0
    refused(L.soar_mesh_atlas_bytes(0, C.byref(n)), "F=0")
    refused(L.soar_mesh_atlas_bytes(10, None), "soar_mesh_atlas_bytes")
    refused(L.soar_mesh_texels_bytes(-1, C.byref(n)), "F=-1")
    refused(L.soar_mesh_atlas_levels(0, 10, p, p, p, R.LADDER_N, p, 1 << 20, hist, None), "V=0")
    refused(L.soar_mesh_atlas_levels(10, 10, p, p, p, 2000, p, 1 << 20, hist, None), "n_ladder=2000")
    refused(L.soar_mesh_atlas_levels(10, 10, p, None, p, R.LADDER_N, p, 1 << 20, hist, None), "NULL")
    refused(L.soar_mesh_atlas_levels(10, 10, p, p, p, R.LADDER_N, None, 1 << 20, hist, None), "workspace")
    refused(L.soar_mesh_atlas_levels(10, 10, p, p, p, R.LADDER_N, 0x1000, 16, hist, None), "need")
    refused(L.soar_mesh_atlas_place(10, 48, R.LADDER_N, 0, 0x1000, 1 << 20, p, p, p, None), "texture_size=48")
    refused(L.soar_mesh_atlas_place(10, 8, R.LADDER_N, 0, 0x1000, 1 << 20, p, p, p, None), "texture_size=8")
    refused(L.soar_mesh_atlas_place(10, 64, R.LADDER_N, 5000, 0x1000, 1 << 20, p, p, p, None), "scale_step=5000")
    refused(L.soar_mesh_atlas_place(10, 64, R.LADDER_N, 0, 0x1000, 1 << 20, p, None, p, None), "NULL")
    refused(L.soar_mesh_atlas_place(10, 64, R.LADDER_N, 0, 0x1010, 1 << 20, p, p, p, None), "aligned")
    refused(L.soar_mesh_texel_offsets(10, 10, 32768, p, p, 0x1000, 1 << 20, C.byref(total), None), "texture_size=32768")
    refused(L.soar_mesh_texel_offsets(10, 10, 64, p, None, 0x1000, 1 << 20, C.byref(total), None), "NULL")
    refused(L.soar_mesh_texel_offsets(10, 10, 64, p, p, 0x1000, 8, C.byref(total), None), "need")
    refused(L.soar_mesh_texels(10, 10, 64, p, p, p, 0x1000, 1 << 20, 0, 0, p, p, None, None, None, None), "count=0")
    refused(L.soar_mesh_texels(10, 10, 64, p, p, p, 0x1000, 1 << 20, 4000, 200, p, p, None, None, None, None), "64^2")
    refused(L.soar_mesh_texels(10, 10, 64, p, p, p, 0x1000, 1 << 20, 0, 10, None, p, None, None, None, None), "NULL")
    refused(L.soar_mesh_texels(10, 10, 64, p, p, p, None, 1 << 20, 0, 10, p, p, None, None, None, None), "workspace")
    refused(L.soar_mesh_texture_write(0, 64, p, p, p, None, None), "count=0")
    refused(L.soar_mesh_texture_write(10, 20, p, p, p, None, None), "texture_size=20")
    refused(L.soar_mesh_texture_write(64 * 64 + 1, 64, p, p, p, None, None), "count=4097")
    refused(L.soar_mesh_texture_write(2 ** 31 - 1, 16384, p, p, p, None, None), "count=2147483647")
    refused(L.soar_mesh_texture_write(10, 64, p, None, p, None, None), "NULL")
