"""tests/mesh_cases.py against the restatements of tests/mesh_ref.py alone, on every case tests/test_mesh_gpu.py uses: each fusion
case keeps its ambiguous set under the cap and sees what it is built to see, the planted non-finite pixels are reached, the
marching-cubes fields have the crossings, ties and empty results they claim, and the filter cases keep what they should -- with the
kernel's float32 diagonals deciding as the float64 ones do."""
import numpy as np
import pytest
import torch

import mesh_cases as mc
import mesh_ref as R


# ---- fusion ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(mc.FUSION_CASES))
def test_fusion_case_stays_under_the_ambiguous_cap_and_sees_what_it_claims(name):
    case = mc.fusion_case(name)
    n, H, W, dims, _ = mc.FUSION_CASES[name]
    assert case.depth.shape == (n, H, W) and case.dims == dims and max(abs(o) for o in case.origin) == 1.0
    rs, rw, amb = mc.reference(case, R)
    share = float(amb.float().mean())
    print(f"{name}: ambiguous share {share:.4f}, observed {float((rw > 0).float().mean()):.3f}")
    assert share <= mc.AMBIGUOUS_CAP, f"{name}: {share:.3f} of the voxels are ambiguous: change the seed"
    band = (rw > 0) & ((rs / rw.clamp_min(1)).abs() < 1) & ~amb
    assert band.any() and ((rw > 0) & ~amb).float().mean() > 0.5       # observed voxels and band voxels outside the ambiguous set
    z = mc.view_z(case)
    if name == "offcube":
        X, Y, Z = dims
        assert len({Y * Z, Z, 1}) == 3 and X != Y != Z != X and (X * Y * Z) % 256 != 0
        assert len(torch.unique(rw[~amb])) >= 4                        # voxels seen by different numbers of views
    if name == "thin":
        assert 1 in dims
    if name == "inside":
        assert case.near_views == [1, 3, 5]
        for k in case.near_views:                                       # behind the camera, nearer than znear, and in front of it
            assert (z[k] < 0).any() and ((z[k] > 0) & (z[k] <= mc.ZNEAR)).any() and (z[k] > mc.ZNEAR).any()
            assert float(case.depth[k].min()) >= 0.2 and float(case.depth[k].max()) <= 0.8
        assert ((rw == 0) & ~amb).any()                                 # a voxel no view observes
        near_only = mc.SimpleNamespace(**{**vars(case), "depth": case.depth[1::2], "opac": case.opac[1::2], "viewm": case.viewm[1::2],
                                          "projm": case.projm[1::2], "prcp": case.prcp[1::2], "n": 3})
        assert (mc.reference(near_only, R)[1] > 0).any()                # the near cameras do observe voxels
    else:
        assert (z > mc.ZNEAR).all()                                     # every camera outside the grid


def test_chunk_case_needs_the_single_view_comparison():
    case = mc.fusion_case("chunk")
    assert case.n == 130 > 2 * 64 and mc.CHUNK_VIEW >= 64
    _, _, amb = mc.reference(case, R)
    assert amb.float().mean() > mc.AMBIGUOUS_CAP                        # all views at once: no per-voxel comparison with float64
    rs, rw, amb = mc.reference(mc.one_view(case, mc.CHUNK_VIEW), R)
    assert amb.float().mean() <= mc.AMBIGUOUS_CAP and ((rw > 0) & ~amb).any()
    # the views differ: fusing view 0 in the place of view CHUNK_VIEW gives another field
    rs0, rw0, _ = mc.reference(mc.one_view(case, 0), R)
    assert not torch.equal(rs0, rs)


def test_every_planted_kind_is_reached():
    case = mc.fusion_case("offcube")
    cols = [c + k for _, _, _, c in mc.NONFINITE_KINDS for k in range(case.n)]
    assert min(cols) >= 0 and max(cols) < case.W and len({c for _, _, _, c in mc.NONFINITE_KINDS}) == 6
    rs, rw, amb = mc.reference(case, R)
    ps, pw, pamb = mc.reference(mc.plant_nonfinite(case), R)
    assert pamb.float().mean() <= mc.AMBIGUOUS_CAP
    assert not ps.isnan().any() and not pw.isnan().any() and not ps.isinf().any()
    for name, plane, value, _ in mc.NONFINITE_KINDS:
        ks, kw, kamb = mc.reference(mc.plant_nonfinite(case, (name,)), R)
        ok = ~(amb | kamb)
        changed = ok & ((ks != rs) | (kw != rw))
        assert changed.any(), name
        if name in ("depth nan", "opac nan", "depth -inf"):             # no observation / hidden: weights only ever go down
            assert (kw <= rw)[ok].all() and (kw < rw)[ok].any(), name
        if name == "depth nan":                                         # ... but a NaN depth under a free-space pixel still counts
            p = mc.plant_nonfinite(case, (name,))
            assert (p.depth.isnan() & (p.opac < mc.MIN_OPACITY)).any() and (p.depth.isnan() & (p.opac >= mc.MIN_OPACITY)).any()
        if name == "depth +inf":
            assert (kw >= rw)[ok].all() and (ks >= rs)[ok].all()


# ---- marching cubes -------------------------------------------------------------------------------------------------------------

def test_marching_cubes_fields():
    shapes = [mc.mc_field(o)[0].shape for o in mc.MC_AXES]
    assert shapes == [(5, 33, 70), (70, 5, 33), (33, 70, 5)]
    f, m = mc.mc_field("xyz")
    g, gm = mc.mc_field("zxy")
    assert g[7, 2, 3] == f[2, 3, 7] and gm[7, 2, 3] == m[2, 3, 7] and 0.05 < 1 - m.mean() < 0.15
    assert f.size <= 15000
    for shape in mc.MC_SIZE_GRIDS + mc.MC_FLAT_GRIDS + [mc.MC_TIE_GRID]:
        assert int(np.prod(shape)) <= 15000
    assert [int(np.prod(s)) for s in mc.MC_SIZE_GRIDS] == [255, 256, 257]


@pytest.mark.parametrize("order", ["zxy", "yzx"])
def test_axis_orders_give_the_same_vertex_set_and_face_count(order):
    """the property the GPU test asks of the kernel, here of the table driver on a slab of the field (the driver is pure Python)"""
    f, m = mc.mc_field("xyz")
    g, gm = mc.mc_field(order)
    cut = tuple(slice(0, 5 if d == 5 else 9) for d in f.shape)
    gcut = tuple(cut[a] for a in mc.MC_AXES[order])
    v, fc = R.marching_cubes(f[cut], 0.25, m[cut])
    gv, gf = R.marching_cubes(g[gcut], 0.25, gm[gcut])
    assert len(fc) == len(gf) == R.table_face_count(f[cut], 0.25, m[cut]) > 0
    assert np.array_equal(mc.sorted_rows(v).view(np.int32), mc.sorted_rows(mc.mc_unpermute(gv, order)).view(np.int32))


@pytest.mark.parametrize("negative_zeros", [False, True])
def test_tie_fields_have_vertices_on_grid_points_and_flat_triangles(negative_zeros):
    f = mc.mc_ties(negative_zeros)
    assert set(np.unique(f).tolist()) == {-1.0, 0.0, 1.0} and bool(np.signbit(f[f == 0]).any()) == negative_zeros
    v, fc = R.marching_cubes(f)
    assert len(fc) == R.table_face_count(f) > 0
    on_grid = (v == np.floor(v)).all(1)
    assert on_grid.any() and not on_grid.all()                          # t = 0 or 1 on some edges, 0.5 on others
    assert not np.signbit(v).any()
    tri = v[fc].astype(np.float64)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
    assert (area == 0).any()
    same = R.marching_cubes(np.where(f == 0, np.float32(0.0), f))
    assert np.array_equal(v.view(np.int32), same[0].view(np.int32)) and np.array_equal(fc, same[1])     # -0.0 decides as 0.0


def test_flat_and_empty_fields():
    for shape in mc.MC_FLAT_GRIDS:
        v, fc = R.marching_cubes(mc.mc_random(shape, 320))
        assert len(v) > 0 and fc.shape == (0, 3) and R.table_face_count(mc.mc_random(shape, 320)) == 0
    f = np.abs(mc.mc_random((6, 7, 8), 321)) + 0.5
    v, fc = R.marching_cubes(f)
    assert v.shape == (0, 3) and fc.shape == (0, 3)
    one = np.zeros(f.shape, bool)
    one[2, 3, 4] = True
    for valid in (np.zeros(f.shape, bool), one):
        v, fc = R.marching_cubes(mc.mc_random(f.shape, 322), 0.0, valid)
        assert v.shape == (0, 3) and fc.shape == (0, 3)


def test_table_face_count_is_the_drivers():
    f, m = mc.mc_random((7, 6, 9), 323), np.random.default_rng(324).uniform(size=(7, 6, 9)) > 0.1
    for level, valid in ((0.0, None), (0.25, m)):
        assert R.table_face_count(f, level, valid) == len(R.marching_cubes(f, level, valid)[1]) > 0


# ---- the component filter -------------------------------------------------------------------------------------------------------

def _restated(case):
    """the restatement with float64 diagonals, after checking that the kernel's float32 diagonals decide the same"""
    v, f = R.filter_components(case.verts, case.faces, case.min_faces, case.min_diag_frac)
    v32, f32 = R.filter_components(case.verts, case.faces, case.min_faces, case.min_diag_frac, diag=R.box_diag32)
    assert np.array_equal(v, v32) and np.array_equal(f, f32), "float32 and float64 diagonals decide differently"
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape[1:] == (3,) and f.shape[1:] == (3,)
    return v, f


def _keeps_what_it_should(case):
    v, f = _restated(case)
    assert case.faces.min() >= 0 and case.faces.max() < len(case.verts)
    assert np.array_equal(v, case.verts[case.keep_v]) and len(f) == int(case.keep_f.sum())
    new_id = np.cumsum(case.keep_v) - 1
    assert np.array_equal(f, new_id[case.faces[case.keep_f]])
    return v, f


@pytest.mark.parametrize("min_faces", mc.FAN_MIN_FACES)
def test_fans_stay_from_min_faces_on(min_faces):
    case = mc.fans_case(min_faces)
    assert len(case.faces) == 2 * sum(range(1, 131)) and len(case.verts) == len(case.faces) + 2 * 260
    v, f = _keeps_what_it_should(case)
    assert len(f) == 2 * sum(k for k in range(1, 131) if k >= min_faces)
    if min_faces == 1:
        # mixed waves: almost every run of 64 faces (and of 64 vertices) holds several components
        label, *_ = R.component_stats(case.verts, case.faces)
        runs = [len(set(label[case.faces[i:i + 64, 0]].tolist())) for i in range(0, len(case.faces), 64)]
        assert np.mean(np.array(runs) > 1) > 0.95


@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("strays", [False, True])
def test_boxes_at_the_threshold(permute, strays):
    case = mc.tie_case(permute, strays)
    label, used, labs, n_faces, lo, hi, glo, ghi = R.component_stats(case.verts, case.faces)
    assert int((~used).sum()) == (3 if strays else 0)
    assert np.array_equal(ghi - glo, np.array([12, 16, 0], np.float32)) and R.box_diag32(glo, ghi) == R.box_diag64(glo, ghi) == 20.0
    d32, d64 = R.box_diag32(lo, hi), R.box_diag64(lo, hi)
    assert int((d32 == 5).sum()) == 3 and int((d64 == 5).sum()) == 2           # the longer box's float32 diagonal rounds to 5
    assert int(((d64 < 5) & (d64 > 5 - 1e-6) & (d32 < 5)).sum()) == 1             # the shorter one: below 5 in both
    assert int(((d64 > 5) & (d64 < 5 + 1e-6)).sum()) == 1
    assert (lo.min(1) < 0).all()                                                  # every component has negative coordinates
    v, f = _keeps_what_it_should(case)
    plain = mc.tie_case(permute, False)
    pv, pf = _restated(plain)
    assert np.array_equal(v, pv) and np.array_equal(f, pf)                        # the strays change nothing
    if strays:                                                                    # ... and would, if they counted
        assert np.abs(case.verts[~used]).max() == 1000
        everything = R.box_diag64(case.verts.min(0), case.verts.max(0))
        assert (d64 < case.min_diag_frac * everything).all()


@pytest.mark.parametrize("shuffled", [False, True])
def test_strips_are_one_component_kept_whole(shuffled):
    case = mc.strip_case(shuffled)
    assert len(case.faces) == 20000
    if not shuffled:
        assert (np.diff(case.faces[:, 0]) == -1).all() and (case.faces[:, 0] > case.faces[:, 1]).all()
    label, used, labs, *_ = R.component_stats(case.verts, case.faces)
    assert used.all() and labs.tolist() == [0]
    v, f = _keeps_what_it_should(case)
    assert np.array_equal(v, case.verts) and np.array_equal(f, case.faces)


def test_single_triangle():
    _keeps_what_it_should(mc.single_triangle())


@pytest.mark.parametrize("V,F,seed", mc.SIZED_CASES)
def test_sized_meshes(V, F, seed):
    case = mc.sized_case(V, F, seed)
    assert case.verts.shape == (V, 3) and case.faces.shape == (F, 3) and case.faces.min() >= 0 and case.faces.max() < V
    v, f = _restated(case)
    label, used, labs, n_faces, lo, hi, glo, ghi = R.component_stats(case.verts, case.faces)
    rel = np.abs(R.box_diag64(lo, hi) / R.box_diag64(glo, ghi) - case.min_diag_frac)
    assert rel.min() > 1e-4, "a component sits on the diagonal threshold: change the seed"
    if F >= 255:
        assert case.twice > 0 and (case.faces[:, 0] == case.faces[:, 1]).sum() == case.twice
    if min(V, F) >= 255:
        assert 0 < len(v) < int(used.sum()) and 0 < len(f) < F                 # some components stay, some go
        small, short = n_faces < case.min_faces, R.box_diag64(lo, hi) < case.min_diag_frac * R.box_diag64(glo, ghi)
        assert (small & ~short).any() and (short & ~small).any()               # each criterion decides alone somewhere
        assert not used.all()
