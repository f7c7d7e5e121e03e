"""CPU tests of the normal priors (soar_amd/prior.py, csrc/prior.hip): the definition as tests/prior_ref.py restates it on
hand-worked inputs, the topology's host checks, the refusals, the exported symbols, and the condition the GPU tests rely on (few
near-ties in their own inputs).  Nothing is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import prior_cases as pc
import prior_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def raster(px, faces, H, W, z=None, dtype=np.float64):
    """Triangles given in pixels (and depths): snapped = 256 x, unit normals along -z."""
    px = np.asarray(px, np.float64)
    snapped = np.rint(px * 256).astype(np.int64)
    z = np.ones(len(px)) if z is None else np.asarray(z, np.float64)
    nrm = np.tile(np.array([0.0, 0.0, -1.0]), (len(px), 1))
    return pr.rasterize(snapped, 1.0 / z, nrm, np.asarray(faces, np.int64), H, W, dtype)


def test_a_hand_worked_triangle_on_8x8():
    # (1, 1), (7, 1), (1, 7): the samples (j + 0.5, i + 0.5) with x >= 1, y >= 1 and x + y < 8 or, on the hypotenuse x + y = 8, owned
    # by the edge's direction.  The hypotenuse runs (7, 1) -> (1, 7): towards +y, so its samples belong to the face
    res = raster([(1, 1), (7, 1), (1, 7)], [(0, 1, 2)], 8, 8)
    want = sorted((i, j) for i in range(8) for j in range(8) if j + 0.5 >= 1 and i + 0.5 >= 1 and (j + 0.5) + (i + 0.5) <= 8)
    got = sorted(zip(*np.nonzero(res["mask"][0])))
    assert [tuple(int(x) for x in g) for g in got] == want
    assert len(want) == 6 + 5 + 4 + 3 + 2 + 1                       # rows 1 .. 6: columns 1 .. 7 - i
    assert (res["mask"][0] == res["mask"][1]).all() and (res["face"][0][res["mask"][0] == 1] == 0).all()
    # listed the other way round the hypotenuse runs towards -y ... after the swap of vertices 1 and 2 it is the same face
    rev = raster([(1, 1), (1, 7), (7, 1)], [(0, 1, 2)], 8, 8)
    assert (rev["mask"] == res["mask"]).all()
    # a left edge on sample centres (x = 1.5) runs towards -y in a face of positive area: not owned; the top edge (y = 1.5) runs
    # along +x: owned
    res = raster([(1.5, 1.5), (6.5, 1.5), (1.5, 6.5)], [(0, 1, 2)], 8, 8)
    assert res["mask"][0][1, 2] == 1 and res["mask"][0][1, 1] == 0 and res["mask"][0][2, 1] == 0


def test_a_shared_diagonal_through_pixel_centres_is_owned_exactly_once():
    quad = [(0.5, 0.5), (6.5, 0.5), (6.5, 6.5), (0.5, 6.5)]
    for faces in ([(0, 1, 2), (0, 2, 3)], [(0, 2, 1), (0, 2, 3)], [(2, 0, 1), (3, 0, 2)]):
        one, two = raster(quad, faces[:1], 8, 8), raster(quad, faces[1:], 8, 8)
        both = one["mask"][0].astype(int) + two["mask"][0].astype(int)
        assert all(both[i, i] == 1 for i in range(1, 6)), faces     # never both, never none
        assert both.max() == 1 and both[0, 0] == 0 and both[6, 6] == 0     # the ends lie on the square's left and bottom borders
        # the square's own border: the top row y = 0.5 (along +x) and the right column x = 6.5 (towards +y) are owned
        assert both[0, 3] == 1 and both[3, 6] == 1 and both[6, 3] == 0 and both[3, 0] == 0


def test_the_same_face_twice_the_lower_index_wins_in_both_views():
    tri = [(1, 1), (7, 1), (1, 7)]
    res = raster(tri, [(0, 1, 2), (0, 1, 2)], 8, 8, z=[2.0, 3.0, 4.0])
    on = res["mask"][0] == 1
    assert on.sum() == 21 and (res["face"][0][on] == 0).all() and (res["face"][1][on] == 0).all()
    assert np.isnan(res["q2"][0][on]).all()                        # and a copy is no runner-up
    # a nearer face in front of both: the front view takes it, the rear keeps index 0
    res = raster(tri + [(2, 2), (5, 2), (2, 5)], [(0, 1, 2), (0, 1, 2), (3, 4, 5)], 8, 8, z=[2.0, 3.0, 4.0, 1.0, 1.0, 1.0])
    assert res["face"][0][2, 2] == 2 and res["face"][1][2, 2] == 0


def test_a_negatively_oriented_face_equals_its_swapped_twin():
    px, z = [(1.2, 0.7), (6.9, 2.1), (2.4, 7.3)], [2.0, 2.5, 3.0]
    a, b = raster(px, [(0, 1, 2)], 8, 8, z=z, dtype=np.float32), raster(px, [(0, 2, 1)], 8, 8, z=z, dtype=np.float32)
    assert a["mask"][0].sum() > 10
    for k in ("mask", "face", "prior"):
        assert (a[k] == b[k]).all(), k
    assert (a["q"][a["mask"] == 1] == b["q"][b["mask"] == 1]).all()


def test_a_zero_area_face_and_a_face_behind_the_camera_cover_nothing():
    assert raster([(1, 1), (3, 3), (6, 6)], [(0, 1, 2)], 8, 8)["mask"].sum() == 0
    assert raster([(1, 1), (6, 1), (6, 1)], [(0, 1, 1)], 8, 8)["mask"].sum() == 0
    verts = np.array([[0, 0, 2], [1, 0, 2], [0, 1, -1], [0, 1, 2], [3e6, 0, 2]], np.float32)
    K = np.array([[4, 0, 4], [0, 4, 4], [0, 0, 1]], np.float32)
    faces = np.array([(0, 1, 2), (0, 1, 3), (0, 4, 3)])
    vs = pr.vertex_setup(verts, faces, np.eye(4), K)
    assert vs["valid"].tolist() == [True, True, False, True, False]
    assert vs["snapped"][2].tolist() == [pr.INVALID] * 2 and vs["inv_z"][2] == 0 and vs["snapped"][0].tolist() == [1024, 1024]
    res = pr.rasterize(vs["snapped"], vs["inv_z"], vs["normals"], faces, 8, 8)
    assert set(np.unique(res["face"])) == {-1, 1}                    # only the face in front and inside the guard band
    assert np.allclose(vs["normals"][3], [0, 0, 1]) and res["mask"][0][4, 4] == 1


def test_csr_table_of_a_small_mesh_with_an_unused_vertex():
    from soar_amd.prior import MeshTopology
    faces = [(0, 1, 2), (2, 1, 4), (4, 0, 2)]                        # vertex 3 is unused
    topo = MeshTopology(torch.tensor(faces), 5)
    assert topo.csr_offsets.tolist() == [0, 2, 4, 7, 7, 9]
    assert topo.csr_corners.tolist() == [0, 7, 1, 4, 2, 3, 8, 5, 6]
    off, cor = pr.csr(faces, 5)
    assert off.tolist() == topo.csr_offsets.tolist() and cor.tolist() == topo.csr_corners.tolist()
    assert topo.faces.dtype == topo.csr_corners.dtype == topo.csr_offsets.dtype == torch.int32 and topo.device.type == "cpu"
    v, f = pc.torus(5, 4)
    t2 = MeshTopology(f, v.shape[0])
    off, cor = pr.csr(f, v.shape[0])
    assert off.tolist() == t2.csr_offsets.tolist() and cor.tolist() == t2.csr_corners.tolist()
    assert MeshTopology(np.zeros((0, 3), np.int64), 3).csr_offsets.tolist() == [0, 0, 0, 0]


def test_mesh_topology_names_a_bad_index():
    from soar_amd.prior import MeshTopology
    with pytest.raises(ValueError, match=r"face 1 corner 2 has vertex index 5, outside \[0, 5\)"):
        MeshTopology(torch.tensor([(0, 1, 2), (2, 1, 5)]), 5)
    with pytest.raises(ValueError, match="face 0 corner 0 has vertex index -1"):
        MeshTopology(np.array([(-1, 1, 2)]), 5)
    with pytest.raises(ValueError, match=r"\[F,3\]"):
        MeshTopology(torch.zeros(4, 2, dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="integers"):
        MeshTopology(torch.zeros(4, 3), 5)


def test_cpu_tensors_and_bad_shapes_are_refused_without_a_launch():
    from soar_amd import prior
    topo = prior.MeshTopology(torch.tensor([(0, 1, 2)]), 3)
    K, eye = torch.eye(3).expand(2, 3, 3), torch.eye(4)
    with pytest.raises(RuntimeError, match="soar_amd.prior runs on HIP devices only; there is no CPU fallback"):
        prior.render_normal_priors(topo, torch.zeros(2, 3, 3), eye, K)
    with pytest.raises(ValueError, match=r"verts must be \[N,3,3\]"):
        prior.render_normal_priors(topo, torch.zeros(2, 4, 3), eye, K)
    with pytest.raises(ValueError, match="space"):
        prior.render_normal_priors(topo, torch.zeros(2, 3, 3), eye, K, space="blender")
    with pytest.raises(TypeError, match="MeshTopology"):
        prior.render_normal_priors(None, torch.zeros(2, 3, 3), eye, K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prior.estimate_normals_from_body(None, torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.uint8), K,
                                         torch.zeros(2, 3, 3), topo, eye)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prior.body_normal_priors(None, {k: torch.zeros(2, 3) for k in ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose",
                                                                        "left_hand_pose", "right_hand_pose", "betas", "expression", "transl")},
                                 K, eye, topo)
    assert prior.full_pose({k: torch.full((2, n), float(i)) for i, (k, n) in enumerate(
        (("global_orient", 3), ("body_pose", 63), ("jaw_pose", 3), ("leye_pose", 3), ("reye_pose", 3), ("left_hand_pose", 45),
         ("right_hand_pose", 45)))}).shape == (2, 165)


def test_the_c_calls_refuse_bad_arguments_without_a_launch():
    from soar_amd import build, hip_lib
    build.build()
    L = hip_lib.lib()
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)
    st = (C.c_int64 * 3)(9, 3, 1)
    assert L.soar_prior_vertex_setup(-1, 3, 1, p, st, p, 0, p, p, p, p, p, p, p, None) != 0 and "N must be" in hip_lib.last_error()
    assert L.soar_prior_vertex_setup(1, 0, 1, p, st, p, 0, p, p, p, p, p, p, p, None) != 0 and "V" in hip_lib.last_error()
    assert L.soar_prior_vertex_setup(1, 3, 1, None, st, p, 0, p, p, p, p, p, p, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert L.soar_prior_vertex_setup(0, 3, 1, None, st, p, 0, p, p, p, p, p, p, p, None) == 0
    assert L.soar_prior_face_boxes(1, 3, 1 << 25, p, p, p, None) != 0 and "F" in hip_lib.last_error()
    assert L.soar_prior_face_boxes(1, 3, 1, p, None, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert L.soar_prior_face_boxes(0, 3, 1, None, None, None, None) == 0 and L.soar_prior_face_boxes(1, 3, 0, None, None, None, None) == 0
    assert L.soar_prior_raster(1, 3, 1, 0, 8, 1, p, p, p, p, p, p, p, p, None) != 0 and "H and W" in hip_lib.last_error()
    assert L.soar_prior_raster(1, 3, 1, 8, 5000, 1, p, p, p, p, p, p, p, p, None) != 0
    assert L.soar_prior_raster(1, 3, 1, 8, 8, 1, p, p, p, p, None, p, p, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert L.soar_prior_raster(1, 3, 1, 8, 8, 1, p, p, p, p, p, None, p, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert L.soar_prior_raster(0, 3, 1, 8, 8, 1, None, None, None, None, None, None, None, None, None) == 0


def test_symbols_sources_and_abi_version():
    from soar_amd import build, hip_lib
    assert "prior.hip" in build.SOURCES and build.EXTRA_FLAGS["prior.hip"] == ["-ffp-contract=off"]
    assert {"soar_prior_vertex_setup", "soar_prior_face_boxes", "soar_prior_raster"} <= set(hip_lib.SIGNATURES)
    header = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    assert "int soar_prior_vertex_setup(" in header and "int soar_prior_face_boxes(" in header and "int soar_prior_raster(" in header and "#define SOAR_HIP_ABI_VERSION 8" in header
    assert hip_lib.ABI_VERSION == 8
    assert "soar_amd.prior" in open(os.path.join(ROOT, "__graft_entry__.py")).read()


def case_oracle(name, quad=True):
    c = pc.make_case(name, quad)
    vs = pr.vertex_setup(c["verts"], c["faces"], c["w2c"], c["K"], np.float32)       # the snapped vertices a float32 setup gives
    v64 = pr.vertex_setup(c["verts"], c["faces"], c["w2c"], c["K"], np.float64)
    return c, vs, v64, pr.rasterize(vs["snapped"], v64["inv_z"], v64["normals"], c["faces"], c["H"], c["W"])


@pytest.mark.parametrize("name", list(pc.CASES))
def test_the_gpu_cases_hold_what_they_promise_and_few_near_ties(name):
    """The condition the GPU tests rely on, on their own inputs: at most 0.5 % of the covered pixels of each view have their best and
    second-best q within 1e-5 relative (measured here: 0 of every case's pixels in both views but for single pixels)."""
    c, vs, v64, res = case_oracle(name)
    H, W, F = c["H"], c["W"], c["faces"].shape[0]
    assert (vs["valid"] == v64["valid"]).all() and int((~vs["valid"]).sum()) == 2          # behind the camera, past the guard band
    # the collinear face and the needle that reaches past the guard band (7 pixels wide, 2^22 long): no normal to compare
    assert int((~v64["well"]).sum()) == 6 and (v64["well"] == vs["well"]).all()
    ok = vs["valid"]
    assert np.abs(vs["snapped"][ok] - v64["xy"][ok] * 256).max() <= 1.0
    assert np.abs(v64["xy"][ok]).max() <= 4096 and vs["snapped"][ok].min() < -256          # float32 resolves 1/256 px there; negative coordinates
    assert (res["mask"] == 1).all()                                                        # the quad fills both views
    ties = pr.near_ties(res)
    for view in (0, 1):
        covered, n = int((res["face"][view] >= 0).sum()), int(ties[view].sum())
        print(f"{name} view {view}: {n} near-ties of {covered} covered pixels")
        assert n <= 0.005 * covered
    # the front view shows the body, some border faces and copies' originals; the rear view the quad
    front = set(np.unique(res["face"][0]).tolist())
    assert set(np.unique(res["face"][1]).tolist()) <= {F0q for F0q in (c["copies_of"][-1] - 1, c["copies_of"][-1])}
    assert len(front & set(c["copies_of"])) >= 3 and max(front) < c["first_copy"]            # copies never win
    body_faces = c["copies_of"][-1] - 1
    assert len([f for f in front if f >= body_faces + 2]) >= 5                               # the faces across the borders and the corner
    # the faces the busiest 32-pixel tile queues: those whose box of samples (prior_ref.face_boxes) meets it
    bx = pr.face_boxes(vs["snapped"], c["faces"])
    assert (bx[c["first_copy"] - 15:c["first_copy"] - 11, 0] > bx[c["first_copy"] - 15:c["first_copy"] - 11, 1]).sum() == 0      # outside, not empty
    hits = 0
    for ty in range(0, H, 32):
        for tx in range(0, W, 32):
            hits = max(hits, int(((bx[:, 0] <= min(tx + 32, W) - 1) & (bx[:, 1] >= tx) & (bx[:, 2] <= min(ty + 32, H) - 1) & (bx[:, 3] >= ty)).sum()))
    print(f"{name}: {F} faces, {hits} in the busiest tile")
    if name == "torus48x24_48x40":
        assert hits > 3 * 256                                                               # the ring is emptied more than once before the end, and wraps


def test_without_the_quad_the_rear_view_is_the_far_layer():
    c, vs, v64, res = case_oracle("torus24x12_96x80", quad=False)
    both = (res["face"][0] >= 0)
    assert (res["mask"][0] == res["mask"][1]).all() and 0.2 < both.mean() < 0.9
    assert (res["face"][0][both] != res["face"][1][both]).mean() > 0.9          # a closed surface: two layers but on its rim
    assert (res["q"][0][both] >= res["q"][1][both]).all()
    ties = pr.near_ties(res)
    assert ties[0].sum() <= 0.005 * both.sum() and ties[1].sum() <= 0.005 * both.sum()
