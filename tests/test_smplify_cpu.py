"""CPU tests of the keypoint fitting (soar_amd/smplify.py, csrc/smplify.hip): the restatement of tests/smplify_ref.py against the
golden run of the reference's own objective, the gathered sub-model against the full model bit for bit, the rig's index checks,
the host readers and the exported symbols.  Nothing is launched."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import smplify_ref as sr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def golden():
    g = np.load(os.path.join(HERE, "golden", "smplify.npz"))
    params, init, tables = sr.golden_inputs(g)
    return g, sr.golden_model(g), params, init, tables


def golden_call(g):
    t = lambda k: torch.from_numpy(g[k])
    return dict(Ks=t("Ks"), w2c=t("w2c"), img_wh=tuple(int(x) for x in g["img_wh"]), target_kps=t("target_kps"), scales=t("target_scales"),
                weights=tuple(float(x) for x in g["weights"]), sigma=float(g["sigma"]))


def test_golden_holds_the_cases_it_promises():
    g, m, p, i, tables = golden()
    assert p["transl"].shape == (5, 3) and m.v_template.shape == (96, 3) and m.lmk_faces_idx.numel() == 51 + 17
    assert len(set(m.extra_joints_idxs.tolist()) & set(m.faces_tensor[m.lmk_faces_idx].reshape(-1).tolist())) >= 1     # a shared vertex
    assert max(tables[0]) < 55 + 21 + 68 and len(tables[0]) == len(tables[1]) == 123
    kz = sr.model_points(m, sr.full_rotations({k: v.double() for k, v in p.items()}, False),
                         torch.cat([p["betas"].expand(5, -1), p["expression"]], -1).double(), p["transl"].double())
    kc = torch.einsum("ij,nkj->nki", torch.from_numpy(g["w2c"]).double()[:3],
                      torch.nn.functional.pad(sr.convert_kps(kz, tables[0], tables[1]), (0, 1), value=1.0))
    z = torch.einsum("nij,nkj->nki", torch.from_numpy(g["Ks"]).double(), kc)[..., 2]
    assert int((z[3] < 1e-5).sum()) >= 1 and int((z[[0, 1, 2, 4]] < 1e-5).sum()) == 0                        # under the clamp
    assert int((torch.from_numpy(g["target_kps"])[..., 2] == 0).sum()) > 50                                   # zero confidences
    assert all(torch.equal(p[k][2], p[k][1]) for k in sr.POSE_KEYS)                                           # smooth angle 0
    assert torch.equal(p["body_pose"][1, 4], i["body_pose"][1, 4]) and torch.equal(p["transl"][2], i["transl"][2])   # preserve norm 0
    for ih in (0, 1):
        for k in sr.GRAD_KEYS:
            assert np.isfinite(g[f"g_{k}_f64_ih{ih}"]).all() and np.abs(g[f"g_{k}_f64_ih{ih}"]).max() > 0


@pytest.mark.parametrize("ignore_hands", [False, True])
def test_float64_restatement_reproduces_the_reference(ignore_hands):
    g, m, p, i, tables = golden()
    tag = f"f64_ih{int(ignore_hands)}"
    ls, gr = sr.objective(m, tables, p, i, **golden_call(g), ignore_hands=ignore_hands, detour=True)
    for n, k in enumerate(("kp", "preserve", "smooth")):
        assert abs(float(ls[k]) - g[f"loss_{tag}"][n]) <= 1e-9 * abs(g[f"loss_{tag}"][n]), k
    for k in sr.GRAD_KEYS:
        assert gr[k].shape == g[f"g_{k}_{tag}"].shape
        assert sr.worst(gr[k].numpy(), g[f"g_{k}_{tag}"]) <= 1e-9, k
    kps = sr.keypoints(m, tables, {k: v.double() for k, v in p.items()}, torch.from_numpy(g["Ks"]).double(),
                       torch.from_numpy(g["w2c"]).double(), detour=True)
    assert sr.worst(kps.numpy(), g[f"kps_{tag}"]) <= 1e-9
    # the identity detour that the kernels skip moves nothing above 1e-6 of a tensor's largest value
    _, gr0 = sr.objective(m, tables, p, i, **golden_call(g), ignore_hands=ignore_hands, detour=False)
    assert max(sr.worst(gr0[k].numpy(), g[f"g_{k}_{tag}"]) for k in sr.GRAD_KEYS) <= 1e-7
    # the float32 composition sits where the reference's own float32 run sits
    _, g32 = sr.objective(m, tables, p, i, **golden_call(g), ignore_hands=ignore_hands, detour=True, dtype=torch.float32)
    for k in sr.GRAD_KEYS:
        ref = sr.worst(g[f"g_{k}_f32_ih{int(ignore_hands)}"], g[f"g_{k}_{tag}"])
        assert sr.worst(g32[k].numpy(), g[f"g_{k}_{tag}"]) <= 4 * max(ref, sr.FLOOR), k


def test_hand_confidences_matter_and_the_smooth_term_of_one_frame_is_zero():
    g, m, p, i, tables = golden()
    assert abs(g["loss_f64_ih0"][0] - g["loss_f64_ih1"][0]) > 1.0
    one = lambda d: {k: (v if k == "betas" else v[:1]) for k, v in d.items()}
    c = golden_call(g)
    c.update(Ks=c["Ks"][:1], target_kps=c["target_kps"][:1], scales=c["scales"][:1])
    ls, gr = sr.objective(m, tables, one(p), one(i), **c)
    assert float(ls["smooth"]) == 0.0 and all(torch.isfinite(v).all() for v in gr.values())


def test_gathered_sub_model_equals_the_full_model_bit_for_bit():
    g, m, p, i, tables = golden()
    for dt in (torch.float64, torch.float32):
        q = {k: v.to(dt) for k, v in p.items()}
        Ks, w2c = torch.from_numpy(g["Ks"]).to(dt), torch.from_numpy(g["w2c"]).to(dt)
        full = sr.keypoints(m, tables, q, Ks, w2c, exact=True)
        sub = sr.keypoints(m, tables, q, Ks, w2c, exact=True, gather=True)
        assert torch.equal(full, sub)
    used = sr.used_vertices(m)
    assert used.numel() < 96 and used.unique().numel() == used.numel() and bool((used[1:] > used[:-1]).all())


def test_rig_checks_every_index_on_the_host():
    from soar_amd import smplify
    g, m, p, i, (src, dst, mask) = golden()
    base = dict(v_template=m.v_template, shapedirs=m.shapedirs, posedirs=m.posedirs, J_regressor=m.J_regressor, parents=m.parents,
                lbs_weights=m.lbs_weights, faces=m.faces_tensor, lmk_faces_idx=m.lmk_faces_idx, lmk_bary_coords=m.lmk_bary_coords,
                extra_joints_idxs=m.extra_joints_idxs, src_inds=src, dst_inds=dst, kp_mask=mask, device="cpu")

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            smplify.KeypointRig(**{**base, **kw})
    bad("src_inds", src_inds=[55 + 21 + 68] + src[1:])
    bad("src_inds", src_inds=[-1] + src[1:])
    bad("dst_inds", dst_inds=[137] + dst[1:])
    bad("written twice", dst_inds=[dst[1]] + dst[1:])
    bad("faces", faces=torch.where(m.faces_tensor == m.faces_tensor.max(), torch.tensor(96), m.faces_tensor))
    bad("lmk_faces_idx", lmk_faces_idx=torch.cat([m.lmk_faces_idx[:-1], torch.tensor([60])]))
    bad("extra_joints_idxs", extra_joints_idxs=torch.cat([m.extra_joints_idxs[:-1], torch.tensor([-3])]))
    bad("parents", parents=torch.cat([m.parents[:-1], torch.tensor([54])]))
    bad("one length", src_inds=src[:-1])
    bad("kp_mask", kp_mask=mask[:-1])
    # valid tables pass every check and then ask for a HIP device: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smplify.KeypointRig(**base)


def test_readers_round_trip(tmp_path):
    from soar_amd import smplify
    rng = np.random.default_rng(3)
    kp_dir, sx_dir = tmp_path / "keypoints", tmp_path / "smplx"
    kp_dir.mkdir()
    sx_dir.mkdir()
    want = rng.random((3, 137, 3)).astype(np.float32)
    sizes = {"betas": (1, 10), "global_orient": (1, 3), "body_pose": (21, 3), "left_hand_pose": (15, 3), "right_hand_pose": (15, 3),
             "jaw_pose": (1, 3), "leye_pose": (1, 3), "reye_pose": (1, 3), "expression": (1, 10), "transl": (1, 3)}
    est = [{k: rng.standard_normal(s).astype(np.float32) for k, s in sizes.items()} for _ in range(3)]
    for n in range(3):
        flat = lambda a, b: want[n, a:b].reshape(-1).tolist()
        person = {"pose_keypoints_2d": flat(0, 25), "hand_left_keypoints_2d": flat(25, 46), "hand_right_keypoints_2d": flat(46, 67),
                  "face_keypoints_2d": flat(67, 137)}
        (kp_dir / f"{n:05d}_keypoints.json").write_text(json.dumps({"people": [person, {"pose_keypoints_2d": []}]}))
        np.savez(sx_dir / f"{n:05d}_0.npz", **est[n])
    got = smplify.load_keypoints(str(kp_dir))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    sx = smplify.load_smplerx(str(sx_dir))
    assert {k: tuple(v.shape) for k, v in sx.items()} == {k: (3, int(np.prod(s))) for k, s in sizes.items()}
    assert all(np.array_equal(sx[k][n].numpy(), est[n][k].reshape(-1)) for k in sizes for n in range(3))
    with pytest.raises(FileNotFoundError):
        smplify.load_keypoints(str(sx_dir))
    # params.pth: the reference's keys
    path = tmp_path / "params.pth"
    smplify.save_params(str(path), sx, torch.eye(3)[None].repeat(3, 1, 1), torch.eye(4), (640, 480))
    back = torch.load(str(path))
    assert set(back) == set(sizes) | {"Ks", "w2c", "img_wh"} and back["img_wh"] == (640, 480)
    assert torch.equal(back["body_pose"], sx["body_pose"]) and back["Ks"].shape == (3, 3, 3)
    # rotation vectors survive the trip through the 6-D form the optimiser works in, near 0 and near pi too
    rv = torch.tensor([[0.3, -0.2, 0.9], [0.0, 0.0, 0.0], [1e-5, 0.0, 0.0], [0.0, 3.1, 0.3], [2.2, -2.2, 0.1]], dtype=torch.float64)
    out = smplify.rotmat_to_rotvec(smplify.rotation_6d_to_matrix(smplify.rotation_6d_from_rotvec(rv)))
    assert float((out - rv).abs().max()) <= 1e-9


def test_symbols_are_exported_and_refuse_bad_arguments():
    from soar_amd import build, hip_lib, smplify
    build.build()
    L = hip_lib.lib()
    header = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    for name in ("soar_smplify_objective", "soar_smplify_target_scales"):
        assert name in hip_lib.SIGNATURES and name in header and hasattr(L, name)
    assert "smplify.hip" in build.SOURCES and hip_lib.ABI_VERSION == 8 == L.soar_abi_version()
    for name in ("KeypointRig", "smplify_objective", "project_keypoints", "target_scales", "SMPLify", "save_params", "load_keypoints",
                 "load_smplerx"):
        assert hasattr(smplify, name)
    assert C.sizeof(hip_lib.SoarSmplifyRig) == 24 + 12 * 8 and C.sizeof(hip_lib.SoarSmplifyArgs) == 16 + 24 * 8 + 14 * 4 + 10 * 8
    assert L.soar_smplify_objective(None, None, None) == 1 and "NULL" in hip_lib.last_error()
    rig, args = hip_lib.SoarSmplifyRig(), hip_lib.SoarSmplifyArgs()
    rig.J, rig.NBS, rig.NE, rig.VS, rig.P = 55, 10, 10, 300, 10
    assert L.soar_smplify_objective(C.byref(rig), C.byref(args), None) == 1 and "VS" in hip_lib.last_error()
    rig.VS, rig.J = 77, 24
    assert L.soar_smplify_objective(C.byref(rig), C.byref(args), None) == 1
    rig.J, args.N = 55, 4
    assert L.soar_smplify_objective(C.byref(rig), C.byref(args), None) == 1 and "NULL rig table" in hip_lib.last_error()
    assert L.soar_smplify_target_scales(-1, None, 1.0, 1.0, None, None) == 1
    assert L.soar_smplify_target_scales(3, None, 1.0, 1.0, None, None) == 1 and "NULL" in hip_lib.last_error()
    assert L.soar_smplify_target_scales(0, None, 1.0, 1.0, None, None) == 0
