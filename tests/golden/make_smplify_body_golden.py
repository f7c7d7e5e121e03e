"""Generate ``smplify_body.npz`` by RUNNING the reference's own SMPLify objective on the body model the reference creates
(``use_face_contour=True``, ``flat_hand_mean=False``), where the reference tree is present.

Run once:  ``python tests/golden/make_smplify_body_golden.py <reference root>``.  Only inputs and outputs (data) are written; no
reference source is copied.

Made the way ``make_smplify_golden.py`` is: ``gmof``, ``compute_smooth_loss``, ``rotation_6d_to_matrix``,
``matrix_to_rotation_6d``, ``get_target_scales``, ``prepare_smplx_to_openpose137`` and the class ``SMPLify`` are cut out of
``preproc/utils.py`` with ``ast`` and executed as they stand.  The body model is the vendored ``lbs``, ``vertices2landmarks`` and
``find_dynamic_lmk_idx_and_bcoords`` (soar/threestudio-soar/utils/smplx/lbs.py) plus the vertex selector's gather, composed as
``SMPLX.forward`` composes them (body_models.py:1306-1383): ``full_pose += pose_mean``, ``lbs``, the per-frame contour rows
appended to the static landmarks, ``vertices2landmarks``.  ``roma`` is absent: ``rotmat_to_rotvec`` / ``rotvec_to_rotmat`` are this
project's (tests/smplify_ref.py), as in the first golden.

Model: seeded, V = 400, J = 55, NB = 10 + 10, 300 random faces, 51 static landmarks, 21 selected vertices, a random 79 x 17 contour
table (its distinct vertices are asserted to exceed 256), ``pose_mean`` non-zero on the 30 hand joints only.  N = 8 frames whose
float64 yaw of the neck's world rotation selects: frame 0 row 0; 1 a row in 1 .. 38; 2 row 39 by the clamp; 3 a row in 40 .. 77;
4 row 78 by the clamp; 5 the back-facing fold (the body turned by more than 90 degrees); 6 a row that comes from the spine and
neck rotations (the root alone would give another); 7 row 40 (y = -1).  Every frame's ``-e 180 / pi`` is asserted to lie at least
0.02 degrees from a half-integer.  ``rule_R`` / ``rule_rows``: rotations about y (``rule_angles`` degrees, exact half-degree yaws
among them) and the rows ``find_dynamic_lmk_idx_and_bcoords`` itself picks for them in float64.  Stored: the inputs, the reference's three tables, the rows, and for ``ignore_hands`` on and off
the three losses, every gradient by autograd and the projected keypoints, in float32 and in float64 on the same (float32) inputs.
Every float64 gradient is checked to be finite: pick another seed if not.
"""
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [OUT, os.path.join(OUT, "..", ".."), os.path.join(OUT, "..")]

SEED = 97531
NECK_CHAIN = (12, 9, 6, 3, 0)
# frame -> the yaw in degrees (what is rounded) the root is turned to reach; frame 6's comes from the spine instead
TARGETS = {0: (0.21, 1), 1: (17.3, 1), 2: (61.7, 1), 3: (-22.3, 1), 4: (-66.2, 1), 5: (21.4, -1), 7: (-0.7, 1)}     # (yaw, facing)


def main(ref):
    sys.path.insert(0, os.path.join(ref, "soar", "threestudio-soar", "utils"))
    import smplx.lbs as ref_lbs                                    # the vendored SMPL-X lbs module
    from smplx.utils import rot_mat_to_euler
    import body_ref
    import smplify_ref as sr
    import smplify_body_ref as sb
    from make_smplify_golden import reference_namespace
    from soar_amd import synthetic as syn
    ns = reference_namespace(ref, sr)

    g = torch.Generator().manual_seed(SEED)
    rn = lambda *s: torch.randn(*s, generator=g)
    V, J, NBS, NE, N, RANK, NF, L, LD, NX = 400, 55, 10, 10, 8, 8, 300, 51, 17, 21
    v_template, _ = syn.sample_capsule_surface(V, g)
    shapedirs = rn(V, 3, NBS + NE) * 5e-3
    U, Wt = rn((J - 1) * 9, RANK) * 0.1, rn(RANK, V * 3) * 0.05
    posedirs = torch.from_numpy(body_ref.posedirs_from_factors(U.numpy(), Wt.numpy()))
    jr = torch.rand(J, V, generator=g) ** 8
    J_regressor = jr / jr.sum(1, keepdim=True)
    parents = torch.tensor(syn.SMPLX_PARENTS)
    assert all(int(parents[a]) == b for a, b in zip(NECK_CHAIN[:-1], NECK_CHAIN[1:]))
    neck_kin_chain = torch.tensor(NECK_CHAIN)
    lbs_weights = torch.softmax(2.0 * rn(V, J), dim=1)
    faces = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(NF)])
    lmk_faces_idx = torch.randint(0, NF, (L,), generator=g)
    bary = torch.rand(L, 3, generator=g) + 0.05
    lmk_bary_coords = bary / bary.sum(1, keepdim=True)
    dyn_faces = torch.randint(0, NF, (79, LD), generator=g)
    dbary = torch.rand(79, LD, 3, generator=g) + 0.05
    dyn_bary = dbary / dbary.sum(-1, keepdim=True)
    assert torch.unique(faces[dyn_faces].reshape(-1)).numel() > 256                      # the union does not fit the old rig
    assert torch.unique(dyn_faces, dim=0).shape[0] == 79                                 # a row is recognised by its faces
    extra = torch.randperm(V, generator=g)[:NX]
    pose_mean = torch.zeros(J, 3)
    pose_mean[25:] = 0.25 * rn(30, 3)                                                    # the 30 hand joints
    pose_mean = pose_mean.reshape(-1)

    def random_6d(n, jk, lo=0.2, span=1.0):
        axis = F.normalize(rn(n, jk, 3), dim=-1)
        ang = lo + span * torch.rand(n, jk, 1, generator=g)        # away from 0 and pi
        R = sr.rotvec_to_rotmat(axis * ang)
        a1 = R[..., 0, :] * (0.7 + 0.6 * torch.rand(n, jk, 1, generator=g))        # not orthonormal: Gram-Schmidt has work to do
        a2 = R[..., 1, :] * (0.7 + 0.6 * torch.rand(n, jk, 1, generator=g)) + 0.3 * rn(n, jk, 1) * R[..., 0, :] + 0.05 * rn(n, jk, 3)
        return torch.cat([a1, a2], -1)

    sizes = {"global_orient": 1, "body_pose": 21, "left_hand_pose": 15, "right_hand_pose": 15}
    params = {k: random_6d(N, jk) for k, jk in sizes.items()}
    params["body_pose"] = random_6d(N, 21, 0.05, 0.45)             # moderate, so that a turned root is a turned head
    tilt = sr.rotvec_to_rotmat(0.15 * rn(N, 3)).double()
    # frame 6: the root is nearly upright and unturned, spine and neck turn the head
    spine = sb.y_rotation([-7.0, -9.0, -6.0, -8.0]) @ sr.rotvec_to_rotmat(0.03 * rn(4, 3)).double()
    for n_, j in enumerate((3, 6, 9, 12)):
        params["body_pose"][6, j - 1] = sr.matrix_to_rotation_6d(spine[n_]).float() * 1.2
    tilt[6] = sr.rotvec_to_rotmat(torch.tensor([[0.04, 0.0, -0.03]])).double()

    def neck_yaw(go6, bp6):
        """the float64 yaw in degrees of the float32 inputs, by the reference's own functions"""
        Rg = ns["rotation_6d_to_matrix"](go6.double())[:, 0]
        Rb = ns["rotation_6d_to_matrix"](bp6.double())
        rv = torch.stack([sr.rotmat_to_rotvec(Rb[:, j - 1]) for j in NECK_CHAIN[:-1]] + [sr.rotmat_to_rotvec(Rg)], 1)
        rot = ref_lbs.batch_rodrigues(rv.reshape(-1, 3)).reshape(rv.shape[0], -1, 3, 3)
        rel = torch.eye(3, dtype=torch.float64).repeat(rv.shape[0], 1, 1)
        for i in range(rot.shape[1]):
            rel = torch.bmm(rot[:, i], rel)
        return -rot_mat_to_euler(rel) * 180.0 / np.pi, rel

    # turn every root about y until the neck's yaw is the frame's target: a scan, then the closest angle
    grid = torch.arange(-180.0, 180.0, 0.01, dtype=torch.float64)
    go = torch.zeros(N, 1, 6)
    for f in range(N):
        if f in TARGETS:
            cand = sr.matrix_to_rotation_6d(sb.y_rotation(grid) @ tilt[f]).float()[:, None]                  # [G,1,6]
            yaw, rel = neck_yaw(cand, params["body_pose"][f:f + 1].expand(len(grid), -1, -1))
            want, facing = TARGETS[f]
            err = (yaw - want).abs() + (rel[:, 0, 0] * facing < 0.2) * 1e3                                   # towards the camera, or away
            go[f] = cand[int(err.argmin())]
        else:
            go[f] = sr.matrix_to_rotation_6d(tilt[f][None]).float()
    params["global_orient"] = go * (0.8 + 0.4 * torch.rand(N, 1, 1, generator=g))                            # not unit rows
    yaw, rel = neck_yaw(params["global_orient"], params["body_pose"])
    rows = sb.contour_row(rel)
    margin = ((yaw - 0.5) - torch.round(yaw - 0.5)).abs()                                                    # distance to a half-integer
    print("yaw", [f"{float(x):.4f}" for x in yaw], "rows", rows.tolist(), "margin", [f"{float(x):.3f}" for x in margin])
    assert float(margin.min()) >= 0.02
    root_rows = sb.contour_row(ns["rotation_6d_to_matrix"](params["global_orient"].double())[:, 0])
    assert int(rows[0]) == 0 and 1 <= int(rows[1]) <= 38 and int(rows[2]) == 39 and float(yaw[2]) > 39.5 and 40 <= int(rows[3]) <= 77
    assert int(rows[4]) == 78 and float(yaw[4]) < -39.5 and float(rel[5, 0, 0]) < 0 and int(rows[7]) == 40
    assert int(rows[6]) >= 10 and int(root_rows[6]) != int(rows[6]) and abs(int(root_rows[6]) - int(rows[6])) >= 10 and int(rows[6]) < 39

    # the row rule alone: rotations about y (degrees) through the reference's function, exact half-degree yaws among them
    rule_angles = torch.tensor([0.0, 10.2, -10.2, 38.6, 40.3, -39.6, -80.0, 120.0, 179.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 38.5, -38.5,
                                39.5, -39.5, 40.5, -0.2, 0.2, 89.0, -89.0, -150.0], dtype=torch.float64)
    rule_R = sb.y_rotation(rule_angles)
    K = len(rule_angles)
    one_face = torch.arange(79)[:, None]                            # a table whose row r names face r
    rule_rows, _ = ref_lbs.find_dynamic_lmk_idx_and_bcoords(torch.zeros(K, 1, 3, dtype=torch.float64), rule_R[:, None], one_face,
                                                            torch.zeros(79, 1, 3, dtype=torch.float64), torch.tensor([0]), pose2rot=False)
    rule_rows = rule_rows.reshape(K)
    assert rule_rows[:9].tolist() == [0, 49, 10, 78, 78, 39, 39, 78, 40], rule_rows.tolist()

    params.update(betas=rn(1, NBS) * 0.7, transl=0.1 * rn(N, 3), jaw_pose=0.2 * rn(N, 3), leye_pose=0.1 * rn(N, 3),
                  reye_pose=0.1 * rn(N, 3), expression=rn(N, NE) * 0.7)
    init = {k: v + 0.05 * rn(*v.shape) for k, v in params.items()}
    for k in sr.FIXED_KEYS:
        init[k] = params[k].clone()                                # the closure's fixed keys are clones of the initial values

    img_wh = (640, 480)
    w2c = torch.eye(4)
    w2c[:3, :3] = sr.rotvec_to_rotmat(torch.tensor([0.05, -0.1, 0.02]))
    w2c[:3, 3] = torch.tensor([0.05, 0.1, 3.0])
    Ks = torch.zeros(N, 3, 3)
    Ks[:, 0, 0], Ks[:, 1, 1] = 520.0 + 10.0 * rn(N), 515.0 + 10.0 * rn(N)
    Ks[:, 0, 2], Ks[:, 1, 2], Ks[:, 2, 2] = 320.0 + 5.0 * rn(N), 240.0 + 5.0 * rn(N), 1.0
    Ks[:, 0, 1] = 0.5 * rn(N)

    seen_rows = {}

    def body_model(dt):
        c = lambda t: t.to(dt)

        def run(betas, body_pose, global_orient, left_hand_pose, right_hand_pose, jaw_pose, leye_pose, reye_pose, expression, transl):
            B = global_orient.shape[0]
            full_pose = torch.cat([global_orient.reshape(-1, 1, 3), body_pose.reshape(-1, 21, 3), jaw_pose.reshape(-1, 1, 3),
                                   leye_pose.reshape(-1, 1, 3), reye_pose.reshape(-1, 1, 3), left_hand_pose.reshape(-1, 15, 3),
                                   right_hand_pose.reshape(-1, 15, 3)], dim=1).reshape(-1, 165)
            full_pose = full_pose + c(pose_mean)
            vertices, joints = ref_lbs.lbs(torch.cat([betas, expression], dim=-1), full_pose, c(v_template), c(shapedirs), c(posedirs),
                                           c(J_regressor), parents, c(lbs_weights), pose2rot=True)
            lf = lmk_faces_idx[None].expand(B, -1).contiguous()
            lb = c(lmk_bary_coords)[None].repeat(B, 1, 1)
            dlf, dlb = ref_lbs.find_dynamic_lmk_idx_and_bcoords(vertices, full_pose, dyn_faces, c(dyn_bary), neck_kin_chain, pose2rot=True)
            seen_rows[dt] = [int((dyn_faces == dlf[b][None]).all(1).nonzero()[0, 0]) for b in range(B)]
            landmarks = ref_lbs.vertices2landmarks(vertices, faces, torch.cat([lf, dlf], 1), torch.cat([lb, dlb], 1))
            joints = torch.cat([joints, torch.index_select(vertices, 1, extra)], dim=1)
            joints = torch.cat([joints, landmarks], dim=1)
            return types.SimpleNamespace(joints=joints + transl.unsqueeze(dim=1), vertices=vertices + transl.unsqueeze(dim=1))
        return run

    def pred_kps(fit, p, dt):
        with torch.no_grad():
            out = fit.body_model(**{k: (sr.rotmat_to_rotvec(ns["rotation_6d_to_matrix"](v)).reshape(*v.shape[:-1], -1) if k in sizes
                                        else (v if k != "betas" else v.repeat_interleave(N, dim=0))) for k, v in p.items()})
            kc = torch.einsum("ij,nkj->nki", w2c.to(dt)[:3], F.pad(fit.convert_kps(out.joints), (0, 1), value=1.0))
            q = torch.einsum("nij,nkj->nki", Ks.to(dt), kc)
            return q[..., :2] / q[..., 2:].clamp(min=1e-5), q[..., 2]

    fit64 = ns["SMPLify"](body_model(torch.float64))
    _, z = pred_kps(fit64, {k: v.double() for k, v in params.items()}, torch.float64)
    assert float(z.min()) > 0.5                                    # every keypoint in front of the camera: the clamp is the first golden's case
    uv0, _ = pred_kps(fit64, {k: v.double() for k, v in init.items()}, torch.float64)
    wh = torch.tensor(img_wh, dtype=torch.float32)
    target = torch.cat([((uv0.float() + 4.0 * rn(N, 137, 2)) / wh).clamp(-1.0, 2.0), torch.rand(N, 137, 1, generator=g)], -1)
    target[..., 2][torch.rand(N, 137, generator=g) < 0.2] = 0.0
    scales = ns["get_target_scales"](torch.cat([target[..., :-1] * target.new_tensor(img_wh), target[..., -1:]], dim=-1))

    out = {}
    worst = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        fit = ns["SMPLify"](body_model(dt))
        c = lambda t: t.to(dt)
        for ih in (0, 1):
            p = {k: c(v).clone().requires_grad_(k in sr.GRAD_KEYS) for k, v in params.items()}
            p0 = {k: c(v) for k, v in init.items()}
            opt = torch.optim.SGD([p[k] for k in sr.GRAD_KEYS], lr=0.0)
            fit.create_closure(opt, p, c(Ks), c(w2c), img_wh, c(target), c(scales), p0, ignore_hands=bool(ih))()
            assert seen_rows[dt] == rows.tolist(), (name, seen_rows[dt], rows.tolist())      # the reference's own selection, both dtypes
            tag = f"{name}_ih{ih}"
            out[f"loss_{tag}"] = np.array([float(fit.loss_dict[k].detach()) for k in ("kp", "preserve", "smooth")], np.float64)
            for k in sr.GRAD_KEYS:
                out[f"g_{k}_{tag}"] = p[k].grad.numpy()
                assert np.isfinite(out[f"g_{k}_{tag}"]).all(), (k, tag)
            out[f"kps_{tag}"] = pred_kps(fit, {k: v.detach() for k, v in p.items()}, dt)[0].numpy()
    for ih in (0, 1):
        for k in sr.GRAD_KEYS:
            a, b = out[f"g_{k}_f32_ih{ih}"], out[f"g_{k}_f64_ih{ih}"]
            worst[f"{k}_ih{ih}"] = float(np.abs(a - b).max() / np.abs(b).max())
    cell = dict(zip(fit64.convert_kps.__code__.co_freevars, (c.cell_contents for c in fit64.convert_kps.__closure__)))
    assert max(cell["src_inds"]) < 55 + NX + L + LD and len(cell["src_inds"]) == len(cell["dst_inds"])
    assert set(range(55 + NX + L, 55 + NX + L + LD)) <= set(cell["src_inds"])                # the tables do map the contour
    np.savez_compressed(
        os.path.join(OUT, "smplify_body.npz"), v_template=v_template.numpy(), shapedirs=shapedirs.numpy(), posedirs_U=U.numpy(),
        posedirs_Wt=Wt.numpy(), J_regressor=J_regressor.numpy(), parents=parents.numpy(), lbs_weights=lbs_weights.numpy(),
        faces=faces.numpy(), lmk_faces_idx=lmk_faces_idx.numpy(), lmk_bary_coords=lmk_bary_coords.numpy(),
        dynamic_lmk_faces_idx=dyn_faces.numpy(), dynamic_lmk_bary_coords=dyn_bary.numpy(), neck_kin_chain=neck_kin_chain.numpy(),
        pose_mean=pose_mean.numpy(), rows=rows.numpy(), yaw_degrees=yaw.numpy(), rule_angles=rule_angles.numpy(), rule_R=rule_R.numpy(),
        rule_rows=rule_rows.numpy(),
        extra_joints_idxs=extra.numpy(), src_inds=np.array(cell["src_inds"], np.int64), dst_inds=np.array(cell["dst_inds"], np.int64),
        kp_mask=fit64.kp_mask.numpy(), Ks=Ks.numpy(), w2c=w2c.numpy(), img_wh=np.array(img_wh, np.int64), target_kps=target.numpy(),
        target_scales=scales.numpy(), weights=np.array([fit64.kp_weight, fit64.preserve_weight, fit64.smooth_weight]),
        sigma=np.array(float(fit64.sigma)), **{"p_" + k: v.numpy() for k, v in params.items()},
        **{"i_" + k: v.numpy() for k, v in init.items()}, **out)
    print("wrote smplify_body.npz", os.path.getsize(os.path.join(OUT, "smplify_body.npz")), "bytes; rows", rows.tolist(),
          "losses f64", out["loss_f64_ih0"], out["loss_f64_ih1"])
    print("f32 against f64, worst element over the largest magnitude:", {k: f"{v:.2e}" for k, v in worst.items()})


if __name__ == "__main__":
    main(sys.argv[1])
