"""CPU tests of the keypoint fitting with per-frame contour landmarks and the hands' mean pose (soar_amd/smplify.py,
csrc/smplify.hip: ``soar_smplify_objective_body``): the restatement of tests/smplify_body_ref.py against the golden run of the
reference's own objective (tests/golden/smplify_body.npz), the row rule, the rig's checks, the exported symbol and the consumers'
``pose_mean=None`` path.  Nothing is launched."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import smplify_body_ref as sb
import smplify_ref as sr
from test_smplify_cpu import golden_call

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_CACHE = {}


def golden():
    """(npz, body, params, init, tables), loaded once and left unchanged."""
    if not _CACHE:
        g = np.load(os.path.join(HERE, "golden", "smplify_body.npz"))
        params, init, tables = sr.golden_inputs(g)
        _CACHE["g"] = (g, sb.golden_model(g), params, init, tables)
    return _CACHE["g"]


def test_golden_holds_the_cases_it_promises():
    g, m, p, i, tables = golden()
    assert p["transl"].shape == (8, 3) and m.v_template.shape == (400, 3) and m.lmk_faces_idx.numel() == 51
    assert m.dynamic_lmk_faces_idx.shape == (79, 17) and m.dynamic_lmk_bary_coords.shape == (79, 17, 3)
    assert torch.unique(m.faces_tensor[m.dynamic_lmk_faces_idx].reshape(-1)).numel() > 256            # the union exceeds the old rig
    assert sr.used_vertices(m).numel() + 51 <= 256                                                     # a frame's active set fits
    pm = m.pose_mean.reshape(55, 3)
    assert bool((pm[:25] == 0).all()) and bool((pm[25:] != 0).any(1).all())                           # the 30 hand joints only
    rows, yaw = g["rows"].tolist(), g["yaw_degrees"]
    assert rows[0] == 0 and 1 <= rows[1] <= 38 and rows[2] == 39 and yaw[2] > 39.5 and 40 <= rows[3] <= 77 and rows[4] == 78 and yaw[4] < -39.5
    assert rows[7] == 40
    assert float(np.abs((yaw - 0.5) - np.round(yaw - 0.5)).min()) >= 0.02                               # away from every rounding edge
    R = sb.full_rotations({k: v.double() for k, v in p.items()}, m.pose_mean)
    neck = sb.neck_rotation(m, R)
    assert float(neck[5, 0, 0]) < 0                                                                     # frame 5 faces away: the fold
    assert abs(int(sb.contour_row(R[:, 0])[6]) - rows[6]) >= 10                                         # frame 6: the spine turns the head
    src = tables[0]
    assert set(range(55 + 21 + 51, 55 + 21 + 51 + 17)) <= set(src) and len(src) == len(tables[1])
    for ih in (0, 1):
        for k in sr.GRAD_KEYS:
            assert np.isfinite(g[f"g_{k}_f64_ih{ih}"]).all() and np.abs(g[f"g_{k}_f64_ih{ih}"]).max() > 0
    assert os.path.getsize(os.path.join(HERE, "golden", "smplify_body.npz")) < 1_000_000


@pytest.mark.parametrize("ignore_hands", [False, True])
def test_float64_restatement_reproduces_the_reference(ignore_hands):
    g, m, p, i, tables = golden()
    tag = f"f64_ih{int(ignore_hands)}"
    ls, gr = sb.objective(m, tables, p, i, **golden_call(g), ignore_hands=ignore_hands, detour=True)
    for n, k in enumerate(("kp", "preserve", "smooth")):
        assert abs(float(ls[k]) - g[f"loss_{tag}"][n]) <= 1e-9 * abs(g[f"loss_{tag}"][n]), k
    for k in sr.GRAD_KEYS:
        assert gr[k].shape == g[f"g_{k}_{tag}"].shape
        assert sr.worst(gr[k].numpy(), g[f"g_{k}_{tag}"]) <= 1e-9, k
    kps, rows = sb.keypoints(m, tables, {k: v.double() for k, v in p.items()}, torch.from_numpy(g["Ks"]).double(),
                             torch.from_numpy(g["w2c"]).double(), detour=True, with_rows=True)
    assert rows.tolist() == g["rows"].tolist()                                                          # exactly, every frame
    assert sr.worst(kps.numpy(), g[f"kps_{tag}"]) <= 1e-9
    # the float32 restatement picks the same rows, and the joints without a mean may skip the detour (what the kernel does)
    _, rows32 = sb.keypoints(m, tables, p, torch.from_numpy(g["Ks"]), torch.from_numpy(g["w2c"]), with_rows=True)
    assert rows32.tolist() == g["rows"].tolist()
    _, gr0 = sb.objective(m, tables, p, i, **golden_call(g), ignore_hands=ignore_hands, detour=False)
    assert max(sr.worst(gr0[k].numpy(), g[f"g_{k}_{tag}"]) for k in sr.GRAD_KEYS) <= 1e-7
    # mean and table matter: without either the keypoint loss moves by far more than any tolerance here
    for other in (sb.golden_model(g, mean=False), sb.static_model(m)):
        lo, _ = sb.objective(other, tables, p, i, **golden_call(g), ignore_hands=ignore_hands)
        assert abs(float(lo["kp"]) - g[f"loss_{tag}"][0]) > 1e-3 * g[f"loss_{tag}"][0]


def test_row_rule_against_the_rows_the_reference_recorded():
    """Rotations about y, exact half-degree yaws among them (torch.round is half to even): only the golden's rows are the truth."""
    g = golden()[0]
    R = torch.from_numpy(g["rule_R"])
    assert R.dtype == torch.float64 and len(R) >= 20
    assert sb.contour_row(R).tolist() == g["rule_rows"].tolist()
    table = dict(zip(g["rule_angles"].tolist(), g["rule_rows"].tolist()))
    want = {0.0: 0, 10.2: 49, -10.2: 10, 38.6: 78, 40.3: 78, -39.6: 39, -80.0: 39, 120.0: 78, 179.0: 40}
    assert {a: table[a] for a in want} == want
    assert {0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 38.5, -38.5, 39.5, -39.5} <= set(table)                    # the 0.5-degree inputs


def rig_kwargs(m, src, dst, mask, **kw):
    base = dict(v_template=m.v_template, shapedirs=m.shapedirs, posedirs=m.posedirs, J_regressor=m.J_regressor, parents=m.parents,
                lbs_weights=m.lbs_weights, faces=m.faces_tensor, lmk_faces_idx=m.lmk_faces_idx, lmk_bary_coords=m.lmk_bary_coords,
                extra_joints_idxs=m.extra_joints_idxs, src_inds=src, dst_inds=dst, kp_mask=mask, device="cpu",
                dynamic_lmk_faces_idx=m.dynamic_lmk_faces_idx, dynamic_lmk_bary_coords=m.dynamic_lmk_bary_coords, neck_joint=12,
                pose_mean=m.pose_mean)
    base.update(kw)
    return base


def accepted(smplify, **kw):
    """Valid tables pass every host check and then ask for a HIP device: there is no CPU path."""
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        smplify.KeypointRig(**kw)


def test_rig_accepts_a_large_union_and_refuses_a_large_active_set():
    from soar_amd import smplify
    g, m, p, i, (src, dst, mask) = golden()
    accepted(smplify, **rig_kwargs(m, src, dst, mask))                                                  # the union exceeds 256
    # the static set is grown through the selector to exactly 205 and 206 vertices; only joints are mapped, so no index shifts
    used = sr.used_vertices(m)
    rest = torch.tensor([v for v in range(400) if v not in set(used.tolist())])
    for static, ok in ((205, True), (206, False)):
        extra = torch.cat([m.extra_joints_idxs, rest[:static - used.numel()]])
        kw = rig_kwargs(m, [0, 1, 2], [0, 1, 2], mask, extra_joints_idxs=extra)
        if ok:
            accepted(smplify, **kw)
        else:
            with pytest.raises(ValueError, match=r"206 static vertices \+ 3 x 17 contour corners = 257 slots; at most 256"):
                smplify.KeypointRig(**kw)
    # without a table the old limit is the old message
    with pytest.raises(ValueError, match="distinct vertices; at most 256"):
        smplify.KeypointRig(**rig_kwargs(m, [0], [0], mask, extra_joints_idxs=torch.arange(300), dynamic_lmk_faces_idx=None,
                                         dynamic_lmk_bary_coords=None))


def test_rig_checks_the_table_and_the_mean_on_the_host():
    from soar_amd import smplify
    g, m, p, i, (src, dst, mask) = golden()

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            smplify.KeypointRig(**rig_kwargs(m, src, dst, mask, **kw))
    df, db = m.dynamic_lmk_faces_idx, m.dynamic_lmk_bary_coords
    out_of_range = df.clone()
    out_of_range[40, 3] = 300                                                                           # 300 faces: 0 .. 299
    bad("dynamic_lmk_faces_idx: index 300", dynamic_lmk_faces_idx=out_of_range)
    negative = df.clone()
    negative[78, 16] = -1
    bad("dynamic_lmk_faces_idx: index -1", dynamic_lmk_faces_idx=negative)
    bad("bad shapes: dynamic_lmk_faces_idx", dynamic_lmk_faces_idx=df[:78], dynamic_lmk_bary_coords=db[:78])
    bad("bad shapes: dynamic_lmk_faces_idx", dynamic_lmk_bary_coords=db[:, :16])
    bad("bad shapes: dynamic_lmk_faces_idx", dynamic_lmk_faces_idx=torch.cat([df, df[:, :1]], 1), dynamic_lmk_bary_coords=torch.cat([db, db[:, :1]], 1))
    bad("must hold integers", dynamic_lmk_faces_idx=df.float())
    bad("come together", dynamic_lmk_bary_coords=None)
    bad("neck_joint", neck_joint=55)
    bad("pose_mean must hold 165", pose_mean=m.pose_mean[:-3])
    bad("pose_mean is not finite", pose_mean=torch.full((165,), float("nan")))
    bad("src_inds", src_inds=[55 + 21 + 51 + 17] + src[1:])                                             # one past the last contour landmark
    assert 55 + 21 + 51 in src[1:]
    bad("named twice", src_inds=[55 + 21 + 51] + src[1:])


def test_defaults_keep_the_static_rig():
    """``from_body_model`` without the new arguments: the frontal row as 17 static landmarks, and a non-zero mean refused."""
    from soar_amd import smplify
    g, m, p, i, (src, dst, mask) = golden()
    with pytest.raises(ValueError, match=r"non-zero pose_mean \(flat_hand_mean=False\): create it with flat_hand_mean=True"):
        smplify.KeypointRig.from_body_model(m, src, dst, mask, device="cpu")
    flat = sb.golden_model(g, mean=False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                          # 51 + 17 landmarks: src_inds are in range
        smplify.KeypointRig.from_body_model(flat, src, dst, mask, device="cpu")
    no_table = sb.golden_model(g, dynamic=False, mean=False)
    with pytest.raises(ValueError, match="src_inds"):                                                   # without the table there are only 51
        smplify.KeypointRig.from_body_model(no_table, src, dst, mask, device="cpu")
    with pytest.raises(ValueError, match="dynamic_contour=True needs"):
        smplify.KeypointRig.from_body_model(no_table, src, dst, mask, device="cpu", dynamic_contour=True)
    for kw in (dict(dynamic_contour=True), dict(use_pose_mean=True), dict(dynamic_contour=True, use_pose_mean=True)):
        body = m if kw.get("use_pose_mean") else flat
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            smplify.KeypointRig.from_body_model(body, src, dst, mask, device="cpu", **kw)
    # positional unpacking of three still works, and the new field trails with a default
    a, b, c = smplify.SmplifyResult(1, 2, 3)[:3]
    assert smplify.SmplifyResult._fields == ("losses", "grads", "frame_betas", "contour_rows") and smplify.SmplifyResult(1, 2, 3).contour_rows is None


def test_symbol_is_exported_and_refuses_bad_arguments():
    from soar_amd import build, hip_lib
    build.build()
    L = hip_lib.lib()
    header = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    name = "soar_smplify_objective_body"
    assert name in hip_lib.SIGNATURES and name in header and "SoarSmplifyBody" in header and hasattr(L, name)
    assert C.sizeof(hip_lib.SoarSmplifyBody) == 16 + 4 * 8 + 8 + 8
    # the old structs keep their layout
    assert C.sizeof(hip_lib.SoarSmplifyRig) == 24 + 12 * 8 and C.sizeof(hip_lib.SoarSmplifyArgs) == 16 + 24 * 8 + 14 * 4 + 10 * 8
    assert L.soar_smplify_objective_body(None, None, None, None) == 1 and "NULL" in hip_lib.last_error()
    rig, body, args = hip_lib.SoarSmplifyRig(), hip_lib.SoarSmplifyBody(), hip_lib.SoarSmplifyArgs()
    assert L.soar_smplify_objective_body(C.byref(rig), None, C.byref(args), None) == 1 and "NULL" in hip_lib.last_error()
    rig.J, rig.NBS, rig.NE, rig.VS, rig.P = 55, 10, 10, 206, 10
    body.L_dyn, body.n_rows, body.neck, body.VU = 17, 79, 12, 700
    for n in (0, -3):
        args.N = n
        assert L.soar_smplify_objective_body(C.byref(rig), C.byref(body), C.byref(args), None) == 1 and f"N={n}" in hip_lib.last_error()
    args.N = 4
    assert L.soar_smplify_objective_body(C.byref(rig), C.byref(body), C.byref(args), None) == 1
    assert "206 static slots + 3 x 17 contour slots" in hip_lib.last_error()
    rig.VS = 205
    assert L.soar_smplify_objective_body(C.byref(rig), C.byref(body), C.byref(args), None) == 1 and "NULL contour table" in hip_lib.last_error()
    body.n_rows = 78
    assert L.soar_smplify_objective_body(C.byref(rig), C.byref(body), C.byref(args), None) == 1 and "n_rows" in hip_lib.last_error()
    body.L_dyn, body.n_rows, body.mean_mask = 0, 0, 1 << 30
    assert L.soar_smplify_objective_body(C.byref(rig), C.byref(body), C.byref(args), None) == 1 and "pose_mean" in hip_lib.last_error()


def test_consumers_without_a_mean_are_todays_expressions():
    from soar_amd import playback, prior, smpl_guidance
    gen = torch.Generator().manual_seed(5)
    N = 3
    parms = {"global_orient": torch.randn(N, 3, generator=gen), "body_pose": torch.randn(N, 63, generator=gen),
             "jaw_pose": torch.randn(N, 3, generator=gen), "leye_pose": torch.randn(N, 3, generator=gen), "reye_pose": torch.randn(N, 3, generator=gen),
             "left_hand_pose": torch.randn(N, 45, generator=gen), "right_hand_pose": torch.randn(N, 45, generator=gen),
             "betas": torch.randn(1, 10, generator=gen), "expression": torch.randn(N, 10, generator=gen), "transl": torch.randn(N, 3, generator=gen)}
    order = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
    today = torch.cat([parms[k].reshape(N, -1) for k in order], dim=1)
    mean = torch.zeros(165)
    mean[75:] = torch.randn(90, generator=gen)
    assert torch.equal(prior.full_pose(parms), today) and torch.equal(prior.full_pose(parms, None), today)
    assert torch.equal(prior.full_pose(parms, mean), today + mean)
    assert torch.equal(prior.full_pose(parms, mean)[:, :75], today[:, :75])
    # SMPLGuidance._full_pose and the player's key-pose packer: the objects are made without their device-side state
    guide = object.__new__(smpl_guidance.SMPLGuidance)
    guide.device, guide.pose_mean = torch.device("cpu"), None
    one = {k: v[1:2] for k, v in parms.items()}
    assert torch.equal(guide._full_pose(one), today[1:2])
    guide.pose_mean = mean.reshape(1, 165)
    assert torch.equal(guide._full_pose(one), today[1:2] + mean)
    player = object.__new__(playback.AvatarPlayer)
    player.guidance, player.pose_mean = types.SimpleNamespace(device=torch.device("cpu")), None
    pose, transl, expr, betas = player._keys_of(parms)
    assert torch.equal(pose, today) and torch.equal(transl, parms["transl"]) and torch.equal(expr, parms["expression"])
    back = player._pose_dict(pose, transl, expr, betas)
    assert all(torch.equal(back[k], parms[k]) for k in order)
    player.pose_mean = mean.reshape(1, 165)
    assert torch.equal(player._keys_of(parms)[0], today + mean)
    assert torch.equal(player._pose_dict(today + mean, transl, expr, betas)["left_hand_pose"], (today + mean - mean)[:, 75:120])
    import inspect
    for fn in (prior.full_pose, prior.body_normal_priors, smpl_guidance.SMPLGuidance.__init__, playback.AvatarPlayer.__init__):
        assert inspect.signature(fn).parameters["pose_mean"].default is None
