"""GPU tests of the keypoint fitting with per-frame contour landmarks and the hands' mean pose (soar_amd/smplify.py,
csrc/smplify.hip: ``soar_smplify_objective_body``) against the golden run of the reference's own objective on the body model it
creates (tests/golden/smplify_body.npz) and against the restatement of tests/smplify_body_ref.py.

The bar (``smplify_ref.bar_check``): HIP against float64 at most 4 x (float32 against float64), floor 1e-6
of the tensor's largest magnitude, for every loss, every gradient tensor and the keypoints.  One workgroup per frame: N <= 8 is
the whole shape (the row-rule test runs 14 frames).  The float32 and float64 restatements run on the CPU, once per model.

Measured on an MI355X: the golden's gradients, HIP worst element 9.7e-8 .. 7.8e-7 of the largest magnitude against 2.1e-7 .. 1.0e-5
for the reference's own float32 run; the fit (N = 6, 2 + 2 L-BFGS steps of at most 8 iterations; the float64 objective at each
drive's final parameters, initial 13136.1): HIP 9560.63, float32 restatement 9560.63, float64 restatement 9560.63; 44 closure
evaluations each."""
import types

import numpy as np
import pytest
import torch

import smplify_body_ref as sb
import smplify_ref as sr
from test_smplify_body_cpu import golden
from test_smplify_cpu import golden_call

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOSSES = ("kp", "preserve", "smooth")
HAND = ("left_hand_pose", "right_hand_pose")


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def frames(d, sl):
    return {k: (v if k == "betas" else v[sl]) for k, v in d.items()}


@pytest.fixture(scope="module")
def w():
    from soar_amd import smplify
    g, m, p, i, tables = golden()
    rig = smplify.KeypointRig.from_body_model(m, *tables, device=DEV, dynamic_contour=True, use_pose_mean=True)
    assert (rig.VS, rig.LD, rig.L, rig.P, rig.NB) == (sr.used_vertices(m).numel(), 17, 51, len(tables[0]), 20)
    assert rig.VU > 256 and rig.VS + 51 <= 256 and rig.mean_mask == ((1 << 55) - 1) ^ ((1 << 25) - 1) and rig.body_path
    return types.SimpleNamespace(g=g, m=m, p=p, i=i, tables=tables, rig=rig, c=golden_call(g), smplify=smplify, refs={})


def hip_objective(w, rig, p=None, sl=slice(None), **kw):
    c = w.c
    p = w.p if p is None else p
    weights = kw.pop("weights", c["weights"])
    return w.smplify.smplify_objective(rig, to_dev(frames(p, sl)), to_dev(frames(w.i, sl)), c["Ks"][sl].to(DEV), c["w2c"].to(DEV), c["img_wh"],
                                       c["target_kps"][sl].to(DEV), c["scales"][sl].to(DEV), weights, c["sigma"], **kw)


def restated(w, name, m, p=None, ignore_hands=False):
    """(float32, float64) restatements of model ``m`` on the CPU, computed once per ``name`` and shared."""
    key = (name, ignore_hands)
    if key not in w.refs:
        p = w.p if p is None else p
        w.refs[key] = tuple(sb.objective(m, w.tables, p, w.i, **w.c, ignore_hands=ignore_hands, dtype=dt) for dt in (torch.float32, torch.float64))
    return w.refs[key]


def check_against(tag, res, ref32, ref64):
    (l32, g32), (l64, g64) = ref32, ref64
    for n, k in enumerate(LOSSES):
        sr.bar_check(f"{tag} loss {k}", res.losses[n], l32[k], l64[k])
    for k in sr.GRAD_KEYS:
        sr.bar_check(f"{tag} grad {k}", res.grads[k], g32[k], g64[k])


@pytest.mark.parametrize("ignore_hands", [False, True])
def test_objective_against_the_reference_golden(w, ignore_hands):
    ih = int(ignore_hands)
    res = hip_objective(w, w.rig, ignore_hands=ignore_hands)
    assert res.contour_rows.dtype == torch.int32 and res.contour_rows.tolist() == w.g["rows"].tolist()       # every frame
    assert res.losses.shape == (3,) and res.losses.dtype == torch.float32
    for n, k in enumerate(LOSSES):
        sr.bar_check(f"golden ih{ih} loss {k}", res.losses[n], w.g[f"loss_f32_ih{ih}"][n], w.g[f"loss_f64_ih{ih}"][n])
    for k in sr.GRAD_KEYS:
        assert res.grads[k].shape == w.p[k].shape
        sr.bar_check(f"golden ih{ih} grad {k}", res.grads[k], w.g[f"g_{k}_f32_ih{ih}"], w.g[f"g_{k}_f64_ih{ih}"])
    kps = w.smplify.project_keypoints(w.rig, to_dev(w.p), w.c["Ks"].to(DEV), w.c["w2c"].to(DEV))
    assert kps.shape == (8, 137, 2)
    sr.bar_check(f"golden ih{ih} keypoints", kps, w.g[f"kps_f32_ih{ih}"], w.g[f"kps_f64_ih{ih}"])
    losses, grads, frame_betas = res[:3]                                # three-field unpacking as before
    again = hip_objective(w, w.rig, ignore_hands=ignore_hands)
    assert torch.equal(res.losses, again.losses) and all(torch.equal(res.grads[k], again.grads[k]) for k in sr.GRAD_KEYS)
    assert torch.equal(res.contour_rows, again.contour_rows)


def test_the_table_alone_and_the_mean_alone(w):
    sm = w.smplify
    flat = sb.golden_model(w.g, mean=False)
    rig = sm.KeypointRig.from_body_model(flat, *w.tables, device=DEV, dynamic_contour=True)
    assert rig.LD == 17 and rig.mean_mask == 0 and rig.body_path
    res = hip_objective(w, rig)
    assert res.contour_rows.tolist() == w.g["rows"].tolist()            # the mean touches the hands only: the same rows
    check_against("table alone", res, *restated(w, "flat", flat))
    static = sb.static_model(w.m)                                       # the frontal row as static landmarks, the mean kept
    rig = sm.KeypointRig.from_body_model(w.m, *w.tables, device=DEV, use_pose_mean=True)
    assert rig.LD == 0 and rig.L == 68 and rig.mean_mask != 0 and rig.body_path
    res = hip_objective(w, rig)
    assert res.contour_rows is None
    check_against("mean alone", res, *restated(w, "static mean", static))


def test_a_table_of_equal_rows_against_the_static_rig(w):
    sm = w.smplify
    flat = sb.golden_model(w.g, mean=False)
    same = sb.golden_model(w.g, mean=False)
    same.dynamic_lmk_faces_idx = flat.dynamic_lmk_faces_idx[:1].repeat(79, 1)
    same.dynamic_lmk_bary_coords = flat.dynamic_lmk_bary_coords[:1].repeat(79, 1, 1)
    dyn = sm.KeypointRig.from_body_model(same, *w.tables, device=DEV, dynamic_contour=True)
    today = sm.KeypointRig.from_body_model(flat, *w.tables, device=DEV)
    assert today.L == 68 and today.LD == 0 and not today.body_path and dyn.body_path
    ref = restated(w, "static flat", sb.static_model(flat))
    a, b = hip_objective(w, dyn), hip_objective(w, today)
    assert b.contour_rows is None and a.contour_rows.tolist() == w.g["rows"].tolist()
    check_against("equal rows, table", a, *ref)
    check_against("equal rows, static", b, *ref)


def test_an_all_zero_mean_changes_no_bit(w):
    sm = w.smplify
    flat = sb.golden_model(w.g, mean=False)
    assert not bool(flat.pose_mean.any())
    for dynamic in (True, False):
        with_mean = sm.KeypointRig.from_body_model(flat, *w.tables, device=DEV, dynamic_contour=dynamic, use_pose_mean=True)
        without = sm.KeypointRig.from_body_model(flat, *w.tables, device=DEV, dynamic_contour=dynamic)
        assert with_mean.mean_mask == 0 and with_mean.pose_mean is not None and without.pose_mean is None
        assert with_mean.body_path and without.body_path == dynamic         # the new entry point either way; it picks the kernel
        a, b = hip_objective(w, with_mean), hip_objective(w, without)
        assert torch.equal(a.losses, b.losses) and all(torch.equal(a.grads[k], b.grads[k]) for k in sr.GRAD_KEYS), dynamic
        assert torch.equal(a.frame_betas, b.frame_betas)


def test_a_frame_alone_equals_the_frame_in_the_batch(w):
    """The keypoint and preserve parts (smooth weight 0; the means divide by the batch's 8 frames in both runs)."""
    wk, wp, _ = w.c["weights"]
    call = lambda sl, **kw: hip_objective(w, w.rig, sl=sl, weights=(wk, wp, 0.0), **kw)
    batch = call(slice(None))
    for f in range(8):
        one = call(slice(f, f + 1), norm_frames=8)
        for k in sr.POSE_KEYS + ("transl",):
            assert torch.equal(one.grads[k][0], batch.grads[k][f]), (f, k)
        assert torch.equal(one.frame_betas[0], batch.frame_betas[f]) and int(one.contour_rows[0]) == int(batch.contour_rows[f]), f
    perm = [3, 0, 7, 4, 2, 6, 1, 5]
    shuffled = call(perm)
    for k in sr.POSE_KEYS + ("transl",):
        assert torch.equal(shuffled.grads[k], batch.grads[k][perm]), k
    assert torch.equal(shuffled.contour_rows, batch.contour_rows[perm])
    # N = 1: no pair, the smooth term is zero whatever its weight
    one = hip_objective(w, w.rig, sl=slice(2, 3))
    assert float(one.losses[2]) == 0.0
    no_smooth = hip_objective(w, w.rig, sl=slice(2, 3), weights=(wk, wp, 0.0))
    assert all(torch.equal(one.grads[k], no_smooth.grads[k]) for k in sr.GRAD_KEYS)


def test_hands_at_the_mean(w):
    """Every hand 6-D vector at the identity's rows (R = I: the log map's series, v = 0), one joint turned by 1e-4 rad and one by
    5e-3 rad, on either side of the kernel's series threshold (|a| = 1e-3) and of the restatement's (1e-6)."""
    p = {k: v.clone() for k, v in w.p.items()}
    eye6 = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    for k in HAND:
        p[k] = eye6.expand(8, 15, 6).clone()
    p["left_hand_pose"][:, 4] = w.smplify.rotation_6d_from_rotvec(torch.tensor([0.6e-4, -0.5e-4, 0.62e-4]).expand(8, 3))
    p["right_hand_pose"][:, 9] = w.smplify.rotation_6d_from_rotvec(torch.tensor([-3e-3, 3e-3, 2.6e-3]).expand(8, 3))
    res = hip_objective(w, w.rig, p)
    assert all(bool(torch.isfinite(res.grads[k]).all()) for k in sr.GRAD_KEYS) and bool(torch.isfinite(res.losses).all())
    assert float(res.grads["left_hand_pose"].abs().max()) > 0
    check_against("hands at the mean", res, *restated(w, "at the mean", w.m, p))
    kps = w.smplify.project_keypoints(w.rig, to_dev(p), w.c["Ks"].to(DEV), w.c["w2c"].to(DEV))
    k32, k64 = (sb.keypoints(w.m, w.tables, {k: v.to(dt) for k, v in p.items()}, w.c["Ks"].to(dt), w.c["w2c"].to(dt)) for dt in (torch.float32, torch.float64))
    sr.bar_check("hands at the mean keypoints", kps, k32, k64)


def test_the_row_rule_in_the_kernel(w):
    """Roots turned about y by the angles of the golden's row-rule list that are not rounding edges, everything above the root at
    rest: the kernel's float32 rule picks the rows the reference's function recorded."""
    ang, rows = w.g["rule_angles"], w.g["rule_rows"]
    yaw = -np.degrees(np.arctan2(np.sin(np.radians(ang)), np.abs(np.cos(np.radians(ang)))))
    keep = np.abs((yaw - 0.5) - np.round(yaw - 0.5)) >= 0.02
    assert keep.sum() >= 14 and {0.0, 10.2, -10.2, 38.6, 40.3, -39.6, -80.0, 120.0, 179.0} <= set(ang[keep].tolist())
    n = int(keep.sum())
    rep = lambda d: {k: (v if k == "betas" else v[:1].expand((n,) + v.shape[1:]).clone()) for k, v in d.items()}
    p, i = rep(w.p), rep(w.i)
    p["global_orient"] = sr.matrix_to_rotation_6d(torch.from_numpy(w.g["rule_R"][keep])).float()[:, None]
    p["body_pose"] = torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]).expand(n, 21, 6).clone()
    c = w.c
    res = w.smplify.smplify_objective(w.rig, to_dev(p), to_dev(i), c["Ks"][:1].expand(n, 3, 3).to(DEV), c["w2c"].to(DEV), c["img_wh"],
                                      c["target_kps"][:1].expand(n, 137, 3).to(DEV), c["scales"][:1].expand(n).to(DEV), c["weights"], c["sigma"])
    assert res.contour_rows.tolist() == rows[keep].tolist()


# ---- the fit, and one convention from the fit to its consumers ----------------------------------------------------------------------

def fit_inputs(w, N=6):
    """Known parameters (rotation vectors, as SMPLer-X gives them: the hands' are offsets from the mean), a perturbed start, and the
    known parameters' keypoints.  The head turns through the sequence, so the contour rows differ between the frames."""
    gen = torch.Generator().manual_seed(78)
    rn = lambda *s: torch.randn(*s, generator=gen)
    t = torch.linspace(0.0, 1.0, N)[:, None]
    true = {"global_orient": torch.tensor([[0.15, -0.5, -0.05]]) + t * torch.tensor([[0.0, 1.1, 0.0]]) + 0.05 * t * rn(1, 3),
            "body_pose": 0.2 * rn(1, 63) + 0.1 * t * rn(1, 63), "left_hand_pose": 0.15 * rn(1, 45) + 0.1 * t * rn(1, 45),
            "right_hand_pose": 0.15 * rn(1, 45) + 0.1 * t * rn(1, 45), "jaw_pose": 0.1 * rn(N, 3), "leye_pose": 0.05 * rn(N, 3),
            "reye_pose": 0.05 * rn(N, 3), "betas": (0.5 * rn(1, 10)).expand(N, -1), "expression": 0.5 * rn(N, 10), "transl": 0.05 * rn(N, 3)}
    start = {k: (v + (0.08 if k in sr.POSE_KEYS else 0.03) * rn(*v.shape) if k in sr.GRAD_KEYS else v.clone()) for k, v in true.items()}
    six = {k: (w.smplify.rotation_6d_from_rotvec(v.double().reshape(N, -1, 3)) if k in sr.POSE_KEYS else v.double()) for k, v in true.items()}
    six["betas"] = six["betas"][:1]
    Ks, w2c = w.c["Ks"][:N].double(), w.c["w2c"].double()
    uv, rows = sb.keypoints(w.m, w.tables, six, Ks, w2c, with_rows=True)
    assert len(set(rows.tolist())) >= 4
    conf = 0.4 + 0.6 * torch.rand(N, 137, 1, generator=gen)
    target = torch.cat([uv / torch.tensor(w.c["img_wh"], dtype=torch.float64), conf.double()], -1).float()
    return start, target, Ks.float(), six


def test_fit_reaches_the_float64_objective_and_returns_offsets(w):
    sm = w.smplify
    start, target, Ks, _ = fit_inputs(w)
    w2c, wh = w.c["w2c"], w.c["img_wh"]
    steps = dict(body_steps=2, hand_steps=2, max_iters=8)

    def restated_drive(dtype):
        def objective(rig, params, init, Ks_, w2c_, img_wh, tk, scales, weights, sigma, ignore_hands):
            ls, gr = sb.objective(w.m, w.tables, params, init, Ks_, w2c_, img_wh, tk, scales, dtype=dtype, weights=weights, sigma=sigma,
                                  ignore_hands=ignore_hands)
            return types.SimpleNamespace(losses=torch.stack([ls[k] for k in LOSSES]), grads=gr)
        return sm.SMPLify(types.SimpleNamespace(device=torch.device("cpu")), objective=objective,
                          scales=lambda t, img_wh: sr.target_scales(t, img_wh), dtype=dtype, **steps)

    drives = {"hip": sm.SMPLify(w.rig, **steps), "f32": restated_drive(torch.float32), "f64": restated_drive(torch.float64)}
    scales = sr.target_scales(target.double(), wh)

    def f64_objective(six, init):
        ls, _ = sb.objective(w.m, w.tables, {k: v.cpu() for k, v in six.items()}, {k: v.cpu() for k, v in init.items()}, Ks, w2c, wh, target, scales)
        return float(sum(ls.values()))

    final = {}
    for name, fit in drives.items():
        out = fit.fit(start, Ks, w2c, wh, target)
        assert out["global_orient"].shape == (6, 3) and out["body_pose"].shape == (6, 63) and out["left_hand_pose"].shape == (6, 45)
        if name == "hip":
            init6 = {k: (sm.rotation_6d_from_rotvec(v.reshape(6, -1, 3)) if k in sr.POSE_KEYS else v) for k, v in start.items()}
            init6["betas"] = init6["betas"].mean(0, keepdim=True)
            initial = f64_objective(init6, init6)
            assert fit.last.contour_rows is not None and len(set(fit.last.contour_rows.tolist())) >= 3
            # the returned hand rotation vectors are offsets from the mean: rodrigues(v + mean) is the rotation the body model saw.
            # float32: rotation entries are at most 1, two short chains of operations with 6e-8 each: 1e-5 leaves two digits to spare
            mean = w.m.pose_mean.reshape(55, 3)
            fitted = sb.full_rotations({k: v.cpu().double() for k, v in fit.params_6d.items()}, w.m.pose_mean, detour=True)
            for k, j0 in (("left_hand_pose", 25), ("right_hand_pose", 40)):
                v = out[k].cpu().double().reshape(6, 15, 3) + mean[j0:j0 + 15].double()
                again = sb.sj.batch_rodrigues(v.reshape(-1, 3)).reshape(6, 15, 3, 3)
                assert float((again - fitted[:, j0:j0 + 15]).abs().max()) <= 1e-5, k
        final[name] = f64_objective(fit.params_6d, init6)
    print(f"fit: initial {initial:.6g} final hip {final['hip']:.6g} f32 {final['f32']:.6g} f64 {final['f64']:.6g} "
          f"(closure evaluations: hip {drives['hip'].evaluations}, f32 {drives['f32'].evaluations}, f64 {drives['f64'].evaluations})")
    assert final["hip"] < initial
    assert final["hip"] - final["f64"] <= max(2.0 * abs(final["f32"] - final["f64"]), 0.01 * final["f64"])


def test_one_convention_from_the_fit_to_the_joint_chain(w):
    """The hand joints' keypoints of ``project_keypoints`` against the joints of the existing chain (``smplx_joints``) fed
    ``prior.full_pose(params, pose_mean)``, ``params`` being the rotation vectors ``fit`` would return for these 6-D values."""
    from soar_amd import prior
    from soar_amd.smplx_joints import JointTransformer
    sm = w.smplify
    kps = sm.project_keypoints(w.rig, to_dev(w.p), w.c["Ks"].to(DEV), w.c["w2c"].to(DEV))
    src, dst = torch.tensor(w.tables[0]), torch.tensor(w.tables[1])
    hand = (src >= 25) & (src < 55)
    assert int(hand.sum()) >= 20
    ref = {}
    for dt in (torch.float32, torch.float64):
        q = {k: v.to(dt) for k, v in w.p.items()}
        rv = {k: (sm.rotmat_to_rotvec(sm.rotation_6d_to_matrix(v)).reshape(8, -1) if k in sr.POSE_KEYS else v) for k, v in q.items()}
        pose = prior.full_pose(rv, w.m.pose_mean)
        assert pose.dtype == dt and torch.equal(pose[:, :75], prior.full_pose(rv)[:, :75])
        jt = JointTransformer(w.m.v_template.to(dt), w.m.shapedirs.to(dt), w.m.J_regressor.to(dt), w.m.parents)
        betas = torch.cat([q["betas"].expand(8, -1), q["expression"]], 1)
        A = jt(betas, pose, q["transl"])
        joints = (A[..., :3, :3] @ jt.joints(betas)[..., None])[..., 0] + A[..., :3, 3]
        ref[dt] = sr.project(joints[:, src[hand]], w.c["Ks"].to(dt), w.c["w2c"].to(dt))
    sr.bar_check("hand joints through the chain", kps[:, dst[hand]], ref[torch.float32], ref[torch.float64])
