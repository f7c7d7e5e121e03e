"""GPU tests of the keypoint fitting (soar_amd/smplify.py, csrc/smplify.hip): the HIP objective and its gradient against the golden
run of the reference's own objective and against the float64 restatement of tests/smplify_ref.py, and one whole fit.

The bar: HIP against float64 at most 4 x (float32 against float64), floor 1e-6 of the tensor's largest
magnitude, for every loss and every gradient tensor.

The fit (N = 6, 2 + 3 L-BFGS steps of at most 10 iterations, measured on an MI355X; the float64 objective at each drive's final
parameters, initial objective 8185.97): HIP 191.204, float32 restatement 191.401, float64 restatement 191.377; 57 closure
evaluations each."""
import types

import numpy as np
import pytest
import torch

import smplify_ref as sr
from test_smplify_cpu import golden, golden_call

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOSSES = ("kp", "preserve", "smooth")


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def frames(d, sl):
    """The frames ``sl`` of a parameter dict (betas is one row for all frames)."""
    return {k: (v if k == "betas" else v[sl]) for k, v in d.items()}


@pytest.fixture(scope="module")
def w():
    from soar_amd import smplify
    g, m, p, i, tables = golden()
    rig = smplify.KeypointRig.from_body_model(m, *tables, device=DEV)
    assert (rig.VS, rig.P, rig.NB) == (sr.used_vertices(m).numel(), 123, 20)
    c = golden_call(g)
    return types.SimpleNamespace(g=g, m=m, p=p, i=i, tables=tables, rig=rig, c=c, smplify=smplify)


def hip_objective(w, sl=slice(None), **kw):
    c = w.c
    return w.smplify.smplify_objective(w.rig, to_dev(frames(w.p, sl)), to_dev(frames(w.i, sl)), c["Ks"][sl].to(DEV), c["w2c"].to(DEV), c["img_wh"],
                                       c["target_kps"][sl].to(DEV), c["scales"][sl].to(DEV), c["weights"], c["sigma"], **kw)


def restated(w, sl, dtype, device, ignore_hands):
    c = dict(w.c)
    c.update(Ks=c["Ks"][sl], target_kps=c["target_kps"][sl], scales=c["scales"][sl])
    return sr.objective(w.m, w.tables, frames(w.p, sl), frames(w.i, sl), **c, ignore_hands=ignore_hands, detour=True, dtype=dtype, device=device)


@pytest.mark.parametrize("ignore_hands", [False, True])
def test_objective_against_the_reference_golden(w, ignore_hands):
    ih = int(ignore_hands)
    res = hip_objective(w, ignore_hands=ignore_hands)
    assert res.losses.shape == (3,) and res.losses.dtype == torch.float32
    for n, k in enumerate(LOSSES):
        sr.bar_check(f"golden ih{ih} loss {k}", res.losses[n], w.g[f"loss_f32_ih{ih}"][n], w.g[f"loss_f64_ih{ih}"][n])
    for k in sr.GRAD_KEYS:
        assert res.grads[k].shape == w.p[k].shape
        sr.bar_check(f"golden ih{ih} grad {k}", res.grads[k], w.g[f"g_{k}_f32_ih{ih}"], w.g[f"g_{k}_f64_ih{ih}"])
    kps = w.smplify.project_keypoints(w.rig, to_dev(w.p), w.c["Ks"].to(DEV), w.c["w2c"].to(DEV))
    assert kps.shape == (5, 137, 2)
    sr.bar_check(f"golden ih{ih} keypoints", kps, w.g[f"kps_f32_ih{ih}"], w.g[f"kps_f64_ih{ih}"])
    # two runs agree bit for bit
    again = hip_objective(w, ignore_hands=ignore_hands)
    assert torch.equal(res.losses, again.losses) and all(torch.equal(res.grads[k], again.grads[k]) for k in sr.GRAD_KEYS)


@pytest.mark.parametrize("sl", [slice(0, 1), slice(0, 2), slice(1, 4)], ids=["N1", "N2", "N3"])
def test_short_sequences_against_the_float64_restatement(w, sl):
    """N = 1: no pair, the smooth term and its gradient are zero.  N = 2, 3: the end frames have one neighbour each; frames 1 .. 3
    hold the repeated pose and the frame under the clamp."""
    res = hip_objective(w, sl)
    l64, g64 = restated(w, sl, torch.float64, "cpu", False)
    l32, g32 = restated(w, sl, torch.float32, DEV, False)
    for n, k in enumerate(LOSSES):
        sr.bar_check(f"{sl} loss {k}", res.losses[n], l32[k], l64[k])
    for k in sr.GRAD_KEYS:
        sr.bar_check(f"{sl} grad {k}", res.grads[k], g32[k], g64[k])
    if sl.stop - sl.start == 1:
        assert float(res.losses[2]) == 0.0
        no_smooth = w.smplify.smplify_objective(w.rig, to_dev(frames(w.p, sl)), to_dev(frames(w.i, sl)), w.c["Ks"][sl].to(DEV), w.c["w2c"].to(DEV),
                                                w.c["img_wh"], w.c["target_kps"][sl].to(DEV), w.c["scales"][sl].to(DEV),
                                                (w.c["weights"][0], w.c["weights"][1], 0.0), w.c["sigma"])
        assert all(torch.equal(res.grads[k], no_smooth.grads[k]) for k in sr.GRAD_KEYS)


def test_a_frame_alone_equals_the_frame_in_the_batch(w):
    """The keypoint and preserve parts (smooth weight 0; the means divide by the batch's 5 frames in both runs)."""
    wk, wp, _ = w.c["weights"]
    call = lambda sl, **kw: w.smplify.smplify_objective(
        w.rig, to_dev(frames(w.p, sl)), to_dev(frames(w.i, sl)), w.c["Ks"][sl].to(DEV), w.c["w2c"].to(DEV), w.c["img_wh"],
        w.c["target_kps"][sl].to(DEV), w.c["scales"][sl].to(DEV), (wk, wp, 0.0), w.c["sigma"], **kw)
    batch = call(slice(None))
    for f in range(5):
        one = call(slice(f, f + 1), norm_frames=5)
        for k in sr.POSE_KEYS + ("transl",):
            assert torch.equal(one.grads[k][0], batch.grads[k][f]), (f, k)
        assert torch.equal(one.frame_betas[0], batch.frame_betas[f]), f
    # and a batch in another order gives every frame the same bits: no result depends on which workgroup ran the frame
    perm = [3, 0, 4, 2, 1]
    shuffled = call(perm)
    for k in sr.POSE_KEYS + ("transl",):
        assert torch.equal(shuffled.grads[k], batch.grads[k][perm]), k


def test_strided_inputs_are_accepted(w):
    res = hip_objective(w)
    p, i = to_dev(w.p), to_dev(w.i)
    wide = {}
    for k, v in p.items():
        buf = torch.zeros(v.shape[:-1] + (2 * v.shape[-1],), device=DEV)
        buf[..., ::2] = v
        wide[k] = buf[..., ::2]
        assert not wide[k].is_contiguous()
    tk = torch.zeros(5, 137, 6, device=DEV)
    tk[..., ::2] = w.c["target_kps"].to(DEV)
    Ks = w.c["Ks"].to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    got = w.smplify.smplify_objective(w.rig, wide, i, Ks, w.c["w2c"].to(DEV), w.c["img_wh"], tk[..., ::2], w.c["scales"].to(DEV), w.c["weights"],
                                      w.c["sigma"])
    assert torch.equal(got.losses, res.losses) and all(torch.equal(got.grads[k], res.grads[k]) for k in sr.GRAD_KEYS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.smplify.smplify_objective(w.rig, w.p, i, Ks, w.c["w2c"].to(DEV), w.c["img_wh"], tk[..., ::2], w.c["scales"].to(DEV))


def test_target_scales_and_the_frame_without_a_confident_keypoint(w):
    t = w.c["target_kps"].to(DEV)
    got = w.smplify.target_scales(t, w.c["img_wh"])
    assert torch.equal(got.cpu(), w.c["scales"])                       # min, max and one subtraction: the reference's bits
    bad = t.clone()
    bad[2, :, 2] = 0.3                                                  # "above 0.3": 0.3 itself does not count
    with pytest.raises(ValueError, match="frame 2 has no keypoint"):
        w.smplify.target_scales(bad, w.c["img_wh"])
    fit = w.smplify.SMPLify(w.rig, body_steps=1, hand_steps=1)
    with pytest.raises(ValueError, match="frame 2 has no keypoint"):
        fit.fit(fit_inputs(w)[0], w.c["Ks"], w.c["w2c"], w.c["img_wh"], bad)
    assert fit.evaluations == 0                                         # raised before the objective was launched


def test_a_bad_table_index_raises_before_any_launch(w):
    src, dst, mask = w.tables
    with pytest.raises(ValueError, match="src_inds"):
        w.smplify.KeypointRig.from_body_model(w.m, [w.rig.J + w.rig.NX + w.rig.L] + src[1:], dst, mask, device=DEV)
    with pytest.raises(ValueError, match="dst_inds"):
        w.smplify.KeypointRig.from_body_model(w.m, src, [137] + dst[1:], mask, device=DEV)


# ---- the fit ----------------------------------------------------------------------------------------------------------------------

def fit_inputs(w, N=6):
    """Known parameters (rotation vectors, as SMPLer-X gives them), a perturbed start, and the known parameters' keypoints."""
    gen = torch.Generator().manual_seed(77)
    rn = lambda *s: torch.randn(*s, generator=gen)
    t = torch.linspace(0.0, 1.0, N)[:, None]
    true = {"global_orient": torch.tensor([[0.25, 0.15, -0.1]]) + 0.1 * t * rn(1, 3), "body_pose": 0.25 * rn(1, 63) + 0.15 * t * rn(1, 63),
            "left_hand_pose": 0.2 * rn(1, 45) + 0.1 * t * rn(1, 45), "right_hand_pose": 0.2 * rn(1, 45) + 0.1 * t * rn(1, 45),
            "jaw_pose": 0.1 * rn(N, 3), "leye_pose": 0.05 * rn(N, 3), "reye_pose": 0.05 * rn(N, 3), "betas": (0.5 * rn(1, 10)).expand(N, -1),
            "expression": 0.5 * rn(N, 10), "transl": 0.05 * rn(N, 3)}
    start = {k: (v + (0.08 if k in sr.POSE_KEYS else 0.03) * rn(*v.shape) if k in sr.GRAD_KEYS else v.clone()) for k, v in true.items()}
    six = {k: (w.smplify.rotation_6d_from_rotvec(v.double().reshape(N, -1, 3)) if k in sr.POSE_KEYS else v.double()) for k, v in true.items()}
    six["betas"] = six["betas"][:1]
    Ks, w2c = w.c["Ks"][[0, 1, 2, 4, 0, 1]][:N].double(), w.c["w2c"].double()
    uv = sr.keypoints(w.m, w.tables, six, Ks, w2c)
    conf = 0.4 + 0.6 * torch.rand(N, 137, 1, generator=gen)
    target = torch.cat([uv / torch.tensor(w.c["img_wh"], dtype=torch.float64), conf.double()], -1).float()
    return start, target, Ks.float(), six


def test_fit_reaches_the_float64_objective(w):
    start, target, Ks, _ = fit_inputs(w)
    w2c, wh = w.c["w2c"], w.c["img_wh"]
    steps = dict(body_steps=2, hand_steps=3, max_iters=10)

    def restated_drive(dtype, device):
        def objective(rig, params, init, Ks_, w2c_, img_wh, tk, scales, weights, sigma, ignore_hands):
            ls, gr = sr.objective(w.m, w.tables, params, init, Ks_, w2c_, img_wh, tk, scales, dtype=dtype, device=device, weights=weights,
                                  sigma=sigma, ignore_hands=ignore_hands)
            return types.SimpleNamespace(losses=torch.stack([ls[k] for k in LOSSES]), grads=gr)
        return w.smplify.SMPLify(types.SimpleNamespace(device=torch.device(device)), objective=objective,
                                 scales=lambda t, img_wh: sr.target_scales(t, img_wh), dtype=dtype, **steps)

    drives = {"hip": w.smplify.SMPLify(w.rig, **steps), "f32": restated_drive(torch.float32, DEV), "f64": restated_drive(torch.float64, "cpu")}
    scales = sr.target_scales(target.double(), wh)

    def f64_objective(six, init):
        ls, _ = sr.objective(w.m, w.tables, {k: v.cpu() for k, v in six.items()}, {k: v.cpu() for k, v in init.items()}, Ks, w2c, wh, target,
                             scales)
        return float(sum(ls.values()))

    final = {}
    for name, fit in drives.items():
        out = fit.fit(start, Ks, w2c, wh, target)
        assert out["global_orient"].shape == (6, 3) and out["body_pose"].shape == (6, 63) and out["left_hand_pose"].shape == (6, 45)
        assert out["betas"].shape == (1, 10) and out["transl"].shape == (6, 3) and torch.equal(out["jaw_pose"].cpu().float(), start["jaw_pose"])
        if name == "hip":
            init6 = {k: (w.smplify.rotation_6d_from_rotvec(v.reshape(6, -1, 3)) if k in sr.POSE_KEYS else v) for k, v in start.items()}
            init6["betas"] = init6["betas"].mean(0, keepdim=True)
            initial = f64_objective(init6, init6)
        final[name] = f64_objective(fit.params_6d, init6)
    print(f"fit: initial {initial:.6g} final hip {final['hip']:.6g} f32 {final['f32']:.6g} f64 {final['f64']:.6g} "
          f"(closure evaluations: hip {drives['hip'].evaluations}, f32 {drives['f32'].evaluations}, f64 {drives['f64'].evaluations})")
    assert final["hip"] < initial
    assert final["hip"] - final["f64"] <= max(2.0 * abs(final["f32"] - final["f64"]), 0.01 * final["f64"])


def test_stage_one_leaves_the_hands_alone(w):
    """Parameters outside a stage's list get no update: after stage one alone the hands' gradients are exactly zero and their
    values are the initial ones, bit for bit."""
    start, target, Ks, _ = fit_inputs(w)
    fit = w.smplify.SMPLify(w.rig, body_steps=1, hand_steps=0, max_iters=3)
    out = fit.fit(start, Ks, w.c["w2c"], w.c["img_wh"], target)
    assert fit.evaluations >= 2
    p6 = fit.params_6d
    for k in ("left_hand_pose", "right_hand_pose"):
        assert torch.equal(p6[k], w.smplify.rotation_6d_from_rotvec(start[k].to(DEV).reshape(6, -1, 3)))
    assert not torch.equal(p6["body_pose"], w.smplify.rotation_6d_from_rotvec(start["body_pose"].to(DEV).reshape(6, -1, 3)))
    # the stage's closure writes the gradients of its own list and of no other
    params = {k: v.clone().requires_grad_(k in sr.GRAD_KEYS) for k, v in p6.items()}
    for k in sr.GRAD_KEYS:
        params[k].grad = torch.zeros_like(params[k])
    tk = target.to(DEV)
    closure = fit.make_closure(params, {k: v.clone() for k, v in p6.items()}, w.smplify.STAGE_KEYS[0], Ks.to(DEV), w.c["w2c"].to(DEV), w.c["img_wh"],
                               tk, w.smplify.target_scales(tk, w.c["img_wh"]), True)
    closure()
    assert float(params["left_hand_pose"].grad.abs().max()) == 0.0 and float(params["right_hand_pose"].grad.abs().max()) == 0.0
    assert float(params["body_pose"].grad.abs().max()) > 0.0 and float(params["betas"].grad.abs().max()) > 0.0
    assert float(fit.last.grads["left_hand_pose"].abs().max()) > 0.0          # the objective itself has a hand gradient (preserve, smooth)
    assert out["right_hand_pose"].shape == (6, 45)
