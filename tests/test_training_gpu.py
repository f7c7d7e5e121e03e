"""System test: the pieces of the per-frame training step fit a synthetic avatar.

A teacher model renders four frames; a student with the same geometry but random colours is optimised with Adam through
KNN weights -> LBS warp -> rasterizer fwd/bwd -> fused frame loss (all HIP), then densified mid-way (the model grows) and
optimised further.  Gradients that were wrong in sign or scale, a
stale KNN cache, or a broken optimizer hand-over would all show up as a loss that does not fall.
"""
import pytest
import torch

from soar_amd import synthetic as syn
from soar_amd.frame_step import AvatarSequence

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _frame_targets(seq, frames, bg):
    with torch.no_grad():
        outs = seq.render_frames(frames, bg, with_occ=False)
    return [{"color": o.render.clone(), "mask": o.mask.clone(), "normal": o.normal.clone()} for o in outs]


def test_student_fits_teacher_and_survives_densification():
    from soar_amd.densify import SurfelDensifier
    P, W, H, frames = 4000, 160, 128, [0, 1, 2, 3]
    body, poses, cam = syn.make_body_model(0, V=2048), syn.make_pose_sequence(4, 0), syn.make_camera(W, H)
    bg = torch.tensor([0.1, 0.1, 0.1], device=DEV)
    teacher = syn.make_surfels(P, 0)
    targets = _frame_targets(AvatarSequence(teacher, body, poses, cam, DEV), frames, bg)

    g = torch.Generator().manual_seed(1)
    student = syn.make_surfels(P, 0)
    student.colors = torch.rand(P, 3, generator=g)
    seq = AvatarSequence(student, body, poses, cam, DEV)

    def run(seq, opt, steps):
        losses = []
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            seq.refresh_blend_weights()                       # canonical positions move: weights once per step
            outs = seq.render_frames(frames, bg, with_occ=False, loss_targets=targets, loss_weights=(1.0, 0.0, 0.0, 0.0))
            loss = sum(o.loss for o in outs) / len(outs)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses, outs

    opt = torch.optim.Adam([{"params": [seq.colors], "lr": 5e-2}, {"params": [seq.xyz], "lr": 1e-5}])
    l1, outs = run(seq, opt, 40)
    assert l1[-1] < 0.1 * l1[0], (l1[0], l1[-1])
    err0 = float((student.colors.to(DEV) - teacher.colors.to(DEV)).abs().mean())
    err1 = float((seq.colors.detach() - teacher.colors.to(DEV)).abs().mean())
    assert err1 < 0.8 * err0

    # densify from the statistics of the last step, rebuild the sequence on the grown model, keep training
    # the densifier works on the raw parameters of the reference (log scales, logit opacities); the synthetic sequence holds
    # activated scales with the surfel convention z = -1e10
    raw_scaling = torch.log(seq.scales.detach().clamp(min=1e-30))
    raw_scaling[:, 2] = -1e10
    names = dict(xyz=seq.xyz, rotation=seq.rot, scaling=raw_scaling, color=seq.colors, opacity=torch.full((P, 1), 5.0, device=DEV),
                 f_dc=torch.zeros(P, 1, 3, device=DEV), f_rest=torch.zeros(P, 3, 3, device=DEV))
    dens = SurfelDensifier(names, None, percent_dense=0.01, surface=True)
    for o in outs:
        dens.add_densification_stats(o.radii, o.viewspace_points.grad, torch.zeros(P, 3, device=DEV))
    r = dens.adaptive_densify(float(dens.accum[0].div(dens.accum[4].clamp(min=1)).median()), 1.3,
                              generator=torch.Generator(device=DEV).manual_seed(5))
    assert r["num_points"] > P and r["cloned"] + r["split"] > 100
    grown_scales = torch.exp(dens.params["scaling"].detach())
    grown_scales[:, 2] = -1e10
    grown = syn.Surfels(dens.params["xyz"].detach().cpu(), dens.params["rotation"].detach().cpu(),
                        grown_scales.cpu(), dens.params["color"].detach().cpu(),
                        torch.ones(r["num_points"], 1), torch.full((r["num_points"], 1), 0.01))
    seq2 = AvatarSequence(grown, body, poses, cam, DEV)
    opt2 = torch.optim.Adam([{"params": [seq2.colors], "lr": 2e-2}, {"params": [seq2.xyz], "lr": 1e-5}])
    l2, _ = run(seq2, opt2, 25)
    # split children are resampled around their parents, so the picture changes a little; training recovers it
    assert all(torch.isfinite(torch.tensor(l2))) and l2[-1] < l2[0] and l2[-1] < 0.2 * l1[0], (l1[0], l2[0], l2[-1])


@pytest.mark.parametrize("use_graphs", [False, True], ids=["eager", "graphs"])
def test_step_plan_trains_with_adam(use_graphs):
    """The explicit launch plan as a training loop: FrameStepPlan writes the summed gradients into the flat buffer whose views
    are the leaves' .grad, Adam updates the leaves in place (the graphs read the same storage), the loss falls."""
    from soar_amd import rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan
    P, W, H, frames = 4000, 160, 128, [0, 1, 2, 3]
    body, poses, cam = syn.make_body_model(0, V=2048), syn.make_pose_sequence(4, 0), syn.make_camera(W, H)
    bg = torch.tensor([0.1, 0.1, 0.1], device=DEV)
    teacher = syn.make_surfels(P, 0)
    t = _frame_targets(AvatarSequence(teacher, body, poses, cam, DEV), frames, bg)
    pool = torch.stack([torch.cat([d["color"], d["mask"], d["normal"]], 0) for d in t]).contiguous()      # [4,7,H,W]
    student = syn.make_surfels(P, 0)
    student.colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(1))
    seq = AvatarSequence(student, body, poses, cam, DEV)
    flat = FlatGradBuffer(seq.leaves())
    with torch.no_grad():
        seq.render_frames(frames, bg, with_occ=True)
    cap = 3 * rasterizer.last_num_rendered
    try:
        plan = FrameStepPlan(seq, 4, pool, bg, cap, flat, loss_weights=(1.0, 0.0, 0.0, 0.0), use_graphs=use_graphs)
    except Exception as e:                      # pragma: no cover - capture unsupported on this stack
        if use_graphs:
            pytest.skip(f"HIP graph capture unavailable: {e}")
        raise
    opt = torch.optim.Adam([{"params": [seq.colors], "lr": 5e-2}, {"params": [seq.xyz], "lr": 1e-5}])
    losses = []
    for _ in range(40):
        per_frame = plan.run(frames)            # zeroes the flat buffer, fills it with d(sum of frame losses)/d(leaves)
        opt.step()
        losses.append(float(per_frame.mean()))
    plan.check()
    assert losses[-1] < 0.1 * losses[0], (losses[0], losses[-1])
    assert seq.colors.grad is not None and seq.colors.grad.data_ptr() == flat.views["colors"].data_ptr()


_AV = dict(P=3000, W=160, H=128, frames=[0, 1, 2, 3],
           lr={"xyz": 1.6e-5, "rot": 1e-3, "scales": 5e-5, "colors": 2.5e-3, "occ": 1e-2},
           lam=dict(recon=1.0, mask=1.0, normal=1.0, occ=0.1))


def _avatar_scene(P=None):
    P, W, H = _AV["P"] if P is None else P, _AV["W"], _AV["H"]
    body, poses, cam = syn.make_body_model(0, V=2048), syn.make_pose_sequence(4, 0), syn.make_camera(W, H)
    seq = AvatarSequence(syn.make_surfels(P, 0), body, poses, cam, DEV)
    seq.occ.requires_grad_(True)
    bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
    pool = syn.make_loss_target_pool(H, W, 4, 1, DEV)
    return seq, dict(seq.leaves(), occ=seq.occ), cam, bg, pool


def _avatar_plan_steps(steps, P=None):
    """`steps` training steps of FrameStepPlan(loss="avatar") + optim.FusedAdam: per-step losses, first-step gradients, per-step leaves."""
    from soar_amd import optim, rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan
    seq, leaves, cam, bg, pool = _avatar_scene(P)
    flat = FlatGradBuffer(leaves)
    with torch.no_grad():
        seq.render_frames(_AV["frames"], bg, with_occ=True)
    plan = FrameStepPlan(seq, 4, pool, bg, 3 * rasterizer.last_num_rendered, flat, use_graphs=False, loss="avatar", lambdas=_AV["lam"])
    adam = optim.FusedAdam(flat, lr=_AV["lr"])
    losses_, grads, snaps = [], None, []
    for _ in range(steps):
        losses_.append(plan.run(_AV["frames"]).clone())
        if grads is None:
            grads = {n: flat.views[n].clone() for n in _AV["lr"]}
        adam.step()
        snaps.append({n: leaves[n].detach().clone() for n in _AV["lr"]})
    plan.check()
    return losses_, grads, snaps


def _avatar_composed_steps(steps, P=None):
    """The same steps composed from the autograd pieces of the plugin path: lbs_warp, GaussianRasterizer twice, the post-op functions
    (TS/renderer/diff_gaussian_rasterizer.py:292-303), losses.avatar_stage_loss + loss_occ, torch.optim.Adam."""
    from scenes import avatar_frame_loss
    seq, leaves, cam, bg, pool = _avatar_scene(P)
    lr = _AV["lr"]
    opt = torch.optim.Adam([{"params": [leaves[n]], "lr": lr[n]} for n in lr], lr=0.0, eps=1e-15)
    losses_, grads, snaps = [], None, []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        seq.refresh_blend_weights()
        per_frame = [avatar_frame_loss(seq, f, bg, pool, _AV["lam"]) for f in _AV["frames"]]
        sum(per_frame).backward()
        if grads is None:
            grads = {n: leaves[n].grad.clone() for n in lr}
        opt.step()
        losses_.append(torch.stack([l.detach() for l in per_frame]))
        snaps.append({n: leaves[n].detach().clone() for n in lr})
    return losses_, grads, snaps


def test_step_plan_avatar_loss_with_fused_adam_equals_the_composed_training_steps():
    """FrameStepPlan(loss="avatar") + optim.FusedAdam -- the reference's image losses on the video frame (0.8 masked L1 + 0.2 (1 -
    SSIM), mask L1, cosine normal loss through the renderer's post-ops, loss_occ through the occlusion image;
    TS/system/gaussian_surfel_mvdream.py:305-338, 412-417) and its optimizer step (:471-472) as explicit launches -- against the
    same 20 training steps composed from the autograd pieces of the plugin path: the same gradients (1e-5 of the largest) on the
    first step, the same losses along the 20 steps, the occlusion values trained."""
    losses_a, grads_a, snaps_a = _avatar_plan_steps(20)
    losses_b, grads_b, snaps_b = _avatar_composed_steps(20)
    for n in _AV["lr"]:
        assert float((grads_a[n] - grads_b[n]).abs().max()) <= 1e-5 * float(grads_b[n].abs().max()), n
    for step, (la, lb) in enumerate(zip(losses_a, losses_b)):
        torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-6, msg=lambda m: f"step {step}: {m}")
    for n in _AV["lr"]:
        a, b = snaps_a[-1][n], snaps_b[-1][n]
        finite = b.abs() < 1e9                                             # (scales carry the surfel marker z = -1e10)
        assert float((a[finite] - b[finite]).abs().max()) <= 1e-5 * max(float(b[finite].abs().max()), 1.0), n
        assert float((snaps_a[-1][n] - snaps_a[0][n])[finite].abs().max()) > 5 * _AV["lr"][n], n      # ... and every leaf trained
    assert float(losses_a[-1].sum()) < float(losses_a[0].sum())


def test_adam_keeps_torchs_overflow_behaviour():
    """A gradient beyond ~1.8e19 (the rotation gradient of a surfel does reach that: the marker scale z = -1e10 is a factor of it)
    squares to infinity in torch.optim.Adam -- the second moment is infinite from then on and the value never moves again.  The fused
    Adam squares first too; it used to scale first, moved those values by lr per step, and 20 steps later nothing agreed."""
    from soar_amd import optim
    from soar_amd.frame_dp import FlatGradBuffer
    p = torch.nn.Parameter(torch.tensor([[1.0, 2.0, 3.0, 4.0]], device=DEV))
    q = torch.nn.Parameter(p.detach().clone())
    g = torch.tensor([[5.0e19, -3.0e19, 1.0e19, 1e-3]], device=DEV)
    flat = FlatGradBuffer({"rot": p})
    adam, ref = optim.FusedAdam(flat, lr={"rot": 1e-2}), torch.optim.Adam([q], lr=1e-2, eps=1e-15)
    for _ in range(3):
        flat.views["rot"].copy_(g)
        q.grad = g.clone()
        adam.step(); ref.step()
    torch.cuda.synchronize()
    assert torch.equal(p.detach()[0, :2], torch.tensor([1.0, 2.0], device=DEV))
    torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-6, atol=0)


def test_plan_optimizer_hook_is_the_explicit_optimizer_step():
    """FrameStepPlan.optimizer: the update from the previous step's gradients inside the next run -- the positions behind the first
    gradient bucket and in front of the KNN refresh, the rest behind the second (soar_adam_step_rows) -- gives the losses of
    `plan.run(); adam.step()` step for step."""
    from soar_amd import optim, rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan

    def run(hooked):
        seq, leaves, cam, bg, pool = _avatar_scene()
        leaves = seq.leaves()
        flat = FlatGradBuffer(leaves)
        with torch.no_grad():
            seq.render_frames(_AV["frames"], bg, with_occ=True)
        plan = FrameStepPlan(seq, 4, pool, bg, 3 * rasterizer.last_num_rendered, flat, use_graphs=False)
        adam = optim.FusedAdam(flat, lr={k: v for k, v in _AV["lr"].items() if k in leaves})
        if hooked:
            plan.optimizer = adam
            plan.optimizer_in_two_parts = hooked == "two parts"
        out = []
        for _ in range(6):
            out.append(plan.run(_AV["frames"]).clone())
            if not hooked:
                adam.step()
        plan.check()
        return torch.stack(out)

    a, b, c = run(False), run("one launch"), run("two parts")
    assert float(a[0].sum()) != float(a[-1].sum())
    torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(a, c, rtol=1e-6, atol=1e-7)


def test_spatially_sorted_model_renders_the_same_images():
    """bench.py keeps its synthetic model in Morton order (synthetic.sort_surfels_spatially): a permutation of the surfels -- the
    images are those of the generator's order (only exactly equal depths could be blended in another order)."""
    body, poses, cam = syn.make_body_model(0, V=2048), syn.make_pose_sequence(4, 0), syn.make_camera(160, 128)
    bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
    surf = syn.make_surfels(4000, 0)
    outs = []
    for s in (surf, syn.sort_surfels_spatially(surf)):
        seq = AvatarSequence(s, body, poses, cam, DEV)
        with torch.no_grad():
            outs.append(seq.render_frame(1, bg, with_occ=True))
    for name in ("render", "normal", "depth", "mask", "occ"):
        a, b = getattr(outs[0], name), getattr(outs[1], name)
        assert float((a - b).abs().max()) <= 2e-6 * max(float(a.abs().max()), 1.0), name
