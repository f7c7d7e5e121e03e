"""The per-frame training path at surfel counts that are no multiple of anything: after the first densification P is an arbitrary
integer.  The per-frame slabs [n, P, 3] of the step plan then start off 16 bytes, the flat gradient buffer's slices (at 3P, 7P,
10P, 13P floats) too, the 64-surfel workgroups of the batched warp, the fused head and the fused tail and the 256-thread geometry
backward end in a partial group, and Adam runs its scalar path over most leaves.  The kernels have ragged-count tests of their own
(test_lbs_gpu.py, test_optim_gpu.py); here the plan that strings them together, with the bars of the tests it is tested by at P =
5000 (test_plugin_gpu.py) and P = 3000 (test_training_gpu.py).  The scene is the 160 x 128 one of test_training_gpu.py."""
import numpy as np
import pytest
import torch

from test_training_gpu import _AV, _avatar_composed_steps, _avatar_plan_steps, _avatar_scene

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _assert_ragged(P, flat, plan):
    """The premise of these tests, asserted: the slabs and slices really are off 16 bytes."""
    if P % 4:
        assert plan.xyz_p_all.shape[1:] == (P, 3) and plan.xyz_p_all[1].data_ptr() % 16 != 0
        assert all(flat.views[n].data_ptr() % 16 != 0 for n in ("rot", "scales"))
    assert P % 64 != 0 and P % 256 != 0


# 65 and 257: one surfel past a 64-surfel workgroup and a 256-thread block; 2997, 2998, 2999: P = 1, 2, 3 mod 4.  The sequence has
# four frames: ids past it wrap, [3, 3, 0] renders one frame twice
_FOUR = ([0, 1, 2, 3], [5, 2, 7, 0])
_CASES = ([(P, "synthetic", _FOUR, False) for P in (65, 257, 2997, 2998, 2999)] + [(P, "avatar", _FOUR, False) for P in (257, 2999)]
          + [(2998, "synthetic", ([2, 1, 7], [3, 3, 0]), False), (2999, "synthetic", _FOUR, True)])
_IDS = [f"P{P}-{loss}-n{len(fr[0])}-{'graphs' if gr else 'eager'}" for P, loss, fr, gr in _CASES]


@pytest.mark.parametrize("P,loss,frame_lists,use_graphs", _CASES, ids=_IDS)
def test_step_plan_matches_autograd_at_ragged_counts(P, loss, frame_lists, use_graphs):
    """test_plugin_gpu.py::test_step_plan_matches_autograd at ragged P: losses, the flat buffer and every image of every slot against
    the autograd path (render_frames + fused loss + backward; the avatar-stage loss against scenes.avatar_frame_loss)."""
    from scenes import avatar_frame_loss
    from soar_amd import rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan
    from soar_amd.synthetic import pool_targets
    seq, leaves, cam, bg, pool = _avatar_scene(P)
    if loss != "avatar":
        leaves = seq.leaves()
    flat = FlatGradBuffer(leaves)
    n = len(frame_lists[0])
    with torch.no_grad():
        seq.render_frames(_AV["frames"], bg, with_occ=True)
    assert rasterizer.last_num_rendered > 0
    cap = 3 * rasterizer.last_num_rendered
    try:
        plan = FrameStepPlan(seq, n, pool, bg, cap, flat, use_graphs=use_graphs, loss=loss)
    except Exception as e:                      # pragma: no cover - capture unsupported on this stack
        if use_graphs:
            pytest.skip(f"HIP graph capture unavailable: {e}")
        raise
    _assert_ragged(P, flat, plan)
    if not use_graphs:
        assert plan.fused_head and plan.fused_tail and plan.batched
    for frames in frame_lists:
        flat.zero()
        seq.refresh_blend_weights()
        if loss == "avatar":
            per_frame = [avatar_frame_loss(seq, f, bg, pool, plan.lam) for f in frames]
            sum(per_frame).backward()
            want, want_losses = flat.flat.clone(), torch.stack([l.detach() for l in per_frame])
            with torch.no_grad():
                outs = seq.render_frames(frames, bg)
        else:
            outs = seq.render_frames(frames, bg, loss_targets=[pool_targets(pool, f % seq.num_frames) for f in frames])
            sum(o.loss for o in outs).backward()
            want, want_losses = flat.flat.clone(), torch.stack([o.loss.detach() for o in outs])
        assert rasterizer.last_num_rendered > 0
        want_views = {name: flat.views[name].clone() for name in flat.leaves}
        losses = plan.run(frames)
        torch.cuda.synchronize()
        assert all(o == 0 for _, o in plan.check())
        for name in flat.leaves:                                              # every leaf's slice carries a gradient
            assert float(want_views[name].abs().sum()) > 0 and float(flat.views[name].abs().sum()) > 0, name
        np.testing.assert_allclose(losses.cpu().numpy(), want_losses.cpu().numpy(), rtol=1e-6)
        assert _rel(flat.flat.cpu().numpy(), want.cpu().numpy()) < 1e-4
        for i, o in enumerate(outs):
            v = plan.views[i]
            for name, img in (("color", o.render), ("normal", o.normal), ("depth", o.depth), ("opac", o.mask)):
                assert torch.equal(v[name].reshape(img.shape), img), (frames, i, name)


@pytest.mark.parametrize("n", [3, 4])
def test_step_plan_batched_launches_equal_the_per_frame_chains_at_ragged_count(n):
    """test_plugin_gpu.py::test_step_plan_batched_launches_equal_the_per_frame_chains at P = 2999: same images bit for bit, same losses,
    gradients to float-atomic order, over several steps with moving frames."""
    from soar_amd import rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan
    P = 2999
    seq, _, cam, bg, pool = _avatar_scene(P)
    flats = [FlatGradBuffer(seq.leaves()) for _ in range(2)]
    with torch.no_grad():
        seq.render_frames(_AV["frames"], bg, with_occ=True)
    cap = 2 * rasterizer.last_num_rendered
    assert cap > 0
    plans = [FrameStepPlan(seq, n, pool, bg, cap, flats[k], use_graphs=False, batched=(k == 0)) for k in range(2)]
    assert plans[0].batched and not plans[1].batched
    _assert_ragged(P, flats[0], plans[0])
    steps = ([0, 1, 2, 3], [9, 2, 30, 17], [3, 2, 1, 0], [3, 2, 1, 0]) if n == 4 else ([0, 1, 2], [5, 2, 15], [3, 3, 0], [3, 3, 0])
    for frames in steps:
        losses = []
        for plan in plans:
            losses.append(plan.run(frames).clone())
            torch.cuda.synchronize()
            assert all(o == 0 for _, o in plan.check())
        assert torch.equal(losses[0], losses[1])
        for va, vb in zip(plans[0].views, plans[1].views):
            for name in ("color", "normal", "depth", "opac", "occ", "radii"):
                assert torch.equal(va[name], vb[name]), (frames, name)
            assert int((va["radii"] > 0).sum()) > 0
        a, b = flats[0].flat, flats[1].flat
        assert b.abs().max() > 0 and (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()


@pytest.mark.parametrize("P", [2997, 2999])
def test_plan_and_fused_adam_equal_the_composed_training_steps_at_ragged_counts(P):
    """Five steps of FrameStepPlan(loss="avatar") + optim.FusedAdam against the same steps composed from the autograd pieces and
    torch.optim.Adam, with the bars of test_training_gpu.py's 20-step test: the plan writes the gradients through the flat
    buffer's misaligned views, Adam reads them on its scalar path."""
    losses_a, grads_a, snaps_a = _avatar_plan_steps(5, P)
    losses_b, grads_b, snaps_b = _avatar_composed_steps(5, P)
    for n in _AV["lr"]:
        assert grads_a[n].shape[0] == P and float(grads_b[n].abs().max()) > 0
        assert float((grads_a[n] - grads_b[n]).abs().max()) <= 1e-5 * float(grads_b[n].abs().max()), n
    for step, (la, lb) in enumerate(zip(losses_a, losses_b)):
        torch.testing.assert_close(la, lb, rtol=1e-5, atol=1e-6, msg=lambda m: f"step {step}: {m}")
    for n in _AV["lr"]:
        a, b = snaps_a[-1][n], snaps_b[-1][n]
        finite = b.abs() < 1e9                                             # (scales carry the surfel marker z = -1e10)
        assert float((a[finite] - b[finite]).abs().max()) <= 1e-5 * max(float(b[finite].abs().max()), 1.0), n
        assert float((snaps_a[-1][n] - snaps_a[0][n])[finite].abs().max()) > _AV["lr"][n], n          # ... and every leaf moved on


def test_plan_optimizer_hook_is_the_explicit_optimizer_step_at_ragged_count():
    """test_training_gpu.py::test_plan_optimizer_hook_is_the_explicit_optimizer_step at P = 2999: the update inside the next run, in
    one launch (with the step's input gather riding along) and in two parts, gives the losses of `plan.run(); adam.step()`."""
    from soar_amd import optim, rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan
    P = 2999

    def run(hooked):
        seq, leaves, cam, bg, pool = _avatar_scene(P)
        leaves = seq.leaves()
        flat = FlatGradBuffer(leaves)
        with torch.no_grad():
            seq.render_frames(_AV["frames"], bg, with_occ=True)
        plan = FrameStepPlan(seq, 4, pool, bg, 3 * rasterizer.last_num_rendered, flat, use_graphs=False)
        _assert_ragged(P, flat, plan)
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
