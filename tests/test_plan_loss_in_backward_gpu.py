"""The batched step plan with the frame loss inside the backward blend's launch (SOAR_PLAN_LOSS_IN_BACKWARD, soar_amd/step_plan.py;
soar_rast_backward_plan_loss, csrc/rast_render_bwd.hip) against the chain with the loss launch it replaces:

* the blend makes the loss's pixel gradients in its own prologue (the eight gradient planes are neither written nor read);
* the loss's value pass rides in the blend's launch and leaves a partial per wavefront of soar_frame_loss's grid, which the tail adds
  up in that kernel's order.

Switch on against switch off: a fresh plan and FusedAdam on the same snapshot of the leaves, two steps plus the third call that applies
the second update (the scheme of tests/test_plan_fused_small_launches_gpu.py).  Losses and images are the same bits wherever the
parameters they were computed from are.  With the order-insensitive backward (rasterizer.DETERMINISTIC_BACKWARD: float64 rows) there
is no order noise: losses, the five image planes, radii, the flat gradient buffer and the parameters are the same bits after both
steps.  With float32 atomics gradients and parameters differ between two runs of the SAME form by the order of the atomics; that
distance (L2, per leaf) is measured from this test's own two switch-off runs, and the new form may be 2 x as far from the first of
them, with floors from the number format where two samples measure 0: gradients float32 epsilon times the leaf's gradient norm,
parameters 2 lr of the leaf (Adam moves one element whose gradient is of the size of the order noise by +-lr either way).

Cases: `tiny` (5k Gaussians, 256 x 192) at 1, 4 and 5 frames per step (5: a second group of frames in the tail's kernel) with the
blend's form forced to single blocks and to pairs, the pool and explicit targets; ragged images of 2000-3000 Gaussians built from
soar_amd.synthetic: 252 x 190 (float4 path, partial tiles, bg_tiles in use), 254 x 189 (pixel count not a multiple of 4: scalar path,
no bg_tiles), and a step one frame of which shows nothing (the body moved behind the camera: the riders still leave that frame's
all-background loss, the blend has no tile with work).  One direct case without the plan: soar_frame_loss + soar_rast_backward_plan
against soar_rast_backward_plan_loss on one 192 x 200 frame with float64 rows -- accumulation rows and loss bit for bit.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -23
LRS = {"xyz": 1.6e-5, "rot": 1e-3, "scales": 5e-5, "colors": 2.5e-3}
SWITCH = "SOAR_PLAN_LOSS_IN_BACKWARD"
STEPS = {1: ([3], [17]), 3: ([0, 1, 2], [2, 5, 1]), 4: ([0, 1, 2, 3], [9, 2, 30, 17]), 5: ([0, 1, 2, 3, 4], [9, 2, 30, 17, 5])}
IMAGES = ("color", "normal", "depth", "opac", "occ", "radii")


def _scene(seq, pool):
    """-> (seq, pool, bg, binning capacity, snapshot of the leaves): one autograd step sizes the binning buffers"""
    import bench
    from soar_amd import rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
    before = rasterizer.stats["num_rendered"]
    bench.run_step(seq, pool, FlatGradBuffer(seq.leaves()), [0, 1, 2, 3], bg)
    # (twice the last frame's instance count, as the other plan tests take it -- or the four frames' total where the last frame is
    # the one that shows nothing)
    cap = max(2 * rasterizer.last_num_rendered, rasterizer.stats["num_rendered"] - before)
    leaves = seq.leaves()
    return seq, pool, bg, cap, {n: leaves[n].detach().clone() for n in leaves}


@pytest.fixture(scope="module")
def tiny():
    import bench
    seq, pool, _ = bench.build_sequence("tiny", DEV)
    return _scene(seq, pool)


@pytest.fixture(scope="module")
def parts():
    from soar_amd import synthetic as syn
    return syn.make_body_model(0), syn.make_pose_sequence(8, 0)


def _ragged(parts, P, W, H, hidden_frame=None):
    from soar_amd import synthetic as syn
    from soar_amd.frame_step import AvatarSequence
    body, poses = parts
    seq = AvatarSequence(syn.sort_surfels_spatially(syn.make_surfels(P, 0)), body, poses, syn.make_camera(W, H), DEV)
    if hidden_frame is not None:
        # every joint of that frame carries the body to the far side of the camera: x -> x + 2 (camera - body)
        shift = 2.0 * (seq.campos.reshape(3).to(DEV) - seq.xyz.detach().mean(0))
        seq.cano2live[hidden_frame, :, :3, 3] += shift
    return _scene(seq, syn.make_loss_target_pool(H, W, 3, 0, DEV))


@pytest.fixture(scope="module")
def ragged_vec4(parts):
    return _ragged(parts, 2500, 252, 190)


@pytest.fixture(scope="module")
def ragged_scalar(parts):
    return _ragged(parts, 2000, 254, 189)


@pytest.fixture(scope="module")
def ragged_hidden(parts):
    return _ragged(parts, 3000, 252, 190, hidden_frame=1)


def _two_steps(scene, n, on, monkeypatch, explicit=False):
    """a fresh plan + optimizer on the snapshot's leaves, the switch set to `on` -> what its two steps left"""
    from soar_amd import synthetic as syn
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.optim import FusedAdam
    from soar_amd.step_plan import FrameStepPlan
    seq, pool, bg, cap, snap = scene
    leaves = seq.leaves()
    with torch.no_grad():
        for name, t in snap.items():
            leaves[name].copy_(t)
    monkeypatch.setenv(SWITCH, "1" if on else "0")
    flat = FlatGradBuffer(leaves)
    plan = FrameStepPlan(seq, n, syn.pool_targets(pool, 1) if explicit else pool, bg, cap, flat, use_graphs=False)
    assert plan.batched and plan.fused_tail and plan.loss_in_tail and plan.loss_in_backward == on
    plan.optimizer = FusedAdam(flat, lr=LRS)
    out = []
    for frames in STEPS[n] + (STEPS[n][0],):            # (a third call applies the second step's gradients: the parameters after it)
        losses = plan.run(frames).clone()
        torch.cuda.synchronize()
        assert all(o == 0 for _, o in plan.check())
        out.append(dict(losses=losses, grads=flat.flat.clone(), images=[{k: v[k].clone() for k in IMAGES} for v in plan.views],
                        params={k: leaves[k].detach().clone() for k in LRS}))
    return out[:2] + [dict(params=out[2]["params"])]


def _hold(scene, n, exact, monkeypatch, explicit=False, hidden=None):
    from soar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "DETERMINISTIC_BACKWARD", exact)
    seq = scene[0]
    parent = _two_steps(scene, n, False, monkeypatch, explicit)
    again = parent if exact else _two_steps(scene, n, False, monkeypatch, explicit)
    got = _two_steps(scene, n, True, monkeypatch, explicit)
    dist = lambda a, b: float((a.double() - b.double()).norm())
    P = int(seq.xyz.shape[0])
    slices = {"xyz": (0, 3 * P), "rot": (3 * P, 7 * P), "scales": (7 * P, 10 * P), "colors": (10 * P, 13 * P)}
    same_params = lambda a, b: all(torch.equal(a["params"][k], b["params"][k]) for k in LRS)
    assert torch.equal(parent[0]["losses"], again[0]["losses"])              # the form itself repeats these bits
    for step in range(2):
        a, b = parent[step], got[step]
        # (a step's parameters: the leaves as its forward saw them = what the optimizer left at the start of that call)
        comparable = same_params(a, b)
        assert comparable or (step > 0 and not exact), step
        if not comparable:
            continue
        assert torch.isfinite(b["losses"]).all() and float(b["losses"].abs().min()) > 0
        assert torch.equal(a["losses"], b["losses"]), (step, a["losses"], b["losses"])
        for f, (va, vb) in enumerate(zip(a["images"], b["images"])):
            for name in va:
                assert torch.equal(va[name], vb[name]), (step, f, name)
        if hidden is not None and step == 0:
            assert int(b["images"][hidden]["radii"].max()) == 0              # nothing of that frame is in front of the camera
        if exact:
            assert torch.equal(a["grads"], b["grads"]), step
            continue
        for name, (lo, hi) in slices.items():
            d0, d = dist(a["grads"][lo:hi], again[step]["grads"][lo:hi]), dist(a["grads"][lo:hi], b["grads"][lo:hi])
            print(f"n={n} step {step} grad {name}: off-off {d0:.3e}, on-off {d:.3e}")
            floor = EPS32 * float(a["grads"][lo:hi].double().norm())
            assert float(b["grads"][lo:hi].abs().max()) > 0 and d <= max(2 * d0, floor), (step, name, d, d0, floor)
    for step in (1, 2):                              # after the update from the first / the second step's gradients
        for name in LRS:
            d0 = dist(parent[step]["params"][name], again[step]["params"][name])
            d = dist(parent[step]["params"][name], got[step]["params"][name])
            print(f"n={n} params after update {step} {name}: off-off {d0:.3e}, on-off {d:.3e}")
            assert d <= (0.0 if exact else max(2 * d0, 2 * LRS[name])), (step, name, d, d0)
    assert not torch.equal(got[2]["params"]["xyz"], scene[4]["xyz"])         # (the optimizer did move the model)


@pytest.mark.parametrize("exact", [False, True], ids=["float32_atomics", "float64_rows"])
@pytest.mark.parametrize("region", ["1", "2"], ids=["single_blocks", "pairs"])
@pytest.mark.parametrize("n", [1, 4, 5])
def test_tiny_pool(tiny, n, region, exact, monkeypatch):
    monkeypatch.setenv("SOAR_PLAN_BWD_REGION", region)
    _hold(tiny, n, exact, monkeypatch)


@pytest.mark.parametrize("exact", [False, True], ids=["float32_atomics", "float64_rows"])
def test_tiny_explicit_targets(tiny, exact, monkeypatch):
    _hold(tiny, 4, exact, monkeypatch, explicit=True)


@pytest.mark.parametrize("exact", [False, True], ids=["float32_atomics", "float64_rows"])
def test_ragged_float4_path_with_partial_tiles(ragged_vec4, exact, monkeypatch):
    assert (252 * 190) % 4 == 0 and 252 % 4 == 0 and 252 % 16 and 190 % 16
    _hold(ragged_vec4, 3, exact, monkeypatch)


@pytest.mark.parametrize("exact", [False, True], ids=["float32_atomics", "float64_rows"])
def test_ragged_scalar_path(ragged_scalar, exact, monkeypatch):
    assert (254 * 189) % 4 != 0
    _hold(ragged_scalar, 3, exact, monkeypatch)


@pytest.mark.parametrize("exact", [False, True], ids=["float32_atomics", "float64_rows"])
def test_a_frame_that_shows_nothing(ragged_hidden, exact, monkeypatch):
    """frame 1 of the sequence is behind the camera; it is slot 1 of the first step and slot 2 of the second"""
    _hold(ragged_hidden, 3, exact, monkeypatch, hidden=1)


def test_direct_calls_leave_the_same_rows_and_loss(parts, monkeypatch):
    """soar_frame_loss + soar_rast_backward_plan against soar_rast_backward_plan_loss (+ the tail that finishes its value) on the same
    forward of one 192 x 200 frame, float64 rows: accumulation rows and loss bit for bit, in both forms of the blend"""
    from soar_amd import hip_lib, rasterizer, synthetic as syn
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.hip_lib import check, ptr
    from soar_amd.step_plan import FrameStepPlan
    monkeypatch.setattr(rasterizer, "DETERMINISTIC_BACKWARD", True)
    monkeypatch.setenv(SWITCH, "0")
    seq, pool, bg, cap, _ = _ragged(parts, 2500, 192, 200)
    flat = FlatGradBuffer(seq.leaves())
    plan = FrameStepPlan(seq, 1, pool, bg, cap, flat, use_graphs=False)
    plan.run([2])                                      # the forward of frame 2 stays in the plan's buffers
    torch.cuda.synchronize()
    L, s, v, W, H, P = plan.L, plan.seq, plan.views[0], plan.W, plan.H, plan.P
    prm, stream = plan.ctx.params, torch.cuda.current_stream(DEV).cuda_stream
    assert prm.debug & 2 and prm.debug & 8
    tg = syn.pool_targets(pool, 2)
    tc, tm, tn = (tg[k].contiguous() for k in ("color", "mask", "normal"))
    wc, wm, wn, wd = plan.weights
    f32 = dict(dtype=torch.float32, device=DEV)
    rows_of = lambda: v["work"][:4 * 16 * P].view(torch.float32).clone()
    head = (C.byref(prm),)
    model = (ptr(v["xyz_p"]), ptr(v["radii"]), None, ptr(s.colors.detach()), ptr(s.scales.detach()), ptr(v["rot_p"]), None, ptr(v["geom"]),
             ptr(v["binning"]), ptr(v["img"]), plan.capacity)
    outs = (ptr(v["g_means2D"]), ptr(plan.g_colors[0]), ptr(v["g_opacity"]), ptr(v["g_means3D"]), ptr(v["g_cov3D"]), None, ptr(plan.g_scales[0]),
            ptr(v["g_rot_p"]), ptr(v["g_view"]), ptr(v["g_proj"]), ptr(v["g_campos"]), ptr(v["work"]), v["work"].numel())
    for region in (1, 2):
        loss_a, loss_b = torch.zeros((), **f32), torch.zeros((), **f32)
        check(L.soar_frame_loss(W, H, ptr(v["color"]), ptr(v["normal"]), ptr(v["depth"]), ptr(v["opac"]), ptr(tc), ptr(tm), ptr(tn), wc, wm, wn, wd,
                                ptr(loss_a), ptr(v["sums"]), ptr(v["gC"]), ptr(v["gN"]), ptr(v["gD"]), ptr(v["gO"]), ptr(v["img"]), prm.bg_dev,
                                int(prm.cfg_normalize_depth), stream), "frame_loss")
        check(L.soar_rast_backward_plan(*head, region, *model, ptr(v["gC"]), ptr(v["gN"]), ptr(v["gD"]), ptr(v["gO"]), *outs, stream), "backward_plan")
        torch.cuda.synchronize()
        rows_a = rows_of()
        v["work"].zero_()
        rec = hip_lib.SoarBackwardLoss()
        rec.color, rec.normal, rec.depth, rec.opac = ptr(v["color"]), ptr(v["normal"]), ptr(v["depth"]), ptr(v["opac"])
        rec.target_color, rec.target_mask, rec.target_normal, rec.set_index_dev, rec.n_sets = ptr(tc), ptr(tm), ptr(tn), None, 1
        rec.w_color, rec.w_mask, rec.w_normal, rec.w_depth = wc, wm, wn, wd
        wave_sums = torch.zeros((hip_lib.BACKWARD_LOSS_SCRATCH_FLOATS,), **f32)
        rec.loss_out, rec.wave_sums = ptr(loss_b), ptr(wave_sums)
        fin = (hip_lib.SoarLossFinish * 1)()
        check(L.soar_rast_backward_plan_loss(*head, region, *model, C.addressof(rec), *outs, C.addressof(fin[0]), stream), "backward_plan_loss")
        torch.cuda.synchronize()
        rows_b = rows_of()
        fv = flat.views
        check(L.soar_frames_geometry_warp_backward_wave_losses(1, plan._tail_frames, ptr(s.xyz.detach()), ptr(s.rot.detach()), ptr(plan.blend_weights),
                                                               ptr(plan.mats), P, int(plan.blend_weights.shape[1]), ptr(s.scales.detach()),
                                                               ptr(fv["xyz"]), ptr(fv["rot"]), ptr(fv["scales"]), ptr(fv["colors"]), None, fin, stream),
              "tail")
        torch.cuda.synchronize()
        assert float(rows_a.abs().max()) > 0 and torch.equal(rows_a, rows_b), region
        assert torch.isfinite(loss_a) and float(loss_a) != 0 and torch.equal(loss_a, loss_b), (region, float(loss_a), float(loss_b))
