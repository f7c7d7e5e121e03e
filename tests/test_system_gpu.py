"""GPU tests of the training system (soar_amd/system.py) on a small synthetic scene: about 2 000 surfels on the synthetic
body with a small hash field (``use_explicit: false``), 5 video frames at 48x64 (the fewest the data module splits), normal views at 32x32, 4 SDS views at 32x32, an
``LPIPSVGG`` and a ``LatentEncoder`` with random weights, a guidance with a fixed linear ``eps_fn``, ``t`` and noises.

1. One step of each stage against the same step composed by hand (``compose_reference_step``: the parent's public functions and plain
   torch ops in the reference's order, TS/system/gaussian_surfel_mvdream.py:87-474).  The logged values agree within 2 float32 ulps.
   The leaves' gradients agree within a bound measured here: the composed step is run twice from the same state, ``s`` is the largest
   difference relative to the leaf's largest gradient (the rasterizer's backward sums with float atomics: the composed path's own
   run-to-run spread; two samples underestimate a range, hence the factor 4), and system against composed must stay within
   ``max(4 s, 1e-6)`` of the same scale (1e-6: the reordering of about ten float32 contributions per leaf, 10 x 2^-24).
2. Three steps of ``fit``, a checkpoint, ``AvatarPlayer.from_checkpoint``, ``load_checkpoint`` and a further step.
3. ``densify=True``."""
import gc

import pytest
import torch

from soar_amd import synthetic as syn
from system_scene import DEV, GUIDANCE, SMALL, build, compose_reference_step, make_world, seeded, system_step

pytestmark = pytest.mark.gpu
P, FRAMES, H, W, RES, VIEW = SMALL


@pytest.fixture(scope="module")
def world():
    return make_world(SMALL)


def ulps(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float32).cpu(), torch.as_tensor(b, dtype=torch.float32).cpu()
    if torch.equal(a, b):
        return 0.0
    spacing = torch.nextafter(b.abs(), torch.tensor(float("inf"))) - b.abs()
    return float((a - b).abs() / spacing)


def spread(g1, g2):
    """largest difference of two gradient sets, relative to each leaf's largest gradient"""
    worst = 0.0
    for k in g1:
        if g1[k] is None or g2[k] is None:
            assert g1[k] is None and g2[k] is None, k
            continue
        if g2[k].numel() == 0:
            continue
        scale = float(g2[k].abs().max())
        if scale > 0:
            worst = max(worst, float((g1[k] - g2[k]).abs().max()) / scale)
    return worst


@pytest.mark.parametrize("stage,it", [(0, 501), (1, 3)])
def test_one_step_equals_the_step_composed_by_hand(world, stage, it):
    w = world
    ref_sys = build(w, stage)
    log1, g1 = compose_reference_step(ref_sys, w.batch, it)
    log2, g2 = compose_reference_step(ref_sys, w.batch, it)
    s = spread(g1, g2)
    system = build(w, stage)
    logged, g = system_step(system, w.batch, it)
    assert set(logged) == set(log1), sorted(set(logged) ^ set(log1))
    for k in sorted(logged):
        e = ulps(logged[k], log1[k])
        print(f"\nstage {stage} {k}: {float(torch.as_tensor(logged[k])):.9g} against {float(torch.as_tensor(log1[k])):.9g} ({e:.2f} ulp)")
        assert e <= 2.0, k
    d = spread(g, g1)
    bound = max(4 * s, 1e-6)
    print(f"\nstage {stage}: the composed step's own spread s = {s:.3e}; system against composed {d:.3e} (bound {bound:.3e})")
    assert any(v is not None and v.numel() and float(v.abs().max()) > 0 for v in g.values())
    assert d <= bound
    # the guidance saw what the reference hands it (:182-210)
    call = system.guidance.calls[-1]
    ref = 512 if stage == 0 else RES                       # (stage 0 resizes its reference image to 512, stage 1 hands the crop on)
    assert call["normal_flag"] is (stage == 0) and call["ref_rgb"] == (3, ref, ref) and call["ref_mask"] == (1, ref, ref)
    assert call["comp_bg"] == (3, VIEW, VIEW) and call["grad_scale"] == (4, VIEW, VIEW) and call["has_batch"]
    assert system.global_step == it + 1


def test_stage_0_holds_the_sds_gradient_back_until_step_500(world):
    w = world
    ref_sys = build(w, 0)
    _, r1 = compose_reference_step(ref_sys, w.batch, 500)
    _, r2 = compose_reference_step(ref_sys, w.batch, 500)
    s = spread(r1, r2)
    logged_a, with_g = system_step(build(w, 0), w.batch, 500)
    logged_b, without_g = system_step(build(w, 0, with_guidance=False), w.batch, 500)
    assert "train/loss_sds" in logged_a and "train/loss_sds" not in logged_b
    d = spread(with_g, without_g)
    print(f"\nstep 500: with against without guidance {d:.3e} (spread {s:.3e})")
    assert d <= max(4 * s, 1e-6)
    _, with_g = system_step(build(w, 0), w.batch, 501)
    _, without_g = system_step(build(w, 0, with_guidance=False), w.batch, 501)
    d = spread(with_g, without_g)
    print(f"step 501: with against without guidance {d:.3e}")
    assert d > max(4 * s, 1e-6)


@pytest.mark.parametrize("train_background", [False, True])
def test_the_background_only_moves_when_asked_to(world, train_background):
    # (without the random augmentation: a step whose background is a drawn colour leaves the network a zero gradient)
    system = build(world, 1, random_aug=False, train_background=train_background)
    before = [p.detach().clone() for p in system.background.parameters()]
    system_step(system, world.batch, 3)
    moved = any(not torch.equal(a, p.detach()) for a, p in zip(before, system.background.parameters()))
    if not train_background:                               # the gradient is there (and stays: nobody zeroes it), the step is not
        assert any(p.grad is not None and float(p.grad.abs().max()) > 0 for p in system.background.parameters())
    assert moved is train_background


def test_fit_checkpoint_player_and_reload(world, tmp_path):
    from soar_amd.playback import AvatarPlayer
    from soar_amd.renderer import cameras
    from soar_amd.system import C
    w = world
    system = build(w, 1)
    w.dataset.steps.clear()
    seeded()
    try:
        system.fit(w.dataset, 3)
    finally:
        gc.unfreeze()
    assert system.global_step == 3 and w.dataset.steps == [(0, 0), (0, 1), (0, 2)]
    assert system.guidance.ranges == [(0.02, C(GUIDANCE["max_step_percent"], 0, i)) for i in range(3)]
    lrs = {g["name"]: g["lr"] for g in system.geometry.optimizer.param_groups}
    assert lrs["xyz"] == system.geometry.xyz_scheduler_args(2)
    assert all(torch.isfinite(torch.as_tensor(v, dtype=torch.float32)).all() for v in system.logged.values())
    path = tmp_path / "last.ckpt"
    system.save_checkpoint(path)
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert ckpt["global_step"] == 3 and {"geometry._xyz", "geometry._rotation", "geometry._occ", "geometry._colors", "geometry._scaling",
                                         "geometry._opacity", "geometry.attribute_field.encoding.hash_table"} <= set(ckpt["state_dict"])
    assert any(k.startswith("background.") for k in ckpt["state_dict"])
    # the file opens in the player as written.  What is compared: validation_step's PLAYBACK branch renders the live leaves the way the
    # player renders a checkpoint (CheckpointSurfels + AvatarPlayer.render), so equal bytes say that the checkpoint round trip loses
    # nothing (leaves, field, activations); the system's own path through renderer.batch_forward is exercised below, not compared
    player = AvatarPlayer.from_checkpoint(path, w.guide)
    spec = syn.make_camera(W, H, distance=3.0, elevation=0.1, azimuth=0.4)
    cam = cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(DEV), image_width=W, image_height=H,
                         world_view_transform=spec.world_view_transform.to(DEV), full_proj_transform=spec.full_proj_transform.to(DEV),
                         prcppoint=spec.prcppoint.to(DEV))
    pose = player.frame_pose(player.turntable(n=4, frame=0), 1)
    played = player.render(pose, cam)
    val = system.validation_step({"camera": cam, "pose": pose})
    for k in ("rgb", "normal", "occ", "mask"):
        assert torch.equal(played[k][0], val[k]), k
    assert int(val["mask"].sum()) > 0 and val["rgb"].shape == (H, W, 4) and val["rgb"].dtype == torch.uint8
    # the reference's validation images of a batch
    val = system.validation_step(dict(w.batch))
    for k in ("rgb", "normal", "pred_normal", "occ"):
        assert val[k].shape == (VIEW, VIEW, 4) and val[k].dtype == torch.uint8, k
    # a fresh system takes the checkpoint and trains on
    other = build(w, 1)
    other.load_checkpoint(path)
    assert other.global_step == 3 and other.geometry.num_points == system.geometry.num_points
    assert torch.equal(other.geometry._xyz.detach(), system.geometry._xyz.detach())
    assert torch.equal(other.geometry.attribute_field.encoding.hash_table.detach(), system.geometry.attribute_field.encoding.hash_table.detach())
    seeded()
    other.training_step(dict(w.batch))
    assert other.global_step == 4 and not torch.equal(other.geometry._xyz.detach(), system.geometry._xyz.detach())


@pytest.mark.parametrize("densify", [False, True])
def test_densification_is_an_opt_in(world, densify):
    system = build(world, 1, geometry_cfg={"densify_from_iter": 0, "densification_interval": 1, "densify_grad_threshold": 1e-9}, densify=densify)
    geo = system.geometry
    calls = []
    inner = geo.update_states
    geo.update_states = lambda *a, **k: (calls.append(a[0]), inner(*a, **k))[1]
    n0 = geo.num_points
    system_step(system, world.batch, 1)
    n1 = geo.num_points
    logged, _ = system_step(system, world.batch, 2)
    print(f"\ndensify={densify}: {n0} -> {n1} surfels")
    if densify:
        assert calls == [1, 2] and n1 != n0 and logged["gauss_num"] == n1
    else:
        assert calls == [] and n1 == n0 and logged["gauss_num"] == n0


def test_the_timing_script_runs_at_the_small_sizes(tmp_path):
    """scripts/system_time.py end to end at the tests' sizes: both stages, both forms, two repeats each (no number is asserted)"""
    import importlib.util
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "system_time.py")
    spec = importlib.util.spec_from_file_location("system_time", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "system_time.json"
    res = mod.main(["--small", "--steps", "2", "--warmup", "1", "--out", str(out)])
    saved = json.load(open(out))
    assert saved["shapes"] == {"P": P, "sds_views": [4, VIEW, VIEW], "frame": [H, W], "normal_views": [2, RES, RES]}
    for stage in ("0", "1"):
        for form in ("system", "composed_by_hand"):
            assert res["stages"][stage][form]["steps"] == 2 and res["stages"][stage][form]["wall_ms_median"] > 0
