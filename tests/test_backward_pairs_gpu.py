"""The backward blend with a wavefront per PAIR of 4 x 4 pixel blocks (csrc/rast_render_bwd.hip, REGION = 2), which the training step
plan asks for from 2^20 pixels up (soar_rast_backward_plan / soar_rast_backward_occ_plan), against the single-block form every other
caller keeps:

  * ragged images, where the right block of a pair is partly or wholly outside the image and the last row of blocks is partial:
    both forms against the CPU oracle and against each other, at the bars of tests/test_rasterizer_gpu.py;
  * which form a plan launches: read from the library's own counters (soar_rast_backward_region_counts);
  * the batched launch and the variant that takes the occlusion chain along: a step with pairs against the same step with single blocks;
  * the strict 1e-4 element-wise bar against the reference's kernels with the loss-derived upstream gradients the plan produces.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import scenes as S
from test_rasterizer_gpu import REL, check_backward, run_hip

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

GRAD_NAMES = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations",
              "dL_dviewmat", "dL_dprojmat", "dL_dcampos"]


def _counts():
    from soar_amd import hip_lib
    single, pairs = C.c_int64(0), C.c_int64(0)
    hip_lib.check(hip_lib.lib().soar_rast_backward_region_counts(C.byref(single), C.byref(pairs)), "region_counts")
    return single.value, pairs.value


def run_plan_backward(scene, grads, region):
    """forward through the C interface, backward through the plan-side entry (soar_rast_backward_plan) in the form `region`:
    the gradient tensors under the names run_hip uses, and the forward's radii / means2D"""
    from soar_amd import hip_lib
    from soar_amd.hip_lib import check, ptr
    from soar_amd.rasterizer import _C, _Ctx
    L = hip_lib.lib()
    st = S.torch_settings(scene, DEV)
    t = lambda a: torch.empty(0) if a is None else torch.as_tensor(a, dtype=torch.float32, device=DEV)
    means, opac = t(scene.means3D), t(scene.opacities)
    cols, scl, rot, cov, sh = t(scene.colors), t(scene.scales), t(scene.rotations), t(scene.cov3D), t(scene.shs)
    R, color, normal, depth, opac_img, radii, geom, binning, img = _C.rasterize_gaussians(
        st.bg, means, cols, opac, scl, rot, st.scale_modifier, cov, st.viewmatrix, st.projmatrix, st.prcppoint, st.patch_bbox,
        st.tanfovx, st.tanfovy, st.image_height, st.image_width, sh, st.sh_degree, st.campos, st.prefiltered, st.render_front,
        st.sort_descending, st.debug, st.config)
    P, H, W = int(means.shape[0]), scene.H, scene.W
    ctx = _Ctx(P, 0, H, W, st.tanfovx, st.tanfovy, st.scale_modifier, st.sh_degree, False, False, False, False, st.bg, st.viewmatrix,
               st.projmatrix, st.prcppoint, st.patch_bbox, st.campos, st.config, DEV)
    f = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    out = dict(dL_dmeans2D=f(P, 3), dL_dcolors=f(P, 3), dL_dopacity=f(P, 1), dL_dmeans3D=f(P, 3), dL_dcov3D=f(P, 6), dL_dsh=f(P, 0, 3),
               dL_dscales=f(P, 3), dL_drotations=f(P, 4), dL_dviewmat=f(4, 4), dL_dprojmat=f(4, 4), dL_dcampos=f(3))
    nbytes = C.c_size_t(0)
    check(L.soar_rast_backward_workspace_bytes(P, C.byref(nbytes)), "workspace_bytes")
    work = torch.empty(nbytes.value + 256, dtype=torch.uint8, device=DEV)
    work = work[(-work.data_ptr()) % 256:][:nbytes.value]
    g = [torch.as_tensor(x, dtype=torch.float32, device=DEV).contiguous() for x in grads]
    before = _counts()
    check(L.soar_rast_backward_plan(C.byref(ctx.params), region, ptr(means), ptr(radii), None, ptr(cols), ptr(scl), ptr(rot), None,
                                    ptr(geom), ptr(binning), ptr(img), int(R), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
                                    *[ptr(out[k]) if out[k].numel() else None for k in GRAD_NAMES], ptr(work), work.numel(),
                                    torch.cuda.current_stream(DEV).cuda_stream), "soar_rast_backward_plan")
    torch.cuda.synchronize()
    after = _counts()
    assert (after[0] - before[0], after[1] - before[1]) == ((1, 0) if region == 1 else (0, 1))
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(R=R, radii=radii.cpu().numpy())
    return res


def ragged_scene(W, H, where, seed=0):
    """About 200 Gaussians of tests/scenes.py's blob scene, moved so that their centres are spread over the whole W x H image
    (`where` = "any"), or all lie in the left (x mod 8 in 1..2) or the right (x mod 8 in 5..6) 4 x 4 block of a pair, with footprints
    of a pixel or so.  The image's width leaves the right block of the last pair partly or wholly outside, its height a partial last
    row of blocks."""
    P = 200
    sc = S.blob_scene(P=P, W=W, H=H, seed=40 + seed, config=(1, 1, 1, 0), random_quat_norm=False)
    rng = np.random.default_rng(seed + 5)
    cam = sc.cam
    fx, fy = W / (2 * cam.tanfovx), H / (2 * cam.tanfovy)
    if where == "any":
        u = rng.uniform(-0.5, W - 0.5, P)
        sigma_px = rng.uniform(0.5, 3.0, (P, 1))
    else:
        first = 1 if where == "left" else 5
        u = 8 * rng.integers(0, (W + 7) // 8, P) + first + rng.uniform(0.0, 2.0, P)
        u = np.where(u > W - 0.5, u - 8, u)                       # (a column outside the image: the pair to its left)
        sigma_px = rng.uniform(0.3, 0.6, (P, 1))
    v = rng.uniform(-0.5, H - 0.5, P)
    z = rng.uniform(2.0, 4.0, P)
    V = cam.world_view_transform.numpy().astype(np.float64)            # row vectors: p_view = [p, 1] @ V
    pv = np.stack([(u - W / 2 + 0.5) * z / fx, (v - H / 2 + 0.5) * z / fy, z], 1)
    sc.means3D = ((pv - V[3, :3]) @ np.linalg.inv(V[:3, :3])).astype(np.float32)
    sc.scales = (sigma_px * (z[:, None] / fx) * rng.uniform(0.5, 1.0, (P, 3))).astype(np.float32)
    sc.name = f"ragged_{where}_{W}x{H}"
    # where the centres land, computed like the rasterizer does (ndc2Pix)
    hom = np.concatenate([sc.means3D.astype(np.float64), np.ones((P, 1))], 1) @ cam.full_proj_transform.numpy().astype(np.float64)
    x = ((hom[:, 0] / hom[:, 3] + 1.0) * W - 1.0) * 0.5
    y = ((hom[:, 1] / hom[:, 3] + 1.0) * H - 1.0) * 0.5
    assert np.abs(x - u).max() < 1e-3 and np.abs(y - v).max() < 1e-3
    if where != "any":
        half = (np.floor(x).astype(int) % 8) // 4
        assert (half == (0 if where == "left" else 1)).all()
    return sc


RAGGED = [(W, H, "any") for W in (20, 28, 37) for H in (5, 19)] + [(37, 19, "left"), (37, 19, "right"), (28, 5, "left"), (20, 19, "right")]


@pytest.mark.parametrize("W,H,where", RAGGED, ids=[f"{w}x{h}-{k}" for w, h, k in RAGGED])
def test_pairs_and_single_blocks_on_ragged_images(W, H, where):
    """Widths 20, 28 and 37: the right block of the last pair of a row wholly (20, 28) or partly (37) outside the image; heights 5 and
    19: a partial last row of blocks.  Through the plan-side entry with region 1 and 2: every gradient tensor against the CPU oracle at
    check_backward's bars, and pairs against single blocks at the same bars.  "left" / "right": every Gaussian's centre in the left
    (right) block of its pair -- batches whose entries touch one half of the wavefront's 8 x 4 pixels."""
    scene = ragged_scene(W, H, where)
    grads = S.upstream_grads(scene)
    fw, bw = S.run_oracle(scene, grads)
    assert fw.num_rendered > 50 and float(np.abs(bw.dL_dmeans2D).sum()) > 0
    got = {region: run_plan_backward(scene, grads, region) for region in (1, 2)}
    for region in (1, 2):
        assert got[region]["R"] == fw.num_rendered
        np.testing.assert_array_equal(got[region]["radii"], fw.radii)
        check_backward(scene, got[region], bw)
    check_backward(scene, got[2], types.SimpleNamespace(**{k: got[1][k] for k in GRAD_NAMES}))
    # ... and single blocks through the plan-side entry are what the general entry point computes (same kernel, same grid)
    general = run_hip(scene, grads, export=False)
    check_backward(scene, got[1], types.SimpleNamespace(**{k: general[k] for k in GRAD_NAMES}))


def _small_sequence(P, W, H, seed=0):
    """bench.build_sequence's scene at a size of the test's choosing, with one target set"""
    from soar_amd import synthetic as syn
    from soar_amd.frame_step import AvatarSequence
    surfels = syn.sort_surfels_spatially(syn.make_surfels(P, seed))
    seq = AvatarSequence(surfels, syn.make_body_model(seed), syn.make_pose_sequence(4, seed), syn.make_camera(W, H), DEV)
    return seq, syn.make_loss_target_pool(H, W, 1, seed, DEV)


@pytest.mark.parametrize("W,H,env,want", [(256, 192, None, 1), (1024, 1024, None, 2), (256, 192, "2", 2), (1024, 1024, "1", 1)],
                         ids=["256x192-single", "1024x1024-pairs", "256x192-forced-pairs", "1024x1024-forced-single"])
def test_the_plan_chooses_the_form_by_image_size(W, H, env, want, monkeypatch):
    """A plan asks for pairs from 2^20 pixels up and for single blocks below; SOAR_PLAN_BWD_REGION=1|2, read where the plan is built,
    wins in both directions.  What was launched is read from the library's counters of blended frames per form."""
    import bench
    from soar_amd import rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan
    if env is None:
        monkeypatch.delenv("SOAR_PLAN_BWD_REGION", raising=False)
    else:
        monkeypatch.setenv("SOAR_PLAN_BWD_REGION", env)
    seq, pool = _small_sequence(2000, W, H)
    flat = FlatGradBuffer(seq.leaves())
    bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
    before = _counts()
    bench.run_step(seq, pool, flat, [0, 1], bg)
    torch.cuda.synchronize()
    mid = _counts()
    assert (mid[0] - before[0], mid[1] - before[1]) == (2, 0)          # the autograd path: single blocks whatever the size
    plan = FrameStepPlan(seq, 2, pool, bg, 3 * rasterizer.last_num_rendered, flat, use_graphs=False)
    monkeypatch.setenv("SOAR_PLAN_BWD_REGION", "1" if want == 2 else "2")     # (read once, where the plan was built)
    assert plan.bwd_region == want
    plan.run([0, 1])
    plan.run([2, 3])
    torch.cuda.synchronize()
    assert all(o == 0 for _, o in plan.check())
    after = _counts()
    assert (after[0] - mid[0], after[1] - mid[1]) == ((4, 0) if want == 1 else (0, 4))
    assert float(flat.flat.abs().sum()) > 0


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("loss,n", [(loss, n) for loss in ("synthetic", "avatar") for n in (1, 3, 4)],
                         ids=[f"{loss}-n{n}" for loss in ("synthetic", "avatar") for n in (1, 3, 4)])
def test_a_batched_step_with_pairs_equals_the_step_with_single_blocks(loss, n, monkeypatch):
    """The person scene at `tiny` size (5k surfels, 256 x 192), 1, 3 and 4 frames per step as ONE batched launch per stage, the default
    loss (render_backward_blocks_kernel) and the avatar-stage loss (the _occ kernel, which takes the occlusion chain along): the step's
    losses and images bit for bit (the forward is the same), its leaf gradients within the 1e-4 that the plan is held to against the
    autograd path (tests/test_plugin_gpu.py::test_step_plan_matches_autograd)."""
    import bench
    from soar_amd import rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.step_plan import FrameStepPlan
    seq, pool, _ = bench.build_sequence("tiny", DEV)
    leaves = seq.leaves()
    if loss == "avatar":
        seq.occ.requires_grad_(True)
        leaves = dict(leaves, occ=seq.occ)
    flats = [FlatGradBuffer(leaves) for _ in range(2)]
    bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
    bench.run_step(seq, pool, flats[0], [0, 1, 2, 3], bg)
    cap = 3 * rasterizer.last_num_rendered
    plans = []
    for region in (1, 2):
        monkeypatch.setenv("SOAR_PLAN_BWD_REGION", str(region))
        plans.append(FrameStepPlan(seq, n, pool, bg, cap, flats[region - 1], use_graphs=False, loss=loss))
        assert plans[-1].bwd_region == region and plans[-1].batched
    for frames in {1: ([13], [2]), 3: ([5, 2, 15], [3, 3, 0]), 4: ([5, 2, 7, 1], [3, 3, 0, 6])}[n]:
        losses = []
        for region, plan in zip((1, 2), plans):
            before = _counts()
            losses.append(plan.run(frames).clone())
            torch.cuda.synchronize()
            assert all(o == 0 for _, o in plan.check())
            after = _counts()
            assert (after[0] - before[0], after[1] - before[1]) == ((n, 0) if region == 1 else (0, n))
        assert torch.equal(losses[0], losses[1])
        for va, vb in zip(plans[0].views, plans[1].views):
            for name in ("color", "normal", "depth", "opac", "occ", "radii"):
                assert torch.equal(va[name], vb[name]), (frames, name)
        for name in flats[0].leaves:
            a, b = flats[1].views[name].cpu().numpy(), flats[0].views[name].cpu().numpy()
            assert float(np.abs(b).sum()) > 0, name
            assert _rel(a, b) < 1e-4, (name, frames)
        assert _rel(flats[1].flat.cpu().numpy(), flats[0].flat.cpu().numpy()) < 1e-4


def test_pairs_meet_the_strict_bar_with_loss_derived_gradients():
    """Where the plan uses pairs: the person scene at C2 size (50k surfels, 960 x 540) with the upstream gradients of the workload's own
    loss (synthetic.loss_and_pixel_grads at the reference's render), through the plan-side entry with region 2, against the
    reference's kernels: every gradient tensor within 1e-4 of its largest value, element by element and norm-wise -- the strict bar of
    tests/test_reference_build_gpu.py::test_surfel_scenes_meet_the_strict_gradient_bar."""
    from oracle import ref_rasterizer as rr
    from test_reference_build_gpu import _AsOracle
    if not rr.available():
        pytest.skip("oracle/_ref/libref_rasterizer.so not built (needs the reference's sources at build time)")
    ref_r = rr.RefRasterizer()
    scene = S.person_scene(P=50_000, W=960, H=540, seed=3, config=(1, 1, 1, 0), opacity=None)
    grads = S.loss_grads(scene, ref_r.run(scene, grads=None, state=False))
    ref = ref_r.run(scene, grads=grads)
    hip = run_plan_backward(scene, grads, 2)
    assert hip["R"] == ref["R"] and ref["R"] > 100_000
    np.testing.assert_array_equal(hip["radii"], ref["radii"])
    worst = check_backward(scene, hip, _AsOracle(ref, scene), rel=REL, strict=True)
    print("C2 loss-derived, pairs", {k: f"{v[0]:.1e}" for k, v in worst.items()})
