"""GPU tests of the training data module (csrc/data.hip, soar_amd/data.py) against the torch-CPU restatement of the reference
(tests/data_ref.py): boxes, crops, the gathered frame, rays, matrices, reproducibility, the ring, and a batch through the renderer
plugin with the environment-map background and the avatar-stage loss.  Synthetic sequences from a seeded generator at 270 x 480
(270 is no multiple of 16 or of the vector width) and 1080 x 1920, and 54 x 98 where no frame starts on a 16-byte boundary;
frame 0's mask is cut by the image border (the crop box leaves the image: zero padding), frame 1's is a single pixel.

Bars.  Boxes: equal.  Crops: 1e-6 absolute against F.grid_sample on the CPU over ALL pixels -- none is set aside: the kernel's
sampling positions are torch's own bit for bit (tests/test_data_cpu.py), what is left are four products and three sums of values
in [0, 1].  The gathered frame: bit-equal to byte.float() / 255 * mask; the crops a batch carries: bit-equal to the store's rows
(the gather copies) and therefore 1e-6 from the restatement like them.  Unit rays: 1e-6 absolute.  Un-normalised rays, cam_d and
the matrices: 1e-6 relative to the largest magnitude.  rays_o, c2w and the per-camera vectors: bit-equal (they are not computed
on the device).  The ring holds data.RING_DEPTH = 4 batches."""
import random
import types

import pytest
import torch

import data_ref as R
from soar_amd import data as D

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = {"small": (6, 270, 480), "large": (16, 1080, 1920)}


@pytest.fixture(scope="module", params=["small", "large"])
def world(request):
    N, H, W = SIZES[request.param]
    seq = R.synthetic_sequence(N, H, W, seed=2)
    store = D.FrameStore.from_arrays(**seq, device=DEV)
    state = R.make_state({}, **seq, with_crops=False)            # the float video of the reference, on the host
    return types.SimpleNamespace(N=N, H=H, W=W, seq=seq, store=store, state=state)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def test_boxes_equal_nonzero_min_max(world):
    w = world
    boxes = w.store.boxes.cpu()
    assert boxes.dtype == torch.int32 and boxes.shape == (w.N, 4)
    for n in range(w.N):
        assert boxes[n].tolist() == R.mask_bbox(w.seq["masks"][n]).tolist(), n
    assert boxes[0, 0] == 0                                          # the blob cut by the border
    assert boxes[1, 0] == boxes[1, 2] and boxes[1, 1] == boxes[1, 3]  # the single pixel


def test_an_empty_mask_gives_the_sentinel_and_the_store_refuses_it():
    seq = R.synthetic_sequence(4, 54, 98, seed=5, empty=(2,))        # 54 x 98: rows and frames off every 16-byte boundary
    boxes = D.mask_bbox(seq["masks"].to(DEV)).cpu()
    assert boxes[2].tolist() == [98, 54, -1, -1]
    for n in (0, 1, 3):
        assert boxes[n].tolist() == R.mask_bbox(seq["masks"][n]).tolist()
    with pytest.raises(ValueError, match="frame 2"):
        D.FrameStore.from_arrays(**seq, device=DEV)


def test_crops_match_grid_sample(world):
    w = world
    frames = range(w.N) if w.N <= 6 else (0, 1, 2, w.N - 1)
    rgb, msk = w.store.rgb_crop.cpu(), w.store.mask_crop.cpu()
    assert rgb.shape == (w.N, 512, 512, 3) and msk.shape == (w.N, 512, 512)
    for n in frames:
        want_rgb, want_mask, _ = R.crop_frame(w.state.frames_img[n], w.state.frames_mask[n])
        e_rgb, e_mask = float((rgb[n] - want_rgb).abs().max()), float((msk[n] - want_mask).abs().max())
        print(f"{w.H}x{w.W} frame {n}: crop abs err rgb {e_rgb:.3g} mask {e_mask:.3g}")
        assert e_rgb <= 1e-6 and e_mask <= 1e-6, n
    assert float(rgb[0][:, :8].abs().max()) == 0.0                   # left of the image: zero padding
    assert float(msk[1].max()) > 0.0                                 # the single pixel is in its crop


def test_crops_off_the_vector_width():
    """54 x 98 frames: no row and no frame starts on a 16-byte boundary (the byte paths of the box scan and of the gather)."""
    seq = R.synthetic_sequence(6, 54, 98, seed=6)                    # (the reference's split needs five frames or more)
    store = D.FrameStore.from_arrays(**seq, device=DEV)
    imgs, masks = R.float_frames(seq["images"], seq["masks"])
    for n in range(6):
        want_rgb, want_mask, _ = R.crop_frame(imgs[n], masks[n])
        assert float((store.rgb_crop[n].cpu() - want_rgb).abs().max()) <= 1e-6
        assert float((store.mask_crop[n].cpu() - want_mask).abs().max()) <= 1e-6
    ds = D.RandomMultiviewCameraDataset(dict(height=64, width=64, batch_size=4, n_view=4, smpl_type="smplx"), store, "train")
    for i in range(6):
        b = ds.collate(None, gt_index=i)
        assert torch.equal(b["gt_rgb"].cpu(), imgs[i:i + 1]) and torch.equal(b["gt_mask"].cpu(), masks[i:i + 1])


def _dataset(w, B, res, normalize, strategy="dreamfusion"):
    cfg = dict(height=res, width=res, batch_size=B, n_view=4, smpl_type="smplx", rays_d_normalize=normalize, zoom_range=(0.9, 1.0),
               light_sample_strategy=strategy, elevation_range=(-10, 45), camera_distance_range=(0.8, 1.0), fovy_range=(15, 60))
    return cfg, D.RandomMultiviewCameraDataset(cfg, w.store, "train")


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("B,res", [(4, 512), (8, 64), (4, 64), (8, 512)])
def test_a_batch_matches_the_restatement(world, normalize, B, res):
    w = world
    cfg, ds = _dataset(w, B, res, normalize, "magic3d" if B == 8 else "dreamfusion")
    s = w.state
    s.cfg = types.SimpleNamespace(**dict(R.CFG_DEFAULTS, **cfg))
    s.heights, s.widths, s.batch_sizes, s.resolution_milestones = [res], [res], [B], [-1]
    s.directions_unit_focals = [R.get_ray_directions(H=res, W=res, focal=1.0)]
    s.elevation_range, s.azimuth_range = s.cfg.elevation_range, s.cfg.azimuth_range
    s.camera_distance_range, s.fovy_range, s.zoom_range = s.cfg.camera_distance_range, s.cfg.fovy_range, s.cfg.zoom_range
    R.update_step(s, 0)
    for frame in (0, 1, w.N // 2, w.N - 1):                          # the first and the last among them
        torch.manual_seed(10 + frame)
        random.seed(10 + frame)
        want = R.collate(s, gt_index=frame)
        torch.manual_seed(10 + frame)
        random.seed(10 + frame)
        got = ds.collate(None, gt_index=frame)
        assert set(R.KEYS) <= set(got)
        for k in ("gt_index", "height", "width", "gt_height", "gt_width", "gt_normal_res"):
            assert isinstance(got[k], int) and got[k] == want[k], k
        g = {k: v.cpu() for k, v in got.items() if torch.is_tensor(v) and k != "frames_rays_d"}
        for k, v in g.items():
            if k in want and want[k] is not None:
                assert v.shape == want[k].shape and v.dtype == torch.float32 and got[k].device == DEV, k
        # the frame: bit for bit
        for k in ("gt_rgb", "gt_mask", "gt_normal_F", "gt_normal_B", "gt_normal_mask"):
            assert torch.equal(g[k], want[k]), (frame, k)
        assert torch.equal(g["gt_rgb_crop"][0], w.store.rgb_crop[frame].cpu()) and torch.equal(g["gt_mask_crop"][0], w.store.mask_crop[frame].cpu())
        want_rgb, want_mask, _ = R.crop_frame(s.frames_img[frame], s.frames_mask[frame])
        assert float((g["gt_rgb_crop"][0] - want_rgb).abs().max()) <= 1e-6 and float((g["gt_mask_crop"][0] - want_mask).abs().max()) <= 1e-6
        # what travels through the launch untouched
        for k in ("c2w", "fovy", "elevation", "azimuth", "camera_distances", "camera_positions", "light_positions", "gt_c2w", "gt_fovx",
                  "gt_fovy", "gt_cx", "gt_cy", "gt_normal_fovx", "gt_normal_fovy", "gt_normal_cx", "gt_normal_cy", "gt_near", "rays_o",
                  "gt_rays_o"):
            assert torch.equal(g[k], want[k]), (frame, k)
        assert torch.equal(g["rays_o"], want["c2w"][:, None, None, :3, 3].expand(B, res, res, 3))
        for k in ("betas", "body_pose", "global_orient", "transl"):
            assert torch.equal(got["gt_smpl"][k].cpu(), want["gt_smpl"][k]), k
        # rays
        errs = {"gt_rays_d": float((g["gt_rays_d"] - want["gt_rays_d"]).abs().max()), "gt_cam_d": _rel(g["gt_cam_d"], want["gt_cam_d"]),
                "cam_d": _rel(g["cam_d"], want["cam_d"]),
                "rays_d": float((g["rays_d"] - want["rays_d"]).abs().max()) if normalize else _rel(g["rays_d"], want["rays_d"]),
                "mvp_mtx": _rel(g["mvp_mtx"], want["mvp_mtx"]), "gt_mvp_mtx": _rel(g["gt_mvp_mtx"], want["gt_mvp_mtx"]),
                "proj_mtx": _rel(g["proj_mtx"], R.get_projection_matrix(want["fovy"], 1.0, 0.1, 1000.0))}
        print(f"{w.H}x{w.W} B={B} res={res} normalize={normalize} frame {frame}:", {k: f"{v:.2g}" for k, v in errs.items()})
        assert all(v <= 1e-6 for v in errs.values()), errs
        if normalize:
            assert float((g["rays_d"].norm(dim=-1) - 1).abs().max()) <= 1e-6
    fr = ds.frames_rays_d
    assert fr.shape == (w.N, 512, 512, 3)
    for n in (0, w.N - 1):
        assert float((fr[n].cpu() - R.frame_rays_d(w.seq["normal_Ks"][n], w.seq["w2c"])[0]).abs().max()) <= 1e-6


def test_same_seed_same_bits_and_the_ring_keeps_its_depth(world):
    w = world
    _, ds = _dataset(w, 4, 64, False)
    _, ds2 = _dataset(w, 4, 64, False)

    def run(d, n):
        torch.manual_seed(7)
        random.seed(7)
        return [d.collate(None) for _ in range(n)]

    first = run(ds, 1)[0]
    kept = {k: v.clone() for k, v in first.items() if torch.is_tensor(v)}
    later = [ds.collate(None) for _ in range(D.RING_DEPTH - 1)]       # the ring is now full: `first` is its oldest batch
    assert len({b["gt_index"] for b in [first] + later}) > 1
    for k, v in kept.items():
        assert torch.equal(first[k], v), k                          # ... and untouched
    assert len({b["gt_rgb"].data_ptr() for b in [first] + later}) == D.RING_DEPTH == 4
    again = run(ds2, D.RING_DEPTH)
    for a, b in zip([first] + later, again):
        assert a["gt_index"] == b["gt_index"]
        for k, v in a.items():
            if torch.is_tensor(v):
                assert torch.equal(v, b[k]), k
    nxt = ds.collate(None)                                          # one more: the oldest batch's memory is used again
    assert nxt["gt_rgb"].data_ptr() == first["gt_rgb"].data_ptr()
    # the training iterator goes on for ever; the val split walks its frames in order
    it = iter(ds)
    assert all(next(it)["gt_index"] in ds.index_list for _ in range(3))
    dv = D.RandomMultiviewCameraDataset(dict(height=64, width=64, batch_size=4, n_view=4, smpl_type="smplx"), w.store, "val")
    assert [b["gt_index"] for b in dv] == R.split_indices(w.N, "val") and len(dv) == len(dv.index_list)


def test_a_batch_drives_the_renderer_the_background_and_the_avatar_loss():
    """End to end: dataset -> batch_forward (registered renderer, real NeuralEnvironmentMapBackground) -> avatar_stage_loss ->
    backward.  Everything finite; the background of the frame's view varies over the image (with the zero rays of a hand-made
    batch it is one colour)."""
    import test_plugin_gpu as TP
    from soar_amd import synthetic as syn
    from soar_amd.background import NeuralEnvironmentMapBackground as Env
    from soar_amd.losses import avatar_stage_loss
    from soar_amd.renderer import registry
    from soar_amd.smpl_guidance import SMPLGuidance
    import soar_amd.renderer  # noqa: F401
    torch.manual_seed(0)
    random.seed(0)
    seq = R.synthetic_sequence(TP.FRAMES, TP.H, TP.W, seed=3)
    store = D.FrameStore.from_arrays(**seq, device=DEV)
    ds = registry.find("mvdream-random-multiview-camera-datamodule")(
        dict(height=512, width=512, batch_size=4, n_view=4, smpl_type="smplx", rays_d_normalize=False, elevation_range=(0, 30),
             camera_distance_range=(0.8, 1.0), fovy_range=(15, 60), camera_perturb=0.0, center_perturb=0.0, up_perturb=0.0), store, "train")
    guide = SMPLGuidance(syn.make_body_model(0), TP._smpl_parms(syn.make_pose_sequence(TP.FRAMES, 0)), device=DEV)
    pc = TP.SurfelModel(syn.make_surfels(TP.P, 0), guide)
    renderer = registry.find("gaussiansurfel-rasterizer")({"use_explicit": True}, geometry=pc)
    env = renderer.background = Env({"random_aug": False}).to(DEV)
    batch = ds.collate(None, gt_index=2)
    assert float(batch["rays_d"].abs().max()) > 0 and float(batch["gt_rays_d"].std()) > 1e-4
    out, gt_out = renderer.batch_forward(batch)
    G = {k: v.permute(0, 3, 1, 2) for k, v in gt_out.items() if torch.is_tensor(v) and v.dim() == 4}
    frame = {"render": G["comp_rgb"][0], "mask": G["comp_mask"][0], "normal": torch.full((3, TP.H, TP.W), 0.5, device=DEV),
             "depth": G["comp_depth"][0], "curv": G["comp_curv"][0]}
    gt_rgb, gt_mask = batch["gt_rgb"][0].permute(2, 0, 1).contiguous(), batch["gt_mask"]
    loss = avatar_stage_loss(frame, gt_rgb, gt_mask, torch.zeros_like(gt_rgb), gt_mask[0] > 1e-5, lambda_normal=0.0)
    loss = loss + out["comp_rgb"].square().mean() + (gt_out["comp_bg"] * torch.linspace(-1, 1, 3, device=DEV)).mean()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for k, v in list(out.items()) + list(gt_out.items()):
        if torch.is_tensor(v) and v.is_floating_point():
            assert bool(torch.isfinite(v).all()), k
    for t in (pc._xyz, pc._rot, pc._scale, pc._color, env.network.layers[0].weight):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
    assert gt_out["comp_bg"].shape == (1, 512, 512, 3)
    assert float(gt_out["comp_bg"].detach().std()) > 1e-4, "comp_bg is one colour: the rays did not reach the background"
