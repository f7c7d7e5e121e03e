"""CPU tests of the training data module (soar_amd/data.py, csrc/data.hip): the restatement (tests/data_ref.py) against the
reference's key list and split, the host draw order of the dataset against the restatement bit for bit, the argument checks of the
three C calls (nothing is launched), the directory reader, and the crop kernel's position arithmetic -- restated in numpy, one
float32 rounding per line -- against F.grid_sample, with the share of pixels that sit on a tap boundary."""
import ctypes as C
import random
import types

import numpy as np
import pytest
import torch

import data_ref as R


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def _seq(N=6, H=54, W=96, seed=0):
    return R.synthetic_sequence(N, H, W, seed)


def test_restatement_has_the_reference_keys_and_shapes():
    seq = _seq()
    s = R.make_state(dict(height=64, width=64, batch_size=4, n_view=4, rays_d_normalize=False), **seq)
    torch.manual_seed(0)
    random.seed(0)
    b = R.collate(s)
    assert tuple(b) == R.KEYS and len(R.KEYS) == 40
    B, H, W = 4, 54, 96
    shapes = {"rays_o": (B, 64, 64, 3), "rays_d": (B, 64, 64, 3), "frames_rays_d": (6, 512, 512, 3), "cam_d": (B, 64, 64, 3),
              "mvp_mtx": (B, 4, 4), "camera_positions": (B, 3), "c2w": (B, 4, 4), "light_positions": (B, 3), "elevation": (B,),
              "azimuth": (B,), "camera_distances": (B,), "fovy": (B,), "gt_rays_o": (1, 512, 512, 3), "gt_rays_d": (1, 512, 512, 3),
              "gt_cam_d": (1, 512, 512, 3), "gt_mvp_mtx": (1, 4, 4), "gt_c2w": (1, 4, 4), "gt_rgb": (1, H, W, 3), "gt_mask": (1, H, W),
              "gt_rgb_crop": (1, 512, 512, 3), "gt_mask_crop": (1, 512, 512), "gt_normal_F": (1, 512, 512, 3),
              "gt_normal_B": (1, 512, 512, 3), "gt_normal_mask": (1, 512, 512)}
    for k in ("gt_fovx", "gt_fovy", "gt_cx", "gt_cy", "gt_normal_fovx", "gt_normal_fovy", "gt_normal_cx", "gt_normal_cy", "gt_near"):
        shapes[k] = (1,)
    for k, shp in shapes.items():
        assert tuple(b[k].shape) == shp and b[k].dtype == torch.float32, k
    for k in ("gt_index", "height", "width", "gt_height", "gt_width", "gt_normal_res"):
        assert isinstance(b[k], int), k
    assert set(b["gt_smpl"]) == {"betas", "body_pose", "global_orient", "transl"}
    assert b["gt_index"] in s.index_list
    # un-normalised rays: cam_d rotated; normalised ones are unit vectors
    assert torch.allclose(b["gt_rays_d"].norm(dim=-1), torch.ones(1, 512, 512), atol=1e-6)
    assert float((b["rays_d"].norm(dim=-1) - 1).abs().max()) > 1e-3


@pytest.mark.parametrize("n", [10, 50, 400])
def test_split_agrees_with_the_reference_and_the_dataset(n):
    from soar_amd import data as D
    num_val = n // 5
    length = int(1 / num_val * n)
    val = list(range(n))[length // 2::length]
    for split, want in (("train", sorted(set(range(n)) - set(val))), ("test", val[:len(val) // 2]), ("val", val[len(val) // 2:])):
        assert sorted(R.split_indices(n, split)) == want
        assert D.split_indices(n, split) == R.split_indices(n, split)
    assert len(val) >= num_val and not set(R.split_indices(n, "train")) & set(val)
    with pytest.raises(ValueError, match="cannot be split"):
        D.split_indices(4, "train")


def _host_dataset(seq, cfg, split="train"):
    """The dataset over a store that holds only the host side (no device in this container): enough for _draw()."""
    from soar_amd import data as D
    N, H, W = seq["masks"].shape
    store = types.SimpleNamespace(device="cpu", n_frames=N, height=H, width=W, Ks_host=seq["Ks"], normal_Ks_host=seq["normal_Ks"],
                                  c2w_host=torch.inverse(seq["w2c"]), smpl_parms_host=seq["smpl_parms"], frames_rays_d=lambda: None)
    return D.RandomMultiviewCameraDataset(cfg, store, split)


@pytest.mark.parametrize("strategy", ["dreamfusion", "magic3d"])
def test_host_draw_order_is_the_reference_order_bit_for_bit(strategy):
    seq = _seq(N=10)
    cfg = dict(height=64, width=64, batch_size=4, n_view=4, smpl_type="smplx", light_sample_strategy=strategy, zoom_range=(0.9, 1.0),
               elevation_range=(-10, 45), camera_distance_range=(0.8, 1.0), fovy_range=(15, 60), index_range=(0, -1))
    ds = _host_dataset(seq, cfg)
    s = R.make_state(cfg, **seq, with_crops=False)
    assert ds.index_list == s.index_list and ds.index_range == (0, 10)
    seed = 3
    torch.manual_seed(seed)
    random.seed(seed)
    want = [R.collate(s) for _ in range(20)]
    torch.manual_seed(seed)
    random.seed(seed)
    got = [ds._draw() for _ in range(20)]
    assert {g["elevation_uniform"] for g in got} == {True, False}, "the seed must reach both branches of random.random() < 0.5"
    assert len({g["gt_index"] for g in got}) > 1
    for g, w in zip(got, want):
        assert g["gt_index"] == w["gt_index"]
        for k in ("c2w", "fovy", "elevation", "azimuth", "camera_distances", "camera_positions", "light_positions", "gt_c2w", "gt_fovx",
                  "gt_fovy", "gt_cx", "gt_cy", "gt_normal_fovx", "gt_normal_fovy", "gt_normal_cx", "gt_normal_cy", "gt_near"):
            assert g[k].shape == w[k].shape and torch.equal(g[k], w[k]), k
    # the val split walks its frames in order and draws no frame index
    dv = _host_dataset(seq, cfg, "val")
    assert [dv._draw(gt_index=i)["gt_index"] for i in dv.index_list] == R.split_indices(10, "val")


def test_update_step_follows_the_resolution_milestones():
    ds = _host_dataset(_seq(), dict(height=[64, 512], width=[64, 512], batch_size=[8, 4], n_view=4, resolution_milestones=[100]))
    assert (ds.height, ds.width, ds.batch_size) == (64, 64, 8)
    ds.update_step(0, 99)
    assert ds.height == 64
    ds.update_step(0, 100)
    assert (ds.height, ds.width, ds.batch_size) == (512, 512, 4)
    with pytest.raises(ValueError, match="at most 8"):
        _host_dataset(_seq(), dict(batch_size=16, n_view=4))
    with pytest.raises(ValueError, match="light sample strategy"):
        _host_dataset(_seq(), dict(light_sample_strategy="sun"))


def test_registered_under_the_reference_name_with_its_config_fields():
    import dataclasses
    import soar_amd.renderer  # noqa: F401
    from soar_amd import data as D
    from soar_amd.renderer import registry
    cls = registry.find("mvdream-random-multiview-camera-datamodule")
    assert cls is D.RandomMultiviewCameraDataset
    f = {x.name: x.default for x in dataclasses.fields(cls.Config) if x.default is not dataclasses.MISSING}
    assert f["n_view"] == 1 and f["zoom_range"] == (1.0, 1.0) and f["smpl_type"] == "smpl" and f["index_range"] == (0, 1)
    assert f["occ_range"] == 405 and f["occ_mid"] == 451 and f["occ_width"] == 86 and f["rays_d_normalize"] is True
    assert f["elevation_range"] == (-10, 90) and f["fovy_range"] == (40, 70) and f["light_sample_strategy"] == "dreamfusion"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.FrameStore.from_arrays(**_seq(N=2, H=8, W=8), device="cpu")


def test_data_calls_refuse_bad_arguments_before_any_launch(lib):
    from soar_amd import hip_lib
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)           # any non-NULL address: nothing reads it before the checks fail
    assert lib.soar_data_mask_bbox(2, 8, 8, None, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert lib.soar_data_mask_bbox(2, 0, 8, p, p, None) != 0 and "H=0" in hip_lib.last_error()
    assert lib.soar_data_mask_bbox(-1, 8, 8, p, p, None) != 0
    assert lib.soar_data_mask_bbox(0, 8, 8, None, None, None) == 0                 # nothing to do
    assert lib.soar_data_crops(2, 8, 8, p, p, None, p, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert lib.soar_data_crops(2, 8, 0, p, p, p, p, p, None) != 0 and "W=0" in hip_lib.last_error()
    assert lib.soar_data_step_batch(None, None) != 0 and "NULL args" in hip_lib.last_error()
    aligned = C.c_void_p(0x1000)

    def args(**kw):
        a = hip_lib.SoarDataStepArgs()
        a.B, a.H, a.W, a.n_frames, a.Hv, a.Wv, a.frame = 4, 64, 64, 10, 270, 480, 3
        a.near_plane, a.far_plane, a.gt_near = 0.1, 1000.0, 3.0
        for name in ("images", "masks", "normal_F", "normal_B", "normal_mask", "rgb_crop", "mask_crop", "normal_Ks", "rays_d", "cam_d",
                     "gt_rays_d", "gt_cam_d", "gt_rgb", "gt_mask", "gt_normal_F", "gt_normal_B", "gt_normal_mask", "gt_rgb_crop",
                     "gt_mask_crop", "mvp_mtx", "proj", "gt_mvp_mtx", "small_out"):
            setattr(a, name, aligned)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, word in ((dict(B=9), "B=9"), (dict(B=-1), "B=-1"), (dict(H=0), "zero-size"), (dict(W=0), "zero-size"),
                     (dict(Hv=0), "zero-size"), (dict(frame=10), "out of range"), (dict(frame=-1), "out of range"),
                     (dict(images=None), "NULL source"), (dict(masks=None), "NULL source"), (dict(normal_Ks=None), "NULL normal_Ks"),
                     (dict(rgb_crop=None), "NULL source"), (dict(n_small=257), "n_small"), (dict(far_plane=0.05), "far_plane"),
                     (dict(gt_rgb=C.c_void_p(0x1004)), "16-byte")):
        assert lib.soar_data_step_batch(C.byref(args(**kw)), None) != 0, kw
        assert word in hip_lib.last_error(), (kw, hip_lib.last_error())
    # nothing wanted: nothing launched, no error
    empty = hip_lib.SoarDataStepArgs()
    assert lib.soar_data_step_batch(C.byref(empty), None) == 0
    assert C.sizeof(hip_lib.SoarDataStepArgs) < 4096                               # travels in the kernel's arguments


def test_read_dataroot_round_trips_a_png_directory(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from soar_amd import data as D
    seq = _seq(N=3, H=20, W=28)
    for d in ("images", "masks", "normal_F", "normal_B", "smplx"):
        (tmp_path / d).mkdir()
    seq["masks"][2] *= 200                                      # any non-zero value is "inside"
    for i in range(3):
        if i == 1:                                              # one frame carries its mask as alpha
            rgba = torch.cat([seq["images"][i], (seq["masks"][i] * 255)[..., None]], dim=-1).numpy()
            Image.fromarray(rgba, "RGBA").save(tmp_path / "images" / f"{i:04d}.png")
        else:
            Image.fromarray(seq["images"][i].numpy(), "RGB").save(tmp_path / "images" / f"{i:04d}.png")
        Image.fromarray(seq["masks"][i].numpy(), "L").save(tmp_path / "masks" / f"{i:04d}.png")
        nf = torch.cat([seq["normal_F"][i], seq["normal_mask"][i][..., None]], dim=-1).numpy()
        Image.fromarray(nf, "RGBA").save(tmp_path / "normal_F" / f"{i:04d}.png")
        Image.fromarray(seq["normal_B"][i].numpy(), "RGB").save(tmp_path / "normal_B" / f"{i:04d}.png")
    w2c_file = seq["w2c"].clone()
    w2c_file[1:3] *= -1                                          # the file holds the extrinsic BEFORE the reader's flip
    torch.save(dict(w2c=w2c_file, Ks=seq["Ks"], normal_Ks=seq["normal_Ks"], **seq["smpl_parms"]), tmp_path / "smplx" / "params.pth")
    got = D.FrameStore.read_dataroot(str(tmp_path), "smplx")
    for k in ("images", "normal_F", "normal_B", "normal_mask"):
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], seq[k].numpy()), k
    assert np.array_equal(got["masks"], (seq["masks"] > 0).numpy().astype(np.uint8)) and got["masks"].max() == 1
    assert torch.equal(got["w2c"], seq["w2c"]) and torch.equal(got["Ks"], seq["Ks"]) and torch.equal(got["normal_Ks"], seq["normal_Ks"])
    for k, v in seq["smpl_parms"].items():
        assert torch.equal(got["smpl_parms"][k], v), k
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.FrameStore.from_dataroot(str(tmp_path), "smplx", device="cpu")
    (tmp_path / "normal_B" / "0002.png").unlink()
    with pytest.raises(ValueError, match="must agree"):
        D.FrameStore.read_dataroot(str(tmp_path), "smplx")


# ---- the crop kernel's arithmetic (csrc/data.hip: linspace_at, crop_position, crops_kernel), one float32 rounding per line --------
f32 = np.float32


def _fma(a, b, c):
    """a * b + c with one rounding (exact in float64 for float32 operands up to the final rounding)"""
    return (a.astype(np.float64) * np.float64(b) + np.float64(c)).astype(f32)


def kernel_crop_positions(box, size):
    """the pixel coordinates crops_kernel samples along one axis for the inclusive integer box (lo, hi), as float32 [512]"""
    lo, hi, span = box
    c = f32(f32(lo) + f32(f32(hi - lo) / f32(2)))
    hs = f32(np.float64(span) * 1.1 / 2.0)
    start, end = f32(c - hs), f32(c + hs)
    step = f32(f32(end - start) / f32(R.CROP - 1))
    i = np.arange(R.CROP)
    lin = np.where(i < R.CROP // 2, _fma(i.astype(f32), step, start), _fma((R.CROP - 1 - i).astype(f32), -step, end))
    g = (lin / f32(size)).astype(f32)
    g = (g * f32(2)).astype(f32)
    g = (g - f32(1)).astype(f32)
    return _fma((g + f32(1)).astype(f32), f32(size) / f32(2), f32(-0.5))


def kernel_crop(img, mask):
    """crops_kernel for one frame in numpy (the taps and weights in float32, the four-term sum in float64: it is not what is pinned)"""
    H, W = mask.shape
    b = R.mask_bbox(mask).tolist()
    span = max(b[2] - b[0], b[3] - b[1])
    x, y = kernel_crop_positions((b[0], b[2], span), W), kernel_crop_positions((b[1], b[3], span), H)
    x0, y0 = np.floor(x), np.floor(y)
    wx, wy = (x - x0).astype(f32), (y - y0).astype(f32)
    src = np.concatenate([img.numpy(), mask.numpy()[..., None]], axis=-1).astype(np.float64)
    pad = np.zeros((H + 2, W + 2, 4))
    out = np.zeros((R.CROP, R.CROP, 4))
    pad[1:-1, 1:-1] = src
    for dy in (0, 1):
        for dx in (0, 1):
            ix, iy = np.clip(x0.astype(np.int64) + dx + 1, 0, W + 1), np.clip(y0.astype(np.int64) + dy + 1, 0, H + 1)
            wgt = np.outer((wy if dy else f32(1) - wy), (wx if dx else f32(1) - wx)).astype(np.float64)
            out += pad[iy][:, ix] * wgt[..., None]
    return out, (wx, wy)


@pytest.mark.parametrize("hw", [(270, 480), (1080, 1920)])
def test_the_crop_arithmetic_of_the_kernel_is_grid_samples(hw):
    """The positions of the kernel are F.grid_sample's own, bit for bit (torch's fused linspace and un-normalisation included), so
    no pixel has to be set aside for a tap that flips: the 1e-6 bar is about the four products and three sums only."""
    H, W = hw
    seq = R.synthetic_sequence(3, H, W, seed=1)
    imgs, masks = R.float_frames(seq["images"], seq["masks"])
    for n in range(3):
        want_rgb, want_mask, grid = R.crop_frame(imgs[n], masks[n])
        got, _ = kernel_crop(imgs[n], masks[n])
        err = np.abs(got - torch.cat([want_rgb, want_mask[..., None]], dim=-1).numpy().astype(np.float64))
        fx, fy = R.crop_fractions(grid, H, W)
        near = ((fx < 1e-4) | (fx > 1 - 1e-4) | (fy < 1e-4) | (fy > 1 - 1e-4)).numpy()
        print(f"{H}x{W} frame {n}: max err {err.max():.3g} over ALL pixels; {near.mean():.5f} of them within 1e-4 of a tap boundary")
        assert err.max() <= 1e-6
