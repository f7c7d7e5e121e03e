"""GPU tests of avatar playback (soar_amd/playback.py, csrc/playback.hip): the motion kernel against its float64
restatement, the turntable, the output stage against torch's expression bit for bit, and the player against one plugin ``forward`` per
frame."""
import math
import types

import numpy as np
import pytest
import torch

import playback_ref as R
from soar_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# The bound on rotation-matrix entries between the kernel and the float64 restatement: 4 times the worst difference between the
# float32 and the float64 restatement on the inputs of playback_ref.motion_case() (measured: 4.4745e-07 with the turn of the root,
# 3.5935e-07 without).  The factor covers the device's sin / cos / acos / atan2, which differ from NumPy's by a few ulp.
MOTION_MEASURED = 4.4745e-07
MOTION_BOUND = 4 * MOTION_MEASURED

P, W, H, KEYS = 2000, 96, 64, 4
# Pixels allowed to differ by one byte level between the player and one forward() per frame: none.  The existing tests hold the
# batched path and the per-view path equal bit for bit (test_plugin_gpu.py: test_the_seven_views_of_a_step_as_one_node_equal_the_
# per_pose_nodes, test_plugin_default_sizes_binning_buffers_from_earlier_frames), and the per-view path against itself across chunk
# sizes gives identical floats, so identical bytes.
ONE_LEVEL_CAP = 0.0


def torch_bytes(x: torch.Tensor) -> torch.Tensor:
    """torchvision's save_image conversion on the CPU; NaN -> 0 (torch leaves it undefined, the kernel defines it)"""
    x = x.detach().cpu()
    b = x.clone().mul(255).add_(0.5).clamp_(0, 255).nan_to_num_(nan=0.0).to(torch.uint8)
    return b


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. motion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("turn", [False, True], ids=["plain", "yaw"])
def test_motion_resample_matches_the_float64_restatement(turn):
    from soar_amd import playback as pb
    kp, kt, ke, t, yaw = R.motion_case()
    yw = yaw if turn else None
    # the bound is what it says: the float32 restatement against the float64 one, on these inputs
    p64, t64, e64 = R.motion_resample(kp, kt, ke, t, yw, np.float64)
    p32, t32, e32 = R.motion_resample(kp, kt, ke, t, yw, np.float32)
    measured = np.abs(R.rotation_matrices(p32) - R.rotation_matrices(p64)).max()
    print(f"float32 against float64 restatement: {measured:.4e} (recorded {MOTION_MEASURED:.4e})")
    assert measured <= MOTION_MEASURED * 1.0001
    pose, transl, expr = pb.motion_resample(dev(kp), dev(kt), dev(ke), dev(t), None if yw is None else dev(yw))
    pose = pose.cpu().numpy().reshape(len(t), R.JOINTS, 3)
    assert pose.shape == p64.shape and np.isfinite(pose).all()
    err = np.abs(R.rotation_matrices(pose) - R.rotation_matrices(p64))
    print(f"kernel against float64 restatement: {err.max():.4e} (bound {MOTION_BOUND:.4e}), worst joint {np.unravel_index(err.argmax(), err.shape)}")
    assert err.max() <= MOTION_BOUND
    # on a key without a turn: the key's rotation (its own numbers, in fact)
    for f, k in ((0, 0), (1, 2), (2, 1)):
        joints = slice(1, None) if turn and yaw[f] != 0 else slice(None)
        assert np.abs(R.rotation_matrices(pose[f, joints]) - R.rotation_matrices(kp[k, joints])).max() <= MOTION_BOUND
        if not turn or yaw[f] == 0:
            assert np.array_equal(pose[f], kp[k])
    # every result is the canonical vector (angle in [0, pi]) unless it is a key copied as it is
    off_key = [f for f in range(len(t)) if t[f] != np.floor(t[f])]
    assert np.linalg.norm(pose[off_key], axis=-1).max() <= np.pi * (1 + 1e-6)
    # transl and expression: the float32 lerp to within 1 ulp
    for got, want in ((transl.cpu().numpy(), t32), (expr.cpu().numpy(), e32)):
        assert (np.abs(got - want) <= np.spacing(np.abs(want))).all(), np.abs(got - want).max()


# ---- the world of the turntable, player and file tests --------------------------------------------------------------------------
def _smpl_parms(poses):
    fp = poses["full_pose"]
    return {"betas": poses["betas"], "expression": poses["expression"], "global_orient": fp[:, :3], "body_pose": fp[:, 3:66],
            "jaw_pose": fp[:, 66:69], "leye_pose": fp[:, 69:72], "reye_pose": fp[:, 72:75], "left_hand_pose": fp[:, 75:120],
            "right_hand_pose": fp[:, 120:165], "transl": poses["transl"]}


def _checkpoint(surf):
    """a checkpoint with the reference's key names over the synthetic surfels and a small seeded attribute field"""
    from soar_amd.field import HashMLPField
    torch.manual_seed(11)
    lo, hi = surf.xyz.min(0)[0], surf.xyz.max(0)[0]
    c = (lo + hi) / 2
    field = HashMLPField(torch.stack([(lo - c) * 1.5 + c, (hi - c) * 1.5 + c]), log2_hashmap_size=10)
    fsd = {k: v.clone() for k, v in field.state_dict().items()}
    fsd["encoding.hash_table"] *= 300.0                           # (an untrained table gives one grey: let the colours vary)
    g = torch.Generator().manual_seed(4)
    sd = {"geometry._xyz": surf.xyz.clone(), "geometry._rotation": surf.rot * 1.3, "geometry._colors": torch.logit(surf.colors.clamp(0.02, 0.98)),
          "geometry._occ": torch.logit(torch.rand(surf.xyz.shape[0], 1, generator=g).clamp(0.02, 0.98)),
          "geometry._scaling": torch.log(surf.scales[:, :1])}
    sd.update({"geometry.attribute_field." + k: v for k, v in fsd.items()})
    return {"state_dict": sd, "epoch": 0}


@pytest.fixture(scope="module")
def world():
    from soar_amd import playback as pb
    from soar_amd.renderer import cameras
    from soar_amd.smpl_guidance import SMPLGuidance
    body = syn.make_body_model(0, V=2048)
    parms = _smpl_parms(syn.make_pose_sequence(KEYS, 0))
    guide = SMPLGuidance(body, parms, device=DEV)
    player = pb.AvatarPlayer.from_checkpoint(_checkpoint(syn.make_surfels(P, 0)), guide)
    spec = syn.make_camera(W, H, distance=3.0, elevation=0.1, azimuth=0.4)
    cam = cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(DEV), image_width=W, image_height=H,
                         world_view_transform=spec.world_view_transform.to(DEV), full_proj_transform=spec.full_proj_transform.to(DEV),
                         prcppoint=spec.prcppoint.to(DEV))
    poses = player.resample(parms, [0.0, 0.6, 1.5, 2.25, 3.0])          # 5 frames: chunk = 2 leaves a ragged last chunk
    return types.SimpleNamespace(player=player, guide=guide, parms=parms, cam=cam, poses=poses, cache={})


# ---- 2. turntable ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 36])
def test_turntable_turns_the_first_frame_about_y(world, n):
    from soar_amd import playback as pb
    tt = world.player.turntable(n=n, frame=0)
    assert set(tt) == set(pb.POSE_KEYS) | {"betas", "transl", "expression"}
    g = world.guide.smpl_parms
    for k, width in zip(pb.POSE_KEYS, pb.POSE_WIDTHS):
        assert tt[k].shape == (n, width)
        if k != "global_orient":
            assert torch.equal(tt[k], g[k][0:1].expand(n, -1))
    assert torch.equal(tt["transl"], g["transl"][0:1].expand(n, -1)) and torch.equal(tt["expression"], g["expression"][0:1].expand(n, -1))
    assert tt["betas"].shape == (1, 10)
    go = tt["global_orient"].cpu().numpy()
    a0 = g["global_orient"][0].cpu().numpy()
    R0 = R.rotation_matrices(a0)
    want = R0 @ R.rot_y(2 * np.pi * np.arange(n) / n)
    err = np.abs(R.rotation_matrices(go) - want).max(axis=(1, 2))
    print(f"turntable n={n}: worst {err.max():.4e} at step {err.argmax()}, step n/2 {err[n // 2]:.4e} (bound {MOTION_BOUND:.4e})")
    assert np.isfinite(go).all() and err.max() <= MOTION_BOUND
    assert np.array_equal(go[0], a0)                                    # step 0 reproduces R0
    assert np.linalg.norm(go[1:], axis=1).max() <= np.pi * (1 + 1e-6)


# ---- 3. finish ------------------------------------------------------------------------------------------------------------------
def _finish_inputs(B, Hh, Ww, strided):
    """random images with the crafted values of the CPU test in the first and the last pixels of rows (and everywhere in between)"""
    rng = np.random.default_rng(5)
    v = R.crafted_values()
    ins = []
    for i, c in enumerate((3, 3, 1, 3)):
        x = rng.uniform(-0.1, 1.1, (B, c, Hh, Ww)).astype(np.float32)
        flat = x.reshape(-1)
        idx = rng.permutation(flat.size)[:min(v.size, flat.size // 2)]
        flat[idx] = np.roll(v, 97 * i)[:idx.size]
        edge = np.roll(v, 13 * i + 5)
        n = B * c * Hh
        x[..., 0] = edge[:n].reshape(B, c, Hh)
        x[..., Ww - 1] = edge[-n:].reshape(B, c, Hh)
        t = dev(x)
        if strided:                                                      # frames 5 planes apart, as a renderer's block leaves them
            big = torch.full((B, 5, Hh, Ww), float("nan"), device=DEV)
            big[:, :c] = t
            t = big[:, :c]
        ins.append(t)
    return ins


def _guarded(B, Hh, Ww):
    """the four output tensors with a guard row of sentinel bytes behind each"""
    bufs, out = {}, {}
    for k, px in (("rgb", 4), ("normal", 4), ("occ", 4), ("mask", 1)):
        n = B * Hh * Ww * px
        bufs[k] = torch.full((n + Ww * px,), 0xA5, dtype=torch.uint8, device=DEV)
        out[k] = bufs[k][:n].view((B, Hh, Ww, 4) if px == 4 else (B, Hh, Ww))
    return bufs, out


@pytest.mark.parametrize("shape,strided", [((2, 5, 67), False), ((2, 5, 67), True), ((2, 4, 68), False), ((3, 4, 68), True), ((1, 1, 1), False)],
                         ids=["5x67", "5x67-strided", "4x68-wide", "4x68-wide-strided", "1x1"])
def test_playback_finish_equals_torch_bit_for_bit(shape, strided):
    from soar_amd import playback as pb
    B, Hh, Ww = shape
    render, normal, mask, occ = _finish_inputs(B, Hh, Ww, strided)
    assert torch.isnan(render[..., 0]).any() or torch.isnan(normal).any() or torch.isnan(occ).any() or B * Hh * Ww == 1
    rgba = lambda img, m: torch.cat([torch_bytes(img), torch_bytes(m)], dim=1).permute(0, 2, 3, 1).contiguous()

    def run(occ_in, as_rgb):
        bufs, out = _guarded(B, Hh, Ww)
        res = pb.playback_finish(render, normal, mask, occ_in, normal_as_rgb=as_rgb, out=out)
        host = {k: v.cpu() for k, v in bufs.items()}                    # read back, then compared on the host
        for k, px in (("rgb", 4), ("normal", 4), ("occ", 4), ("mask", 1)):
            n = B * Hh * Ww * px
            assert bool((host[k][n:] == 0xA5).all()), f"guard row behind {k} was written"
            if k == "occ" and occ_in is None:
                assert bool((host[k] == 0xA5).all()) and res["occ"] is None
        return {k: (None if v is None else v.cpu()) for k, v in res.items()}

    full = run(occ, False)
    assert torch.equal(full["rgb"], rgba(render, mask)) and torch.equal(full["normal"], rgba(normal, mask))
    assert torch.equal(full["occ"], rgba(occ, mask)) and torch.equal(full["mask"], torch_bytes(mask)[:, 0])
    # the NumPy restatement says the same
    want = R.playback_finish(*[t.cpu().numpy() for t in (render, normal, mask, occ)])
    for k, a in zip(("rgb", "normal", "occ", "mask"), want):
        assert np.array_equal(full[k].numpy(), a), k
    no_occ = run(None, False)
    for k in ("rgb", "normal", "mask"):
        assert torch.equal(no_occ[k], full[k]), k
    as_rgb = run(occ, True)
    assert torch.equal(as_rgb["normal"], rgba(normal.cpu() * 0.5 + 0.5, mask)) and torch.equal(as_rgb["rgb"], full["rgb"])
    # without `out` the function allocates the same results
    plain = pb.playback_finish(render, normal, mask, occ)
    for k in full:
        assert torch.equal(plain[k].cpu(), full[k]), k


# ---- 4. player ------------------------------------------------------------------------------------------------------------------
def _per_frame_reference(w):
    """one plugin forward per frame under no_grad, pushed through torch's expression on the CPU (computed once, shared)"""
    if "ref" not in w.cache:
        pl = w.player
        bg = torch.ones(3, device=DEV)
        frames = []
        with torch.no_grad():
            for i in range(5):
                o = pl.renderer.forward(w.cam, bg, gt=True, gt_a_smpl=pl.frame_pose(w.poses, i))
                m = torch_bytes(o["mask"])
                frames.append({k: torch.cat([torch_bytes(o[src]), m], dim=0).permute(1, 2, 0).contiguous()
                               for k, src in (("rgb", "render"), ("normal", "normal"), ("occ", "occ"))} | {"mask": m[0]})
        w.cache["ref"] = {k: torch.stack([f[k] for f in frames]) for k in frames[0]}
    return w.cache["ref"]


def test_player_renders_what_one_forward_per_frame_renders(world):
    from soar_amd.renderer import fused_view
    w = world
    ref = _per_frame_reference(w)
    assert ref["rgb"].shape == (5, H, W, 4) and 0.02 < (ref["mask"] > 127).float().mean() < 0.9      # an avatar is in the picture
    assert ref["rgb"][..., :3].float().std() > 10 and ref["occ"][..., :3].float().std() > 1
    fused_view.capacity_book.reset()                 # chunk = 2 from a cold book: read-back frame, one-pose call, two-pose calls
    runs = []
    for chunk in (2, 2, 1, 8):
        got = {k: v.cpu() for k, v in w.player.render(w.poses, w.cam, chunk=chunk).items()}
        for k in ("rgb", "normal", "occ", "mask"):
            d = (got[k].int() - ref[k].int()).abs()
            share = (d > 0).float().mean().item()
            print(f"chunk {chunk} {k}: {share:.2e} of the bytes differ, worst by {int(d.max())}")
            assert int(d.max()) <= 1 and share <= ONE_LEVEL_CAP, (chunk, k)
        runs.append(got)
    for k in runs[0]:                                # two runs give identical bytes
        assert torch.equal(runs[0][k], runs[1][k]), k
    # normal_as_rgb only changes the normal image
    alt = w.player.render(w.poses, w.cam, chunk=2, normal_as_rgb=True)
    assert torch.equal(alt["rgb"].cpu(), runs[0]["rgb"]) and not torch.equal(alt["normal"].cpu(), runs[0]["normal"])
    w.cache["bytes"] = runs[0]


def test_player_joint_transforms_of_all_frames_equal_the_per_frame_ones(world):
    w = world
    mats = w.player.joint_mats(w.poses)
    assert mats.shape == (5, 55, 4, 4)
    for i in range(5):
        assert torch.equal(mats[i], w.guide.joint_mats(smpl_parms_in=w.player.frame_pose(w.poses, i)))


# ---- 5. files -------------------------------------------------------------------------------------------------------------------
def test_play_writes_the_four_folders(world, tmp_path):
    from PIL import Image
    w = world
    res = w.player.play(w.poses, w.cam, str(tmp_path), chunk=2)
    for k, mode in (("rgb", "RGBA"), ("normal", "RGBA"), ("occ", "RGBA"), ("mask", "L")):
        files = sorted(p.name for p in (tmp_path / k).iterdir())
        assert files == [f"{i:05d}.png" for i in range(5)]
        host = res[k].cpu().numpy()
        for i in range(5):
            img = Image.open(tmp_path / k / f"{i:05d}.png")
            assert img.mode == mode and img.size == (W, H)
            assert np.array_equal(np.asarray(img), host[i]), (k, i)
    assert not (tmp_path / "rgb" / "video.mp4").exists()
