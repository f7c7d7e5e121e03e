"""MJPEG video output on the device: soar_amd.video.encode_jpeg against the NumPy restatement (tests/jpeg_ref.py) byte for byte, header
included, and against Pillow's scan bytes; the output buffer's guard bytes; MjpegWriter; play(video=) and save_strips(video=)."""
import io
import types

import numpy as np
import pytest
import torch

import jpeg_ref as J
from test_video_cpu import make_image, pillow_jpeg, split_jpeg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 0xAB

_REF = {}


def ref_file(img, quality, subsampling, restart):
    """the restatement's complete file for a host image (computed once per case)"""
    from soar_amd.video import jpeg_tables
    key = (img.shape, img.tobytes(), quality, subsampling, restart)
    if key not in _REF:
        _REF[key] = J.jpeg_file(img, jpeg_tables(quality), subsampling, restart)
    return _REF[key]


def decode(jpeg):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpeg)).convert("RGB"))


def files_of(data, offsets):
    host, off = data.cpu().numpy().tobytes(), offsets.cpu().tolist()
    return [host[off[i]:off[i + 1]] for i in range(len(off) - 1)]


@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("size", [(1, 1), (8, 8), (17, 23), (16, 17), (24, 8), (33, 70)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_jpeg_equals_the_restatement_and_pillows_scan(size, subsampling):
    from soar_amd.video import encode_jpeg
    for kind in ("noise", "extremes"):
        img = make_image(kind, *size)
        frames = torch.from_numpy(img)[None].to(DEV)
        for quality in (50, 90, 100):
            for restart in (1, 3, 7, 1000):                       # 1000: above the MCU count
                data, offsets = encode_jpeg(frames, quality=quality, subsampling=subsampling, restart_interval=restart)
                want = ref_file(img, quality, subsampling, restart)
                got = files_of(data, offsets)
                assert offsets.dtype == torch.int64 and offsets.cpu().tolist() == [0, len(want)], (kind, quality, restart)
                assert got == [want], (kind, quality, restart)
                assert split_jpeg(got[0])[1] == split_jpeg(pillow_jpeg(img, quality, subsampling, restart))[1], (kind, quality, restart)


@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("slack", [52, 51], ids=["stride on 4 bytes", "odd stride"])
def test_a_strided_rgba_batch_into_a_guarded_buffer_equals_the_single_calls(subsampling, slack):
    from soar_amd.video import encode_jpeg
    H, W, B = 17, 23, 3
    imgs = [make_image("noise", H, W, seed=i) for i in range(B)]
    alpha = make_image("noise", H, W, seed=9)[..., :1]
    store = torch.full((B, H * W * 4 + slack), 7, dtype=torch.uint8, device=DEV)
    frames = store[:, :H * W * 4].view(B, H, W, 4)
    frames.copy_(torch.from_numpy(np.stack([np.concatenate([im, alpha], axis=2) for im in imgs])).to(DEV))
    assert frames.stride(0) == H * W * 4 + slack and frames.data_ptr() == store.data_ptr()
    want = [ref_file(im, 90, subsampling, 3) for im in imgs]
    total = sum(len(f) for f in want)
    big = torch.full((total + 64,), GUARD, dtype=torch.uint8, device=DEV)
    data, offsets = encode_jpeg(frames, quality=90, subsampling=subsampling, restart_interval=3, out=big[:total])
    assert data.data_ptr() == big.data_ptr()
    assert offsets.cpu().tolist() == [0] + list(np.cumsum([len(f) for f in want]))              # exact
    assert files_of(data, offsets) == want
    assert bool((big[total:] == GUARD).all())
    for i in range(B):                                            # a frame's bytes depend neither on the batch nor on its place
        one, off = encode_jpeg(frames[i:i + 1, :, :, :3].contiguous(), quality=90, subsampling=subsampling, restart_interval=3)
        assert files_of(one, off) == [want[i]]


def test_a_batch_cut_out_of_a_taller_buffer_is_encoded_where_it_lies():
    """big[:, :H]: every frame contiguous, the step from frame to frame wider than a frame; no copy is made of it"""
    from soar_amd import codec_io
    from soar_amd.video import encode_jpeg
    H, W, B = 17, 13, 3
    imgs = [make_image(k, H, W, seed=i) for i, k in enumerate(("noise", "blob", "ramp"))]
    big = torch.full((B, H + 5, W, 3), 7, dtype=torch.uint8, device=DEV)
    frames = big[:, :H]
    frames.copy_(torch.from_numpy(np.stack(imgs)).to(DEV))
    assert not frames.is_contiguous()
    _, pointer, stride = codec_io.batch_view("encode_jpeg", frames)
    assert pointer == big.data_ptr() and stride == (H + 5) * W * 3
    want = [ref_file(im, 90, "420", 3) for im in imgs]
    assert files_of(*encode_jpeg(frames, quality=90, subsampling="420", restart_interval=3)) == want
    for i in range(B):
        assert files_of(*encode_jpeg(frames[i:i + 1], quality=90, subsampling="420", restart_interval=3)) == [want[i]]
    assert bool((big[:, H:] == 7).all())


def test_an_empty_batch_gives_the_offsets_of_nothing():
    from soar_amd.video import encode_jpeg
    data, offsets = encode_jpeg(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=DEV))
    assert data.numel() == 0 and offsets.dtype == torch.int64 and offsets.cpu().tolist() == [0]


def test_a_frame_stride_past_2_to_the_31_bytes():
    """two small frames 2^31 + 4096 bytes apart in one (untouched) allocation: the frame's address is 64-bit arithmetic"""
    from soar_amd.video import encode_jpeg
    H, W, step = 16, 17, 2 ** 31 + 4096
    imgs = [make_image("noise", H, W, seed=i) for i in range(2)]
    store = torch.empty(step + H * W * 3, dtype=torch.uint8, device=DEV)
    frames = store.as_strided((2, H, W, 3), (step, W * 3, 3, 1))
    frames.copy_(torch.from_numpy(np.stack(imgs)).to(DEV))
    data, offsets = encode_jpeg(frames, quality=90, subsampling="420", restart_interval=1)
    assert files_of(data, offsets) == [ref_file(im, 90, "420", 1) for im in imgs]


def test_a_too_small_out_is_reported_and_nothing_is_written():
    from soar_amd.video import encode_jpeg
    img = make_image("noise", 33, 70)
    frames = torch.from_numpy(np.stack([img, img[::-1].copy()])).to(DEV)
    want = [ref_file(img, 90, "420", 3), ref_file(img[::-1].copy(), 90, "420", 3)]
    total = len(want[0]) + len(want[1])
    for capacity in (total - 1, len(want[0]), 0):
        big = torch.full((total + 64,), GUARD, dtype=torch.uint8, device=DEV)
        data, offsets = encode_jpeg(frames, quality=90, subsampling="420", restart_interval=3, out=big[:capacity])
        assert int(offsets[-1]) == total > data.numel() == capacity                # the need is reported ...
        assert offsets.cpu().tolist() == [0, len(want[0]), total]
        assert bool((big == GUARD).all())                                          # ... and nothing was written, in or behind out


def test_interval_boundaries_on_a_medium_frame():
    """270 x 480 at 4:2:0: 17 x 30 = 510 MCUs, not a multiple of the default interval; 270 is even and no multiple of 16"""
    from soar_amd.video import DEFAULT_RESTART_INTERVAL, encode_jpeg
    ri = DEFAULT_RESTART_INTERVAL["420"]
    assert 510 % ri
    img = np.random.RandomState(3).randint(0, 256, (270, 480, 3)).astype(np.uint8)
    data, offsets = encode_jpeg(torch.from_numpy(img)[None].to(DEV), quality=90, subsampling="420")
    got = files_of(data, offsets)
    assert got == [ref_file(img, 90, "420", ri)]
    assert split_jpeg(got[0])[1] == split_jpeg(pillow_jpeg(img, 90, "420", ri))[1]


def test_save_jpeg_writes_a_file_pillow_opens(tmp_path):
    from soar_amd.video import save_jpeg
    img = make_image("blob", 30, 5)
    path = tmp_path / "still.jpg"
    save_jpeg(str(path), torch.from_numpy(img).to(DEV), quality=50, subsampling="420", restart_interval=7)
    assert path.read_bytes() == ref_file(img, 50, "420", 7)
    assert decode(path.read_bytes()).shape == (30, 5, 3)


def test_mjpeg_writer_round_trip_in_chunks_of_two(tmp_path):
    from soar_amd.video import DEFAULT_RESTART_INTERVAL, MjpegWriter, read_mjpeg_avi
    H, W = 40, 56
    imgs = [make_image("blob" if i & 1 else "noise", H, W, seed=i) for i in range(5)]
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    path = str(tmp_path / "clip.avi")
    with MjpegWriter(path, H, W, fps=25, quality=90) as w:
        for f0 in range(0, 5, 2):
            w.write(frames[f0:f0 + 2])
    got = read_mjpeg_avi(path)
    want = [ref_file(im, 90, "420", DEFAULT_RESTART_INTERVAL["420"]) for im in imgs]
    assert w.frames == 5 and len(got) == 5
    assert w.bytes_to_host == sum(len(f) for f in want)           # the compressed bytes, and nothing else, crossed to the host
    for i in range(5):
        assert np.array_equal(decode(got[i]), decode(want[i])), i
        assert got[i] == want[i], i
    with pytest.raises(ValueError, match="expected"):
        MjpegWriter(str(tmp_path / "other.avi"), H, W + 1).write(frames)


# ---- the two callers ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    """the tiny world of tests/test_playback_gpu.py"""
    import test_playback_gpu as T
    from soar_amd import playback as pb
    from soar_amd import synthetic as syn
    from soar_amd.renderer import cameras
    from soar_amd.smpl_guidance import SMPLGuidance
    body = syn.make_body_model(0, V=2048)
    parms = T._smpl_parms(syn.make_pose_sequence(T.KEYS, 0))
    guide = SMPLGuidance(body, parms, device=DEV)
    player = pb.AvatarPlayer.from_checkpoint(T._checkpoint(syn.make_surfels(T.P, 0)), guide)
    spec = syn.make_camera(T.W, T.H, distance=3.0, elevation=0.1, azimuth=0.4)
    cam = cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(DEV), image_width=T.W, image_height=T.H,
                         world_view_transform=spec.world_view_transform.to(DEV), full_proj_transform=spec.full_proj_transform.to(DEV),
                         prcppoint=spec.prcppoint.to(DEV))
    poses = player.resample(parms, [0.0, 0.6, 1.5, 2.25, 3.0])
    return types.SimpleNamespace(player=player, cam=cam, poses=poses)


def test_play_with_video_writes_three_avi_files_of_the_rendered_bytes(world, tmp_path):
    from soar_amd.video import DEFAULT_RESTART_INTERVAL, read_mjpeg_avi
    w = world
    res = w.player.play(w.poses, w.cam, str(tmp_path / "with"), chunk=2, video=True)
    plain = w.player.play(w.poses, w.cam, str(tmp_path / "without"), chunk=2)
    pngs = [f"{i:05d}.png" for i in range(5)]
    for k in ("rgb", "normal", "occ", "mask"):
        assert torch.equal(res[k], plain[k])
        assert sorted(p.name for p in (tmp_path / "without" / k).iterdir()) == pngs                      # what it held before
        assert sorted(p.name for p in (tmp_path / "with" / k).iterdir()) == pngs + (["video.avi"] if k != "mask" else [])
        for i in range(5):
            assert (tmp_path / "with" / k / pngs[i]).read_bytes() == (tmp_path / "without" / k / pngs[i]).read_bytes()
    for k in ("rgb", "normal", "occ"):
        frames = read_mjpeg_avi(str(tmp_path / "with" / k / "video.avi"))
        host = res[k].cpu().numpy()
        assert len(frames) == 5
        for i in range(5):
            want = ref_file(np.ascontiguousarray(host[i, :, :, :3]), 90, "420", DEFAULT_RESTART_INTERVAL["420"])      # the alpha is dropped
            assert np.array_equal(decode(frames[i]), decode(want)), (k, i)
    # the options reach the writer
    w.player.play(w.poses, w.cam, str(tmp_path / "opts"), chunk=8, video=dict(fps=10, quality=50, subsampling="444"))
    frames = read_mjpeg_avi(str(tmp_path / "opts" / "rgb" / "video.avi"))
    want = ref_file(np.ascontiguousarray(res["rgb"].cpu().numpy()[4, :, :, :3]), 50, "444", DEFAULT_RESTART_INTERVAL["444"])
    assert len(frames) == 5 and frames[4] == want


def test_save_strips_with_video_writes_the_avi_next_to_the_pngs(tmp_path):
    from soar_amd.fitviz import save_strips
    from soar_amd.video import DEFAULT_RESTART_INTERVAL, read_mjpeg_avi
    strips = np.stack([make_image("blob", 20, 50), make_image("noise", 20, 50)])
    dev = torch.from_numpy(strips).to(DEV)
    save_strips(dev, str(tmp_path / "plain"))
    save_strips(dev, str(tmp_path / "video"), video=dict(fps=5, quality=90))
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["00000.png", "00001.png"]
    assert sorted(p.name for p in (tmp_path / "video").iterdir()) == ["00000.png", "00001.png", "video.avi"]
    for n in ("00000.png", "00001.png"):
        assert (tmp_path / "video" / n).read_bytes() == (tmp_path / "plain" / n).read_bytes()
    frames = read_mjpeg_avi(str(tmp_path / "video" / "video.avi"))
    assert len(frames) == 2
    for i in range(2):
        want = ref_file(strips[i], 90, "420", DEFAULT_RESTART_INTERVAL["420"])
        assert np.array_equal(decode(frames[i]), decode(want)), i
