"""PNG output on the device: soar_amd.png.encode_png against the restatement (tests/png_ref.py) byte for byte on every case of
tests/test_png_cpu.py; batches, strides, streams, the output buffer's guard bytes; and the six writers with ``device_png``."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import png_ref as P
import test_png_cpu as T
from test_video_gpu import world  # noqa: F401  (the fixture: the tiny world of tests/test_playback_gpu.py)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD = 0xAB

_REF = {}


def ref_file(img, filters, piece):
    """the restatement's file for a host image (computed once per case)"""
    key = (img.shape, img.tobytes(), filters, piece)
    if key not in _REF:
        _REF[key] = P.png_file(img, filters, piece)
    return _REF[key]


def files_of(data, offsets):
    host, off = data.cpu().numpy().tobytes(), offsets.cpu().tolist()
    return [host[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def first_difference(a, b):
    n = min(len(a), len(b))
    at = next((i for i in range(n) if a[i] != b[i]), n)
    return f"{len(a)} bytes against {len(b)}, first difference at {at}: {a[at:at + 8].hex()} against {b[at:at + 8].hex()}"


def same_pictures(a, b):
    """two folders (or files): the same names, and every pair decodes to the same pixels and mode"""
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names
    for n in names:
        if n.endswith(".png"):
            x, y = Image.open(os.path.join(a, n)), Image.open(os.path.join(b, n))
            assert x.mode == y.mode and x.size == y.size and np.array_equal(np.asarray(x), np.asarray(y)), n
    return names


@pytest.mark.parametrize("c", T.CHANNELS)
@pytest.mark.parametrize("shape", T.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encode_png_equals_the_restatement(shape, c):
    from soar_amd.png import encode_png
    for kind in T.KINDS:
        img = T.make_image(kind, *shape, c)
        dev = torch.from_numpy(img)[None].to(DEV)
        for f in T.FILTERS:
            for piece in T.PIECES:
                data, offsets = encode_png(dev, filters=f, piece_bytes=piece)
                want = ref_file(img, f, piece)
                got = files_of(data, offsets)
                assert offsets.dtype == torch.int64 and offsets.cpu().tolist() == [0, len(want)], (kind, f, piece)
                assert got == [want], (kind, f, piece, first_difference(got[0], want))


@pytest.mark.parametrize("case", T.EDGE_CASES + [("fibonacci", T.fibonacci_image()[0], 0, 65535)], ids=lambda t: t[0])
def test_edge_cases_equal_the_restatement(case):
    from soar_amd.png import encode_png
    name, img, f, piece = case
    data, offsets = encode_png(torch.from_numpy(img)[None].to(DEV), filters=f, piece_bytes=piece)
    want = ref_file(img, f, piece)
    got = files_of(data, offsets)
    assert got == [want], first_difference(got[0], want)


@pytest.mark.parametrize("c", [3, 4])
def test_the_avatar_like_image_at_the_default_piece_size(c):
    from soar_amd.png import encode_png
    img = T.avatar_image(c)
    data, offsets = encode_png(torch.from_numpy(img)[None].to(DEV))
    want = ref_file(img, "adaptive", P.DEFAULT_PIECE_BYTES)
    got = files_of(data, offsets)
    assert got == [want], first_difference(got[0], want)
    back = Image.open(io.BytesIO(got[0]))
    assert back.mode == T.MODES[c] and np.array_equal(np.asarray(back), img)


@pytest.mark.parametrize("slack", [52, 51], ids=["stride on 4 bytes", "odd stride"])
@pytest.mark.parametrize("c", T.CHANNELS)
def test_a_strided_batch_into_a_guarded_buffer_equals_the_single_calls(c, slack):
    from soar_amd.png import encode_png, png_bound
    H, W, B = 17, 23, 3
    imgs = [T.make_image(k, H, W, c, seed=i) for i, k in enumerate(("noise", "blob", "ramp"))]
    store = torch.full((B, H * W * c + slack), 7, dtype=torch.uint8, device=DEV)
    images = store[:, :H * W * c].view(B, H, W, c)
    images.copy_(torch.from_numpy(np.stack(imgs)).to(DEV))
    assert images.stride(0) == H * W * c + slack and images.data_ptr() == store.data_ptr()
    want = [ref_file(im, "adaptive", 256) for im in imgs]
    total = sum(len(f) for f in want)
    assert all(len(f) <= png_bound(H, W, c, 256) for f in want)
    big = torch.full((total + 64,), GUARD, dtype=torch.uint8, device=DEV)
    data, offsets = encode_png(images, piece_bytes=256, out=big[:total])            # an out of exact size: no read-back
    assert data.data_ptr() == big.data_ptr()
    assert offsets.cpu().tolist() == [0] + list(np.cumsum([len(f) for f in want]))
    assert files_of(data, offsets) == want
    assert bool((big[total:] == GUARD).all())
    for i in range(B):                                            # an image's bytes depend neither on the batch nor on its place
        one, off = encode_png(images[i:i + 1].contiguous(), piece_bytes=256)
        assert files_of(one, off) == [want[i]]


def test_a_batch_cut_out_of_a_taller_buffer_is_encoded_where_it_lies():
    """big[:, :H]: every image contiguous, the step from image to image wider than an image; no copy is made of it"""
    from soar_amd import codec_io
    from soar_amd.png import encode_png
    H, W, B = 17, 13, 3
    imgs = [T.make_image(k, H, W, 3, seed=i) for i, k in enumerate(("noise", "blob", "ramp"))]
    big = torch.full((B, H + 5, W, 3), 7, dtype=torch.uint8, device=DEV)
    images = big[:, :H]
    images.copy_(torch.from_numpy(np.stack(imgs)).to(DEV))
    assert not images.is_contiguous()
    _, pointer, stride = codec_io.batch_view("encode_png", images)
    assert pointer == big.data_ptr() and stride == (H + 5) * W * 3
    want = [ref_file(im, "adaptive", 256) for im in imgs]
    assert files_of(*encode_png(images, piece_bytes=256)) == want
    for i in range(B):
        assert files_of(*encode_png(images[i:i + 1], piece_bytes=256)) == [want[i]]
    assert bool((big[:, H:] == 7).all())


def test_an_image_stride_past_2_to_the_31_bytes():
    """two small images 2^31 + 4096 bytes apart in one (untouched) allocation: the image's address is 64-bit arithmetic"""
    from soar_amd.png import encode_png
    H, W, step = 16, 17, 2 ** 31 + 4096
    imgs = [T.make_image("blob", H, W, 3, seed=i) for i in range(2)]
    store = torch.empty(step + H * W * 3, dtype=torch.uint8, device=DEV)
    images = store.as_strided((2, H, W, 3), (step, W * 3, 3, 1))
    images.copy_(torch.from_numpy(np.stack(imgs)).to(DEV))
    data, offsets = encode_png(images, piece_bytes=256)
    assert files_of(data, offsets) == [ref_file(im, "adaptive", 256) for im in imgs]


def test_two_runs_and_a_side_stream_give_the_same_bytes():
    from soar_amd.png import encode_png
    imgs = np.stack([T.make_image(k, 33, 70, 4) for k in ("blob", "extremes", "noise", "white")])
    dev = torch.from_numpy(imgs).to(DEV)
    a, oa = encode_png(dev, piece_bytes=256)
    b, ob = encode_png(dev, piece_bytes=256)
    assert torch.equal(a, b) and torch.equal(oa, ob)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        c, oc = encode_png(dev, piece_bytes=256)
    side.synchronize()
    assert torch.equal(a, c) and torch.equal(oa, oc)
    assert files_of(a, oa) == [ref_file(im, "adaptive", 256) for im in imgs]


def test_an_empty_batch_gives_the_offsets_of_nothing():
    from soar_amd.png import encode_png
    data, offsets = encode_png(torch.empty((0, 5, 7, 3), dtype=torch.uint8, device=DEV))
    assert data.numel() == 0 and offsets.dtype == torch.int64 and offsets.cpu().tolist() == [0]


def test_a_too_small_out_is_reported_and_nothing_is_written():
    from soar_amd.png import encode_png
    a, b = T.make_image("blob", 33, 70, 3), T.make_image("noise", 33, 70, 3)
    images = torch.from_numpy(np.stack([a, b])).to(DEV)
    want = [ref_file(a, "adaptive", 256), ref_file(b, "adaptive", 256)]
    total = len(want[0]) + len(want[1])
    for capacity in (total - 1, len(want[0]), 0):
        big = torch.full((total + 64,), GUARD, dtype=torch.uint8, device=DEV)
        data, offsets = encode_png(images, piece_bytes=256, out=big[:capacity])
        assert int(offsets[-1]) == total > data.numel() == capacity                # the need is reported ...
        assert offsets.cpu().tolist() == [0, len(want[0]), total]
        assert bool((big == GUARD).all())                                          # ... and nothing was written, in or behind out


def test_cpu_tensors_wrong_dtypes_and_wrong_options_are_refused():
    from soar_amd.png import encode_png
    ok = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encode_png(ok.cpu())
    for bad in (ok.float(), ok.to(torch.int8), ok[0], ok[..., :2], torch.zeros((1, 8, 8, 5), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError, match="images must be uint8"):
            encode_png(bad)
    for f in (5, -1, "paeth", True):
        with pytest.raises(ValueError, match="filters"):
            encode_png(ok, filters=f)
    for piece in (31, 65536):
        with pytest.raises(ValueError, match="piece_bytes"):
            encode_png(ok, piece_bytes=piece)
    for out in (torch.zeros(4096, dtype=torch.uint8), torch.zeros(4096, dtype=torch.int8, device=DEV),
                torch.zeros((2, 4096), dtype=torch.uint8, device=DEV)):
        with pytest.raises(ValueError, match="out must be"):
            encode_png(ok, out=out)


def test_save_png_and_write_png_files(tmp_path):
    from soar_amd.png import save_png, write_png_files
    grey = T.make_image("blob", 30, 5, 1)
    save_png(str(tmp_path / "grey.png"), torch.from_numpy(grey[..., 0]).to(DEV))            # [H,W]
    assert (tmp_path / "grey.png").read_bytes() == ref_file(grey, "adaptive", P.DEFAULT_PIECE_BYTES)
    imgs = np.stack([T.make_image("blob" if i & 1 else "noise", 20, 30, 4, seed=i) for i in range(5)])
    paths = [str(tmp_path / f"{i}.png") for i in range(5)]
    copied = write_png_files(paths, torch.from_numpy(imgs).to(DEV), chunk=2)
    want = [ref_file(im, "adaptive", P.DEFAULT_PIECE_BYTES) for im in imgs]
    assert copied == sum(len(f) for f in want)                    # the compressed bytes, and nothing else, crossed to the host
    assert [open(p, "rb").read() for p in paths] == want
    with pytest.raises(ValueError, match="paths"):
        write_png_files(paths[:4], torch.from_numpy(imgs).to(DEV))


# ---- the six writers ----------------------------------------------------------------------------------------------------------------
def test_play_with_device_png_writes_the_same_pictures(world, tmp_path):  # noqa: F811
    """without device_png the files are Pillow's, as before"""
    w = world
    res = w.player.play(w.poses, w.cam, str(tmp_path / "device"), chunk=2, device_png=True)
    plain = w.player.play(w.poses, w.cam, str(tmp_path / "host"), chunk=2)
    for k in ("rgb", "normal", "occ", "mask"):
        assert torch.equal(res[k], plain[k])
        names = same_pictures(tmp_path / "device" / k, tmp_path / "host" / k)
        assert names == [f"{i:05d}.png" for i in range(5)]
        host = plain[k].cpu().numpy()
        for i, n in enumerate(names):
            b = io.BytesIO()
            Image.fromarray(host[i]).save(b, "PNG")
            assert (tmp_path / "host" / k / n).read_bytes() == b.getvalue()          # the default's bytes are those written before
            assert Image.open(tmp_path / "device" / k / n).mode == ("L" if k == "mask" else "RGBA")
            assert (tmp_path / "device" / k / n).read_bytes() == ref_file(host[i].reshape(host.shape[1], host.shape[2], -1), "adaptive",
                                                                          P.DEFAULT_PIECE_BYTES)


def test_save_masks_with_device_png(tmp_path):
    from soar_amd.masks import save_masks
    m = np.zeros((2, 20, 30), np.uint8)
    m[0, 3:9, 4:20] = 1
    m[1, ::3, ::2] = 200
    dev = torch.from_numpy(m).to(DEV)
    a = save_masks(dev, str(tmp_path / "device"), device_png=True)
    b = save_masks(dev, str(tmp_path / "host"))
    assert [os.path.relpath(p, tmp_path / "device") for p in a] == [os.path.relpath(p, tmp_path / "host") for p in b]
    assert same_pictures(tmp_path / "device" / "masks", tmp_path / "host" / "masks") == ["00000.png", "00001.png"]
    for i, p in enumerate(b):
        buf = io.BytesIO()
        Image.fromarray(((m[i] != 0) * np.uint8(255)).astype(np.uint8)).save(buf, "PNG")
        assert open(p, "rb").read() == buf.getvalue() and Image.open(a[i]).mode == "L"
    with pytest.raises(ValueError, match="device_png"):
        save_masks(m, str(tmp_path / "array"), device_png=True)


def test_save_normals_with_device_png(tmp_path):
    from soar_amd.normals import save_normals
    g = torch.Generator().manual_seed(5)
    N, H, W = 2, 24, 40
    res = dict(normal_F=torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(DEV),
               normal_B=torch.from_numpy(np.stack([T.make_image("blob", H, W, 3, seed=i) for i in range(N)])).to(DEV),
               normal_mask=(torch.randint(0, 2, (N, H, W), generator=g, dtype=torch.uint8) * 255).to(DEV))
    save_normals(res, str(tmp_path / "device"), device_png=True)
    save_normals(res, str(tmp_path / "host"))
    for name in ("normal_F", "normal_B"):
        assert same_pictures(tmp_path / "device" / name, tmp_path / "host" / name) == ["00000.png", "00001.png"]
        for i in range(N):
            rgba = np.concatenate([res[name][i].cpu().numpy(), res["normal_mask"][i].cpu().numpy()[..., None]], axis=-1)
            buf = io.BytesIO()
            Image.fromarray(rgba, "RGBA").save(buf, "PNG")
            assert (tmp_path / "host" / name / f"{i:05d}.png").read_bytes() == buf.getvalue()
            assert Image.open(tmp_path / "device" / name / f"{i:05d}.png").mode == "RGBA"


def test_save_strips_with_device_png(tmp_path):
    from soar_amd.fitviz import save_strips
    strips = np.stack([T.make_image("blob", 20, 50, 3), T.make_image("noise", 20, 50, 3)])
    dev = torch.from_numpy(strips).to(DEV)
    save_strips(dev, str(tmp_path / "device"), device_png=True)
    save_strips(dev, str(tmp_path / "host"))
    assert same_pictures(tmp_path / "device", tmp_path / "host") == ["00000.png", "00001.png"]
    for i in range(2):
        buf = io.BytesIO()
        Image.fromarray(strips[i]).save(buf, "PNG")
        assert (tmp_path / "host" / f"{i:05d}.png").read_bytes() == buf.getvalue()
        assert Image.open(tmp_path / "device" / f"{i:05d}.png").mode == "RGB"


def test_save_textured_obj_with_device_png(tmp_path):
    """the fixture of tests/test_texture_cpu.py's writer test"""
    import texture_ref as R
    from soar_amd import mesh
    fx, size = R.fixture("d"), 64
    a = R.build_atlas(fx.verts, fx.faces, size)
    atlas = mesh.Atlas(torch.from_numpy(a.uv), torch.from_numpy(a.uv_faces), torch.from_numpy(a.cell), a.scale_step, size)
    tex = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (size, size, 3), dtype=np.uint8))
    m = mesh.Mesh(torch.from_numpy(fx.verts), torch.from_numpy(fx.faces))
    (tmp_path / "device").mkdir()
    (tmp_path / "host").mkdir()
    mesh.save_textured_obj(str(tmp_path / "device" / "avatar.obj"), m, atlas, tex.to(DEV), device_png=True)
    mesh.save_textured_obj(str(tmp_path / "host" / "avatar.obj"), m, atlas, tex.to(DEV))
    assert same_pictures(tmp_path / "device", tmp_path / "host") == ["avatar.mtl", "avatar.obj", "avatar.png"]
    for n in ("avatar.mtl", "avatar.obj"):
        assert (tmp_path / "device" / n).read_bytes() == (tmp_path / "host" / n).read_bytes()
    buf = io.BytesIO()
    Image.fromarray(tex.numpy()).save(buf, "PNG")
    assert (tmp_path / "host" / "avatar.png").read_bytes() == buf.getvalue()
    back = Image.open(tmp_path / "device" / "avatar.png")
    assert back.mode == "RGB" and np.array_equal(np.asarray(back), tex.numpy())


def test_the_evaluator_writes_its_images_with_device_png(tmp_path):
    """finish(device_png=True) on an evaluator that holds two images: the same names and pixels as the default's files"""
    from soar_amd.evaluate import TestEvaluator
    g = torch.Generator().manual_seed(3)
    frames = [(torch.rand((1, 24, 36, 3), generator=g).to(DEV), torch.from_numpy(T.make_image(k, 24, 36, 3)[None] / np.float32(255)).to(DEV),
               torch.from_numpy((T.make_image("blob", 24, 36, 1)[None, ..., 0] < 250).astype(np.float32)).to(DEV)) for k in ("blob", "ramp")]
    kept = None
    for sub, flag in (("device", True), ("host", False)):
        ev = TestEvaluator(None, 2, keep_images=True)
        for index, (pred, gt, mask) in zip((3, 11), frames):
            ev.add(pred, {"gt_rgb": gt, "gt_mask": mask, "gt_index": index})
        ev.finish(str(tmp_path / sub), step=7, device_png=True) if flag else ev.finish(str(tmp_path / sub), step=7)
        kept = ev.images
    assert same_pictures(tmp_path / "device" / "it7-test", tmp_path / "host" / "it7-test") == ["11.png", "3.png"]
    for i, im in zip((3, 11), kept):
        buf = io.BytesIO()
        Image.fromarray(im.cpu().numpy()).save(buf, "PNG")
        assert (tmp_path / "host" / "it7-test" / f"{i}.png").read_bytes() == buf.getvalue()
        assert Image.open(tmp_path / "device" / "it7-test" / f"{i}.png").mode == "RGB"
