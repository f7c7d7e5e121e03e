"""PNG input on the device: soar_amd.png.decode_png against the restatement (tests/png_decode_ref.py) on every file of
tests/test_png_decode_cpu.py -- pixels, status and segments; malformed files between good ones, with guard bytes around the output and
the workspace (the same files the host build of csrc/png_inflate.h runs clean on under the sanitizers: they show refusal here, nothing
else); batches, streams and positions; the round trip through encode_png; read_png_files; and FrameStore.from_dataroot(device_png=True)
against the host path."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import png_decode_ref as D
import test_png_cpu as TE
import test_png_decode_cpu as T
from test_data_cpu import _seq

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, MARGIN = 0xAB, 4096


def upload(files):
    off = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    data = torch.frombuffer(bytearray(b"".join(files)) or bytearray(1), dtype=torch.uint8)[:int(off[-1])].to(DEV)
    return data, torch.from_numpy(off).to(DEV)


def run(files, shape, **kw):
    """-> (images, status, segments) as NumPy"""
    from soar_amd.png import decode_png
    data, offsets = upload(files)
    out, status, segments = decode_png(data, offsets, *shape, strict=False, return_info=True, **kw)
    return out.cpu().numpy(), status.cpu().numpy(), segments.cpu().numpy()


def by_shape():
    groups = {}
    for name, data, img, seg in T.corpus():
        groups.setdefault(img.shape, []).append((name, data))
    return sorted(groups.items())


@pytest.mark.parametrize("shape,files", by_shape(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_decode_png_equals_the_restatement_on_the_corpus(shape, files):
    out, status, segments = run([d for _, d in files], shape)
    for i, (name, data) in enumerate(files):
        want = T.decoded(name, data)
        assert status[i] == want.status == 0, (name, status[i])
        assert segments[i] == want.segments, (name, segments[i], want.segments)
        assert np.array_equal(out[i], want.image), name


def guarded_call(files, shape):
    """the C ABI itself, with out and the workspace inside larger buffers filled with a pattern -> (images, status) and the guards"""
    from soar_amd import hip_lib
    h, w, c = shape
    data, offsets = upload(files)
    B, n = len(files), h * w * c
    a = hip_lib.SoarPngDecodeArgs()
    a.B, a.H, a.W, a.channels, a.total_bytes = B, h, w, c, data.numel()
    a.data, a.offsets = data.data_ptr(), offsets.data_ptr()
    lib = hip_lib.lib()
    need = hip_lib._bytes(lib.soar_png_decode_workspace_bytes, "soar_png_decode_workspace_bytes", C.byref(a))
    ws = torch.full((need + 2 * MARGIN,), GUARD, dtype=torch.uint8, device=DEV)
    big = torch.full((B * n + 2 * MARGIN,), GUARD, dtype=torch.uint8, device=DEV)
    status = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    segments = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    assert (ws.data_ptr() + MARGIN) % 256 == 0
    hip_lib.check(lib.soar_png_decode(C.byref(a), ws.data_ptr() + MARGIN, need, big.data_ptr() + MARGIN, status.data_ptr() + 4,
                                      segments.data_ptr() + 4, torch.cuda.current_stream(DEV).cuda_stream), "soar_png_decode")
    torch.cuda.synchronize()
    guards = torch.cat([ws[:MARGIN], ws[MARGIN + need:], big[:MARGIN], big[MARGIN + B * n:]])
    assert bool((guards == GUARD).all()), "bytes outside the output or the workspace were written"
    assert status[0] == -7 and status[-1] == -7 and segments[0] == -7 and segments[-1] == -7
    return big[MARGIN:MARGIN + B * n].reshape(B, h, w, c).cpu().numpy(), status[1:-1].cpu().numpy()


def test_good_and_malformed_files_alternate_in_a_batch():
    shape, good = (7, 5, 3), T.good_file()
    image = D.decode(good).image
    bad = [(n, d) for n, d, _ in T.malformed()] + T.truncations()[::3]
    files, want = [], []
    for name, data in bad:
        files += [good, data]
        want += [0, D.decode(data, want=shape, report=False).status]
    files.append(good)
    want.append(0)
    assert all(s != 0 for s in want[1::2]) and set(want) == set(range(8))      # every status is met
    out, status = guarded_call(files, shape)
    assert status.tolist() == want, [(bad[i // 2][0], int(s), w) for i, (s, w) in enumerate(zip(status, want)) if s != w]
    for i, s in enumerate(want):
        assert np.array_equal(out[i], image) if s == 0 else not out[i].any(), i
    # another shape than the call's: every file is unsupported, nothing but zeros
    out, status = guarded_call([good, good], (7, 5, 4))
    assert status.tolist() == [D.UNSUPPORTED] * 2 and not out.any()


def test_runs_streams_batches_and_positions_give_the_same_bytes():
    img = TE.make_image("blob", 33, 70, 3)
    three = [T.pillow_file(img, compress_level=9), TE.P.png_file(img, "adaptive", 256), D.make_png(img, filters=4, level=1, idat_sizes=100)]
    singles = [run([f], img.shape) for f in three]
    for out, status, _ in singles:
        assert status[0] == 0 and np.array_equal(out[0], img)
    again = run([three[0]], img.shape)
    assert all(np.array_equal(x, y) for x, y in zip(again, singles[0]))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = run([three[1]], img.shape)
    side.synchronize()
    assert all(np.array_equal(x, y) for x, y in zip(on_side, singles[1]))
    out, status, segments = run(three, img.shape)
    for i in range(3):
        assert np.array_equal(out[i], singles[i][0][0]) and status[i] == 0 and segments[i] == singles[i][2][0]
    assert segments.tolist() == [1, -(-33 * 211 // 256), 1]
    other = TE.make_image("noise", 33, 70, 3)
    out, status, segments = run([three[1], T.pillow_file(other), three[1]], img.shape)
    assert np.array_equal(out[0], img) and np.array_equal(out[2], img) and np.array_equal(out[1], other)
    assert status.tolist() == [0, 0, 0] and segments[0] == segments[2]


def test_empty_batches_callers_buffers_strictness_and_refusals():
    from soar_amd.png import decode_png
    img = TE.make_image("ramp", 17, 23, 4)
    good, bad = T.pillow_file(img), T.pillow_file(img)[:-20]
    out = decode_png(torch.empty(0, dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 17, 23, 4)
    assert out.shape == (0, 17, 23, 4) and out.dtype == torch.uint8
    data, offsets = upload([good, good])
    mine = torch.full((2, 17, 23, 4), 9, dtype=torch.uint8, device=DEV)
    got = decode_png(data, offsets, 17, 23, 4, out=mine)
    assert got.data_ptr() == mine.data_ptr() and np.array_equal(mine[1].cpu().numpy(), img)
    got, segments = decode_png(data, offsets, 17, 23, 4, return_info=True)
    assert segments.tolist() == [1, 1] and segments.dtype == torch.int32
    data, offsets = upload([good, bad, good, bad])
    with pytest.raises(ValueError, match=r"file 1 of 4: bad signature or chunk structure.*\[1, 3\]"):
        decode_png(data, offsets, 17, 23, 4)
    data, offsets = upload([good])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_png(data.cpu(), offsets, 17, 23, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_png(data, offsets.cpu(), 17, 23, 4)
    for d, o in ((data.to(torch.int8), offsets), (data, offsets.to(torch.int32)), (data[None], offsets), (data, offsets[None])):
        with pytest.raises(ValueError, match="contiguous 1-D"):
            decode_png(d, o, 17, 23, 4)
    with pytest.raises(ValueError, match="C = 1, 3 or 4"):
        decode_png(data, offsets, 17, 23, 2)
    with pytest.raises(ValueError, match="out must be"):
        decode_png(data, offsets, 17, 23, 4, out=mine)
    # offsets that are not ascending, or leave the buffer: no file of the call is looked at
    data, offsets = upload([good, good])
    for wrong in ([0, 2 * len(good), len(good)], [0, len(good), 2 * len(good) + 1], [-1, len(good), 2 * len(good)]):
        o = torch.tensor(wrong, dtype=torch.int64, device=DEV)
        with pytest.raises(ValueError, match="file 0 of 2"):
            decode_png(data, o, 17, 23, 4)
        out, status = decode_png(data, o, 17, 23, 4, strict=False)
        assert status.tolist() == [D.BAD_STRUCTURE] * 2 and not out.any()


def test_two_files_in_a_buffer_of_no_bytes():
    """offsets [0, 0, 0] over empty data: the decoder is called (with a pointer that is never read) and both files are refused"""
    from soar_amd.png import decode_png
    data, offsets = torch.empty(0, dtype=torch.uint8, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    want = D.decode(b"", want=(8, 8, 3), report=False)
    assert want.status == D.BAD_STRUCTURE
    out, status = decode_png(data, offsets, 8, 8, 3, strict=False)
    assert status.tolist() == [want.status] * 2 and out.shape == (2, 8, 8, 3) and np.array_equal(out[1].cpu().numpy(), want.image)
    with pytest.raises(ValueError, match=r"decode_png: file 0 of 2: bad signature or chunk structure.*\[0, 1\]"):
        decode_png(data, offsets, 8, 8, 3)


def test_a_bad_file_behind_a_chunk_boundary_is_named_by_its_path(tmp_path):
    from soar_amd.png import PNG_STATUS, read_png_files
    imgs = [TE.make_image(kind, 17, 13, 3, seed=i) for i, kind in enumerate(("noise", "blob", "ramp"))]
    files = [T.pillow_file(im) for im in imgs]
    paths = [str(tmp_path / f"{i}.png") for i in range(3)]
    for p, f in zip(paths, files):
        open(p, "wb").write(f)
    got = read_png_files(paths, DEV, chunk=2)                       # two calls: two files, then one
    assert np.array_equal(got.cpu().numpy(), np.stack([D.decode(f).image for f in files]))
    cut = files[2][:-20]
    open(paths[2], "wb").write(cut)
    reason = PNG_STATUS[D.decode(cut, want=(17, 13, 3), report=False).status]
    with pytest.raises(ValueError, match=re.escape(f"{paths[2]}: {reason}")):
        read_png_files(paths, DEV, chunk=2)


@pytest.mark.parametrize("c", TE.CHANNELS)
@pytest.mark.parametrize("shape", TE.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_round_trip_through_the_encoder(shape, c):
    from soar_amd.png import decode_png, encode_png
    x = torch.from_numpy(np.stack([TE.make_image(kind, *shape, c) for kind in TE.KINDS])).to(DEV)
    S = shape[0] * (1 + shape[1] * c)
    for f in TE.FILTERS:
        for piece in (32, 256, 65535):
            back, segments = decode_png(*encode_png(x, filters=f, piece_bytes=piece), *shape, c, return_info=True)
            assert torch.equal(back, x), (f, piece)
            assert segments.tolist() == [-(-S // piece)] * len(TE.KINDS), (f, piece, segments.tolist())


def test_read_png_files(tmp_path):
    from soar_amd.png import read_png_files, write_png_files
    imgs = np.stack([TE.make_image(kind, 33, 70, 4, seed=i) for i, kind in enumerate(TE.KINDS)])
    ours, theirs = [str(tmp_path / f"ours{i}.png") for i in range(5)], [str(tmp_path / f"pil{i}.png") for i in range(5)]
    write_png_files(ours, torch.from_numpy(imgs).to(DEV))
    for p, im in zip(theirs, imgs):
        Image.fromarray(im, "RGBA").save(p)
    got = read_png_files(ours + theirs, DEV, chunk=3)
    assert got.shape == (10, 33, 70, 4) and got.dtype == torch.uint8 and got.device == DEV
    assert np.array_equal(got.cpu().numpy(), np.concatenate([imgs, imgs]))
    Image.fromarray(imgs[0][..., :3].copy(), "RGB").save(tmp_path / "rgb.png")
    with pytest.raises(ValueError, match="rgb.png: 33 x 70 with 3 channels"):
        read_png_files(ours + [str(tmp_path / "rgb.png")], DEV)
    cut = tmp_path / "cut.png"
    cut.write_bytes(open(theirs[2], "rb").read()[:-30])
    with pytest.raises(ValueError, match="cut.png: bad signature or chunk structure"):
        read_png_files([theirs[0], str(cut)], DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        read_png_files(ours, "cpu")


# ---- a sequence directory read both ways ----------------------------------------------------------------------------------------------
STORE_TENSORS = ("images", "masks", "normal_F", "normal_B", "normal_mask", "Ks", "normal_Ks", "w2c", "boxes", "rgb_crop", "mask_crop", "Ks_host",
                 "normal_Ks_host", "w2c_host", "c2w_host")


def write_sequence(root, seq, variant, device_writers):
    from soar_amd.png import write_png_files
    N = seq["images"].shape[0]
    for d in ("images", "masks", "normal_F", "normal_B", "smplx"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    masks = seq["masks"] * 200
    images = {"rgb": seq["images"], "mask3": seq["images"], "grey": seq["images"][..., :1],
              "rgba": torch.cat([seq["images"], masks[..., None]], dim=-1)}[variant]
    folders = {"images": images, "normal_F": torch.cat([seq["normal_F"], seq["normal_mask"][..., None]], dim=-1), "normal_B": seq["normal_B"]}
    if variant != "rgba":
        folders["masks"] = masks[..., None].expand(-1, -1, -1, 3).contiguous() if variant == "mask3" else masks
    else:
        os.rmdir(os.path.join(root, "masks"))
    for d, t in folders.items():
        paths = [os.path.join(root, d, f"{i:04d}.png") for i in range(N)]
        if device_writers:
            write_png_files(paths, t.contiguous().to(DEV))
        else:
            for p, im in zip(paths, t.numpy()):
                Image.fromarray(im[..., 0] if im.ndim == 3 and im.shape[2] == 1 else im).save(p)
    w2c_file = seq["w2c"].clone()
    w2c_file[1:3] *= -1
    torch.save(dict(w2c=w2c_file, Ks=seq["Ks"], normal_Ks=seq["normal_Ks"], **seq["smpl_parms"]), os.path.join(root, "smplx", "params.pth"))


@pytest.mark.parametrize("variant,device_writers", [("rgb", False), ("rgb", True), ("rgba", False), ("grey", True), ("mask3", False)])
def test_from_dataroot_with_device_png_builds_the_same_store(tmp_path, variant, device_writers):
    from soar_amd.data import FrameStore
    seq = _seq(N=4, H=48, W=40)
    write_sequence(str(tmp_path), seq, variant, device_writers)
    host = FrameStore.from_dataroot(str(tmp_path), "smplx", device=DEV)
    dev = FrameStore.from_dataroot(str(tmp_path), "smplx", device=DEV, device_png=True)
    assert (host.n_frames, host.height, host.width) == (dev.n_frames, dev.height, dev.width) == (4, 48, 40)
    for k in STORE_TENSORS:
        x, y = getattr(host, k), getattr(dev, k)
        assert x.dtype == y.dtype and x.device == y.device and torch.equal(x, y), k
    for k in host.smpl_parms:
        assert torch.equal(host.smpl_parms[k], dev.smpl_parms[k]) and torch.equal(host.smpl_parms_host[k], dev.smpl_parms_host[k]), k
    assert torch.equal(host.frames_rays_d(), dev.frames_rays_d())
    if variant == "grey":
        assert torch.equal(dev.images[..., 0], dev.images[..., 2])
    if variant == "rgb" and not device_writers:
        # normal_F without alpha: both paths refuse it with the same words
        for i in range(4):
            Image.fromarray(seq["normal_F"][i].numpy(), "RGB").save(tmp_path / "normal_F" / f"{i:04d}.png")
        for flag in (False, True):
            with pytest.raises(ValueError, match=r"normal_F/0000.png: normal_F needs an alpha channel \(the normal mask\)"):
                FrameStore.from_dataroot(str(tmp_path), "smplx", device=DEV, device_png=flag)
