"""JPEG input on the device: soar_amd.jpeg.decode_jpeg against the restatement (tests/jpeg_decode_ref.py, itself bit-equal to Pillow on
the CPU) on every file of tests/test_jpeg_decode_cpu.py -- pixels, status and intervals; malformed files between good ones, with guard
bytes around the output and the workspace; batches, streams and positions; the round trip through encode_jpeg; resize_images against
Pillow; MjpegReader, read_video and read_jpeg_files; and extract_frames from an AVI and from a directory, read back with Pillow and
opened by FrameStore.from_dataroot(device_png=True)."""
import io
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_decode_ref as D
import test_jpeg_decode_cpu as T

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GUARD, MARGIN = 0xAB, 4096


def upload(files):
    off = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    data = torch.frombuffer(bytearray(b"".join(files)) or bytearray(1), dtype=torch.uint8)[:int(off[-1])].to(DEV)
    return data, torch.from_numpy(off).to(DEV)


def run(files, shape, **kw):
    """-> (images, status, intervals) as NumPy"""
    from soar_amd.jpeg import decode_jpeg
    data, offsets = upload(files)
    out, status, intervals = decode_jpeg(data, offsets, *shape, strict=False, return_info=True, **kw)
    return out.cpu().numpy(), status.cpu().numpy(), intervals.cpu().numpy()


def pillow(data):
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a[..., None] if a.ndim == 2 else a


def by_shape():
    groups = {}
    for name, data, shape, restarts in T.corpus_files():
        groups.setdefault(shape, []).append((name, data, restarts))
    return sorted(groups.items())


@pytest.mark.parametrize("shape,files", by_shape(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_decode_jpeg_equals_the_restatement_on_the_corpus(shape, files):
    out, status, intervals = run([d for _, d, _ in files], shape)
    for i, (name, data, restarts) in enumerate(files):
        want = T.decoded(name, data, shape)
        assert status[i] == want.status == 0, (name, status[i])
        assert intervals[i] == want.intervals and (intervals[i] > 1) == restarts, (name, intervals[i], want.intervals)
        assert np.array_equal(out[i], want.image), (name, int(np.abs(out[i].astype(int) - want.image).max()))
        assert np.array_equal(out[i], pillow(data)), name


def guarded_call(files, shape):
    """the C ABI itself, with out and the workspace inside larger buffers filled with a pattern -> (images, status) and the guards"""
    import ctypes as C
    from soar_amd import hip_lib
    h, w, c = shape
    data, offsets = upload(files)
    B, n = len(files), h * w * c
    a = hip_lib.SoarJpegDecodeArgs()
    a.B, a.H, a.W, a.channels, a.total_bytes = B, h, w, c, data.numel()
    a.data, a.offsets = data.data_ptr(), offsets.data_ptr()
    lib = hip_lib.lib()
    need = C.c_size_t(0)
    assert lib.soar_jpeg_decode_workspace_bytes(C.byref(a), C.byref(need)) == 0
    ws = torch.full((need.value + 2 * MARGIN,), GUARD, dtype=torch.uint8, device=DEV)
    out = torch.full((B * n + 2 * MARGIN,), GUARD, dtype=torch.uint8, device=DEV)
    status = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    intervals = torch.full((B + 2,), -7, dtype=torch.int32, device=DEV)
    assert ws.data_ptr() % 256 == 0 and MARGIN % 256 == 0
    rc = lib.soar_jpeg_decode(C.byref(a), ws.data_ptr() + MARGIN, need.value, out.data_ptr() + MARGIN, status.data_ptr() + 4,
                              intervals.data_ptr() + 4, torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0, hip_lib.last_error()
    torch.cuda.synchronize()
    guards = [ws[:MARGIN], ws[MARGIN + need.value:], out[:MARGIN], out[MARGIN + B * n:]]
    assert all(bool((g == GUARD).all()) for g in guards)
    assert status[0] == -7 and status[-1] == -7 and intervals[0] == -7 and intervals[-1] == -7
    return out[MARGIN:MARGIN + B * n].reshape(B, h, w, c).cpu().numpy(), status[1:-1].cpu().numpy()


def test_malformed_files_between_good_ones():
    shape = (17, 33, 3)
    bad = [(n, d, st) for n, d, s, st in T.malformed() if s == shape]
    good = [(n, d) for n, d, s, _ in T.corpus_files() if s == shape][:len(bad) + 1]
    assert len(bad) >= 18 and len(good) == len(bad) + 1
    files, kinds = [], []
    for i, g in enumerate(good):
        files.append(g[1])
        kinds.append(("good", g[0]))
        if i < len(bad):
            files.append(bad[i][1])
            kinds.append(("bad", bad[i][0]))
    out, status = guarded_call(files, shape)
    for i, (kind, name) in enumerate(kinds):
        want = T.decoded(name, files[i], shape)
        assert status[i] == want.status, (name, status[i], want.status)
        if kind == "good":
            solo, st, _ = run([files[i]], shape)
            assert status[i] == 0 and st[0] == 0 and np.array_equal(out[i], solo[0]) and np.array_equal(out[i], want.image), name
        else:
            assert status[i] != 0 and not out[i].any(), name
    # the small grey ones
    grey = [(n, d) for n, d, s, _ in T.malformed() if s == (8, 8, 1)]
    ok = T.pillow_file(8, 8, "grey")
    out, status = guarded_call([ok] + [d for _, d in grey] + [ok], (8, 8, 1))
    assert status[0] == 0 and status[-1] == 0 and np.array_equal(out[0], out[-1]) and np.array_equal(out[0], pillow(ok))
    for i, (name, data) in enumerate(grey):
        assert status[1 + i] == T.decoded(name, data, (8, 8, 1)).status == D.CORRUPT and not out[1 + i].any(), name


def test_corrupted_and_cut_files_get_the_restatements_status():
    """the seeded corruptions and a stride of the prefixes the host program runs under the sanitizers: status and, where the file
    still decodes, pixels"""
    for shape in ((17, 33, 3), (17, 33, 1), (7, 9, 3), (16, 16, 3)):
        files = [(n, d) for n, d, s, _ in T.corruptions(40) + T.prefixes()[::9] if s == shape]
        assert files
        out, status = guarded_call([d for _, d in files], shape)
        for i, (name, data) in enumerate(files):
            want = T.decoded(name, data, shape)
            assert status[i] == want.status, (name, status[i], want.status)
            assert np.array_equal(out[i], want.image), name


def test_calls_streams_positions_and_arguments():
    from soar_amd.jpeg import decode_jpeg
    shape = (17, 33, 3)
    files = [d for n, d, s, _ in T.corpus_files() if s == shape][:9]
    first, st, iv = run(files, shape)
    again, st2, iv2 = run(files, shape)
    assert not st.any() and np.array_equal(first, again) and np.array_equal(iv, iv2)
    stream = torch.cuda.Stream(DEV)
    with torch.cuda.stream(stream):
        other, _, _ = run(files, shape)
    stream.synchronize()
    assert np.array_equal(first, other)
    back, _, ivb = run(files[::-1], shape)
    assert np.array_equal(first, back[::-1]) and np.array_equal(iv, ivb[::-1])
    data, offsets = upload(files)
    mine = torch.full((len(files),) + shape, 7, dtype=torch.uint8, device=DEV)
    got = decode_jpeg(data, offsets, *shape, out=mine)
    assert got is mine and np.array_equal(mine.cpu().numpy(), first)
    images, status = decode_jpeg(data, offsets, *shape, strict=False)
    assert status.is_cuda and status.dtype == torch.int32 and np.array_equal(images.cpu().numpy(), first)
    cut, off2 = upload([files[0], files[1][:-10]])
    with pytest.raises(ValueError, match="file 1 of 2: truncated"):
        decode_jpeg(cut, off2, *shape)
    with pytest.raises(ValueError, match="B >= 1"):
        decode_jpeg(data, offsets[:1], *shape)
    with pytest.raises(ValueError, match="C = 1 or 3"):
        decode_jpeg(data, offsets, 17, 33, 4)
    with pytest.raises(ValueError, match="out must be"):
        decode_jpeg(data, offsets, *shape, out=mine[:2])
    with pytest.raises(ValueError, match="contiguous 1-D"):
        decode_jpeg(data, offsets.to(torch.int32), *shape)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_jpeg(data.cpu(), offsets, *shape)
    # offsets that are not ascending inside the buffer: no file of the call is looked at
    wrong = offsets.clone()
    wrong[3] = data.numel() + 5
    out, status = decode_jpeg(data, wrong, *shape, strict=False)
    assert bool((status == D.BAD_STRUCTURE).all()) and not bool(out.any())


def test_two_files_in_a_buffer_of_no_bytes():
    """offsets [0, 0, 0] over empty data: the decoder is called (with a pointer that is never read) and both files are refused"""
    from soar_amd.jpeg import decode_jpeg
    data, offsets = torch.empty(0, dtype=torch.uint8, device=DEV), torch.zeros(3, dtype=torch.int64, device=DEV)
    want = D.decode(b"", 8, 8, 3)
    assert want.status == D.BAD_STRUCTURE
    out, status = decode_jpeg(data, offsets, 8, 8, 3, strict=False)
    assert status.tolist() == [want.status] * 2 and out.shape == (2, 8, 8, 3) and np.array_equal(out[1].cpu().numpy(), want.image)
    with pytest.raises(ValueError, match=r"decode_jpeg: file 0 of 2: bad structure.*\[0, 1\]"):
        decode_jpeg(data, offsets, 8, 8, 3)


def test_a_bad_file_behind_a_chunk_boundary_is_named_by_its_path(tmp_path):
    from soar_amd.jpeg import JPEG_STATUS, read_jpeg_files
    files = [T.pillow_file(17, 13, "420", quality=q) for q in (50, 75, 90)]
    paths = [str(tmp_path / f"{i}.jpg") for i in range(3)]
    for p, f in zip(paths, files):
        open(p, "wb").write(f)
    got = read_jpeg_files(paths, DEV, chunk=2)                      # two calls: two files, then one
    assert np.array_equal(got.cpu().numpy(), np.stack([D.decode(f, 17, 13, 3).image for f in files]))
    cut = files[2][:-10]
    open(paths[2], "wb").write(cut)
    reason = JPEG_STATUS[D.decode(cut, 17, 13, 3).status]
    with pytest.raises(ValueError, match=re.escape(f"{paths[2]}: {reason}")):
        read_jpeg_files(paths, DEV, chunk=2)


@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("restart_interval", [None, 5])
def test_round_trip_through_the_projects_encoder(subsampling, restart_interval):
    from soar_amd.jpeg import decode_jpeg
    from soar_amd.video import encode_jpeg
    frames = torch.from_numpy(np.stack([T.picture("noise", 50, 70, 3, seed=i) for i in range(3)])).to(DEV)
    data, offsets = encode_jpeg(frames, quality=85, subsampling=subsampling, restart_interval=restart_interval)
    out, intervals = decode_jpeg(data, offsets, 50, 70, 3, return_info=True)
    host, off = data.cpu().numpy().tobytes(), offsets.tolist()
    mcus = (7 * 9) if subsampling == "444" else (4 * 5)
    per = restart_interval or {"444": 8, "420": 4}[subsampling]
    for b in range(3):
        assert np.array_equal(out[b].cpu().numpy(), pillow(host[off[b]:off[b + 1]])), b
        assert int(intervals[b]) == -(-mcus // per)


RESIZES = [((37, 53), (16, 23)), ((16, 23), (37, 53)), ((64, 48), (64, 48)), ((1080, 8), (540, 8)), ((9, 5), (4, 11))]


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("src,dst", RESIZES)
def test_resize_images_equals_pillow(src, dst, channels):
    from soar_amd.jpeg import resize_images
    a = np.random.default_rng(src[0] + channels).integers(0, 256, (2,) + src + (channels,), dtype=np.uint8)
    got = resize_images(torch.from_numpy(a).to(DEV), dst[0], dst[1]).cpu().numpy()
    assert got.shape == (2,) + dst + (channels,)
    for b in range(2):
        im = Image.fromarray(a[b, ..., 0] if channels == 1 else a[b])
        assert np.array_equal(got[b].reshape(dst + (channels,)), np.asarray(im.resize((dst[1], dst[0]), Image.BICUBIC)).reshape(dst + (channels,)))
    if src == (37, 53):
        assert resize_images(torch.from_numpy(a).to(DEV), 16).shape == (2, 16, 23, channels)      # round(53 * 16 / 37)
        with pytest.raises(ValueError):
            resize_images(torch.from_numpy(a).to(DEV).float(), 16)


def movie(n=10, H=48, W=64):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([np.stack([(x * 4 + 9 * i) % 256, (y * 5 + 3 * i) % 256, ((x + y) * 2 + 17 * i) % 256], axis=-1) for i in range(n)]).astype(np.uint8)


def write_movie(path, fps=5, **options):
    from soar_amd.video import MjpegWriter
    frames = torch.from_numpy(movie()).to(DEV)
    with MjpegWriter(str(path), 48, 64, fps=fps, **options) as w:
        w.write(frames[:4])
        w.append_jpeg(b"")                                        # a dropped frame: a chunk of length zero
        w.write(frames[4:])


def test_mjpeg_reader_read_video_and_read_jpeg_files(tmp_path):
    from soar_amd.jpeg import read_jpeg_files
    from soar_amd.video import MjpegReader, read_mjpeg_avi, read_video
    path = tmp_path / "clip.avi"
    write_movie(path)
    chunks = [c for c in read_mjpeg_avi(str(path)) if c]
    assert len(chunks) == 10
    want = np.stack([pillow(c) for c in chunks])
    r = MjpegReader(str(path))
    assert (r.height, r.width, r.fps, r.frames, r.channels) == (48, 64, 5.0, 10, 3)
    whole = read_video(str(path), DEV)
    assert whole.shape == (10, 48, 64, 3) and whole.device == DEV and np.array_equal(whole.cpu().numpy(), want)
    parts = list(r.read(1, 9, 3, DEV, chunk=2))
    assert [p.shape[0] for p in parts] == [2, 1] and np.array_equal(torch.cat(parts).cpu().numpy(), want[1:9:3])
    assert list(r.read(10, None, 1, DEV)) == []
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(r.read(device="cpu"))
    # the same frames without their Huffman tables, as an MJPG chunk may come
    bare = tmp_path / "bare.avi"
    from soar_amd.video import MjpegWriter
    with MjpegWriter(str(bare), 48, 64, fps=29.97) as w:
        for c in chunks:
            w.append_jpeg(T.without(c, 0xC4))
    assert abs(MjpegReader(str(bare)).fps - 29.97) < 1e-9
    assert np.array_equal(read_video(str(bare), DEV).cpu().numpy(), want)
    names = []
    for i, c in enumerate(chunks[:5]):
        names.append(str(tmp_path / f"f{i}.jpg"))
        open(names[-1], "wb").write(c)
    got = read_jpeg_files(names, DEV, chunk=2)
    assert got.shape == (5, 48, 64, 3) and np.array_equal(got.cpu().numpy(), want[:5])
    open(tmp_path / "cut.jpg", "wb").write(chunks[0][:-30])
    with pytest.raises(ValueError, match="cut.jpg: truncated"):
        read_jpeg_files(names + [str(tmp_path / "cut.jpg")], DEV)
    open(tmp_path / "small.jpg", "wb").write(T.pillow_file(16, 16, "420"))
    with pytest.raises(ValueError, match="small.jpg: 16 x 16 with 3 components"):
        read_jpeg_files(names + [str(tmp_path / "small.jpg")], DEV)


def test_extract_frames(tmp_path):
    from soar_amd.data import FrameStore
    from soar_amd.frames import extract_frames, frame_indices
    from soar_amd.video import read_mjpeg_avi
    from test_data_cpu import _seq
    from test_png_decode_gpu import write_sequence
    path = tmp_path / "clip.avi"
    write_movie(path)                                             # 10 frames at 5 per second: frame n at n / 5 s
    frames = [Image.open(io.BytesIO(c)).convert("RGB") for c in read_mjpeg_avi(str(path)) if c]
    root = tmp_path / "data"
    assert extract_frames(str(path), str(root)) == 10
    folder = root / "clip" / "images"
    assert sorted(os.listdir(folder)) == [f"{i:05d}.png" for i in range(10)]
    for i in range(10):
        assert np.array_equal(np.asarray(Image.open(folder / f"{i:05d}.png")), np.asarray(frames[i])), i
    assert os.path.islink(root / "clip" / "video.avi") and os.path.samefile(root / "clip" / "video.avi", path)
    stamp = {f: os.stat(folder / f).st_mtime_ns for f in os.listdir(folder)}
    assert extract_frames(str(path), str(root), height=24, skip_time=3) == 0                       # frames already extracted
    assert {f: os.stat(folder / f).st_mtime_ns for f in os.listdir(folder)} == stamp
    # every third frame of those between 0.4 s and 1.7 s: frames 3 and 6 (0 lies before, 9 behind)
    assert frame_indices(10, 5.0, 3, "00:00:00.4", "00:00:01.7") == [3, 6]
    root2 = tmp_path / "data2"
    assert extract_frames(str(path), str(root2), height=24, skip_time=3, start_time="00:00:00.4", end_time="00:00:01.7", chunk=1) == 2
    assert sorted(os.listdir(root2 / "clip" / "images")) == ["00000.png", "00001.png"]
    for k, n in enumerate((3, 6)):
        want = np.asarray(frames[n].resize((32, 24), Image.BICUBIC))
        assert np.array_equal(np.asarray(Image.open(root2 / "clip" / "images" / f"{k:05d}.png")), want), n
    # a directory of .jpg files gives the same images
    shots = tmp_path / "shots"
    shots.mkdir()
    for i, c in enumerate(c for c in read_mjpeg_avi(str(path)) if c):
        open(shots / f"{i:03d}.jpg", "wb").write(c)
    root3 = tmp_path / "data3"
    assert extract_frames(str(shots), str(root3), chunk=4) == 10
    for i in range(10):
        assert open(root3 / "shots" / "images" / f"{i:05d}.png", "rb").read() == open(folder / f"{i:05d}.png", "rb").read()
    with pytest.raises(ValueError, match="has no times"):
        extract_frames(str(shots), str(tmp_path / "data4"), skip_time=2)
    # the rest of a sequence directory around the extracted frames: the data module opens it
    seq = _seq(N=10, H=48, W=64)
    other = tmp_path / "rest"
    write_sequence(str(other), seq, "rgb", True)
    for d in ("masks", "normal_F", "normal_B", "smplx"):
        os.rename(other / d, root / "clip" / d)
    store = FrameStore.from_dataroot(str(root / "clip"), "smplx", device=DEV, device_png=True)
    assert (store.n_frames, store.height, store.width) == (10, 48, 64)
    host = FrameStore.from_dataroot(str(root / "clip"), "smplx", device=DEV)
    assert torch.equal(store.images, host.images)


# ---- guards: what was there before stays as it was --------------------------------------------------------------------------------------
def test_the_encoders_bytes_are_unchanged():
    import jpeg_ref as E
    from soar_amd.video import encode_jpeg, jpeg_tables
    frame = T.picture("noise", 40, 56, 3)
    for sub, ri in (("444", 8), ("420", 4)):
        data, offsets = encode_jpeg(torch.from_numpy(frame[None]).to(DEV), quality=90, subsampling=sub)
        assert data.cpu().numpy().tobytes() == E.jpeg_file(frame, jpeg_tables(90), sub, ri)


def test_read_mjpeg_avi_returns_the_same_chunks(tmp_path):
    from soar_amd.video import encode_jpeg, read_mjpeg_avi
    path = tmp_path / "clip.avi"
    write_movie(path)
    data, offsets = encode_jpeg(torch.from_numpy(movie()).to(DEV), quality=90, subsampling="420")
    host, off = data.cpu().numpy().tobytes(), offsets.tolist()
    want = [host[off[b]:off[b + 1]] for b in range(10)]
    assert read_mjpeg_avi(str(path)) == want[:4] + [b""] + want[4:]
