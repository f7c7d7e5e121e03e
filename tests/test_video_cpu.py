"""MJPEG video output without a device: the quantisation tables and the NumPy restatement of the encoder (tests/jpeg_ref.py) against
Pillow (libjpeg-turbo) byte for byte, and the AVI container on JPEG bytes made by Pillow."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import jpeg_ref as J

SIZES = [(1, 1), (2, 2), (8, 8), (17, 23), (16, 17), (24, 8), (30, 5), (33, 70), (48, 80)]          # (H, W)
KINDS = ["noise", "ramp", "blob", "extremes"]


def make_image(kind, h, w, seed=0):
    rs = np.random.RandomState(seed + 1000 * h + w)
    if kind == "noise":
        return rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind == "ramp":
        return (np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[..., None] + np.array([0, 40, 90])).clip(0, 255).astype(np.uint8)
    if kind == "blob":                                            # a soft coloured blob on white
        y, x = np.mgrid[0:h, 0:w]
        a = np.exp(-(((y - 0.4 * h) / (0.3 * h + 1)) ** 2 + ((x - 0.6 * w) / (0.25 * w + 1)) ** 2))[..., None]
        return (255 * (1 - a) + a * np.array([200.0, 40.0, 90.0])).astype(np.uint8)
    if kind == "extremes":
        # all-0 and all-255 8x8 blocks in a checker pattern; every third block split half black, half white; every fifth alternating
        # per pixel
        y, x = np.mgrid[0:h, 0:w]
        by, bx = y // 8, x // 8
        n = by * 7 + bx
        v = ((by + bx) & 1) * 255
        v = np.where(n % 3 == 1, np.where((x & 7) < 4, 0, 255), v)
        v = np.where(n % 5 == 2, ((x + y) & 1) * 255, v)
        return np.repeat(v[..., None], 3, axis=2).astype(np.uint8)
    raise ValueError(kind)


def pillow_jpeg(img, quality, subsampling, restart):
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling={"444": 0, "420": 2}[subsampling], optimize=False,
                              restart_marker_blocks=restart)
    return b.getvalue()


def split_jpeg(d):
    """a baseline JPEG file -> (header up to the end of SOS, scan bytes, {table id: [64] natural order})"""
    assert d[:2] == b"\xff\xd8" and d[-2:] == b"\xff\xd9"
    i, tables = 2, {}
    while True:
        assert d[i] == 0xFF
        m, n = d[i + 1], (d[i + 2] << 8) | d[i + 3]
        if m == 0xDB:
            seg, p = d[i + 4:i + 2 + n], 0
            while p < len(seg):
                t = np.zeros(64, np.int64)
                t[J.ZIGZAG] = list(seg[p + 1:p + 65])
                tables[seg[p] & 15] = t
                p += 65
        if m == 0xDA:
            return d[:i + 2 + n], d[i + 2 + n:-2], tables
        i += 2 + n


@pytest.mark.parametrize("quality", range(1, 101))
def test_jpeg_tables_are_the_tables_pillow_writes(quality):
    from soar_amd.video import jpeg_tables
    _, _, tables = split_jpeg(pillow_jpeg(np.zeros((8, 8, 3), np.uint8), quality, "444", 0))
    ours = jpeg_tables(quality)
    assert ours.dtype == np.uint8 and ours.shape == (2, 64)
    assert np.array_equal(ours[0], tables[0]) and np.array_equal(ours[1], tables[1])


def test_jpeg_tables_refuse_a_quality_outside_1_to_100():
    from soar_amd.video import jpeg_tables
    for q in (0, 101, -5):
        with pytest.raises(ValueError, match="quality"):
            jpeg_tables(q)


@pytest.mark.parametrize("subsampling", ["444", "420"])
@pytest.mark.parametrize("quality", [50, 90, 100])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_scan_bytes_equal_pillows(size, kind, quality, subsampling):
    from soar_amd.video import jpeg_tables
    img = make_image(kind, *size)
    q = jpeg_tables(quality)
    for restart in (1, 3, 7, 1000):                               # 1000: above every MCU count here (48 x 80 at 4:4:4 has 60)
        head, scan, stats = J.encode(img, q, subsampling, restart)
        assert stats["mcus"] < 1000
        p_head, p_scan, _ = split_jpeg(pillow_jpeg(img, quality, subsampling, restart))
        assert scan == p_scan, (restart, len(scan), len(p_scan))
        assert head == p_head, restart                            # (more than asked: the header is Pillow's too)


def test_the_inputs_reach_the_coders_corners():
    """every assert on the restatement's own statistics"""
    from soar_amd.video import jpeg_tables
    noise = make_image("noise", 33, 70)
    s444 = J.encode(noise, jpeg_tables(50), "444", 7)[2]
    s420 = J.encode(noise, jpeg_tables(50), "420", 7)[2]
    assert s444["zrl"] >= 1 and s420["zrl"] >= 1
    assert s420["dummy_blocks"] >= 1                              # 33 rows: the MCUs of the last row have no lower luma blocks
    stuffed = sum(J.encode(make_image("noise", h, w), jpeg_tables(100), "444", 3)[2]["stuffed"] for h, w in SIZES)
    assert stuffed >= 1
    ext = J.encode(make_image("extremes", 48, 80), jpeg_tables(100), "444", 1000)[2]
    assert ext["dc_category"] == 11 and ext["ac_category"] == 10
    assert any(h % 2 == 0 and h % 16 for h, _ in SIZES)           # an even H off the MCU grid: the last DOWNSAMPLED row is replicated
    assert J.encode(make_image("noise", 24, 8), jpeg_tables(90), "420", 1)[2]["restarts"] == 1


@pytest.mark.parametrize("subsampling", ["444", "420"])
def test_pillow_decodes_the_restatements_file_to_the_pixels_of_its_own(subsampling):
    from soar_amd.video import jpeg_tables
    for kind in KINDS:
        img = make_image(kind, 33, 70)
        ours = J.jpeg_file(img, jpeg_tables(90), subsampling, 3)
        theirs = pillow_jpeg(img, 90, subsampling, 3)
        a, b = Image.open(io.BytesIO(ours)), Image.open(io.BytesIO(theirs))
        assert a.size == b.size == (70, 33) and a.mode == b.mode == "RGB"
        assert np.array_equal(np.asarray(a), np.asarray(b)), kind


def test_a_fourth_channel_is_ignored():
    from soar_amd.video import jpeg_tables
    img = make_image("noise", 17, 23)
    rgba = np.concatenate([img, make_image("noise", 17, 23, seed=5)[..., :1]], axis=2)
    assert J.encode(rgba, jpeg_tables(90), "420", 3)[:2] == J.encode(img, jpeg_tables(90), "420", 3)[:2]


# ---- the container ------------------------------------------------------------------------------------------------------------------
def _frames(n=3):
    out = [pillow_jpeg(make_image("noise", 24, 40, seed=i), 70 + i, "420", 0) for i in range(n)]
    if not any(len(f) & 1 for f in out):                          # make sure an odd-length frame is among them
        out[1] = out[1][:-2] + b"\x00\xff\xd9"
    return out


def test_avi_container_sizes_counts_padding_and_index(tmp_path):
    from soar_amd.video import MjpegWriter, read_mjpeg_avi
    frames = _frames()
    assert any(len(f) & 1 for f in frames)
    path = str(tmp_path / "v.avi")
    with MjpegWriter(path, 24, 40, fps=25, quality=90) as w:
        for f in frames:
            w.append_jpeg(f)
    assert w.frames == 3 and w.bytes_to_host == 0
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and struct.unpack_from("<I", d, 4)[0] == len(d) - 8 and d[8:12] == b"AVI "
    assert d[12:16] == b"LIST" and d[20:24] == b"hdrl" and d[24:28] == b"avih" and struct.unpack_from("<I", d, 28)[0] == 56
    hdrl = struct.unpack_from("<I", d, 16)[0]
    usec, _, _, flags, total, _, streams, _, width, height = struct.unpack_from("<10I", d, 32)
    assert (usec, flags & 0x10, total, streams, width, height) == (40000, 0x10, 3, 1, 40, 24)
    strl = d.index(b"strl")
    assert d[strl + 4:strl + 8] == b"strh" and d[strl + 12:strl + 20] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack_from("<4I", d, strl + 12 + 20)
    assert (scale, rate, length) == (1, 25, 3)
    strf = d.index(b"strf")
    size, bw, bh, planes, bits, comp = struct.unpack_from("<IiiHH4s", d, strf + 8)
    assert (size, bw, bh, planes, bits, comp) == (40, 40, 24, 1, 24, b"MJPG")
    movi_list = 12 + 8 + hdrl
    assert d[movi_list:movi_list + 4] == b"LIST" and d[movi_list + 8:movi_list + 12] == b"movi"
    movi_size = struct.unpack_from("<I", d, movi_list + 4)[0]
    # the chunks: one 00dc per frame, padded to even length, filling the list exactly
    p, at = movi_list + 12, []
    for f in frames:
        assert d[p:p + 4] == b"00dc" and struct.unpack_from("<I", d, p + 4)[0] == len(f) and d[p + 8:p + 8 + len(f)] == f
        at.append(p)
        p += 8 + len(f) + (len(f) & 1)
        assert p % 2 == 0
    assert p == movi_list + 8 + movi_size
    assert d[p:p + 4] == b"idx1" and struct.unpack_from("<I", d, p + 4)[0] == 16 * 3 and p + 8 + 48 == len(d)
    for i, f in enumerate(frames):
        cc, fl, off, n = struct.unpack_from("<4sIII", d, p + 8 + 16 * i)
        assert cc == b"00dc" and fl & 0x10 and n == len(f) and movi_list + 8 + off == at[i]
    assert read_mjpeg_avi(path) == frames


def test_avi_fractional_frame_rate_and_empty_file(tmp_path):
    from soar_amd.video import MjpegWriter, read_mjpeg_avi
    path = str(tmp_path / "e.avi")
    MjpegWriter(path, 8, 8, fps=29.97).close()
    d = open(path, "rb").read()
    assert struct.unpack_from("<I", d, 4)[0] == len(d) - 8 and read_mjpeg_avi(path) == []
    strl = d.index(b"strl")
    assert struct.unpack_from("<2I", d, strl + 32) == (1000, 29970)


def test_avi_refuses_the_frame_that_would_cross_4_gb(tmp_path):
    """by arithmetic on a faked size: the writer's count of bytes so far is moved close to the limit, no large file is written"""
    from soar_amd.video import AVI_MAX_BYTES, MjpegWriter, read_mjpeg_avi
    frames = _frames(2)
    path = str(tmp_path / "big.avi")
    w = MjpegWriter(path, 24, 40)
    w.append_jpeg(frames[0])
    true_pos = w._pos
    n = len(frames[1])
    need = 8 + n + (n & 1) + 8 + 16 * 2                           # the chunk, and the index of two frames behind it
    w._pos = AVI_MAX_BYTES - need + 1                             # one byte too many
    with pytest.raises(ValueError, match="OpenDML"):
        w.append_jpeg(frames[1])
    assert w.frames == 1
    w._pos = true_pos
    w.close()                                                     # the refused frame left nothing behind
    assert read_mjpeg_avi(path) == frames[:1]
    w = MjpegWriter(str(tmp_path / "edge.avi"), 24, 40)
    w.append_jpeg(frames[0])
    w._pos = AVI_MAX_BYTES - need                                 # ends at exactly 2^32 - 1 bytes: allowed
    w.append_jpeg(frames[1])
    assert w.frames == 2
    w._file.close()


def test_video_refuses_cpu_tensors():
    import torch
    from soar_amd.video import encode_jpeg, save_jpeg
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encode_jpeg(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        save_jpeg("unused.jpg", torch.zeros((8, 8, 3), dtype=torch.uint8))


def test_jpeg_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    from soar_amd import build, hip_lib
    build.build()
    lib = hip_lib.lib()
    a = hip_lib.SoarJpegArgs()
    a.B, a.H, a.W, a.channels, a.subsampling, a.restart_interval = 1, 16, 16, 3, 420, 4
    n = C.c_size_t(0)
    assert lib.soar_jpeg_workspace_bytes(C.byref(a), C.byref(n)) != 0 and "quantisation" in hip_lib.last_error()     # tables of zeros
    C.memset(a.qtables, 1, 128)
    assert lib.soar_jpeg_workspace_bytes(C.byref(a), C.byref(n)) == 0
    assert n.value % 256 == 0 and n.value >= 6 * 128                      # one MCU of six blocks of int16 coefficients
    for field, bad in (("H", 0), ("W", 65536), ("channels", 2), ("subsampling", 422), ("restart_interval", 0), ("restart_interval", 65536),
                       ("B", -1)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.soar_jpeg_workspace_bytes(C.byref(a), C.byref(n)) != 0 and "bad arguments" in hip_lib.last_error(), field
        assert lib.soar_jpeg_measure(C.byref(a), 0x1000, 1 << 20, 0x1000, None) != 0, field
        assert lib.soar_jpeg_emit(C.byref(a), 0x1000, 1 << 20, 0x1000, 100, None) != 0, field
        setattr(a, field, keep)
    assert lib.soar_jpeg_measure(C.byref(a), None, 0, 0x1000, None) != 0 and "workspace" in hip_lib.last_error()
    assert lib.soar_jpeg_measure(C.byref(a), 0x1000, 1 << 20, None, None) != 0 and "offsets" in hip_lib.last_error()
    assert lib.soar_jpeg_measure(C.byref(a), 0x1000, 1 << 20, 0x1000, None) != 0 and "frames" in hip_lib.last_error()
    assert lib.soar_jpeg_emit(C.byref(a), 0x1000, 16, 0x1000, 100, None) != 0 and "workspace" in hip_lib.last_error()
    assert lib.soar_jpeg_emit(C.byref(a), 0x1000, 1 << 20, None, 100, None) != 0 and "capacity" in hip_lib.last_error()
