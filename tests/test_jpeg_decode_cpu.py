"""CPU tests of the JPEG reader: the NumPy restatement (tests/jpeg_decode_ref.py) against Pillow on the whole corpus,
the resize restatement against ``Image.resize(BICUBIC)``, the restatement's status for every malformed file, and the decoder's shared
header (csrc/jpeg_entropy.h) built for the host under the address and undefined-behaviour sanitizers and run over all of them.

The corpus is built here from seeded noise and smooth gradients; tests/test_jpeg_decode_gpu.py holds the device to the same files.
"""
import io
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import jpeg_decode_ref as D  # noqa: E402
import jpeg_ref as E  # noqa: E402
from soar_amd.video import jpeg_tables  # noqa: E402

SAMPLINGS = {"grey": None, "444": 0, "422": 1, "420": 2}
SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (3, 5), (4, 4)]       # (H, W); the last two: a downsampled width of 2 or less


def picture(kind, H, W, C, seed=0):
    if kind == "noise":
        a = np.random.default_rng(1000 * H + W + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    else:
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(x * 255) // max(W - 1, 1), (y * 255) // max(H - 1, 1), ((x + y) * 255) // max(H + W - 2, 1)], axis=-1).astype(np.uint8)
    return a if C == 3 else a[..., 1]


def pillow_file(H, W, sampling, kind="noise", quality=90, **options):
    a = picture(kind, H, W, 1 if sampling == "grey" else 3)
    buf = io.BytesIO()
    if sampling != "grey":
        options["subsampling"] = SAMPLINGS[sampling]
    Image.fromarray(a).save(buf, "JPEG", quality=quality, **options)
    return buf.getvalue()


def segments_of(f):
    """[(marker, first byte, end)] of the segments from SOI to the end of SOS"""
    out, p = [], 2
    while True:
        m, n = f[p + 1], f[p + 2] << 8 | f[p + 3]
        out.append((m, p, p + 2 + n))
        p += 2 + n
        if m == 0xDA:
            return out


def without(f, marker):
    return f[:2] + b"".join(f[a:b] for m, a, b in segments_of(f) if m != marker) + f[segments_of(f)[-1][2]:]


def split_tables(f):
    """every DQT and DHT cut into one segment per table"""
    out = f[:2]
    for m, a, b in segments_of(f):
        if m == 0xDB:
            for p in range(a + 4, b, 65):
                out += E._segment(0xDB, f[p:p + 65])
        elif m == 0xC4:
            p = a + 4
            while p < b:
                n = 17 + sum(f[p + 1:p + 17])
                out += E._segment(0xC4, f[p:p + n])
                p += n
        else:
            out += f[a:b]
    return out + f[segments_of(f)[-1][2]:]


_CORPUS = []


def corpus_files():
    """[(name, bytes, (H, W, C), restart markers expected)]"""
    if _CORPUS:
        return _CORPUS
    out = []

    def add(name, data, H, W, sampling, restarts):
        out.append((name, data, (H, W, 1 if sampling == "grey" else 3), restarts))

    for H, W in SIZES + [(40, 40)]:
        for s in SAMPLINGS:
            for kind in ("noise", "smooth"):
                add(f"p_{H}x{W}_{s}_{kind}", pillow_file(H, W, s, kind), H, W, s, False)
    for H, W in ((17, 33), (40, 40)):
        for s in SAMPLINGS:
            for q in (1, 50, 100):
                for opt in (False, True):
                    add(f"p_{H}x{W}_{s}_q{q}_opt{int(opt)}", pillow_file(H, W, s, quality=q, optimize=opt), H, W, s, False)
    for H, W in ((7, 9), (17, 33), (40, 40)):
        for s in SAMPLINGS:
            for key, val in (("restart_marker_blocks", 1), ("restart_marker_blocks", 3), ("restart_marker_rows", 1)):
                data = pillow_file(H, W, s, **{key: val})
                add(f"p_{H}x{W}_{s}_{key[15:]}{val}", data, H, W, s, b"\xff\xd0" in data)
    for s in SAMPLINGS:                                            # several MCU rows: intervals that cross row ends
        for opts in ({}, {"restart_marker_blocks": 3}, {"restart_marker_rows": 1}):
            data = pillow_file(48, 64, s, quality=100, optimize=True, **opts)
            add(f"p_48x64_{s}_" + "_".join(f"{k[15:]}{v}" for k, v in opts.items()), data, 48, 64, s, bool(opts))
    for H, W in ((17, 33), (40, 40), (48, 64)):                    # the project's own encoder
        for s in ("444", "420"):
            for ri in (1, 3, 8):
                mcus = -(-H // (8 if s == "444" else 16)) * -(-W // (8 if s == "444" else 16))
                add(f"e_{H}x{W}_{s}_ri{ri}", E.jpeg_file(picture("noise", H, W, 3), jpeg_tables(90), s, ri), H, W, s, mcus > ri)
    base = pillow_file(17, 33, "420")
    add("x_com_app1", base[:2] + E._segment(0xFE, b"a comment \xff\xd9 in it") + E._segment(0xE1, b"Exif\x00\x00" + bytes(40)) + base[2:], 17, 33, "420", False)
    add("x_after_eoi", base + b"\x00\xff\xd8\xff\xda\x00", 17, 33, "420", False)
    add("x_no_dht", without(base, 0xC4), 17, 33, "420", False)
    add("x_no_dht_grey", without(pillow_file(17, 33, "grey"), 0xC4), 17, 33, "grey", False)
    add("x_split_tables", split_tables(base), 17, 33, "420", False)
    add("x_fill_bytes", base[:2] + b"\xff\xff\xff" + base[2:], 17, 33, "420", False)
    _CORPUS.extend(out)
    return _CORPUS


def _bits_to_scan(bits):
    bits += "1" * (-len(bits) % 8)
    raw = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    return raw.replace(b"\xff", b"\xff\x00")


def _code(spec, symbol):
    code, length = E._codes(spec)[symbol]
    return format(code, f"0{length}b")


_MALFORMED = []


def malformed():
    """[(name, bytes, (H, W, C) of the call, the status it must get)]"""
    if _MALFORMED:
        return _MALFORMED
    out = []
    plain = pillow_file(17, 33, "420")
    seg = segments_of(plain)
    scan = seg[-1][2]
    dht = [a for m, a, b in seg if m == 0xC4][0]
    shape = (17, 33, 3)
    out.append(("t_header", plain[:10], shape, D.BAD_STRUCTURE))
    out.append(("t_table", plain[:dht + 30], shape, D.BAD_STRUCTURE))
    for k, cut in enumerate((scan, scan + 1, scan + (len(plain) - scan) // 2, len(plain) - 3)):
        out.append((f"t_scan{k}", plain[:cut], shape, D.TRUNCATED))
    rst = pillow_file(17, 33, "420", restart_marker_blocks=1)
    rscan = segments_of(rst)[-1][2]
    out.append(("t_rst_scan", rst[:rscan + (len(rst) - rscan) // 2], shape, D.TRUNCATED))
    out.append(("u_progressive", pillow_file(17, 33, "420", progressive=True), shape, D.UNSUPPORTED))
    f422 = bytearray(pillow_file(17, 33, "422"))
    sof = [a for m, a, b in segments_of(bytes(f422)) if m == 0xC0][0]
    f422[sof + 11] = 0x12                                          # luma 1 x 2: 4:4:0
    out.append(("u_440", bytes(f422), shape, D.UNSUPPORTED))
    buf = io.BytesIO()
    Image.fromarray(picture("noise", 17, 33, 3)).convert("CMYK").save(buf, "JPEG")
    out.append(("u_cmyk", buf.getvalue(), shape, D.UNSUPPORTED))
    out.append(("u_size", pillow_file(16, 16, "420"), shape, D.UNSUPPORTED))
    out.append(("u_grey", pillow_file(17, 33, "grey"), shape, D.UNSUPPORTED))
    m = bytearray(plain)
    m[seg[-1][1] + 4 + 2] = 0x22                                   # the first component's DC and AC tables: 2, never defined
    out.append(("m_huffman", bytes(m), shape, D.MISSING_TABLE))
    m = bytearray(plain)
    m[sof + 12] = 3                                                # the first component's quantiser
    out.append(("m_quant", bytes(m), shape, D.MISSING_TABLE))
    r = bytearray(rst)
    at = r.index(b"\xff\xd1", rscan)
    r[at + 1] = 0xD3
    out.append(("c_rst_sequence", bytes(r), shape, D.CORRUPT))
    r = bytearray(rst)
    del r[at:at + 2]
    out.append(("c_rst_missing", bytes(r), shape, D.CORRUPT))
    # an invalid code: sixteen 1 bits begin no code of Annex K's tables
    grey = pillow_file(8, 8, "grey")
    head = grey[:segments_of(grey)[-1][2]]
    out.append(("c_invalid_code", head + b"\xff\x00\xff\x00\xff\x00" + b"\xff\xd9", (8, 8, 1), D.CORRUPT))
    for at in range(scan, len(plain) - 2):                         # the first byte of the scan whose flip begins no code later on
        flipped = bytearray(plain)
        flipped[at] ^= 0xFF
        if D.decode(bytes(flipped), *shape).status == D.CORRUPT:
            break
    out.append(("c_flipped", bytes(flipped), shape, D.CORRUPT))
    zrl, dc0 = _code(E.AC_LUM, 0xF0), _code(E.DC_LUM, 0)
    out.append(("c_run_zrl", head + _bits_to_scan(dc0 + zrl * 4) + b"\xff\xd9", (8, 8, 1), D.CORRUPT))
    out.append(("c_run_63", head + _bits_to_scan(dc0 + zrl * 3 + _code(E.AC_LUM, 0xF1) + "1") + b"\xff\xd9", (8, 8, 1), D.CORRUPT))
    out.append(("s_no_soi", plain[2:], shape, D.BAD_STRUCTURE))
    out.append(("s_empty", b"", shape, D.BAD_STRUCTURE))
    out.append(("s_sos_first", plain[:2] + plain[seg[-1][1]:], shape, D.BAD_STRUCTURE))
    z = bytearray(plain)
    z[sof + 5:sof + 7] = b"\x00\x00"
    out.append(("s_zero_height", bytes(z), shape, D.BAD_STRUCTURE))
    _MALFORMED.extend(out)
    return _MALFORMED


def prefixes():
    """every prefix of two small files"""
    out = []
    for name, data, shape in (("pre_a", pillow_file(7, 9, "420"), (7, 9, 3)),
                              ("pre_b", pillow_file(16, 16, "444", restart_marker_blocks=1, optimize=True), (16, 16, 3))):
        out += [(f"{name}_{n:04d}", data[:n], shape, None) for n in range(len(data))]
    return out


def corruptions(per_file=120):
    """seeded single-byte corruptions of one file of each sampling"""
    out = []
    for i, s in enumerate(SAMPLINGS):
        rng = np.random.default_rng(7 + i)                         # (per sampling: a shorter list is the beginning of a longer one)
        data = pillow_file(17, 33, s, restart_marker_blocks=3 if s in ("444", "420") else 0)
        for k in range(per_file):
            d = bytearray(data)
            at = int(rng.integers(2, len(d)))
            d[at] = int(rng.integers(0, 256))
            out.append((f"cor_{s}_{k:03d}", bytes(d), (17, 33, 1 if s == "grey" else 3), None))
    return out


_DECODED = {}


def decoded(name, data, shape):
    key = (name, shape)
    if key not in _DECODED:
        _DECODED[key] = D.decode(data, *shape) if shape is not None else D.decode(data)
    return _DECODED[key]


# ---- the restatement against Pillow -------------------------------------------------------------------------------------------------------
def test_the_restatement_equals_pillow_on_the_whole_corpus():
    files = corpus_files()
    assert len(files) > 150
    names = [n for n, *_ in files]
    assert len(set(names)) == len(names)
    for name, data, shape, restarts in files:
        want = np.asarray(Image.open(io.BytesIO(data)))
        want = want.reshape(shape)
        r = decoded(name, data, shape)
        assert r.status == D.OK, (name, r.status)
        assert r.image.shape == want.shape and np.array_equal(r.image, want), (name, int(np.abs(r.image.astype(int) - want).max()))
        assert (r.intervals > 1) == restarts, (name, r.intervals)
    # the corners the corpus is there for
    by = {n: d for n, d, *_ in files}
    assert by["p_40x40_444_blocks1"].count(b"\xff\xd7") >= 3       # the RSTn counter wraps past 7 three times
    assert any(b"\xff\x00" in d for n, d, *_ in files if "q100" in n)
    assert np.array_equal(decoded("x_no_dht", by["x_no_dht"], (17, 33, 3)).image, decoded("p_17x33_420_noise", by["p_17x33_420_noise"], (17, 33, 3)).image)


def test_without_a_shape_the_file_says_its_own():
    name, data, shape, _ = corpus_files()[8]
    assert D.decode(data).image.shape == shape


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("src,dst", [((37, 53), (16, 23)), ((16, 23), (37, 53)), ((64, 48), (64, 48)), ((1080, 8), (540, 8)), ((9, 5), (4, 11))])
def test_the_resize_restatement_equals_pillow(src, dst, channels):
    a = np.random.default_rng(src[0] + channels).integers(0, 256, src + (channels,), dtype=np.uint8)
    a = a[..., 0] if channels == 1 else a
    want = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), Image.BICUBIC))
    assert np.array_equal(D.resize_bicubic(a, *dst), want)


def test_malformed_files():
    seen = set()
    for name, data, shape, status in malformed():
        r = decoded(name, data, shape)
        if status is not None:
            assert r.status == status, (name, r.status, status)
        assert r.status != D.OK, name
        assert r.image.shape == shape and not r.image.any()
        seen.add(r.status)
    assert seen == {D.BAD_STRUCTURE, D.UNSUPPORTED, D.MISSING_TABLE, D.CORRUPT, D.TRUNCATED}


def test_jpeg_info_on_the_host():
    from soar_amd import jpeg
    for name, data, shape, _ in [c for c in corpus_files() if c[0][0] in "pe"][::7]:
        H, W, C, sub = jpeg.jpeg_info(data)
        assert (H, W, C) == shape
        assert sub == ("grey" if C == 1 else name.split("_")[2]), name
    for name in ("u_progressive", "u_440", "u_cmyk", "t_header", "s_no_soi"):
        data = [d for n, d, *_ in malformed() if n == name][0]
        with pytest.raises(ValueError):
            jpeg.jpeg_info(data)


def test_cpu_tensors_and_bad_arguments_are_refused():
    import torch
    from soar_amd import frames, jpeg, video
    data, offsets = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 4])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg.decode_jpeg(data, offsets, 8, 8, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg.resize_images(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        jpeg.read_jpeg_files(["a.jpg"], device="cpu")
    assert jpeg.JPEG_STATUS[0] == "ok" and len(jpeg.JPEG_STATUS) == 6
    assert callable(video.MjpegReader) and callable(video.read_video) and callable(frames.extract_frames)


def test_the_c_entry_points_check_their_arguments():
    import ctypes as C
    from soar_amd import build, hip_lib
    build.build()
    lib = hip_lib.lib()
    a = hip_lib.SoarJpegDecodeArgs()
    n = C.c_size_t(0)
    a.B, a.H, a.W, a.channels, a.total_bytes = 2, 17, 33, 3, 1000
    assert lib.soar_jpeg_decode_workspace_bytes(C.byref(a), C.byref(n)) == 0 and n.value % 256 == 0
    assert n.value >= 2 * 3 * 3 * 5 * 64 * 3                       # coefficients and samples of the 4:4:4 block grid
    a.channels = 2
    assert lib.soar_jpeg_decode_workspace_bytes(C.byref(a), C.byref(n)) != 0 and "bad arguments" in hip_lib.last_error()
    a.channels = 3
    assert lib.soar_jpeg_decode(C.byref(a), None, 0, None, None, None, None) != 0 and "NULL" in hip_lib.last_error()
    a.data, a.offsets = 256, 256
    assert lib.soar_jpeg_decode(C.byref(a), 256, 16, 256, 256, 256, None) != 0 and "workspace" in hip_lib.last_error()
    r = hip_lib.SoarResizeArgs()
    r.B, r.H, r.W, r.channels, r.out_h, r.out_w, r.ksize_h, r.ksize_v = 1, 8, 8, 3, 4, 4, 0, 5
    assert lib.soar_resize_u8(C.byref(r), None, None) != 0 and "bad arguments" in hip_lib.last_error()
    r.ksize_h = 5
    assert lib.soar_resize_u8(C.byref(r), None, None) != 0 and "NULL" in hip_lib.last_error()


# ---- the shared header on the host, under the sanitizers ----------------------------------------------------------------------------------
def _host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "jpeg_entropy_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(HERE, "..", "soar_amd", "csrc"), os.path.join(HERE, "tools", "jpeg_entropy_host.cpp"), "-o", exe]
    probe = subprocess.run(cmd, capture_output=True, text=True)
    if probe.returncode != 0:
        if "asan" in probe.stderr.lower() or "ubsan" in probe.stderr.lower() or "sanitizer" in probe.stderr.lower():
            pytest.skip("the compiler has no sanitizer runtime: " + probe.stderr[-300:])
        raise AssertionError(probe.stderr[-3000:])
    return exe


def test_the_shared_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = _host_program(tmp_path)
    files = [(n, d, s) for n, d, s, _ in corpus_files() + malformed() + prefixes() + corruptions()]
    folder = tmp_path / "files"
    folder.mkdir()
    with open(tmp_path / "list.txt", "w") as f:
        for name, data, shape in files:
            (folder / name).write_bytes(data)
            f.write(f"{name} {' '.join(str(v) for v in (shape or (0, 0, 0)))}\n")
    run = subprocess.run([exe, str(folder), str(tmp_path / "list.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
    got = {}
    for line in run.stdout.splitlines():
        name, status, intervals, checksum = line.split()
        got[name] = (int(status), int(intervals), int(checksum, 16))
    assert sorted(got) == sorted(n for n, *_ in files)
    statuses = set()
    for name, data, shape in files:
        r = decoded(name, data, shape)
        assert got[name] == (r.status, r.intervals, r.checksum), (name, got[name], (r.status, r.intervals, r.checksum))
        statuses.add(r.status)
    assert statuses == set(range(6))
