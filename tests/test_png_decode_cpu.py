"""PNG input without a device: the restatement (tests/png_decode_ref.py) against Pillow on a corpus whose coverage of
RFC 1951 and of the PNG format is asserted from the restatement's own reports; the segment rule; malformed files; and the decoder's
shared header (csrc/png_inflate.h) built for the host under the address and undefined-behaviour sanitizers and run over all of them.
tests/test_png_decode_gpu.py asks the same of the kernels."""
import io
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import png_decode_ref as D
import png_ref as P
import test_png_cpu as T

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_SHAPES = [(1, 1), (1, 7), (7, 1), (3, 5), (33, 70), (65, 3), (130, 2)]         # (H, W); 65 and 130 rows: past a 64-row band
MODES = T.MODES
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY,
              "filtered": zlib.Z_FILTERED}


def pillow_file(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img[..., 0] if img.shape[2] == 1 else img).save(buf, "PNG", **kw)
    return buf.getvalue()


# how a small image becomes a file: (name, image -> file, the segments expected or None: whatever the restatement says)
def _sources():
    out = [(f"pillow{lv}", (lambda im, lv=lv: pillow_file(im, compress_level=lv)), 1) for lv in (0, 1, 6, 9)]
    out.append(("pillow-optimize", lambda im: pillow_file(im, optimize=True), 1))
    for piece in (32, 256, 65535):
        for f in ("adaptive", 3):
            out.append((f"ours{piece}-{f}", (lambda im, piece=piece, f=f: P.png_file(im, f, piece)), "pieces"))
    for i, (name, strat) in enumerate(STRATEGIES.items()):
        out.append((f"zlib-{name}", (lambda im, strat=strat, i=i: D.make_png(im, filters=i % 5, level=6, strategy=strat)), 1))
    for f in (0, 1, 2, 4):
        out.append((f"zlib-forced{f}", (lambda im, f=f: D.make_png(im, filters=f, level=9)), 1))
    out.append(("zlib-1-byte-idats", lambda im: D.make_png(im, idat_sizes=1), None))
    out.append(("zlib-empty-idats", lambda im: D.make_png(im, idat_sizes=[0, 3, 0, 0, 1]), None))
    out.append(("zlib-ancillary", lambda im: D.make_png(im, idat_sizes=7, extra_chunks=[(b"tEXt", b"Comment\0before", "before"),
                                                                                       (b"tIME", bytes(7), 1), (b"zzZz", b"", 2)]), None))
    return out


SOURCES = _sources()
_CORPUS = []


def period_image():
    """72 x 900 grey noise whose rows repeat with a period of 36 rows: with filter None a distance of 36 x 901 = 32436"""
    rows = np.random.RandomState(5).randint(0, 256, (36, 900, 1)).astype(np.uint8)
    return np.concatenate([rows, rows])


def corpus():
    """[(name, file, image, segments expected or None)], made once"""
    if _CORPUS:
        return _CORPUS
    i = 0
    for h, w in SMALL_SHAPES:
        for c in T.CHANNELS:
            for kind in T.KINDS:
                name, make, seg = SOURCES[i % len(SOURCES)]
                img = T.make_image(kind, h, w, c, seed=i)
                if seg == "pieces":
                    piece = int(name[4:].split("-")[0])
                    seg = -(-h * (1 + w * c) // piece)
                _CORPUS.append((f"{h}x{w}x{c}-{kind}-{name}", make(img), img, seg))
                i += 1
    img = period_image()
    _CORPUS.append(("72x900-period36-level6", D.make_png(img, filters=0, level=6), img, 1))
    _CORPUS.append(("72x900-period36-stored", D.make_png(img, filters=0, level=0, mem_level=1), img, 1))
    img = T.make_image("white", 72, 900, 1)
    _CORPUS.append(("72x900-white-adaptive", D.make_png(img, level=6), img, 1))
    img = T.avatar_image(3)
    _CORPUS.append(("270x480x3-avatar-pillow", pillow_file(img), img, 1))
    img = T.avatar_image(4)
    _CORPUS.append(("270x480x4-avatar-ours", P.png_file(img), img, -(-270 * (1 + 480 * 4) // 65535)))
    img = T.make_image("blob", 33, 70, 3)
    _CORPUS.append(("33x70x3-plte", D.make_png(img, extra_chunks=[(b"PLTE", bytes(range(30)), "before")]), img, 1))
    # every filter in one file, forced row by row; and adaptive filtering of content that uses all five
    img = T.make_image("blob", 10, 9, 3)
    _CORPUS.append(("10x9x3-filters-by-row", D.make_png(img, filters=[0, 1, 2, 3, 4, 4, 3, 2, 1, 0]), img, 1))
    _CORPUS.extend(segment_cases())
    return _CORPUS


def repeating_image():
    """33 x 70 grey: a blob's rows twice over, so that the second half is matches into the first"""
    half = T.make_image("blob", 16, 70, 1)
    return np.concatenate([half, half, half[:1]])


def segment_cases():
    out = []
    img = repeating_image()
    S = 33 * 71
    # a full flush forgets the window: every part stands alone, and holds matches of its own (the blob's smooth rows)
    flat = np.repeat(T.make_image("noise", 33, 10, 1), 7, axis=1)                  # runs inside a row: matches inside every part
    out.append(("33x70-full-flush", D.make_png(flat, filters=0, flush_at=[S // 3, 2 * S // 3], flush_mode=zlib.Z_FULL_FLUSH, split_at_flushes=True),
                flat, 3))
    # a sync flush leaves the window: the second part's matches reach into the first
    out.append(("33x70-sync-flush", D.make_png(img, filters=0, flush_at=[16 * 71 + 5], flush_mode=zlib.Z_SYNC_FLUSH, split_at_flushes=True), img, 1))
    # a stored block whose content holds 00 00 FF FF, cut right behind it: the candidate begins inside the block
    row = np.asarray([5, 0, 0, 255, 255] + [9] * 20, np.uint8).reshape(1, -1, 1)
    z = D.zlib_stream_of(D.make_png(row, filters=0, level=0))
    at = z.index(b"\x00\x00\xff\xff", 7) + 4
    out.append(("1x25-marker-in-stored", D.make_png(row, filters=0, level=0, idat_sizes=[at]), row, 1))
    return out


_DECODED = {}


def decoded(name, data):
    if name not in _DECODED:
        _DECODED[name] = D.decode(data)
    return _DECODED[name]


def test_the_restatement_gives_pillows_pixels_and_mode():
    for name, data, img, seg in corpus():
        r = decoded(name, data)
        assert r.status == D.OK, (name, r.status)
        if "ancillary" in name:
            # a chunk between two IDATs: the PNG specification wants the IDATs consecutive and Pillow stops at the chunk ("image file
            # is truncated"); this decoder skips it, as libpng's readers do, and the pixels are checked against the source alone
            assert others_refuse(data) and np.array_equal(r.image, img), name
            continue
        back = Image.open(io.BytesIO(data))
        assert r.shape == img.shape and back.mode == MODES[img.shape[2]], name
        assert np.array_equal(r.image, np.asarray(back).reshape(img.shape)) and np.array_equal(r.image, img), name


def test_the_corpus_covers_the_format():
    reps = {name: decoded(name, data).report for name, data, _, _ in corpus()}
    every = list(reps.values())
    assert {0, 1, 2} <= set().union(*(r.block_types for r in every))
    assert max(r.stored_blocks for r in every) > 1
    assert {16, 17, 18} <= set().union(*(r.clen_symbols for r in every))
    assert max(r.max_length for r in every) == 258
    assert any(r.overlap for r in every)
    assert max(r.max_distance for r in every) >= 16385
    assert max(r.longest_code for r in every) >= 12
    assert set().union(*(r.filters for r in every)) == {0, 1, 2, 3, 4}
    for f in range(5):                                           # forced, each on its own
        assert any(r.filters == {f} for n, r in reps.items() if "forced" in n or "ours" in n or "zlib-" in n), f
    assert any(len(r.filters) >= 3 for n, r in reps.items() if "adaptive" in n or "pillow" in n)
    assert any(r.idat_sizes and max(r.idat_sizes) == 1 and r.idats > 4 for r in every)
    assert any(0 in r.idat_sizes for r in every)
    assert any(r.boundary_in_code for r in every)
    assert any(r.chunks[1] == b"tEXt" for r in every)
    assert any(b"tIME" in r.chunks[2:] and r.chunks.index(b"tIME") > r.chunks.index(b"IDAT") for r in every)
    assert any(b"PLTE" in r.chunks for r in every)
    # measured once: the period of 36 rows makes level 6 halve the noise, so the far matches are real; level 0 stores; a 2-byte
    # stream at level 6 is one fixed block
    far = reps["72x900-period36-level6"]
    assert far.max_distance == 36 * 901 and len(dict(corpus_files())["72x900-period36-level6"]) < 0.55 * 72 * 901
    assert reps["72x900-period36-stored"].block_types == {0} and reps["72x900-period36-stored"].stored_blocks > 1
    tiny = D.decode(D.make_png(np.full((1, 1, 1), 7, np.uint8), filters=0, level=6))
    assert tiny.status == 0 and tiny.report.block_types == {1}


def corpus_files():
    return [(name, data) for name, data, _, _ in corpus()]


def test_segments():
    for name, data, img, seg in corpus():
        r = decoded(name, data)
        if seg is not None:
            assert r.segments == seg, (name, r.segments, seg)
    reps = {name: decoded(name, data) for name, data, _, _ in corpus()}
    assert reps["33x70-full-flush"].report.max_distance > 1 and reps["33x70-full-flush"].report.max_length >= 3
    assert reps["33x70-sync-flush"].report.max_distance == 16 * 71     # the second half's matches reach across the marker
    assert reps["270x480x4-avatar-ours"].segments == 8


# ---- malformed files ------------------------------------------------------------------------------------------------------------------
def good_file():
    return D.make_png(T.make_image("blob", 7, 5, 3), filters=4, level=6)


def ihdr_edit(png, **kw):
    def edit(i, kind, data):
        if kind != b"IHDR":
            return [(kind, data)]
        f = dict(zip(("w", "h", "depth", "colour", "comp", "filt", "lace"), struct.unpack(">IIBBBBB", data)))
        f.update(kw)
        return [(kind, struct.pack(">IIBBBBB", *(f[k] for k in ("w", "h", "depth", "colour", "comp", "filt", "lace"))))]
    return D.rebuild(png, edit)


def flip(png, at):
    return png[:at] + bytes([png[at] ^ 0x40]) + png[at + 1:]


def zstream(blocks, data=b""):
    """78 01, the blocks' bytes, the Adler-32 of ``data``"""
    return b"\x78\x01" + blocks + struct.pack(">I", zlib.adler32(data))


def bits(*fields):
    """(value, n) integer fields, or (code, n, "code") Huffman codes -> bytes"""
    w = P.BitWriter()
    for f in fields:
        (w.code if len(f) == 3 else w.bits)(f[0], f[1])
    w.align()
    return bytes(w.out)


def incomplete_literal_code():
    """a dynamic block whose literal/length code is a 1-bit code for 0 and a 2-bit code for 256: 3/4 of a code"""
    order = P.CLEN_ORDER
    cl = {0: 1, 1: 2, 2: 2}                                      # the code-length code: 0 -> 0, 1 -> 10, 2 -> 11 (complete)
    f = [(1, 1), (2, 2), (0, 5), (0, 5), (14, 4)] + [(cl.get(order[i], 0), 3) for i in range(18)]
    code = {0: (0, 1, "code"), 1: (2, 2, "code"), 2: (3, 2, "code")}
    lens = [1] + [0] * 255 + [2] + [0]                           # 257 literal/length lengths and one distance length
    return bits(*(f + [code[l] for l in lens]))


def malformed():
    """[(name, file, status)]"""
    g = good_file()
    ch = D.chunks_of(g)
    z = D.zlib_stream_of(g)
    stream = D.decode(g).stream
    idat_at = next(o for o, k, _ in ch if k == b"IDAT")
    S = len(stream)
    out = [
        ("bad-signature", b"\x89PNX" + g[4:], D.BAD_STRUCTURE),
        ("truncated-in-idat", g[:idat_at + 20], D.BAD_STRUCTURE),
        ("no-iend", g[:-12], D.BAD_STRUCTURE),
        ("no-idat", D.rebuild(g, lambda i, k, d: [] if k == b"IDAT" else [(k, d)]), D.BAD_STRUCTURE),
        ("ihdr-not-first", D.rebuild(g, lambda i, k, d: [(b"tEXt", b"a\0b"), (k, d)] if k == b"IHDR" else [(k, d)]), D.BAD_STRUCTURE),
        ("two-ihdr", D.rebuild(g, lambda i, k, d: [(k, d), (k, d)] if k == b"IHDR" else [(k, d)]), D.BAD_STRUCTURE),
        ("width-0", ihdr_edit(g, w=0), D.BAD_STRUCTURE),
        ("height-0", ihdr_edit(g, h=0), D.BAD_STRUCTURE),
        ("interlaced", ihdr_edit(g, lace=1), D.UNSUPPORTED),
        ("depth-16", ihdr_edit(g, depth=16), D.UNSUPPORTED),
        ("palette", ihdr_edit(g, colour=3), D.UNSUPPORTED),
        ("grey-alpha", ihdr_edit(g, colour=4), D.UNSUPPORTED),
        ("fdict", D.with_zlib_stream(g, b"\x78\x20" + z[2:]), D.UNSUPPORTED),
        ("method-7", D.with_zlib_stream(g, b"\x77\x0a" + z[2:]), D.UNSUPPORTED),
        ("zlib-check-bits", D.with_zlib_stream(g, b"\x78\x02" + z[2:]), D.CORRUPT),
        ("ihdr-crc", flip(g, 8 + 8 + 13 + 1), D.BAD_CRC),
        ("idat-crc", flip(g, idat_at + 8 + len(z) + 2), D.BAD_CRC),
        ("idat-byte", flip(g, idat_at + 8 + len(z) // 2), D.BAD_CRC),
        ("block-type-3", D.with_zlib_stream(g, zstream(b"\x07")), D.CORRUPT),
        ("len-nlen", D.with_zlib_stream(g, zstream(b"\x01\x05\x00\x00\x00" + bytes(5))), D.CORRUPT),
        ("over-subscribed", D.with_zlib_stream(g, zstream(bits((1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (1, 3), (1, 3), (1, 3)) + bytes(8))),
         D.CORRUPT),
        ("incomplete-code-lengths", D.with_zlib_stream(g, zstream(bits((1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (0, 3), (0, 3), (0, 3)) + bytes(8))),
         D.CORRUPT),
        ("incomplete-literals", D.with_zlib_stream(g, zstream(incomplete_literal_code() + bytes(8))), D.CORRUPT),
        ("symbol-286", D.with_zlib_stream(g, zstream(bits((1, 1), (1, 2), (0b11000110, 8, "code")) + bytes(4))), D.CORRUPT),
        ("distance-code-30", D.with_zlib_stream(g, zstream(bits((1, 1), (1, 2), (0x30 + 65, 8, "code"), (1, 7, "code"), (30, 5, "code")) + bytes(4))),
         D.CORRUPT),
        ("distance-before-start", D.with_zlib_stream(g, zstream(bits((1, 1), (1, 2), (1, 7, "code"), (0, 5, "code"), (0, 7, "code")))), D.CORRUPT),
        ("distance-2-after-1", D.with_zlib_stream(g, zstream(bits((1, 1), (1, 2), (0x30 + 65, 8, "code"), (1, 7, "code"), (1, 5, "code"), (0, 7, "code")))),
         D.CORRUPT),
        ("input-ends", D.with_zlib_stream(g, z[:len(z) // 2]), D.CORRUPT),
        ("adler-cut-short", D.with_zlib_stream(g, z[:-2]), D.CORRUPT),
        ("one-byte-more", D.with_zlib_stream(g, zlib.compress(stream + b"\x00")), D.WRONG_LENGTH),
        ("one-byte-fewer", D.with_zlib_stream(g, zlib.compress(stream[:-1])), D.WRONG_LENGTH),
        ("a-row-more", D.with_zlib_stream(g, zlib.compress(stream + stream[:16])), D.WRONG_LENGTH),
        ("bytes-behind-the-adler", D.with_zlib_stream(g, z + b"\x00"), D.WRONG_LENGTH),
        ("adler", D.with_zlib_stream(g, z[:-1] + bytes([z[-1] ^ 1])), D.BAD_ADLER),
        ("filter-5", D.with_zlib_stream(g, zlib.compress(stream[:16] + b"\x05" + stream[17:])), D.BAD_FILTER),
        ("filter-255-last-row", D.with_zlib_stream(g, zlib.compress(stream[:S - 16] + b"\xff" + stream[S - 15:])), D.BAD_FILTER),
        ("unknown-critical-chunk", D.rebuild(g, lambda i, k, d: [(b"ABCD", b"x"), (k, d)] if k == b"IDAT" else [(k, d)]), D.UNSUPPORTED),
    ]
    return out


# what Pillow and zlib still open: Pillow stops reading at the image's last row, so neither the Adler-32 nor bytes behind it nor a
# stream that is too long is looked at; zlib.decompress knows nothing of the image's size
# and Pillow checks no IDAT's CRC
OTHERS_ACCEPT = {"one-byte-more", "a-row-more", "bytes-behind-the-adler", "adler", "adler-cut-short", "idat-crc", "no-iend", "two-ihdr",
                 "unknown-critical-chunk", "ihdr-not-first"}


def truncations():
    g = good_file()
    return [(f"cut-{n:04d}", g[:n]) for n in list(range(100)) + list(range(100, len(g), 7)) + [len(g) - 1]]


def others_refuse(data):
    try:
        im = Image.open(io.BytesIO(data))
        im.load()
        np.asarray(im)
    except Exception:
        return True
    return False


def test_malformed_files_have_their_status_and_other_decoders_refuse_them_too():
    accepted = set()
    for name, data, status in malformed():
        r = D.decode(data)
        assert r.status == status, (name, r.status, status)
        assert not r.image.any(), name
        if not others_refuse(data):
            accepted.add(name)
    # (an Adler-32 that Pillow does not reach is still wrong for zlib itself)
    g = good_file()
    z = D.zlib_stream_of(g)
    with pytest.raises(zlib.error):
        zlib.decompress(z[:-1] + bytes([z[-1] ^ 1]))
    with pytest.raises(zlib.error):
        zlib.decompress(z[:-2])
    assert accepted <= OTHERS_ACCEPT, accepted - OTHERS_ACCEPT


def test_every_truncation_is_refused():
    g = good_file()
    assert D.decode(g).status == D.OK
    # Pillow is content with the bytes that give the last row: the smallest prefix of the zlib stream that inflates to all of it
    z, at = D.zlib_stream_of(g), next(o for o, k, _ in D.chunks_of(g) if k == b"IDAT") + 8
    enough = next(k for k in range(len(z) + 1) if len(zlib.decompressobj().decompress(z[:k])) == 7 * 16)
    for name, data in truncations():
        r = D.decode(data)
        assert r.status == D.BAD_STRUCTURE, (name, r.status)
        assert others_refuse(data) or len(data) >= at + enough, name


def test_another_shape_than_the_calls_is_unsupported():
    g = good_file()
    assert D.decode(g, want=(7, 5, 3)).status == D.OK
    for want in ((7, 5, 4), (5, 7, 3), (7, 6, 3)):
        r = D.decode(g, want=want)
        assert r.status == D.UNSUPPORTED and r.image.shape == want and not r.image.any()


def test_png_info():
    from soar_amd.png import png_info
    for name, data, img, _ in corpus()[:20]:
        assert png_info(data) == img.shape == D.png_info(data)
    for bad in (b"", good_file()[:25], b"GIF89a" + bytes(40), ihdr_edit(good_file(), depth=16), ihdr_edit(good_file(), colour=3)):
        with pytest.raises(ValueError):
            png_info(bad)


def test_statuses_of_the_package_are_the_restatements():
    from soar_amd import png
    for n in ("OK", "BAD_STRUCTURE", "UNSUPPORTED", "BAD_CRC", "CORRUPT", "WRONG_LENGTH", "BAD_ADLER", "BAD_FILTER"):
        assert getattr(png, "PNG_" + n) == getattr(D, n)
    header = open(os.path.join(HERE, "..", "include", "soar_hip.h")).read()
    for n in ("BAD_STRUCTURE", "UNSUPPORTED", "BAD_CRC", "CORRUPT", "WRONG_LENGTH", "BAD_ADLER", "BAD_FILTER"):
        assert f"#define SOAR_PNG_{n} {getattr(D, n)}" in " ".join(header.split())


def test_decode_refuses_cpu_tensors_and_bad_arguments_before_any_launch():
    import ctypes as C
    import torch
    from soar_amd import hip_lib
    from soar_amd.png import decode_png
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        decode_png(torch.zeros(100, dtype=torch.uint8), torch.tensor([0, 100]), 1, 1, 1)
    lib = hip_lib.lib()
    a = hip_lib.SoarPngDecodeArgs()
    nb = C.c_size_t(0)
    a.B, a.H, a.W, a.channels, a.total_bytes = 1, 4, 4, 3, 100
    assert lib.soar_png_decode_workspace_bytes(C.byref(a), C.byref(nb)) == 0 and nb.value > 0
    for field, value in (("B", -1), ("channels", 2), ("H", 0), ("W", -3), ("total_bytes", -1)):
        b = hip_lib.SoarPngDecodeArgs()
        b.B, b.H, b.W, b.channels, b.total_bytes = 1, 4, 4, 3, 100
        setattr(b, field, value)
        assert lib.soar_png_decode_workspace_bytes(C.byref(b), C.byref(nb)) != 0 and field.split("_")[0] in hip_lib.last_error()
    # null pointers and a workspace that is too small: refused before any launch, so this needs no device
    assert lib.soar_png_decode(C.byref(a), None, 0, None, None, None, None) != 0 and "NULL" in hip_lib.last_error()
    a.data, a.offsets = 256, 256
    assert lib.soar_png_decode(C.byref(a), 256, 16, 256, 256, 256, None) != 0 and "workspace" in hip_lib.last_error()


# ---- the shared header on the host, under the sanitizers ----------------------------------------------------------------------------------
def _host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "png_inflate_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(HERE, "..", "soar_amd", "csrc"), os.path.join(HERE, "tools", "png_inflate_host.cpp"), "-o", exe]
    probe = subprocess.run(cmd, capture_output=True, text=True)
    if probe.returncode != 0:
        if "asan" in probe.stderr.lower() or "ubsan" in probe.stderr.lower() or "sanitizer" in probe.stderr.lower():
            pytest.skip("the compiler has no sanitizer runtime: " + probe.stderr[-300:])
        raise AssertionError(probe.stderr[-3000:])
    return exe


def test_the_shared_header_on_the_host_under_the_sanitizers(tmp_path):
    exe = _host_program(tmp_path)
    files = corpus_files() + [(n, d) for n, d, _ in malformed()] + truncations()
    folder = tmp_path / "files"
    folder.mkdir()
    for name, data in files:
        (folder / name).write_bytes(data)
    run = subprocess.run([exe, str(folder)], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-3000:])
    got = {}
    for line in run.stdout.splitlines():
        name, status, segments, adler = line.split()
        got[name] = (int(status), int(segments), int(adler, 16))
    assert sorted(got) == sorted(n for n, _ in files)
    for name, data in files:
        r = _DECODED.get(name) or D.decode(data, report=False)
        want = (r.status, r.segments if r.status == 0 else got[name][1], zlib.adler32(r.stream) if r.status == 0 else 0)
        assert got[name] == want, (name, got[name], want)
