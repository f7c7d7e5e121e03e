"""PNG output without a device: the NumPy / pure-Python restatement of the encoder (tests/png_ref.py) against Pillow, zlib and a plain
unfiltering loop -- any decoder must give the pixels back bit for bit -- its size conditions, and the C entry points' argument checks."""
import heapq
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_ref as P
from test_video_cpu import make_image as make_rgb

SHAPES = [(1, 1), (1, 3), (2, 2), (7, 5), (17, 23), (33, 70)]                                        # (H, W)
CHANNELS = [1, 3, 4]
KINDS = ["noise", "ramp", "blob", "extremes", "white"]
FILTERS = ["adaptive", 0, 1, 2, 3, 4]
PIECES = [32, 256]
MODES = {1: "L", 3: "RGB", 4: "RGBA"}
# The restatement's deflate bytes against zlib's own Z_RLE level-1 pieces of the same filtered bytes, on the avatar-like image at the
# default piece size: measured 1.027 (RGB) and 1.033 (RGBA); the cause is the 153-byte header without run-length coding and Shannon
# lengths in place of Huffman's.  The bar leaves one point for another platform's rounding of the image itself.
RLE_BAR = 1.045


def make_image(kind, h, w, c, seed=0):
    """uint8 [h,w,c]: test_video_cpu's kinds, and all-white; one channel is the red one, a fourth is another seed's noise or blob"""
    if kind == "white":
        return np.full((h, w, c), 255, np.uint8)
    rgb = make_rgb(kind, h, w, seed)
    if c == 1:
        return np.ascontiguousarray(rgb[..., :1])
    if c == 3:
        return rgb
    alpha = make_rgb("noise" if kind == "noise" else "blob", h, w, seed + 7)[..., 1:2]
    return np.concatenate([rgb, alpha], axis=2)


def avatar_image(c):
    """the avatar-like image the piece size was chosen on: a shaded body with 2-level noise on white, 270 x 480"""
    H, W = 270, 480
    y, x = np.mgrid[0:H, 0:W]
    a = np.exp(-(((y - 0.5 * H) / (0.35 * H)) ** 2 + ((x - 0.5 * W) / (0.12 * W)) ** 2) ** 2)[..., None]
    rs = np.random.RandomState(0)
    shade = np.array([200.0, 120.0, 90.0]) * (0.6 + 0.4 * np.sin(x / 9.0 + y / 13.0)[..., None]) + rs.randn(H, W, 3) * 2
    img = (255 * (1 - a) + a * shade).clip(0, 255).astype(np.uint8)
    return img if c == 3 else np.concatenate([img, (a * 255).astype(np.uint8)], -1)


def row_image(row):
    """one row of grey pixels: with filter 0 forced the filtered stream is a 0 and then these bytes"""
    return np.asarray(row, np.uint8).reshape(1, -1, 1)


def run_row(n, lead=3):
    """``lead`` distinct bytes, a run of n equal ones, two distinct bytes"""
    return list(range(1, lead + 1)) + [200] * n + [17, 18]


def fibonacci_image():
    """one row whose byte counts are the Fibonacci numbers 2, 3, 5 .. 17711 (46 365 bytes, 20 values) -- the filter byte in front and the
    end of the block are the sequence's two ones -- with no two equal bytes adjacent: the most frequent first, into the even places
    and then the odd ones"""
    fib = [2, 3]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    n = sum(fib)
    order = np.concatenate([np.full(cnt, 1 + v, np.uint8) for v, cnt in sorted(enumerate(fib), key=lambda t: -t[1])])
    row = np.zeros(n, np.uint8)
    row[0::2] = order[:(n + 1) // 2]
    row[1::2] = order[(n + 1) // 2:]
    return row_image(row), fib


# (name, image, filters, piece_bytes): every one at 64-byte pieces, one channel, filter 0
EDGE_CASES = [(f"run of {n}", row_image(run_row(n)), 0, 64) for n in (2, 3, 4, 258, 259, 260, 261, 517)] + [
    ("a run across a piece end", row_image(list(range(1, 58)) + [200] * 20 + [5]), 0, 64),
    ("rows of piece - 2 bytes", make_image("noise", 9, 62, 1), 0, 64),                   # with the filter byte: piece - 1, piece, piece + 1
    ("rows of piece - 1 bytes", make_image("noise", 9, 63, 1), 0, 64),
    ("rows of piece bytes", make_image("noise", 9, 64, 1), 0, 64),
    ("a last piece of one byte", row_image(np.arange(64) * 3 + 1), 0, 64),
    ("one distinct byte value", np.zeros((1, 200, 1), np.uint8), 0, 64),
]
# A block's header is 153 bytes, so a piece of 64 bytes is always stored: the same run lengths again behind 600 bytes that cost a bit
# each, in pieces large enough for the dynamic block to win, so that the tokens are coded and not only found
CALM = [1, 2] * 300
EDGE_CASES += [(f"coded run of {n}", row_image(CALM + run_row(n)), 0, 2048) for n in (2, 3, 4, 258, 259, 260, 261, 517)] + [
    ("a coded run across a piece end", row_image([1, 2] * 250 + [200] * 40 + [1, 2] * 250), 0, 512),
    ("one distinct byte value, coded", np.zeros((1, 2000, 1), np.uint8), 0, 1024),
    ("coded rows of piece bytes", make_image("blob", 5, 512, 1), 1, 512),
]


def all_cases():
    """(name, image, filters, piece_bytes): what tests/test_png_gpu.py asks of the kernels too"""
    for h, w in SHAPES:
        for c in CHANNELS:
            for kind in KINDS:
                img = make_image(kind, h, w, c)
                for f in FILTERS:
                    for piece in PIECES:
                        yield f"{kind} {h}x{w}x{c} filter {f} piece {piece}", img, f, piece
    yield from EDGE_CASES
    yield "fibonacci", fibonacci_image()[0], 0, 65535
    for c in (3, 4):
        yield f"avatar x{c}", avatar_image(c), "adaptive", P.DEFAULT_PIECE_BYTES


def chunks_of(png):
    """walks the chunks by hand: [(type, data)], every CRC checked against zlib's"""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    p, out = 8, []
    while p < len(png):
        n = struct.unpack_from(">I", png, p)[0]
        kind, data = png[p + 4:p + 8], png[p + 8:p + 8 + n]
        assert len(data) == n and struct.unpack_from(">I", png, p + 8 + n)[0] == zlib.crc32(kind + data), (kind, p)
        out.append((kind, data))
        p += 12 + n
    assert p == len(png)
    return out


def unfilter(stream, h, w, c):
    """the PNG specification's reconstruction, byte by byte"""
    stride = w * c
    assert len(stream) == h * (1 + stride)
    out = np.zeros((h, stride), np.uint8)
    prev = [0] * stride
    for y in range(h):
        t = stream[y * (1 + stride)]
        line = stream[y * (1 + stride) + 1:(y + 1) * (1 + stride)]
        cur = [0] * stride
        for x in range(stride):
            a = cur[x - c] if x >= c else 0
            b = prev[x]
            cc = prev[x - c] if x >= c else 0
            if t == 0:
                pred = 0
            elif t == 1:
                pred = a
            elif t == 2:
                pred = b
            elif t == 3:
                pred = (a + b) // 2
            else:
                assert t == 4
                pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else cc)
            cur[x] = (line[x] + pred) & 255
        out[y] = cur
        prev = cur
    return out.reshape(h, w, c)


def check_file(img, png, stats, piece_bytes, unfiltered=True):
    h, w, c = img.shape
    back = Image.open(io.BytesIO(png))
    assert back.mode == MODES[c] and back.size == (w, h)
    assert np.array_equal(np.asarray(back).reshape(h, w, c), img)
    chunks = chunks_of(png)
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and set(kinds[1:-1]) == {b"IDAT"} and chunks[-1][1] == b""
    assert chunks[0][1] == struct.pack(">IIBBBBB", w, h, 8, P.COLOUR_TYPE[c], 0, 0, 0)
    S = h * (1 + w * c)
    assert len(chunks) == 2 + (S + piece_bytes - 1) // piece_bytes + 1                # a piece per IDAT, and the final one
    assert chunks[-2][1][:2] == b"\x03\x00" and len(chunks[-2][1]) == 6
    stream = zlib.decompress(b"".join(d for k, d in chunks if k == b"IDAT"))
    assert stream == stats["stream"] and len(stream) == S
    assert len(png) <= P.png_bound(h, w, c, piece_bytes)
    for piece in stats["pieces"]:
        assert piece["lengths"] is None and piece["stored"] and piece["bytes"] <= 153 or max(piece["lengths"]) <= 15
        assert piece["stored"] or len(piece["payload"]) < 5 + piece["bytes"]
    if unfiltered:
        assert np.array_equal(unfilter(stream, h, w, c), img)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_decoder_gives_the_pixels_back(shape, c, kind):
    img = make_image(kind, *shape, c)
    for f in FILTERS:
        for piece in PIECES:
            png, stats = P.encode(img, f, piece)
            assert f == "adaptive" or set(stats["types"]) == {f}
            check_file(img, png, stats, piece, unfiltered=piece == PIECES[0])          # (the stream does not depend on the piece size)


def test_the_adaptive_filter_takes_the_smallest_sum_and_the_lowest_type_on_a_tie():
    # a white image: None costs 1 per byte (|255 as int8|), Sub costs 1 per pixel's first byte only, Up costs 0 below the first row
    assert P.encode(make_image("white", 4, 6, 3), "adaptive", 64)[1]["types"] == [1, 2, 2, 2]
    # all zeros: every filter costs 0, None wins
    assert P.encode(np.zeros((3, 5, 4), np.uint8), "adaptive", 64)[1]["types"] == [0, 0, 0]
    kinds = set()
    for kind in KINDS:
        kinds |= set(P.encode(make_image(kind, 33, 70, 3), "adaptive", 256)[1]["types"])
    assert kinds == {0, 1, 2, 3, 4}                                   # the cases reach every type through the adaptive choice too


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda t: t[0])
def test_edge_cases_of_runs_pieces_and_rows(case):
    name, img, f, piece = case
    png, stats = P.encode(img, f, piece)
    check_file(img, png, stats, piece)
    S = len(stats["stream"])
    if name.startswith("run of"):
        n = int(name.split()[-1])
        toks = [t for o in range(0, S, piece) for t in P.tokens(stats["stream"][o:o + piece])]
        assert (max(s for s, _, _ in toks) >= 257) == (n >= 4)                     # a match from 4 equal bytes on
    if name == "a run across a piece end":
        a, b = P.tokens(stats["stream"][:64]), P.tokens(stats["stream"][64:])
        assert a[-1][0] == P.length_symbol(5)[0] and b[:2] == [(200, 0, 0), P.length_symbol(13)]       # 6 bytes of it, then 14
    if name.startswith("rows of"):
        at = {(y * (img.shape[1] + 1)) % piece for y in range(img.shape[0])}
        assert 0 in at and (piece - 1 in at) == (img.shape[1] == piece - 2)        # the filter byte first, and last, in a piece
    if name.startswith("coded") or name.endswith("coded"):
        assert not stats["pieces"][0]["stored"]
    if name.startswith("coded run of"):
        n = int(name.split()[-1])
        want = [258] * ((n - 1) // 258) + ([(n - 1) % 258] if (n - 1) % 258 >= 3 else []) if n >= 4 else []
        got = [P.LENGTH_TABLE[s - 257][1] + ev for s, _, ev in P.tokens(stats["stream"][:piece]) if s >= 257]
        assert got == want and sum(1 for s, _, _ in P.tokens(stats["stream"][:piece]) if s == 200) == n - sum(want)
    if name == "a coded run across a piece end":
        assert not stats["pieces"][1]["stored"]
        assert P.tokens(stats["stream"][:512])[-1] == P.length_symbol(10) and P.tokens(stats["stream"][512:])[1] == P.length_symbol(28)
    if name == "a last piece of one byte":
        assert S % piece == 1 and stats["pieces"][-1]["bytes"] == 1 and stats["pieces"][-1]["stored"]
    if name == "one distinct byte value":
        assert all(p["stored"] for p in stats["pieces"])                           # (153 bytes of header never pay at 64)
    if name == "one distinct byte value, coded":
        # the literal, the end of block and length 249 once, length 258 three times: T = 6, Shannon 3, 3, 3, 1, and the eighth that is
        # missing shortens the first symbol
        assert [l for l in stats["pieces"][0]["lengths"] if l] == [2, 3, 3, 1]


def test_token_rule_on_runs_of_every_length_up_to_600():
    for n in range(1, 601):
        toks = P.tokens(bytes([9] * n))
        lits = [t for t in toks if t[0] < 256]
        lens = [P.LENGTH_TABLE[s - 257][1] + ev for s, _, ev in toks if s >= 257]
        assert len(lits) + sum(lens) == n and all(3 <= m <= 258 for m in lens)
        assert toks[0] == (9, 0, 0) and (n < 4) == (not lens)
        assert len(lits) - 1 in (0, 1, 2) and all(m == 258 for m in lens[:-1])


def test_the_15_bit_limit_holds_where_huffman_would_pass_it():
    img, fib = fibonacci_image()
    stream = bytes([0]) + img.tobytes()
    assert len(stream) <= 65535 and not np.any(img.ravel()[1:] == img.ravel()[:-1])
    assert all(s < 256 for s, _, _ in P.tokens(stream))
    heap = [(cnt, 0) for cnt in [1, 1] + fib]                      # with the filter byte and the end of block: Huffman's depth, unlimited
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    assert heap[0][1] > 15
    png, stats = P.encode(img, 0, 65535)
    assert len(stats["pieces"]) == 1 and not stats["pieces"][0]["stored"]
    L = stats["pieces"][0]["lengths"]
    assert max(L) == 15 and sum(2 ** (15 - l) for l in L if l) == 2 ** 15              # at the limit, and complete
    check_file(img, png, stats, 65535, unfiltered=False)
    assert zlib.decompress(b"".join(d for k, d in chunks_of(png) if k == b"IDAT")) == stream


def test_code_lengths_are_complete_and_at_most_15_bits():
    rs = np.random.RandomState(4)
    for trial in range(300):
        used = rs.choice(286, rs.randint(1, 286), replace=False)
        counts = np.zeros(286, np.int64)
        counts[used] = np.maximum(1, (rs.pareto(0.7, len(used)) * rs.choice([1, 10, 100])).astype(np.int64))
        counts[256] = 1
        if counts.sum() > 65536:
            counts = np.maximum(counts * 65000 // counts.sum(), (counts > 0).astype(np.int64))
            counts[256] = 1
        L = P.code_lengths(counts)
        assert all((l > 0) == (c > 0) for l, c in zip(L, counts)) and max(L) <= 15
        assert sum(2 ** (15 - l) for l in L if l) == 2 ** 15, trial
    # the extreme the floor f is there for: 65 535 tokens and 285 symbols seen once
    counts = np.ones(286, np.int64)
    counts[0] = 65536 - 285
    L = P.code_lengths(counts)
    assert max(L) <= 15 and sum(2 ** (15 - l) for l in L) == 2 ** 15


def test_noise_is_stored_and_nothing_passes_the_bound():
    for h, w in ((17, 23), (33, 70)):
        for c in CHANNELS:
            img = make_image("noise", h, w, c)
            for f in ("adaptive", 0):
                for piece in PIECES + [P.DEFAULT_PIECE_BYTES]:
                    png, stats = P.encode(img, f, piece)
                    assert all(p["stored"] for p in stats["pieces"]), (h, w, c, f, piece)
                    assert len(png) <= P.png_bound(h, w, c, piece)
                    if f == 0:
                        assert len(png) == P.png_bound(h, w, c, piece)             # the bound is the all-stored file


def test_png_bound_of_the_package_is_the_restatements():
    from soar_amd.png import DEFAULT_PIECE_BYTES, png_bound
    assert DEFAULT_PIECE_BYTES == P.DEFAULT_PIECE_BYTES
    for h, w, c, piece in ((1, 1, 1, 32), (33, 70, 4, 256), (1080, 1920, 4, None), (270, 480, 3, 65535)):
        assert png_bound(h, w, c, piece) == P.png_bound(h, w, c, piece or P.DEFAULT_PIECE_BYTES)
    for bad in (31, 65536):
        with pytest.raises(ValueError, match="piece_bytes"):
            png_bound(8, 8, 3, bad)


@pytest.mark.parametrize("c", [3, 4])
def test_the_avatar_like_image_is_no_larger_than_pillows_level_1_and_close_to_zlibs_rle(c):
    img = avatar_image(c)
    png, stats = P.encode(img)
    check_file(img, png, stats, P.DEFAULT_PIECE_BYTES, unfiltered=False)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "PNG", compress_level=1)
    print(f"avatar x{c}: {len(png)} bytes, Pillow at level 1 {len(b.getvalue())}")
    assert len(png) <= len(b.getvalue())
    rle = 0
    for o in range(0, len(stats["stream"]), P.DEFAULT_PIECE_BYTES):
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        rle += len(co.compress(stats["stream"][o:o + P.DEFAULT_PIECE_BYTES]) + co.flush(zlib.Z_FULL_FLUSH))
    ours = sum(len(p["payload"]) for p in stats["pieces"])
    print(f"avatar x{c}: deflate bytes {ours}, zlib's Z_RLE pieces {rle}, ratio {ours / rle:.4f}")
    assert ours <= RLE_BAR * rle


def test_png_refuses_cpu_tensors_and_wrong_dtypes():
    import torch
    from soar_amd.png import encode_png, save_png, write_png_files
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encode_png(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        save_png("unused.png", torch.zeros((8, 8, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        write_png_files(["unused.png"], torch.zeros((1, 8, 8), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        encode_png(np.zeros((1, 8, 8, 3), np.uint8))
    with pytest.raises(ValueError, match="paths"):
        write_png_files(["a.png", "b.png"], torch.zeros((1, 8, 8), dtype=torch.uint8))


def test_png_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes as C
    from soar_amd import build, hip_lib
    build.build()
    lib = hip_lib.lib()
    a = hip_lib.SoarPngArgs()
    a.B, a.H, a.W, a.channels, a.filter, a.piece_bytes = 1, 16, 16, 3, -1, 64
    n = C.c_size_t(0)
    assert lib.soar_png_workspace_bytes(C.byref(a), C.byref(n)) == 0
    assert n.value % 256 == 0 and n.value >= 16 * 49 + 13 * 286                  # the filtered stream, and 13 pieces' code lengths
    assert lib.soar_png_workspace_bytes(C.byref(a), None) != 0 and "NULL" in hip_lib.last_error()
    assert lib.soar_png_workspace_bytes(None, C.byref(n)) != 0 and "NULL" in hip_lib.last_error()
    for field, bad in (("channels", 2), ("channels", 0), ("channels", 5), ("piece_bytes", 31), ("piece_bytes", 65536), ("H", 0), ("W", 65536),
                       ("filter", 5), ("filter", -2), ("B", -1)):
        keep = getattr(a, field)
        setattr(a, field, bad)
        assert lib.soar_png_workspace_bytes(C.byref(a), C.byref(n)) != 0 and "bad arguments" in hip_lib.last_error(), field
        assert lib.soar_png_measure(C.byref(a), 0x1000, 1 << 20, 0x1000, None) != 0, field
        assert lib.soar_png_emit(C.byref(a), 0x1000, 1 << 20, 0x1000, 100, None) != 0, field
        setattr(a, field, keep)
    assert lib.soar_png_measure(C.byref(a), None, 0, 0x1000, None) != 0 and "workspace" in hip_lib.last_error()
    assert lib.soar_png_measure(C.byref(a), 0x1000, 16, 0x1000, None) != 0 and "workspace" in hip_lib.last_error()       # short
    assert lib.soar_png_measure(C.byref(a), 0x1000, 1 << 20, None, None) != 0 and "offsets" in hip_lib.last_error()
    assert lib.soar_png_measure(C.byref(a), 0x1000, 1 << 20, 0x1000, None) != 0 and "images" in hip_lib.last_error()
    assert lib.soar_png_emit(C.byref(a), None, 1 << 20, 0x1000, 100, None) != 0 and "workspace" in hip_lib.last_error()
    assert lib.soar_png_emit(C.byref(a), 0x1000, 16, 0x1000, 100, None) != 0 and "workspace" in hip_lib.last_error()
    assert lib.soar_png_emit(C.byref(a), 0x1000, 1 << 20, None, 100, None) != 0 and "capacity" in hip_lib.last_error()
    assert lib.soar_png_emit(C.byref(a), 0x1000, 1 << 20, 0x1000, -1, None) != 0 and "capacity" in hip_lib.last_error()
