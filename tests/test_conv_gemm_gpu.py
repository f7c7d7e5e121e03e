"""GPU tests of the shared implicit-GEMM convolution and the weight packer by themselves (csrc/conv_gemm.hip), through
soar_selftest_conv_gemm / soar_selftest_conv_pack, against the float64 restatement of tests/conv_gemm_ref.py.

Exact oracle: x, w and res are integers in -2 .. 2, bias multiples of 0.25, alpha 1 or 0.5, K <= 360: every product and partial sum
is an integer below 2^24, so the float32 result is exact whatever the order of summation, and the comparison has no tolerance.
Guards: x and w lie in NaN (between rows, images, channels, behind Cout), y in a canary; everything is allocated, so a gather out
of bounds is a NaN in the output and a stray write a dead canary, not a fault."""
import ctypes as C
from dataclasses import replace

import pytest
import torch

import conv_gemm_ref as ref
from soar_amd import hip_lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(dev, *shape, seed):
    return torch.randint(-2, 3, shape, generator=_gen(seed)).float().to(dev)


def _quarters(dev, n, seed):
    return (torch.randint(-8, 9, (n,), generator=_gen(seed)).float() * 0.25).to(dev)


def _normal(dev, *shape, seed):
    return torch.randn(*shape, generator=_gen(seed)).to(dev)


def _launch(b, d=None, y=None):
    """runs descriptor d (default: the case's) over the case's buffers into y (default: the case's); returns the tile size"""
    d = b.d if d is None else d
    y = b.y if y is None else y
    a = ref.c_args(d, b.x.data_ptr(), b.w.data_ptr(), None if b.bias is None else b.bias.data_ptr(),
                   None if b.res is None else b.res.data_ptr(), y.data_ptr())
    tile = C.c_int32(0)
    hip_lib.check(hip_lib.lib().soar_selftest_conv_gemm(C.byref(a), C.byref(tile), torch.cuda.current_stream().cuda_stream),
                  "selftest_conv_gemm")
    return tile.value


def _bits(t):
    return t.view(torch.int32)


def _exact(b, tile=64, layouts=(0, 1)):
    """the case under both tile geometries: every written element equals the restatement, everything else is the canary, bit for bit"""
    want, written = ref.expected(b)
    assert bool(torch.isfinite(want).all())
    for per_image in layouts:
        if b.d.wbat and not per_image:
            continue
        y = torch.full_like(b.y, ref.CANARY)
        got_tile = _launch(b, replace(b.d, per_image=per_image), y)
        assert got_tile == (64 if per_image else tile)
        assert torch.equal(_bits(y[~written]), _bits(b.y[~written])), "the canary around the output died"
        assert torch.equal(y.double(), want), f"per_image={per_image}: {(y.double() != want).sum().item()} elements differ"
    return want, written


def _extras(dev, d, kind, seed):
    """kind: none / bias / res / all (all: alpha = 0.5 too)"""
    bias = _quarters(dev, d.Cout, seed) if kind in ("bias", "all") else None
    res = _ints(dev, d.N, d.Hout, d.Wout, d.Cout, seed=seed + 1) if kind in ("res", "all") else None
    if kind == "all":
        d.alpha = 0.5
    return dict(bias=bias, res=res)


def _square(N, H, W, Cin, Cout, side):
    """side x side taps around the pixel, zero padding"""
    return ref._grid(N, H, W, H, W, Cin, Cout, [ref.square_taps(side, -(side // 2))])


# M = N H W rows, Cout, Cin, the kernel's side (Kp = side^2 Cin: 8, 32, 72, 216, 360 and 40, 96), the epilogue
TILE_EDGES = [
    ((1, 1, 1), 1, 8, 1, "none"),
    ((3, 3, 7), 63, 8, 2, "bias"),
    ((2, 4, 8), 64, 8, 3, "res"),
    ((1, 5, 13), 65, 24, 3, "all"),
    ((3, 1, 43), 130, 40, 3, "all"),
    ((1, 1, 1), 130, 40, 3, "bias"),
    ((1, 3, 43), 1, 8, 2, "res"),
    ((1, 7, 9), 64, 24, 3, "none"),
    ((1, 8, 8), 65, 40, 3, "none"),
    ((5, 1, 13), 63, 8, 3, "bias"),
    ((3, 43, 1), 64, 8, 1, "all"),
    ((2, 4, 8), 130, 24, 2, "res"),
    ((1, 13, 5), 1, 40, 1, "none"),
]
assert {n * h * w for (n, h, w), *_ in TILE_EDGES} == {1, 63, 64, 65, 129}
assert {c for _, c, *_ in TILE_EDGES} == {1, 63, 64, 65, 130}
assert {8, 32, 72, 216, 360} <= {s * s * c for _, _, c, s, _ in TILE_EDGES}
assert {k for *_, k in TILE_EDGES} == {"none", "bias", "res", "all"}


@pytest.mark.parametrize("i", range(len(TILE_EDGES)))
def test_tile_edges_at_64(i, dev):
    (N, H, W), Cout, Cin, side, kind = TILE_EDGES[i]
    d = _square(N, H, W, Cin, Cout, side)
    b = ref.guarded(d, _ints(dev, N, H, W, Cin, seed=10 * i), [_ints(dev, Cout, side * side, Cin, seed=10 * i + 1)], **_extras(dev, d, kind, 10 * i + 2))
    _exact(b)


def test_flat_rows_cross_images(dev):
    """N = 3, 5 x 10: the first tile of 64 flat rows ends 14 rows into the second image"""
    d = ref.conv3x3(3, 5, 10, 8, 8)
    b = ref.guarded(d, _ints(dev, 3, 5, 10, 8, seed=200), [_ints(dev, 8, 9, 8, seed=201)], **_extras(dev, d, "all", 202))
    _exact(b)


@pytest.mark.parametrize("form", ["conv", "matmul"])
def test_per_image_tiles_with_b_per_image(form, dev):
    """N = 3, 70 rows an image: two tiles and a 6-row tail each; a different B for every image (wbat); Cout = 72: a second column tile"""
    if form == "conv":
        d = replace(ref.conv3x3(3, 7, 10, 8, 72), per_image=1)
        x, w, wide = _ints(dev, 3, 7, 10, 8, seed=210), _ints(dev, 3, 72, 9, 8, seed=211), 0
    else:
        # x: the columns 24 .. 48 of rows of 76 floats, as the attention reads a slice of its [T][3 C] buffer
        d = ref.matmul(3, 70, 24, 72)
        x, w, wide = _ints(dev, 3, 1, 70, 24, seed=212), _ints(dev, 3, 72, 1, 24, seed=213), 24
    b = ref.guarded(d, x, [w], x_wide=wide, **_extras(dev, d, "all", 214))
    assert b.d.wbat > 0 and (not wide or b.d.ldx == 76)
    _exact(b)
    # the images' B do differ: image 1 with image 0's B is another result
    assert not torch.equal(w[0], w[1])


@pytest.mark.parametrize("H,W,stride", [(2, 2, 1), (3, 5, 1), (6, 4, 2)])
def test_reflect(H, W, stride, dev):
    d = ref.conv3x3_reflect(2, H, W, 8, 8, stride=stride)
    b = ref.guarded(d, _ints(dev, 2, H, W, 8, seed=220), [_ints(dev, 8, 9, 8, seed=221)], **_extras(dev, d, "bias", 222))
    _exact(b)


@pytest.mark.parametrize("builder,H,W", [("conv3x3_stride2", 5, 7), ("conv3x3_stride2_rb", 6, 6), ("conv3x3_stride2_rb", 7, 5)])
def test_zero_padding_with_stride_2(builder, H, W, dev):
    d = getattr(ref, builder)(2, H, W, 8, 8)
    b = ref.guarded(d, _ints(dev, 2, H, W, 8, seed=230), [_ints(dev, 8, 9, 8, seed=231)], **_extras(dev, d, "res", 232))
    _exact(b)


@pytest.mark.parametrize("H,W", [(2, 2), (6, 8), (7, 9), (10, 4), (11, 5)])
def test_dilated_data_gradient(H, W, dev):
    """the stride-2 convolution's data gradient over an H x W input, from a gradient of 1 x 1, 3 x 4 and 5 x 2: per image and flat"""
    d = ref.conv3x3_stride2_rb_grad(2, H, W, 8, 16)
    assert (d.Hin, d.Win) in ((1, 1), (3, 4), (5, 2)) and d.dil == 2
    b = ref.guarded(d, _ints(dev, 2, d.Hin, d.Win, 16, seed=240), [_ints(dev, 8, 9, 16, seed=241)])
    _exact(b)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8)])
def test_four_phases(H, W, dev):
    d = ref.conv_transpose_phases(2, H, W, 8, 8)
    ws = [_ints(dev, 8, t.ntaps, 8, seed=250 + p) for p, t in enumerate(d.ph)]
    b = ref.guarded(d, _ints(dev, 2, H, W, 8, seed=255), ws, **_extras(dev, d, "all", 256))
    _exact(b)


@pytest.mark.parametrize("p", range(4))
def test_one_phase_alone_leaves_the_other_parities(p, dev):
    full = ref.conv_transpose_phases(2, 3, 5, 8, 8)
    d = replace(full, ph=[full.ph[p]])
    b = ref.guarded(d, _ints(dev, 2, 3, 5, 8, seed=260), [_ints(dev, 8, d.ph[0].ntaps, 8, seed=261 + p)], **_extras(dev, d, "bias", 265))
    _, written = _exact(b)
    seen = ref.logical(b.d, written)[..., 0]
    for py in (0, 1):
        for px in (0, 1):
            assert bool(seen[:, py::2, px::2].all()) == ((py, px) == (p >> 1, p & 1)) and bool(seen[:, py::2, px::2].any()) == ((py, px) == (p >> 1, p & 1))


# ---- the 128 x 128 tile: N = 2, 91 x 90, Cin = 24, Cout = 136: M = 16380 = 127 x 128 + 124 rows, two column tiles, the second of 8 ----
BIG = dict(N=2, H=91, W=90, Cin=24, Cout=136)
_cache = {}


def _big_desc(form):
    N, H, W, Cin, Cout = BIG.values()
    return {"zero": ref.conv3x3, "reflect": ref.conv3x3_reflect, "phases": ref.conv_transpose_phases}[form](N, H, W, Cin, Cout)


def _big(form, real, dev):
    """the case, laid out once and left unchanged"""
    if (form, real) not in _cache:
        d = _big_desc(form)
        draw = _normal if real else _ints
        ws = [draw(dev, d.Cout, t.ntaps, d.Cin, seed=300 + p) for p, t in enumerate(d.ph)]
        bias = _normal(dev, d.Cout, seed=310) if real else _quarters(dev, d.Cout, 310)
        res = draw(dev, d.N, d.Hout, d.Wout, d.Cout, seed=311)
        d.alpha = 0.5
        _cache[form, real] = ref.guarded(d, draw(dev, d.N, d.Hin, d.Win, d.Cin, seed=312), ws, bias=bias, res=res)
    return _cache[form, real]


def _single(b, n):
    """image n of the case by itself, over the same buffers"""
    return replace(b.d, N=1, x_off=b.d.x_off + n * b.d.xim * b.d.ldx, y_off=b.d.y_off + n * b.d.yim * b.d.ldy)


@pytest.mark.parametrize("form", ["zero", "reflect", "phases"])
def test_tile_128_exact(form, dev):
    b = _big(form, False, dev)
    assert b.d.N * b.d.Hg * b.d.Wg == 127 * 128 + 124 and b.d.Cout == 128 + 8
    _exact(b, tile=128)
    if form != "phases":
        # one image alone is 64 x 2 tiles of 128: under 256, so the launcher falls back to 64 (four phases still make 512)
        for n in (0, 1):
            assert _launch(b, _single(b, n), torch.full_like(b.y, ref.CANARY)) == 64


@pytest.mark.parametrize("form", ["zero", "reflect"])
def test_order_of_summation_is_the_tiles_and_the_batchs(form, dev):
    """conv_gemm.h: "the sums' order is the same".  Real inputs: the batch at 128 x 128 tiles, its images alone at 64 x 64, the tiles
    per image and a second run agree bit for bit."""
    b = _big(form, True, dev)
    y = torch.full_like(b.y, ref.CANARY)
    assert _launch(b, y=y) == 128
    again = torch.full_like(b.y, ref.CANARY)
    assert _launch(b, y=again) == 128
    assert torch.equal(_bits(again), _bits(y))
    alone = torch.full_like(b.y, ref.CANARY)
    for n in (0, 1):
        assert _launch(b, _single(b, n), alone) == 64
    assert torch.equal(_bits(alone), _bits(y))
    per = torch.full_like(b.y, ref.CANARY)
    assert _launch(b, replace(b.d, per_image=1), per) == 64
    assert torch.equal(_bits(per), _bits(y))


@pytest.mark.parametrize("form", ["zero", "reflect", "phases"])
def test_real_numbers_within_the_summation_bound(form, dev):
    """Every element within (K + 4) 2^-23 (|alpha| sum |a||w| + |bias| + |res|) of float64: the any-order summation bound
    of K products, K - 1 additions and the epilogue's three operations at unit roundoff 2^-24, doubled because the rounding inside
    the MFMA's two-term step is unspecified.  Derived, not measured; at both tile sizes."""
    b = _big(form, True, dev)
    want, written = ref.expected(b)
    scale, _, K = ref.expected(b, absolute=True, with_k=True)
    assert sorted(set(K[written].tolist())) == ([216] if form != "phases" else [24, 48, 96])
    bound = (K + 4) * 2.0 ** -23 * scale
    for per_image, tile in ((0, 128), (1, 64)):
        y = torch.full_like(b.y, ref.CANARY)
        assert _launch(b, replace(b.d, per_image=per_image), y) == tile
        assert torch.equal(_bits(y[~written]), _bits(b.y[~written]))
        err = (y.double() - want)[written].abs()
        ratio = (err / bound[written]).max().item()
        print(f"conv_gemm {form} tile {tile}: worst |error| {err.max().item():.3e}, worst ratio to the bound {ratio:.4f}")
        assert bool(torch.isfinite(y[written]).all()) and ratio <= 1.0


# ---- the packer ----
@pytest.mark.parametrize("Cout,Cin,kk", [(3, 8, 49), (72, 24, 9), (130, 40, 1), (64, 3, 9)])
def test_packer(Cout, Cin, kk, dev):
    n = Cout * Cin * kk
    assert n % 256 != 0 and n > 256                     # whole blocks and a part of one
    w = _normal(dev, Cout, Cin, kk, seed=400)
    ldb = Cout + 3
    fwd = torch.full((n + 64,), ref.CANARY, device=dev)
    bwd = torch.full((Cin * kk * ldb + 64,), ref.CANARY, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    hip_lib.check(hip_lib.lib().soar_selftest_conv_pack(w.data_ptr(), fwd.data_ptr(), bwd.data_ptr(), Cout, Cin, kk, ldb, stream), "conv_pack")
    assert torch.equal(fwd[:n].view(Cout, kk, Cin), w.permute(0, 2, 1))
    assert torch.equal(fwd[:n].view(Cout, kk, Cin), ref.pack_fwd(w))
    assert bool((fwd[n:] == ref.CANARY).all())
    want = ref.pack_bwd(w, ldb=ldb, fill=ref.CANARY)    # the columns behind Cout: untouched
    assert torch.equal(want[:, :, :Cout], w.flip(2).permute(1, 2, 0))
    assert torch.equal(_bits(bwd[:Cin * kk * ldb].view(Cin, kk, ldb)), _bits(want))
    assert bool((bwd[Cin * kk * ldb:] == ref.CANARY).all())
    # without bwd
    fwd2 = torch.full_like(fwd, ref.CANARY)
    hip_lib.check(hip_lib.lib().soar_selftest_conv_pack(w.data_ptr(), fwd2.data_ptr(), None, Cout, Cin, kk, 0, stream), "conv_pack")
    assert torch.equal(_bits(fwd2), _bits(fwd))
