"""GPU tests of the shared implicit-GEMM convolution with 16-bit operands and of its weight packer (csrc/conv_gemm.hip
conv_gemm16_kernel / conv_pack16_kernel), through soar_selftest_conv_gemm16 / soar_selftest_conv_pack16, against the
float64 restatement of tests/conv_gemm_ref.py.  Every case runs at bf16 and at f16.

Exact oracle: the float32 tests' (tests/test_conv_gemm_gpu.py).  x, w and res are integers in -2 .. 2, bias multiples of 0.25, alpha
1 or 0.5, K <= 360: every operand is exact in both 16-bit types, every product and partial sum an integer below 2^24, so the result
is exact whatever the order of summation and the comparison has no tolerance.
Guards: conv_gemm_ref's buffers (x in NaN, y in a canary).  B is packed by soar_selftest_conv_pack16 and laid into a 16-bit buffer
of NaN of its own (8 NaN elements in front, 8 behind every row, 3 NaN rows behind Cout): the float32 layout's pitches are no
multiples of 8.  Everything is allocated, so a gather out of bounds is a NaN in the output and a stray write a dead canary."""
import ctypes as C
from dataclasses import dataclass, replace
from typing import List, Tuple

import pytest
import torch

import conv_gemm_ref as ref
from soar_amd import hip_lib

pytestmark = pytest.mark.gpu

TYPES = {"bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}
PRECS = ["bf16", "f16"]


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


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pack16(w, Cinp, prec):
    """torch [Cout][Cin][kk] float32 -> the packer's [Cout][kk][Cinp] of the type"""
    Cout, Cin, kk = w.shape
    out = torch.empty((Cout, kk, Cinp), dtype=TYPES[prec][1], device=w.device)
    w = w.contiguous()
    hip_lib.check(hip_lib.lib().soar_selftest_conv_pack16(w.data_ptr(), out.data_ptr(), Cout, Cin, Cinp, kk, TYPES[prec][0], _stream()),
                  "selftest_conv_pack16")
    return out


@dataclass
class HalfW:
    """a case's B as the kernel's 16-bit values: the flat NaN-guarded buffer, every tap table's (offset, ldw) in elements, wbat"""
    buf: torch.Tensor
    tabs: List[Tuple[int, int]]
    wbat: int
    wtype: int


def _half_w(b, ws, prec):
    """ws as conv_gemm_ref.guarded took them ([Cout][ntaps][Cin] or [N][Cout][ntaps][Cin] per tap table), packed on the device"""
    wtype, dt = TYPES[prec]
    dev = b.x.device
    nan = float("nan")
    parts, off, tabs, wbat = [], 8, [], 0
    for w in ws:
        w = w if w.dim() == 4 else w[None]
        B, Cout, nt, Cin = w.shape
        packed = _pack16(w.reshape(B * Cout, nt, Cin).permute(0, 2, 1).contiguous(), Cin, prec)
        ldw = nt * Cin + 8
        blk = torch.full((B, Cout + 3, ldw), nan, dtype=dt, device=dev)
        blk[:, :Cout, :nt * Cin] = packed.view(B, Cout, nt * Cin)
        tabs.append((off, ldw))
        if B > 1:
            wbat = (Cout + 3) * ldw
        parts.append(blk.reshape(-1))
        off += blk.numel()
    return HalfW(torch.cat([torch.full((8,), nan, dtype=dt, device=dev)] + parts), tabs, wbat, wtype)


def _launch(b, hw, d=None, y=None):
    """runs descriptor d (default: the case's) with B = hw into y (default: the case's); returns the tile size"""
    d = b.d if d is None else d
    y = b.y if y is None else y
    a = ref.c_args(d, b.x.data_ptr(), b.w.data_ptr(), None if b.bias is None else b.bias.data_ptr(),
                   None if b.res is None else b.res.data_ptr(), y.data_ptr())
    a.wbat = hw.wbat if d.wbat else 0
    for p, (off, ldw) in enumerate(hw.tabs[:d.nph]):
        a.ph[p].w, a.ph[p].ldw = hw.buf.data_ptr() + 2 * off, ldw
    tile = C.c_int32(0)
    hip_lib.check(hip_lib.lib().soar_selftest_conv_gemm16(C.byref(a), hw.wtype, C.byref(tile), _stream()), "selftest_conv_gemm16")
    return tile.value


def _exact(b, ws, prec, tile=64, layouts=(0, 1)):
    """the case under both tile geometries: every written element equals the restatement, everything else is the canary, bit for bit"""
    want, written = ref.expected(b)
    assert bool(torch.isfinite(want).all())
    hw = _half_w(b, ws, prec)
    for per_image in layouts:
        if b.d.wbat and not per_image:
            continue
        y = torch.full_like(b.y, ref.CANARY)
        got_tile = _launch(b, hw, replace(b.d, per_image=per_image), y)
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
    return ref._grid(N, H, W, H, W, Cin, Cout, [ref.square_taps(side, -(side // 2))])


# M = N H W rows, Cout, Cin, the kernel's side (Kp = side^2 Cin: 8, 32, 72, 216, 360 and 40, 96), the epilogue: the float32 test's list.
# Kp = 8 is shorter than one MFMA step of 16, 40 / 72 / 216 / 360 end inside a step, 32 and 96 inside a chunk of 64
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
assert {8, 32, 40, 72, 96, 216, 360} <= {s * s * c for _, _, c, s, _ in TILE_EDGES}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("i", range(len(TILE_EDGES)))
def test_tile_edges_at_64(i, prec, dev):
    (N, H, W), Cout, Cin, side, kind = TILE_EDGES[i]
    d = _square(N, H, W, Cin, Cout, side)
    ws = [_ints(dev, Cout, side * side, Cin, seed=10 * i + 1)]
    b = ref.guarded(d, _ints(dev, N, H, W, Cin, seed=10 * i), ws, **_extras(dev, d, kind, 10 * i + 2))
    _exact(b, ws, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_flat_rows_cross_images(prec, dev):
    """N = 3, 5 x 10: the first tile of 64 flat rows ends 14 rows into the second image"""
    d = ref.conv3x3(3, 5, 10, 8, 8)
    ws = [_ints(dev, 8, 9, 8, seed=201)]
    b = ref.guarded(d, _ints(dev, 3, 5, 10, 8, seed=200), ws, **_extras(dev, d, "all", 202))
    _exact(b, ws, prec)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("form", ["conv", "matmul"])
def test_per_image_tiles_with_b_per_image(form, prec, dev):
    """N = 3, 70 rows an image; a different B for every image (wbat); the matmul's x is a slice of wider rows (ldx = 76, x_wide = 24)"""
    if form == "conv":
        d = replace(ref.conv3x3(3, 7, 10, 8, 72), per_image=1)
        x, w, wide = _ints(dev, 3, 7, 10, 8, seed=210), _ints(dev, 3, 72, 9, 8, seed=211), 0
    else:
        d = ref.matmul(3, 70, 24, 72)
        x, w, wide = _ints(dev, 3, 1, 70, 24, seed=212), _ints(dev, 3, 72, 1, 24, seed=213), 24
    b = ref.guarded(d, x, [w], x_wide=wide, **_extras(dev, d, "all", 214))
    assert b.d.wbat > 0 and (not wide or b.d.ldx == 76)
    _exact(b, [w], prec)
    assert not torch.equal(w[0], w[1])


@pytest.mark.parametrize("prec", PRECS)
def test_stride_2(prec, dev):
    d = ref.conv3x3_stride2(2, 5, 7, 8, 8)
    ws = [_ints(dev, 8, 9, 8, seed=231)]
    b = ref.guarded(d, _ints(dev, 2, 5, 7, 8, seed=230), ws, **_extras(dev, d, "res", 232))
    _exact(b, ws, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_reflect(prec, dev):
    d = ref.conv3x3_reflect(2, 3, 5, 8, 8)
    ws = [_ints(dev, 8, 9, 8, seed=221)]
    b = ref.guarded(d, _ints(dev, 2, 3, 5, 8, seed=220), ws, **_extras(dev, d, "bias", 222))
    _exact(b, ws, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_four_phases(prec, dev):
    d = ref.conv_transpose_phases(2, 3, 5, 8, 8)
    ws = [_ints(dev, 8, t.ntaps, 8, seed=250 + p) for p, t in enumerate(d.ph)]
    b = ref.guarded(d, _ints(dev, 2, 3, 5, 8, seed=255), ws, **_extras(dev, d, "all", 256))
    _exact(b, ws, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_dilation_2(prec, dev):
    d = ref.conv3x3_stride2_rb_grad(2, 7, 9, 8, 16)
    assert d.dil == 2
    ws = [_ints(dev, 8, 9, 16, seed=241)]
    b = ref.guarded(d, _ints(dev, 2, d.Hin, d.Win, 16, seed=240), ws)
    _exact(b, ws, prec)


@pytest.mark.parametrize("prec", PRECS)
def test_three_table_row_split(prec, dev):
    """unet.hip's conv3x3 at its small sizes: the 3 x 3 kernel's rows as three tap tables of three taps, their results at the
    parities (0, 0), (0, 1), (1, 0) of an output twice the grid (os = 2, nph = 3); parity (1, 1) stays canary"""
    N, H, W, Cin, Cout = 2, 4, 6, 24, 40
    ph = [ref.Taps([r - 1] * 3, [-1, 0, 1], py=r >> 1, px=r & 1) for r in range(3)]
    d = ref._grid(N, H, W, H, W, Cin, Cout, ph, os=2)
    w9 = _ints(dev, Cout, 9, Cin, seed=271)
    ws = [w9[:, 3 * r:3 * r + 3].contiguous() for r in range(3)]
    b = ref.guarded(d, _ints(dev, N, H, W, Cin, seed=270), ws)
    _, written = _exact(b, ws, prec)
    seen = ref.logical(b.d, written)[..., 0]
    assert bool(seen[:, 0::2, 0::2].all()) and bool(seen[:, 0::2, 1::2].all()) and bool(seen[:, 1::2, 0::2].all())
    assert not bool(seen[:, 1::2, 1::2].any())
    # the three parities sum to the whole 3 x 3 convolution
    whole = ref.conv3x3(N, H, W, Cin, Cout)
    bw = ref.guarded(whole, _ints(dev, N, H, W, Cin, seed=270), [w9])
    want, _ = ref.expected(bw)
    y = torch.full_like(b.y, ref.CANARY)
    _launch(b, _half_w(b, ws, prec), y=y)
    parts = ref.logical(b.d, y).double()
    assert torch.equal(parts[:, 0::2, 0::2] + parts[:, 0::2, 1::2] + parts[:, 1::2, 0::2], ref.logical(bw.d, want))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("act", [1, 2])
def test_activations(act, prec, dev):
    """y = act(alpha acc + bias) + res with act = GELU (exact, erf) and ReLU, through soar_selftest_conv_gemm_act (SoarConvGemmArgs has
    no act).  Integer data: the pre-activation v is exact, so ReLU equals the restatement exactly; both equal the float32 kernel's
    bits (the epilogue is one function); GELU lies within 2^-21 (|v| + 1) + 2^-23 |y| of float64: erff's 2 ulp of a value up to 1,
    the argument's, the sum's and the two products' roundings come to under 2^-22 |v| + 2^-23, doubled, and the sum with res rounds
    once more."""
    d = _square(2, 5, 7, 24, 65, 3)
    ws = [_ints(dev, 65, 9, 24, seed=281)]
    b = ref.guarded(d, _ints(dev, 2, 5, 7, 24, seed=280), ws, **_extras(dev, d, "all", 282))
    hw = _half_w(b, ws, prec)

    def run(wtype):
        y = torch.full_like(b.y, ref.CANARY)
        a = ref.c_args(b.d, b.x.data_ptr(), b.w.data_ptr(), b.bias.data_ptr(), b.res.data_ptr(), y.data_ptr())
        if wtype:
            for p, (off, ldw) in enumerate(hw.tabs):
                a.ph[p].w, a.ph[p].ldw = hw.buf.data_ptr() + 2 * off, ldw
        tile = C.c_int32(0)
        hip_lib.check(hip_lib.lib().soar_selftest_conv_gemm_act(C.byref(a), wtype, act, C.byref(tile), _stream()), "selftest_conv_gemm_act")
        return y

    y = run(hw.wtype)
    assert torch.equal(_bits(y), _bits(run(0)))
    # v from the restatement without res; then the activation and res in float64
    pre, written = ref.expected(replace(b, res=None))
    res = b.res.double()
    v = pre[written]
    if act == 2:
        assert torch.equal(y.double()[written], v.clamp(min=0) + res[written])
    else:
        want = 0.5 * v * (1 + torch.erf(v * 0.5 ** 0.5)) + res[written]
        err = (y.double()[written] - want).abs()
        bound = 2.0 ** -21 * (v.abs() + 1) + 2.0 ** -23 * want.abs()
        print(f"conv_gemm16 {prec} GELU: worst ratio to the bound {(err / bound).max().item():.4f}")
        assert bool((err <= bound).all())
    assert torch.equal(_bits(y[~written]), _bits(b.y[~written]))


# ---- the 128 x 128 tile: the float32 test's case.  M = 16380 = 127 x 128 + 124 rows, two column tiles, the second of 8 ----
BIG = dict(N=2, H=91, W=90, Cin=24, Cout=136)
_cache = {}


def _big(real, dev):
    """the case, laid out once and left unchanged: (buffers, the tap tables' weights)"""
    if real not in _cache:
        N, H, W, Cin, Cout = BIG.values()
        d = ref.conv3x3(N, H, W, Cin, Cout)
        draw = _normal if real else _ints
        ws = [draw(dev, d.Cout, 9, d.Cin, seed=300)]
        bias = _normal(dev, d.Cout, seed=310) if real else _quarters(dev, d.Cout, 310)
        res = draw(dev, d.N, d.Hout, d.Wout, d.Cout, seed=311)
        d.alpha = 0.5
        x = draw(dev, d.N, d.Hin, d.Win, d.Cin, seed=312)
        _cache[real] = (ref.guarded(d, x, ws, bias=bias, res=res), ws, x, bias, res)
    return _cache[real]


def _single(b, n):
    return replace(b.d, N=1, x_off=b.d.x_off + n * b.d.xim * b.d.ldx, y_off=b.d.y_off + n * b.d.yim * b.d.ldy)


@pytest.mark.parametrize("prec", PRECS)
def test_tile_128_exact(prec, dev):
    b, ws, *_ = _big(False, dev)
    # 128 row tiles times two column tiles: the 256 tiles of 128 x 128 at which conv_gemm_tile returns 128 (_exact asserts it)
    assert b.d.N * b.d.Hg * b.d.Wg == 127 * 128 + 124 and b.d.Cout == 128 + 8
    _exact(b, ws, prec, tile=128)


@pytest.mark.parametrize("prec", PRECS)
def test_real_numbers_within_the_summation_bound(prec, dev):
    """The 216-long case with normal data: every element within (K + 4) 2^-23 (|alpha| sum |a||w| + |bias| + |res|) of the float64
    restatement over the operands rounded to the type (by torch, here): the float32 test's derived bound, one whole ulp per addition,
    so an adder that truncates inside the instruction is covered.  At both tile sizes."""
    b, ws, x, bias, res = _big(True, dev)
    dt = TYPES[prec][1]
    rounded = ref.guarded(replace(b.d), x.to(dt).float(), [ws[0].to(dt).float()], bias=bias, res=res)
    want, written = ref.expected(rounded)
    scale, _, K = ref.expected(rounded, absolute=True, with_k=True)
    assert sorted(set(K[written].tolist())) == [216]
    bound = (K + 4) * 2.0 ** -23 * scale
    hw = _half_w(b, ws, prec)
    for per_image, tile in ((0, 128), (1, 64)):
        y = torch.full_like(b.y, ref.CANARY)
        assert _launch(b, hw, replace(b.d, per_image=per_image), y) == tile
        assert torch.equal(_bits(y[~written]), _bits(b.y[~written]))
        err = (y.double() - want)[written].abs()
        ratio = (err / bound[written]).max().item()
        print(f"conv_gemm16 {prec} tile {tile}: worst |error| {err.max().item():.3e}, worst ratio to the bound {ratio:.4f}")
        assert bool(torch.isfinite(y[written]).all()) and ratio <= 1.0


@pytest.mark.parametrize("prec", PRECS)
def test_runs_tiles_and_batches_agree_and_f32_is_untouched(prec, dev):
    """Real inputs: the batch at 128 x 128 tiles twice, its images alone at 64 x 64 and the tiles per image agree bit for bit.  The
    float32 entry point still gives its exact result on the integer case in the same process, and differs from the 16-bit result on
    the real one."""
    b, ws, *_ = _big(True, dev)
    hw = _half_w(b, ws, prec)
    y = torch.full_like(b.y, ref.CANARY)
    assert _launch(b, hw, y=y) == 128
    again = torch.full_like(b.y, ref.CANARY)
    assert _launch(b, hw, y=again) == 128
    assert torch.equal(_bits(again), _bits(y))
    alone = torch.full_like(b.y, ref.CANARY)
    for n in (0, 1):
        assert _launch(b, hw, _single(b, n), alone) == 64
    assert torch.equal(_bits(alone), _bits(y))
    per = torch.full_like(b.y, ref.CANARY)
    assert _launch(b, hw, replace(b.d, per_image=1), per) == 64
    assert torch.equal(_bits(per), _bits(y))

    def f32(case):
        out = torch.full_like(case.y, ref.CANARY)
        a = ref.c_args(case.d, case.x.data_ptr(), case.w.data_ptr(), case.bias.data_ptr(), case.res.data_ptr(), out.data_ptr())
        tile = C.c_int32(0)
        hip_lib.check(hip_lib.lib().soar_selftest_conv_gemm(C.byref(a), C.byref(tile), _stream()), "selftest_conv_gemm")
        return out, tile.value

    bi, *_ = _big(False, dev)
    want, _ = ref.expected(bi)
    got, tile = f32(bi)
    assert tile == 128 and torch.equal(got.double(), want)
    assert not torch.equal(_bits(f32(b)[0]), _bits(y))


# ---- the rounding rule ----
@pytest.mark.parametrize("prec", PRECS)
def test_a_is_rounded_to_nearest_even(prec, dev):
    """B = the identity (Cin = Cout = 64, one tap), x [130][64]: y must be x.to(type).float() bit for bit.  x: normals scaled over
    2^-10 .. 2^10, and hand-built ties at both signs and several exponents: 1 + u/2 (between an even mantissa below and an odd one
    above: rounds down), 1 + 3u/2 (odd below, even above: rounds up) with u the type's ulp at 1 (bf16 2^-7: 1 + 2^-8 and 1 + 3 2^-8;
    f16 2^-10), and their float32 neighbours on both sides.
    |x| stays inside the type's normal range: denormal and overflowing operands are not part of the contract."""
    dt = TYPES[prec][1]
    M, Cc = 130, 64
    g = _gen(500)
    n = torch.randn(M, Cc, generator=g)
    n = torch.where(n.abs() < 0.125, torch.full_like(n, 0.125), n)              # (2^-3 2^-10 is still a normal f16)
    x = n * torch.exp2(torch.rand(M, Cc, generator=g) * 20 - 10)
    u = 2.0 ** -7 if prec == "bf16" else 2.0 ** -10
    e = 2.0 ** -23
    ties = []
    for scale in (1.0, 2.0 ** -9, 2.0 ** 9, 2.0 ** -3, 2.0 ** 5):
        for m in (1 + u / 2, 1 + 3 * u / 2, 1 + 5 * u / 2, 1 + 7 * u / 2, 2 - u / 2, 1 + u / 2 + e, 1 + u / 2 - e, 1 + 3 * u / 2 + e,
                  1 + 3 * u / 2 - e, 1.0, 1 + u, 2 - u):
            ties += [m * scale, -m * scale]
    ties = torch.tensor(ties, dtype=torch.float64).float()
    x.view(-1)[:ties.numel()] = ties
    x.view(-1)[5000:5000 + ties.numel()] = ties                  # a second copy: other lanes, rows and a later tile
    x = x.to(dev)
    tiny, big = torch.finfo(dt).tiny, torch.finfo(dt).max
    assert bool(((x.abs() >= tiny) & (x.abs() < big / 2)).all())
    d = ref._grid(1, 1, M, 1, M, Cc, Cc, [ref.square_taps(1, 0)])
    ws = [torch.eye(Cc, device=dev).view(Cc, 1, Cc)]
    b = ref.guarded(d, x.view(1, 1, M, Cc), ws)
    y = torch.full_like(b.y, ref.CANARY)
    _launch(b, _half_w(b, ws, prec), y=y)
    got = ref.logical(b.d, y).view(M, Cc)
    want = x.to(dt).float()
    assert not torch.equal(want, x)
    assert torch.equal(_bits(got), _bits(want)), f"{(got != want).sum().item()} elements round differently"


# ---- the packer ----
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cout,Cin,Cinp,kk", [(3, 8, 16, 49), (71, 24, 32, 9), (130, 40, 48, 1), (65, 3, 8, 9)])
def test_packer(Cout, Cin, Cinp, kk, prec, dev):
    wtype, dt = TYPES[prec]
    n = Cout * kk * Cinp
    assert n % 256 != 0 and n > 256 and Cinp > Cin                # whole blocks and a part of one
    w = _normal(dev, Cout, Cin, kk, seed=400)
    w.view(-1)[:4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], device=dev)     # ties of both types
    canary = -2.5
    out = torch.full((n + 64,), canary, dtype=dt, device=dev)
    hip_lib.check(hip_lib.lib().soar_selftest_conv_pack16(w.data_ptr(), out.data_ptr(), Cout, Cin, Cinp, kk, wtype, _stream()), "conv_pack16")
    got = out[:n].view(Cout, kk, Cinp)
    assert torch.equal(_bits(got[:, :, :Cin]), _bits(w.to(dt).permute(0, 2, 1).contiguous()))
    assert bool((_bits(got[:, :, Cin:]) == 0).all())             # the pad: +0
    assert bool((out[n:] == canary).all())
