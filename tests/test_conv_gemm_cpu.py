"""CPU tests of the shared implicit-GEMM convolution (csrc/conv_gemm.h): the float64 restatement of its descriptor
(tests/conv_gemm_ref.py), the oracle of tests/test_conv_gemm_gpu.py, equals torch for every descriptor the networks build; and the
launcher refuses, before it launches anything, the descriptors the kernel cannot run (through soar_selftest_conv_gemm, with
addresses nothing ever reads)."""
import ctypes as C
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

import conv_gemm_ref as ref

# float64 against float64, sums of at most 360 terms of magnitude ~1 in two different orders: about 360 x 2^-53 x sum |terms| ~ 1e-12
# absolute at the very worst, relative to results of magnitude ~10
TOL = dict(rtol=1e-12, atol=1e-12)


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def _restated(d, x, ws, **kw):
    """the restatement over guarded buffers (NaN between rows, images and channels), as [N][Hout][Wout][Cout] in NCHW"""
    b = ref.guarded(d, x, ws, **kw)
    y, written = ref.expected(b)
    assert torch.equal(ref.logical(b.d, written), torch.ones(d.N, d.Hout, d.Wout, d.Cout, dtype=torch.bool))
    assert int(written.sum()) == d.N * d.Hout * d.Wout * d.Cout and bool((y[~written] == ref.CANARY).all())
    out = ref.logical(b.d, y)
    assert bool(torch.isfinite(out).all())
    return _nchw(out)


SIZES = [(5, 7), (6, 4), (2, 2), (1, 3)]


@pytest.mark.parametrize("H,W", SIZES)
def test_3x3_pad1_and_1x1_equal_conv2d(H, W):
    x, w, w1 = _rand(2, H, W, 8, seed=1), _rand(5, 8, 3, 3, seed=2), _rand(3, 8, 1, 1, seed=3)
    bias, res = _rand(5, seed=4), _rand(2, H, W, 5, seed=5)
    d = ref.conv3x3(2, H, W, 8, 5)
    d.alpha = 0.5
    got = _restated(d, x, [ref.pack_fwd(w)], bias=bias, res=res)
    want = 0.5 * F.conv2d(_nchw(x), w.double(), padding=1) + bias.double()[None, :, None, None] + _nchw(res)
    torch.testing.assert_close(got, want, **TOL)
    got = _restated(ref.conv1x1(2, H, W, 8, 3), x, [ref.pack_fwd(w1)])
    torch.testing.assert_close(got, F.conv2d(_nchw(x), w1.double()), **TOL)


@pytest.mark.parametrize("H,W", [(5, 7), (6, 6), (7, 5), (2, 3)])
def test_stride2_equals_conv2d(H, W):
    x, w = _rand(2, H, W, 16, seed=6), _rand(4, 16, 3, 3, seed=7)
    got = _restated(ref.conv3x3_stride2(2, H, W, 16, 4), x, [ref.pack_fwd(w)])
    torch.testing.assert_close(got, F.conv2d(_nchw(x), w.double(), stride=2, padding=1), **TOL)
    # the VAE's: zeros on the right and the bottom only
    got = _restated(ref.conv3x3_stride2_rb(2, H, W, 16, 4), x, [ref.pack_fwd(w)])
    torch.testing.assert_close(got, F.conv2d(F.pad(_nchw(x), (0, 1, 0, 1)), w.double(), stride=2), **TOL)


@pytest.mark.parametrize("H,W,stride", [(2, 2, 1), (3, 5, 1), (6, 4, 1), (6, 4, 2), (5, 7, 2)])
def test_reflect_equals_reflection_pad_and_conv2d(H, W, stride):
    x, w = _rand(2, H, W, 8, seed=8), _rand(6, 8, 3, 3, seed=9)
    got = _restated(ref.conv3x3_reflect(2, H, W, 8, 6, stride=stride), x, [ref.pack_fwd(w)])
    torch.testing.assert_close(got, F.conv2d(F.pad(_nchw(x), (1, 1, 1, 1), mode="reflect"), w.double(), stride=stride), **TOL)


def test_reflect_refuses_a_second_mirror():
    x, w = _rand(1, 1, 4, 8, seed=10), _rand(2, 8, 3, 3, seed=11)
    with pytest.raises(AssertionError, match="mirrors more than once"):
        _restated(ref.conv3x3_reflect(1, 1, 4, 8, 2), x, [ref.pack_fwd(w)])


@pytest.mark.parametrize("M", [1, 5, 8])
def test_per_image_matrix_product(M):
    x, B = _rand(2, 1, M, 24, seed=12), _rand(2, 7, 1, 24, seed=13)
    bias, res = _rand(7, seed=14), _rand(2, 1, M, 7, seed=15)
    d = ref.matmul(2, M, 24, 7)
    d.alpha = 0.25
    b = ref.guarded(d, x, [B], bias=bias, res=res, x_wide=24)
    assert b.d.wbat > 0 and b.d.ldx == 76 and b.d.x_off == 32
    y, _ = ref.expected(b)
    want = 0.25 * torch.matmul(x[:, 0].double(), B[:, :, 0].double().transpose(1, 2)) + bias.double() + res[:, 0].double()
    torch.testing.assert_close(ref.logical(b.d, y)[:, 0], want, **TOL)


@pytest.mark.parametrize("H,W", SIZES + [(8, 8)])
def test_four_phases_equal_conv_transpose2d(H, W):
    x, w = _rand(2, H, W, 8, seed=16), _rand(8, 5, 3, 3, seed=17)          # torch [Cin][Cout][3][3]
    d = ref.conv_transpose_phases(2, H, W, 8, 5)
    assert [t.ntaps for t in d.ph] == [1, 2, 2, 4] and (d.Hout, d.Wout) == (2 * H, 2 * W)
    got = _restated(d, x, ref.pack_transpose_phases(w))
    torch.testing.assert_close(got, F.conv_transpose2d(_nchw(x), w.double(), stride=2, padding=1, output_padding=1), **TOL)


@pytest.mark.parametrize("H,W", [(2, 2), (6, 8), (10, 4), (7, 9), (11, 5)])
def test_dilated_form_equals_the_stride2_data_gradient(H, W):
    """the VAE downsample's backward: a grid of the forward input's size over the output gradient, zero-dilated, packer's bwd weights"""
    w = _rand(16, 8, 3, 3, seed=18).double()                                 # forward: 8 -> 16 channels
    xin = _rand(2, 8, H, W, seed=19).double().requires_grad_(True)
    out = F.conv2d(F.pad(xin, (0, 1, 0, 1)), w, stride=2)
    assert out.shape[2:] == (H // 2, W // 2)
    g = _rand(2, H // 2, W // 2, 16, seed=20)
    want, = torch.autograd.grad(out, xin, _nchw(g))
    bwd = ref.pack_bwd(w.float())                                            # [Cin = 8][9][Cout = 16]: B's rows are the forward's inputs
    got = _restated(ref.conv3x3_stride2_rb_grad(2, H, W, 8, 16), g, [bwd])
    torch.testing.assert_close(got, want, **TOL)


def test_packer_layouts():
    w = _rand(5, 8, 3, 3, seed=21)
    fwd, bwd = ref.pack_fwd(w), ref.pack_bwd(w, ldb=7, fill=9.0)
    for co, ci, t in [(0, 0, 0), (4, 7, 8), (2, 3, 5)]:
        assert fwd[co, t, ci] == w[co, ci, t // 3, t % 3]
        assert bwd.reshape(-1)[(ci * 9 + 8 - t) * 7 + co] == w[co, ci, t // 3, t % 3]
    assert bool((bwd[:, :, 5:] == 9.0).all())
    # the bwd layout as the weights of a 3 x 3 padding-1 convolution over the output gradient is that convolution's data gradient
    xin = _rand(2, 8, 5, 6, seed=22).double().requires_grad_(True)
    g = _rand(2, 5, 6, 5, seed=23)
    want, = torch.autograd.grad(F.conv2d(xin, w.double(), padding=1), xin, _nchw(g))
    pad = torch.zeros(2, 5, 6, 3)                                            # Cin of the gradient's GEMM must be a multiple of 8
    got = _restated(ref.conv3x3(2, 5, 6, 8, 8), torch.cat([g, pad], dim=3), [ref.pack_bwd(w, ldb=8)])
    torch.testing.assert_close(got, want, **TOL)


# ---- the launcher's refusals ----
@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


X, W_, B, R, Y = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000       # addresses nothing reads: every call below stops at a check


def _desc(d, **kw):
    """d over unguarded layouts at the fake addresses"""
    d = replace(d, ph=[replace(t) for t in d.ph], **kw)
    d.ldx, d.xim, d.ldy, d.yim = d.Cin, d.Hin * d.Win, d.Cout, d.Hout * d.Wout
    off = 0
    for t in d.ph:
        t.ldw, t.w_off = t.ntaps * d.Cin, off
        off += d.Cout * t.ldw
    return d


def _call(lib, a):
    from soar_amd import hip_lib
    tile = C.c_int32(-1)
    rc = lib.soar_selftest_conv_gemm(C.byref(a), C.byref(tile), None)
    return rc, hip_lib.last_error(), tile.value


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _tab(p, **kw):
    def f(a):
        for k, v in kw.items():
            setattr(a.ph[p], k, v)
    return f


REFUSED = {
    # what the launcher already checked
    "Cin=12": (ref.conv3x3(2, 4, 4, 8, 8), _set(Cin=12), "Cin a multiple of 8"),
    "nph=5": (ref.conv3x3(2, 4, 4, 8, 8), _set(nph=5), "1 .. 4 tap tables"),
    "nph=0": (ref.conv3x3(2, 4, 4, 8, 8), _set(nph=0), "1 .. 4 tap tables"),
    "wbat without per_image": (ref.conv3x3(2, 4, 4, 8, 8), _set(wbat=1024), "B per image only with tiles per image"),
    "rows": (ref.conv1x1(2, 1 << 15, 1 << 15, 8, 8), _set(), "at most 2^30 rows"),
    # what were comments in conv_gemm.h
    "dil=0": (ref.conv3x3(2, 4, 4, 8, 8), _set(dil=0), "dil must be 1, or 2"),
    "dil=3": (ref.conv3x3(2, 4, 4, 8, 8), _set(dil=3), "dil must be 1, or 2"),
    "dil=2 reflect": (ref.conv3x3_reflect(2, 4, 4, 8, 8), _set(dil=2), "dil must be 1, or 2 with zero padding"),
    "stride=0": (ref.conv3x3(2, 4, 4, 8, 8), _set(stride=0), "stride=0"),
    "os=0": (ref.conv3x3(2, 4, 4, 8, 8), _set(os=0), "os=0"),
    "Cout=0": (ref.conv3x3(2, 4, 4, 8, 8), _set(Cout=0), "Cout=0"),
    "Hin=0": (ref.conv3x3(2, 4, 4, 8, 8), _set(Hin=0), "Hin=0"),
    "Win=-1": (ref.conv3x3(2, 4, 4, 8, 8), _set(Win=-1), "Win=-1"),
    "ntaps=0": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, ntaps=0), "tap table 0: ntaps must be 1 .. 9 (got 0)"),
    "ntaps=10": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, ntaps=10), "tap table 0: ntaps must be 1 .. 9 (got 10)"),
    "ntaps of a later table": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(3, ntaps=0), "tap table 3: ntaps"),
    "py=os": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, py=1), "py and px must lie in [0, os) (py=1, px=0, os=1)"),
    "px=-1": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(2, px=-1), "tap table 2: py and px"),
    "px=2, os=2": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(1, px=2), "tap table 1: py and px"),
    "reflect, one row": (ref.conv3x3_reflect(2, 1, 4, 8, 8), _set(), "mirrors once: rows -1 .. 1 of a 1-row input"),
    "reflect, one column": (ref.conv3x3_reflect(2, 4, 1, 8, 8), _set(), "columns -1 .. 1 of a 1-column input"),
    "reflect, far above": (ref.conv3x3_reflect(2, 2, 4, 8, 8), _tab(0, dy=(C.c_int8 * 9)(-2, -2, -2, -1, -1, -1, 0, 0, 0)), "rows -2 .. 1 of a 2-row"),
    "reflect, grid too tall": (ref.conv3x3_reflect(2, 4, 4, 8, 8), _set(Hg=8), "rows -1 .. 8 of a 4-row"),
    "reflect, stride past the mirror": (ref.conv3x3_reflect(2, 4, 4, 8, 8), _set(stride=3), "rows -1 .. 10 of a 4-row"),
    "x NULL": (ref.conv3x3(2, 4, 4, 8, 8), _set(x=None), "NULL x"),
    "y NULL": (ref.conv3x3(2, 4, 4, 8, 8), _set(y=None), "NULL y"),
    "w NULL": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(1, w=None), "tap table 1: NULL w"),
    "x off 16 bytes": (ref.conv3x3(2, 4, 4, 8, 8), _set(x=X + 4), "x must be 16-byte aligned"),
    "x off 16 bytes by 8": (ref.conv3x3(2, 4, 4, 8, 8), _set(x=X + 8), "x must be 16-byte aligned"),
    "ldx=10": (ref.conv3x3(2, 4, 4, 8, 8), _set(ldx=10), "ldx=10"),
    "wbat=6": (ref.matmul(2, 4, 8, 8), _set(wbat=6), "wbat=6"),
    "w off 16 bytes": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(2, w=W_ + 4), "tap table 2: w must be 16-byte aligned"),
    "ldw=74": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, ldw=74), "ldw=74"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_launcher_refuses(lib, name):
    d, mutate, telling = REFUSED[name]
    d = _desc(d)
    a = ref.c_args(d, X, W_, B, R, Y)
    mutate(a)
    rc, err, _ = _call(lib, a)
    assert rc != 0 and err.startswith("conv_gemm:") and telling in err, err
    # ... and the same descriptor without rows is nothing to do, whatever else it says
    a.N = 0
    assert _call(lib, a)[0] == 0


def test_no_rows_is_no_error_and_the_tile_rule_is_reported(lib):
    from soar_amd import hip_lib
    for kw in (dict(N=0), dict(Hg=0), dict(Wg=0)):
        a = ref.c_args(_desc(ref.conv3x3(2, 4, 4, 8, 8)), X, W_, None, None, Y)
        _set(**kw)(a)
        rc, _, tile = _call(lib, a)
        assert rc == 0 and tile == 64
    tile = C.c_int32(0)
    assert lib.soar_selftest_conv_gemm(None, C.byref(tile), None) != 0 and "NULL args" in hip_lib.last_error()
    a = ref.c_args(_desc(ref.conv3x3(2, 4, 4, 8, 8)), X, W_, None, None, Y)
    assert lib.soar_selftest_conv_gemm(C.byref(a), None, None) != 0 and "NULL tile_out" in hip_lib.last_error()
    # the packer's entry: arguments only
    assert lib.soar_selftest_conv_pack(None, Y, None, 4, 8, 9, 0, None) != 0 and "soar_selftest_conv_pack" in hip_lib.last_error()
    assert lib.soar_selftest_conv_pack(X, None, None, 4, 8, 9, 0, None) != 0
    assert lib.soar_selftest_conv_pack(X, Y, None, 0, 8, 9, 0, None) != 0
    assert lib.soar_selftest_conv_pack(X, Y, R, 4, 8, 9, 3, None) != 0 and "ldb=3" in hip_lib.last_error()
