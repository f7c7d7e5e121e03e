"""GPU tests of the data-gradient direction of the shared implicit-GEMM convolution with 16-bit operands (csrc/conv_gemm.hip:
conv_pack16_bwd_kernel, and conv_gemm16_kernel reading what it packs), through soar_selftest_conv_pack16_bwd and
soar_selftest_conv_gemm16.  Every case runs at bf16 and at f16.

The packer: bit for bit ``w.flip(-1).permute(1, 2, 0).to(type)`` laid out at ldb, the columns Cout .. ldb - 1 zeros, nothing written
behind the last row.

The data gradient of a 3 x 3 pad-1 convolution, of a 1 x 1 and of the encoder's 3 x 3 stride-2 downsample (as a convolution over the
gradient zero-dilated by two, dil = 2) against ``torch.nn.grad.conv2d_input`` in float64, exactly: weights and gradients are integers
in -8 .. 8, exact in both types, K <= 648, so every product and partial sum is an integer below 2^24 and the comparison has no
tolerance.  Sizes: 5 x 7 and 9 x 9 pixels at N = 2 (70 and 162 rows: off the 64-row tile, more than one tile, flat tiles that cross
the images), Cin != Cout (16 -> 24, so the gradient's GEMM has K = taps x 24 and 16 columns), K = 24 (inside a chunk of 64), 72,
216 and 648 (past one).  A is conv_gemm_ref's guarded buffers (x in NaN, y in a canary); B is the packer's output between NaN
elements of its own."""
import ctypes as C
from dataclasses import replace

import pytest
import torch
import torch.nn.functional as F

import conv_gemm_ref as ref
from soar_amd import hip_lib

pytestmark = pytest.mark.gpu

TYPES = {"bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}
PRECS = ["bf16", "f16"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _ints(dev, *shape, seed):
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float().to(dev)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _stream():
    return torch.cuda.current_stream().cuda_stream


GUARD = 64                     # 16-bit NaN elements on either side of the packed B (128 bytes: B stays 16-byte aligned)


def _pack_bwd(w, ldb, prec):
    """torch [Cout][Cin][kk] float32 -> (the whole guarded buffer, its [Cin][kk][ldb] part) as soar_selftest_conv_pack16_bwd writes it"""
    wtype, dt = TYPES[prec]
    Cout, Cin, kk = w.shape
    n = Cin * kk * ldb
    buf = torch.full((GUARD + n + GUARD,), float("nan"), dtype=dt, device=w.device)
    w = w.contiguous()
    hip_lib.check(hip_lib.lib().soar_selftest_conv_pack16_bwd(w.data_ptr(), buf.data_ptr() + 2 * GUARD, Cout, Cin, kk, ldb, wtype, _stream()),
                  "selftest_conv_pack16_bwd")
    return buf, buf[GUARD:GUARD + n].view(Cin, kk, ldb)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cout,Cin,kk,ldb", [(24, 16, 9, 24), (20, 17, 9, 24), (65, 3, 9, 72), (130, 40, 1, 136), (7, 33, 49, 8),
                                             (16, 24, 1, 16)])
def test_packer_matches_the_float32_layout_rounded(Cout, Cin, kk, ldb, prec, dev):
    wtype, dt = TYPES[prec]
    assert ldb % 8 == 0 and ldb >= Cout and Cin * kk * ldb > 256            # whole blocks of threads and, mostly, a part of one
    w = torch.randn(Cout, Cin, kk, generator=torch.Generator().manual_seed(400)).to(dev)
    w.view(-1)[:4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], device=dev)     # ties of both types
    buf, got = _pack_bwd(w, ldb, prec)
    want = w.flip(-1).permute(1, 2, 0).to(dt).contiguous()
    assert not torch.equal(want.float(), w.flip(-1).permute(1, 2, 0))
    assert torch.equal(_bits(got[:, :, :Cout].contiguous()), _bits(want))
    assert bool((_bits(got[:, :, Cout:].contiguous()) == 0).all())          # the tail: +0
    assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
    # ... and it is conv_gemm_ref's restatement of the float32 packer's bwd form, rounded
    assert torch.equal(_bits(got.contiguous()), _bits(ref.pack_bwd(w, ldb).to(dt)))


def _run_gradient(d, g, w, prec, dev):
    """d: the gradient's descriptor (its Cin = the convolution's Cout and the other way round); g [N][Hin][Win][Cout] the output
    gradient, NHWC; w torch [Cout][Cin][kk].  Runs it under both tile layouts with B from the new packer; returns [N][H][W][Cin]
    float64 after checking the canary and that the layouts agree."""
    Cout, Cin, kk = w.shape
    assert (d.Cin, d.Cout) == (Cout, Cin)
    # the float32 layout of the same B serves the restatement (which output elements are written) only
    b = ref.guarded(d, g, [ref.pack_bwd(w).view(Cin, kk, Cout)])
    _, written = ref.expected(b)
    buf, _ = _pack_bwd(w, Cout, prec)
    outs = []
    for per_image in (0, 1):
        dd = replace(b.d, per_image=per_image)
        y = torch.full_like(b.y, ref.CANARY)
        a = ref.c_args(dd, b.x.data_ptr(), b.w.data_ptr(), None, None, y.data_ptr())
        a.ph[0].w, a.ph[0].ldw = buf.data_ptr() + 2 * GUARD, kk * Cout
        tile = C.c_int32(0)
        hip_lib.check(hip_lib.lib().soar_selftest_conv_gemm16(C.byref(a), TYPES[prec][0], C.byref(tile), _stream()), "selftest_conv_gemm16")
        assert tile.value == 64
        assert torch.equal(_bits(y[~written]), _bits(b.y[~written])), "the canary around the output died"
        assert bool(torch.isfinite(y[written]).all())
        outs.append(ref.logical(b.d, y).double())
    assert torch.equal(outs[0], outs[1])
    return outs[0]


SIZES = [(2, 5, 7), (2, 9, 9)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,H,W", SIZES)
@pytest.mark.parametrize("Cin,Cout", [(16, 24), (24, 72)])
def test_3x3_data_gradient_is_exact(Cin, Cout, N, H, W, prec, dev):
    """K = 216 and 648"""
    w = _ints(dev, Cout, Cin, 3, 3, seed=H)
    g = _ints(dev, N, H, W, Cout, seed=H + 1)
    got = _run_gradient(ref.conv3x3(N, H, W, Cout, Cin), g, w.view(Cout, Cin, 9), prec, dev)
    want = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), g.permute(0, 3, 1, 2).double(), padding=1)
    assert float(want.abs().max()) > 0 and torch.equal(got, want.permute(0, 2, 3, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,H,W", SIZES)
@pytest.mark.parametrize("Cin,Cout", [(16, 24), (24, 72)])
def test_1x1_data_gradient_is_exact(Cin, Cout, N, H, W, prec, dev):
    """K = 24 (less than a chunk) and 72 (one chunk and an eighth)"""
    w = _ints(dev, Cout, Cin, 1, 1, seed=H + 10)
    g = _ints(dev, N, H, W, Cout, seed=H + 11)
    got = _run_gradient(ref.conv1x1(N, H, W, Cout, Cin), g, w.view(Cout, Cin, 1), prec, dev)
    want = torch.nn.grad.conv2d_input((N, Cin, H, W), w.double(), g.permute(0, 3, 1, 2).double())
    assert float(want.abs().max()) > 0 and torch.equal(got, want.permute(0, 2, 3, 1))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,H,W", SIZES)
@pytest.mark.parametrize("Cin,Cout", [(16, 24), (24, 72)])
def test_stride_2_data_gradient_through_dilation_is_exact(Cin, Cout, N, H, W, prec, dev):
    """The encoder's downsample, y = conv2d(pad(x, right and bottom by one), w, stride 2), over an odd H x W: its data gradient as
    a 3 x 3 convolution with taps at -2 .. 0 over the gradient zero-dilated by two.  The last input row and column of an odd size
    are read by the forward's padding-side taps only."""
    h, wd = H // 2, W // 2
    w = _ints(dev, Cout, Cin, 3, 3, seed=H + 20)
    g = _ints(dev, N, h, wd, Cout, seed=H + 21)
    d = ref.conv3x3_stride2_rb_grad(N, H, W, Cin, Cout)
    assert d.dil == 2 and (d.Hin, d.Win) == (h, wd)
    got = _run_gradient(d, g, w.view(Cout, Cin, 9), prec, dev)
    # the oracle, from the forward: autograd's gradient of the padded strided convolution, in float64
    x = torch.zeros(N, Cin, H, W, dtype=torch.float64, device=dev, requires_grad=True)
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), w.double(), stride=2)
    assert tuple(y.shape) == (N, Cout, h, wd)
    (want,) = torch.autograd.grad(y, x, g.permute(0, 3, 1, 2).double())
    padded = torch.nn.grad.conv2d_input((N, Cin, H + 1, W + 1), w.double(), g.permute(0, 3, 1, 2).double(), stride=2)
    assert torch.equal(want, padded[:, :, :H, :W])
    assert float(want.abs().max()) > 0 and torch.equal(got, want.permute(0, 2, 3, 1))
