"""Float64 restatement of the shared implicit-GEMM convolution's descriptor (csrc/conv_gemm.h), written from the header's
comments: index grids, dilation, mirror or zero mask, a gather through ldx / xim, the product with w[co][tap][:] (wbat per image),
alpha / bias / res, and the scatter through ldy / yim / Wout.  It works on the flat buffers the kernel sees, at their offsets and
pitches, so the addressing is restated too; what lies between the rows (guards) is never touched.

Also: the descriptors the three networks build (vae.hip, normalnet.hip), restated; the weight packer's two layouts; a layout of
guarded buffers (NaN around x and w, a canary under y) shared by tests/test_conv_gemm_cpu.py and tests/test_conv_gemm_gpu.py."""
import ctypes as C
from dataclasses import dataclass, replace
from typing import List, Optional

import torch

CANARY = -12345.625            # exactly a float32; no sum of the tests' inputs comes near it


@dataclass
class Taps:
    """ConvTaps: w_off is the table's first element in the flat weight buffer"""
    dy: List[int]
    dx: List[int]
    py: int = 0
    px: int = 0
    w_off: int = 0
    ldw: int = 0

    @property
    def ntaps(self):
        return len(self.dy)


@dataclass
class Desc:
    """ConvGemm, the pointers as element offsets into flat buffers"""
    N: int
    Hg: int
    Wg: int
    Hin: int
    Win: int
    Cin: int
    Cout: int
    ph: List[Taps]
    stride: int = 1
    dil: int = 1
    reflect: int = 0
    os: int = 1
    Wout: int = 0
    Hout: int = 0              # the output's rows (what yim must hold; the kernel does not know it)
    alpha: float = 1.0
    per_image: int = 0
    x_off: int = 0
    ldx: int = 0
    xim: int = 0
    wbat: int = 0
    y_off: int = 0
    ldy: int = 0
    yim: int = 0

    @property
    def nph(self):
        return len(self.ph)


def square_taps(side, off):
    """a square kernel of side x side taps, tap (ky, kx) at offset (ky + off, kx + off)"""
    return Taps([t // side + off for t in range(side * side)], [t % side + off for t in range(side * side)])


def _grid(N, Hg, Wg, Hin, Win, Cin, Cout, ph, **kw):
    d = Desc(N=N, Hg=Hg, Wg=Wg, Hin=Hin, Win=Win, Cin=Cin, Cout=Cout, ph=ph, **kw)
    d.Wout, d.Hout = Wg * d.os, Hg * d.os
    return d


# ---- the descriptors the networks use ----
def conv3x3(N, H, W, Cin, Cout):
    """3 x 3, zero padding 1 (vae.hip conv_k with off = -1)"""
    return _grid(N, H, W, H, W, Cin, Cout, [square_taps(3, -1)])


def conv3x3_stride2(N, H, W, Cin, Cout):
    """3 x 3, stride 2, zero padding 1 (normalnet.hip's downsampling)"""
    return _grid(N, (H + 1) // 2, (W + 1) // 2, H, W, Cin, Cout, [square_taps(3, -1)], stride=2)


def conv3x3_stride2_rb(N, H, W, Cin, Cout):
    """3 x 3, stride 2, one row / column of zeros on the bottom / right only (vae.hip's downsample: taps at 0 .. 2)"""
    return _grid(N, H // 2, W // 2, H, W, Cin, Cout, [square_taps(3, 0)], stride=2)


def conv3x3_reflect(N, H, W, Cin, Cout, stride=1):
    """3 x 3, reflection padding 1 (normalnet.hip's residual trunk; stride 1 there)"""
    return _grid(N, (H - 1) // stride + 1, (W - 1) // stride + 1, H, W, Cin, Cout, [square_taps(3, -1)], stride=stride, reflect=1)


def conv1x1(N, H, W, Cin, Cout):
    return _grid(N, H, W, H, W, Cin, Cout, [square_taps(1, 0)])


def matmul(N, M, K, Cout):
    """y[n] (M x Cout) = alpha x[n] (M x K) B[n]^T, B[n] rows Cout x K (vae.hip mm_k): a one-row image of M pixels, one tap"""
    return _grid(N, 1, M, 1, M, K, Cout, [square_taps(1, 0)], per_image=1)


def _phase_axis(p):
    """the taps of output parity p of a stride-2, padding-1, 3-tap transposed convolution along one axis: (kernel index, offset)"""
    return [(1, 0)] if p == 0 else [(2, 0), (0, 1)]


def conv_transpose_phases(N, H, W, Cin, Cout):
    """ConvTranspose2d(3, stride 2, padding 1, output_padding 1) as four stride-1 convolutions, one per output parity, with 1, 2, 2 and
    4 taps (normalnet.hip's upsampling): zero padding, os = 2"""
    ph = []
    for p in range(4):
        ay, ax = _phase_axis(p >> 1), _phase_axis(p & 1)
        ph.append(Taps([d for _, d in ay for _ in ax], [d for _ in ay for _, d in ax], py=p >> 1, px=p & 1))
    return _grid(N, H, W, H, W, Cin, Cout, ph, os=2)


def pack_transpose_phases(w):
    """torch [Cin][Cout][3][3] -> the four phases' [Cout][tap][Cin] (normalnet.hip nn_pack_up_kernel)"""
    out = []
    for p in range(4):
        ay, ax = _phase_axis(p >> 1), _phase_axis(p & 1)
        out.append(torch.stack([w[:, :, ky, kx].t() for ky, _ in ay for kx, _ in ax], dim=1).contiguous())
    return out


def conv3x3_stride2_rb_grad(N, H, W, Cin, Cout):
    """the data gradient of conv3x3_stride2_rb over an H x W input: a 3 x 3 convolution with taps at -2 .. 0 over the output gradient
    ([N][H // 2][W // 2][Cout]) zero-dilated by two, weights in the packer's bwd form (vae.hip's backward)"""
    return _grid(N, H, W, H // 2, W // 2, Cout, Cin, [square_taps(3, -2)], dil=2)


# ---- the packer ----
def pack_fwd(w):
    """torch [Cout][Cin][kh][kw] -> [Cout][kk][Cin]"""
    return w.reshape(w.shape[0], w.shape[1], -1).permute(0, 2, 1).contiguous()


def pack_bwd(w, ldb=None, fill=0.0):
    """... -> the data gradient's form, spatially flipped and transposed: bwd[(ci kk + kk - 1 - t) ldb + co], as [Cin][kk][ldb]"""
    Cout, Cin = w.shape[:2]
    ldb = Cout if ldb is None else ldb
    out = torch.full((Cin, w[0, 0].numel(), ldb), fill, dtype=w.dtype, device=w.device)
    out[:, :, :Cout] = w.reshape(Cout, Cin, -1).flip(2).permute(1, 2, 0)
    return out


# ---- the restatement ----
def _mirror(i, n):
    m = torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))
    assert bool(((m >= 0) & (m < n)).all()), "a coordinate mirrors more than once"
    return m


def run(d: Desc, x, w, bias, res, y, absolute=False, with_k=False):
    """x, w, res, y: flat float64 buffers; bias [Cout] or None.  Returns (y with the descriptor's outputs written, mask of what was
    written).  absolute: the same sums over magnitudes, |alpha| sum |a||w| + |bias| + |res| (the scale of the rounding bound);
    with_k: also every output's K."""
    assert x.dtype == w.dtype == y.dtype == torch.float64
    dev = x.device
    ar = lambda n: torch.arange(n, device=dev, dtype=torch.int64)
    mag = (lambda t: t.abs()) if absolute else (lambda t: t)
    n = ar(d.N)[:, None, None]
    gy, gx = ar(d.Hg)[None, :, None], ar(d.Wg)[None, None, :]
    y = y.clone()
    written = torch.zeros(y.shape, dtype=torch.bool, device=dev)
    klen = torch.zeros(y.shape, dtype=torch.int64, device=dev)           # the length K = ntaps Cin of the sum behind every output
    for t in d.ph:
        acc = torch.zeros(d.N, d.Hg, d.Wg, d.Cout, dtype=torch.float64, device=dev)
        for i in range(t.ntaps):
            iy = (gy * d.stride + t.dy[i]).expand(d.N, d.Hg, d.Wg)
            ix = (gx * d.stride + t.dx[i]).expand(d.N, d.Hg, d.Wg)
            ok = torch.ones_like(iy, dtype=torch.bool)
            if d.dil == 2:
                ok = (iy % 2 == 0) & (ix % 2 == 0)
                iy, ix = torch.div(iy, 2, rounding_mode="floor"), torch.div(ix, 2, rounding_mode="floor")
            else:
                assert d.dil == 1
            if d.reflect:
                iy, ix = _mirror(iy, d.Hin), _mirror(ix, d.Win)
            else:
                ok = ok & (iy >= 0) & (iy < d.Hin) & (ix >= 0) & (ix < d.Win)
            iy, ix = torch.where(ok, iy, 0), torch.where(ok, ix, 0)
            row = d.x_off + (n * d.xim + iy * d.Win + ix) * d.ldx
            a = mag(x[row[..., None] + ar(d.Cin)])
            a = torch.where(ok[..., None], a, torch.zeros((), dtype=torch.float64, device=dev))
            wi = t.w_off + (n if d.wbat else n[:1]) * d.wbat + ar(d.Cout)[None, :, None] * t.ldw + i * d.Cin + ar(d.Cin)[None, None, :]
            acc += torch.einsum("nhwc,noc->nhwo", a, mag(w[wi]).expand(d.N, d.Cout, d.Cin))
        out = (abs(d.alpha) if absolute else d.alpha) * acc
        if bias is not None:
            out = out + mag(bias)
        idx = (d.y_off + (n * d.yim + (gy * d.os + t.py) * d.Wout + (gx * d.os + t.px)) * d.ldy)[..., None] + ar(d.Cout)
        if res is not None:
            out = out + mag(res[idx])
        assert not bool(written[idx].any()), "two grid rows write the same output"
        y[idx] = out
        written[idx] = True
        klen[idx] = t.ntaps * d.Cin
    return (y, written, klen) if with_k else (y, written)


# ---- guarded buffers ----
@dataclass
class Buffers:
    d: Desc
    x: torch.Tensor            # flat float32
    w: torch.Tensor
    bias: Optional[torch.Tensor]
    res: Optional[torch.Tensor]
    y: torch.Tensor            # flat float32, all canary


def guarded(d: Desc, x, ws, bias=None, res=None, x_wide=0, pad=True):
    """Lays a case out in flat float32 buffers and completes the descriptor's offsets and pitches.
    x [N][Hin][Win][Cin]; ws: per tap table [Cout][ntaps][Cin], or [N][Cout][ntaps][Cin] (B per image: wbat);
    bias [Cout]; res [N][Hout][Wout][Cout].
    pad: x sits 8 floats into a NaN buffer, its rows 4 floats apart (x_wide: the columns x_wide .. x_wide + Cin of a row of
    3 Cin + 4), 3 NaN rows behind every image; w has 4 NaN floats behind every row and 3 NaN rows behind Cout; y has 5 columns of
    canary behind Cout, 2 rows of it behind every image and starts 3 floats in; res is laid out as y, NaN where y has canary.
    All of it is allocated: a read out of bounds shows as NaN in the output, a write as a dead canary."""
    g = 1 if pad else 0
    dev = x.device
    nan = float("nan")
    d = replace(d, ph=[replace(t) for t in d.ph])
    N = d.N
    assert tuple(x.shape) == (N, d.Hin, d.Win, d.Cin)
    d.ldx = (3 * d.Cin + 4 if x_wide else d.Cin + 4) if pad else d.Cin
    d.xim = d.Hin * d.Win + 3 * g
    d.x_off = 8 * g + x_wide
    xb = torch.full((8 * g + N * d.xim * d.ldx + 8 * g,), nan, dtype=torch.float32, device=dev)
    xv = xb[8 * g: 8 * g + N * d.xim * d.ldx].view(N, d.xim, d.ldx)
    xv[:, :d.Hin * d.Win, x_wide:x_wide + d.Cin] = x.reshape(N, -1, d.Cin)

    per_img = any(w.dim() == 4 for w in ws)
    assert not per_img or (d.nph == 1 and d.per_image)
    parts, off = [], 4 * g
    for t, w in zip(d.ph, ws):
        w = w if w.dim() == 4 else w[None]
        B, Cout, nt, Cin = w.shape
        assert (Cout, nt, Cin) == (d.Cout, t.ntaps, d.Cin) and B in (1, N)
        t.ldw = nt * Cin + 4 * g
        blk = torch.full((B, Cout + 3 * g, t.ldw), nan, dtype=torch.float32, device=dev)
        blk[:, :Cout, :nt * Cin] = w.reshape(B, Cout, nt * Cin)
        t.w_off = off
        if per_img:
            d.wbat = (Cout + 3 * g) * t.ldw
        parts.append(blk.reshape(-1))
        off += blk.numel()
    wb = torch.cat([torch.full((4 * g,), nan, dtype=torch.float32, device=dev)] + parts)

    d.ldy = d.Cout + 5 * g
    d.yim = d.Hout * d.Wout + 2 * g
    d.y_off = 3 * g
    ny = 3 * g + N * d.yim * d.ldy
    yb = torch.full((ny,), CANARY, dtype=torch.float32, device=dev)
    rb = None
    if res is not None:
        assert tuple(res.shape) == (N, d.Hout, d.Wout, d.Cout)
        rb = torch.full((ny,), nan, dtype=torch.float32, device=dev)
        rb[3 * g:].view(N, d.yim, d.ldy)[:, :d.Hout * d.Wout, :d.Cout] = res.reshape(N, -1, d.Cout)
    bb = None
    if bias is not None:
        bb = torch.full((d.Cout + 4 * g,), nan, dtype=torch.float32, device=dev)
        bb[:d.Cout] = bias
    return Buffers(d, xb, wb, bb, rb, yb)


def expected(b: Buffers, absolute=False, with_k=False):
    """the float64 restatement over a case's buffers: (y, written)"""
    return run(b.d, b.x.double(), b.w.double(), None if b.bias is None else b.bias[:b.d.Cout].double(),
               None if b.res is None else b.res.double(), b.y.double(), absolute=absolute, with_k=with_k)


def logical(d: Desc, y):
    """the descriptor's output as [N][Hout][Wout][Cout], out of a flat y"""
    return y[d.y_off: d.y_off + d.N * d.yim * d.ldy].view(d.N, d.yim, d.ldy)[:, :d.Hout * d.Wout, :d.Cout].reshape(d.N, d.Hout, d.Wout, d.Cout)


# ---- the C descriptor ----
def c_args(d: Desc, x_ptr, w_ptr, bias_ptr, res_ptr, y_ptr):
    """SoarConvGemmArgs of d over buffers at these byte addresses (None: NULL)"""
    from soar_amd import hip_lib
    a = hip_lib.SoarConvGemmArgs()
    at = lambda p, off: None if p is None else p + 4 * off
    a.x, a.ldx, a.xim, a.wbat = at(x_ptr, d.x_off), d.ldx, d.xim, d.wbat
    a.bias, a.res = bias_ptr, at(res_ptr, d.y_off)
    a.y, a.ldy, a.yim, a.alpha = at(y_ptr, d.y_off), d.ldy, d.yim, d.alpha
    a.N, a.Hg, a.Wg, a.Hin, a.Win, a.Cin, a.Cout = d.N, d.Hg, d.Wg, d.Hin, d.Win, d.Cin, d.Cout
    a.stride, a.dil, a.reflect, a.Wout, a.os, a.per_image, a.nph = d.stride, d.dil, d.reflect, d.Wout, d.os, d.per_image, d.nph
    for p, t in enumerate(d.ph):
        s = a.ph[p]
        s.w, s.ldw, s.ntaps, s.py, s.px = at(w_ptr, t.w_off), t.ldw, t.ntaps, t.py, t.px
        s.dy, s.dx = (C.c_int8 * 9)(*t.dy), (C.c_int8 * 9)(*t.dx)
    return a
