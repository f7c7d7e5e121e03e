"""The image-space loss and post-op kernels (soar_amd/csrc/ssim.hip, image_losses.hip, postops.hip) against the float64 references of
tests/image_ops_ref.py, through the C ABI, at the shapes where tiled and vectorised kernels go wrong: below a tile and below the
vector width, on and around the tile seams, both code paths (16-byte and scalar), misaligned views, the second trip of the capped loss
walks, the batched launches (the remainder branch of SSIM's remap across the XCDs among them), soar_ssim_rendered's promise about what
it writes, soar_view_finish / _backward with every combination of incoming gradients.

Every output and scratch buffer is filled with NaN before the call and sits inside a larger allocation with guard floats on both
sides: a kernel that leaves part of its output undefined, or writes outside it, fails here.  The bars are the project's existing ones
(tests/image_ops_ref.py); tests/test_image_ops_cpu.py shows that float32 reaches half of each on every case."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import image_ops_ref as R
from soar_amd import hip_lib
from soar_amd.hip_lib import check, ptr

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
GUARD = 64                                  # floats on either side of a buffer (256 bytes: the buffer keeps its allocation's alignment)
SENTINEL = -7777.25
NAN = float("nan")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """a NaN-filled float32 buffer of `shape` inside a larger allocation whose first and last GUARD floats hold a sentinel"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)
        self.t.fill_(NAN)
        assert self.t.data_ptr() % 16 == 0

    def cpu(self, what="buffer"):
        """the contents, after checking that the guards on both sides are untouched"""
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all()), f"{what}: a guard was written"
        return self.t.detach().cpu().clone()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    """bit for bit, NaN included (an untouched NaN fill equals an untouched NaN fill)"""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _misaligned(t, offset=1):
    """a contiguous copy of t that starts `offset` elements into its allocation"""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == offset * t.element_size() and v.is_contiguous()
    return v


def _within(got, ref, bar, what):
    """max-norm relative distance <= bar; a reference that is all zero asks for zeros"""
    if float(ref.abs().max()) == 0.0:
        assert float(got.abs().max()) == 0.0, what
        return 0.0
    d = R.rel_max(got, ref)
    assert d <= bar, (what, d, bar)
    return d


class _Batch:
    """soar_batch_begin(n) ... soar_batch_end(): the same entry point walked over n frames, launched once"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        check(hip_lib.lib().soar_batch_begin(self.n), "soar_batch_begin")
        return self

    def frame(self, f):
        check(hip_lib.lib().soar_batch_frame(f), "soar_batch_frame")

    def __exit__(self, *exc):
        hip_lib.lib().soar_batch_end()
        return False


# =====================================================================================================================================
# SSIM
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _ssim_ref64(name):
    a, b = R.ssim_inputs(R.ssim_case(name))
    return R.ssim_ref(a, b)


def _ssim_scratch(shape):
    k = C.c_size_t(0)
    check(hip_lib.lib().soar_ssim_scratch_floats(*shape, C.byref(k)), "soar_ssim_scratch_floats")
    return Guarded(int(k.value))


def _ssim_launch(shape, a, b, out, scratch, grad, rendered=None):
    L = hip_lib.lib()
    if rendered is None:
        check(L.soar_ssim(*shape, ptr(a), ptr(b), ptr(out.t), ptr(scratch.t), ptr(grad.t), _stream()), "soar_ssim")
    else:
        check(L.soar_ssim_rendered(*shape, ptr(a), ptr(b), ptr(out.t), ptr(scratch.t), ptr(grad.t), ptr(rendered), _stream()), "soar_ssim_rendered")


def _ssim_call(shape, a, b, rendered=None):
    """(value [1], gradient [C,H,W], scratch) on the CPU, from NaN-filled guarded buffers"""
    out, scratch, grad = Guarded(1), _ssim_scratch(shape), Guarded(*shape)
    _ssim_launch(shape, a, b, out, scratch, grad, rendered)
    return out.cpu("ssim value"), grad.cpu("ssim gradient"), scratch.cpu("ssim scratch")


def _ssim_written(shape, scratch):
    """the derivative maps and the per-wave partial sums of a scratch buffer"""
    Cn, H, W = shape
    maps = 3 * Cn * H * W
    tiles = (-(-H // 32)) * (-(-W // 32))
    start = (maps + 3) & ~3
    return scratch[:maps], scratch[start:start + 4 * tiles * Cn]


@pytest.mark.parametrize("case", R.SSIM_CASES, ids=R.SSIM_IDS)
def test_ssim_value_and_gradient_against_float64(case):
    """soar_ssim on every case of the table: value to 2e-6, gradient to 1e-4 of its largest element, everything it owns written and
    nothing else.  The misaligned views take the scalar kernels and give the aligned call's bits (the two instantiations stage the same
    values and run the same arithmetic), through the C ABI and through losses.ssim.  The flat cases -- E[x^2] - mu^2 cancels completely
    on the constant regions, C2 = 9e-4 is all that is left of the denominator -- are held to FLAT_SSIM_FACTOR times the float32
    oracle's own distance from float64, computed on the spot: the kernel rounds differently (one sum E[x^2] + E[y^2], two 1-ulp
    reciprocals), the same kind of error and not a larger one.
    Measured on an MI355X, kernel / float32 oracle: flat_vector value 3.9e-7 / 5.7e-7, gradient 1.6e-5 / 1.5e-4; flat_scalar value
    4.2e-7 / 7.2e-7, gradient 2.0e-5 / 9.2e-5 (both distances are printed with the result)."""
    name, shape, kind = case
    a, b = R.ssim_inputs(case)
    v64, g64 = _ssim_ref64(name)
    ad, bd = a.to(DEV), b.to(DEV)
    am, bm = (_misaligned(ad), _misaligned(bd)) if kind == "misaligned" else (ad, bd)
    v, g, scratch = _ssim_call(shape, am, bm)
    maps, partials = _ssim_written(shape, scratch)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(maps).all()) and bool(torch.isfinite(partials).all())
    dv, dg = abs(float(v) - v64), R.rel_max(g, g64)
    if kind == "flat":
        v32, g32 = R.ssim_ref(a, b, torch.float32)
        dv32, dg32 = abs(v32 - v64), R.rel_max(g32, g64)
        print(f"\nSSIM {name} {shape}: kernel - float64: value {dv:.2e}, gradient {dg:.2e}; float32 oracle - float64: value {dv32:.2e}, gradient {dg32:.2e}")
        assert dv <= R.FLAT_SSIM_FACTOR * dv32 and dg <= R.FLAT_SSIM_FACTOR * dg32
    else:
        print(f"\nSSIM {name} {shape}: kernel - float64: value {dv:.2e} (bar {R.SSIM_VALUE_BAR:.0e}), gradient {dg:.2e} (bar {R.SSIM_GRAD_BAR:.0e})")
        assert dv < R.SSIM_VALUE_BAR and dg < R.SSIM_GRAD_BAR
    if kind == "misaligned":
        v0, g0, _ = _ssim_call(shape, ad, bd)
        assert _same_bits(v, v0) and _same_bits(g, g0)
        from soar_amd.losses import ssim
        x = am.requires_grad_(True)
        out = ssim(x, bm)
        out.backward()
        assert _same_bits(out.detach().cpu().reshape(1), v) and _same_bits(x.grad.cpu(), g)


@pytest.mark.parametrize("shape,frames", [((3, 33, 36), 3), ((3, 65, 67), 2)], ids=["36_workgroups", "54_workgroups"])
def test_ssim_batched_with_a_remainder_in_the_xcd_remap(shape, frames):
    """Frames of different content through soar_batch_begin / _frame / _end: 36 and 54 workgroups, no multiple of 8, so the remap
    across the XCDs takes its remainder branch.  Values, gradients and everything written to the scratch equal the single calls bit
    for bit: a tile the remap misses or visits twice shows as NaN or as a wrong sum."""
    imgs = [tuple(t.to(DEV) for t in R.ssim_images(shape, 900 + f)) for f in range(frames)]
    singles = [_ssim_call(shape, a, b) for a, b in imgs]
    bufs = [(Guarded(1), _ssim_scratch(shape), Guarded(*shape)) for _ in range(frames)]
    with _Batch(frames) as batch:
        for f, ((a, b), (out, scratch, grad)) in enumerate(zip(imgs, bufs)):
            batch.frame(f)
            _ssim_launch(shape, a, b, out, scratch, grad)
    for f, ((out, scratch, grad), (v0, g0, s0)) in enumerate(zip(bufs, singles)):
        v, g, s = out.cpu(), grad.cpu(), scratch.cpu()
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(v).all()), f
        assert _same_bits(v, v0) and _same_bits(g, g0) and _same_bits(s, s0), f
    assert not _same_bits(singles[0][1], singles[1][1])              # (the frames do differ)


@pytest.mark.parametrize("name", ["flat_vector", "flat_scalar"])
def test_ssim_rendered_writes_the_gradient_of_rendered_tiles_only(name):
    """soar_ssim_rendered on the flat cases with one rendered pixel in the middle tile, in a corner tile, in the last (partial) tile,
    with nothing and with everything rendered: the value is soar_ssim's bit for bit; so is the gradient on every pixel of a tile that
    holds a rendered pixel (no NaN of an unwritten derivative map reaches it); the gradient plane of every other tile is untouched."""
    case = R.ssim_case(name)
    _, shape, _ = case
    a, b = R.ssim_inputs(case)
    ad, bd = a.to(DEV), b.to(DEV)
    v64, g64 = _ssim_ref64(name)
    v32, g32 = R.ssim_ref(a, b, torch.float32)
    dv32, dg32 = abs(v32 - v64), R.rel_max(g32, g64)
    v_full, g_full, _ = _ssim_call(shape, ad, bd)
    for rname, rendered in R.ssim_rendered_cases(shape):
        v, g, _ = _ssim_call(shape, ad, bd, rendered.to(DEV))
        tm = R.ssim_tile_mask(rendered)[None].expand(shape)
        assert _same_bits(v, v_full), rname
        assert bool(torch.isfinite(g[tm]).all()) and _same_bits(g[tm], g_full[tm]), rname
        assert bool(torch.isnan(g[~tm]).all()), rname
        assert (int(tm.sum()) == 0) if rname == "none" else (int(tm.sum()) == g.numel()) if rname == "all" else (0 < int(tm.sum()) <= 3 * 1024)
        dv = abs(float(v) - v64)
        dg = float((g[tm].double() - g64[tm]).abs().max() / g64.abs().max()) if bool(tm.any()) else 0.0
        print(f"\nsoar_ssim_rendered {name} '{rname}': {int(tm[0].sum())} pixels per plane written; kernel - float64: value {dv:.2e}, gradient "
              f"{dg:.2e}; float32 oracle - float64: value {dv32:.2e}, gradient {dg32:.2e}")
        assert dv <= R.FLAT_SSIM_FACTOR * dv32 and dg <= R.FLAT_SSIM_FACTOR * dg32, rname


# =====================================================================================================================================
# depth2normal, normal2curv
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _postop_ref64(hw):
    p = R.postop_inputs(hw)
    return R.d2n_ref(p.depth, p.mask, p.up_n), R.n2c_ref(p.normal, p.mask, p.up_c)


def _mask_bytes(mask):
    return mask.to(DEV).contiguous().view(torch.uint8)


def _d2n_call(hw, depth, mask_u8, up=None):
    """values [3,H,W] and (with an upstream gradient) dL/ddepth [1,H,W], from NaN-filled guarded buffers"""
    L = hip_lib.lib()
    H, W = hw
    k00, k11 = R.focals(H, W)
    out = Guarded(3, H, W)
    check(L.soar_depth2normal(W, H, ptr(depth), ptr(mask_u8), R.PRCP[0], R.PRCP[1], k00, k11, ptr(out.t), _stream()), "soar_depth2normal")
    if up is None:
        return out.cpu("depth normal"), None
    gd = Guarded(1, H, W)
    check(L.soar_depth2normal_backward(W, H, ptr(depth), ptr(mask_u8), R.PRCP[0], R.PRCP[1], k00, k11, ptr(up), ptr(gd.t), _stream()),
          "soar_depth2normal_backward")
    return out.cpu("depth normal"), gd.cpu("dL/ddepth")


def _n2c_call(hw, normal, mask_u8, up=None):
    L = hip_lib.lib()
    H, W = hw
    out = Guarded(1, H, W)
    check(L.soar_normal2curv(W, H, ptr(normal), ptr(mask_u8), ptr(out.t), _stream()), "soar_normal2curv")
    if up is None:
        return out.cpu("curvature"), None
    gn = Guarded(3, H, W)
    check(L.soar_normal2curv_backward(W, H, ptr(normal), ptr(mask_u8), ptr(up), ptr(gn.t), _stream()), "soar_normal2curv_backward")
    return out.cpu("curvature"), gn.cpu("dL/dnormal")


@pytest.mark.parametrize("hw", R.POSTOP_CASES, ids=R.POSTOP_IDS)
def test_depth2normal_and_normal2curv_against_float64(hw):
    """Values and gradients of the two stencil kernels below, at and just past their 32 x 8 block, fully written.  On 1 x 1, 1 x 9 and
    9 x 1 no pixel has two independent differences: the depth normal and its gradient are exactly zero."""
    p = R.postop_inputs(hw)
    (o64, g64), (c64, gn64) = _postop_ref64(hw)
    m = _mask_bytes(p.mask)
    out, gd = _d2n_call(hw, p.depth.to(DEV), m, p.up_n.to(DEV))
    curv, gn = _n2c_call(hw, p.normal.to(DEV), m, p.up_c.to(DEV))
    for t in (out, gd, curv, gn):
        assert bool(torch.isfinite(t).all())
    dv, dc = float((out - o64).abs().max()), float((curv - c64).abs().max())
    if hw in R.DEGENERATE_POSTOP_CASES:
        assert float(out.abs().max()) == 0.0 and float(gd.abs().max()) == 0.0
        dg = dl = 0.0
    else:
        dg, dl = R.rel_max(gd, g64), R.rel_l2(gd, g64)
    print(f"\n{hw}: kernel - float64: depth2normal value {dv:.2e} (bar {R.D2N_VALUE_BAR:.0e}), gradient {dg:.2e} max / {dl:.2e} L2 (bars "
          f"{R.D2N_GRAD_BAR:.0e} / {R.D2N_GRAD_L2_BAR:.0e}); normal2curv value {dc:.2e} (bar {R.N2C_VALUE_BAR:.0e})")
    assert dv <= R.D2N_VALUE_BAR and dg < R.D2N_GRAD_BAR and dl < R.D2N_GRAD_L2_BAR
    assert dc <= R.N2C_VALUE_BAR
    _within(gn, gn64, R.N2C_GRAD_BAR, "normal2curv gradient")


# =====================================================================================================================================
# view_finish
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _view_ref64(hw, seed_offset, combo):
    return R.view_finish_ref(R.view_inputs(hw, seed_offset), combo)


class _ViewDev:
    """a view_finish case on the device"""

    def __init__(self, hw, seed_offset=0):
        self.hw, self.seed_offset = hw, seed_offset
        self.v = v = R.view_inputs(hw, seed_offset)
        self.normal, self.depth, self.opac = v.normal.to(DEV), v.depth.to(DEV), v.opac.to(DEV)
        self.ups = [t.to(DEV) for t in (v.up_no, v.up_curv, v.up_pred, v.up_dd)]
        self.prcp = torch.tensor(R.PRCP, dtype=torch.float32, device=DEV)
        self.k = R.focals(*hw)

    def forward(self, outs):
        H, W = self.hw
        check(hip_lib.lib().soar_view_finish(W, H, ptr(self.normal), ptr(self.depth), ptr(self.opac), ptr(self.prcp), self.k[0], self.k[1],
                                             ptr(outs[0].t), ptr(outs[1].t), ptr(outs[2].t), _stream()), "soar_view_finish")

    def backward(self, combo, block):
        H, W = self.hw
        g = [ptr(t) if use else None for t, use in zip(self.ups, combo)]
        check(hip_lib.lib().soar_view_finish_backward(W, H, ptr(self.normal), ptr(self.depth), ptr(self.opac), ptr(self.prcp), self.k[0], self.k[1],
                                                      g[0], g[1], g[2], g[3], ptr(block.t), _stream()), "soar_view_finish_backward")

    def outs(self):
        H, W = self.hw
        return Guarded(3, H, W), Guarded(1, H, W), Guarded(3, H, W)

    def block(self):
        return Guarded(4, *self.hw)


def _check_view_gradient(block, ref, what):
    assert bool(torch.isfinite(block).all()), what                 # the block [4][H][W] is fully written
    _within(block[:3], ref[:3], R.N2C_GRAD_BAR, what + ": dL/dnormal")
    _within(block[3:], ref[3:], R.D2N_GRAD_BAR, what + ": dL/ddepth")
    if float(ref[3:].abs().max()) > 0:
        assert R.rel_l2(block[3:], ref[3:]) < R.D2N_GRAD_L2_BAR, what


@pytest.mark.parametrize("hw", R.POSTOP_CASES, ids=R.POSTOP_IDS)
def test_view_finish_forward(hw):
    """The three images of soar_view_finish against float64 (the bars of the separate kernels) and, bit for bit, against
    soar_depth2normal / soar_normal2curv composed with mask = opac > 1e-5 as include/soar_hip.h states it.  An opacity of exactly
    1e-5f is outside, the next float above it inside; under a region that is entirely outside -- the kernel's shortcut --
    normal_out still is (n (1,-1,-1) + 1) / 2."""
    d = _ViewDev(hw)
    v, (H, W) = d.v, hw
    outs = d.outs()
    d.forward(outs)
    normal_out, curv, pred = outs[0].cpu("normal_out"), outs[1].cpu("curv"), outs[2].cpu("pred_normal")
    for t in (normal_out, curv, pred):
        assert bool(torch.isfinite(t).all())
    no64, c64, p64 = _view_ref64(hw, 0, None)
    dn, dc, dp = float((normal_out - no64).abs().max()), float((curv - c64).abs().max()), float((pred - p64).abs().max())
    print(f"\nview_finish {hw}: kernel - float64: normal_out {dn:.2e}, curv {dc:.2e} (bar {R.N2C_VALUE_BAR:.0e}), pred_normal {dp:.2e} (bar {R.D2N_VALUE_BAR:.0e})")
    assert dn <= R.N2C_VALUE_BAR and dc <= R.N2C_VALUE_BAR and dp <= R.D2N_VALUE_BAR
    # ---- the same values as the separate entry points give
    mask = R.view_mask(v.opac)
    s = torch.tensor(R.SIGNS)[:, None, None]
    m = _mask_bytes(mask)
    n_sep, _ = _d2n_call(hw, d.depth, m)
    c_sep, _ = _n2c_call(hw, (v.normal * s).to(DEV), m)
    assert _same_bits(normal_out, (v.normal * s + 1.0) * 0.5)
    assert _same_bits(curv, c_sep)
    assert _same_bits(pred, (n_sep * s + 1.0) * 0.5)
    # ---- the side of the threshold
    flat_c, flat_p = curv.reshape(-1), pred.reshape(3, -1)
    for j, val in v.special.items():
        if val in (float(R.OPAC_LIMIT), 0.0):                       # outside: no curvature, the zero depth normal
            assert float(flat_c[j]) == 0.0 and bool((flat_p[:, j] == 0.5).all()), (j, val)
    if v.hole is not None:
        y, x = v.hole
        assert float(curv[0, y, x]) == 0.0 and bool((pred[:, y, x] == 0.5).all())
        assert _same_bits(normal_out[:, y, x], (v.normal[:, y, x] * s[:, 0, 0] + 1.0) * 0.5) and float((normal_out[:, y, x] - 0.5).abs().min()) > 1e-4


@pytest.mark.parametrize("combo", R.VIEW_COMBOS, ids=R.VIEW_COMBO_IDS)
@pytest.mark.parametrize("hw", R.POSTOP_CASES, ids=R.POSTOP_IDS)
def test_view_finish_backward(hw, combo):
    """soar_view_finish_backward with all four incoming gradients, with normal_out + depth_direct only (the point-wise kernel), with
    the curvature's, the depth normal's and the direct depth gradient alone: the block [4][H][W] against float64 with the bars of the
    separate backward kernels, fully written every time."""
    cname, use = combo
    d = _ViewDev(hw)
    block = d.block()
    d.backward(use, block)
    got = block.cpu("dL/dnormal and dL/ddepth")
    _check_view_gradient(got, _view_ref64(hw, 0, use), f"{hw} {cname}")
    if cname == "normal_out+depth_direct":
        # the threshold pixels: gradient of normal_out inside the mask only
        flat = got[:3].reshape(3, -1)
        for j, val in d.v.special.items():
            inside = val in (d.v.above, 1.0)
            assert bool((flat[:, j] != 0).all()) == inside and bool((flat[:, j] == 0).all()) == (not inside), (j, val)
        assert _same_bits(got[3:], d.v.up_dd)


def test_view_finish_batched():
    """Three frames of 9 x 33 with different content as one launch each way.  Forward: the single calls' bits.  Backward: inside a
    batch the general kernel runs even when only normal_out and the depth itself carry gradient -- each element then receives one
    addend onto zero, the point-wise kernel's bits; with stencil atomics the order of the float additions is free, so those
    combinations are held to the float64 bars."""
    hw, frames = (9, 33), 3
    ds = [_ViewDev(hw, f) for f in range(frames)]
    singles = []
    for d in ds:
        outs = d.outs()
        d.forward(outs)
        singles.append([o.cpu() for o in outs])
    bouts = [d.outs() for d in ds]
    with _Batch(frames) as batch:
        for f, d in enumerate(ds):
            batch.frame(f)
            d.forward(bouts[f])
    for f in range(frames):
        for name, o, want in zip(("normal_out", "curv", "pred_normal"), bouts[f], singles[f]):
            got = o.cpu(name)
            assert bool(torch.isfinite(got).all()) and _same_bits(got, want), (f, name)
    assert not _same_bits(singles[0][1], singles[1][1])
    for cname, use in R.VIEW_COMBOS:
        blocks = [d.block() for d in ds]
        with _Batch(frames) as batch:
            for f, d in enumerate(ds):
                batch.frame(f)
                d.backward(use, blocks[f])
        for f, d in enumerate(ds):
            got = blocks[f].cpu(cname)
            _check_view_gradient(got, _view_ref64(hw, f, use), f"frame {f} {cname}")
            if cname in ("normal_out+depth_direct", "depth_direct"):
                single = d.block()
                d.backward(use, single)
                assert _same_bits(got, single.cpu()), (f, cname)


# =====================================================================================================================================
# masked L1 and cosine loss
# =====================================================================================================================================
def _chw(t):
    return t.permute(2, 0, 1).contiguous().to(DEV)


def _loss_scratch():
    k = C.c_size_t(0)
    check(hip_lib.lib().soar_image_loss_scratch_floats(C.byref(k)), "soar_image_loss_scratch_floats")
    return Guarded(int(k.value))


def _loss_mask(mask, kind):
    if mask is None:
        return None
    m = mask.reshape(-1).to(DEV).view(torch.uint8)
    if kind == "offset1":
        m = _misaligned(m)
        assert m.data_ptr() % 4 == 1
    return m


class _LossCall:
    """one image pair through soar_masked_l1 / soar_cos_loss and its backward; cos = (cos(thrsh), weight) or None for the L1"""

    def __init__(self, hw, a, b, m, cos=None):
        self.hw, self.a, self.b, self.m, self.cos = hw, a, b, m, cos
        self.stats, self.scratch, self.grad = Guarded(2), _loss_scratch(), Guarded(3, *hw)
        self.up = torch.tensor([R.LOSS_UPSTREAM], dtype=torch.float32, device=DEV)

    def forward(self):
        L, (H, W) = hip_lib.lib(), self.hw
        if self.cos is None:
            check(L.soar_masked_l1(3, H, W, ptr(self.a), ptr(self.b), ptr(self.m), ptr(self.stats.t), ptr(self.scratch.t), _stream()), "soar_masked_l1")
        else:
            check(L.soar_cos_loss(3, H, W, ptr(self.a), ptr(self.b), ptr(self.m), self.cos[0], self.cos[1], ptr(self.stats.t), ptr(self.scratch.t),
                                  _stream()), "soar_cos_loss")

    def backward(self):
        L, (H, W) = hip_lib.lib(), self.hw
        if self.cos is None:
            check(L.soar_masked_l1_backward(3, H, W, ptr(self.a), ptr(self.b), ptr(self.m), ptr(self.stats.t), ptr(self.up), ptr(self.grad.t),
                                            _stream()), "soar_masked_l1_backward")
        else:
            check(L.soar_cos_loss_backward(3, H, W, ptr(self.a), ptr(self.b), ptr(self.m), self.cos[0], self.cos[1], ptr(self.stats.t), ptr(self.up),
                                           ptr(self.grad.t), _stream()), "soar_cos_loss_backward")

    def results(self):
        """(stats [2], gradient [H,W,3]) on the CPU; the scratch's guards are checked too"""
        self.scratch.cpu("loss scratch")
        return self.stats.cpu("stats"), self.grad.cpu("loss gradient").permute(1, 2, 0)


def _run_loss(hw, o, t, mask, kind, cos=None):
    call = _LossCall(hw, _chw(o), _chw(t), _loss_mask(mask, kind), cos)
    call.forward()
    call.backward()
    return call.results()


def _check_loss(what, stats, grad, ref):
    v64, n64, g64 = ref
    assert bool(torch.isfinite(grad).all()), what                  # fully written
    assert float(stats[1]) == n64, (what, float(stats[1]), n64)     # the selected count is exact
    if n64 == 0:
        assert math.isnan(float(stats[0])) and float(grad.abs().max()) == 0.0, what
        return f"\n    {what}: empty selection, NaN and zeros"
    dv = abs(float(stats[0]) - v64)
    assert dv < R.LOSS_VALUE_BAR * max(1.0, abs(v64)), (what, dv)
    dg = _within(grad, g64, R.LOSS_GRAD_BAR, what)
    return f"\n    {what}: value {dv:.2e}, gradient {dg:.2e} ({n64} selected)"


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=R.LOSS_IDS)
def test_masked_l1_against_float64(case):
    """soar_masked_l1 and its backward with and without the mask: value, exact count, gradient; gradient 0 where img == gt; an all-false
    mask gives NaN and an all-zero, fully written gradient; a mask at byte offset 1 drops the walk to the scalar path and gives the
    bits of an aligned copy.  513 x 513 (scalar) and 1026 x 1024 (16-byte) need a second trip of the capped grid-stride loop."""
    name, hw, kind = case
    o, t, m, eq = R.l1_inputs(case)
    line = f"\nmasked L1 {name}: kernel - float64 (bars {R.LOSS_VALUE_BAR:.0e} max(1, |v|), {R.LOSS_GRAD_BAR:.0e})"
    for mask in (m, None):
        stats, grad = _run_loss(hw, o, t, mask, kind)
        line += _check_loss(f"mask {mask is not None}", stats, grad, R.masked_l1_ref(o, t, mask))
        assert float(grad[eq].abs().max()) == 0.0
        if mask is not None and kind == "offset1":
            stats0, grad0 = _run_loss(hw, o, t, mask, "random")
            assert _same_bits(stats, stats0) and _same_bits(grad.contiguous(), grad0.contiguous())
    print(line)


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=R.LOSS_IDS)
def test_cos_loss_against_float64(case):
    """soar_cos_loss and its backward at (thrsh, weight) = (0, 1) and (0.6, 0.5), with and without the mask.  No pixel's float64 cosine
    lies within 1e-5 of cos(thrsh), so the selected count must match exactly and no tolerance absorbs a flipped pixel."""
    name, hw, kind = case
    line = f"\ncosine loss {name}: kernel - float64 (bars {R.LOSS_VALUE_BAR:.0e} max(1, |v|), {R.LOSS_GRAD_BAR:.0e})"
    for thr, wt in R.COS_SETTINGS:
        o, t, m = R.cos_inputs(case, thr, wt)
        cos = (float(math.cos(thr)), float(wt))
        for mask in (m, None):
            stats, grad = _run_loss(hw, o, t, mask, kind, cos)
            line += _check_loss(f"({thr}, {wt}) mask {mask is not None}", stats, grad, R.cos_loss_ref(o, t, mask, thr, wt))
            if mask is not None and kind == "offset1":
                stats0, grad0 = _run_loss(hw, o, t, mask, "random", cos)
                assert _same_bits(stats, stats0) and _same_bits(grad.contiguous(), grad0.contiguous())
    print(line)


@pytest.mark.parametrize("cos", [None, (1.0, 1.0)], ids=["masked_l1", "cos_loss"])
@pytest.mark.parametrize("hw", [(16, 17), (2, 2), (15, 17)], ids=["16x17", "2x2", "15x17"])
def test_loss_walks_batched(hw, cos):
    """Three views through the batch calls (the frame's argument block by blockIdx.y): the single calls' bits, forward and backward."""
    frames = 3
    data = [R.loss_images(hw, 700 + f) for f in range(frames)]
    for _, _, m in data:
        m[0, 0] = True                                              # (no view without a selected pixel: 2 x 2 could draw one)

    def calls():
        return [_LossCall(hw, _chw(o), _chw(t), _loss_mask(m, "random"), cos) for o, t, m in data]
    singles = calls()
    for c in singles:
        c.forward()
        c.backward()
    batched = calls()
    for step in ("forward", "backward"):
        with _Batch(frames) as batch:
            for f, c in enumerate(batched):
                batch.frame(f)
                getattr(c, step)()
    res = [c.results() for c in singles]
    for f, (c, (stats0, grad0)) in enumerate(zip(batched, res)):
        stats, grad = c.results()
        assert bool(torch.isfinite(stats).all()) and bool(torch.isfinite(grad).all()) and float(stats[1]) > 0, f
        assert _same_bits(stats, stats0) and _same_bits(grad.contiguous(), grad0.contiguous()), f
    assert not _same_bits(res[0][0], res[1][0])
