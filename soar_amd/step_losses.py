"""The training step's image terms that had no kernel (csrc/step_terms.hip), as autograd nodes:

    consistency_loss(pred_normal, normal)        the predicted-normal consistency term with the gradient of BOTH images
    normal_view_terms(...)                       the front / back normal views: 0.2 cos_loss each, the normal-mask L1, the LPIPS inputs
    frame_extra_terms(comp_occ, gt_rgb, ...)     loss_occ with the count kept on the device, and gt_rgb_blended
    abs_mean(x)                                  mean|x|

(TS/system/gaussian_surfel_mvdream.py:305-460.)  HIP only -- no eager fallback; current stream, no synchronisation, no read-back, no
atomics.  Accepted without a copy: the plugin's ``[B,H,W,C]`` outputs (permuted views of planar memory), ``[B,C,H,W]`` batches whose
views lie a fixed stride apart in a larger allocation, base pointers that are only 4-byte aligned.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import torch

from . import hip_lib
from .hip_lib import check, ptr


def _need_hip(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} runs on HIP devices only (torch device type 'cuda' on ROCm); there is no CPU fallback")


def _scratch(dev) -> torch.Tensor:
    n = C.c_size_t(0)
    check(hip_lib.lib().soar_step_terms_scratch_bytes(C.byref(n)), "soar_step_terms_scratch_bytes")
    return torch.empty((int(n.value) // 8,), dtype=torch.float64, device=dev)


def _channel_first(t: torch.Tensor, Cn: int) -> Tuple[torch.Tensor, str]:
    """([..,C,H,W] view, how it was made) of an image given channel-last (the plugin's [B,H,W,C]: "moved"), channel-first ("as is") or,
    with Cn = 1, without a channel axis ("added").  (A shape that reads both ways, [..,C,H,C], is channel-last when its last axis is
    not the dense one: a permuted view of planar memory.  The limit of reading the layout from the shape: an INTERLEAVED image whose
    height equals its channel count, [..,C,W,C] with a dense last axis, is read as channel-first -- hand such an image over as a
    channel-first view.)"""
    if t.dim() >= 3:
        last, first = t.shape[-1] == Cn, t.shape[-3] == Cn
        if last and (not first or t.stride(-1) != 1):
            return t.movedim(-1, -3), "moved"
        if first:
            return t, "as is"
    if Cn == 1 and t.dim() >= 2:
        return t.unsqueeze(-3), "added"
    raise ValueError(f"expected an image with {Cn} channels, first or last, got {tuple(t.shape)}")


def _planar(t: torch.Tensor) -> bool:
    """the last three axes [C,H,W] lie plane after plane, row after row (axes of one entry may carry any stride)"""
    want = 1
    for size, stride in zip(reversed(t.shape[-3:]), reversed(t.stride()[-3:])):
        if size != 1 and stride != want:
            return False
        want *= size
    return True


def _planar_batch(t: torch.Tensor, Cn: int, dev) -> torch.Tensor:
    """[B,C,H,W] float32 on `dev` whose views are planar (the views themselves may lie any stride >= C H W apart): the tensor's own
    memory when it has that form, else a copy"""
    t, _ = _channel_first(t.detach(), Cn)
    if t.dim() == 3:
        t = t.unsqueeze(0)
    if t.dim() != 4:
        raise ValueError(f"expected [B,{Cn},H,W] / [B,H,W,{Cn}], got {tuple(t.shape)}")
    B, _, H, W = t.shape
    ok = t.dtype is torch.float32 and t.device == dev and _planar(t) and (B == 1 or t.stride(0) >= Cn * H * W)
    return t if ok else t.to(device=dev, dtype=torch.float32).contiguous()


def _dense(t: torch.Tensor) -> bool:
    """the elements fill one stretch of memory without gaps or overlaps, in whatever order of the axes"""
    want = 1
    for size, stride in sorted(((n, st) for n, st in zip(t.shape, t.stride()) if n != 1), key=lambda p: p[1]):
        if stride != want:
            return False
        want *= size
    return True


def _layout_of(t: torch.Tensor, Cn: int):
    """what the backward needs of an input to hand its gradient back in the input's form: (channel-first shape, how it was made)"""
    cf, how = _channel_first(t.detach(), Cn)
    return tuple(cf.shape), how


def _to_layout(grad: torch.Tensor, layout) -> torch.Tensor:
    """the planar gradient [B,C,H,W] in the form of the input `_layout_of` described (a permuted view for a channel-last input: no copy)"""
    shape, how = layout
    g = grad.reshape(shape)
    return g.movedim(-3, -1) if how == "moved" else (g.squeeze(-3) if how == "added" else g)


# ---- predicted-normal consistency ---------------------------------------------------------------------------------------------
class _Consistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, normal, thrsh, weight):
        _need_hip(pred, "consistency_loss")
        dev = pred.device
        a, b = _planar_batch(pred, 3, dev), _planar_batch(normal, 3, dev)
        if a.shape != b.shape:
            raise ValueError(f"consistency_loss: the two images differ in shape: {tuple(pred.shape)} and {tuple(normal.shape)}")
        B, _, H, W = a.shape
        L = hip_lib.lib()
        stats = torch.empty((B, 2), dtype=torch.float32, device=dev)
        scratch = _scratch(dev)
        ct, wt = float(math.cos(thrsh)), float(weight)
        sa, sb = (a.stride(0) if B > 1 else 3 * H * W), (b.stride(0) if B > 1 else 3 * H * W)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for v0 in range(0, B, 8):                            # (a launch holds 8 views at the most, like cos_loss's)
                nb = min(8, B - v0)
                check(L.soar_consistency_loss(nb, H, W, a.data_ptr() + 4 * v0 * sa, sa, b.data_ptr() + 4 * v0 * sb, sb, ct, wt,
                                              stats.data_ptr() + 8 * v0, scratch.data_ptr(), stream), "soar_consistency_loss")
        cnt = stats[:, 1]
        total = cnt.sum()
        ctx.saved = (a, b, stats, ct, wt, total, sa, sb)
        ctx.like = (_layout_of(pred, 3), _layout_of(normal, 3))
        # the fold of the views' {mean, count} pairs is losses.cos_loss's, expression for expression: the value has its bits
        # (a view without a selected pixel holds NaN = 0 / 0: its sum is 0; no view with one: 0 / 0 = NaN, as in the reference)
        return (torch.nan_to_num(stats[:, 0]) * cnt).sum() / total

    @staticmethod
    def backward(ctx, g):
        a, b, stats, ct, wt, total, sa, sb = ctx.saved
        pred, normal = ctx.like
        dev = a.device
        B, _, H, W = a.shape
        L = hip_lib.lib()
        ga = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        gb = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        # the kernel scales a view's gradients by upstream / max(count(view), 1): upstream_v = g count_v / total gives g / total
        # everywhere (no selected pixel anywhere: every gradient is the kernel's SELECTED zero, not a product with the NaN factor)
        up = (g.detach().to(device=dev, dtype=torch.float32).reshape(1) * stats[:, 1] / total).contiguous()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            for v0 in range(0, B, 8):
                nb = min(8, B - v0)
                check(L.soar_consistency_loss_backward(nb, H, W, a.data_ptr() + 4 * v0 * sa, sa, b.data_ptr() + 4 * v0 * sb, sb, ct, wt,
                                                       stats.data_ptr() + 8 * v0, up.data_ptr() + 4 * v0, ga.data_ptr() + 12 * v0 * H * W,
                                                       gb.data_ptr() + 12 * v0 * H * W, stream), "soar_consistency_loss_backward")
        return (_to_layout(ga, pred) if ctx.needs_input_grad[0] else None,
                _to_layout(gb, normal) if ctx.needs_input_grad[1] else None, None, None)


def consistency_loss(pred_normal: torch.Tensor, normal: torch.Tensor, thrsh: float = math.pi / 10000, weight: float = 1.0) -> torch.Tensor:
    """The reference's ``cos_loss(comp_pred_normal, comp_normal, thrsh=pi/10000)`` (TS/system/gaussian_surfel_mvdream.py:429-453)
    over a batch of views ``[B,H,W,3]`` / ``[B,3,H,W]``: one mean of ``1 - cos`` over the selected pixels of all views, differentiable
    in BOTH images, as the reference has it (its ``.detach()`` is commented out).  Value and ``pred_normal``'s gradient are those of
    ``losses.cos_loss(pred_normal, normal.detach(), None, thrsh)`` bit for bit, ``normal``'s gradient that of the call with the
    arguments exchanged: the products commute.  One launch each way per 8 views (and a finishing launch for the sums)."""
    return _Consistency.apply(pred_normal, normal, float(thrsh), float(weight))


# ---- the two normal views ------------------------------------------------------------------------------------------------------
class _NormalViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, comp_normal, comp_normal_mask, gt_F, gt_B, gt_mask):
        _need_hip(comp_normal, "normal_view_terms")
        dev = comp_normal.device
        n = _planar_batch(comp_normal, 3, dev)
        V, _, R, R2 = n.shape
        views = 2 if gt_B is not None else 1
        if R != R2 or V < views:
            raise ValueError(f"normal_view_terms: comp_normal must hold {views} square views, got {tuple(comp_normal.shape)}")
        m0 = _planar_batch(comp_normal_mask, 1, dev)[0]
        tF = _planar_batch(gt_F, 3, dev)[0]
        tB = _planar_batch(gt_B, 3, dev)[0] if gt_B is not None else None
        tm = _planar_batch(gt_mask, 1, dev)[0]
        for t, name, count in ((m0, "comp_normal_mask", R * R), (tF, "gt_normal_F", 3 * R * R), (tB, "gt_normal_B", 3 * R * R),
                               (tm, "gt_normal_mask", R * R)):
            if t is not None and t.numel() != count:
                raise ValueError(f"normal_view_terms: {name} must have {count} elements, got {tuple(t.shape)}")
        values = torch.zeros((3,), dtype=torch.float32, device=dev)
        stats = torch.zeros((6,), dtype=torch.float32, device=dev)
        lpips_in = torch.empty((2 * views, 3, R, R), dtype=torch.float32, device=dev)
        scratch = _scratch(dev)
        args = hip_lib.SoarNormalViewArgs(R=R, views=views, normal=ptr(n), normal_stride=n.stride(0) if V > 1 else 3 * R * R, mask0=ptr(m0),
                                          gt_F=ptr(tF), gt_B=ptr(tB), gt_mask=ptr(tm), values=ptr(values), stats=ptr(stats),
                                          lpips_in=ptr(lpips_in), scratch=ptr(scratch))
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_normal_view_terms(C.byref(args), 1, torch.cuda.current_stream(dev).cuda_stream), "soar_normal_view_terms")
        ctx.args, ctx.keep = args, (n, m0, tF, tB, tm, stats, scratch)
        ctx.like = (_layout_of(comp_normal, 3), _layout_of(comp_normal_mask, 1))
        ctx.n_masks = _planar_batch(comp_normal_mask, 1, dev).shape[0]
        ctx.views, ctx.V, ctx.R = views, V, R
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(stats)
        return values[0], values[1], values[2], lpips_in, stats

    @staticmethod
    def backward(ctx, g_f, g_b, g_l1, g_lp, _g_stats):
        n, m0, tF, tB, tm, stats, scratch = ctx.keep
        comp_normal, comp_normal_mask = ctx.like
        dev = n.device
        views, V, R = ctx.views, ctx.V, ctx.R
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        up = torch.stack([(zero if g is None else g.detach().to(device=dev, dtype=torch.float32).reshape(())) for g in (g_f, g_b, g_l1)])
        if g_lp is not None:
            g_lp = g_lp.detach().to(device=dev, dtype=torch.float32)[:views].contiguous()        # (the targets' rows are constants)
        # (views of the batch beyond the two this node reads get zeros)
        g_n = (torch.zeros if V > views else torch.empty)((V, 3, R, R), dtype=torch.float32, device=dev)
        g_m = (torch.zeros if ctx.n_masks > 1 else torch.empty)((ctx.n_masks, 1, R, R), dtype=torch.float32, device=dev)
        a = ctx.args
        a.up, a.g_lpips, a.g_normal, a.g_mask0 = ptr(up), ptr(g_lp), ptr(g_n), ptr(g_m)
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_normal_view_terms(C.byref(a), 2, torch.cuda.current_stream(dev).cuda_stream), "soar_normal_view_terms")
        return (_to_layout(g_n, comp_normal) if ctx.needs_input_grad[0] else None,
                _to_layout(g_m, comp_normal_mask) if ctx.needs_input_grad[1] else None, None, None, None)


def normal_view_terms(comp_normal: torch.Tensor, comp_normal_mask: torch.Tensor, gt_normal_F: torch.Tensor,
                      gt_normal_B: Optional[torch.Tensor], gt_normal_mask: torch.Tensor) -> Dict[str, Optional[torch.Tensor]]:
    """The front and back normal views of the video frame in one pass (TS/system/gaussian_surfel_mvdream.py:332-399).

    comp_normal ``[V,R,R,3]`` and comp_normal_mask ``[V,R,R,1]`` with V = 2 (front, back) are the plugin's; gt_normal_F / gt_normal_B
    ``[1,R,R,3]`` (``gt_normal_B`` may be None: the front view only) and gt_normal_mask ``[1,R,R]`` the batch's.  Returns

        "cos_F", "cos_B"   0.2 * cos_loss(comp_normal[v], gt_v, gt_normal_mask > 1e-5, thrsh=0)      ("cos_B": None without gt_normal_B)
        "mask_l1"          mean|comp_normal_mask[0, ..., 0] - gt_normal_mask[0]|
        "lpips_in"         [2 views,3,R,R]: ((x * m) - 0.5) * 2 of the rendered views, then of their targets -- ready for
                           ``LPIPSVGG(lpips_in[:views], lpips_in[views:])``.  The front view multiplies by the FLOAT mask, the back
                           view by ``(gt_normal_mask > 1e-5).float()``: the reference's asymmetry (:346, :378), kept.
        "stats"            detached {value, selected pixels} of the three terms

    The values are what ``losses.cos_loss`` / ``losses.masked_l1`` give for the same inputs, bit for bit.  The backward is one pass:
    comp_normal's gradient is the cosine terms' plus ``2 m`` times the upstream of the rendered views' LPIPS inputs."""
    f, b, l1, lp, stats = _NormalViews.apply(comp_normal, comp_normal_mask, gt_normal_F, gt_normal_B, gt_normal_mask)
    return {"cos_F": f, "cos_B": b if gt_normal_B is not None else None, "mask_l1": l1, "lpips_in": lp, "stats": stats.detach()}


# ---- loss_occ and the blended target --------------------------------------------------------------------------------------------
def _pixel_strides(t: torch.Tensor, H: int, W: int, name: str) -> Tuple[torch.Tensor, int, int]:
    """(tensor, channel stride, pixel stride) of one 3-channel image [..,H,W,3] / [..,3,H,W] or of one colour [3]"""
    if t.numel() == 3:
        t = t.reshape(3)
        return t, t.stride(0), 0
    cf, _ = _channel_first(t, 3)
    while cf.dim() > 3 and cf.shape[0] == 1:
        cf = cf[0]
    if cf.shape != (3, H, W):
        raise ValueError(f"frame_extra_terms: {name} must be one [H,W,3] / [3,H,W] image or a colour [3], got {tuple(t.shape)}")
    if H > 1 and W > 1 and cf.stride(1) != W * cf.stride(2):
        cf = cf.contiguous()                             # (rows that do not follow each other)
    return cf, cf.stride(0), (cf.stride(2) if W > 1 else cf.stride(1))


class _FrameExtra(torch.autograd.Function):
    @staticmethod
    def forward(ctx, comp_occ, gt_rgb, gt_mask, rand_bg):
        _need_hip(comp_occ, "frame_extra_terms")
        dev = comp_occ.device
        occ = _planar_batch(comp_occ, 3, dev)
        if occ.shape[0] != 1:
            raise ValueError(f"frame_extra_terms: comp_occ must hold one view, got {tuple(comp_occ.shape)}")
        _, _, H, W = occ.shape
        f32 = lambda t: t.detach().to(device=dev, dtype=torch.float32)
        m = f32(gt_mask).reshape(-1)
        if m.numel() != H * W:
            raise ValueError(f"frame_extra_terms: gt_mask must have H*W = {H * W} elements, got {tuple(gt_mask.shape)}")
        m = m.contiguous()
        rgb, rc, rp = _pixel_strides(f32(gt_rgb), H, W, "gt_rgb")
        bg, bc, bp = _pixel_strides(f32(rand_bg), H, W, "rand_bg")
        stats = torch.empty((2,), dtype=torch.float32, device=dev)
        blended = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)
        scratch = _scratch(dev)
        args = hip_lib.SoarFrameExtraArgs(H=H, W=W, occ=ptr(occ), gt_rgb=ptr(rgb), gt_mask=ptr(m), rand_bg=ptr(bg), stats=ptr(stats),
                                          blended=ptr(blended), scratch=ptr(scratch))
        args.rgb_stride[0], args.rgb_stride[1], args.bg_stride[0], args.bg_stride[1] = rc, rp, bc, bp
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_frame_extra_terms(C.byref(args), torch.cuda.current_stream(dev).cuda_stream), "soar_frame_extra_terms")
        ctx.args, ctx.keep, ctx.like = args, (occ, m, stats), _layout_of(comp_occ, 3)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(blended, stats)
        return stats[0], blended, stats

    @staticmethod
    def backward(ctx, g, _g_blended, _g_stats):
        if g is None:
            return None, None, None, None
        occ, m, stats = ctx.keep
        dev = occ.device
        up = g.detach().to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        g_occ = torch.empty(occ.shape, dtype=torch.float32, device=dev)
        a = ctx.args
        a.up, a.g_occ = ptr(up), ptr(g_occ)
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_frame_extra_terms_backward(C.byref(a), torch.cuda.current_stream(dev).cuda_stream),
                  "soar_frame_extra_terms_backward")
        return _to_layout(g_occ, ctx.like), None, None, None


def frame_extra_terms(comp_occ: torch.Tensor, gt_rgb: torch.Tensor, gt_mask: torch.Tensor, rand_bg: torch.Tensor) -> Dict[str, torch.Tensor]:
    """``loss_occ = (1 - comp_occ[gt_mask > 0]).mean()`` (TS/system/gaussian_surfel_mvdream.py:412-417) and
    ``gt_rgb_blended = gt_rgb * m + rand_bg * (1 - m)`` (:307-309) in one pass over the video frame.

    comp_occ ``[1,H,W,3]`` (the plugin's), gt_rgb ``[1,H,W,3]``, gt_mask ``[1,H,W]``, rand_bg an image like gt_rgb or the colour ``[3]``.
    Returns {"loss_occ": scalar (float64 sums; NaN with zero gradients for an empty mask -- the count never leaves the device),
    "gt_rgb_blended": [1,H,W,3] (a permuted view of planar memory, like the plugin's images; torch's bits), "stats": {value, elements}}."""
    loss, blended, stats = _FrameExtra.apply(comp_occ, gt_rgb, gt_mask, rand_bg)
    return {"loss_occ": loss, "gt_rgb_blended": blended.permute(0, 2, 3, 1), "stats": stats.detach()}


class _AbsMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        _need_hip(x, "abs_mean")
        d = x.detach()
        # the mean does not care about the order: any dense layout is walked as it lies in memory
        if d.dtype is not torch.float32 or not _dense(d):
            d = d.to(torch.float32).contiguous()
        if d.numel() == 0:
            raise ValueError("abs_mean: empty tensor")
        stats = torch.empty((2,), dtype=torch.float32, device=d.device)
        scratch = _scratch(d.device)
        with torch.cuda.device(d.device):
            check(hip_lib.lib().soar_abs_mean(d.numel(), d.data_ptr(), ptr(stats), ptr(scratch), torch.cuda.current_stream(d.device).cuda_stream),
                  "soar_abs_mean")
        ctx.keep = d
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        d = ctx.keep
        up = g.detach().to(device=d.device, dtype=torch.float32).reshape(1).contiguous()
        grad = torch.empty_strided(d.size(), d.stride(), dtype=torch.float32, device=d.device)
        with torch.cuda.device(d.device):
            check(hip_lib.lib().soar_abs_mean_backward(d.numel(), d.data_ptr(), ptr(up), ptr(grad), torch.cuda.current_stream(d.device).cuda_stream),
                  "soar_abs_mean_backward")
        return grad


def abs_mean(x: torch.Tensor) -> torch.Tensor:
    """``torch.abs(x).mean()`` (the curvature term, TS/system/gaussian_surfel_mvdream.py:455-460) as one node: float64 sums, gradient
    ``sign(x) / n`` with ``sign(0) = 0``."""
    return _AbsMean.apply(x)
