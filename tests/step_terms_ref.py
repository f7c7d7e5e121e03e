"""Torch-CPU restatement of the image terms of the reference's training step (TS/system/gaussian_surfel_mvdream.py:305-460 and
:622-630), written fresh from the formulas, parameterised by dtype.  Images are channel-last, as the reference has them:
normals [B,H,W,3], masks [B,H,W]."""
import math

import torch


def cos_loss(output, gt, mask=None, thrsh=0.0, weight=1.0, dtype=torch.float64):
    """mean of 1 - cos over the masked pixels whose cosine is below cos(thrsh); NaN when there is none (:622-630)"""
    o = output.to(dtype) * 2 - 1
    g = gt.to(dtype) * 2 - 1
    if mask is not None:
        o, g = o[mask], g[mask]
    cos = (o * g * weight).sum(-1)
    return (1 - cos[cos < math.cos(thrsh)]).mean()


def blended(gt_rgb, gt_mask, rand_bg, dtype=torch.float64):
    """gt_rgb * m + rand_bg * (1 - m) (:307-309)"""
    m = gt_mask.to(dtype)[..., None]
    return gt_rgb.to(dtype) * m + rand_bg.to(dtype) * (1 - m)


def lpips_inputs(comp_normal, gt_F, gt_B, gt_normal_mask, dtype=torch.float64):
    """the four LPIPS inputs [2 views,3,R,R] (:342-358, :374-390): the front view multiplies by the float mask, the back view by its
    binarisation; the rendered views first, then the targets"""
    mf = gt_normal_mask.to(dtype)[..., None]
    mb = (gt_normal_mask > 1e-5).to(dtype)[..., None]
    f = lambda x, m: ((x.to(dtype) * m).permute(0, 3, 1, 2) - 0.5) * 2
    rows = [f(comp_normal[[0]], mf)] + ([f(comp_normal[[1]], mb)] if gt_B is not None else [])
    rows += [f(gt_F, mf)] + ([f(gt_B, mb)] if gt_B is not None else [])
    return torch.cat(rows, 0)


def normal_view_values(comp_normal, comp_normal_mask, gt_F, gt_B, gt_normal_mask, dtype=torch.float64):
    """{"cos_F", "cos_B", "mask_l1"}: 0.2 cos_loss per view over gt_normal_mask > 1e-5 (:332-341, :363-373), the normal-mask L1 (:395-399)"""
    sel = gt_normal_mask > 1e-5
    out = {"cos_F": 0.2 * cos_loss(comp_normal[[0]], gt_F, sel, 0.0, 1.0, dtype),
           "cos_B": None if gt_B is None else 0.2 * cos_loss(comp_normal[[1]], gt_B, sel, 0.0, 1.0, dtype),
           "mask_l1": (comp_normal_mask[0, ..., 0].to(dtype) - gt_normal_mask[0].to(dtype)).abs().mean()}
    return out


def loss_occ(comp_occ, gt_mask, dtype=torch.float64):
    """(1 - comp_occ[gt_mask > 0]).mean() (:412-417); NaN for an empty mask"""
    return (1 - comp_occ.to(dtype)[gt_mask > 0.0]).mean()


def abs_mean(x, dtype=torch.float64):
    """|x|.mean() (:455-460)"""
    return x.to(dtype).abs().mean()


def consistency_weight(lam, it):
    """C(lambda_normal_consistency) + 0.1 min(2 it / 2000, 1) (:450-453)"""
    return lam + 0.1 * min(2 * it / 2000, 1)
