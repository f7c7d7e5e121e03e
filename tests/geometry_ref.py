"""The geometry model's specification restated in plain torch, in float64 or float32: the five activations
(TS/geometry/surfel_base.py:441-476), the per-surfel regularizers (TS/system/gaussian_surfel_mvdream.py:257-296), the positions'
learning-rate schedule (TS/utils/general_utils.py:48-82) and the parameter-group table (TS/geometry/surfel_base.py:596-673).
Gradients come from autograd over these expressions."""
import math

import torch
import torch.nn.functional as F

LAMBDAS = ("lambda_position", "lambda_delta", "lambda_opacity", "lambda_sparsity", "lambda_scales")


def activations(rotation, scaling, opacity, occ, colors):
    return (F.normalize(rotation), torch.exp(scaling), torch.sigmoid(opacity), torch.sigmoid(occ), torch.sigmoid(colors))


def regularizer_terms(xyz, original_pos, scaling, opacity, scales):
    """The five terms as the reference writes them (scaling, opacity: activated; opacity [P,1])."""
    return (xyz.norm(dim=-1).mean(),
            (xyz - original_pos).norm(dim=-1).mean(),
            (scaling.norm(dim=-1).detach().unsqueeze(-1) * opacity).sum(),
            -(opacity - 0.5).pow(2).mean(),
            torch.mean(scales))


def regularizers(xyz, original_pos, scaling, opacity, scales, lambdas):
    """-> (loss, [5 terms]); a term whose weight is 0 is skipped (reported as 0), as the reference's ``if lambda > 0`` does."""
    terms = regularizer_terms(xyz, original_pos, scaling, opacity, scales)
    loss = xyz.new_zeros(())
    out = []
    for name, t in zip(LAMBDAS, terms):
        lam = float(lambdas.get(name, 0.0))
        if lam != 0.0:
            loss = loss + lam * t
            out.append(t.detach())
        else:
            out.append(xyz.new_zeros(()))
    return loss, out


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The closed form of get_expon_lr_func in Python doubles (math, not numpy)."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if lr_delay_steps > 0:
        delay = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
    else:
        delay = 1.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return delay * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)


def group_table(cfg, spatial_lr_scale):
    """(name, learning rate) of every parameter group, in the order of training_setup; cfg: any object with the *_lr fields."""
    return [("xyz", cfg.position_lr_init * spatial_lr_scale), ("f_dc", cfg.feature_lr), ("f_rest", cfg.feature_lr / 20.0),
            ("color", cfg.feature_lr), ("attribute_field_encoding", cfg.field_lr), ("attribute_field_quat_encoding", cfg.field_lr),
            ("attribute_field_shs", cfg.field_lr), ("attribute_field_quats", cfg.field_lr), ("attribute_field_scales", cfg.field_lr * 10),
            ("attribute_field_offests", cfg.field_lr * 0.01), ("opacity", cfg.opacity_lr), ("scaling", cfg.scaling_lr),
            ("rotation", cfg.rotation_lr), ("occ", cfg.occ_lr), ("latent_pose", cfg.latent_pose_lr)]


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def worst(a, b):
    """worst element over the largest magnitude"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300)) if b.numel() else 0.0
