"""The surfels' attribute field: a drop-in for the reference's ``HashMLPSDFField`` (TS/geometry/sdf_fields.py:41-219) whose
encodings and heads run as HIP kernels (csrc/field.hip).

Every SOAR configuration sets ``use_explicit: false``: the renderer takes the surfels' colours, scales and offsets from
``pc.attribute_field(points)`` (TS/renderer/diff_gaussian_rasterizer.py:88-135), and the scale loss calls it once more on the
positions themselves.  The reference builds the field from nerfstudio's ``HashEncoding`` and ``MLP``; tiny-cuda-nn does not
build for gfx950, so on ROCm those fall back to their plain-torch forms, whose numerics this module follows (DESIGN.md
"Attribute field" states them in full):

* two multiresolution hash encodings (``encoding``; ``quat_encoding`` for the quaternions), 16 levels x 2 features, level
  resolutions ``floor(base_res * g ** arange(L))`` in float32, corners from ceil / floor of ``p * res``, nerfstudio's hash;
* five heads ``Linear(in, 64) -> ReLU -> Linear(64, out)``: shs (sigmoid), scales (sigmoid * 2e-2), quats (F.normalize),
  offsets (input ``[encoding, z]``, no activation), opacities (sigmoid).

One autograd node over two C calls, on the current stream, with no host synchronisation.  The gradients of the heads' weights
and of ``xyz`` / ``z`` are bitwise reproducible; the hash-table gradients are float atomics and may differ in the last bits from
run to run.  HIP only: ``forward`` refuses CPU tensors.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check

HEADS = ("shs", "scales", "quats", "offsets", "opacities")     # the C ABI's head order
HEAD_OUT = {"shs": 3, "scales": 1, "quats": 4, "offsets": 3, "opacities": 1}
HIDDEN = 64


def level_resolutions(num_levels: int = 16, base_res: int = 16, max_res: int = 2048) -> torch.Tensor:
    """nerfstudio's ``scalings``: computed on the CPU in float32, so that the finest default level is 2047, not 2048."""
    g = np.exp((np.log(max_res) - np.log(base_res)) / (num_levels - 1)) if num_levels > 1 else 1
    return torch.floor(base_res * g ** torch.arange(num_levels))


class HashEncoding(nn.Module):
    """The table of one multiresolution hash encoding: ``hash_table`` [L * 2^log2_hashmap_size, 2], U(-1, 1) * 1e-3."""

    def __init__(self, num_levels: int = 16, min_res: int = 16, max_res: int = 2048, log2_hashmap_size: int = 18,
                 features_per_level: int = 2, hash_init_scale: float = 0.001) -> None:
        super().__init__()
        self.num_levels, self.features_per_level, self.log2_hashmap_size = num_levels, features_per_level, log2_hashmap_size
        self.hash_table_size = 2 ** log2_hashmap_size
        self.scalings = level_resolutions(num_levels, min_res, max_res)
        table = torch.rand(self.hash_table_size * num_levels, features_per_level) * 2 - 1
        self.hash_table = nn.Parameter(table * hash_init_scale)

    def get_out_dim(self) -> int:
        return self.num_levels * self.features_per_level


class MLP(nn.Module):
    """``Linear(in, hidden) -> ReLU -> Linear(hidden, out)`` as nerfstudio's MLP with num_layers = 2 names it (``layers``)."""

    def __init__(self, in_dim: int, out_dim: int, layer_width: int = HIDDEN) -> None:
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(in_dim, layer_width), nn.Linear(layer_width, out_dim)])


class _FieldFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, field_cfg, xyz, z, table, qtable, *weights):
        log2_T, res, aabb, normalized = field_cfg
        N, dev = xyz.shape[0], xyz.device
        outs = [torch.empty(N, HEAD_OUT[h], device=dev) for h in HEADS]
        enc = torch.empty(N, 32, device=dev)
        qenc = torch.empty(N, 32, device=dev)
        a = _args(log2_T, res, aabb, normalized, xyz, z, table, qtable, weights, enc, qenc)
        for k in range(5):
            a.out[k] = outs[k].data_ptr()
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_field_forward(C.byref(a), _stream(dev)), "soar_field_forward")
        ctx.field_cfg = field_cfg
        ctx.save_for_backward(xyz, z, table, qtable, enc, qenc, *weights)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        log2_T, res, aabb, normalized = ctx.field_cfg
        xyz, z, table, qtable, enc, qenc, *weights = ctx.saved_tensors
        need = ctx.needs_input_grad
        N, dev = xyz.shape[0], xyz.device
        a = _args(log2_T, res, aabb, normalized, xyz, z, table, qtable, weights, enc, qenc)
        keep = []                                  # the float32 copies must outlive the launch
        for k, g in enumerate(grads):
            if g is not None:
                g = g.to(torch.float32).contiguous()
                keep.append(g)
                a.g_out[k] = g.data_ptr()
        # as in autograd over the torch form: what no upstream gradient reaches gets None (an optimizer then skips it)
        has = [g is not None for g in grads]
        enc_has = has[0] or has[1] or has[3] or has[4]
        d_xyz = torch.empty(N, 3, device=dev) if need[1] and any(has) else None
        d_z = torch.empty(2, device=dev) if need[2] and has[3] else None
        d_table = torch.empty_like(table) if need[3] and enc_has else None
        d_qtable = torch.empty_like(qtable) if need[4] and has[2] else None
        d_heads: List[Optional[torch.Tensor]] = []
        for k, h in enumerate(HEADS):
            want = any(need[5 + 4 * k: 9 + 4 * k]) and has[k]
            d_heads.append(torch.empty(_head_floats(h), device=dev) if want else None)
            if want:
                a.d_head[k] = d_heads[k].data_ptr()
        for name, t in (("d_xyz", d_xyz), ("d_z", d_z), ("d_table", d_table), ("d_qtable", d_qtable)):
            if t is not None:
                setattr(a, name, t.data_ptr())
        L = hip_lib.lib()
        ws = _workspace(_bytes(L.soar_field_workspace_bytes, "soar_field_workspace_bytes", N), dev)
        with torch.cuda.device(dev):
            check(L.soar_field_backward(C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)), "soar_field_backward")
        w_grads: List[Optional[torch.Tensor]] = []
        for k, h in enumerate(HEADS):
            in_dim, out = 34 if h == "offsets" else 32, HEAD_OUT[h]
            buf = d_heads[k]
            if buf is None:
                w_grads += [None] * 4
                continue
            o1, o2, o3 = HIDDEN * in_dim, HIDDEN * in_dim + HIDDEN, HIDDEN * in_dim + HIDDEN + out * HIDDEN
            parts = (buf[:o1].view(HIDDEN, in_dim), buf[o1:o2], buf[o2:o3].view(out, HIDDEN), buf[o3:])
            w_grads += [p if need[5 + 4 * k + i] else None for i, p in enumerate(parts)]
        return (None, d_xyz, d_z, d_table, d_qtable, *w_grads)


def _head_floats(h: str) -> int:
    in_dim, out = 34 if h == "offsets" else 32, HEAD_OUT[h]
    return HIDDEN * in_dim + HIDDEN + out * HIDDEN + out


def _args(log2_T, res, aabb, normalized, xyz, z, table, qtable, weights, enc, qenc) -> hip_lib.SoarFieldArgs:
    a = hip_lib.SoarFieldArgs()
    a.N, a.log2_T, a.normalized = xyz.shape[0], log2_T, int(normalized)
    for l, r in enumerate(res):
        a.res[l] = r
    a.xyz = xyz.data_ptr() if xyz.numel() else None
    a.aabb = None if normalized else aabb.data_ptr()
    a.table, a.qtable = table.data_ptr(), qtable.data_ptr()
    a.z = z.data_ptr() if z is not None else None
    for k in range(5):
        w1, b1, w2, b2 = weights[4 * k: 4 * k + 4]
        a.head[k].w1, a.head[k].b1, a.head[k].w2, a.head[k].b2 = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    a.enc, a.qenc = enc.data_ptr(), qenc.data_ptr()
    return a


class HashMLPField(nn.Module):
    """Drop-in for ``HashMLPSDFField``: same constructor, parameter names, buffers and outputs.

    ``implementation`` and ``device`` are accepted and ignored (the field always runs csrc/field.hip; construct it on the CPU
    and move it with ``.to("cuda")`` as the reference does).  The kernels support the reference's shape only: 16 levels,
    2 features per level, 2 layers of width 64, at most 2^24 rows per level; anything else raises NotImplementedError, as
    ``use_linear=True`` does (the reference's ``get_attributes`` raises for it too)."""

    aabb: torch.Tensor

    def __init__(self, aabb: torch.Tensor, num_layers: int = 2, hidden_dim: int = 64, color_dim: int = 3, use_linear: bool = False,
                 num_levels: int = 16, max_res: int = 2048, base_res: int = 16, log2_hashmap_size: int = 18,
                 features_per_level: int = 2, implementation: str = "tcnn", device: str = "cuda") -> None:
        super().__init__()
        if use_linear:
            raise NotImplementedError("HashMLPField: use_linear=True is not implemented (nor is it in the reference's get_attributes)")
        unsupported = [(num_layers != 2, f"num_layers={num_layers} (2)"), (hidden_dim != HIDDEN, f"hidden_dim={hidden_dim} (64)"),
                       (features_per_level != 2, f"features_per_level={features_per_level} (2)"),
                       (num_levels != hip_lib.FIELD_LEVELS, f"num_levels={num_levels} (16)"),
                       (not 1 <= log2_hashmap_size <= 24, f"log2_hashmap_size={log2_hashmap_size} (1..24)")]
        bad = [m for b, m in unsupported if b]
        if bad:
            raise NotImplementedError("HashMLPField: the HIP kernels do not support " + ", ".join(bad))
        self.register_buffer("aabb", aabb)
        self.use_linear = use_linear
        self.register_buffer("max_res", torch.tensor(max_res))
        self.register_buffer("num_levels", torch.tensor(num_levels))
        self.register_buffer("log2_hashmap_size", torch.tensor(log2_hashmap_size))
        kw = dict(num_levels=num_levels, min_res=base_res, max_res=max_res, log2_hashmap_size=log2_hashmap_size,
                  features_per_level=features_per_level)
        self.encoding = HashEncoding(**kw)
        self.quat_encoding = HashEncoding(**kw)
        self.color_dim = color_dim
        d = self.encoding.get_out_dim()
        self.mlp_base_shs = MLP(d, 3)
        self.mlp_base_scales = MLP(d, 1)
        self.mlp_base_quats = MLP(d, 4)
        self.mlp_base_offsets = MLP(d + 2, 3)
        self.mlp_base_offsets.layers[-1].weight.data.zero_()
        self.mlp_base_offsets.layers[-1].bias.data.zero_()
        self.mlp_base_opacities = MLP(d, 1)
        self.device = device
        self._res = [float(r) for r in self.encoding.scalings]
        self._log2_T = log2_hashmap_size

    def _weights(self) -> List[torch.Tensor]:
        out = []
        for h in HEADS:
            m = getattr(self, f"mlp_base_{h}")
            out += [m.layers[0].weight, m.layers[0].bias, m.layers[1].weight, m.layers[1].bias]
        return out

    def get_attributes(self, xyzs: torch.Tensor, z: Optional[torch.Tensor] = None, pose=None, is_normalized: bool = False
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (shs [N,3], scales [N,1], quats [N,4], offsets [N,3], opacities [N,1]) for xyzs [..., 3] (N = their count).
        ``pose`` is accepted and unused, as in the reference."""
        if not isinstance(xyzs, torch.Tensor) or xyzs.shape[-1:] != (3,):
            raise ValueError(f"xyzs must be a [..., 3] tensor (got {tuple(getattr(xyzs, 'shape', ()))})")
        if not xyzs.is_cuda:
            raise RuntimeError(f"xyzs is on '{xyzs.device}': soar_amd.field runs on HIP devices only; there is no CPU fallback")
        dev = xyzs.device
        params = [self.encoding.hash_table, self.quat_encoding.hash_table] + self._weights()
        if any(p.device != dev for p in params) or (not is_normalized and self.aabb.device != dev):
            raise RuntimeError(f"HashMLPField: parameters are not on {dev}: move the module with .to('{dev}')")
        if any(p.dtype != torch.float32 for p in params):
            raise TypeError("HashMLPField: parameters must be float32")
        if z is not None:
            if not isinstance(z, torch.Tensor) or z.shape != (2,):
                raise ValueError(f"z must be a [2] tensor or None (got {tuple(getattr(z, 'shape', ()))})")
            if z.device != dev:
                raise RuntimeError(f"z is on '{z.device}', xyzs on '{dev}'")
            z = z.to(torch.float32).contiguous()
        x = xyzs.reshape(-1, 3).to(torch.float32).contiguous()
        aabb = self.aabb.to(torch.float32).contiguous()
        cfg = (self._log2_T, self._res, aabb, bool(is_normalized))
        return _FieldFn.apply(cfg, x, z, self.encoding.hash_table.contiguous(), self.quat_encoding.hash_table.contiguous(),
                              *[w.contiguous() for w in self._weights()])

    def forward(self, xyzs: torch.Tensor, pose: Optional[torch.Tensor] = None, z: Optional[torch.Tensor] = None,
                is_normalized: bool = False) -> Dict[str, torch.Tensor]:
        shs, scales, quats, offsets, opacities = self.get_attributes(xyzs, z=z, pose=pose, is_normalized=is_normalized)
        return {"shs": shs, "scales": scales, "quats": quats, "offsets": offsets, "opacities": opacities}

    def reset_field(self, xyzs: torch.Tensor, gt_shs: torch.Tensor, gt_scales: torch.Tensor, gt_quats: torch.Tensor,
                    weights: Optional[torch.Tensor] = None, ori_colors: Optional[torch.Tensor] = None, iterations: int = 1000,
                    log_every: int = 20) -> List[float]:
        """The reference's initial fit (surfel_base.py:274 calls it on 2P points): Adam at lr 1e-3 over every parameter,
        ``iterations`` steps of mean((shs - gt_shs)^2) + 1000 * mse(scales, gt_scales) + mse(quats, gt_quats).  ``weights`` and
        ``ori_colors`` are unused, as in the reference.  Returns the loss of every ``log_every``-th step (the reference prints
        them)."""
        xyzs = xyzs.detach()
        gt_scales_, gt_quats_ = gt_scales.detach(), gt_quats.detach()
        optimizer = torch.optim.Adam(self.parameters(), lr=1e-3)
        losses = []
        for i in range(iterations):
            out = self(xyzs)
            loss = (((out["shs"] - gt_shs) ** 2).mean() + 1000 * F.mse_loss(out["scales"], gt_scales_)
                    + F.mse_loss(out["quats"], gt_quats_))
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            if i % log_every == 0:
                losses.append(float(loss.item()))
        return losses
