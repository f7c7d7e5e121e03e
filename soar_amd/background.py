"""The environment-map background: a drop-in for the reference's ``NeuralEnvironmentMapBackground``
(``"gaussiandreamer-background"``, TS/background/gaussian_mvdream_background.py:15-73) whose hot path runs as HIP kernels
(csrc/envmap.hip).

Every SOAR configuration sets this background with ``random_aug: true``, ``share_aug_bg: true`` and ``random_aug_prob: 0.5``.
The renderer calls it once per optimizer step on the ray directions of the SDS views and the video frame, composites it behind
the SDS renders, and hands its last row to the guidance as ``comp_bg``.  The reference builds it from threestudio's
``get_encoding`` / ``get_mlp``: tiny-cuda-nn's ``SphericalHarmonics`` (degree 3: 9 values) of ``(dirs + 1) / 2`` and a
``VanillaMLP`` ``Linear(9, 16) -> ReLU -> Linear(16, 16) -> ReLU -> Linear(16, 3)`` without bias, then ``sigmoid``
(DESIGN.md 9d states it in full).  tiny-cuda-nn does not build for gfx950; this module computes the same in one kernel each way.

``forward(dirs)`` is the drop-in (one autograd node).  ``composite(dirs, renders, masks, n_comp)`` also forms
``renders + (1 - masks) * bg[:n_comp]`` in the same launch (one node, one C call each way); ``GaussianBatchRenderer`` uses it when
the background has it.  The weights' gradients are bitwise reproducible.  HIP only: CPU tensors are refused.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import random
from typing import Optional, Tuple

import torch
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check
from .renderer import registry
from .renderer.cameras import device_constant

ENC, HIDDEN, OUT = 9, 16, 3
DRAW = object()          # composite(color=DRAW): the module makes its own draws (see draw_color)

_SHIPPED_ENCODING = {"otype": "SphericalHarmonics", "degree": 3}
_SHIPPED_MLP = {"otype": "VanillaMLP", "activation": "ReLU", "n_neurons": HIDDEN, "n_hidden_layers": 2}


class _ColorRing:
    """Page-locked host buffers handed out in turn, as ``renderer/batch.py``'s ``_PinnedRing``: a pageable copy of the drawn colour
    would drain the stream.  A buffer is handed out again only when the copy that read it has completed."""

    def __init__(self, n: int = 8):
        self.n, self.bufs, self.events, self.k = n, [None] * n, [None] * n, 0

    def to_device(self, values: torch.Tensor, device) -> torch.Tensor:
        i, self.k = self.k, (self.k + 1) % self.n
        if self.events[i] is not None:
            self.events[i].synchronize()
        m = values.numel()
        if self.bufs[i] is None or self.bufs[i].numel() < m:
            self.bufs[i] = torch.empty(max(m, 3 * 16)).pin_memory()
        buf = self.bufs[i][:m]
        buf.copy_(values.reshape(-1))
        out = buf.to(device, non_blocking=True)
        self.events[i] = torch.cuda.Event()
        self.events[i].record(torch.cuda.current_stream(device))
        return out


_color_ring = _ColorRing()


class VanillaMLP(nn.Module):
    """threestudio's VanillaMLP as SOAR configures it: ``layers`` = Linear(9, 16) ReLU Linear(16, 16) ReLU Linear(16, 3), no bias
    (parameter names ``layers.0.weight``, ``layers.2.weight``, ``layers.4.weight``).  Evaluated by csrc/envmap.hip only."""

    def __init__(self, dim_in: int = ENC, dim_out: int = OUT, n_neurons: int = HIDDEN):
        super().__init__()
        self.layers = nn.Sequential(nn.Linear(dim_in, n_neurons, bias=False), nn.ReLU(inplace=True),
                                    nn.Linear(n_neurons, n_neurons, bias=False), nn.ReLU(inplace=True),
                                    nn.Linear(n_neurons, dim_out, bias=False))


def _image_stride(x: torch.Tensor, channels: int, H: int, W: int) -> Optional[int]:
    """elements from one image of x [n, channels, H, W] to the next when every image is contiguous and the images do not overlap,
    else None (the caller then makes x contiguous).  An expanded tensor (image stride 0, or less than one image) is None: the
    kernels read n images from the stride they are given."""
    st = x.stride()
    if st[3] != 1 and W > 1 or st[2] != W and H > 1 or channels > 1 and st[1] != H * W:
        return None
    if x.shape[0] <= 1:
        return channels * H * W
    return st[0] if st[0] >= channels * H * W else None


def _args(B, H, W, n_comp, color, dirs, renders, masks, weights) -> hip_lib.SoarEnvmapArgs:
    a = hip_lib.SoarEnvmapArgs()
    a.B, a.H, a.W, a.n_comp = B, H, W, n_comp
    if color is not None:
        a.color, a.color_rows = color.data_ptr(), color.numel() // 3
    else:
        a.dirs = hip_lib.ptr(dirs)
        a.w1, a.w2, a.w3 = (w.data_ptr() for w in weights)
    if n_comp > 0 and H * W > 0:
        rs, ms = _image_stride(renders, 3, H, W), _image_stride(masks, 1, H, W)
        if rs is None or ms is None:
            raise ValueError("renders / masks must hold contiguous, non-overlapping images (composite makes them so)")
        a.render, a.render_stride = renders.data_ptr(), rs
        a.mask, a.mask_stride = masks.data_ptr(), ms
    return a


class _EnvmapFn(torch.autograd.Function):
    """(n_comp, color, dirs, renders, masks, w1, w2, w3) -> (comp [n_comp, 3, H, W], bg [B, H, W, 3]); one C call each way"""

    @staticmethod
    def forward(ctx, n_comp, color, dirs, renders, masks, w1, w2, w3):
        B, H, W = dirs.shape[:3]
        dev = dirs.device
        bg = torch.empty(B, H, W, OUT, device=dev)
        comp = torch.empty(n_comp, OUT, H, W, device=dev)
        a = _args(B, H, W, n_comp, color, dirs, renders, masks, (w1, w2, w3))
        a.bg, a.comp = hip_lib.ptr(bg), hip_lib.ptr(comp)
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_envmap_forward(C.byref(a), _stream(dev)), "soar_envmap_forward")
        ctx.n_comp = n_comp
        ctx.save_for_backward(color, dirs, renders, masks, w1, w2, w3)
        ctx.set_materialize_grads(False)
        return comp, bg

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_comp, g_bg):
        color, dirs, renders, masks, w1, w2, w3 = ctx.saved_tensors
        need = ctx.needs_input_grad
        n_comp = ctx.n_comp
        B, H, W = dirs.shape[:3]
        dev = dirs.device
        a = _args(B, H, W, n_comp, color, dirs, renders, masks, (w1, w2, w3))
        keep = []                                          # float32 / contiguous copies must outlive the launch
        if g_comp is not None and n_comp > 0:
            g_comp = g_comp.to(torch.float32)
            keep.append(g_comp)
            a.g_comp = hip_lib.ptr(g_comp)
            for i, s in enumerate(g_comp.stride()):
                a.g_comp_stride[i] = s
        if g_bg is not None:
            g_bg = g_bg.to(torch.float32).contiguous()
            keep.append(g_bg)
            a.g_bg = hip_lib.ptr(g_bg)
        g_mask = None
        if need[4] and g_comp is not None:
            g_mask = torch.empty(n_comp, 1, H, W, device=dev)
            a.g_mask = hip_lib.ptr(g_mask)
        d_w = None
        if any(need[5:8]):
            # the weights' gradients: exact zeros (not None) when the colour was a constant, as the reference's ``color * 0 + ...``
            d_w = [torch.empty_like(w1), torch.empty_like(w2), torch.empty_like(w3)]
            a.d_w1, a.d_w2, a.d_w3 = (t.data_ptr() for t in d_w)
        L = hip_lib.lib()
        ws = _workspace(_bytes(L.soar_envmap_workspace_bytes, "soar_envmap_workspace_bytes", B, H, W), dev)
        with torch.cuda.device(dev):
            check(L.soar_envmap_backward(C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)), "soar_envmap_backward")
        g_render = g_comp if need[3] else None
        dw = [d_w[k] if d_w is not None and need[5 + k] else None for k in range(3)]
        return (None, None, None, g_render, g_mask, *dw)


@registry.register("gaussiandreamer-background")
class NeuralEnvironmentMapBackground(registry.BaseModule):
    """Drop-in for the reference's ``NeuralEnvironmentMapBackground``: same ``Config`` fields and defaults, same parameter names
    (``network.layers.{0,2,4}.weight``), same draws of Python's ``random`` and torch's CPU generator in the same order.

    Only what SOAR ships is supported: the SphericalHarmonics encoding of degree 3, a VanillaMLP of 16 neurons and 2 hidden layers
    with ReLU, 3 outputs, sigmoid.  Anything else raises NotImplementedError at construction, naming the key."""

    @dataclasses.dataclass
    class Config:
        n_output_dims: int = 3
        color_activation: str = "sigmoid"
        dir_encoding_config: dict = dataclasses.field(default_factory=lambda: dict(_SHIPPED_ENCODING))
        mlp_network_config: dict = dataclasses.field(default_factory=lambda: dict(_SHIPPED_MLP))
        random_aug: bool = False
        random_aug_prob: float = 0.5
        eval_color: Optional[Tuple[float, float, float]] = None
        share_aug_bg: bool = False

    cfg: Config

    def configure(self) -> None:
        cfg = self.cfg
        bad = []
        if cfg.n_output_dims != OUT:
            bad.append(f"n_output_dims={cfg.n_output_dims} (3)")
        if str(cfg.color_activation).lower() != "sigmoid":
            bad.append(f"color_activation={cfg.color_activation!r} ('sigmoid')")
        enc, mlp = dict(cfg.dir_encoding_config), dict(cfg.mlp_network_config)
        for name, got, shipped in (("dir_encoding_config", enc, _SHIPPED_ENCODING), ("mlp_network_config", mlp, _SHIPPED_MLP)):
            for key in sorted(set(got) | set(shipped)):
                if key == "output_activation" and name == "mlp_network_config" and got[key] in (None, "none"):
                    continue
                if key not in shipped or got.get(key) != shipped[key]:
                    bad.append(f"{name}.{key}={got.get(key)!r} ({shipped.get(key, 'absent')!r})")
        if cfg.eval_color is not None and len(cfg.eval_color) != OUT:
            bad.append(f"eval_color={cfg.eval_color!r} (3 values)")
        if bad:
            raise NotImplementedError("NeuralEnvironmentMapBackground: the HIP kernels do not support " + ", ".join(bad))
        # (the encoding has no parameters; a reference checkpoint's empty tensor of tiny-cuda-nn's encoding is dropped on load)
        self.network = VanillaMLP()
        self._register_load_state_dict_pre_hook(_drop_empty_encoding_params)

    # ---- the reference's draws --------------------------------------------------------------------------------------------
    def draw_color(self, n_rows: int, device) -> Optional[torch.Tensor]:
        """The constant colour the next call shows, or None for the MLP, drawn as the reference's ``forward`` draws it: with
        ``training and random_aug``, ``random.random() < random_aug_prob``, then ``random.random() < 0.5``, then
        ``torch.randn(n_color, 1, 1, 3)`` on the CPU generator (n_color = 1 with share_aug_bg, else n_rows).  In eval mode with
        ``eval_color``: that colour, no draws.  -> a device tensor [n_color * 3] (copied without draining the stream) or None."""
        if not self.training and self.cfg.eval_color is not None:
            return device_constant(self.cfg.eval_color, device)
        if self.training and self.cfg.random_aug and random.random() < self.cfg.random_aug_prob:
            n_color = 1 if self.cfg.share_aug_bg else n_rows
            value = random.random() < 0.5
            c = torch.randn(n_color, 1, 1, self.cfg.n_output_dims)
            # color * 0 + randn * value: +0.0 where value is False (randn * 0 may be -0.0; +0.0 + -0.0 = +0.0)
            return _color_ring.to_device(c if value else torch.zeros_like(c), device)
        return None

    def _weights(self, dev):
        ws = [self.network.layers[k].weight for k in (0, 2, 4)]
        if any(w.device != dev for w in ws):
            raise RuntimeError(f"NeuralEnvironmentMapBackground: parameters are not on {dev}: move the module with .to('{dev}')")
        if any(w.dtype != torch.float32 for w in ws):
            raise TypeError("NeuralEnvironmentMapBackground: parameters must be float32")
        return [w.contiguous() for w in ws]

    @staticmethod
    def _check_dirs(dirs) -> torch.Tensor:
        if not isinstance(dirs, torch.Tensor) or dirs.dim() != 4 or dirs.shape[-1] != 3:
            raise ValueError(f"dirs must be a [B, H, W, 3] tensor (got {tuple(getattr(dirs, 'shape', ()))})")
        if dirs.requires_grad:
            raise NotImplementedError("NeuralEnvironmentMapBackground: gradients with respect to dirs are not implemented "
                                      "(the reference's rays never require them): pass dirs.detach()")
        if not dirs.is_cuda:
            raise RuntimeError(f"dirs is on '{dirs.device}': soar_amd.background runs on HIP devices only; there is no CPU fallback")
        if dirs.dtype != torch.float32:
            raise TypeError(f"dirs must be float32 (got {dirs.dtype})")
        return dirs.contiguous()

    def forward(self, dirs: torch.Tensor) -> torch.Tensor:
        """-> bg [B, H, W, 3] for dirs [B, H, W, 3]: one autograd node, one C call each way."""
        dirs = self._check_dirs(dirs)
        color = self.draw_color(dirs.shape[0], dirs.device)
        return _EnvmapFn.apply(0, color, dirs, None, None, *self._weights(dirs.device))[1]

    def composite(self, dirs: torch.Tensor, renders: torch.Tensor, masks: torch.Tensor, n_comp: int,
                  color=DRAW) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (comp_rgb, bg): bg = self(dirs) [B, H, W, 3] and comp_rgb = (renders + (1 - masks) * bg[:n_comp].permute(0, 3, 1, 2))
        .permute(0, 2, 3, 1), an NHWC view of an NCHW buffer, each operation rounded as torch's.  renders [n_comp, 3, H, W] and
        masks [n_comp, 1, H, W] as the rasterizer stacks them.  One autograd node; gradients go to renders, masks and the weights.
        ``color``: what ``draw_color`` returned, when the caller made the draws earlier (the renderer makes them where the
        reference calls the background); by default the draws are made here."""
        dirs = self._check_dirs(dirs)
        B, H, W = dirs.shape[:3]
        if not 0 <= n_comp <= B:
            raise ValueError(f"need 0 <= n_comp <= B (n_comp={n_comp}, B={B})")
        for name, t, ch in (("renders", renders, 3), ("masks", masks, 1)):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n_comp, ch, H, W):
                raise ValueError(f"{name} must be a [{n_comp}, {ch}, {H}, {W}] tensor (got {tuple(getattr(t, 'shape', ()))})")
            if t.device != dirs.device or t.dtype != torch.float32:
                raise ValueError(f"{name} must be float32 on {dirs.device} (got {t.dtype} on {t.device})")
        if _image_stride(renders, 3, H, W) is None:
            renders = renders.contiguous()
        if _image_stride(masks, 1, H, W) is None:
            masks = masks.contiguous()
        if color is DRAW:
            color = self.draw_color(B, dirs.device)
        comp, bg = _EnvmapFn.apply(n_comp, color, dirs, renders, masks, *self._weights(dirs.device))
        return comp.permute(0, 2, 3, 1), bg


def _drop_empty_encoding_params(state_dict, prefix, *args):
    for k in [k for k in state_dict if k.startswith(prefix + "encoding.") and state_dict[k].numel() == 0]:
        del state_dict[k]
