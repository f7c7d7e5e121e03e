"""LPIPS-VGG: a drop-in for ``lpips.LPIPS(net='vgg', version='0.1').eval()`` (the normal-map loss of every SOAR configuration,
TS/system/gaussian_surfel_mvdream.py:21-24, 332-393) whose hot path runs as HIP kernels (csrc/lpips.hip).

``LPIPSVGG(state_dict)`` takes its weights from either layout:

* ``lpips.LPIPS(net='vgg').state_dict()``: ``net.slice{1..5}.{i}.weight|bias``, ``lin{k}.model.1.weight`` (the ``lins.{k}.*``
  duplicates are ignored) and ``scaling_layer.shift|scale``;
* torchvision's ``vgg16().state_dict()`` (``features.{i}.*``; ``classifier.*`` ignored) merged with lpips' ``weights/v0.1/vgg.pth``
  (``lin{k}.model.1.weight``); the scaling layer's constants then are lpips' own.

There is no default and no random initialisation: a missing or misshapen key raises, naming it.  ``forward(in0, in1)`` returns
``[N, 1, 1, 1]`` through one autograd node on the current stream, with no read-back; gradients go to whichever input requires them
(the target's branch keeps nothing when it does not).  Inputs may have any strides: ``x.permute(0, 3, 1, 2)`` of a channels-last
image goes in without a copy and its gradient comes back in the same layout.  HIP only: CPU tensors are refused.
(DESIGN.md 9e states the computation in full.)
"""
from __future__ import annotations

import ctypes as C
from typing import List, Mapping, Tuple

import torch
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check

# (Cin, Cout) of the 13 convolutions of VGG16 features[0:30] and their indices in torchvision's ``features``
CONV_CH: List[Tuple[int, int]] = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512),
                                  (512, 512), (512, 512), (512, 512), (512, 512), (512, 512)]
FEATURE_INDEX = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
TAP_CH = [64, 128, 256, 512, 512]
SHIFT = (-.030, -.088, -.188)         # lpips' ScalingLayer
SCALE = (.458, .448, .450)
MIN_SIZE = 16


def _slice_of(fi: int) -> int:
    """lpips' vgg16 keeps features[0:4], [4:9], [9:16], [16:23], [23:30] as slice1..slice5 under their torchvision indices"""
    return 1 if fi < 4 else 2 if fi < 9 else 3 if fi < 16 else 4 if fi < 23 else 5


def _take(sd: Mapping[str, torch.Tensor], key: str, shape: Tuple[int, ...]) -> torch.Tensor:
    if key not in sd:
        raise KeyError(f"LPIPSVGG: missing key '{key}' (expected shape {list(shape)})")
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        raise ValueError(f"LPIPSVGG: key '{key}' has shape {list(getattr(t, 'shape', ()))}, expected {list(shape)}")
    return t.detach().to(torch.float32).contiguous().clone()


def _constant(sd: Mapping[str, torch.Tensor], key: str, default: Tuple[float, float, float]) -> torch.Tensor:
    if key not in sd:
        return torch.tensor(default, dtype=torch.float32)
    t = sd[key]
    if not isinstance(t, torch.Tensor) or tuple(t.shape) not in ((1, 3, 1, 1), (3,)):
        raise ValueError(f"LPIPSVGG: key '{key}' has shape {list(getattr(t, 'shape', ()))}, expected [1, 3, 1, 1]")
    return t.detach().to(torch.float32).reshape(3).contiguous().clone()


class _LpipsFn(torch.autograd.Function):
    """(module, grads, in0, in1) -> [N]; one C call each way.  The forward's workspace (the kept branches' activations and tap
    gradients) is handed to the backward."""

    @staticmethod
    def forward(ctx, module, grads, in0, in1):
        N, _, H, W = in0.shape
        dev = in0.device
        L = hip_lib.lib()
        ws = _workspace(_bytes(L.soar_lpips_workspace_bytes, "soar_lpips_workspace_bytes", N, H, W, grads), dev)
        out = torch.empty(N, device=dev)
        a = module._args(in0, in1, grads)
        a.out = hip_lib.ptr(out)
        with torch.cuda.device(dev):
            check(L.soar_lpips_forward(C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)), "soar_lpips_forward")
        ctx.module, ctx.grads, ctx.ws = module, grads, ws
        ctx.save_for_backward(in0, in1)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        in0, in1 = ctx.saved_tensors
        need = ctx.needs_input_grad
        dev = in0.device
        g_out = g_out.to(torch.float32).contiguous()
        a = ctx.module._args(in0, in1, ctx.grads)
        a.g_out = hip_lib.ptr(g_out)
        g = [None, None]
        for b, (x, name) in enumerate(((in0, "g_in0"), (in1, "g_in1"))):
            if need[2 + b] and ctx.grads & (1 << b):
                g[b] = torch.empty_like(x)                   # the input's own layout: a permuted view's gradient is one too
                setattr(a, name, hip_lib.ptr(g[b]))
                st = getattr(a, name + "_stride")
                for i, s in enumerate(g[b].stride()):
                    st[i] = s
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_lpips_backward(C.byref(a), ctx.ws.data_ptr(), ctx.ws.numel(), _stream(dev)), "soar_lpips_backward")
        return None, None, g[0], g[1]


class LPIPSVGG(nn.Module):
    """``lpips.LPIPS(net='vgg', version='0.1', spatial=False).eval()`` from a state dict (see the module's docstring).  The weights
    are frozen buffers (``conv{i}_weight``, ``conv{i}_bias``, ``lin{k}``, ``shift``, ``scale``); move the module with ``.to(device)``.
    They are packed for the kernels once per device, on first use."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor]):
        super().__init__()
        sd = dict(state_dict)
        if "net.slice1.0.weight" in sd:
            prefix = [f"net.slice{_slice_of(fi)}.{fi}" for fi in FEATURE_INDEX]
        elif "features.0.weight" in sd:
            prefix = [f"features.{fi}" for fi in FEATURE_INDEX]
        else:
            raise KeyError("LPIPSVGG: missing key 'net.slice1.0.weight' (lpips' layout) or 'features.0.weight' (torchvision's vgg16)")
        for i, (p, (cin, cout)) in enumerate(zip(prefix, CONV_CH)):
            self.register_buffer(f"conv{i}_weight", _take(sd, p + ".weight", (cout, cin, 3, 3)))
            self.register_buffer(f"conv{i}_bias", _take(sd, p + ".bias", (cout,)))
        for k, c in enumerate(TAP_CH):
            self.register_buffer(f"lin{k}", _take(sd, f"lin{k}.model.1.weight", (1, c, 1, 1)).reshape(c))
        self.register_buffer("shift", _constant(sd, "scaling_layer.shift", SHIFT))
        self.register_buffer("scale", _constant(sd, "scaling_layer.scale", SCALE))
        self._pack = hip_lib.PackedWeights()
        self.eval()

    def _weights(self) -> List[torch.Tensor]:
        return ([getattr(self, f"conv{i}_weight") for i in range(13)] + [getattr(self, f"conv{i}_bias") for i in range(13)]
                + [getattr(self, f"lin{k}") for k in range(5)] + [self.shift, self.scale])

    def _packed(self, dev) -> torch.Tensor:
        ws = self._weights()

        def pack():
            L = hip_lib.lib()
            packed = _workspace(_bytes(L.soar_lpips_weights_bytes, "soar_lpips_weights_bytes"), dev)
            w = hip_lib.SoarLpipsWeights()
            for i in range(13):
                w.conv_w[i], w.conv_b[i] = ws[i].data_ptr(), ws[13 + i].data_ptr()
            for k in range(5):
                w.lin[k] = ws[26 + k].data_ptr()
            w.shift, w.scale = self.shift.data_ptr(), self.scale.data_ptr()
            with torch.cuda.device(dev):
                check(L.soar_lpips_pack_weights(C.byref(w), packed.data_ptr(), packed.numel(), _stream(dev)), "soar_lpips_pack_weights")
            return packed

        return self._pack.get(ws, dev, f"LPIPSVGG: weights are not on {dev}: move the module with .to('{dev}')", pack)

    def _args(self, in0, in1, grads) -> hip_lib.SoarLpipsArgs:
        a = hip_lib.SoarLpipsArgs()
        a.N, _, a.H, a.W = in0.shape
        a.grads = grads
        a.in0, a.in1 = hip_lib.ptr(in0), hip_lib.ptr(in1)
        for i in range(4):
            a.in0_stride[i], a.in1_stride[i] = in0.stride(i), in1.stride(i)
        a.weights = self._pack.packed.data_ptr()
        return a

    @staticmethod
    def _check(in0, in1):
        for name, t in (("in0", in0), ("in1", in1)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"LPIPSVGG: {name} must be an [N, 3, H, W] tensor (got {tuple(getattr(t, 'shape', ()))})")
        if in0.shape != in1.shape:
            raise ValueError(f"LPIPSVGG: in0 and in1 must have the same shape (got {tuple(in0.shape)} and {tuple(in1.shape)})")
        for name, t in (("in0", in0), ("in1", in1)):
            if not t.is_cuda:
                raise RuntimeError(f"LPIPSVGG: {name} is on '{t.device}': soar_amd.lpips runs on HIP devices only; there is no CPU fallback")
            if t.dtype != torch.float32:
                raise TypeError(f"LPIPSVGG: {name} must be float32 (got {t.dtype})")
        if in0.device != in1.device:
            raise ValueError(f"LPIPSVGG: in0 and in1 must be on the same device (got {in0.device} and {in1.device})")
        H, W = in0.shape[2:]
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LPIPSVGG: H, W >= {MIN_SIZE} needed so that relu5_3 has at least one pixel (got {H} x {W})")

    def forward(self, in0: torch.Tensor, in1: torch.Tensor) -> torch.Tensor:
        """-> [N, 1, 1, 1]: the LPIPS distance of every image pair (the reference then takes ``.mean()``)."""
        self._check(in0, in1)
        self._packed(in0.device)
        on = torch.is_grad_enabled()
        grads = (1 if on and in0.requires_grad else 0) | (2 if on and in1.requires_grad else 0)
        return _LpipsFn.apply(self, grads, in0, in1).view(-1, 1, 1, 1)
