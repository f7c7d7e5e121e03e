"""The differentiable part of the multi-view SDS guidance (ImageDream's ``MultiviewDiffusionGuidance``,
TS/guidance/imagedream_guidance.py, ``guidance_type: imagedream-multiview-diffusion-guidance`` in every SOAR config) as HIP kernels
(csrc/vae.hip): the Stable-Diffusion-2.1 VAE encoder with the resize folded into its first convolution, and the loss tail around
the caller's UNet.

* ``LatentEncoder(state_dict, scale_factor=0.18215, precision="f32")`` takes the ldm ``AutoencoderKL`` key layout (``encoder.*``, ``quant_conv.*``),
  with or without the ``first_stage_model.`` prefix; other keys (the decoder, the UNet) are ignored, a missing or misshapen key
  raises, naming it.  ``forward(rgb_NCHW, image_size=256, posterior_noise=None, grad_scale=None) -> latents`` is
  ``get_first_stage_encoding(encode_first_stage(interpolate(rgb) * 2 - 1))`` through one autograd node; the weights are frozen.
  ``encode(...) -> (mean, logvar)`` (no gradient) serves the tests.  ``precision="bf16"`` / ``"f16"`` (the reference's
  ``half_precision_weights``; the default ``"f32"`` is what the reference's encoder runs at) puts every product with a weight tensor,
  forward and data gradient, on the 16-bit matrix core; the rest and every activation in memory stay float32.
* ``MultiviewSDS(encoder, ...)`` is the guidance's ``forward`` with the UNet left to the caller: ``eps_fn(latent_model_input [2B, 4,
  h, w], t_expand [2B]) -> [2B, 4, h, w]`` in the order (text, uncond), a closure over ``model.apply_model`` and its context.

* ``MultiviewGuidance(encoder, unet, text_embeddings, image_tokens=None, ...)`` is the whole guidance: ``MultiviewSDS`` with
  ``soar_amd.unet.MultiviewUNet`` as its ``eps_fn``, the callable ``soar_amd.system`` takes as ``guidance``.

HIP only: CPU tensors are refused.  Inputs may have any strides (``comp_rgb.permute(0, 3, 1, 2)`` goes in without a copy; its
gradient comes back in the same layout).  DESIGN.md 9f states the computation in full.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Mapping, Optional, Tuple

import torch
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check
from .unet import PRECISIONS

CH, CH_MULT, Z = 128, (1, 2, 4, 4), 4
SCALE_FACTOR = 0.18215
PREFIX = "first_stage_model."


def _block(p: str, cin: int, cout: int) -> List[Tuple[str, Tuple[int, ...]]]:
    out = [(f"{p}.norm1.weight", (cin,)), (f"{p}.norm1.bias", (cin,)), (f"{p}.conv1.weight", (cout, cin, 3, 3)), (f"{p}.conv1.bias", (cout,)),
           (f"{p}.norm2.weight", (cout,)), (f"{p}.norm2.bias", (cout,)), (f"{p}.conv2.weight", (cout, cout, 3, 3)), (f"{p}.conv2.bias", (cout,))]
    if cin != cout:
        out += [(f"{p}.nin_shortcut.weight", (cout, cin, 1, 1)), (f"{p}.nin_shortcut.bias", (cout,))]
    return out


def weight_order() -> List[Tuple[str, Tuple[int, ...]]]:
    """(ldm key, shape) of every encoder tensor in the order of the flat array soar_vae_pack_weights reads (include/soar_hip.h)"""
    order = [("encoder.conv_in.weight", (CH, 3, 3, 3)), ("encoder.conv_in.bias", (CH,))]
    c = CH
    for i, m in enumerate(CH_MULT):
        for j in range(2):
            order += _block(f"encoder.down.{i}.block.{j}", c, CH * m)
            c = CH * m
        if i < len(CH_MULT) - 1:
            order += [(f"encoder.down.{i}.downsample.conv.weight", (c, c, 3, 3)), (f"encoder.down.{i}.downsample.conv.bias", (c,))]
    order += _block("encoder.mid.block_1", c, c)
    order += [("encoder.mid.attn_1.norm.weight", (c,)), ("encoder.mid.attn_1.norm.bias", (c,))]
    for n in ("q", "k", "v", "proj_out"):
        order += [(f"encoder.mid.attn_1.{n}.weight", (c, c, 1, 1)), (f"encoder.mid.attn_1.{n}.bias", (c,))]
    order += _block("encoder.mid.block_2", c, c)
    order += [("encoder.norm_out.weight", (c,)), ("encoder.norm_out.bias", (c,)), ("encoder.conv_out.weight", (2 * Z, c, 3, 3)),
              ("encoder.conv_out.bias", (2 * Z,)), ("quant_conv.weight", (2 * Z, 2 * Z, 1, 1)), ("quant_conv.bias", (2 * Z,))]
    return order


WEIGHT_ORDER = weight_order()


def ldm_schedule(n: int = 1000, linear_start: float = 0.00085, linear_end: float = 0.012) -> torch.Tensor:
    """ldm's ``register_schedule(beta_schedule='linear')``: betas = linspace(sqrt(start), sqrt(end), n)^2, alphas_cumprod in float64"""
    betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def schedule_tables(alphas_cumprod: torch.Tensor) -> torch.Tensor:
    """[5, n] float32: sqrt(ac), sqrt(1 - ac), sqrt(1 / ac), sqrt(1 / ac - 1), ac -- computed in float64, stored as float32 (ldm)"""
    ac = alphas_cumprod.detach().to("cpu", torch.float64).reshape(-1)
    return torch.stack([ac.sqrt(), (1 - ac).sqrt(), (1 / ac).sqrt(), (1 / ac - 1).sqrt(), ac]).to(torch.float32).contiguous()


def _strides(dst, t: torch.Tensor) -> None:
    for i, s in enumerate(t.stride()):
        dst[i] = s


def _check_image(t: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{what}: rgb must be an [N, 3, H, W] tensor (got {tuple(getattr(t, 'shape', ()))})")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: rgb is on '{t.device}': soar_amd.sds runs on HIP devices only; there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: rgb must be float32 (got {t.dtype})")


def _noise(t: Optional[torch.Tensor], shape, dev, what: str) -> torch.Tensor:
    if t is None:
        return torch.randn(shape, device=dev)
    if tuple(t.shape) != tuple(shape) or t.device != dev or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 {list(shape)} tensor on {dev} (got {list(t.shape)} {t.dtype} on {t.device})")
    return t.contiguous()


def _grad_scale(gs: Optional[torch.Tensor], N: int, H: int, W: int, dev) -> Optional[torch.Tensor]:
    if gs is None:
        return None
    if gs.dim() == 4 and gs.shape[-1] == 1:
        gs = gs[..., 0]
    if tuple(gs.shape) != (N, H, W) or gs.device != dev or gs.dtype != torch.float32:
        raise ValueError(f"grad_scale must be a float32 [N, H, W] or [N, H, W, 1] tensor on {dev} matching rgb (got {list(gs.shape)})")
    return gs.detach()


class _EncodeFn(torch.autograd.Function):
    """(module, image_size, x, eps, grad_scale) -> latents; one C call each way, the forward's workspace handed to the backward."""

    @staticmethod
    def forward(ctx, module, image_size, x, eps, grad_scale):
        lat, ws = module._run(x, image_size, eps=eps, want_latents=True)
        ctx.module, ctx.image_size, ctx.ws, ctx.grad_scale = module, image_size, ws, grad_scale
        ctx.save_for_backward(x)
        return lat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_lat):
        (x,) = ctx.saved_tensors
        g = ctx.module._backward(x, ctx.image_size, ctx.ws, g_lat.to(torch.float32).contiguous(), None, ctx.grad_scale)
        return None, None, g, None, None


class LatentEncoder(nn.Module):
    """The SD-2.1 VAE encoder + quant_conv + posterior sample (see the module's docstring).  The weights are one frozen flat buffer
    (``weights``, in WEIGHT_ORDER); move the module with ``.to(device)``.  They are packed for the kernels once per device.

    ``precision``: ``"f32"`` (the default), ``"bf16"`` or ``"f16"``.  With a 16-bit precision the packed copy holds the weight matrices
    of conv1 / conv2 / nin_shortcut, the downsamples, q | k | v and proj_out, in both directions, in that type; those products round
    their activations to it as they are loaded and sum in float32.  ``weights`` stays the float32 buffer.  In the backward the
    incoming gradient's scale is applied behind the last 16-bit product, so a small loss weight reaches no 16-bit operand; f16 also
    runs the backward on the gradient times 2^10 and divides at the end.  That constant has been checked on random weights only:
    bf16 is the precision to train with."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor], scale_factor: float = SCALE_FACTOR, precision: str = "f32"):
        super().__init__()
        if not isinstance(precision, str) or precision not in PRECISIONS:
            raise ValueError(f"LatentEncoder: precision must be one of 'f32', 'bf16', 'f16' (got {precision!r})")
        self.precision, self._code = precision, PRECISIONS[precision]
        sd = dict(state_dict)
        prefix = PREFIX if any(k.startswith(PREFIX + "encoder.") for k in sd) else ""
        parts = []
        for key, shape in WEIGHT_ORDER:
            k = prefix + key
            if k not in sd:
                raise KeyError(f"LatentEncoder: missing key '{k}' (expected shape {list(shape)})")
            t = sd[k]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
                raise ValueError(f"LatentEncoder: key '{k}' has shape {list(getattr(t, 'shape', ()))}, expected {list(shape)}")
            parts.append(t.detach().to(torch.float32).reshape(-1))
        self.register_buffer("weights", torch.cat(parts).contiguous())
        self.scale_factor = float(scale_factor)
        self._pack = hip_lib.PackedWeights()
        self.eval()

    def _packed(self, dev) -> torch.Tensor:
        w = self.weights

        def pack():
            L = hip_lib.lib()
            nf = _bytes(L.soar_vae_weights_floats, "soar_vae_weights_floats")
            if nf != w.numel():
                raise RuntimeError(f"LatentEncoder: the library expects {nf} weight floats, the module holds {w.numel()}")
            packed = _workspace(_bytes(L.soar_vae_weights_bytes16, "soar_vae_weights_bytes16", self._code), dev)
            with torch.cuda.device(dev):
                check(L.soar_vae_pack_weights16(w.data_ptr(), w.numel(), packed.data_ptr(), packed.numel(), self._code, _stream(dev)),
                      "soar_vae_pack_weights16")
            return packed

        return self._pack.get([w], dev, f"LatentEncoder: weights are not on {dev}: move the module with .to('{dev}')", pack)

    def _args(self, x: torch.Tensor, image_size: int) -> hip_lib.SoarVaeArgs:
        a = hip_lib.SoarVaeArgs()
        a.N, _, a.H, a.W = x.shape
        a.image_size = image_size
        a.x = hip_lib.ptr(x)
        _strides(a.x_stride, x)
        a.weights = self._pack.packed.data_ptr()
        a.scale_factor = self.scale_factor
        return a

    def _run(self, x, image_size, eps=None, want_latents=True, want_moments=False):
        """-> (latents or (mean, logvar), workspace)"""
        N, dev = x.shape[0], x.device
        h = image_size // 8
        L = hip_lib.lib()
        ws = _workspace(_bytes(L.soar_vae_workspace_bytes, "soar_vae_workspace_bytes", N, x.shape[2], x.shape[3], image_size), dev)
        a = self._args(x, image_size)
        outs = {}
        if want_latents:
            outs["latents"] = torch.empty(N, Z, h, h, device=dev)
            a.latents, a.eps = hip_lib.ptr(outs["latents"]), hip_lib.ptr(eps)
        if want_moments:
            outs["mean"], outs["logvar"] = torch.empty(N, Z, h, h, device=dev), torch.empty(N, Z, h, h, device=dev)
            a.mean, a.logvar = hip_lib.ptr(outs["mean"]), hip_lib.ptr(outs["logvar"])
        with torch.cuda.device(dev):
            check(L.soar_vae_forward16(C.byref(a), self._code, ws.data_ptr(), ws.numel(), _stream(dev)), "soar_vae_forward16")
        res = outs["latents"] if want_latents else (outs["mean"], outs["logvar"])
        return res, ws

    def _backward(self, x, image_size, ws, g_lat, g_scale, grad_scale):
        g = torch.empty_like(x)                                  # the input's own layout: a permuted view's gradient is one too
        a = self._args(x, image_size)
        a.g_latents, a.g_x = hip_lib.ptr(g_lat), hip_lib.ptr(g)
        _strides(a.g_x_stride, g)
        if g_scale is not None:
            a.g_scale = g_scale.data_ptr()
        if grad_scale is not None:
            a.grad_scale = grad_scale.data_ptr()
            _strides(a.grad_scale_stride, grad_scale)
        with torch.cuda.device(x.device):
            check(hip_lib.lib().soar_vae_backward16(C.byref(a), self._code, ws.data_ptr(), ws.numel(), _stream(x.device)),
                  "soar_vae_backward16")
        return g

    def _prepare(self, rgb, image_size):
        _check_image(rgb, "LatentEncoder")
        if not isinstance(image_size, int) or image_size < 8 or image_size % 8:
            raise ValueError(f"LatentEncoder: image_size must be a positive multiple of 8 (got {image_size})")
        self._packed(rgb.device)

    def encode(self, rgb: torch.Tensor, image_size: int = 256) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (mean, logvar) of the posterior, [N, 4, image_size / 8, image_size / 8]; logvar clamped to [-30, 20].  No gradient."""
        self._prepare(rgb, image_size)
        if rgb.shape[0] == 0:
            h = image_size // 8
            z = torch.zeros(0, Z, h, h, device=rgb.device)
            return z, z.clone()
        return self._run(rgb.detach(), image_size, want_latents=False, want_moments=True)[0]

    def forward(self, rgb: torch.Tensor, image_size: int = 256, posterior_noise: Optional[torch.Tensor] = None,
                grad_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> latents = scale_factor (mean + std posterior_noise), [N, 4, image_size / 8, image_size / 8].  posterior_noise None: drawn
        on the device.  grad_scale ([N, H, W] or [N, H, W, 1]): multiplied into rgb's gradient per pixel."""
        self._prepare(rgb, image_size)
        N, _, H, W = rgb.shape
        h = image_size // 8
        eps = _noise(posterior_noise, (N, Z, h, h), rgb.device, "posterior_noise")
        gs = _grad_scale(grad_scale, N, H, W, rgb.device)
        if N == 0:
            return torch.zeros(0, Z, h, h, device=rgb.device) + rgb.sum() * 0
        return _EncodeFn.apply(self, image_size, rgb, eps, gs)


class _SdsFn(torch.autograd.Function):
    """(sds, rgb, eps_fn, t, noise, posterior_noise, grad_scale, image_size) -> (loss, grad_norm): the encoder, q_sample, the caller's
    UNet and the loss tail in the forward; the encoder's data gradient of (latents - recon) / B, times the incoming gradient of
    loss (a device scalar), in the backward."""

    @staticmethod
    def forward(ctx, sds, rgb, eps_fn, t, noise, posterior_noise, grad_scale, image_size):
        enc = sds.encoder
        lat, ws = enc._run(rgb, image_size, eps=posterior_noise, want_latents=True)
        B, dev = lat.shape[0], lat.device
        a = sds._args(lat, t, noise)
        x_in = torch.empty((2 * B,) + tuple(lat.shape[1:]), device=dev)
        a.x_in = x_in.data_ptr()
        L = hip_lib.lib()
        with torch.cuda.device(dev):
            check(L.soar_sds_q_sample(C.byref(a), _stream(dev)), "soar_sds_q_sample")
        with torch.no_grad():
            eps = eps_fn(x_in, t.reshape(1).expand(2 * B))
        if not isinstance(eps, torch.Tensor) or tuple(eps.shape) != tuple(x_in.shape) or eps.device != dev:
            raise ValueError(f"MultiviewSDS: eps_fn must return a {list(x_in.shape)} tensor on {dev}")
        eps = eps.detach().to(torch.float32).contiguous()
        loss, gn, g_lat = torch.empty((), device=dev), torch.empty((), device=dev), torch.empty_like(lat)
        a.eps_pred, a.loss, a.grad_norm, a.g_lat = eps.data_ptr(), loss.data_ptr(), gn.data_ptr(), g_lat.data_ptr()
        with torch.cuda.device(dev):
            check(L.soar_sds_loss(C.byref(a), _stream(dev)), "soar_sds_loss")
        ctx.sds, ctx.ws, ctx.image_size, ctx.grad_scale = sds, ws, image_size, grad_scale
        ctx.save_for_backward(rgb, g_lat)
        ctx.mark_non_differentiable(gn)
        return loss, gn

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss, _g_gn):
        rgb, g_lat = ctx.saved_tensors
        g_loss = g_loss.to(torch.float32).contiguous()
        g = ctx.sds.encoder._backward(rgb, ctx.image_size, ctx.ws, g_lat, g_loss, ctx.grad_scale)
        return None, g, None, None, None, None, None, None


class MultiviewSDS(nn.Module):
    """ImageDream's ``MultiviewDiffusionGuidance.forward`` around a caller-supplied UNet (see the module's docstring).  Defaults are
    the s1 config's; the caller moves the step range as ``update_step`` does (``min_step_percent`` / ``max_step_percent``)."""

    def __init__(self, encoder: LatentEncoder, guidance_scale: float = 5.0, n_view: int = 4, recon_loss: bool = True,
                 recon_std_rescale: float = 0.2, min_step_percent: float = 0.02, max_step_percent: float = 0.75,
                 alphas_cumprod: Optional[torch.Tensor] = None, grad_clip: Optional[float] = None, image_size: int = 256):
        super().__init__()
        self.encoder = encoder
        self.guidance_scale, self.n_view, self.recon_loss = float(guidance_scale), int(n_view), bool(recon_loss)
        self.recon_std_rescale, self.grad_clip, self.image_size = float(recon_std_rescale), grad_clip, int(image_size)
        ac = ldm_schedule() if alphas_cumprod is None else alphas_cumprod
        self.register_buffer("tables", schedule_tables(ac))
        self.num_train_timesteps = self.tables.shape[1]
        self.set_step_range(min_step_percent, max_step_percent)

    def set_step_range(self, min_step_percent: float, max_step_percent: float) -> None:
        self.min_step = int(self.num_train_timesteps * min_step_percent)
        self.max_step = int(self.num_train_timesteps * max_step_percent)

    def _args(self, lat, t, noise) -> hip_lib.SoarSdsArgs:
        a = hip_lib.SoarSdsArgs()
        a.B, _, a.h, a.w = lat.shape
        a.n_view = self.n_view
        a.mode = hip_lib.SDS_RECON if self.recon_loss else hip_lib.SDS_PLAIN
        a.n_timesteps = self.num_train_timesteps
        a.guidance_scale, a.recon_std_rescale = self.guidance_scale, self.recon_std_rescale
        a.grad_clip = float(self.grad_clip) if self.grad_clip is not None else 0.0
        a.t, a.tables = t.data_ptr(), self.tables.data_ptr()
        a.latents, a.noise = lat.data_ptr(), noise.data_ptr()
        return a

    def forward(self, rgb: torch.Tensor, eps_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], t: Optional[torch.Tensor] = None,
                noise: Optional[torch.Tensor] = None, posterior_noise: Optional[torch.Tensor] = None,
                grad_scale: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """rgb [B, H, W, 3] (the renderer's comp_rgb / comp_normal) -> {"loss_sds", "grad_norm"} (device scalars).  t: an int64
        device tensor of one element, or None (uniform in [min_step, max_step], drawn on the device); noise / posterior_noise
        [B, 4, h, w] or None (drawn on the device)."""
        if not isinstance(rgb, torch.Tensor) or rgb.dim() != 4 or rgb.shape[3] != 3:
            raise ValueError(f"MultiviewSDS: rgb must be a [B, H, W, 3] tensor (got {tuple(getattr(rgb, 'shape', ()))})")
        x = rgb.permute(0, 3, 1, 2)
        self.encoder._prepare(x, self.image_size)
        B, dev, h = x.shape[0], x.device, self.image_size // 8
        if self.recon_loss and self.recon_std_rescale > 0 and B % self.n_view:
            raise ValueError(f"MultiviewSDS: B = {B} is not a multiple of n_view = {self.n_view} (recon_std_rescale > 0)")
        if self.tables.device != dev:
            raise RuntimeError(f"MultiviewSDS: the schedule is not on {dev}: move the module with .to('{dev}')")
        if t is None:
            t = torch.randint(self.min_step, self.max_step + 1, [1], dtype=torch.long, device=dev)
        elif not isinstance(t, torch.Tensor) or t.numel() != 1 or t.dtype != torch.long or t.device != dev:
            raise ValueError(f"MultiviewSDS: t must be an int64 tensor of one element on {dev}")
        noise = _noise(noise, (B, Z, h, h), dev, "noise")
        post = _noise(posterior_noise, (B, Z, h, h), dev, "posterior_noise")
        gs = _grad_scale(grad_scale, B, x.shape[2], x.shape[3], dev)
        if B == 0:
            z = x.sum() * 0
            return {"loss_sds": z, "grad_norm": z.detach()}
        loss, gn = _SdsFn.apply(self, x, eps_fn, t.reshape(1).contiguous(), noise, post, gs, self.image_size)
        return {"loss_sds": loss, "grad_norm": gn}


class MultiviewGuidance(nn.Module):
    """The guidance's ``forward`` (TS/guidance/imagedream_guidance.py:156-300, without ``ip_mode == "pixel"``'s extra view) with the
    UNet in this library: ``guidance(rgb, grad_scale=..., c2w=..., ref_rgb=..., **batch) -> {"loss_sds", "grad_norm"}``.

    ``text_embeddings [2, T, ctx]``: the prompt's and the unconditional prompt's CLIP text tokens (the caller's encoder); a row is
    repeated for every view of its half.  ``image_tokens(ref_rgb) -> (cond [ip_dim, ctx], uncond [ip_dim, ctx])``: the caller's CLIP
    image encoder and ``Resampler``; None: no image tokens are used, whatever ``ref_rgb`` is.  The cameras ``c2w [B, 4, 4]`` are
    normalised (``soar_amd.unet.normalize_camera``) and repeated for both halves.  Further arguments are ``MultiviewSDS``'s.

    ``unet`` may be a ``MultiviewUNet(..., precision="bf16")`` or ``"f16"`` (the reference's ``half_precision_weights``): its inputs
    and ``eps`` are float32 either way, so nothing here changes (tests/test_unet_half_gpu.py runs it with a bf16 UNet)."""

    def __init__(self, encoder: LatentEncoder, unet, text_embeddings: torch.Tensor, image_tokens: Optional[Callable] = None, **sds_args):
        super().__init__()
        if not isinstance(text_embeddings, torch.Tensor) or text_embeddings.dim() != 3 or text_embeddings.shape[0] != 2 or \
                text_embeddings.shape[2] != unet.cfg["context_dim"]:
            raise ValueError(f"MultiviewGuidance: text_embeddings must be [2, T, {unet.cfg['context_dim']}] (text, uncond) "
                             f"(got {list(getattr(text_embeddings, 'shape', ()))})")
        self.sds = MultiviewSDS(encoder, **sds_args)
        self.unet, self.image_tokens = unet, image_tokens
        self.register_buffer("text_embeddings", text_embeddings.detach().to(torch.float32).contiguous())

    def set_step_range(self, min_step_percent: float, max_step_percent: float) -> None:
        self.sds.set_step_range(min_step_percent, max_step_percent)

    def context(self, B: int, c2w: Optional[torch.Tensor], ref_rgb=None):
        """-> (context [2B, T, ctx], camera [2B, 16] or None, ip_tokens [2B, ip_dim, ctx] or None) in the order (text, uncond)"""
        from .unet import normalize_camera
        ctx = self.text_embeddings.repeat_interleave(B, dim=0)
        camera = None
        if self.unet.cfg["camera_dim"]:
            if c2w is None or tuple(c2w.shape) != (B, 4, 4):
                raise ValueError(f"MultiviewGuidance: c2w must be [{B}, 4, 4] (got {list(getattr(c2w, 'shape', ()))})")
            camera = normalize_camera(c2w.to(torch.float32)).repeat(2, 1)
        ip = None
        if self.image_tokens is not None and ref_rgb is not None:
            cond, uncond = self.image_tokens(ref_rgb)
            ip = torch.cat([cond[None].expand(B, -1, -1), uncond[None].expand(B, -1, -1)]).to(ctx)
        return ctx, camera, ip

    def forward(self, rgb: torch.Tensor, grad_scale: Optional[torch.Tensor] = None, c2w: Optional[torch.Tensor] = None, ref_rgb=None,
                t: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, posterior_noise: Optional[torch.Tensor] = None,
                **ignored) -> Dict[str, torch.Tensor]:
        if not isinstance(rgb, torch.Tensor) or rgb.dim() != 4 or rgb.shape[3] != 3:
            raise ValueError(f"MultiviewGuidance: rgb must be a [B, H, W, 3] tensor (got {tuple(getattr(rgb, 'shape', ()))})")
        if not rgb.is_cuda:
            raise RuntimeError(f"MultiviewGuidance: rgb is on '{rgb.device}': soar_amd.sds runs on HIP devices only; there is no CPU fallback")
        ctx, camera, ip = self.context(rgb.shape[0], c2w, ref_rgb)

        def eps_fn(x_in, t_expand):
            return self.unet(x_in, t_expand, ctx, camera=camera, ip_tokens=ip)

        return self.sds(rgb, eps_fn, t=t, noise=noise, posterior_noise=posterior_noise, grad_scale=grad_scale)
