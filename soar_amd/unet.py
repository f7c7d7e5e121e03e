"""The multi-view diffusion UNet of the SDS guidance on HIP kernels (csrc/unet.hip, csrc/attention.hip): ImageDream's
``sd-v2.1-base-4view-ipmv`` denoiser, forward only, in float32 or -- ``precision="bf16"`` / ``"f16"`` -- with every matrix product
on the 16-bit matrix core and, independently -- ``attention_precision="bf16"`` / ``"f16"`` -- both attentions of
every transformer there too.

``MultiviewUNet(state_dict)`` takes ldm's ``openaimodel.UNetModel`` keys with MVDream's / ImageDream's additions (``camera_embed.*``,
``attn2.to_k_ip`` / ``to_v_ip``), with or without the prefix ``model.diffusion_model.``; other keys (the VAE, CLIP, ``image_embed.*``)
are ignored, a missing or misshapen key raises, naming it.  The sizes are read from the shapes and key names (``infer_config``).
``forward(x, t, context, camera=None, ip_tokens=None) -> eps`` is ``apply_model`` of the latents of ``N / n_view`` groups of
``n_view`` views.  ``imagedream`` is not needed -- and was not available to check against: DESIGN.md 9w states the definition that
was built.

HIP only: CPU tensors are refused, there is no CPU fallback and no gradient.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check

PREFIX = "model.diffusion_model."
# stages of a block a probe can name (include/soar_hip.h SoarUnetArgs)
STAGES = {"res": 0, "attn1": 1, "attn2": 2, "ff": 3, "transformer": 4, "up": 5, "cat": 6, "res2": 7}
# the operands of the matrix products (SoarUnetConfig.precision) and of the attentions (attn_precision; soar_attention16's type)
PRECISIONS = {"f32": 0, "bf16": 1, "f16": 2}


def precision_code(who: str, name: str, value) -> int:
    """``PRECISIONS[value]``, or a ValueError naming the three choices."""
    if not isinstance(value, str) or value not in PRECISIONS:
        raise ValueError(f"{who}: {name} must be one of 'f32', 'bf16', 'f16' (got {value!r})")
    return PRECISIONS[value]


def _shape(sd, key: str, ndim: int) -> Tuple[int, ...]:
    if key not in sd:
        raise KeyError(f"MultiviewUNet: missing key '{key}'")
    s = tuple(getattr(sd[key], "shape", ()))
    if len(s) != ndim:
        raise ValueError(f"MultiviewUNet: key '{key}' has shape {list(s)}, expected {ndim} dimensions")
    return s


def strip_prefix(sd: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The UNet's tensors under ldm's bare keys, whether ``sd`` carries ``model.diffusion_model.`` or not."""
    if any(k.startswith(PREFIX) for k in sd):
        return {k[len(PREFIX):]: v for k, v in sd.items() if k.startswith(PREFIX)}
    return dict(sd)


def infer_config(sd: Mapping[str, torch.Tensor]) -> Dict[str, object]:
    """The model's sizes from the shapes and names of an ldm UNet state dict (bare keys)."""
    mc, cin = _shape(sd, "input_blocks.0.0.weight", 4)[:2]
    rx = re.compile(r"input_blocks\.(\d+)\.")
    n_in = max((int(m.group(1)) for m in (rx.match(k) for k in sd) if m), default=0) + 1
    mult: List[int] = []
    attn: List[bool] = []
    per_level: List[int] = []
    count = 0
    for i in range(1, n_in):
        if f"input_blocks.{i}.0.op.weight" in sd:                # a down-sampling: the level ends
            per_level.append(count)
            count = 0
            continue
        key = f"input_blocks.{i}.0.in_layers.2.weight"
        cout = _shape(sd, key, 4)[0]
        if count == 0:
            if cout % mc:
                raise ValueError(f"MultiviewUNet: key '{key}' has {cout} output channels, no multiple of model_channels = {mc}")
            mult.append(cout // mc)
            attn.append(f"input_blocks.{i}.1.norm.weight" in sd)
        count += 1
    per_level.append(count)
    if not mult or len(set(per_level)) != 1 or per_level[0] < 1:
        raise ValueError(f"MultiviewUNet: input_blocks have {per_level} ResBlocks on their levels: need the same number, at least 1, on each")
    cam = _shape(sd, "camera_embed.0.weight", 2)[1] if "camera_embed.0.weight" in sd else 0
    ctx = _shape(sd, "middle_block.1.transformer_blocks.0.attn2.to_k.weight", 2)[1]
    return dict(in_channels=cin, out_channels=_shape(sd, "out.2.weight", 4)[0], model_channels=mc, channel_mult=tuple(mult),
                num_res_blocks=per_level[0], attention=tuple(attn), context_dim=ctx, camera_dim=cam,
                with_ip="middle_block.1.transformer_blocks.0.attn2.to_k_ip.weight" in sd)


def _res(p: str, cin: int, cout: int, E: int):
    out = [(p + "in_layers.0.weight", (cin,)), (p + "in_layers.0.bias", (cin,)), (p + "in_layers.2.weight", (cout, cin, 3, 3)),
           (p + "in_layers.2.bias", (cout,)), (p + "emb_layers.1.weight", (cout, E)), (p + "emb_layers.1.bias", (cout,)),
           (p + "out_layers.0.weight", (cout,)), (p + "out_layers.0.bias", (cout,)), (p + "out_layers.3.weight", (cout, cout, 3, 3)),
           (p + "out_layers.3.bias", (cout,))]
    if cin != cout:
        out += [(p + "skip_connection.weight", (cout, cin, 1, 1)), (p + "skip_connection.bias", (cout,))]
    return out


def _tr(p: str, C_: int, ctx: int, with_ip: bool):
    b = p + "transformer_blocks.0."
    out = [(p + "norm.weight", (C_,)), (p + "norm.bias", (C_,)), (p + "proj_in.weight", (C_, C_)), (p + "proj_in.bias", (C_,)),
           (b + "norm1.weight", (C_,)), (b + "norm1.bias", (C_,)), (b + "attn1.to_q.weight", (C_, C_)), (b + "attn1.to_k.weight", (C_, C_)),
           (b + "attn1.to_v.weight", (C_, C_)), (b + "attn1.to_out.0.weight", (C_, C_)), (b + "attn1.to_out.0.bias", (C_,)),
           (b + "norm2.weight", (C_,)), (b + "norm2.bias", (C_,)), (b + "attn2.to_q.weight", (C_, C_)), (b + "attn2.to_k.weight", (C_, ctx)),
           (b + "attn2.to_v.weight", (C_, ctx))]
    if with_ip:
        out += [(b + "attn2.to_k_ip.weight", (C_, ctx)), (b + "attn2.to_v_ip.weight", (C_, ctx))]
    return out + [(b + "attn2.to_out.0.weight", (C_, C_)), (b + "attn2.to_out.0.bias", (C_,)), (b + "norm3.weight", (C_,)), (b + "norm3.bias", (C_,)),
                  (b + "ff.net.0.proj.weight", (8 * C_, C_)), (b + "ff.net.0.proj.bias", (8 * C_,)), (b + "ff.net.2.weight", (C_, 4 * C_)),
                  (b + "ff.net.2.bias", (C_,)), (p + "proj_out.weight", (C_, C_)), (p + "proj_out.bias", (C_,))]


def tensor_keys(cfg: Mapping[str, object]) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor the kernels read, in the order of the packed buffer (csrc/unet.hip make_plan)."""
    mc, mult, nrb, ctx, ip = cfg["model_channels"], cfg["channel_mult"], cfg["num_res_blocks"], cfg["context_dim"], cfg["with_ip"]
    E = 4 * mc
    out = [("time_embed.0.weight", (E, mc)), ("time_embed.0.bias", (E,)), ("time_embed.2.weight", (E, E)), ("time_embed.2.bias", (E,))]
    if cfg["camera_dim"]:
        out += [("camera_embed.0.weight", (E, cfg["camera_dim"])), ("camera_embed.0.bias", (E,)), ("camera_embed.2.weight", (E, E)),
                ("camera_embed.2.bias", (E,))]
    out += [("input_blocks.0.0.weight", (mc, cfg["in_channels"], 3, 3)), ("input_blocks.0.0.bias", (mc,))]
    chans, ch, i = [mc], mc, 1
    for l, m in enumerate(mult):
        for _ in range(nrb):
            out += _res(f"input_blocks.{i}.0.", ch, mc * m, E)
            ch = mc * m
            if cfg["attention"][l]:
                out += _tr(f"input_blocks.{i}.1.", ch, ctx, ip)
            chans.append(ch)
            i += 1
        if l != len(mult) - 1:
            out += [(f"input_blocks.{i}.0.op.weight", (ch, ch, 3, 3)), (f"input_blocks.{i}.0.op.bias", (ch,))]
            chans.append(ch)
            i += 1
    out += _res("middle_block.0.", ch, ch, E) + _tr("middle_block.1.", ch, ctx, ip) + _res("middle_block.2.", ch, ch, E)
    i = 0
    for l in reversed(range(len(mult))):
        for r in range(nrb + 1):
            out += _res(f"output_blocks.{i}.0.", ch + chans.pop(), mc * mult[l], E)
            ch = mc * mult[l]
            if cfg["attention"][l]:
                out += _tr(f"output_blocks.{i}.1.", ch, ctx, ip)
            if l > 0 and r == nrb:
                j = 2 if cfg["attention"][l] else 1
                out += [(f"output_blocks.{i}.{j}.conv.weight", (ch, ch, 3, 3)), (f"output_blocks.{i}.{j}.conv.bias", (ch,))]
            i += 1
    return out + [("out.0.weight", (ch,)), ("out.0.bias", (ch,)), ("out.2.weight", (cfg["out_channels"], ch, 3, 3)), ("out.2.bias", (cfg["out_channels"],))]


def block_names(cfg: Mapping[str, object]) -> List[str]:
    """The blocks in the order they run -- ``input_blocks.i``, ``middle_block``, ``output_blocks.i`` -- which is the block number of a
    probe."""
    n_in = 1 + len(cfg["channel_mult"]) * cfg["num_res_blocks"] + len(cfg["channel_mult"]) - 1
    n_out = len(cfg["channel_mult"]) * (cfg["num_res_blocks"] + 1)
    return [f"input_blocks.{i}" for i in range(n_in)] + ["middle_block"] + [f"output_blocks.{i}" for i in range(n_out)]


def normalize_camera(c2w: torch.Tensor) -> torch.Tensor:
    """ImageDream's ``camera_utils.normalize_camera``: ``[B,4,4]`` (or ``[B,16]``) -> ``[B,16]``, the translation column divided by
    (its norm + 1e-8), flattened row-major."""
    m = c2w.reshape(-1, 4, 4)
    t = m[:, :3, 3]
    out = m.clone()
    out[:, :3, 3] = t / (t.norm(dim=1, keepdim=True) + 1e-8)
    return out.reshape(-1, 16)


class MultiviewUNet(nn.Module):
    """The UNet in eval mode from its state dict.  The weights are one frozen flat float32 buffer (``weights``, the tensors of
    ``tensor_keys`` one behind the other; move the module with ``.to(device)``), packed for the kernels once per device on first use.
    ``num_head_channels``, ``ip_dim`` (image tokens), ``ip_weight`` and ``n_view`` are what no shape shows.

    ``precision``: ``"f32"`` (the default), ``"bf16"`` or ``"f16"``.  With a 16-bit precision the packed copy holds the convolutions'
    and linear layers' weights rounded to that type and every product rounds its activations to it as they are loaded, accumulating
    in float32; ``weights``, the activations in memory, the norms, inputs, outputs and probes stay float32, and what the float32
    path promises bit for bit (equal runs, groups independent of the batch, any strides of ``x``) holds as well.

    ``attention_precision``: ``"f32"`` (the default), ``"bf16"`` or ``"f16"``, independent of ``precision``.  With a 16-bit type
    both attentions round ``q scale``, ``k``, ``v`` and the softmax's ``p`` (as the operand of ``p v`` only) to it inside the kernel
    and run their two products on the 16-bit matrix core; the softmax, every sum and everything in memory stay float32
    (``attention`` below states the rule), and the same bit-for-bit promises hold."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor], num_head_channels: int = 64, ip_dim: int = 16, ip_weight: float = 1.0,
                 n_view: int = 4, precision: str = "f32", attention_precision: str = "f32"):
        super().__init__()
        if precision not in PRECISIONS:
            raise ValueError(f"MultiviewUNet: precision must be one of 'f32', 'bf16', 'f16' (got {precision!r})")
        attn_code = precision_code("MultiviewUNet", "attention_precision", attention_precision)
        self.precision, self.attention_precision = precision, attention_precision
        sd = strip_prefix(state_dict)
        cfg = infer_config(sd)
        cfg.update(num_head_channels=int(num_head_channels), ip_dim=int(ip_dim), ip_weight=float(ip_weight), n_view=int(n_view))
        keys = tensor_keys(cfg)
        problems = []
        for key, shape in keys:
            if key not in sd:
                problems.append(f"missing key '{key}' (expected shape {list(shape)})")
            elif not isinstance(sd[key], torch.Tensor) or tuple(sd[key].shape) != tuple(shape):
                problems.append(f"key '{key}' has shape {list(getattr(sd[key], 'shape', ()))}, expected {list(shape)}")
        if problems:
            missing = all(p.startswith("missing") for p in problems)
            raise (KeyError if missing else ValueError)("MultiviewUNet: " + "; ".join(problems))
        if len(cfg["channel_mult"]) > hip_lib.UNET_MAX_LEVELS:
            raise ValueError(f"MultiviewUNet: {len(cfg['channel_mult'])} levels: at most {hip_lib.UNET_MAX_LEVELS}")
        c = hip_lib.SoarUnetConfig()
        c.in_channels, c.out_channels, c.model_channels = cfg["in_channels"], cfg["out_channels"], cfg["model_channels"]
        c.levels, c.num_res_blocks = len(cfg["channel_mult"]), cfg["num_res_blocks"]
        for l, (m, a) in enumerate(zip(cfg["channel_mult"], cfg["attention"])):
            c.channel_mult[l], c.attention[l] = m, int(a)
        c.context_dim, c.camera_dim, c.with_ip = cfg["context_dim"], cfg["camera_dim"], int(cfg["with_ip"])
        c.head_channels, c.n_view, c.precision = cfg["num_head_channels"], cfg["n_view"], PRECISIONS[precision]
        c.attn_precision = attn_code
        nb, cnt, nf = C.c_size_t(0), C.c_int32(0), C.c_size_t(0)
        check(hip_lib.lib().soar_unet_weights_bytes(C.byref(c), C.byref(nb), C.byref(cnt), C.byref(nf)), "soar_unet_weights_bytes")
        self._sizes = [int(np.prod(shape)) for _, shape in keys]
        if cnt.value != len(keys) or nf.value != sum(self._sizes):
            raise RuntimeError(f"MultiviewUNet: the library packs {cnt.value} tensors of {nf.value} floats, tensor_keys lists {len(keys)} "
                               f"of {sum(self._sizes)}")
        self.cfg, self._c, self._packed_bytes = cfg, c, nb.value
        self.blocks = block_names(cfg)
        self.register_buffer("weights", torch.cat([sd[k].detach().to(torch.float32).reshape(-1) for k, _ in keys]).contiguous())
        self._pack = hip_lib.PackedWeights()
        self.eval()

    def _packed(self, dev) -> torch.Tensor:
        w = self.weights

        def pack():
            offs = np.concatenate([[0], np.cumsum(self._sizes)[:-1]])
            arr = (C.c_void_p * len(offs))(*[w.data_ptr() + 4 * int(o) for o in offs])
            sizes = (C.c_int64 * len(offs))(*self._sizes)
            packed = _workspace(self._packed_bytes, dev)
            with torch.cuda.device(dev):
                check(hip_lib.lib().soar_unet_pack_weights(C.byref(self._c), arr, sizes, len(offs), packed.data_ptr(), self._packed_bytes,
                                                           _stream(dev)), "soar_unet_pack_weights")
            return packed

        return self._pack.get([w], dev, f"MultiviewUNet: weights are on {w.device}, the input on {dev}: move the module with .to('{dev}')", pack)

    def probe_code(self, block: str, stage: str) -> int:
        """The code of ``stage`` (a key of ``STAGES``) of ``block`` (``input_blocks.3``, ``middle_block``, ``output_blocks.0``), or of
        ``("emb", "")``."""
        if block == "emb":
            return hip_lib.UNET_PROBE_EMB
        return 8 * self.blocks.index(block) + STAGES[stage]

    def level_sizes(self, h: int, w: int) -> List[Tuple[int, int]]:
        """(h, w) of every level; an odd side at a level that is down-sampled raises, naming the level."""
        out = []
        for l in range(len(self.cfg["channel_mult"])):
            out.append((h, w))
            if l != len(self.cfg["channel_mult"]) - 1:
                if h % 2 or w % 2:
                    raise ValueError(f"MultiviewUNet: level {l} is {h} x {w}: an odd side cannot be down-sampled and up-sampled back "
                                     f"(latents {out[0][0]} x {out[0][1]})")
                h, w = h // 2, w // 2
        return out

    @staticmethod
    def _need_hip(name: str, t, dev=None) -> None:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"MultiviewUNet: {name} must be a torch.Tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise RuntimeError(f"MultiviewUNet: {name} is on '{t.device}': soar_amd.unet runs on HIP devices only; there is no CPU fallback")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"MultiviewUNet: {name} is on {t.device}, x on {dev}")

    @torch.no_grad()
    def forward(self, x: torch.Tensor, t: torch.Tensor, context: torch.Tensor, camera: Optional[torch.Tensor] = None,
                ip_tokens: Optional[torch.Tensor] = None, probes: Optional[Sequence[Tuple[str, str]]] = None,
                workspace: Optional[torch.Tensor] = None):
        """x ``[N,4,h,w]`` (any strides), t ``[N]`` (any number type, read on the device), context ``[N,T,ctx]``, camera
        ``[N,camera_dim]``, ip_tokens ``[N,ip_dim,ctx]`` -> eps ``[N,4,h,w]`` (channels-last in memory).  ``N`` is a multiple of
        ``n_view``; a group's result does not depend on the rest of the batch.  ``probes``: (block, stage) pairs -> also a dict of
        those stages' activations, ``[N,C,h_l,w_l]`` (``("emb", "")``: ``[N,4 model_channels]``)."""
        cfg = self.cfg
        self._need_hip("x", x)
        dev = x.device
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != cfg["in_channels"]:
            raise ValueError(f"MultiviewUNet: x must be float32 [N,{cfg['in_channels']},h,w] (got {x.dtype} {list(x.shape)})")
        N, _, h, w = x.shape
        if N % cfg["n_view"]:
            raise ValueError(f"MultiviewUNet: N = {N} is not a multiple of n_view = {cfg['n_view']}")
        sizes = self.level_sizes(h, w)
        self._need_hip("t", t, dev)
        if tuple(t.shape) != (N,):
            raise ValueError(f"MultiviewUNet: t must be [N] = [{N}] (got {list(t.shape)})")
        self._need_hip("context", context, dev)
        if context.dim() != 3 or context.shape[0] != N or context.shape[1] < 1 or context.shape[2] != cfg["context_dim"]:
            raise ValueError(f"MultiviewUNet: context must be [N,T,{cfg['context_dim']}] with N = {N} (got {list(context.shape)})")
        if camera is not None:
            if not cfg["camera_dim"]:
                raise ValueError("MultiviewUNet: a camera is given, but the weights have no camera_embed")
            self._need_hip("camera", camera, dev)
            if tuple(camera.shape) != (N, cfg["camera_dim"]):
                raise ValueError(f"MultiviewUNet: camera must be [N,{cfg['camera_dim']}] with N = {N} (got {list(camera.shape)})")
            camera = camera.to(torch.float32).contiguous()
        elif cfg["camera_dim"]:
            raise ValueError("MultiviewUNet: the weights have camera_embed, but no camera is given")
        if ip_tokens is not None:
            if not cfg["with_ip"]:
                raise ValueError("MultiviewUNet: image tokens are given, but the weights have no attn2.to_k_ip")
            self._need_hip("ip_tokens", ip_tokens, dev)
            if tuple(ip_tokens.shape) != (N, cfg["ip_dim"], cfg["context_dim"]):
                raise ValueError(f"MultiviewUNet: ip_tokens must be [N,{cfg['ip_dim']},{cfg['context_dim']}] with N = {N} (got {list(ip_tokens.shape)})")
            ip_tokens = ip_tokens.to(torch.float32).contiguous()
        context = context.to(torch.float32).contiguous()
        t = t.to(torch.float32).contiguous()
        T, n_ip = context.shape[1], 0 if ip_tokens is None else cfg["ip_dim"]
        eps = torch.empty((N, h, w, cfg["out_channels"]), dtype=torch.float32, device=dev)
        a = hip_lib.SoarUnetArgs()
        a.N, a.H, a.W, a.T, a.n_ip, a.ip_weight = N, h, w, T, n_ip, cfg["ip_weight"]
        a.x, a.t, a.context, a.eps = x.data_ptr(), t.data_ptr(), context.data_ptr(), eps.data_ptr()
        for i, s in enumerate(x.stride()):
            a.x_stride[i] = s
        a.camera = None if camera is None else camera.data_ptr()
        a.ip_tokens = None if ip_tokens is None else ip_tokens.data_ptr()
        taps = {}
        probes = list(probes or [])
        if len(probes) > hip_lib.UNET_MAX_PROBES:
            raise ValueError(f"MultiviewUNet: {len(probes)} probes: at most {hip_lib.UNET_MAX_PROBES}")
        for i, (block, stage) in enumerate(probes):
            taps[(block, stage)] = self._probe_buffer(block, stage, N, sizes, dev)
            a.probe_code[i], a.probe_dst[i] = self.probe_code(block, stage), taps[(block, stage)].data_ptr()
        a.n_probes = len(probes)
        if N:
            packed = self._packed(dev)
            L = hip_lib.lib()
            need = _bytes(L.soar_unet_workspace_bytes, "soar_unet_workspace_bytes", C.byref(self._c), N, h, w, T, n_ip)
            ws = _workspace(need, dev) if workspace is None else workspace
            with torch.cuda.device(dev):
                check(L.soar_unet_forward(C.byref(self._c), packed.data_ptr(), C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)),
                      "soar_unet_forward")
        eps = eps.permute(0, 3, 1, 2)
        if not probes:
            return eps
        return eps, {k: (v if v.dim() == 2 else v.permute(0, 3, 1, 2)) for k, v in taps.items()}

    def _probe_buffer(self, block: str, stage: str, N: int, sizes, dev) -> torch.Tensor:
        cfg = self.cfg
        mc, mult, nrb = cfg["model_channels"], cfg["channel_mult"], cfg["num_res_blocks"]
        if block == "emb":
            return torch.zeros((N, 4 * mc), dtype=torch.float32, device=dev)
        # (level of the input, input channels, output channels, down-sampling?) of every block, in the order of ``blocks``
        info, chans, ch = [(0, cfg["in_channels"], mc, False)], [mc], mc
        for l, m in enumerate(mult):
            for _ in range(nrb):
                info.append((l, ch, mc * m, False))
                ch = mc * m
                chans.append(ch)
            if l != len(mult) - 1:
                info.append((l, ch, ch, True))
                chans.append(ch)
        info.append((len(mult) - 1, ch, ch, False))
        for l in reversed(range(len(mult))):
            for _ in range(nrb + 1):
                info.append((l, ch + chans.pop(), mc * mult[l], False))
                ch = mc * mult[l]
        l, cin, cout, down = info[self.blocks.index(block)]
        hh, ww = sizes[l]
        if stage == "cat":
            return torch.zeros((N, hh, ww, cin), dtype=torch.float32, device=dev)
        if stage == "up":
            return torch.zeros((N, 2 * hh, 2 * ww, cout), dtype=torch.float32, device=dev)
        if down:
            return torch.zeros((N, hh // 2, ww // 2, cout), dtype=torch.float32, device=dev)
        return torch.zeros((N, hh, ww, cout), dtype=torch.float32, device=dev)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None, k2: Optional[torch.Tensor] = None,
              v2: Optional[torch.Tensor] = None, w2: float = 1.0, precision: str = "f32") -> torch.Tensor:
    """The attention kernel by itself (csrc/attention.hip): q ``[B,Lq,heads hd]``, k, v ``[B,Lk,heads hd]`` (rows may be views into wider
    rows: the last axis contiguous, pitches multiples of 4) -> ``softmax(scale q k^T) v`` per head ``[B,Lq,heads hd]``, plus ``w2``
    times the same with ``k2, v2 [B,Lk2,heads hd]``.

    ``precision="bf16"`` / ``"f16"``: the 16-bit kernel (``soar_attention16``).  Tensors stay float32; inside, ``q scale`` (computed
    in float32), ``k`` and ``v`` are rounded to the type, nearest even, the scores and the softmax are float32 (its sum runs over the
    unrounded ``p``), and ``p`` is rounded only as the operand of ``p v``, which accumulates in float32."""
    code = precision_code("attention", "precision", precision)
    ts = [q, k, v] + ([k2, v2] if k2 is not None else [])
    for t in ts:
        MultiviewUNet._need_hip("q, k, v", t, q.device)
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != q.shape[0] or t.shape[2] != q.shape[2] or t.stride(2) != 1 or \
                (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
            raise ValueError("attention: q, k, v must be float32 [B,L,heads hd] with the last axis contiguous and batches one behind the other")
    B, Lq, Cw = q.shape
    hd = Cw // heads
    out = torch.empty((B, Lq, Cw), dtype=torch.float32, device=q.device)
    a = hip_lib.SoarUnetAttnArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), Cw
    a.B, a.Lq, a.Lk, a.heads, a.hd = B, Lq, k.shape[1], heads, hd
    a.scale, a.w2 = float(hd) ** -0.5 if scale is None else float(scale), float(w2)
    if k2 is not None:
        a.k2, a.v2, a.ldk2, a.ldv2, a.Lk2 = k2.data_ptr(), v2.data_ptr(), k2.stride(1), v2.stride(1), k2.shape[1]
    with torch.cuda.device(q.device):
        if code:
            check(hip_lib.lib().soar_attention16(C.byref(a), code, 0, _stream(q.device)), "soar_attention16")
        else:
            check(hip_lib.lib().soar_unet_attention(C.byref(a), _stream(q.device)), "soar_unet_attention")
    return out
