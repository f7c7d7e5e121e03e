"""The SDS guidance's conditioning on HIP kernels (csrc/clip.hip, csrc/attention.hip): CLIP's text encoder, its ViT image
encoder and IP-Adapter's image-token ``Resampler`` as ImageDream ships them, forward only, in float32 or -- ``precision="bf16"`` /
``"f16"`` -- with every matrix product on the 16-bit matrix core and, independently -- ``attention_precision`` -- the
attention there too.

``ClipTextEncoder(state_dict)`` and ``ClipImageEncoder(state_dict)`` take transformers' or open_clip's keys (detected from the keys, under
their usual prefixes); ``Resampler(state_dict)`` takes IP-Adapter's, with or without ``image_embed.``.  Other keys are ignored, a missing
or misshapen key raises, naming it, and the sizes are read from the shapes.  ``encode_prompts`` gives ``MultiviewGuidance`` its
``text_embeddings`` and ``ImageTokens`` is its ``image_tokens`` callable.  Tokenisation stays the caller's.

Neither ``open_clip`` nor ``imagedream`` is needed -- and neither was available to check against: DESIGN.md 9x states the definitions
that were built.  **Which hidden state ImageDream's ``encode_image_with_transformer`` hands to the Resampler could not be checked; the
defaults (all blocks, no ``ln_post``) are stated from the published code from memory**, which is why ``skip_last`` and ``post_norm`` are
arguments.

HIP only: CPU tensors are refused, there is no CPU fallback and no gradient.
"""
from __future__ import annotations

import ctypes as C
import math
import re
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check
from .unet import precision_code

# the twelve tensors of a block in the packed order (csrc/clip.hip clip_plan): canonical name -> transformers' name
_BLOCK = [("ln_1.weight", "layer_norm1.weight"), ("ln_1.bias", "layer_norm1.bias"), ("attn.in_proj_weight", None), ("attn.in_proj_bias", None),
          ("attn.out_proj.weight", "self_attn.out_proj.weight"), ("attn.out_proj.bias", "self_attn.out_proj.bias"),
          ("ln_2.weight", "layer_norm2.weight"), ("ln_2.bias", "layer_norm2.bias"), ("mlp.c_fc.weight", "mlp.fc1.weight"),
          ("mlp.c_fc.bias", "mlp.fc1.bias"), ("mlp.c_proj.weight", "mlp.fc2.weight"), ("mlp.c_proj.bias", "mlp.fc2.bias")]
STAGES = {"attn": 0, "block": 1}
IMAGE_MEAN = (0.48145466, 0.4578275, 0.40821073)
IMAGE_STD = (0.26862954, 0.26130258, 0.27577711)


def _need_hip(who: str, name: str, t, dev=None) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch.Tensor (got {type(t).__name__})")
    if not t.is_cuda:
        raise RuntimeError(f"{who}: {name} is on '{t.device}': soar_amd.clip runs on HIP devices only; there is no CPU fallback")
    if dev is not None and t.device != dev:
        raise RuntimeError(f"{who}: {name} is on {t.device}, expected {dev}")


def _prefix(sd: Mapping[str, torch.Tensor], suffix: str, but_not: str = "") -> Optional[str]:
    """What stands in front of ``suffix`` in the first key that ends with it (and not with ``but_not``)"""
    for k in sd:
        if k.endswith(suffix) and not (but_not and k.endswith(but_not)):
            return k[:-len(suffix)]
    return None


class _Keys:
    """Collects the tensors of a packed layout from a state dict, and every missing or misshapen key on the way."""

    def __init__(self, who: str, sd: Mapping[str, torch.Tensor]):
        self.who, self.sd, self.problems, self.tensors, self.names = who, sd, [], [], []

    def shape(self, key: str, ndim: int) -> Tuple[int, ...]:
        if key not in self.sd:
            raise KeyError(f"{self.who}: missing key '{key}'")
        s = tuple(getattr(self.sd[key], "shape", ()))
        if len(s) != ndim:
            raise ValueError(f"{self.who}: key '{key}' has shape {list(s)}, expected {ndim} dimensions")
        return s

    def get(self, key: str, shape: Sequence[int]) -> Optional[torch.Tensor]:
        t = self.sd.get(key)
        if t is None:
            self.problems.append(f"missing key '{key}' (expected shape {list(shape)})")
        elif not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
            self.problems.append(f"key '{key}' has shape {list(getattr(t, 'shape', ()))}, expected {list(shape)}")
        else:
            return t.detach().to(torch.float32)
        return None

    def add(self, name: str, key: str, shape: Sequence[int]) -> None:
        self.names.append(name)
        self.tensors.append(self.get(key, shape))

    def add_cat(self, name: str, keys: Sequence[str], shape: Sequence[int]) -> None:
        parts = [self.get(k, shape) for k in keys]
        self.names.append(name)
        self.tensors.append(None if any(p is None for p in parts) else torch.cat(parts))

    def blocks(self, pre: str, hf: bool, layers: int, W: int, mlp: int) -> None:
        shapes = [(W,), (W,), (3 * W, W), (3 * W,), (W, W), (W,), (W,), (W,), (mlp, W), (mlp,), (W, mlp), (W,)]
        for i in range(layers):
            p = f"{pre}encoder.layers.{i}." if hf else f"{pre}transformer.resblocks.{i}."
            for (name, hf_name), shape in zip(_BLOCK, shapes):
                if not hf:
                    self.add(f"blocks.{i}.{name}", p + name, shape)
                elif hf_name is not None:
                    self.add(f"blocks.{i}.{name}", p + hf_name, shape)
                else:                                            # q | k | v is one product
                    kind = "weight" if name.endswith("weight") else "bias"
                    self.add_cat(f"blocks.{i}.{name}", [f"{p}self_attn.{x}_proj.{kind}" for x in "qkv"], (W,) + tuple(shape[1:]))

    def done(self) -> List[torch.Tensor]:
        if self.problems:
            missing = all(p.startswith("missing") for p in self.problems)
            raise (KeyError if missing else ValueError)(f"{self.who}: " + "; ".join(self.problems))
        return self.tensors


def _count_blocks(sd, pre: str, hf: bool) -> int:
    rx = re.compile(re.escape(pre) + (r"encoder\.layers\.(\d+)\." if hf else r"transformer\.resblocks\.(\d+)\."))
    return max((int(m.group(1)) for m in (rx.match(k) for k in sd) if m), default=-1) + 1


class _Packed(nn.Module):
    """A network whose weights are one frozen flat float32 buffer (``weights``: the tensors of the packed order one behind the other;
    move the module with ``.to(device)``), packed for the kernels once per device on first use.

    ``precision``: ``"f32"`` (the default), ``"bf16"`` or ``"f16"``.  With a 16-bit precision the module's packed copy holds the
    linear layers' (and the patch convolution's) weights rounded to that type and every product rounds its activations to it as they
    are loaded, accumulating in float32.  ``attention_precision``, independently: the attention rounds ``q scale``, ``k``, ``v`` and
    the softmax's ``p`` (as the operand of ``p v`` only) to the type inside the kernel.  ``weights``, embeddings, biases, norms, the
    softmax, everything in memory and the probes stay float32, and what the float32 path promises bit for bit holds as well."""
    who = ""
    _pack_fn = _bytes_fn = ""

    def _precisions(self, precision: str, attention_precision: str) -> None:
        self._codes = (precision_code(self.who, "precision", precision), precision_code(self.who, "attention_precision", attention_precision))
        self.precision, self.attention_precision = precision, attention_precision

    def _set_weights(self, tensors: List[torch.Tensor], names: List[str]) -> None:
        L = hip_lib.lib()
        nb, cnt, nf = C.c_size_t(0), C.c_int32(0), C.c_size_t(0)
        check(getattr(L, self._bytes_fn)(C.byref(self._c), C.byref(nb), C.byref(cnt), C.byref(nf)), self._bytes_fn)
        self._sizes = [int(t.numel()) for t in tensors]
        if cnt.value != len(tensors) or nf.value != sum(self._sizes):
            raise RuntimeError(f"{self.who}: the library packs {cnt.value} tensors of {nf.value} floats, this module lists {len(tensors)} "
                               f"of {sum(self._sizes)}")
        self.tensor_names, self._packed_bytes = names, nb.value
        self.register_buffer("weights", torch.cat([t.reshape(-1) for t in tensors]).contiguous())
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
                check(getattr(hip_lib.lib(), self._pack_fn)(C.byref(self._c), arr, sizes, len(offs), packed.data_ptr(), self._packed_bytes,
                                                           _stream(dev)), self._pack_fn)
            return packed

        return self._pack.get([w], dev, f"{self.who}: weights are on {w.device}, the input on {dev}: move the module with .to('{dev}')", pack)

    def _probes(self, args, probes, codes, shape, dev) -> Dict:
        probes = list(probes or [])
        if len(probes) > hip_lib.CLIP_MAX_PROBES:
            raise ValueError(f"{self.who}: {len(probes)} probes: at most {hip_lib.CLIP_MAX_PROBES}")
        taps = {}
        for i, key in enumerate(probes):
            taps[key] = torch.zeros(shape, dtype=torch.float32, device=dev)
            args.probe_code[i], args.probe_dst[i] = codes(key), taps[key].data_ptr()
        args.n_probes = len(probes)
        return taps


class _Tower(_Packed):
    """What the two encoders share: the configuration, the blocks' probes and the call."""
    _pack_fn, _bytes_fn = "soar_clip_pack_weights", "soar_clip_weights_bytes"

    def _configure(self, kind: int, W: int, heads: int, layers: int, mlp: int, tokens: int, vocab: int = 0, patch: int = 0, grid: int = 0,
                   hidden_act: str = "gelu") -> None:
        if hidden_act != "gelu":
            raise ValueError(f"{self.who}: hidden_act = '{hidden_act}': only the erf GELU ('gelu') is built; quick_gelu models are refused")
        if heads < 1 or W % heads:
            raise ValueError(f"{self.who}: width = {W} is no multiple of heads = {heads}")
        if layers > hip_lib.CLIP_MAX_LAYERS:
            raise ValueError(f"{self.who}: {layers} layers: at most {hip_lib.CLIP_MAX_LAYERS}")
        c = hip_lib.SoarClipConfig()
        c.kind, c.width, c.heads, c.layers, c.mlp, c.tokens, c.vocab, c.patch, c.grid = kind, W, heads, layers, mlp, tokens, vocab, patch, grid
        c.precision, c.attn_precision = self._codes
        self._c = c
        self.cfg = dict(width=W, heads=heads, head_dim=W // heads, layers=layers, mlp=mlp, tokens=tokens)

    def _skip(self, skip_last: int) -> int:
        if not 0 <= int(skip_last) <= self.cfg["layers"]:
            raise ValueError(f"{self.who}: skip_last = {skip_last} outside 0 .. {self.cfg['layers']}")
        return int(skip_last)

    def probe_code(self, key) -> int:
        """``("embed", "")``, ``("pre", "")`` (vision: after ``ln_pre``), ``(block, "attn")`` or ``(block, "block")``"""
        if key[0] == "embed":
            return hip_lib.CLIP_PROBE_EMBED
        if key[0] == "pre":
            return hip_lib.CLIP_PROBE_PRE
        return 2 * int(key[0]) + STAGES[key[1]]

    def _run(self, B: int, L: int, dev, ids, patches, final_norm: bool, probes, workspace):
        W = self.cfg["width"]
        out = torch.empty((B, L, W), dtype=torch.float32, device=dev)
        a = hip_lib.SoarClipArgs()
        a.B, a.L, a.run_layers, a.final_norm = B, L, self.cfg["layers"] - self.skip_last, int(final_norm)
        a.ids = None if ids is None else ids.data_ptr()
        a.patches = None if patches is None else patches.data_ptr()
        a.out = out.data_ptr()
        taps = self._probes(a, probes, self.probe_code, (B, L, W), dev)
        if B:
            packed = self._packed(dev)
            lib = hip_lib.lib()
            need = _bytes(lib.soar_clip_workspace_bytes, "soar_clip_workspace_bytes", C.byref(self._c), B, L)
            ws = _workspace(need, dev) if workspace is None else workspace
            with torch.cuda.device(dev):
                check(lib.soar_clip_forward(C.byref(self._c), packed.data_ptr(), C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)),
                      "soar_clip_forward")
        return (out, taps) if probes else out


class ClipTextEncoder(_Tower):
    """CLIP's text transformer: ``forward(input_ids [B, L]) -> [B, L, width]``, the final-normed hidden states of every position
    (``CLIPTextModel(ids)[0]`` / ldm's ``FrozenOpenCLIPEmbedder``), under a causal mask and no padding mask.

    ``skip_last``: final blocks not run -- default 0 for transformers' layout (SD-2.1's converted encoder has 23 layers), 1 for
    open_clip's (``layer="penultimate"`` of 24).  ``heads``: default width / 64.  ``hidden_act``: what the checkpoint's configuration
    says; anything but ``"gelu"`` is refused.  ``precision``, ``attention_precision``: ``"f32"`` (default), ``"bf16"``, ``"f16"``."""
    who = "ClipTextEncoder"

    def __init__(self, state_dict: Mapping[str, torch.Tensor], skip_last: Optional[int] = None, heads: Optional[int] = None,
                 hidden_act: str = "gelu", precision: str = "f32", attention_precision: str = "f32"):
        super().__init__()
        self._precisions(precision, attention_precision)
        sd = state_dict
        pre = _prefix(sd, "embeddings.token_embedding.weight")
        hf = pre is not None
        if not hf:
            pre = _prefix(sd, "token_embedding.weight")
            if pre is None:
                raise KeyError(f"{self.who}: missing key 'token_embedding.weight' (open_clip) or 'embeddings.token_embedding.weight' (transformers)")
        self.layout = "transformers" if hf else "open_clip"
        K = _Keys(self.who, sd)
        tok_key = pre + ("embeddings.token_embedding.weight" if hf else "token_embedding.weight")
        pos_key = pre + ("embeddings.position_embedding.weight" if hf else "positional_embedding")
        vocab, W = K.shape(tok_key, 2)
        ctx = K.shape(pos_key, 2)[0]
        layers = _count_blocks(sd, pre, hf)
        mlp = K.shape(pre + ("encoder.layers.0.mlp.fc1.weight" if hf else "transformer.resblocks.0.mlp.c_fc.weight"), 2)[0] if layers else W
        self._configure(hip_lib.CLIP_TEXT, W, W // 64 if heads is None else int(heads), layers, mlp, ctx, vocab=vocab, hidden_act=hidden_act)
        self.cfg.update(vocab=vocab, context=ctx)
        self.skip_last = self._skip((0 if hf else 1) if skip_last is None else skip_last)
        K.add("token_embedding.weight", tok_key, (vocab, W))
        K.add("positional_embedding", pos_key, (ctx, W))
        K.blocks(pre, hf, layers, W, mlp)
        fin = pre + ("final_layer_norm." if hf else "ln_final.")
        K.add("ln_final.weight", fin + "weight", (W,))
        K.add("ln_final.bias", fin + "bias", (W,))
        self._set_weights(K.done(), K.names)

    @torch.no_grad()
    def forward(self, input_ids: torch.Tensor, probes=None, workspace: Optional[torch.Tensor] = None):
        """input_ids ``[B, L]`` of any integer type, L at most the context length -> ``[B, L, width]``; a sequence's result does not
        depend on the rest of the batch.  The ids are checked against the vocabulary on the host before anything is launched (one
        read-back: the text encoder runs once per prompt, not per step).  ``probes``: keys of ``probe_code`` -> also a dict of those
        stages' tokens ``[B, L, width]``."""
        if not isinstance(input_ids, torch.Tensor) or input_ids.dim() != 2 or input_ids.is_floating_point() or input_ids.dtype == torch.bool:
            raise ValueError(f"{self.who}: input_ids must be an integer tensor [B, L] (got {getattr(input_ids, 'dtype', None)} "
                             f"{list(getattr(input_ids, 'shape', ()))})")
        B, L = input_ids.shape
        if not 1 <= L <= self.cfg["context"]:
            raise ValueError(f"{self.who}: L = {L} tokens: the position embedding has {self.cfg['context']}")
        if B:
            lo, hi = int(input_ids.min()), int(input_ids.max())
            if lo < 0 or hi >= self.cfg["vocab"]:
                raise ValueError(f"{self.who}: token id {lo if lo < 0 else hi} outside the vocabulary of {self.cfg['vocab']}")
        _need_hip(self.who, "input_ids", input_ids)
        ids = input_ids.to(torch.int32).contiguous()
        return self._run(B, L, ids.device, ids, None, True, probes, workspace)


def encode_prompts(encoder: ClipTextEncoder, prompt_ids: torch.Tensor, negative_ids: torch.Tensor) -> torch.Tensor:
    """``[2, L, width]``: the prompt's and the unconditional prompt's tokens in ``MultiviewGuidance``'s (text, uncond) order.  The ids
    (``[L]`` or ``[1, L]`` each, the same L) are the caller's tokenizer's."""
    ids = [t.reshape(1, -1) for t in (prompt_ids, negative_ids)]
    if ids[0].shape != ids[1].shape:
        raise ValueError(f"encode_prompts: the two prompts have {ids[0].shape[1]} and {ids[1].shape[1]} tokens: pad them to one length")
    return encoder(torch.cat(ids))


class ClipImageEncoder(_Tower):
    """CLIP's ViT: ``forward(images) -> [B, 1 + grid^2, width]``, the hidden states of all tokens (class token first) -- without
    ``visual.proj``: the Resampler takes hidden states.  ``skip_last`` final blocks are not run; ``post_norm``: ``ln_post`` on all
    tokens.  ``heads``: default width / 80 when width is 1280 (ViT-H), else width / 64.  ``precision``, ``attention_precision``:
    ``"f32"`` (default), ``"bf16"``, ``"f16"``."""
    who = "ClipImageEncoder"

    def __init__(self, state_dict: Mapping[str, torch.Tensor], skip_last: int = 0, post_norm: bool = False, heads: Optional[int] = None,
                 hidden_act: str = "gelu", precision: str = "f32", attention_precision: str = "f32"):
        super().__init__()
        self._precisions(precision, attention_precision)
        sd = state_dict
        pre = _prefix(sd, "embeddings.patch_embedding.weight")       # under vision_model., or bare as CLIPVisionModel saves it
        hf = pre is not None
        if not hf:
            pre = _prefix(sd, "visual.conv1.weight")
            if pre is None:
                raise KeyError(f"{self.who}: missing key 'visual.conv1.weight' (open_clip) or 'embeddings.patch_embedding.weight' (transformers)")
            pre += "visual."
        self.layout = "transformers" if hf else "open_clip"
        K = _Keys(self.who, sd)
        conv_key = pre + ("embeddings.patch_embedding.weight" if hf else "conv1.weight")
        pos_key = pre + ("embeddings.position_embedding.weight" if hf else "positional_embedding")
        W, cin, p, p2 = K.shape(conv_key, 4)
        T = K.shape(pos_key, 2)[0]
        g = math.isqrt(max(T - 1, 0))
        if cin != 3 or p != p2 or g < 1 or g * g != T - 1:
            raise ValueError(f"{self.who}: key '{conv_key}' has shape {[W, cin, p, p2]} and '{pos_key}' {T} rows: need 3 channels, square "
                             f"patches and 1 + a square number of positions")
        layers = _count_blocks(sd, pre, hf)
        mlp = K.shape(pre + ("encoder.layers.0.mlp.fc1.weight" if hf else "transformer.resblocks.0.mlp.c_fc.weight"), 2)[0] if layers else W
        if heads is None:
            heads = W // 80 if W == 1280 else W // 64
        self._configure(hip_lib.CLIP_VISION, W, int(heads), layers, mlp, T, patch=p, grid=g, hidden_act=hidden_act)
        self.cfg.update(patch=p, grid=g, image_size=g * p, patch_k=(3 * p * p + 7) // 8 * 8)
        self.skip_last, self.post_norm = self._skip(skip_last), bool(post_norm)
        K.add("conv1.weight", conv_key, (W, 3, p, p))
        K.add("class_embedding", pre + ("embeddings.class_embedding" if hf else "class_embedding"), (W,))
        K.add("positional_embedding", pos_key, (T, W))
        ln = pre + ("pre_layrnorm." if hf else "ln_pre.")
        K.add("ln_pre.weight", ln + "weight", (W,))
        K.add("ln_pre.bias", ln + "bias", (W,))
        K.blocks(pre, hf, layers, W, mlp)
        ln = pre + ("post_layernorm." if hf else "ln_post.")
        K.add("ln_post.weight", ln + "weight", (W,))
        K.add("ln_post.bias", ln + "bias", (W,))
        self._set_weights(K.done(), K.names)

    def resized(self, ref_rgb: torch.Tensor) -> torch.Tensor:
        """``[H, W, 3]`` / ``[B, H, W, 3]``, uint8 or float in 0 .. 1 -> uint8 ``[B, S, S, 3]``: ``to_pil_image`` (``mul(255)`` truncated
        to a byte) and ``Resize((S, S), BICUBIC)``, Pillow's bytes."""
        from .jpeg import resize_images
        _need_hip(self.who, "images", ref_rgb)
        x = ref_rgb[None] if ref_rgb.dim() == 3 else ref_rgb
        if x.dim() != 4 or x.shape[3] != 3 or not (x.dtype == torch.uint8 or x.is_floating_point()):
            raise ValueError(f"{self.who}: images must be [H, W, 3] or [B, H, W, 3], uint8 or float (got {ref_rgb.dtype} {list(ref_rgb.shape)})")
        if x.dtype != torch.uint8:
            x = x.detach().mul(255).to(torch.uint8)
        S = self.cfg["image_size"]
        return resize_images(x, S, S)

    @torch.no_grad()
    def preprocess(self, ref_rgb: torch.Tensor) -> torch.Tensor:
        """-> the patch product's rows ``[B, grid^2, Kp]``: ``resized`` bytes as ``(x / 255 - mean) / std``, one row per token in the
        patch convolution's (channel, y, x) order, padded from ``3 patch^2`` to a multiple of 8 with zeros"""
        u8 = self.resized(ref_rgb)
        B, g = u8.shape[0], self.cfg["grid"]
        rows = torch.empty((B, g * g, self.cfg["patch_k"]), dtype=torch.float32, device=u8.device)
        with torch.cuda.device(u8.device):
            check(hip_lib.lib().soar_clip_preprocess(C.byref(self._c), B, u8.data_ptr(), rows.data_ptr(), _stream(u8.device)), "soar_clip_preprocess")
        return rows

    @torch.no_grad()
    def forward(self, images: torch.Tensor, probes=None, workspace: Optional[torch.Tensor] = None):
        """images: what ``preprocess`` takes -> ``[B, 1 + grid^2, width]``; an image's result does not depend on the rest of the batch.
        ``probes``: keys of ``probe_code`` -> also a dict of those stages' tokens."""
        rows = self.preprocess(images)
        return self._run(rows.shape[0], self.cfg["tokens"], rows.device, None, rows, self.post_norm, probes, workspace)


def _resampler_prefix(sd) -> str:
    return "image_embed." if "image_embed.latents" in sd else ""


class Resampler(_Packed):
    """IP-Adapter's ``Resampler`` as ImageDream ships it (``image_embed.*``): ``forward(x [B, n, emb]) -> [B, queries, out]``.
    ``dim_head`` is what no shape shows; everything else is read from the shapes.  ``precision``, ``attention_precision``: ``"f32"``
    (default), ``"bf16"``, ``"f16"``."""
    who = "Resampler"
    _pack_fn, _bytes_fn = "soar_resampler_pack_weights", "soar_resampler_weights_bytes"

    def __init__(self, state_dict: Mapping[str, torch.Tensor], dim_head: int = 64, precision: str = "f32", attention_precision: str = "f32"):
        super().__init__()
        self._precisions(precision, attention_precision)
        sd = state_dict
        pre = _resampler_prefix(sd)
        K = _Keys(self.who, sd)
        one, nq, dim = K.shape(pre + "latents", 3)
        emb = K.shape(pre + "proj_in.weight", 2)[1]
        out = K.shape(pre + "proj_out.weight", 2)[0]
        rx = re.compile(re.escape(pre) + r"layers\.(\d+)\.")
        depth = max((int(m.group(1)) for m in (rx.match(k) for k in sd) if m), default=-1) + 1
        inner = K.shape(pre + "layers.0.0.to_q.weight", 2)[0] if depth else int(dim_head)
        ff = K.shape(pre + "layers.0.1.1.weight", 2)[0] if depth else dim
        if one != 1 or dim_head < 1 or inner % int(dim_head):
            raise ValueError(f"{self.who}: key '{pre}latents' has shape {[one, nq, dim]} and to_q {inner} rows: need [1, queries, dim] and "
                             f"a multiple of dim_head = {dim_head}")
        if depth > hip_lib.CLIP_MAX_LAYERS:
            raise ValueError(f"{self.who}: {depth} layers: at most {hip_lib.CLIP_MAX_LAYERS}")
        c = hip_lib.SoarResamplerConfig()
        c.dim, c.depth, c.heads, c.dim_head, c.queries, c.emb, c.out, c.ff = dim, depth, inner // int(dim_head), int(dim_head), nq, emb, out, ff
        c.precision, c.attn_precision = self._codes
        self._c = c
        self.cfg = dict(dim=dim, depth=depth, heads=c.heads, dim_head=int(dim_head), queries=nq, emb=emb, out=out, ff=ff)
        for name, shape in resampler_keys(self.cfg):
            K.add(name, pre + name, shape)
        self._set_weights(K.done(), K.names)

    def probe_code(self, key) -> int:
        """``(layer, "attn")`` or ``(layer, "ff")``: the latents ``[B, queries, dim]`` after that half of the layer"""
        return 2 * int(key[0]) + {"attn": 0, "ff": 1}[key[1]]

    @torch.no_grad()
    def forward(self, x: torch.Tensor, probes=None, workspace: Optional[torch.Tensor] = None):
        cfg = self.cfg
        _need_hip(self.who, "x", x)
        if x.dim() != 3 or x.shape[1] < 1 or x.shape[2] != cfg["emb"] or not x.is_floating_point():
            raise ValueError(f"{self.who}: x must be float [B, n, {cfg['emb']}] (got {x.dtype} {list(x.shape)})")
        x = x.detach().to(torch.float32).contiguous()
        B, n, dev = x.shape[0], x.shape[1], x.device
        out = torch.empty((B, cfg["queries"], cfg["out"]), dtype=torch.float32, device=dev)
        a = hip_lib.SoarResamplerArgs()
        a.B, a.n, a.x, a.out = B, n, x.data_ptr(), out.data_ptr()
        taps = self._probes(a, probes, self.probe_code, (B, cfg["queries"], cfg["dim"]), dev)
        if B:
            packed = self._packed(dev)
            lib = hip_lib.lib()
            need = _bytes(lib.soar_resampler_workspace_bytes, "soar_resampler_workspace_bytes", C.byref(self._c), B, n)
            ws = _workspace(need, dev) if workspace is None else workspace
            with torch.cuda.device(dev):
                check(lib.soar_resampler_forward(C.byref(self._c), packed.data_ptr(), C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)),
                      "soar_resampler_forward")
        return (out, taps) if probes else out


def resampler_keys(cfg: Mapping[str, int]) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of the Resampler's tensors in the order of the packed buffer (csrc/clip.hip resampler_plan)"""
    D, I, F = cfg["dim"], cfg["heads"] * cfg["dim_head"], cfg["ff"]
    out = [("latents", (1, cfg["queries"], D)), ("proj_in.weight", (D, cfg["emb"])), ("proj_in.bias", (D,)),
           ("proj_out.weight", (cfg["out"], D)), ("proj_out.bias", (cfg["out"],)), ("norm_out.weight", (cfg["out"],)), ("norm_out.bias", (cfg["out"],))]
    for i in range(cfg["depth"]):
        p = f"layers.{i}."
        out += [(p + "0.norm1.weight", (D,)), (p + "0.norm1.bias", (D,)), (p + "0.norm2.weight", (D,)), (p + "0.norm2.bias", (D,)),
                (p + "0.to_q.weight", (I, D)), (p + "0.to_kv.weight", (2 * I, D)), (p + "0.to_out.weight", (D, I)),
                (p + "1.0.weight", (D,)), (p + "1.0.bias", (D,)), (p + "1.1.weight", (F, D)), (p + "1.3.weight", (D, F))]
    return out


class ImageTokens(nn.Module):
    """``MultiviewGuidance``'s ``image_tokens``: ``ImageTokens(encoder, resampler)(ref_rgb) -> (cond [queries, ctx], zeros)`` for one
    image (``[H, W, 3]`` or ``[1, H, W, 3]``, uint8 or float in 0 .. 1): preprocess, encoder, Resampler; the reference's unconditional
    half is zeros.  Nothing is read back and the host does not wait for the device."""

    def __init__(self, image_encoder: ClipImageEncoder, resampler: Resampler):
        super().__init__()
        if resampler.cfg["emb"] != image_encoder.cfg["width"]:
            raise ValueError(f"ImageTokens: the Resampler takes {resampler.cfg['emb']} channels, the encoder gives {image_encoder.cfg['width']}")
        self.image_encoder, self.resampler = image_encoder, resampler

    @torch.no_grad()
    def forward(self, ref_rgb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if ref_rgb.dim() == 4 and ref_rgb.shape[0] != 1:
            raise ValueError(f"ImageTokens: one image, [H, W, 3] or [1, H, W, 3] (got {list(ref_rgb.shape)})")
        cond = self.resampler(self.image_encoder(ref_rgb))[0]
        return cond, torch.zeros_like(cond)


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: Optional[float] = None, causal: bool = False,
              precision: str = "f32") -> torch.Tensor:
    """The towers' attention kernel by itself (csrc/attention.hip): q ``[B, Lq, heads hd]``, k, v ``[B, Lk, heads hd]`` (rows may be views
    into wider rows: the last axis contiguous, pitches multiples of 4), hd a multiple of 4 up to 96 -> ``softmax(scale q k^T) v`` per
    head; ``causal``: key j counts for query i when j <= i.  ``precision="bf16"`` / ``"f16"``: the 16-bit kernel (``soar_attention16``;
    ``soar_amd.unet.attention`` states its rounding rule); tensors stay float32."""
    code = precision_code("attention", "precision", precision)
    for t in (q, k, v):
        _need_hip("attention", "q, k, v", t, q.device)
        if t.dtype != torch.float32 or t.dim() != 3 or t.shape[0] != q.shape[0] or t.shape[2] != q.shape[2] or t.stride(2) != 1 or \
                (t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
            raise ValueError("attention: q, k, v must be float32 [B,L,heads hd] with the last axis contiguous and batches one behind the other")
    B, Lq, Cw = q.shape
    hd = Cw // heads
    out = torch.empty((B, Lq, Cw), dtype=torch.float32, device=q.device)
    a = hip_lib.SoarClipAttnArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), Cw
    a.B, a.Lq, a.Lk, a.heads, a.hd, a.causal = B, Lq, k.shape[1], heads, hd, int(causal)
    a.scale = float(hd) ** -0.5 if scale is None else float(scale)
    with torch.cuda.device(q.device):
        if code:
            u = hip_lib.SoarUnetAttnArgs()
            u.q, u.k, u.v, u.out, u.ldq, u.ldk, u.ldv, u.ldo = a.q, a.k, a.v, a.out, a.ldq, a.ldk, a.ldv, a.ldo
            u.B, u.Lq, u.Lk, u.heads, u.hd, u.scale = a.B, a.Lq, a.Lk, a.heads, a.hd, a.scale
            check(hip_lib.lib().soar_attention16(C.byref(u), code, int(causal), _stream(q.device)), "soar_attention16")
        else:
            check(hip_lib.lib().soar_clip_attention(C.byref(a), _stream(q.device)), "soar_clip_attention")
    return out
