"""SAM (Segment Anything) for point prompts on HIP kernels (csrc/sam.hip): the segmenter of the mask stage.

``SamSegmenter(state_dict)`` takes the original checkpoint's state dict (``segment_anything``'s keys: ``image_encoder.*``,
``prompt_encoder.*``, ``mask_decoder.*``; ViT-B, -L and -H alike, the sizes are read from the shapes) and reproduces
``SamPredictor.set_image`` + ``predict(point_coords, point_labels, multimask_output=True)`` for a batch of frames, forward only, in
float32.  ``segment_anything`` is not needed.

* ``embed(images)``: uint8 ``[B,H,W,3]`` -> image embeddings ``[B,C,g,g]``.
* ``decode(embeddings, points, counts, orig_hw)`` -> ``(low_res_logits [B,3,4g,4g], iou [B,3])``.
* ``logits`` / ``masks``: the whole thing, ``[B,3,H,W]`` float32 / bool.
* ``segmenter(image, coords, labels)`` -> ``[3,H,W]`` logits of one frame: an instance is a ``predict`` for
  ``masks.segment_sequence``, which sees that and takes a batched path.

Points are ``(x, y)`` pixels of the original frame with labels 1 (foreground) / 0 (background); the frames of a batch may have
different numbers of points (``counts``), and a slot past a frame's count takes part in nothing.  Boxes and mask prompts raise
``NotImplementedError``.  HIP only: CPU tensors are refused, there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check

MAX_TOKENS = 64                    # decoder tokens per frame in the kernels: 1 + mask_tokens + points + 1


def _count(sd: Mapping[str, torch.Tensor], pattern: str) -> int:
    rx = re.compile(pattern)
    idx = {int(m.group(1)) for m in (rx.match(k) for k in sd) if m}
    return max(idx) + 1 if idx else 0


def _shape(sd, key: str, ndim: int) -> Tuple[int, ...]:
    if key not in sd:
        raise KeyError(f"SamSegmenter: missing key '{key}'")
    s = tuple(getattr(sd[key], "shape", ()))
    if len(s) != ndim:
        raise ValueError(f"SamSegmenter: key '{key}' has shape {list(s)}, expected {ndim} dimensions")
    return s


def infer_config(sd: Mapping[str, torch.Tensor]) -> Dict[str, object]:
    """The model's sizes from the shapes of a ``segment_anything`` state dict (never from a model name)."""
    _, g, g2, C_ = _shape(sd, "image_encoder.pos_embed", 4)
    patch = _shape(sd, "image_encoder.patch_embed.proj.weight", 4)[-1]
    depth = _count(sd, r"image_encoder\.blocks\.(\d+)\.")
    if depth < 1:
        raise KeyError("SamSegmenter: missing key 'image_encoder.blocks.0.norm1.weight' (no encoder blocks)")
    hd = _shape(sd, "image_encoder.blocks.0.attn.rel_pos_h", 2)[1]
    if g != g2 or hd < 1 or C_ % hd:
        raise ValueError(f"SamSegmenter: key 'image_encoder.pos_embed' has shape {[1, g, g2, C_]}: need a square grid and a width that "
                         f"head_dim = {hd} (the columns of rel_pos_h) divides")
    window, glob = 0, []
    for i in range(depth):
        key = f"image_encoder.blocks.{i}.attn.rel_pos_h"
        rows = _shape(sd, key, 2)[0]
        if rows == 2 * g - 1:
            glob.append(i)
            continue
        w = (rows + 1) // 2
        if rows % 2 == 0 or w > g or (window and w != window):
            raise ValueError(f"SamSegmenter: key '{key}' has {rows} rows: neither the grid's 2 x {g} - 1 nor the 2 S - 1 of a window S"
                             f"{f' = {window} like the other blocks' if window else ''}; tables are not interpolated")
        window = w
    P = _shape(sd, "image_encoder.neck.0.weight", 4)[0]
    dec = "mask_decoder.transformer.layers."
    inner = _shape(sd, dec + "0.cross_attn_token_to_image.q_proj.weight", 2)[0]
    if inner < 1 or P % inner:
        raise ValueError(f"SamSegmenter: key '{dec}0.cross_attn_token_to_image.q_proj.weight' has {inner} rows, which do not divide the width {P}")
    return dict(image_size=g * patch, patch=patch, embed=C_, depth=depth, heads=C_ // hd, window=window, global_blocks=tuple(glob),
                mlp=_shape(sd, "image_encoder.blocks.0.mlp.lin1.weight", 2)[0], out_chans=P, dec_layers=_count(sd, r"mask_decoder\.transformer\.layers\.(\d+)\."),
                dec_heads=8, dec_down=P // inner, dec_mlp=_shape(sd, dec + "0.mlp.lin1.weight", 2)[0],
                mask_tokens=_shape(sd, "mask_decoder.mask_tokens.weight", 2)[0],
                hyper_depth=_count(sd, r"mask_decoder\.output_hypernetworks_mlps\.0\.layers\.(\d+)\.weight"),
                iou_depth=_count(sd, r"mask_decoder\.iou_prediction_head\.layers\.(\d+)\.weight"),
                iou_hidden=_shape(sd, "mask_decoder.iou_prediction_head.layers.0.weight", 2)[0])


def tensor_keys(cfg: Mapping[str, object]) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key, shape) of every tensor the kernels read, in the order of the packed buffer (csrc/sam.hip make_layout)."""
    g, C_, P, p = cfg["image_size"] // cfg["patch"], cfg["embed"], cfg["out_chans"], cfg["patch"]
    hd = C_ // cfg["heads"]
    out: List[Tuple[str, Tuple[int, ...]]] = [("image_encoder.pos_embed", (1, g, g, C_)), ("image_encoder.patch_embed.proj.weight", (C_, 3, p, p)),
                                              ("image_encoder.patch_embed.proj.bias", (C_,))]
    for i in range(cfg["depth"]):
        S = g if i in cfg["global_blocks"] else cfg["window"]
        b = f"image_encoder.blocks.{i}."
        out += [(b + "norm1.weight", (C_,)), (b + "norm1.bias", (C_,)), (b + "attn.qkv.weight", (3 * C_, C_)), (b + "attn.qkv.bias", (3 * C_,)),
                (b + "attn.rel_pos_h", (2 * S - 1, hd)), (b + "attn.rel_pos_w", (2 * S - 1, hd)), (b + "attn.proj.weight", (C_, C_)),
                (b + "attn.proj.bias", (C_,)), (b + "norm2.weight", (C_,)), (b + "norm2.bias", (C_,)), (b + "mlp.lin1.weight", (cfg["mlp"], C_)),
                (b + "mlp.lin1.bias", (cfg["mlp"],)), (b + "mlp.lin2.weight", (C_, cfg["mlp"])), (b + "mlp.lin2.bias", (C_,))]
    n = "image_encoder.neck."
    out += [(n + "0.weight", (P, C_, 1, 1)), (n + "1.weight", (P,)), (n + "1.bias", (P,)), (n + "2.weight", (P, P, 3, 3)), (n + "3.weight", (P,)),
            (n + "3.bias", (P,))]
    out += [("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", (2, P // 2)), ("prompt_encoder.point_embeddings.0.weight", (1, P)),
            ("prompt_encoder.point_embeddings.1.weight", (1, P)), ("prompt_encoder.not_a_point_embed.weight", (1, P)),
            ("prompt_encoder.no_mask_embed.weight", (1, P))]
    d = "mask_decoder."
    out += [(d + "iou_token.weight", (1, P)), (d + "mask_tokens.weight", (cfg["mask_tokens"], P))]

    def attn(prefix: str, inner: int):
        r = []
        for name in ("q_proj", "k_proj", "v_proj"):
            r += [(prefix + name + ".weight", (inner, P)), (prefix + name + ".bias", (inner,))]
        return r + [(prefix + "out_proj.weight", (P, inner)), (prefix + "out_proj.bias", (P,))]

    def norm(prefix: str):
        return [(prefix + ".weight", (P,)), (prefix + ".bias", (P,))]
    inner = P // cfg["dec_down"]
    for l in range(cfg["dec_layers"]):
        b = d + f"transformer.layers.{l}."
        out += attn(b + "self_attn.", P) + norm(b + "norm1") + attn(b + "cross_attn_token_to_image.", inner) + norm(b + "norm2")
        out += [(b + "mlp.lin1.weight", (cfg["dec_mlp"], P)), (b + "mlp.lin1.bias", (cfg["dec_mlp"],)), (b + "mlp.lin2.weight", (P, cfg["dec_mlp"])),
                (b + "mlp.lin2.bias", (P,))]
        out += norm(b + "norm3") + norm(b + "norm4") + attn(b + "cross_attn_image_to_token.", inner)
    out += attn(d + "transformer.final_attn_token_to_image.", inner) + norm(d + "transformer.norm_final_attn")
    u = d + "output_upscaling."
    out += [(u + "0.weight", (P, P // 4, 2, 2)), (u + "0.bias", (P // 4,)), (u + "1.weight", (P // 4,)), (u + "1.bias", (P // 4,)),
            (u + "3.weight", (P // 4, P // 8, 2, 2)), (u + "3.bias", (P // 8,))]
    for m in range(cfg["mask_tokens"]):
        for l in range(cfg["hyper_depth"]):
            o = P // 8 if l == cfg["hyper_depth"] - 1 else P
            out += [(d + f"output_hypernetworks_mlps.{m}.layers.{l}.weight", (o, P)), (d + f"output_hypernetworks_mlps.{m}.layers.{l}.bias", (o,))]
    for l in range(cfg["iou_depth"]):
        i = P if l == 0 else cfg["iou_hidden"]
        o = cfg["mask_tokens"] if l == cfg["iou_depth"] - 1 else cfg["iou_hidden"]
        out += [(d + f"iou_prediction_head.layers.{l}.weight", (o, i)), (d + f"iou_prediction_head.layers.{l}.bias", (o,))]
    return out


def resized_hw(H: int, W: int, image_size: int) -> Tuple[int, int]:
    """``ResizeLongestSide.get_preprocess_shape``."""
    s = image_size * 1.0 / max(H, W)
    return int(H * s + 0.5), int(W * s + 0.5)


class SamSegmenter(nn.Module):
    """SAM in eval mode from its state dict.  The weights are one frozen flat float32 buffer (``weights``, the tensors of
    ``tensor_keys`` one behind the other; move the module with ``.to(device)``), packed for the kernels once per device on first use.
    ``decoder_heads``: the mask decoder's head count, which no shape shows (SAM's is 8)."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor], decoder_heads: int = 8):
        super().__init__()
        sd = state_dict
        cfg = infer_config(sd)
        cfg["dec_heads"] = int(decoder_heads)
        keys = tensor_keys(cfg)
        problems = []
        for key, shape in keys:
            if key not in sd:
                problems.append(f"missing key '{key}' (expected shape {list(shape)})")
            elif not isinstance(sd[key], torch.Tensor) or tuple(sd[key].shape) != tuple(shape):
                problems.append(f"key '{key}' has shape {list(getattr(sd[key], 'shape', ()))}, expected {list(shape)}")
        if problems:
            missing = all(p.startswith("missing") for p in problems)
            raise (KeyError if missing else ValueError)("SamSegmenter: " + "; ".join(problems))
        c = hip_lib.SoarSamConfig()
        c.image_size, c.patch, c.grid = cfg["image_size"], cfg["patch"], cfg["image_size"] // cfg["patch"]
        c.embed, c.depth, c.heads, c.head_dim, c.mlp, c.out_chans = cfg["embed"], cfg["depth"], cfg["heads"], cfg["embed"] // cfg["heads"], cfg["mlp"], cfg["out_chans"]
        if cfg["depth"] > hip_lib.SAM_MAX_DEPTH:
            raise ValueError(f"SamSegmenter: {cfg['depth']} encoder blocks: at most {hip_lib.SAM_MAX_DEPTH}")
        for i in range(cfg["depth"]):
            c.window[i] = 0 if i in cfg["global_blocks"] else cfg["window"]
        c.dec_layers, c.dec_heads, c.dec_down, c.dec_mlp = cfg["dec_layers"], cfg["dec_heads"], cfg["dec_down"], cfg["dec_mlp"]
        c.mask_tokens, c.hyper_depth, c.iou_depth, c.iou_hidden = cfg["mask_tokens"], cfg["hyper_depth"], cfg["iou_depth"], cfg["iou_hidden"]
        nb, cnt = C.c_size_t(0), C.c_int32(0)
        check(hip_lib.lib().soar_sam_weights_bytes(C.byref(c), C.byref(nb), C.byref(cnt)), "soar_sam_weights_bytes")
        if cnt.value != len(keys):
            raise RuntimeError(f"SamSegmenter: the library packs {cnt.value} tensors, tensor_keys lists {len(keys)}")
        self.cfg, self._c, self._packed_bytes = cfg, c, nb.value
        self.max_points = MAX_TOKENS - 2 - cfg["mask_tokens"]
        self._sizes = [int(np.prod(shape)) for _, shape in keys]
        self.register_buffer("weights", torch.cat([sd[k].detach().to(torch.float32).reshape(-1) for k, _ in keys]).contiguous())
        self._pack = hip_lib.PackedWeights()
        self.eval()

    # ---- plumbing ----
    @property
    def image_size(self) -> int:
        return self.cfg["image_size"]

    @property
    def grid(self) -> int:
        return self.cfg["image_size"] // self.cfg["patch"]

    def _packed(self, dev) -> torch.Tensor:
        w = self.weights

        def pack():
            offs = np.concatenate([[0], np.cumsum(self._sizes)[:-1]])
            arr = (C.c_void_p * len(offs))(*[w.data_ptr() + 4 * int(o) for o in offs])
            packed = _workspace(self._packed_bytes, dev)
            with torch.cuda.device(dev):
                check(hip_lib.lib().soar_sam_pack_weights(C.byref(self._c), arr, len(offs), packed.data_ptr(), self._packed_bytes, _stream(dev)),
                      "soar_sam_pack_weights")
            return packed

        return self._pack.get([w], dev, f"SamSegmenter: weights are on {w.device}, the input on {dev}: move the module with .to('{dev}')", pack)

    def _scratch(self, dev, B: int, max_points: int) -> torch.Tensor:
        return _workspace(_bytes(hip_lib.lib().soar_sam_workspace_bytes, "soar_sam_workspace_bytes", C.byref(self._c), B, max_points), dev)

    @staticmethod
    def _need_hip(name: str, t) -> None:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"SamSegmenter: {name} must be a torch.Tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise RuntimeError(f"SamSegmenter: {name} is on '{t.device}': soar_amd.sam runs on HIP devices only; there is no CPU fallback")

    def _check_images(self, images: torch.Tensor) -> None:
        self._need_hip("images", images)
        if images.dtype != torch.uint8:
            raise TypeError(f"SamSegmenter: images must be uint8 [B,H,W,3] (got {images.dtype}); float images are refused")
        if images.dim() != 4 or images.shape[3] != 3 or images.shape[1] < 1 or images.shape[2] < 1:
            raise ValueError(f"SamSegmenter: images must be uint8 [B,H,W,3] (got {tuple(images.shape)})")

    # ---- stages ----
    @torch.no_grad()
    def patches(self, images: torch.Tensor) -> Tuple[torch.Tensor, Tuple[int, int]]:
        """Pre-processing: uint8 ``[B,H,W,3]`` -> (``[B, g g, 3 p p]`` float32, one row per token in the patch convolution's
        (channel, y, x) order, (nh, nw)): Pillow's BILINEAR resize to the longer side, normalisation, zero padding."""
        from .jpeg import resize_images
        self._check_images(images)
        B, H, W, _ = images.shape
        nh, nw = resized_hw(H, W, self.image_size)
        dev = images.device
        resized = resize_images(images, nh, nw, filter="bilinear")
        g, p = self.grid, self.cfg["patch"]
        out = torch.empty((B, g * g, 3 * p * p), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_sam_preprocess(C.byref(self._c), B, nh, nw, resized.data_ptr(), out.data_ptr(),
                                                    _stream(dev)), "soar_sam_preprocess")
        return out, (nh, nw)

    def preprocessed(self, images: torch.Tensor) -> torch.Tensor:
        """The network's input as ``segment_anything`` lays it out, ``[B,3,S,S]`` (a rearrangement of ``patches``)."""
        x, _ = self.patches(images)
        g, p = self.grid, self.cfg["patch"]
        return x.reshape(-1, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(-1, 3, g * p, g * p)

    @torch.no_grad()
    def encode(self, patches: Optional[torch.Tensor] = None, tokens: Optional[torch.Tensor] = None, blocks: Optional[Tuple[int, int]] = None,
               neck: bool = True, workspace: Optional[torch.Tensor] = None):
        """The image encoder or a part of it (csrc/sam.hip soar_sam_encode): from ``patches`` (patch embedding + pos_embed first) or
        from ``tokens [B,g,g,C]``, through blocks ``blocks[0] .. blocks[1] - 1`` (all by default) -> the embeddings ``[B,P,g,g]``
        (``neck``) or the tokens ``[B,g,g,C]``."""
        src = patches if patches is not None else tokens
        self._need_hip("patches" if patches is not None else "tokens", src)
        dev, B, g = src.device, src.shape[0], self.grid
        want = (B, g * g, 3 * self.cfg["patch"] ** 2) if patches is not None else (B, g, g, self.cfg["embed"])
        if src.dtype != torch.float32 or tuple(src.shape) != want:
            raise ValueError(f"SamSegmenter.encode: expected float32 {list(want)} (got {src.dtype} {list(src.shape)})")
        src = src.contiguous()
        b0, b1 = (0, self.cfg["depth"]) if blocks is None else blocks
        a = hip_lib.SoarSamEncodeArgs()
        a.B, a.block_begin, a.block_end = B, b0, b1
        if patches is not None:
            a.patches = src.data_ptr()
        else:
            a.tokens_in = src.data_ptr()
        out = torch.empty((B, g, g, self.cfg["out_chans"] if neck else self.cfg["embed"]), dtype=torch.float32, device=dev)
        if neck:
            a.embeddings = out.data_ptr()
        else:
            a.tokens_out = out.data_ptr()
        if B == 0:
            return out.permute(0, 3, 1, 2) if neck else out
        packed = self._packed(dev)
        ws = self._scratch(dev, B, 0) if workspace is None else workspace
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_sam_encode(C.byref(self._c), packed.data_ptr(), C.byref(a), ws.data_ptr(), ws.numel(),
                                                _stream(dev)), "soar_sam_encode")
        return out.permute(0, 3, 1, 2) if neck else out

    def embed(self, images: torch.Tensor) -> torch.Tensor:
        """uint8 ``[B,H,W,3]`` -> image embeddings ``[B,C,g,g]`` (``SamPredictor.set_image``; channels-last in memory)."""
        x, _ = self.patches(images)
        return self.encode(patches=x)

    def _prompts(self, dev, B: int, points, counts, labels):
        for name, t in (("points", points), ("counts", counts), ("labels", labels)):
            if t is not None:
                self._need_hip(name, t)
        if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 2:
            raise ValueError(f"SamSegmenter: points must be [B,M,2] with B = {B} (got {tuple(points.shape)})")
        M = points.shape[1]
        if M > self.max_points:
            raise ValueError(f"SamSegmenter: {M} points a frame: at most {self.max_points}")
        if counts is None:
            counts = torch.full((B,), M, dtype=torch.int32, device=dev)
        if counts.shape != (B,):
            raise ValueError(f"SamSegmenter: counts must be [B] = [{B}] (got {tuple(counts.shape)})")
        if labels is None:
            labels = torch.ones((B, M), dtype=torch.int32, device=dev)
        if labels.shape != (B, M):
            raise ValueError(f"SamSegmenter: labels must be [B,M] = [{B},{M}] (got {tuple(labels.shape)})")
        return points.to(torch.float32).contiguous(), counts.to(torch.int32).contiguous(), labels.to(torch.int32).contiguous(), M

    @torch.no_grad()
    def decode(self, embeddings: torch.Tensor, points: torch.Tensor, counts: Optional[torch.Tensor], orig_hw: Tuple[int, int],
               labels: Optional[torch.Tensor] = None, return_tokens: bool = False, workspace: Optional[torch.Tensor] = None, boxes=None,
               mask_input=None):
        """embeddings ``[B,C,g,g]``, points ``[B,M,2]`` (x, y) in pixels of the ``orig_hw`` frame, counts ``[B]`` (None: M each),
        labels ``[B,M]`` 1 / 0 (None: ones) -> ``(low_res_logits [B,3,4g,4g], iou [B,3])`` (``multimask_output=True``: masks 1 .. 3).
        ``return_tokens``: also the decoder's tokens ``[B,T,C]`` before and after the two-way transformer, T = 1 + mask tokens + M + 1
        (a frame's tokens are the first ``2 + mask_tokens + counts[b]``; the rest is unspecified)."""
        if boxes is not None or mask_input is not None:
            raise NotImplementedError("SamSegmenter: only point prompts; boxes and mask prompts are not implemented")
        self._need_hip("embeddings", embeddings)
        dev, B, g, P = embeddings.device, embeddings.shape[0], self.grid, self.cfg["out_chans"]
        if embeddings.dtype != torch.float32 or tuple(embeddings.shape) != (B, P, g, g):
            raise ValueError(f"SamSegmenter.decode: embeddings must be float32 [B,{P},{g},{g}] (got {embeddings.dtype} {list(embeddings.shape)})")
        points, counts, labels, M = self._prompts(dev, B, points, counts, labels)
        H, W = int(orig_hw[0]), int(orig_hw[1])
        nh, nw = resized_hw(H, W, self.image_size)
        emb = embeddings.permute(0, 2, 3, 1).contiguous()
        nm = self.cfg["mask_tokens"]
        low = torch.empty((B, nm - 1, 4 * g, 4 * g), dtype=torch.float32, device=dev)
        iou = torch.empty((B, nm - 1), dtype=torch.float32, device=dev)
        T = 2 + nm + M
        tok = torch.empty((2, B, T, P), dtype=torch.float32, device=dev) if return_tokens else None
        if B:
            a = hip_lib.SoarSamDecodeArgs()
            a.B, a.max_points = B, M
            a.scale_x, a.scale_y = float(np.float32(nw) / np.float32(W)), float(np.float32(nh) / np.float32(H))
            a.embeddings, a.points, a.labels, a.counts = emb.data_ptr(), points.data_ptr() if M else None, labels.data_ptr() if M else None, counts.data_ptr()
            a.low_res, a.iou = low.data_ptr(), iou.data_ptr()
            if return_tokens:
                a.prompt_tokens, a.tokens_out = tok[0].data_ptr(), tok[1].data_ptr()
            packed = self._packed(dev)
            ws = self._scratch(dev, B, M) if workspace is None else workspace
            with torch.cuda.device(dev):
                check(hip_lib.lib().soar_sam_decode(C.byref(self._c), packed.data_ptr(), C.byref(a), ws.data_ptr(), ws.numel(),
                                                    _stream(dev)), "soar_sam_decode")
        return (low, iou, tok[0], tok[1]) if return_tokens else (low, iou)

    @torch.no_grad()
    def postprocess(self, low_res: torch.Tensor, orig_hw: Tuple[int, int], binary: bool = False) -> torch.Tensor:
        """``Sam.postprocess_masks``: ``[B,K,L,L]`` -> ``[B,K,H,W]`` float32 logits, or bool (``> 0``) with ``binary``."""
        self._need_hip("low_res", low_res)
        B, K, L, _ = low_res.shape
        H, W = int(orig_hw[0]), int(orig_hw[1])
        nh, nw = resized_hw(H, W, self.image_size)
        dev = low_res.device
        low_res = low_res.to(torch.float32).contiguous()
        out = torch.empty((B, K, H, W), dtype=torch.uint8 if binary else torch.float32, device=dev)
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_sam_postprocess(B, K, L, self.image_size, nh, nw, H, W, low_res.data_ptr(), None if binary else out.data_ptr(),
                                                     out.data_ptr() if binary else None, _stream(dev)), "soar_sam_postprocess")
        return out.view(torch.bool) if binary else out

    def _run(self, images, points, counts, labels, binary: bool) -> torch.Tensor:
        self._check_images(images)
        hw = tuple(images.shape[1:3])
        low, _ = self.decode(self.embed(images), points, counts, hw, labels)
        return self.postprocess(low, hw, binary)

    def logits(self, images: torch.Tensor, points: torch.Tensor, counts: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 ``[B,H,W,3]``, points ``[B,M,2]``, counts ``[B]`` -> full-resolution logits ``[B,3,H,W]`` float32.  No synchronisation."""
        return self._run(images, points, counts, labels, False)

    def masks(self, images: torch.Tensor, points: torch.Tensor, counts: Optional[torch.Tensor] = None, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> ``[B,3,H,W]`` bool: ``logits > 0`` (``SamPredictor.predict``'s masks)."""
        return self._run(images, points, counts, labels, True)

    def forward(self, image, coords, labels=None, boxes=None, mask_input=None) -> torch.Tensor:
        """One frame as ``masks.segment_sequence`` calls its predictor: image uint8 ``[H,W,3]`` (array or tensor), coords ``[M,2]``,
        labels ``[M]`` -> logits ``[3,H,W]`` on the module's device."""
        if boxes is not None or mask_input is not None:
            raise NotImplementedError("SamSegmenter: only point prompts; boxes and mask prompts are not implemented")
        dev = self.weights.device
        if isinstance(image, torch.Tensor):
            self._need_hip("image", image)
        else:
            image = torch.from_numpy(np.ascontiguousarray(image)).to(dev)
        pts = torch.as_tensor(np.asarray(coords.cpu() if isinstance(coords, torch.Tensor) else coords, dtype=np.float32).reshape(1, -1, 2)).to(dev)
        lab = None
        if labels is not None:
            lab = torch.as_tensor(np.asarray(labels.cpu() if isinstance(labels, torch.Tensor) else labels).reshape(1, -1) != 0).to(dev, torch.int32)
        return self.logits(image[None], pts, None, lab)[0]
