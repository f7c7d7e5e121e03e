"""Mask clean-up of the preprocessing: from a segmenter's candidate masks to the one foreground mask per frame that ``FrameStore``,
``crop_frames``, the losses and the evaluation read -- in HIP (csrc/masks.hip).

The reference does this per frame on the host (preproc/compute_kp_and_mask.py:61-79): the union of SAM's three candidates,
``cv2.morphologyEx`` OPEN then CLOSE with a 5 x 5 kernel, ``cv2.connectedComponentsWithStats(connectivity=8)``, the largest
component, a PNG.  The segmenter is ``sam.SamSegmenter`` or the caller's; everything behind it runs here, on bit-planes, for N
frames per call.

* ``open_close(mask)``: union over K (if given), OPEN, CLOSE -> uint8 ``[N,H,W]``.
* ``largest_component(mask)``: the largest 8-connected component of every frame.
* ``clean_masks(candidates)``: the pipeline, in chunks of frames under a workspace cap.
* ``keypoint_prompts`` / ``segment_sequence`` / ``save_masks``: the prompts from the OpenPose keypoints, the loop over the caller's
  predictor (or the batched path of ``sam.SamSegmenter``), and the PNGs ``FrameStore.read_dataroot`` reads.

**Border rule.**  An erosion treats pixels outside the image as set, a dilation as unset, and each of the four operations applies
this to its own input: OpenCV's documented default (``morphologyDefaultBorderValue``), identical to
``scipy.ndimage.binary_erosion(border_value=1)`` / ``binary_dilation(border_value=0)``.  The rule is taken from OpenCV's
documentation, it is **not measured against** ``cv2``, which this project does not import.
**Tie rule.**  A component's label is the smallest raster index ``y W + x`` of its pixels; the largest area wins and, among equal
areas, the smallest label.  The reference's order among equal areas is ``np.argmax`` over OpenCV's label numbering, which for
8-connectivity need not be raster order: this is the project's own definition.
**Empty frames.**  A frame whose cleaned mask is empty gives zeros and ``n_components = 0`` (the reference raises there); refusing
such a frame stays with ``FrameStore.from_arrays``.

Statistics are int32 ``[N,4]``: ``union_area, cleaned_area, n_components, kept_area``.  Integer arithmetic only: two runs, and a
chunked and an unchunked run, give the same bits.  HIP only: CPU tensors are refused, there is no CPU fallback.
"""
from __future__ import annotations

import os
from typing import Callable, List, Sequence, Tuple

import numpy as np
import torch

from . import hip_lib
from .data import _need_cuda
from .hip_lib import _bytes, _stream, _workspace, check

DT_U8, DT_F32 = 0, 1               # dtype codes of soar_masks_open_close / soar_masks_clean
MAX_FRAMES = 65535                 # per call of the library
STATS = ("union_area", "cleaned_area", "n_components", "kept_area")


def workspace_bytes(N: int, H: int, W: int) -> int:
    return _bytes(hip_lib.lib().soar_masks_workspace_bytes, "soar_masks_workspace_bytes", N, H, W)


def _candidates(x, what: str, allow_float: bool = True):
    """-> (device, contiguous tensor the kernels read, dtype code).  ``[N,H,W]`` counts as K = 1."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: expected a torch.Tensor (got {type(x).__name__})")
    dev = _need_cuda(x.device, what)
    if x.dim() == 3:
        x = x.unsqueeze(1)
    if x.dim() != 4:
        raise ValueError(f"{what}: expected [N,H,W] or [N,K,H,W] (got {tuple(x.shape)})")
    if x.dtype == torch.bool:
        x, code = x.contiguous().view(torch.uint8), DT_U8
    elif x.dtype == torch.uint8:
        x, code = x.contiguous(), DT_U8
    elif x.dtype == torch.float32 and allow_float:
        x, code = x.contiguous(), DT_F32
    else:
        raise TypeError(f"{what}: dtype must be uint8, bool{' or float32' if allow_float else ''} (got {x.dtype})")
    if min(x.shape[1:]) < 1:
        raise ValueError(f"{what}: K, H and W must be at least 1 (got {tuple(x.shape)})")
    return dev, x, code


def _run(entry: str, cand: torch.Tensor, code: int, threshold: float, dev: torch.device, out: torch.Tensor, stats: torch.Tensor,
         workspace: torch.Tensor) -> None:
    N, K, H, W = cand.shape
    L = hip_lib.lib()
    with torch.cuda.device(dev):
        s = _stream(dev)
        if entry == "soar_masks_largest_component":
            rc = L.soar_masks_largest_component(N, H, W, cand.data_ptr(), out.data_ptr(), stats.data_ptr(), workspace.data_ptr(),
                                                workspace.numel(), s)
        else:
            rc = getattr(L, entry)(N, K, H, W, cand.data_ptr(), code, float(threshold), out.data_ptr(), stats.data_ptr(),
                                   workspace.data_ptr(), workspace.numel(), s)
    check(rc, entry)


def _chunked(entry: str, cand: torch.Tensor, code: int, threshold: float, dev: torch.device, max_workspace_bytes: int):
    N, K, H, W = cand.shape
    out = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    stats = torch.empty((N, 4), dtype=torch.int32, device=dev)
    if N == 0:
        return out, stats
    per = workspace_bytes(1, H, W)
    chunk = max(1, min(N, MAX_FRAMES, int(max_workspace_bytes) // per))
    while chunk > 1 and workspace_bytes(chunk, H, W) > max_workspace_bytes:
        chunk -= 1
    workspace = _workspace(workspace_bytes(chunk, H, W), dev)
    for i in range(0, N, chunk):          # one stream: a chunk's launches are done with the workspace before the next one's start
        j = min(i + chunk, N)
        _run(entry, cand[i:j], code, threshold, dev, out[i:j], stats[i:j], workspace)
    return out, stats


@torch.no_grad()
def open_close(mask: torch.Tensor, threshold: float = 0.0, return_stats: bool = False, max_workspace_bytes: int = 256 << 20):
    """``mask [N,H,W]`` or ``[N,K,H,W]`` (uint8 / bool: non-zero is set; float32: ``> threshold``) -> uint8 ``[N,H,W]`` in {0, 1}: the
    union over K, then OPEN and CLOSE with the 5 x 5 element under the border rule of the module's docstring (documented, not
    measured against ``cv2``).  Two launches.  With ``return_stats`` also int32 ``[N,4]`` (``union_area, cleaned_area, 0, 0``)."""
    dev, cand, code = _candidates(mask, "open_close")
    out, stats = _chunked("soar_masks_open_close", cand, code, threshold, dev, max_workspace_bytes)
    return (out, stats) if return_stats else out


@torch.no_grad()
def largest_component(mask: torch.Tensor, return_stats: bool = False, max_workspace_bytes: int = 256 << 20):
    """``mask [N,H,W]`` uint8 / bool -> uint8 ``[N,H,W]``: the largest 8-connected component of every frame under the tie rule of the
    module's docstring; an empty frame stays empty.  Stats: ``area, area, n_components, kept_area``."""
    if isinstance(mask, torch.Tensor) and mask.dim() != 3:
        raise ValueError(f"largest_component: expected [N,H,W] (got {tuple(mask.shape)})")
    dev, cand, code = _candidates(mask, "largest_component", allow_float=False)
    out, stats = _chunked("soar_masks_largest_component", cand, code, 0.0, dev, max_workspace_bytes)
    return (out, stats) if return_stats else out


@torch.no_grad()
def clean_masks(candidates: torch.Tensor, threshold: float = 0.0, return_stats: bool = False, max_workspace_bytes: int = 256 << 20):
    """The pipeline: ``candidates [N,K,H,W]`` (or ``[N,H,W]``) -> uint8 ``[N,H,W]``, the largest component of the opened and closed
    union.  Frames go in chunks whose workspace stays under ``max_workspace_bytes`` (one frame at least); a chunked result is
    bit-equal to an unchunked one.  Nothing is read back and nothing synchronises."""
    dev, cand, code = _candidates(candidates, "clean_masks")
    out, stats = _chunked("soar_masks_clean", cand, code, threshold, dev, max_workspace_bytes)
    return (out, stats) if return_stats else out


def keypoint_prompts(keypoints, n_body: int = 25, conf: float = 0.5) -> List[Tuple[np.ndarray, np.ndarray]]:
    """Per frame ``(coords [M,2] float32, labels [M] float32 of ones)``: the first ``n_body`` keypoints (OpenPose's body) whose
    confidence is above ``conf``.  ``keypoints [N,>=n_body,3]`` is what ``smplify.load_keypoints`` returns.  Host only."""
    kp = np.asarray(keypoints, dtype=np.float32)
    if kp.ndim != 3 or kp.shape[2] != 3:
        raise ValueError(f"keypoint_prompts: keypoints must be [N,J,3] (got {kp.shape})")
    out = []
    for frame in kp:
        body = frame[:n_body]
        coords = np.ascontiguousarray(body[body[:, 2] > conf, :2])
        out.append((coords, np.ones_like(coords[:, 0])))
    return out


@torch.no_grad()
def segment_sequence(predict: Callable, images: Sequence, keypoints, chunk: int = 8, reverse_channels: bool = True, device=None,
                     threshold: float = 0.0):
    """The mask half of the preprocessing for a sequence: ``predict(image, coords, labels) -> [K,H,W]`` (the caller's segmenter: a
    tensor or an array, logits or booleans) is called once per frame with the prompts of ``keypoint_prompts``; a chunk of frames is
    stacked on the device and cleaned.  Returns ``(masks [N,H,W] uint8, stats [N,4] int32)``.

    With a ``sam.SamSegmenter`` as ``predict`` a chunk is uploaded once, segmented in one batch (``SamSegmenter.logits``) and cleaned
    without leaving the device; any other callable goes through the loop.

    ``reverse_channels=True`` hands the image over as ``image[..., ::-1]`` because the reference does
    (compute_kp_and_mask.py:61: the RGB file reaches SAM with its channels reversed)."""
    if chunk < 1:
        raise ValueError(f"segment_sequence: chunk must be >= 1 (got {chunk})")
    prompts = keypoint_prompts(keypoints)
    if len(prompts) != len(images):
        raise ValueError(f"segment_sequence: {len(images)} images but keypoints of {len(prompts)} frames")
    from .sam import SamSegmenter
    if isinstance(predict, SamSegmenter):
        return _segment_sequence_sam(predict, images, prompts, chunk, reverse_channels, device, threshold)
    dev = _need_cuda(torch.device("cuda" if device is None else device), "segment_sequence")
    masks, stats = [], []
    for i in range(0, len(images), chunk):
        cands = []
        for image, (coords, labels) in zip(images[i:i + chunk], prompts[i:i + chunk]):
            c = predict(image[..., ::-1] if reverse_channels else image, coords, labels)
            c = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(c))
            if c.dtype not in (torch.bool, torch.uint8, torch.float32):
                c = c.to(torch.float32)
            cands.append(c.to(dev))
        m, s = clean_masks(torch.stack(cands), threshold=threshold, return_stats=True)
        masks.append(m)
        stats.append(s)
    if not masks:
        return torch.empty((0, 0, 0), dtype=torch.uint8, device=dev), torch.empty((0, 4), dtype=torch.int32, device=dev)
    return torch.cat(masks), torch.cat(stats)


def _segment_sequence_sam(sam, images: Sequence, prompts, chunk: int, reverse_channels: bool, device, threshold: float):
    """``segment_sequence`` with this project's segmenter (``sam.SamSegmenter``): a chunk of frames is uploaded once, segmented in
    one batch and cleaned, and nothing comes back to the host in between.  Frames of one chunk that differ in size go in runs of
    equal size.  The prompts' labels count as 1 where non-zero."""
    dev = _need_cuda(sam.weights.device if device is None else torch.device(device), "segment_sequence")
    masks, stats = [], []
    for i in range(0, len(images), chunk):
        frames = [np.asarray(im.detach().cpu() if isinstance(im, torch.Tensor) else im) for im in images[i:i + chunk]]
        j = 0
        while j < len(frames):
            k = j + 1
            while k < len(frames) and frames[k].shape == frames[j].shape:
                k += 1
            run = np.stack(frames[j:k])
            batch = torch.from_numpy(np.ascontiguousarray(run[..., ::-1] if reverse_channels else run)).to(dev, non_blocking=True)
            pr = prompts[i + j:i + k]
            M = max(1, max(len(c) for c, _ in pr))
            pts, lab = np.zeros((k - j, M, 2), np.float32), np.zeros((k - j, M), np.int32)
            for b, (c, l) in enumerate(pr):
                pts[b, :len(c)], lab[b, :len(c)] = c, np.asarray(l) != 0
            counts = torch.tensor([len(c) for c, _ in pr], dtype=torch.int32).to(dev, non_blocking=True)
            cand = sam.logits(batch, torch.from_numpy(pts).to(dev, non_blocking=True), counts, torch.from_numpy(lab).to(dev, non_blocking=True))
            m, s = clean_masks(cand, threshold=threshold, return_stats=True)
            masks.append(m)
            stats.append(s)
            j = k
    if not masks:
        return torch.empty((0, 0, 0), dtype=torch.uint8, device=dev), torch.empty((0, 4), dtype=torch.int32, device=dev)
    if any(m.shape[1:] != masks[0].shape[1:] for m in masks):
        raise ValueError("segment_sequence: the frames differ in size: their masks cannot be stacked")
    return torch.cat(masks), torch.cat(stats)


def save_masks(masks, data_dir: str, device_png: bool = False) -> List[str]:
    """``masks [N,H,W]`` (non-zero is foreground) -> ``data_dir/masks/00000.png`` ..., 8-bit greyscale 0 / 255 (both
    ``FrameStore.read_dataroot`` and the reference's loader read a mask as ``> 0``).  Returns the paths.  ``device_png=True`` makes the
    files on the device (``png.write_png_files``; ``masks`` must then be a tensor on a HIP device): the same names and pixels, and only
    compressed bytes are copied to the host."""
    if device_png:
        from .png import write_png_files
        if not isinstance(masks, torch.Tensor) or masks.dim() != 3:
            raise ValueError("save_masks: with device_png masks must be a [N,H,W] tensor")
        out_dir = os.path.join(data_dir, "masks")
        os.makedirs(out_dir, exist_ok=True)
        paths = [os.path.join(out_dir, f"{i:05d}.png") for i in range(masks.shape[0])]
        write_png_files(paths, (masks.detach() != 0).to(torch.uint8) * 255)
        return paths
    from PIL import Image
    m = masks.detach().cpu().numpy() if isinstance(masks, torch.Tensor) else np.asarray(masks)
    if m.ndim != 3:
        raise ValueError(f"save_masks: masks must be [N,H,W] (got {m.shape})")
    out_dir = os.path.join(data_dir, "masks")
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for i, frame in enumerate(m):
        paths.append(os.path.join(out_dir, f"{i:05d}.png"))
        Image.fromarray(((frame != 0) * np.uint8(255)).astype(np.uint8)).save(paths[-1])
    return paths
