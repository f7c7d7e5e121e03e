"""Test-split evaluation: PSNR, skimage's windowed SSIM and LPIPS-VGG of rendered frames against the white-composited ground truth.

Restates ``test_step`` / ``on_test_epoch_end`` of TS/system/gaussian_surfel_mvdream.py:527-589.  The reference copies three 1080p
images to the host per frame, runs ``skimage.metrics.peak_signal_noise_ratio`` and ``structural_similarity`` in NumPy and moves its
LPIPS network to the CPU.  Here one launch (csrc/eval.hip, soar_eval_image_metrics) makes the white target, the squared error, the
7x7-window SSIM in float64, the two LPIPS inputs and the side-by-side byte image; ``LPIPSVGG`` runs on them under ``no_grad``; the
numbers stay on the device until ``TestEvaluator.finish()`` reads them back once.

``image_metrics`` makes no read-back and no synchronisation and runs on the current stream.  HIP only: CPU tensors are refused.
(DESIGN.md 9j states the computation in full.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Callable, Dict, List, Optional

import torch

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check
from .lpips import LPIPSVGG

WINDOW = 7          # skimage's default win_size


def _check(pred, gt_rgb, gt_mask) -> torch.Tensor:
    """the refusals of image_metrics; -> gt_mask as [N,H,W]"""
    for name, t in (("pred", pred), ("gt_rgb", gt_rgb)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"image_metrics: {name} must be an [N, H, W, 3] tensor (got {tuple(getattr(t, 'shape', ()))})")
    if not isinstance(gt_mask, torch.Tensor) or gt_mask.dim() not in (3, 4) or (gt_mask.dim() == 4 and gt_mask.shape[3] != 1):
        raise ValueError(f"image_metrics: gt_mask must be an [N, H, W] or [N, H, W, 1] tensor (got {tuple(getattr(gt_mask, 'shape', ()))})")
    if gt_mask.dim() == 4:
        gt_mask = gt_mask[..., 0]
    if pred.shape != gt_rgb.shape or tuple(gt_mask.shape) != tuple(pred.shape[:3]):
        raise ValueError(f"image_metrics: pred, gt_rgb and gt_mask must agree in N, H, W (got {tuple(pred.shape)}, {tuple(gt_rgb.shape)} "
                         f"and {tuple(gt_mask.shape)})")
    for name, t in (("pred", pred), ("gt_rgb", gt_rgb), ("gt_mask", gt_mask)):
        if not t.is_cuda:
            raise RuntimeError(f"image_metrics: {name} is on '{t.device}': soar_amd.evaluate runs on HIP devices only; there is no CPU fallback")
        if t.dtype != torch.float32:
            raise TypeError(f"image_metrics: {name} must be float32 (got {t.dtype})")
    if not (pred.device == gt_rgb.device == gt_mask.device):
        raise ValueError(f"image_metrics: pred, gt_rgb and gt_mask must be on the same device (got {pred.device}, {gt_rgb.device} and "
                         f"{gt_mask.device})")
    N, H, W = gt_mask.shape
    if N < 1:
        raise ValueError("image_metrics: an empty batch has no metrics (N = 0)")
    if H < WINDOW or W < WINDOW:
        raise ValueError(f"image_metrics: H, W >= {WINDOW} needed so that one {WINDOW}x{WINDOW} SSIM window fits (got {H} x {W})")
    return gt_mask


def image_metrics(pred: torch.Tensor, gt_rgb: torch.Tensor, gt_mask: torch.Tensor, lpips: Optional[LPIPSVGG] = None,
                  grid: bool = False) -> Dict[str, Any]:
    """pred, gt_rgb [N,H,W,3], gt_mask [N,H,W] or [N,H,W,1] (float32, any strides, on the device) ->
    ``psnr``, ``ssim``, ``mse``: float64 [N];  ``lpips``: float32 [N] through the given module under ``no_grad``, or None;
    ``gt_white`` [N,H,W,3]: the target with everything outside ``gt_mask > 0.5`` painted white;  ``pred2``, ``gt2``: the LPIPS inputs
    ``x * 2 - 1``;  ``grid``: uint8 [N,H,2W,3], ``pred | gt_white``, or None."""
    gt_mask = _check(pred, gt_rgb, gt_mask)
    pred, gt_rgb, gt_mask = pred.detach(), gt_rgb.detach(), gt_mask.detach()
    dev = pred.device
    N, H, W = gt_mask.shape
    L = hip_lib.lib()
    scratch = _workspace(_bytes(L.soar_eval_scratch_bytes, "soar_eval_scratch_bytes", N, H, W), dev)
    out = torch.empty((3, N, H, W, 3), dtype=torch.float32, device=dev)        # gt_white, pred2, gt2
    metrics = torch.empty((N, 3), dtype=torch.float64, device=dev)
    grid_t = torch.empty((N, H, 2 * W, 3), dtype=torch.uint8, device=dev) if grid else None
    a = hip_lib.SoarEvalArgs()
    a.N, a.H, a.W = N, H, W
    a.pred, a.gt_rgb, a.gt_mask = pred.data_ptr(), gt_rgb.data_ptr(), gt_mask.data_ptr()
    for i in range(4):
        a.pred_stride[i], a.gt_stride[i] = pred.stride(i), gt_rgb.stride(i)
    for i in range(3):
        a.mask_stride[i] = gt_mask.stride(i)
    a.gt_white, a.pred2, a.gt2 = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
    a.grid = None if grid_t is None else grid_t.data_ptr()
    a.metrics = metrics.data_ptr()
    with torch.cuda.device(dev):
        check(L.soar_eval_image_metrics(C.byref(a), scratch.data_ptr(), scratch.numel(), _stream(dev)), "soar_eval_image_metrics")
    lp = None
    if lpips is not None:
        with torch.no_grad():
            lp = lpips(out[1].permute(0, 3, 1, 2), out[2].permute(0, 3, 1, 2)).view(-1)
    return {"psnr": metrics[:, 0], "ssim": metrics[:, 1], "mse": metrics[:, 2], "lpips": lp, "gt_white": out[0], "pred2": out[1],
            "gt2": out[2], "grid": grid_t}


class TestEvaluator:
    """Collects the metrics of a test split on the device: ``add`` per frame, ``finish`` once (one read-back).

    ``lpips``: the ``LPIPSVGG`` to use, or None (the lpips column is NaN then).  ``capacity``: the most frames ``add`` will take.
    ``keep_images``: also keep every frame's ``pred | gt_white`` byte image, which ``finish(save_dir)`` writes as PNGs."""
    __test__ = False          # (a class of the library, not a pytest class)

    def __init__(self, lpips: Optional[LPIPSVGG], capacity: int, keep_images: bool = False):
        if capacity < 1:
            raise ValueError(f"TestEvaluator: capacity must be at least 1 (got {capacity})")
        self.lpips, self.capacity, self.keep_images = lpips, int(capacity), bool(keep_images)
        self.buffer: Optional[torch.Tensor] = None      # float64 [capacity, 3] on the device: psnr, ssim, lpips
        self.count = 0
        self.gt_indices: List[int] = []
        self.images: List[torch.Tensor] = []            # uint8 [H, 2W, 3] per frame (keep_images)

    def add(self, pred: torch.Tensor, batch: Dict[str, Any]) -> Dict[str, Any]:
        """pred [1,H,W,3] (the caller's ``gt_out["comp_rgb"]``) against ``batch["gt_rgb"]`` / ``batch["gt_mask"]`` of
        ``RandomMultiviewCameraDataset.collate()``; -> what ``image_metrics`` returned.  No read-back."""
        if pred.dim() != 4 or pred.shape[0] != 1:
            raise ValueError(f"TestEvaluator.add: pred must be [1, H, W, 3], one frame per call (got {tuple(pred.shape)})")
        if self.count >= self.capacity:
            raise RuntimeError(f"TestEvaluator.add: capacity of {self.capacity} frames exhausted")
        m = image_metrics(pred, batch["gt_rgb"], batch["gt_mask"], lpips=self.lpips, grid=self.keep_images)
        if self.buffer is None:
            self.buffer = torch.full((self.capacity, 3), float("nan"), dtype=torch.float64, device=pred.device)
        row = self.buffer[self.count]
        row[0:1].copy_(m["psnr"])
        row[1:2].copy_(m["ssim"])
        if m["lpips"] is not None:
            row[2:3].copy_(m["lpips"])                   # (float32 -> float64 on the device)
        self.gt_indices.append(int(batch["gt_index"]))
        if self.keep_images:
            self.images.append(m["grid"][0])
        self.count += 1
        return m

    def _read_back(self):
        """the ONE device-to-host transfer of finish(): the metrics buffer -> float64 [count, 3] array"""
        if self.buffer is None:
            raise RuntimeError("TestEvaluator.finish: no frame was added")
        return self.buffer.cpu().numpy()[:self.count]

    def finish(self, save_dir: Optional[str] = None, step: int = 0, device_png: bool = False) -> Dict[str, Any]:
        """-> ``psnrs``, ``ssims`` (float64 [count]), ``lpips`` (float32 [count]), ``psnr``, ``ssim``, ``lpips_mean`` (their means) and
        ``gt_indices``.  With ``save_dir``: psnrs.txt, ssims.txt, lpips.txt (``np.savetxt``) and average.txt, the reference's files; with
        ``keep_images`` also ``it{step}-test/{gt_index}.png``, made on the device with ``device_png=True`` (``png.write_png_files``:
        the same names and pixels, and only compressed bytes are copied to the host)."""
        import numpy as np
        host = self._read_back()
        psnrs, ssims = host[:, 0].copy(), host[:, 1].copy()
        lp = host[:, 2].astype(np.float32)               # the reference holds its LPIPS values in a float32 tensor
        res = {"psnrs": psnrs, "ssims": ssims, "lpips": lp, "psnr": psnrs.mean(), "ssim": ssims.mean(), "lpips_mean": lp.mean(),
               "gt_indices": list(self.gt_indices)}
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
            np.savetxt(os.path.join(save_dir, "psnrs.txt"), psnrs)
            np.savetxt(os.path.join(save_dir, "ssims.txt"), ssims)
            np.savetxt(os.path.join(save_dir, "lpips.txt"), lp)
            with open(os.path.join(save_dir, "average.txt"), "w") as f:
                f.write(f"{res['psnr']} {res['ssim']} {res['lpips_mean']}")
            if self.keep_images and self.images:
                from PIL import Image
                folder = os.path.join(save_dir, f"it{step}-test")
                os.makedirs(folder, exist_ok=True)
                if device_png:
                    from .png import write_png_files
                    write_png_files([os.path.join(folder, f"{i}.png") for i in self.gt_indices], torch.stack(self.images))
                    return res
                for i, img in zip(self.gt_indices, torch.stack(self.images).cpu().numpy()):
                    Image.fromarray(img).save(os.path.join(folder, f"{i}.png"))
        return res


def evaluate_split(render: Callable[[Dict[str, Any]], torch.Tensor], dataset, evaluator: TestEvaluator) -> TestEvaluator:
    """Walks a ``split="test"`` dataset in order: ``render(batch) -> [1,H,W,3]`` (the caller's ``gt_out["comp_rgb"]``), ``evaluator.add``."""
    for i in range(len(dataset)):
        batch = dataset[i]
        evaluator.add(render(batch), batch)
    return evaluator
