"""The training data module (``data_type: "mvdream-random-multiview-camera-datamodule"``) on the device.

Restates ``RandomMultiviewCameraIterableDataset`` / ``ValDataset`` of TS/data/uncond_multiview.py.  The reference keeps the video as
float32 on the host, builds every step's rays in torch-CPU and lets Lightning copy ~40 MB of pageable memory to the device per step.
Here the frames stay on the device as bytes (``FrameStore``), the boxes and the ImageDream crops are made once by two launches, and
``RandomMultiviewCameraDataset.collate()`` produces the whole batch dict with ONE launch (csrc/data.hip, soar_data_step_batch): no
device-to-host copy and no pageable host-to-device copy -- the step's small inputs (camera matrices, angles, ...) travel in the
kernel's arguments.  The random draws stay on the host, in the reference's order: a seed gives the reference's cameras.

The outputs of a step live in a ring of ``RING_DEPTH`` batches owned by the dataset: a batch stays valid until ``RING_DEPTH`` further
``collate()`` calls have been made."""
from __future__ import annotations

import bisect
import ctypes as C
import dataclasses
import math
import os
import random
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import hip_lib
from .hip_lib import _stream
from .renderer import registry

CROP = hip_lib.DATA_CROP
RING_DEPTH = 4


def _need_cuda(dev: torch.device, what: str) -> torch.device:
    dev = torch.device(dev)
    if dev.type != "cuda":
        raise RuntimeError(f"{what} runs on the HIP device only: soar_amd has no CPU fallback (device={dev})")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def mask_bbox(masks: torch.Tensor) -> torch.Tensor:
    """masks [N,H,W] uint8 on the device -> int32 [N,4] inclusive (xmin, ymin, xmax, ymax); (W, H, -1, -1) for an empty mask."""
    dev = _need_cuda(masks.device, "mask_bbox")
    assert masks.dtype == torch.uint8 and masks.dim() == 3 and masks.is_contiguous()
    N, H, W = masks.shape
    boxes = torch.empty((N, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        hip_lib.check(hip_lib.lib().soar_data_mask_bbox(N, H, W, hip_lib.ptr(masks), hip_lib.ptr(boxes), _stream(dev)), "soar_data_mask_bbox")
    return boxes


def crops(images: torch.Tensor, masks: torch.Tensor, boxes: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The reference's 512 x 512 crops (:246-313) of N frames in one launch -> float32 [N,512,512,3], [N,512,512]."""
    dev = _need_cuda(images.device, "crops")
    assert images.dtype == torch.uint8 and masks.dtype == torch.uint8 and boxes.dtype == torch.int32
    assert images.is_contiguous() and masks.is_contiguous() and boxes.is_contiguous()
    N, H, W = masks.shape
    assert images.shape == (N, H, W, 3) and boxes.shape == (N, 4) and masks.device == boxes.device == images.device
    rgb = torch.empty((N, CROP, CROP, 3), dtype=torch.float32, device=dev)
    msk = torch.empty((N, CROP, CROP), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        hip_lib.check(hip_lib.lib().soar_data_crops(N, H, W, hip_lib.ptr(images), hip_lib.ptr(masks), hip_lib.ptr(boxes), hip_lib.ptr(rgb),
                                                    hip_lib.ptr(msk), _stream(dev)), "soar_data_crops")
    return rgb, msk


class FrameStore:
    """A video sequence on the device: images / masks / normal maps as uint8, crops and cameras as float32."""

    def __init__(self):
        raise TypeError("use FrameStore.from_arrays(...) or FrameStore.from_dataroot(...)")

    @classmethod
    def from_arrays(cls, images, masks, normal_F, normal_B, normal_mask, Ks, normal_Ks, w2c, smpl_parms, device="cuda") -> "FrameStore":
        """images [N,H,W,3], masks [N,H,W] (non-zero = inside), normal_F / normal_B [N,512,512,3], normal_mask [N,512,512]: uint8 arrays
        or tensors; Ks [N,3,3] (or [3,3]), normal_Ks [N,3,3]; w2c [4,4], the extrinsic AFTER the reference's ``extrinsic[1:3] *= -1``;
        smpl_parms: betas, body_pose [N,..], global_orient [N,3], transl [N,3]."""
        self = object.__new__(cls)
        dev = self.device = _need_cuda(device, "FrameStore")
        u8 = lambda a: torch.as_tensor(a).to(torch.uint8).contiguous()
        f32 = lambda a: torch.as_tensor(a).detach().to("cpu", torch.float32).contiguous()
        images, masks = u8(images), (torch.as_tensor(masks) > 0).to(torch.uint8).contiguous()
        N, H, W = masks.shape
        if N < 1 or H < 1 or W < 1 or images.shape != (N, H, W, 3):
            raise ValueError(f"images {tuple(images.shape)} / masks {tuple(masks.shape)}: need [N,H,W,3] and [N,H,W] with N, H, W >= 1")
        normal_F, normal_B, normal_mask = u8(normal_F), u8(normal_B), u8(normal_mask)
        if normal_F.shape != (N, CROP, CROP, 3) or normal_B.shape != normal_F.shape or normal_mask.shape != (N, CROP, CROP):
            raise ValueError(f"normal maps must be [N,{CROP},{CROP},3] and [N,{CROP},{CROP}]")
        self.n_frames, self.height, self.width = N, H, W
        self.images, self.masks = images.to(dev), masks.to(dev)
        self.normal_F, self.normal_B, self.normal_mask = normal_F.to(dev), normal_B.to(dev), normal_mask.to(dev)
        Ks = f32(Ks)
        self.Ks_host = Ks.expand(N, 3, 3).contiguous() if Ks.dim() == 2 else Ks
        self.normal_Ks_host, self.w2c_host = f32(normal_Ks), f32(w2c)
        if self.Ks_host.shape != (N, 3, 3) or self.normal_Ks_host.shape != (N, 3, 3) or self.w2c_host.shape != (4, 4):
            raise ValueError("Ks / normal_Ks must be [N,3,3] and w2c [4,4]")
        self.Ks, self.normal_Ks, self.w2c = self.Ks_host.to(dev), self.normal_Ks_host.to(dev), self.w2c_host.to(dev)
        self.c2w_host = torch.inverse(self.w2c_host)
        self.smpl_parms_host = {k: f32(v) for k, v in smpl_parms.items()}
        self.smpl_parms = {k: v.to(dev) for k, v in self.smpl_parms_host.items()}
        # boxes and crops: two launches for the whole sequence; the boxes are looked at once, here, to refuse an empty mask
        self.boxes = mask_bbox(self.masks)
        boxes_host = self.boxes.cpu()
        empty = torch.nonzero(boxes_host[:, 2] < 0).reshape(-1).tolist()
        if empty:
            raise ValueError(f"frame {empty[0]} has an empty mask (frames without a mask: {empty}): no crop box")
        self.rgb_crop, self.mask_crop = crops(self.images, self.masks, self.boxes)
        self._frames_rays_d: Optional[torch.Tensor] = None
        return self

    @classmethod
    def from_dataroot(cls, path: str, smpl_type: str = "smplx", device="cuda", device_png: bool = False) -> "FrameStore":
        """The reference's directory layout (:114-244): ``read_dataroot`` on the host, then ``from_arrays``.  With ``device_png`` the
        four folders of PNG files are decoded on the device (soar_amd.png.read_png_files: only the files' bytes are uploaded) and
        ``read_dataroot``'s rules are applied there; the store is the same bit for bit.  That path reads 8-bit grey, RGB and RGBA
        files only, and every folder's files must agree in size and colour type."""
        dev = _need_cuda(device, "FrameStore")
        if device_png:
            return cls.from_arrays(**cls._read_dataroot_device(path, smpl_type, dev), device=device)
        return cls.from_arrays(**cls.read_dataroot(path, smpl_type), device=device)

    @staticmethod
    def _read_dataroot_device(path: str, smpl_type: str, dev: torch.device) -> Dict[str, Any]:
        """``read_dataroot`` with the PNG files decoded on the device: the same lists, rules and messages, on tensors that stay there
        (``from_arrays`` takes device tensors as they are).  Cameras and body parameters are read on the host as there."""
        import numpy as np
        from glob import glob
        from .png import read_png_files
        base = os.path.join(path, "train") if smpl_type == "smpl" else path
        img_list = sorted(glob(os.path.join(base, "images", "*.png")))
        mask_list = sorted(glob(os.path.join(base, "masks", "*.png")))
        nf_list = sorted(glob(os.path.join(path, "normal_F", "*.png")))
        nb_list = sorted(glob(os.path.join(path, "normal_B", "*.png")))
        if not img_list or not (len(img_list) == len(nf_list) == len(nb_list)):
            raise ValueError(f"{path}: {len(img_list)} images, {len(nf_list)} normal_F, {len(nb_list)} normal_B: the numbers must agree")
        img = read_png_files(img_list, dev)
        if img.shape[-1] == 4:
            mask, img = img[..., 3], img[..., :3]
        else:
            if len(mask_list) != len(img_list):
                raise ValueError(f"{path}: {len(img_list)} images without alpha but {len(mask_list)} masks")
            mask = read_png_files(mask_list, dev)[..., 0]
        if img.shape[-1] == 1:
            img = img.expand(-1, -1, -1, 3)
        f = read_png_files(nf_list, dev)
        if f.shape[-1] != 4:
            raise ValueError(f"{nf_list[0]}: normal_F needs an alpha channel (the normal mask)")
        nB = read_png_files(nb_list, dev)[..., :3]
        if smpl_type == "smpl":
            cam = np.load(os.path.join(path, "cameras.npz"))
            Ks, w2c = torch.from_numpy(np.array(cam["intrinsic"])).float(), torch.from_numpy(np.array(cam["extrinsic"])).float()
            if "normal_intrinsic" not in cam:
                raise ValueError(f"{path}/cameras.npz has no normal_intrinsic: the crops' rays need the normal maps' intrinsics")
            normal_Ks = torch.from_numpy(np.array(cam["normal_intrinsic"])).float()
            sp = dict(np.load(os.path.join(path, "poses_optimized.npz")))
        else:
            body = torch.load(os.path.join(path, "smplx", "params.pth"), map_location="cpu")
            w2c, Ks, normal_Ks, sp = body["w2c"].clone().float(), body["Ks"], body["normal_Ks"], dict(body)
        if "thetas" in sp:
            sp["body_pose"], sp["global_orient"] = sp["thetas"][..., 3:], sp["thetas"][..., :3]
        w2c[1:3] *= -1
        smpl = {k: torch.as_tensor(sp[k]).float() for k in ("betas", "body_pose", "global_orient", "transl")}
        return dict(images=img, masks=(mask > 0).to(torch.uint8), normal_F=f[..., :3], normal_B=nB, normal_mask=f[..., 3], Ks=Ks,
                    normal_Ks=normal_Ks, w2c=w2c, smpl_parms=smpl)

    @staticmethod
    def read_dataroot(path: str, smpl_type: str = "smplx") -> Dict[str, Any]:
        """Decodes a sequence directory with PIL into the host arrays ``from_arrays`` takes: images/, masks/ (or the images' alpha),
        normal_F/ (its alpha is the normal mask), normal_B/ and smplx/params.pth; for "smpl": train/images, train/masks, cameras.npz
        and poses_optimized.npz.  mask[mask > 0] = 1 and extrinsic[1:3] *= -1 as the reference does."""
        import numpy as np
        from glob import glob
        from PIL import Image
        base = os.path.join(path, "train") if smpl_type == "smpl" else path
        img_list = sorted(glob(os.path.join(base, "images", "*.png")))
        mask_list = sorted(glob(os.path.join(base, "masks", "*.png")))
        nf_list = sorted(glob(os.path.join(path, "normal_F", "*.png")))
        nb_list = sorted(glob(os.path.join(path, "normal_B", "*.png")))
        if not img_list or not (len(img_list) == len(nf_list) == len(nb_list)):
            raise ValueError(f"{path}: {len(img_list)} images, {len(nf_list)} normal_F, {len(nb_list)} normal_B: the numbers must agree")
        imgs, masks, nF, nB, nM = [], [], [], [], []
        for i, p in enumerate(img_list):
            img = np.array(Image.open(p))
            if img.ndim == 3 and img.shape[-1] == 4:
                mask, img = img[..., 3], img[..., :3]
            else:
                if len(mask_list) != len(img_list):
                    raise ValueError(f"{path}: {len(img_list)} images without alpha but {len(mask_list)} masks")
                mask = np.array(Image.open(mask_list[i]))
                mask = mask[..., 0] if mask.ndim == 3 else mask
            if img.ndim == 2:
                img = np.repeat(img[..., None], 3, axis=-1)
            imgs.append(img)
            masks.append((mask > 0).astype(np.uint8))
            f = np.array(Image.open(nf_list[i]))
            if f.ndim != 3 or f.shape[-1] != 4:
                raise ValueError(f"{nf_list[i]}: normal_F needs an alpha channel (the normal mask)")
            nF.append(f[..., :3])
            nM.append(f[..., 3])
            nB.append(np.array(Image.open(nb_list[i]))[..., :3])
        if smpl_type == "smpl":
            cam = np.load(os.path.join(path, "cameras.npz"))
            Ks, w2c = torch.from_numpy(np.array(cam["intrinsic"])).float(), torch.from_numpy(np.array(cam["extrinsic"])).float()
            if "normal_intrinsic" not in cam:
                raise ValueError(f"{path}/cameras.npz has no normal_intrinsic: the crops' rays need the normal maps' intrinsics")
            normal_Ks = torch.from_numpy(np.array(cam["normal_intrinsic"])).float()
            sp = dict(np.load(os.path.join(path, "poses_optimized.npz")))
        else:
            body = torch.load(os.path.join(path, "smplx", "params.pth"), map_location="cpu")
            w2c, Ks, normal_Ks, sp = body["w2c"].clone().float(), body["Ks"], body["normal_Ks"], dict(body)
        if "thetas" in sp:
            sp["body_pose"], sp["global_orient"] = sp["thetas"][..., 3:], sp["thetas"][..., :3]
        w2c[1:3] *= -1
        smpl = {k: torch.as_tensor(sp[k]).float() for k in ("betas", "body_pose", "global_orient", "transl")}
        return dict(images=np.stack(imgs), masks=np.stack(masks), normal_F=np.stack(nF), normal_B=np.stack(nB), normal_mask=np.stack(nM),
                    Ks=Ks, normal_Ks=normal_Ks, w2c=w2c, smpl_parms=smpl)

    def frames_rays_d(self) -> torch.Tensor:
        """[N,512,512,3]: the normalised rays of every frame's normal-map camera (:287-309), made once."""
        if self._frames_rays_d is None:
            out = torch.empty((self.n_frames, CROP, CROP, 3), dtype=torch.float32, device=self.device)
            a = hip_lib.SoarDataStepArgs()
            a.n_frames, a.normal_Ks = self.n_frames, hip_lib.ptr(self.normal_Ks)
            a.gt_c2w[:] = self.c2w_host.reshape(-1).tolist()
            with torch.cuda.device(self.device):
                for i in range(self.n_frames):
                    a.frame, a.gt_rays_d = i, out[i].data_ptr()
                    hip_lib.check(hip_lib.lib().soar_data_step_batch(C.byref(a), _stream(self.device)), "soar_data_step_batch")
            self._frames_rays_d = out
        return self._frames_rays_d


def split_indices(scene_length: int, split: str) -> List[int]:
    """train / val / test frames of a sequence (:137-154)."""
    num_val = scene_length // 5
    if num_val < 1:
        raise ValueError(f"a sequence of {scene_length} frames cannot be split: the reference sets one frame in five aside (it divides by zero here)")
    length = int(1 / (num_val) * scene_length)
    offset = length // 2
    val_list = list(range(scene_length))[offset::length]
    train_list = list(set(range(scene_length)) - set(val_list))
    test_list = val_list[:len(val_list) // 2]
    val_list = val_list[len(val_list) // 2:]
    return {"train": train_list, "val": val_list, "test": test_list}[split]


# the per-camera vectors a batch carries besides the images, in the order they are packed into the launch's `small` block
_SMALL_VIEW = (("c2w", 16), ("fovy", 1), ("elevation", 1), ("azimuth", 1), ("camera_distances", 1), ("camera_positions", 3),
               ("light_positions", 3))
_SMALL_GT = (("gt_c2w", 16), ("gt_fovx", 1), ("gt_fovy", 1), ("gt_cx", 1), ("gt_cy", 1), ("gt_normal_fovx", 1), ("gt_normal_fovy", 1),
             ("gt_normal_cx", 1), ("gt_normal_cy", 1), ("gt_near", 1))


@registry.register("mvdream-random-multiview-camera-datamodule")
class RandomMultiviewCameraDataset(registry.BaseObject):
    @dataclasses.dataclass
    class Config:
        # threestudio's RandomCameraDataModuleConfig
        height: Any = 64
        width: Any = 64
        batch_size: Any = 1
        resolution_milestones: List[int] = dataclasses.field(default_factory=lambda: [])
        eval_height: int = 512
        eval_width: int = 512
        eval_batch_size: int = 1
        n_val_views: int = 1
        n_test_views: int = 120
        elevation_range: Tuple[float, float] = (-10, 90)
        azimuth_range: Tuple[float, float] = (-180, 180)
        camera_distance_range: Tuple[float, float] = (1, 1.5)
        fovy_range: Tuple[float, float] = (40, 70)
        camera_perturb: float = 0.1
        center_perturb: float = 0.2
        up_perturb: float = 0.02
        light_position_perturb: float = 1.0
        light_distance_range: Tuple[float, float] = (0.8, 1.5)
        eval_elevation_deg: float = 15.0
        eval_camera_distance: float = 1.5
        eval_fovy_deg: float = 70.0
        light_sample_strategy: str = "dreamfusion"
        batch_uniform_azimuth: bool = True
        progressive_until: int = 0
        rays_d_normalize: bool = True
        # RandomMultiviewCameraDataModuleConfig (:93-105)
        dataroot: str = ""
        relative_radius: bool = True
        n_view: int = 1
        zoom_range: Tuple[float, float] = (1.0, 1.0)
        smpl_type: str = "smpl"
        index_range: Tuple[int, int] = (0, 1)
        occ_range: int = 405
        occ_mid: int = 451
        occ_width: int = 86

    cfg: Config

    def configure(self, store: Optional[FrameStore] = None, split: str = "train") -> None:
        cfg = self.cfg
        if store is None:
            store = FrameStore.from_dataroot(cfg.dataroot, cfg.smpl_type, device=self.device or "cuda")
        self.store, self.split, self.device = store, split, store.device
        self.heights = [cfg.height] if isinstance(cfg.height, int) else list(cfg.height)
        self.widths = [cfg.width] if isinstance(cfg.width, int) else list(cfg.width)
        self.batch_sizes = [cfg.batch_size] if isinstance(cfg.batch_size, int) else list(cfg.batch_size)
        assert len(self.heights) == len(self.widths) == len(self.batch_sizes)
        self.resolution_milestones = [-1] + list(cfg.resolution_milestones)
        if max(self.batch_sizes) > hip_lib.DATA_MAX_VIEWS:
            raise ValueError(f"batch_size {max(self.batch_sizes)}: a step carries at most {hip_lib.DATA_MAX_VIEWS} random views")
        if cfg.light_sample_strategy not in ("dreamfusion", "magic3d"):
            raise ValueError(f"Unknown light sample strategy: {cfg.light_sample_strategy}")
        self.elevation_range, self.azimuth_range = cfg.elevation_range, cfg.azimuth_range
        self.camera_distance_range, self.fovy_range, self.zoom_range = cfg.camera_distance_range, cfg.fovy_range, cfg.zoom_range
        self.n_frames, self.gt_height, self.gt_width = store.n_frames, store.height, store.width
        self.index_list = split_indices(self.n_frames, split)
        rng = tuple(cfg.index_range)
        if rng[1] == -1:
            rng = (0, self.n_frames)
        self.index_range = cfg.index_range = (max(0, rng[0]), min(self.n_frames, rng[1]))
        self.frames_rays_d = store.frames_rays_d()
        self._ring: List[Optional[dict]] = [None] * RING_DEPTH
        self._turn = 0
        self.update_step(0, 0)

    # ---- threestudio's Updateable / dataset surface ---------------------------------------------------------------------------------
    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False) -> None:
        size_ind = bisect.bisect_right(self.resolution_milestones, global_step) - 1
        self.height, self.width, self.batch_size = self.heights[size_ind], self.widths[size_ind], self.batch_sizes[size_ind]

    def __iter__(self):
        if self.split != "train":
            for i in range(len(self.index_list)):
                yield self[i]
            return
        while True:
            yield self.collate(None)

    def __len__(self) -> int:
        return len(self.index_list)

    def __getitem__(self, index: int) -> Dict[str, Any]:
        """ValDataset.__getitem__: the frames of the split in order (the cameras are drawn as in training)."""
        return self.collate(None, gt_index=self.index_list[index])

    # ---- the host side of a step: every random draw, in the reference's order (:340-633) ---------------------------------------
    def _draw(self, gt_index: Optional[int] = None) -> Dict[str, Any]:
        cfg, st = self.cfg, self.store
        assert self.batch_size % cfg.n_view == 0, f"batch_size ({self.batch_size}) must be dividable by n_view ({cfg.n_view})!"
        real_batch_size = self.batch_size // cfg.n_view
        if gt_index is None:
            gt_index = self.index_list[torch.randint(0, len(self.index_list), (1,)).item()]
        K, nK = st.Ks_host[gt_index], st.normal_Ks_host[gt_index]
        d: Dict[str, Any] = {"gt_index": gt_index, "gt_c2w": st.c2w_host.unsqueeze(0)}
        d["gt_fovy"] = (2 * torch.atan(self.gt_height / (2 * K[1, 1]))).unsqueeze(0)
        d["gt_fovx"] = (2 * torch.atan(self.gt_width / (2 * K[0, 0]))).unsqueeze(0)
        d["gt_cx"], d["gt_cy"] = K[0, 2].unsqueeze(0), K[1, 2].unsqueeze(0)
        gt_near = 0.1
        if cfg.smpl_type == "smplx":
            gt_near = st.smpl_parms_host["transl"][gt_index][-1].item() - 5.0
        d["gt_near_value"] = gt_near
        d["gt_near"] = torch.tensor(gt_near).unsqueeze(0)
        d["gt_normal_fovy"] = (2 * torch.atan(CROP / (2 * nK[1, 1]))).unsqueeze(0)
        d["gt_normal_fovx"] = (2 * torch.atan(CROP / (2 * nK[0, 0]))).unsqueeze(0)
        d["gt_normal_cx"], d["gt_normal_cy"] = nK[0, 2].unsqueeze(0), nK[1, 2].unsqueeze(0)

        if random.random() < 0.5:
            d["elevation_uniform"] = True
            elevation_deg = (torch.rand(real_batch_size) * (self.elevation_range[1] - self.elevation_range[0])
                             + self.elevation_range[0]).repeat_interleave(cfg.n_view, dim=0)
            elevation = elevation_deg * math.pi / 180
        else:
            d["elevation_uniform"] = False
            pct = [(self.elevation_range[0] + 90.0) / 180.0, (self.elevation_range[1] + 90.0) / 180.0]
            elevation = torch.asin(2 * (torch.rand(real_batch_size) * (pct[1] - pct[0]) + pct[0]) - 1.0).repeat_interleave(cfg.n_view, dim=0)
            elevation_deg = elevation / math.pi * 180.0
        azimuth_deg = (torch.rand(real_batch_size).reshape(-1, 1) + torch.arange(cfg.n_view).reshape(1, -1)).reshape(-1) / cfg.n_view * (
            self.azimuth_range[1] - self.azimuth_range[0]) + self.azimuth_range[0]
        azimuth = azimuth_deg * math.pi / 180
        fovy_deg = (torch.rand(real_batch_size) * (self.fovy_range[1] - self.fovy_range[0])
                    + self.fovy_range[0]).repeat_interleave(cfg.n_view, dim=0)
        fovy = fovy_deg * math.pi / 180
        camera_distances = (torch.rand(real_batch_size) * (self.camera_distance_range[1] - self.camera_distance_range[0])
                            + self.camera_distance_range[0]).repeat_interleave(cfg.n_view, dim=0)
        if cfg.relative_radius:
            camera_distances = 1 / torch.tan(0.5 * fovy) * camera_distances
        zoom = (torch.rand(real_batch_size) * (self.zoom_range[1] - self.zoom_range[0]) + self.zoom_range[0]).repeat_interleave(cfg.n_view, dim=0)
        fovy = fovy * zoom
        camera_positions = torch.stack([camera_distances * torch.cos(elevation) * torch.cos(azimuth),
                                        camera_distances * torch.cos(elevation) * torch.sin(azimuth),
                                        camera_distances * torch.sin(elevation)], dim=-1)
        center = torch.zeros_like(camera_positions)
        up = torch.as_tensor([0, 0, 1], dtype=torch.float32)[None, :].repeat(self.batch_size, 1)
        camera_positions = camera_positions + (torch.rand(real_batch_size, 3) * 2 * cfg.camera_perturb
                                               - cfg.camera_perturb).repeat_interleave(cfg.n_view, dim=0)
        center = center + (torch.randn(real_batch_size, 3) * cfg.center_perturb).repeat_interleave(cfg.n_view, dim=0)
        up = up + (torch.randn(real_batch_size, 3) * cfg.up_perturb).repeat_interleave(cfg.n_view, dim=0)
        light_distances = (torch.rand(real_batch_size) * (cfg.light_distance_range[1] - cfg.light_distance_range[0])
                           + cfg.light_distance_range[0]).repeat_interleave(cfg.n_view, dim=0)
        if cfg.light_sample_strategy == "dreamfusion":
            light_direction = F.normalize(camera_positions + torch.randn(real_batch_size, 3).repeat_interleave(cfg.n_view, dim=0)
                                          * cfg.light_position_perturb, dim=-1)
            light_positions = light_direction * light_distances[:, None]
        else:                                                   # "magic3d" (checked in configure)
            local_z = F.normalize(camera_positions, dim=-1)
            local_x = F.normalize(torch.stack([local_z[:, 1], -local_z[:, 0], torch.zeros_like(local_z[:, 0])], dim=-1), dim=-1)
            local_y = F.normalize(torch.cross(local_z, local_x, dim=-1), dim=-1)
            rot = torch.stack([local_x, local_y, local_z], dim=-1)
            light_azimuth = (torch.rand(real_batch_size) * math.pi - 2 * math.pi).repeat_interleave(cfg.n_view, dim=0)
            light_elevation = (torch.rand(real_batch_size) * math.pi / 3 + math.pi / 6).repeat_interleave(cfg.n_view, dim=0)
            local = torch.stack([light_distances * torch.cos(light_elevation) * torch.cos(light_azimuth),
                                 light_distances * torch.cos(light_elevation) * torch.sin(light_azimuth),
                                 light_distances * torch.sin(light_elevation)], dim=-1)
            light_positions = (rot @ local[:, :, None])[:, :, 0]
        lookat = F.normalize(center - camera_positions, dim=-1)
        right = F.normalize(torch.cross(lookat, up, dim=-1), dim=-1)
        up = F.normalize(torch.cross(right, lookat, dim=-1), dim=-1)
        c2w3x4 = torch.cat([torch.stack([right, up, -lookat], dim=-1), camera_positions[:, :, None]], dim=-1)
        c2w = torch.cat([c2w3x4, torch.zeros_like(c2w3x4[:, :1])], dim=1)
        c2w[:, 3, 3] = 1.0
        d.update(c2w=c2w, fovy=fovy, elevation=elevation_deg, azimuth=azimuth_deg, camera_distances=camera_distances,
                 camera_positions=camera_positions, light_positions=light_positions,
                 focal_length=0.5 * self.height / torch.tan(0.5 * fovy), tan_half=torch.tan(fovy / 2.0),
                 gt_tan_half=torch.tan(d["gt_fovy"] / 2.0))
        return d

    # ---- the device side: one launch ------------------------------------------------------------------------------------------------
    def _slot(self, B: int, H: int, W: int) -> dict:
        """the next batch of the ring (its images are allocated once per resolution)"""
        i, self._turn = self._turn % RING_DEPTH, self._turn + 1
        slot = self._ring[i]
        if slot is None or slot["key"] != (B, H, W):
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
            Hv, Wv = self.gt_height, self.gt_width
            slot = self._ring[i] = {
                "key": (B, H, W), "rays_d": new(B, H, W, 3), "cam_d": new(B, H, W, 3), "gt_rays_d": new(1, CROP, CROP, 3),
                "gt_cam_d": new(1, CROP, CROP, 3), "gt_rgb": new(1, Hv, Wv, 3), "gt_mask": new(1, Hv, Wv),
                "gt_normal_F": new(1, CROP, CROP, 3), "gt_normal_B": new(1, CROP, CROP, 3), "gt_normal_mask": new(1, CROP, CROP),
                "gt_rgb_crop": new(1, CROP, CROP, 3), "gt_mask_crop": new(1, CROP, CROP), "mvp_mtx": new(B, 4, 4), "proj": new(B, 4, 4),
                "gt_mvp_mtx": new(1, 4, 4), "small_out": new(hip_lib.DATA_SMALL_FLOATS)}
        return slot

    def collate(self, batch=None, gt_index: Optional[int] = None) -> Dict[str, Any]:
        """The batch dict of :635-680.  Tensors live on the device, in the dataset's ring: valid for RING_DEPTH further calls."""
        st, cfg = self.store, self.cfg
        d = self._draw(gt_index)
        B, H, W = self.batch_size, self.height, self.width
        slot = self._slot(B, H, W)
        a = hip_lib.SoarDataStepArgs()
        a.B, a.H, a.W, a.n_frames, a.Hv, a.Wv, a.frame = B, H, W, st.n_frames, st.height, st.width, d["gt_index"]
        a.rays_d_normalize, a.gt_has_cxcy = int(bool(cfg.rays_d_normalize)), int(cfg.smpl_type != "smpl")
        a.near_plane, a.far_plane, a.gt_near = 0.1, 1000.0, d["gt_near_value"]
        flat = d["c2w"].reshape(B, 16).tolist()
        focal, tan_half = d["focal_length"].tolist(), d["tan_half"].tolist()
        for b in range(B):
            a.c2w[b][:] = flat[b]
            a.focal[b], a.tan_half[b] = focal[b], tan_half[b]
        a.gt_c2w[:] = d["gt_c2w"].reshape(-1).tolist()
        a.gt_tan_half, a.gt_cx, a.gt_cy = d["gt_tan_half"].item(), d["gt_cx"].item(), d["gt_cy"].item()
        # the per-camera vectors ride along and come back as device tensors
        small: List[float] = []
        where: Dict[str, Tuple[int, int, int]] = {}
        for names, rows in ((_SMALL_VIEW, B), (_SMALL_GT, 1)):
            for name, width in names:
                where[name] = (len(small), rows, width)
                small.extend(d[name].reshape(-1).tolist())
        a.n_small = len(small)
        a.small[:len(small)] = small
        for name in ("images", "masks", "normal_F", "normal_B", "normal_mask", "rgb_crop", "mask_crop", "normal_Ks"):
            setattr(a, name, hip_lib.ptr(getattr(st, name)))
        for name in ("rays_d", "cam_d", "gt_rays_d", "gt_cam_d", "gt_rgb", "gt_mask", "gt_normal_F", "gt_normal_B", "gt_normal_mask",
                     "gt_rgb_crop", "gt_mask_crop", "mvp_mtx", "proj", "gt_mvp_mtx", "small_out"):
            setattr(a, name, hip_lib.ptr(slot[name]))
        with torch.cuda.device(self.device):
            hip_lib.check(hip_lib.lib().soar_data_step_batch(C.byref(a), _stream(self.device)), "soar_data_step_batch")
        self._last_args = a                    # (scripts/data_time.py issues the same launch again to time it alone)

        def vec(name):
            at, rows, width = where[name]
            v = slot["small_out"][at:at + rows * width]
            return v.view(rows, 4, 4) if width == 16 else (v.view(rows, width) if width > 1 else v)

        out = {k: slot[k] for k in ("rays_d", "cam_d", "mvp_mtx", "gt_rays_d", "gt_cam_d", "gt_mvp_mtx", "gt_rgb", "gt_mask", "gt_rgb_crop",
                                    "gt_mask_crop", "gt_normal_F", "gt_normal_B", "gt_normal_mask")}
        out.update({name: vec(name) for name, _ in _SMALL_VIEW + _SMALL_GT})
        # rays_o is the translation column, expanded as in get_rays (no memory of its own)
        out["rays_o"] = out["c2w"][:, None, None, :3, 3].expand(B, H, W, 3)
        out["gt_rays_o"] = out["gt_c2w"][:, None, None, :3, 3].expand(1, CROP, CROP, 3)
        i = d["gt_index"]
        sp = st.smpl_parms
        out.update(frames_rays_d=self.frames_rays_d, proj_mtx=slot["proj"], height=H, width=W, gt_index=i, gt_normal_res=CROP,
                   gt_height=self.gt_height, gt_width=self.gt_width,
                   gt_smpl={"betas": sp["betas"][None], "body_pose": sp["body_pose"][i][None], "global_orient": sp["global_orient"][i][None],
                            "transl": sp["transl"][i][None]})
        return out
