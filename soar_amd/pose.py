"""Body keypoint detection: the first half of the reference's ``preproc/compute_kp_and_mask.py`` (which shells out to
``openpose.bin``) on HIP kernels (csrc/pose.hip and the shared convolution, csrc/conv_gemm.hip).  DESIGN.md 9za states the computation.

* ``PoseNet(state_dict)``: OpenPose's BODY_25 body network from a torch state dict whose keys are the Caffe layer names plus
  ``.weight`` / ``.bias`` (a PReLU layer: ``.weight`` of shape ``[C]``).  Every size is read from the shapes and the key names.
  ``preprocess(images, net_height=368)`` makes the network's input, ``forward(x)`` -> ``(heat [B,h,w,26], paf [B,h,w,52])``.
* ``pose_peaks(heat)`` -> ``(peaks [B,26,max_peaks,3], counts [B,26])``; ``pose_assemble(peaks, counts, paf)`` ->
  ``(people [B,max_people,25,3], n_people [B])``; ``scale_keypoints`` maps net-input pixels to image pixels.
* ``detect(net, images)`` composes them; ``detect_sequence`` runs a sequence in chunks and returns the ``[N,137,3]`` array
  ``smplify.load_keypoints`` reads back from what ``save_keypoints`` writes (OpenPose's ``<stem>_keypoints.json``).

**The network's structure, the concatenation orders and the BODY_25 tables below are stated from the published model; they have not
been compared with OpenPose or its weights** (neither is available to the tests).  Hands and faces are two more networks
(``soar_amd.pose_parts``): ``detect_sequence`` and ``save_keypoints`` take them as options, and without them the 112 rows carry
confidence 0.  HIP only: CPU tensors are refused, there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import re
import warnings
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import hip_lib
from .hip_lib import PackedWeights, _bytes, _stream, _workspace, check

# ---- the tables of BODY_25, in one place (from the published model, unchecked) ----
PARTS = ("Nose", "Neck", "RShoulder", "RElbow", "RWrist", "LShoulder", "LElbow", "LWrist", "MidHip", "RHip", "RKnee", "RAnkle", "LHip",
         "LKnee", "LAnkle", "REye", "LEye", "REar", "LEar", "LBigToe", "LSmallToe", "LHeel", "RBigToe", "RSmallToe", "RHeel")
N_PARTS, N_HEAT, N_PAF = 25, 26, 52          # 25 parts and the background; 26 limbs x (x, y)
# the limbs (part a, part b), in the order in which they are assembled ...
PAIRS = ((1, 8), (1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (8, 9), (9, 10), (10, 11), (8, 12), (12, 13), (13, 14), (1, 0), (0, 15),
         (15, 17), (0, 16), (16, 18), (2, 17), (5, 18), (14, 19), (19, 20), (14, 21), (11, 22), (22, 23), (11, 24))
# ... and the PAF channels of each limb's x and y components
PAF_CHANNELS = ((0, 1), (14, 15), (22, 23), (16, 17), (18, 19), (24, 25), (26, 27), (6, 7), (2, 3), (4, 5), (8, 9), (10, 11), (12, 13),
                (30, 31), (32, 33), (36, 37), (34, 35), (38, 39), (20, 21), (28, 29), (40, 41), (42, 43), (44, 45), (46, 47), (48, 49),
                (50, 51))
# what a stage's first convolution reads, in the order of its weights' input channels: (branch, first stage or a later one)
STAGE_INPUTS = {("L2", True): ("features",), ("L2", False): ("features", "paf"),
                ("L1", True): ("features", "paf"), ("L1", False): ("features", "heat", "paf")}
# the network's output: (last heat maps, last PAF)
OUTPUT_ORDER = ("heat", "paf")
VGG = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv3_4", "conv4_1", "conv4_2", "conv4_3_CPM",
       "conv4_4_CPM")
VGG_PRELU = {"conv4_2": "prelu4_2", "conv4_3_CPM": "prelu4_3_CPM", "conv4_4_CPM": "prelu4_4_CPM"}
POOL_AFTER = ("conv1_2", "conv2_2", "conv3_4")
N_KEYPOINTS, N_HAND, N_FACE = 137, 21, 70
_WIDTH = {"features": None, "paf": N_PAF, "heat": N_HEAT}
CFG_FIELDS = ("c1", "c2", "c3", "c4", "cpm", "feat", "w0", "w1", "m0", "m1", "n_paf", "n_heat")


def layer_keys(cfg: Mapping[str, int]) -> List[Tuple[str, Optional[str], Tuple[int, int, int, int]]]:
    """(convolution's layer name, its PReLU's layer name or None, weight shape) of every convolution, in the order of the layers: the
    VGG front, the PAF branch's stages (L2), the heat-map branch's (L1)."""
    c = cfg
    widths = [(3, c["c1"]), (c["c1"], c["c1"]), (c["c1"], c["c2"]), (c["c2"], c["c2"]), (c["c2"], c["c3"]), (c["c3"], c["c3"]),
              (c["c3"], c["c3"]), (c["c3"], c["c3"]), (c["c3"], c["c4"]), (c["c4"], c["c4"]), (c["c4"], c["cpm"]), (c["cpm"], c["feat"])]
    out = [(name, VGG_PRELU.get(name), (co, ci, 3, 3)) for name, (ci, co) in zip(VGG, widths)]
    for branch, n_stages, maps in (("L2", c["n_paf"], N_PAF), ("L1", c["n_heat"], N_HEAT)):
        for s in range(n_stages):
            w, m = (c["w0"], c["m0"]) if s == 0 else (c["w1"], c["m1"])
            cin0 = sum(c["feat"] if k == "features" else _WIDTH[k] for k in STAGE_INPUTS[branch, s == 0])
            for b in range(1, 6):
                for j in range(3):
                    cin = w if j else (cin0 if b == 1 else 3 * w)
                    out.append((f"Mconv{b}_stage{s}_{branch}_{j}", f"Mprelu{b}_stage{s}_{branch}_{j}", (w, cin, 3, 3)))
            out.append((f"Mconv6_stage{s}_{branch}", f"Mprelu6_stage{s}_{branch}", (m, 3 * w, 1, 1)))
            out.append((f"Mconv7_stage{s}_{branch}", None, (maps, m, 1, 1)))
    return out


def read_config(state_dict: Mapping[str, torch.Tensor]) -> Dict[str, int]:
    """The network's sizes from the shapes and the key names of its state dict.  ``KeyError`` for a missing key."""
    def out_width(name):
        key = f"{name}.weight"
        if key not in state_dict:
            raise KeyError(f"PoseNet: missing key '{key}'")
        return int(state_dict[key].shape[0])

    stages = {"L2": set(), "L1": set()}
    for key in state_dict:
        m = re.fullmatch(r"Mconv7_stage(\d+)_(L[12])\.weight", key)
        if m:
            stages[m.group(2)].add(int(m.group(1)))
    for branch, found in stages.items():
        if not found or found != set(range(len(found))):
            raise KeyError(f"PoseNet: the state dict has no stages 0 .. n - 1 of branch {branch} (Mconv7_stage<s>_{branch}.weight: found {sorted(found)})")
    cfg = dict(c1=out_width("conv1_1"), c2=out_width("conv2_1"), c3=out_width("conv3_1"), c4=out_width("conv4_1"), cpm=out_width("conv4_3_CPM"),
               feat=out_width("conv4_4_CPM"), w0=out_width("Mconv1_stage0_L2_0"), m0=out_width("Mconv6_stage0_L2"),
               n_paf=len(stages["L2"]), n_heat=len(stages["L1"]))
    later = "Mconv1_stage1_L2_0" if cfg["n_paf"] > 1 else ("Mconv1_stage1_L1_0" if cfg["n_heat"] > 1 else None)
    cfg["w1"] = out_width(later) if later else cfg["w0"]
    cfg["m1"] = out_width(later.replace("Mconv1", "Mconv6")[:-2]) if later else cfg["m0"]
    return cfg


def net_size(height: int, width: int, net_height: int = 368) -> Tuple[int, int]:
    """The network's input size for frames of ``height x width``: ``net_height`` x (``net_height * width / height`` rounded up to a
    multiple of 16)."""
    if not isinstance(net_height, int) or net_height < 16 or net_height % 16:
        raise ValueError(f"PoseNet: net_height must be a multiple of 16, at least 16 (got {net_height})")
    return net_height, max(16, int(math.ceil(net_height * width / height / 16.0)) * 16)


def _c_config(cfg: Mapping[str, int]) -> hip_lib.SoarPoseConfig:
    c = hip_lib.SoarPoseConfig()
    for k in CFG_FIELDS:
        setattr(c, k, int(cfg[k]))
    return c


class PoseNet(nn.Module):
    """OpenPose's BODY_25 network in eval mode from its state dict.  The tensors are frozen buffers (``t{i}``, in the order of
    ``tensor_keys``); move the module with ``.to(device)``.  They are packed for the kernels once per device, on first use."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor]):
        super().__init__()
        sd = dict(state_dict)
        self.cfg = read_config(sd)
        bad = [k for k in CFG_FIELDS[:10] if self.cfg[k] < 8 or self.cfg[k] % 8]
        if bad:
            raise ValueError(f"PoseNet: every width must be a multiple of 8 (got {({k: self.cfg[k] for k in bad})})")
        if max(self.cfg["n_paf"], self.cfg["n_heat"]) > hip_lib.POSE_MAX_STAGES:
            raise ValueError(f"PoseNet: at most {hip_lib.POSE_MAX_STAGES} stages per branch (got {self.cfg['n_paf']} and {self.cfg['n_heat']})")
        self.tensor_keys: List[str] = []
        problems = []
        for conv, prelu, shape in layer_keys(self.cfg):
            for key, want in ((f"{conv}.weight", shape), (f"{conv}.bias", shape[:1])) + (((f"{prelu}.weight", shape[:1]),) if prelu else ()):
                self.tensor_keys.append(key)
                if key not in sd:
                    problems.append(f"missing key '{key}' (expected shape {list(want)})")
                elif not isinstance(sd[key], torch.Tensor) or tuple(sd[key].shape) != tuple(want):
                    problems.append(f"key '{key}' has shape {list(getattr(sd[key], 'shape', ()))}, expected {list(want)}")
        if problems:
            missing = all(p.startswith("missing") for p in problems)
            raise (KeyError if missing else ValueError)("PoseNet: " + "; ".join(problems))
        for i, key in enumerate(self.tensor_keys):
            self.register_buffer(f"t{i}", sd[key].detach().to(torch.float32).contiguous().clone())
        self._pack = PackedWeights()
        self.eval()

    def _tensors(self) -> List[torch.Tensor]:
        return [getattr(self, f"t{i}") for i in range(len(self.tensor_keys))]

    def _packed(self, dev) -> torch.Tensor:
        def pack():
            L = hip_lib.lib()
            cfg = _c_config(self.cfg)
            nb, count = C.c_size_t(0), C.c_int32(0)
            check(L.soar_pose_weights_size(C.byref(cfg), C.byref(nb), C.byref(count)), "soar_pose_weights_size")
            ts = self._tensors()
            if count.value != len(ts):
                raise RuntimeError(f"PoseNet: the library lays out {count.value} tensors, the module holds {len(ts)}")
            arr = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            sizes = (C.c_int64 * len(ts))(*[t.numel() for t in ts])
            p = _workspace(nb.value, dev)
            with torch.cuda.device(dev):
                check(L.soar_pose_pack_weights(C.byref(cfg), arr, sizes, len(ts), p.data_ptr(), nb.value, _stream(dev)), "soar_pose_pack_weights")
            return p

        return self._pack.get(self._tensors(), dev, f"PoseNet: weights are not on {dev}: move the module with .to('{dev}')", pack)

    @staticmethod
    @torch.no_grad()
    def preprocess(images: torch.Tensor, net_height: int = 368) -> torch.Tensor:
        """uint8 ``[B,H,W,3]`` RGB on the device -> the network's input, float32 ``[B,3,net_h,net_w]`` (a channels-last view): the
        channels reversed to BGR, resized with ``resize_images(..., filter="bilinear")`` (Pillow's rule on bytes: the project's
        definition; OpenPose resizes with OpenCV's ``warpAffine``, another rule, and this is not measured against it), ``v / 256 - 0.5``."""
        from .jpeg import resize_images
        _need_hip("preprocess", images=images)
        if images.dim() != 4 or images.shape[-1] != 3 or images.dtype != torch.uint8 or images.shape[1] < 1 or images.shape[2] < 1:
            raise ValueError(f"PoseNet.preprocess: images must be uint8 [B,H,W,3] (got {images.dtype} {tuple(images.shape)})")
        B, H, W, _ = images.shape
        nh, nw = net_size(H, W, net_height)
        small = resize_images(images, nh, nw, filter="bilinear")
        out = torch.empty((B, nh, nw, 3), dtype=torch.float32, device=images.device)
        with torch.cuda.device(images.device):
            check(hip_lib.lib().soar_pose_preprocess(B, nh, nw, small.data_ptr(), out.data_ptr(), _stream(images.device)), "soar_pose_preprocess")
        return out.permute(0, 3, 1, 2)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, return_stages: bool = False):
        """x: float32 ``[B,3,H,W]`` with any strides, H and W multiples of 16 -> ``(heat [B,H/8,W/8,26], paf [B,H/8,W/8,52])``.
        ``return_stages=True`` -> ``(features [B,h,w,feat], [every PAF stage's maps ..., every heat stage's maps ...])`` as well."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"PoseNet: x must be a [B,3,H,W] tensor (got {tuple(getattr(x, 'shape', ()))})")
        _need_hip("PoseNet", x=x)
        if x.dtype != torch.float32:
            raise TypeError(f"PoseNet: x must be float32 (got {x.dtype})")
        B, _, H, W = x.shape
        if H < 16 or W < 16 or H % 16 or W % 16:
            raise ValueError(f"PoseNet: H and W must be multiples of 16, at least 16 (got {H} x {W})")
        dev, c = x.device, self.cfg
        h, w = H // 8, W // 8
        n_stages = c["n_paf"] + c["n_heat"]
        wanted = range(n_stages) if return_stages else (c["n_paf"] - 1, n_stages - 1)
        stages = {s: torch.empty((B, h, w, N_PAF if s < c["n_paf"] else N_HEAT), dtype=torch.float32, device=dev) for s in wanted}
        features = torch.empty((B, h, w, c["feat"]), dtype=torch.float32, device=dev) if return_stages else None
        if B:
            packed = self._packed(dev)
            L = hip_lib.lib()
            cfg = _c_config(c)
            ws = _workspace(_bytes(L.soar_pose_workspace_size, "soar_pose_workspace_size", C.byref(cfg), B, H, W), dev)
            a = hip_lib.SoarPoseNetArgs()
            a.B, a.H, a.W, a.x = B, H, W, x.data_ptr()
            for i in range(4):
                a.x_stride[i] = x.stride(i)
            a.features = None if features is None else features.data_ptr()
            for s, t in stages.items():
                a.stage_out[s] = t.data_ptr()
            with torch.cuda.device(dev):
                check(L.soar_pose_forward(C.byref(cfg), packed.data_ptr(), C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)), "soar_pose_forward")
        heat, paf = stages[n_stages - 1], stages[c["n_paf"] - 1]
        if return_stages:
            return heat, paf, features, [stages[s] for s in range(n_stages)]
        return heat, paf


def _need_hip(who: str, **tensors) -> None:
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} is on '{t.device}': soar_amd.pose runs on HIP devices only; there is no CPU fallback")


def pose_peaks(heat: torch.Tensor, threshold: float = 0.05, max_peaks: int = 32, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """heat float32 ``[B,h,w,26]`` -> (peaks ``[B,26,max_peaks,3]`` (x, y, score) in net-input pixels, raster order; counts ``[B,26]``
    int32, the true numbers).  A strict maximum of its 3 x 3 neighbourhood above ``threshold`` in the map upsampled by 8 (bicubic) is a
    peak, so a plateau gives none; the background map (the last) is not read.  ``out=(peaks, counts)``: write into these; rows behind
    ``min(count, max_peaks)`` are left as they are (fresh tensors hold zeros there)."""
    _need_hip("pose_peaks", heat=heat)
    if heat.dim() != 4 or heat.shape[-1] != N_HEAT or heat.dtype != torch.float32:
        raise ValueError(f"pose_peaks: heat must be float32 [B,h,w,{N_HEAT}] (got {heat.dtype} {tuple(heat.shape)})")
    if not 1 <= int(max_peaks) <= hip_lib.POSE_MAX_PEAKS:
        raise ValueError(f"pose_peaks: max_peaks must be 1 .. {hip_lib.POSE_MAX_PEAKS} (got {max_peaks})")
    heat = heat.contiguous()
    B, h, w, P = heat.shape
    dev = heat.device
    if out is None:
        peaks = torch.zeros((B, P, max_peaks, 3), dtype=torch.float32, device=dev)
        counts = torch.zeros((B, P), dtype=torch.int32, device=dev)
    else:
        peaks, counts = out
        if (tuple(peaks.shape), peaks.dtype, tuple(counts.shape), counts.dtype) != ((B, P, max_peaks, 3), torch.float32, (B, P), torch.int32) \
                or not peaks.is_contiguous() or not counts.is_contiguous() or peaks.device != dev or counts.device != dev:
            raise ValueError("pose_peaks: out must be contiguous (float32 [B,26,max_peaks,3], int32 [B,26]) on the maps' device")
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_pose_peaks(B, h, w, heat.data_ptr(), float(threshold), int(max_peaks), peaks.data_ptr(), counts.data_ptr(),
                                            _stream(dev)), "soar_pose_peaks")
    return peaks, counts


def pose_assemble(peaks: torch.Tensor, counts: torch.Tensor, paf: torch.Tensor, inter_threshold: float = 0.05, min_above: float = 0.95,
                  min_parts: int = 3, min_score: float = 0.4, max_people: int = 8) -> Tuple[torch.Tensor, torch.Tensor]:
    """peaks, counts of ``pose_peaks`` and paf float32 ``[B,h,w,52]`` -> (people ``[B,max_people,25,3]`` in net-input pixels, a missing
    part ``(0, 0, 0)``; n_people ``[B]`` int32, the true numbers).  The PAF is read at the 1/8-resolution cell of a sample, not
    upsampled.  People come out in the order in which they were started."""
    _need_hip("pose_assemble", peaks=peaks, counts=counts, paf=paf)
    if peaks.dim() != 4 or peaks.shape[1] != N_HEAT or peaks.shape[3] != 3 or peaks.dtype != torch.float32:
        raise ValueError(f"pose_assemble: peaks must be float32 [B,{N_HEAT},max_peaks,3] (got {peaks.dtype} {tuple(peaks.shape)})")
    B, _, max_peaks, _ = peaks.shape
    if tuple(counts.shape) != (B, N_HEAT) or counts.dtype != torch.int32:
        raise ValueError(f"pose_assemble: counts must be int32 [{B},{N_HEAT}] (got {counts.dtype} {tuple(counts.shape)})")
    if paf.dim() != 4 or paf.shape[0] != B or paf.shape[-1] != N_PAF or paf.dtype != torch.float32:
        raise ValueError(f"pose_assemble: paf must be float32 [{B},h,w,{N_PAF}] (got {paf.dtype} {tuple(paf.shape)})")
    if not 1 <= int(max_people) <= hip_lib.POSE_MAX_PEOPLE or not 1 <= max_peaks <= hip_lib.POSE_MAX_PEAKS:
        raise ValueError(f"pose_assemble: max_people must be 1 .. {hip_lib.POSE_MAX_PEOPLE} and max_peaks 1 .. {hip_lib.POSE_MAX_PEAKS}")
    dev = peaks.device
    peaks, counts, paf = peaks.contiguous(), counts.contiguous(), paf.contiguous()
    people = torch.empty((B, max_people, N_PARTS, 3), dtype=torch.float32, device=dev)
    n_people = torch.empty((B,), dtype=torch.int32, device=dev)
    a = hip_lib.SoarPoseAssembleArgs()
    a.B, a.h, a.w, a.max_peaks, a.max_people, a.min_parts = B, paf.shape[1], paf.shape[2], max_peaks, int(max_people), int(min_parts)
    a.inter_threshold, a.min_above, a.min_score = float(inter_threshold), float(min_above), float(min_score)
    for i, ((pa, pb), (cx, cy)) in enumerate(zip(PAIRS, PAF_CHANNELS)):
        a.pair_a[i], a.pair_b[i], a.paf_x[i], a.paf_y[i] = pa, pb, cx, cy
    a.peaks, a.counts, a.paf, a.people, a.n_people = peaks.data_ptr(), counts.data_ptr(), paf.data_ptr(), people.data_ptr(), n_people.data_ptr()
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_pose_assemble(C.byref(a), _stream(dev)), "soar_pose_assemble")
    return people, n_people


def scale_keypoints(people: torch.Tensor, image_hw: Tuple[int, int], net_hw: Tuple[int, int]) -> torch.Tensor:
    """people ``[...,3]`` in net-input pixels -> a new tensor in image pixels: ``(x * W / net_w, y * H / net_h, score)``."""
    _need_hip("scale_keypoints", people=people)
    if people.shape[-1] != 3 or people.dtype != torch.float32:
        raise ValueError(f"scale_keypoints: people must be float32 [...,3] (got {people.dtype} {tuple(people.shape)})")
    out = people.contiguous().clone()
    with torch.cuda.device(out.device):
        check(hip_lib.lib().soar_pose_scale(out.numel() // 3, out.data_ptr(), float(image_hw[1]), float(net_hw[1]), float(image_hw[0]),
                                            float(net_hw[0]), _stream(out.device)), "soar_pose_scale")
    return out


@torch.no_grad()
def detect(net: PoseNet, images: torch.Tensor, net_height: int = 368, threshold: float = 0.05, max_peaks: int = 32, **thresholds):
    """uint8 ``[B,H,W,3]`` RGB frames on the device -> (people ``[B,max_people,25,3]`` in image pixels, n_people ``[B]``):
    ``preprocess``, the network, ``pose_peaks``, ``pose_assemble`` (which takes ``thresholds``), ``scale_keypoints``."""
    x = net.preprocess(images, net_height)
    heat, paf = net(x)
    peaks, counts = pose_peaks(heat, threshold, max_peaks)
    people, n_people = pose_assemble(peaks, counts, paf, **thresholds)
    return scale_keypoints(people, images.shape[1:3], x.shape[2:4]), n_people


def _read_chunk(paths: Sequence[str], dev) -> torch.Tensor:
    from . import jpeg, png
    ext = {os.path.splitext(p)[1].lower() for p in paths}
    if ext <= {".jpg", ".jpeg"}:
        return jpeg.read_jpeg_files(paths, dev, chunk=len(paths))[..., :3]
    if ext == {".png"}:
        return png.read_png_files(paths, dev, chunk=len(paths))[..., :3]
    raise ValueError(f"detect_sequence: frames must be .jpg / .jpeg or .png files (got {sorted(ext)})")


@torch.no_grad()
def detect_sequence(net: PoseNet, images_or_paths, chunk: int = 8, device=None, net_height: int = 368, hand_net=None, face_net=None,
                    part_net_side: int = 368, **thresholds) -> np.ndarray:
    """A sequence's keypoints, ``[N,137,3]`` float32 in image pixels: the first person's 25 body keypoints, then 112 rows of zeros
    unless ``hand_net`` / ``face_net`` (``pose_parts.CpmNet``) are given, which fill rows 25:46 (left hand), 46:67 (right hand) and
    67:137 (face) from crops of ``part_net_side``.  ``images_or_paths``: uint8 ``[N,H,W,3]`` RGB (moved to ``device``) or a list of
    picture files, decoded on the device; ``chunk`` frames go through the networks per call.  A frame with nobody in it is all zeros."""
    if chunk < 1:
        raise ValueError(f"detect_sequence: chunk must be >= 1 (got {chunk})")
    is_tensor = isinstance(images_or_paths, torch.Tensor)
    if device is None:
        device = images_or_paths.device if is_tensor and images_or_paths.is_cuda else next(net.buffers()).device
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"detect_sequence: device is '{dev}': soar_amd.pose runs on HIP devices only; there is no CPU fallback")
    N = len(images_or_paths)
    out = torch.zeros((N, N_KEYPOINTS, 3), dtype=torch.float32, device=dev)
    for i in range(0, N, chunk):
        part = images_or_paths[i:i + chunk]
        frames = part.to(dev) if is_tensor else _read_chunk(list(part), dev)
        people, n_people = detect(net, frames, net_height, **thresholds)
        out[i:i + chunk, :N_PARTS] = people[:, 0] * (n_people > 0).to(torch.float32)[:, None, None]
        if hand_net is not None or face_net is not None:
            from .pose_parts import detect_parts
            hands, face = detect_parts(hand_net, face_net, frames, people, n_people, 1, part_net_side)
            out[i:i + chunk, N_PARTS:N_PARTS + 2 * N_HAND] = hands[:, 0].reshape(-1, 2 * N_HAND, 3)
            out[i:i + chunk, N_PARTS + 2 * N_HAND:] = face[:, 0]
    return out.cpu().numpy()


def save_keypoints(kp_dir: str, people, n_people, stems: Sequence[str], hands=None, face=None) -> None:
    """Writes OpenPose's ``<stem>_keypoints.json`` per frame: ``version`` and ``people[]`` with ``pose_keypoints_2d`` (75 numbers),
    ``face_keypoints_2d`` (210), ``hand_left_keypoints_2d`` and ``hand_right_keypoints_2d`` (63 each).  ``people``
    ``[N,max_people,25,3]`` and ``n_people [N]`` as ``detect`` returns them (tensors or arrays); ``hands [N,P,2,21,3]`` and ``face
    [N,P,70,3]`` as ``pose_parts.detect_parts`` returns them, for a frame's first P persons: the others', and everybody's without the
    argument, are zeros.  A frame with nobody found gets one all-zero person, so that ``smplify.load_keypoints`` still reads it, and a
    warning names the frame."""
    people = people.detach().cpu().numpy() if isinstance(people, torch.Tensor) else np.asarray(people)
    n_people = n_people.detach().cpu().numpy() if isinstance(n_people, torch.Tensor) else np.asarray(n_people)
    people = people.astype(np.float32, copy=False)
    if people.ndim != 4 or people.shape[2:] != (N_PARTS, 3) or n_people.shape != people.shape[:1] or len(stems) != people.shape[0]:
        raise ValueError(f"save_keypoints: need people [N,max_people,25,3], n_people [N] and N stems (got {people.shape}, {n_people.shape}, {len(stems)})")
    def parts(t, name, tail):
        if t is None:
            return None
        t = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float32, copy=False)
        if t.ndim != 2 + len(tail) or t.shape[0] != people.shape[0] or t.shape[2:] != tail:
            raise ValueError(f"save_keypoints: need {name} [N,P,{','.join(map(str, tail))}] (got {t.shape})")
        return t

    hands, face = parts(hands, "hands", (2, N_HAND, 3)), parts(face, "face", (N_FACE, 3))
    os.makedirs(kp_dir, exist_ok=True)
    zeros = lambda n: [0.0] * (3 * n)
    # person q's rows of a part array, zeros where it has none
    rows_of = lambda t, i, q, n: zeros(n) if t is None or q >= t.shape[1] else [float(v) for v in t[i, q].reshape(-1)]
    for i, stem in enumerate(stems):
        n = min(int(n_people[i]), people.shape[1])
        if n == 0:
            warnings.warn(f"save_keypoints: nobody found in frame '{stem}': writing one all-zero person")
        rows = people[i, :n] if n else np.zeros((1, N_PARTS, 3), np.float32)
        doc = {"version": 1.3, "people": [{"person_id": [-1], "pose_keypoints_2d": [float(v) for v in row.reshape(-1)],
                                           "face_keypoints_2d": rows_of(face, i, q, N_FACE),
                                           "hand_left_keypoints_2d": rows_of(None if hands is None else hands[:, :, 0], i, q, N_HAND),
                                           "hand_right_keypoints_2d": rows_of(None if hands is None else hands[:, :, 1], i, q, N_HAND)}
                                          for q, row in enumerate(rows)]}
        with open(os.path.join(kp_dir, f"{stem}_keypoints.json"), "w") as fh:
            json.dump(doc, fh)
