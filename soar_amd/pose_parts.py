"""Hand and face keypoint detection: what ``openpose.bin --hand --face`` adds to the body keypoints in the reference's
``preproc/compute_kp_and_mask.py``, on HIP kernels (csrc/pose_parts.hip and the shared convolution, csrc/conv_gemm.hip).  DESIGN.md 9zb
states the computation.

* ``CpmNet(state_dict)``: a convolutional pose machine from a torch state dict whose keys are the Caffe layer names plus ``.weight`` /
  ``.bias``; the hand network (22 maps) and the face network (71 maps) are the same design.  Every width, the number of stages, the
  number of maps and every layer's kernel side (1, 3 or 7) are read from the shapes and the key names.
  ``forward(x [M,3,S,S])`` -> ``heat [M,S/8,S/8,n_maps]``.
* ``part_boxes(people, n_people)`` -> the rectangles of the left hand, the right hand and the face, from the body keypoints;
  ``crop_parts(images, boxes)`` -> the two networks' inputs; ``part_keypoints(heat, boxes, which)`` -> each map's maximum in image pixels.
* ``detect_parts`` composes them; ``pose.detect_sequence(..., hand_net=, face_net=)`` fills rows 25:137 of its result with them.

**The network's structure, the concatenation order, the rectangle rules, their thresholds and the mirrored side are stated from the
published code as remembered; they have not been compared with OpenPose or its weights** (neither is available to the tests).  **The
crop is not OpenCV's ``warpAffine`` bit for bit** (see ``crop_parts``).  Detection is single-scale (``--hand_scale_number 1``,
OpenPose's default), and nothing is tracked between frames.  HIP only: CPU tensors are refused, there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, List, Mapping, Optional, Tuple

import torch
from torch import nn

from . import hip_lib
from .hip_lib import PackedWeights, _bytes, _stream, _workspace, check
from .pose import N_FACE, N_HAND, N_PARTS

# ---- the tables, in one place (from the published code as remembered, unchecked) ----
FRONT = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv3_4", "conv4_1", "conv4_2", "conv4_3", "conv4_4",
         "conv5_1", "conv5_2", "conv5_3_CPM")
POOL_AFTER = ("conv1_2", "conv2_2", "conv3_4")
STAGE_1 = ("conv6_1_CPM", "conv6_2_CPM")
N_MCONV = 7                                     # Mconv1_stage{s} .. Mconv7_stage{s}, s = 2 .. n
# what a later stage's first convolution reads, in the order of its weights' input channels
STAGE_INPUT = ("maps", "features")
# the body keypoints the rectangles are made of (BODY_25 indices)
HAND_JOINTS = {"left": (5, 6, 7), "right": (2, 3, 4)}         # shoulder, elbow, wrist
FACE_JOINTS = dict(neck=1, nose=0, r_eye=15, l_eye=16, r_ear=17, l_ear=18)
MIRRORED_HAND = "left"                          # its crop is flipped, so that one network serves both hands
BOX_DEFAULTS = dict(hand_min_conf=0.03, min_hand_area=10.0, face_min_conf=0.25, min_face_area=40.0)
HANDS, FACE = 0, 1                              # `which` of soar_part_keypoints


def layer_names(n_stages: int) -> List[str]:
    """Every convolution's layer name, in the order of the layers."""
    return list(FRONT) + list(STAGE_1) + [f"Mconv{j}_stage{s}" for s in range(2, n_stages + 1) for j in range(1, N_MCONV + 1)]


def _gives_maps(name: str) -> bool:
    return name == STAGE_1[1] or name.startswith(f"Mconv{N_MCONV}_")


def layer_keys(cfg: Mapping) -> List[Tuple[str, Tuple[int, int, int, int]]]:
    """(layer name, weight shape) of every convolution, in the order of the layers."""
    names = layer_names(cfg["n_stages"])
    feat, out = cfg["width"][len(FRONT) - 1], []
    for i, name in enumerate(names):
        if i == 0:
            cin = 3
        elif name.startswith("Mconv1_"):
            cin = cfg["n_maps"] + feat
        else:
            cin = feat if name == STAGE_1[0] else cfg["width"][i - 1]
        out.append((name, (cfg["n_maps"] if _gives_maps(name) else cfg["width"][i], cin, cfg["side"][i], cfg["side"][i])))
    return out


def read_config(state_dict: Mapping[str, torch.Tensor]) -> Dict:
    """``dict(n_stages, n_maps, width=[...], side=[...])`` from the shapes and the key names of a state dict.  ``KeyError`` for a
    missing key."""
    later = set()
    for key in state_dict:
        m = re.fullmatch(rf"Mconv{N_MCONV}_stage(\d+)\.weight", key)
        if m:
            later.add(int(m.group(1)))
    if later != set(range(2, 2 + len(later))):
        raise KeyError(f"CpmNet: the state dict has no stages 2 .. n (Mconv{N_MCONV}_stage<s>.weight: found {sorted(later)})")
    n_stages = 1 + len(later)
    width, side = [], []
    for name in layer_names(n_stages):
        key = f"{name}.weight"
        if key not in state_dict:
            raise KeyError(f"CpmNet: missing key '{key}'")
        shape = tuple(state_dict[key].shape)
        if len(shape) != 4 or shape[2] != shape[3]:
            raise ValueError(f"CpmNet: key '{key}' has shape {list(shape)}, expected [Cout, Cin, k, k]")
        width.append(int(shape[0]))
        side.append(int(shape[2]))
    return dict(n_stages=n_stages, n_maps=width[len(FRONT) + 1], width=width, side=side)


def _c_config(cfg: Mapping) -> hip_lib.SoarCpmConfig:
    c = hip_lib.SoarCpmConfig()
    c.n_stages, c.n_maps, c.n_layers = int(cfg["n_stages"]), int(cfg["n_maps"]), len(cfg["width"])
    c.pool_mask = sum(1 << FRONT.index(name) for name in POOL_AFTER)
    c.maps_first = int(STAGE_INPUT == ("maps", "features"))
    for i, (w, s) in enumerate(zip(cfg["width"], cfg["side"])):
        c.width[i], c.side[i] = int(w), int(s)
    return c


def _need_hip(who: str, **tensors) -> None:
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} is on '{t.device}': soar_amd.pose_parts runs on HIP devices only; there is no CPU fallback")


class CpmNet(nn.Module):
    """OpenPose's hand or face network in eval mode from its state dict.  The tensors are frozen buffers (``t{i}``, in the order of
    ``tensor_keys``); move the module with ``.to(device)``.  They are packed for the kernels once per device, on first use."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor]):
        super().__init__()
        sd = dict(state_dict)
        self.cfg = read_config(sd)
        c = self.cfg
        if c["n_stages"] > hip_lib.CPM_MAX_STAGES:
            raise ValueError(f"CpmNet: at most {hip_lib.CPM_MAX_STAGES} stages (got {c['n_stages']})")
        if c["n_maps"] < 2:
            raise ValueError(f"CpmNet: need at least 2 maps, the background among them (got {c['n_maps']})")
        names = layer_names(c["n_stages"])
        bad = {n: w for n, w in zip(names, c["width"]) if not _gives_maps(n) and (w < 8 or w % 8)}
        if bad:
            raise ValueError(f"CpmNet: every width but the maps' must be a multiple of 8 (got {bad})")
        bad = {n: s for n, s in zip(names, c["side"]) if s not in (1, 3, 7)}
        if bad:
            raise ValueError(f"CpmNet: a kernel side must be 1, 3 or 7 (got {bad})")
        self.tensor_keys: List[str] = []
        problems = []
        for name, shape in layer_keys(c):
            for key, want in ((f"{name}.weight", shape), (f"{name}.bias", shape[:1])):
                self.tensor_keys.append(key)
                if key not in sd:
                    problems.append(f"missing key '{key}' (expected shape {list(want)})")
                elif not isinstance(sd[key], torch.Tensor) or tuple(sd[key].shape) != tuple(want):
                    problems.append(f"key '{key}' has shape {list(getattr(sd[key], 'shape', ()))}, expected {list(want)}")
        if problems:
            missing = all(p.startswith("missing") for p in problems)
            raise (KeyError if missing else ValueError)("CpmNet: " + "; ".join(problems))
        for i, key in enumerate(self.tensor_keys):
            self.register_buffer(f"t{i}", sd[key].detach().to(torch.float32).contiguous().clone())
        self._pack = PackedWeights()
        self.eval()

    @property
    def n_maps(self) -> int:
        return self.cfg["n_maps"]

    def _tensors(self) -> List[torch.Tensor]:
        return [getattr(self, f"t{i}") for i in range(len(self.tensor_keys))]

    def _packed(self, dev) -> torch.Tensor:
        def pack():
            L = hip_lib.lib()
            cfg = _c_config(self.cfg)
            nb, count = C.c_size_t(0), C.c_int32(0)
            check(L.soar_cpm_weights_size(C.byref(cfg), C.byref(nb), C.byref(count)), "soar_cpm_weights_size")
            ts = self._tensors()
            if count.value != len(ts):
                raise RuntimeError(f"CpmNet: the library lays out {count.value} tensors, the module holds {len(ts)}")
            arr = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
            sizes = (C.c_int64 * len(ts))(*[t.numel() for t in ts])
            p = _workspace(nb.value, dev)
            with torch.cuda.device(dev):
                check(L.soar_cpm_pack_weights(C.byref(cfg), arr, sizes, len(ts), p.data_ptr(), nb.value, _stream(dev)), "soar_cpm_pack_weights")
            return p

        return self._pack.get(self._tensors(), dev, f"CpmNet: weights are not on {dev}: move the module with .to('{dev}')", pack)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, return_stages: bool = False):
        """x: float32 ``[M,3,S,S]`` with any strides, S a multiple of 8 -> ``heat [M,S/8,S/8,n_maps]`` (the last map is the background).
        ``return_stages=True`` -> ``(heat, features [M,S/8,S/8,feat], [every stage's maps ...])``."""
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError(f"CpmNet: x must be a [M,3,S,S] tensor (got {tuple(getattr(x, 'shape', ()))})")
        _need_hip("CpmNet", x=x)
        if x.dtype != torch.float32:
            raise TypeError(f"CpmNet: x must be float32 (got {x.dtype})")
        M, _, S, _ = x.shape
        if S < 8 or S % 8:
            raise ValueError(f"CpmNet: S must be a multiple of 8, at least 8 (got {S})")
        dev, c = x.device, self.cfg
        h, n = S // 8, c["n_stages"]
        stages = {s: torch.empty((M, h, h, c["n_maps"]), dtype=torch.float32, device=dev) for s in (range(n) if return_stages else (n - 1,))}
        features = torch.empty((M, h, h, c["width"][len(FRONT) - 1]), dtype=torch.float32, device=dev) if return_stages else None
        if M:
            packed = self._packed(dev)
            L = hip_lib.lib()
            cfg = _c_config(c)
            ws = _workspace(_bytes(L.soar_cpm_workspace_size, "soar_cpm_workspace_size", C.byref(cfg), M, S), dev)
            a = hip_lib.SoarCpmArgs()
            a.M, a.S, a.x = M, S, x.data_ptr()
            for i in range(4):
                a.x_stride[i] = x.stride(i)
            a.features = None if features is None else features.data_ptr()
            for s, t in stages.items():
                a.stage_out[s] = t.data_ptr()
            with torch.cuda.device(dev):
                check(L.soar_cpm_forward(C.byref(cfg), packed.data_ptr(), C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)), "soar_cpm_forward")
        if return_stages:
            return stages[n - 1], features, [stages[s] for s in range(n)]
        return stages[n - 1]


def part_boxes(people: torch.Tensor, n_people: torch.Tensor, part_people: int = 1, hand_min_conf: float = BOX_DEFAULTS["hand_min_conf"],
               min_hand_area: float = BOX_DEFAULTS["min_hand_area"], face_min_conf: float = BOX_DEFAULTS["face_min_conf"],
               min_face_area: float = BOX_DEFAULTS["min_face_area"]) -> torch.Tensor:
    """people float32 ``[B,max_people,25,3]`` in image pixels and n_people int32 ``[B]`` as ``pose.detect`` returns them -> boxes float32
    ``[B,part_people,3,4]``: ``(x0, y0, side, valid)`` of the left hand, the right hand and the face of a frame's first ``part_people``
    persons; an invalid box (joints below the confidence threshold, too small, or no such person) is all zeros.  The rules are those of
    OpenPose's hand and face detectors as include/soar_hip.h states them.  One launch, nothing is read back."""
    _need_hip("part_boxes", people=people, n_people=n_people)
    if people.dim() != 4 or tuple(people.shape[2:]) != (N_PARTS, 3) or people.dtype != torch.float32:
        raise ValueError(f"part_boxes: people must be float32 [B,max_people,{N_PARTS},3] (got {people.dtype} {tuple(people.shape)})")
    B, max_people = people.shape[:2]
    if tuple(n_people.shape) != (B,) or n_people.dtype != torch.int32:
        raise ValueError(f"part_boxes: n_people must be int32 [{B}] (got {n_people.dtype} {tuple(n_people.shape)})")
    if int(part_people) < 1 or max_people < 1:
        raise ValueError(f"part_boxes: part_people and max_people must be >= 1 (got {part_people}, {max_people})")
    dev = people.device
    people, n_people = people.contiguous(), n_people.contiguous()
    boxes = torch.empty((B, int(part_people), 3, 4), dtype=torch.float32, device=dev)
    a = hip_lib.SoarPartBoxArgs()
    a.B, a.max_people, a.part_people = B, max_people, int(part_people)
    a.hand_min_conf, a.min_hand_area, a.face_min_conf, a.min_face_area = float(hand_min_conf), float(min_hand_area), float(face_min_conf), float(min_face_area)
    a.people, a.n_people, a.boxes = people.data_ptr(), n_people.data_ptr(), boxes.data_ptr()
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_part_boxes(C.byref(a), _stream(dev)), "soar_part_boxes")
    return boxes


def _check_boxes(who: str, boxes: torch.Tensor) -> None:
    if boxes.dim() != 4 or tuple(boxes.shape[2:]) != (3, 4) or boxes.dtype != torch.float32 or boxes.shape[1] < 1:
        raise ValueError(f"{who}: boxes must be float32 [B,part_people,3,4] (got {boxes.dtype} {tuple(boxes.shape)})")


def crop_parts(images: torch.Tensor, boxes: torch.Tensor, net_side: int = 368, hands: bool = True, faces: bool = True):
    """uint8 ``[B,H,W,3]`` RGB frames on the device and boxes ``[B,P,3,4]`` -> the two networks' inputs, float32
    ``(hands [B*P*2,3,S,S], faces [B*P,3,S,S])`` with ``S = net_side`` (``None`` for one that is switched off); a person's left hand
    comes before the right.  One launch for both.  With ``s = side / S`` crop pixel ``(u, v)`` samples the image at ``(x0 + u' s,
    y0 + v s)``, ``u' = S - 1 - u`` for the left hand, which is mirrored; integer coordinates are pixel centres.  Bilinear over the four
    neighbours in float32, a neighbour outside the image counting 0; channels reversed to BGR; ``v / 256 - 0.5``.  An invalid box's
    crop is all ``-0.5``.  There is no anti-aliasing when ``side > S``: that is OpenCV's ``warpAffine`` too, and this project's
    definition; OpenCV's fixed-point interpolation coefficients are not reproduced, so the crop is not its output bit for bit, and it
    is not measured against it."""
    _need_hip("crop_parts", images=images, boxes=boxes)
    if images.dim() != 4 or images.shape[-1] != 3 or images.dtype != torch.uint8 or images.shape[1] < 1 or images.shape[2] < 1:
        raise ValueError(f"crop_parts: images must be uint8 [B,H,W,3] (got {images.dtype} {tuple(images.shape)})")
    _check_boxes("crop_parts", boxes)
    B, H, W, _ = images.shape
    if boxes.shape[0] != B or boxes.device != images.device:
        raise ValueError(f"crop_parts: boxes must hold {B} frames on {images.device} (got {tuple(boxes.shape)} on {boxes.device})")
    if not isinstance(net_side, int) or net_side < 8 or net_side % 8:
        raise ValueError(f"crop_parts: net_side must be a multiple of 8, at least 8 (got {net_side})")
    if not hands and not faces:
        raise ValueError("crop_parts: neither hands nor faces asked for")
    P, S, dev = boxes.shape[1], net_side, images.device
    images, boxes = images.contiguous(), boxes.contiguous()
    out_h = torch.empty((B * P * 2, 3, S, S), dtype=torch.float32, device=dev) if hands else None
    out_f = torch.empty((B * P, 3, S, S), dtype=torch.float32, device=dev) if faces else None
    if B:
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_part_crop(B, H, W, P, S, images.data_ptr(), boxes.data_ptr(), None if out_h is None else out_h.data_ptr(),
                                               None if out_f is None else out_f.data_ptr(), _stream(dev)), "soar_part_crop")
    return out_h, out_f


def part_keypoints(heat: torch.Tensor, boxes: torch.Tensor, which: str, net_side: int = 368) -> torch.Tensor:
    """heat float32 ``[M,S/8,S/8,n_maps]`` of the crops ``crop_parts`` made from ``boxes`` (``which``: ``"hands"``, M = B*P*2, or
    ``"face"``, M = B*P) -> float32 ``[M,n_maps-1,3]``: per map ``(x, y, score)`` in image pixels.  The map is upsampled by 8 with
    ``pose_peaks``' bicubic rule and its maximum taken over all ``S x S`` positions, ties to the first in raster order; a maximum
    ``m > 0`` at ``(X, Y)`` gives ``(x0 + X' s, y0 + Y s, m)`` with ``s = side / S`` and ``X' = S - 1 - X`` for a left hand, anything
    else, an invalid box included, ``(0, 0, 0)``.  The background map (the last) is not read; there is no sub-pixel refinement."""
    _need_hip("part_keypoints", heat=heat, boxes=boxes)
    if which not in ("hands", "face"):
        raise ValueError(f"part_keypoints: which must be 'hands' or 'face' (got {which!r})")
    _check_boxes("part_keypoints", boxes)
    per = 2 if which == "hands" else 1
    M = boxes.shape[0] * boxes.shape[1] * per
    if heat.dim() != 4 or heat.dtype != torch.float32 or heat.shape[0] != M or heat.shape[1] != heat.shape[2] or heat.shape[3] < 2 \
            or 8 * heat.shape[1] != net_side or heat.device != boxes.device:
        raise ValueError(f"part_keypoints: heat must be float32 [{M},{net_side // 8},{net_side // 8},n_maps >= 2] on {boxes.device} "
                         f"(got {heat.dtype} {tuple(heat.shape)} on {heat.device})")
    heat, boxes = heat.contiguous(), boxes.contiguous()
    _, h, w, n_maps = heat.shape
    out = torch.empty((M, n_maps - 1, 3), dtype=torch.float32, device=heat.device)
    if M:
        with torch.cuda.device(heat.device):
            check(hip_lib.lib().soar_part_keypoints(M, h, w, n_maps, heat.data_ptr(), boxes.data_ptr(), HANDS if which == "hands" else FACE,
                                                    out.data_ptr(), _stream(heat.device)), "soar_part_keypoints")
    return out


@torch.no_grad()
def detect_parts(hand_net: Optional[CpmNet], face_net: Optional[CpmNet], images: torch.Tensor, people: torch.Tensor, n_people: torch.Tensor,
                 part_people: int = 1, net_side: int = 368, **box_thresholds) -> Tuple[torch.Tensor, torch.Tensor]:
    """uint8 ``[B,H,W,3]`` RGB frames on the device and the body keypoints of ``pose.detect`` -> ``(hands [B,P,2,21,3] (left, right),
    face [B,P,70,3])`` in image pixels: ``part_boxes`` (which takes ``box_thresholds``), ``crop_parts``, the networks, ``part_keypoints``.
    Either net may be ``None``: its rows are zeros.  A person or a part without a valid rectangle is all zeros."""
    for name, net, want in (("hand_net", hand_net, N_HAND + 1), ("face_net", face_net, N_FACE + 1)):
        if net is not None and (not isinstance(net, CpmNet) or net.n_maps != want):
            raise ValueError(f"detect_parts: {name} must be a CpmNet of {want} maps (got {getattr(net, 'n_maps', type(net).__name__)})")
    boxes = part_boxes(people, n_people, part_people, **box_thresholds)
    B, P = boxes.shape[:2]
    dev = boxes.device
    hands = torch.zeros((B, P, 2, N_HAND, 3), dtype=torch.float32, device=dev)
    face = torch.zeros((B, P, N_FACE, 3), dtype=torch.float32, device=dev)
    if B and (hand_net is not None or face_net is not None):
        xh, xf = crop_parts(images, boxes, net_side, hands=hand_net is not None, faces=face_net is not None)
        if hand_net is not None:
            hands = part_keypoints(hand_net(xh), boxes, "hands", net_side).view(B, P, 2, N_HAND, 3)
        if face_net is not None:
            face = part_keypoints(face_net(xf), boxes, "face", net_side).view(B, P, N_FACE, 3)
    return hands, face
