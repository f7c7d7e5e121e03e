"""Avatar playback: look at a trained surfel avatar -- a turntable of one frame, or a key-pose sequence resampled to another frame rate.

Restates the reference's inference harness, TS/test/render_rot.py: load the checkpoint, turn the first frame's global orientation
through 36 steps, render every step and save ``rgb/``, ``normal/``, ``occ/`` (each with the mask as a fourth channel) and ``mask/``
PNGs.  The reference redoes everything per frame: the attribute field, the K = 30 skinning weights, the 55-step joint chain, about 8
torch kernels of LBS, two rasterizations, four float -> byte conversions and a device-to-host copy of float images.  Only the joint
transforms depend on the pose, so here

* the field and the blend weights are computed once per ``render`` call,
* the motion comes from one launch (csrc/playback.hip, soar_motion_resample: the turntable ``R0 Ry(2 pi i / n)`` and per-joint
  quaternion slerp between key poses), the joint transforms of all frames from another (``JointTransformer.hip``),
* the frames go through the renderer's batched path in chunks (``fused_view.render_step_views``: warp, preprocess, binning and blend
  of up to 8 frames per call, the occlusion pass fused into the blend),
* one launch per chunk packs the rendered frames into the four byte images (soar_playback_finish), so the host copies 13 bytes per
  pixel instead of 40.

HIP only: CPU tensors are refused.  (DESIGN.md 9k states the two kernels in full.)
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Any, Dict, Mapping, Optional, Sequence, Union

import torch

from . import hip_lib
from .hip_lib import _stream, check

JOINTS = 55
POSE_KEYS = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
POSE_WIDTHS = (3, 63, 3, 3, 3, 45, 45)             # the 165 floats of full_pose, in SMPLGuidance._full_pose's order
CKPT_PREFIX = "geometry."
FIELD_PREFIX = "geometry.attribute_field."
LEAF_KEYS = {"xyz": ("_xyz", 3), "rotation": ("_rotation", 4), "occ": ("_occ", 1), "colors": ("_colors", 3), "scaling": ("_scaling", 1)}
FIELD_HEADS = {"shs": (32, 3), "scales": (32, 1), "quats": (32, 4), "offsets": (34, 3), "opacities": (32, 1)}      # (inputs, outputs)
FIELD_LEVELS, FIELD_HIDDEN = 16, 64


# ---- the checkpoint ---------------------------------------------------------------------------------------------------------------
def field_state_keys() -> Dict[str, Optional[tuple]]:
    """The state-dict keys of the attribute field (``HashMLPField`` / the reference's ``HashMLPSDFField``) with their shapes; None
    where the shape is free (the tables' row count) or a scalar buffer."""
    keys: Dict[str, Optional[tuple]] = {"aabb": (2, 3), "max_res": (), "num_levels": (), "log2_hashmap_size": (),
                                        "encoding.hash_table": None, "quat_encoding.hash_table": None}
    for h, (n_in, n_out) in FIELD_HEADS.items():
        keys[f"mlp_base_{h}.layers.0.weight"] = (FIELD_HIDDEN, n_in)
        keys[f"mlp_base_{h}.layers.0.bias"] = (FIELD_HIDDEN,)
        keys[f"mlp_base_{h}.layers.1.weight"] = (n_out, FIELD_HIDDEN)
        keys[f"mlp_base_{h}.layers.1.bias"] = (n_out,)
    return keys


def map_checkpoint(ckpt: Mapping[str, Any]) -> Dict[str, Any]:
    """The reference's Lightning checkpoint (or its ``state_dict``) -> ``{"xyz", "rotation", "occ", "colors", "scaling"}`` (raw leaves,
    [P,3], [P,4], [P,1], [P,3], [P,1]), ``"aabb"`` [2,3], ``"field"`` (the attribute field's state dict, prefix stripped) and
    ``"log2_hashmap_size"`` (from the tables' row count).  The key names are render_rot.py's: ``geometry._xyz``, ``_rotation``,
    ``_occ``, ``_colors``, ``_scaling`` and ``geometry.attribute_field.*``.  A pure function of the mapping: nothing is moved or
    copied.  A missing key raises KeyError, a misshapen one ValueError, both naming the key."""
    sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt

    def take(key):
        if key not in sd:
            raise KeyError(f"checkpoint has no '{key}'")
        return sd[key]

    out: Dict[str, Any] = {}
    P = None
    for name, (attr, width) in LEAF_KEYS.items():
        key = CKPT_PREFIX + attr
        t = take(key)
        if t.dim() != 2 or t.shape[1] != width or (P is not None and t.shape[0] != P):
            raise ValueError(f"checkpoint key '{key}' has shape {tuple(t.shape)}; expected [{'P' if P is None else P}, {width}]")
        P = t.shape[0]
        out[name] = t
    field = {}
    for k, shape in field_state_keys().items():
        key = FIELD_PREFIX + k
        t = take(key)
        if shape is not None and tuple(t.shape) != shape:
            raise ValueError(f"checkpoint key '{key}' has shape {tuple(t.shape)}; expected {list(shape)}")
        field[k] = t
    log2 = None
    for k in ("encoding.hash_table", "quat_encoding.hash_table"):
        t = field[k]
        rows = t.shape[0] // FIELD_LEVELS if t.dim() == 2 else 0
        if t.dim() != 2 or t.shape[1] != 2 or rows * FIELD_LEVELS != t.shape[0] or rows < 2 or rows & (rows - 1) or \
                (log2 is not None and rows != 1 << log2):
            raise ValueError(f"checkpoint key '{FIELD_PREFIX + k}' has shape {tuple(t.shape)}; expected [{FIELD_LEVELS} * 2^n, 2], "
                             "the same n for both tables")
        log2 = rows.bit_length() - 1
    out["aabb"], out["field"], out["log2_hashmap_size"] = field["aabb"], field, log2
    return out


class CheckpointSurfels:
    """The geometry duck type of render_rot.py:16-51 over a checkpoint's leaves: what the renderer plugin reads (``get_xyz``,
    ``get_rotation``, ``get_opacity``, ``get_occ``, ``get_scaling``, ``get_colors``, ``attribute_field``, ``smpl_guidance``,
    ``active_sh_degree``, ``config``).  The activations are the reference's (sigmoid of colours and occlusion, exp of the scales);
    the rotations are normalised, which the reference leaves to ``quaternion_to_matrix`` (it divides by the squared length)."""

    def __init__(self, xyz, rotation, occ, colors, scaling, attribute_field, smpl_guidance):
        with torch.no_grad():
            self._xyz = xyz.detach().float().contiguous()
            self._rotation = torch.nn.functional.normalize(rotation.detach().float()).contiguous()
            self._occ = torch.sigmoid(occ.detach().float()).contiguous()
            self._colors = torch.sigmoid(colors.detach().float()).contiguous()
            self._scaling = torch.exp(scaling.detach().float()).contiguous()
        self.attribute_field = attribute_field
        self.smpl_guidance = smpl_guidance
        self.active_sh_degree = 0
        self.config = torch.tensor([1.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=self._xyz.device)

    get_xyz = property(lambda s: s._xyz)
    get_rotation = property(lambda s: s._rotation)
    get_opacity = property(lambda s: torch.ones_like(s._xyz))
    get_occ = property(lambda s: s._occ)
    get_scaling = property(lambda s: s._scaling)
    get_colors = property(lambda s: s._colors)


# ---- the two kernels --------------------------------------------------------------------------------------------------------------
def _need_hip(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on '{t.device}': soar_amd.playback runs on HIP devices only; there is no CPU fallback")


def motion_resample(key_pose: torch.Tensor, key_transl: torch.Tensor, key_expr: torch.Tensor, times: torch.Tensor,
                    yaw: Optional[torch.Tensor] = None):
    """key_pose [K,165] or [K,55,3] (axis-angle, full_pose order), key_transl [K,3], key_expr [K,E], times [F] in key units (clamped
    to [0, K - 1]), yaw [F] radians or None -> pose [F,165], transl [F,3], expr [F,E].  Per joint quaternion slerp along the shorter
    arc, the root joint turned by ``Ry(yaw)`` on the right, transl / expr linear; on a key (and without a turn) the key's numbers come
    back as they are.  One launch on the current stream (soar_motion_resample), no synchronisation."""
    for name, t in (("key_pose", key_pose), ("key_transl", key_transl), ("key_expr", key_expr), ("times", times)):
        _need_hip(t, name)
    dev = key_pose.device
    f = lambda t: t.detach().to(device=dev, dtype=torch.float32).contiguous()
    kp = f(key_pose).reshape(-1, JOINTS * 3)
    K = kp.shape[0]
    kt, ke, tm = f(key_transl).reshape(-1, 3), f(key_expr).reshape(K, -1) if K else f(key_expr), f(times).reshape(-1)
    yw = None if yaw is None else f(yaw).reshape(-1)
    F, E = tm.shape[0], ke.shape[1]
    if K < 1 or kt.shape[0] != K or (yw is not None and yw.shape[0] != F):
        raise ValueError(f"motion_resample: key_pose [K,165], key_transl [K,3], key_expr [K,E] with K >= 1 and yaw [F] like times expected "
                         f"(got {tuple(key_pose.shape)}, {tuple(key_transl.shape)}, {tuple(key_expr.shape)}, times {tuple(times.shape)}, "
                         f"yaw {None if yaw is None else tuple(yaw.shape)})")
    pose = torch.empty((F, JOINTS * 3), dtype=torch.float32, device=dev)
    transl = torch.empty((F, 3), dtype=torch.float32, device=dev)
    expr = torch.empty((F, E), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_motion_resample(K, F, E, hip_lib.ptr(kp), hip_lib.ptr(kt), hip_lib.ptr(ke), hip_lib.ptr(tm),
                                                 hip_lib.ptr(yw), hip_lib.ptr(pose), hip_lib.ptr(transl), hip_lib.ptr(expr),
                                                 _stream(dev)), "soar_motion_resample")
    return pose, transl, expr


def playback_finish(render: torch.Tensor, normal: torch.Tensor, mask: torch.Tensor, occ: Optional[torch.Tensor] = None,
                    normal_as_rgb: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """render, normal, occ [B,3,H,W], mask [B,1,H,W] (float32 on the device; every frame contiguous, any stride from frame to frame;
    occ may be None) -> ``rgb``, ``normal``, ``occ`` (None without occ): uint8 [B,H,W,4], the image with the mask as fourth channel,
    and ``mask``: uint8 [B,H,W].  The conversion is torchvision's ``save_image`` rule, ``x.mul(255).add_(0.5).clamp_(0, 255).to(uint8)``
    (multiply, add, clamp, truncate); NaN gives 0, which torch leaves undefined.  ``normal_as_rgb``: the normal is ``n * 0.5 + 0.5``
    first (off by default: the reference saves ``out['normal']`` as it is).  ``out``: contiguous tensors to write into.  One launch
    on the current stream (soar_playback_finish), no synchronisation."""
    B, _, H, W = render.shape
    ins = [("render", render, 3), ("normal", normal, 3), ("mask", mask, 1)] + ([("occ", occ, 3)] if occ is not None else [])
    dev = render.device
    for name, t, c in ins:
        _need_hip(t, name)
        if t.dtype != torch.float32 or tuple(t.shape) != (B, c, H, W) or t.device != dev:
            raise ValueError(f"playback_finish: {name} must be float32 [{B},{c},{H},{W}] on {dev} (got {t.dtype} {tuple(t.shape)} on {t.device})")
    # a frame's planes must be contiguous; the step from frame to frame is free (the renderer leaves its frames 18 planes apart)
    ins = [(name, t if (B == 0 or t[0].is_contiguous()) and (B < 2 or t.stride(0) >= c * H * W) else t.contiguous(), c) for name, t, c in ins]
    if out is None:
        out = {"rgb": torch.empty((B, H, W, 4), dtype=torch.uint8, device=dev), "normal": torch.empty((B, H, W, 4), dtype=torch.uint8, device=dev),
               "occ": torch.empty((B, H, W, 4), dtype=torch.uint8, device=dev) if occ is not None else None,
               "mask": torch.empty((B, H, W), dtype=torch.uint8, device=dev)}
    for k, shape in (("rgb", (B, H, W, 4)), ("normal", (B, H, W, 4)), ("occ", (B, H, W, 4)), ("mask", (B, H, W))):
        t = out.get(k)
        if t is None and (k != "occ" or occ is not None):
            raise ValueError(f"playback_finish: out['{k}'] is missing")
        if t is not None and (t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"playback_finish: out['{k}'] must be a contiguous uint8 {list(shape)} tensor on {dev}")
    a = hip_lib.SoarPlaybackArgs()
    a.B, a.H, a.W, a.normal_as_rgb = B, H, W, int(bool(normal_as_rgb))
    for name, t, c in ins:
        setattr(a, name, t.data_ptr() if B else None)
        setattr(a, name + "_stride", t.stride(0) if B > 1 else c * H * W)
    a.rgb, a.normal_out, a.mask_out = out["rgb"].data_ptr(), out["normal"].data_ptr(), out["mask"].data_ptr()
    a.occ_out = out["occ"].data_ptr() if occ is not None else None
    if B:
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_playback_finish(C.byref(a), _stream(dev)), "soar_playback_finish")
    return {"rgb": out["rgb"], "normal": out["normal"], "occ": out["occ"] if occ is not None else None, "mask": out["mask"]}


# ---- the player -------------------------------------------------------------------------------------------------------------------
def _split_pose(pose: torch.Tensor) -> Dict[str, torch.Tensor]:
    parts = torch.split(pose, POSE_WIDTHS, dim=1)
    return dict(zip(POSE_KEYS, parts))


def _batch(xs: Sequence[torch.Tensor]) -> torch.Tensor:
    """the frames' images as [B, ...] -- their own memory when they lie a fixed stride apart in one allocation"""
    from .renderer.fused_view import stack_views
    return xs[0][None] if len(xs) == 1 else stack_views(list(xs))


class AvatarPlayer:
    """Plays a trained avatar: ``turntable`` / ``resample`` make the motion, ``render`` the byte images, ``play`` the files.

    ``geometry``: a ``GaussianSurfelModel`` or anything with the duck type of render_rot.py:16-51 (``CheckpointSurfels``);
    ``guidance``: the ``SMPLGuidance`` whose stored frames the turntable starts from; ``renderer``: a ``"gaussiansurfel-rasterizer"``
    plugin instance over ``geometry`` (made with its defaults when None).  ``pose_mean [165]`` (the guidance's own when None): the
    body model's mean pose; pose dicts hold offsets from it, as ``params.pth`` does, and the motion is made on offset + mean."""

    def __init__(self, geometry, guidance, renderer=None, use_explicit: bool = False, pose_mean=None):
        self.geometry, self.guidance = geometry, guidance
        pose_mean = getattr(guidance, "pose_mean", None) if pose_mean is None else pose_mean
        self.pose_mean = None if pose_mean is None else torch.as_tensor(pose_mean, dtype=torch.float32).reshape(1, 165).to(guidance.device)
        if getattr(geometry, "smpl_guidance", None) is None:
            geometry.smpl_guidance = guidance
        if renderer is None:
            from . import renderer as _plugins  # noqa: F401  (registers the plugin)
            from .renderer import registry
            renderer = registry.find("gaussiansurfel-rasterizer")({"use_explicit": bool(use_explicit)}, geometry=geometry)
        self.renderer = renderer

    @classmethod
    def from_checkpoint(cls, ckpt: Union[str, os.PathLike, Mapping[str, Any]], guidance, use_explicit: bool = False) -> "AvatarPlayer":
        """``ckpt``: the path of the reference's Lightning checkpoint (loaded with ``torch.load(map_location="cpu",
        weights_only=False)``, as the reference loads it -- only open files you trust) or the loaded dict.  The leaves and the
        attribute field go to ``guidance.device``."""
        from .field import HashMLPField
        if not isinstance(ckpt, Mapping):
            ckpt = torch.load(os.fspath(ckpt), map_location="cpu", weights_only=False)
        m = map_checkpoint(ckpt)
        dev = torch.device(guidance.device)
        field = HashMLPField(m["aabb"].detach().float().cpu(), log2_hashmap_size=m["log2_hashmap_size"],
                             max_res=int(m["field"]["max_res"]), num_levels=int(m["field"]["num_levels"]))
        field.load_state_dict({k: v.detach().cpu() for k, v in m["field"].items()})
        field = field.to(dev)
        pc = CheckpointSurfels(*[m[k].to(dev) for k in ("xyz", "rotation", "occ", "colors", "scaling")], field, guidance)
        return cls(pc, guidance, use_explicit=use_explicit)

    # ---- motion -------------------------------------------------------------------------------------------------------------------
    def _keys_of(self, parms: Mapping[str, torch.Tensor]):
        """key poses with the reference's names -> (full_pose [K,165], transl [K,3], expression [K,E], betas [1,10])"""
        dev = self.guidance.device
        K = int(parms["body_pose"].shape[0])
        z = lambda n: torch.zeros((K, n), device=dev)
        get = lambda k, n: parms[k].to(dev).reshape(K, n) if parms.get(k) is not None else z(n)
        pose = torch.cat([get(k, n) for k, n in zip(POSE_KEYS, POSE_WIDTHS)], dim=1)
        if self.pose_mean is not None:
            pose = pose + self.pose_mean
        expr = parms.get("expression")
        expr = z(10) if expr is None else expr.to(dev).reshape(-1, expr.shape[-1]).expand(K, -1)
        return pose, get("transl", 3), expr, parms["betas"].to(dev)[:1]

    def _pose_dict(self, pose, transl, expr, betas) -> Dict[str, torch.Tensor]:
        if self.pose_mean is not None:
            pose = pose - self.pose_mean                                      # back to offsets: ``_keys_of`` adds the mean again
        d = _split_pose(pose)
        d.update(betas=betas, transl=transl, expression=expr)
        return d

    def turntable(self, n: int = 36, frame: int = 0) -> Dict[str, torch.Tensor]:
        """n steps of a full turn of the stored frame ``frame``: ``global_orient`` of step i is the axis-angle of ``R0 Ry(2 pi i / n)``
        (render_rot.py:152-156), everything else the frame's own.  -> a pose dict with the reference's key names, n rows each (``betas``
        [1,10]).  One launch."""
        if n < 1:
            raise ValueError(f"turntable: n must be at least 1 (got {n})")
        g = self.guidance
        k = int(frame) % len(g.smpl_parms["body_pose"])
        one = {key: (v[k:k + 1] if v.shape[0] > 1 else v[:1]) for key, v in g.smpl_parms.items() if key != "betas" and v is not None}
        one["betas"] = g.smpl_parms["betas"]
        pose, transl, expr, betas = self._keys_of(one)
        dev = pose.device
        yaw = torch.tensor([2.0 * math.pi * i / n for i in range(n)], dtype=torch.float32).to(dev)
        return self._pose_dict(*motion_resample(pose, transl, expr, torch.zeros(n, device=dev), yaw), betas)

    def resample(self, key_poses: Mapping[str, torch.Tensor], times) -> Dict[str, torch.Tensor]:
        """``key_poses``: a pose dict of K keys (the reference's names; a missing pose part is zero); ``times`` [F] in key units, e.g.
        ``arange(F) * (key_fps / fps)``, clamped to [0, K - 1].  -> the pose dict of the F frames.  One launch."""
        pose, transl, expr, betas = self._keys_of(key_poses)
        t = torch.as_tensor(times, dtype=torch.float32).to(pose.device)
        return self._pose_dict(*motion_resample(pose, transl, expr, t), betas)

    # ---- rendering ----------------------------------------------------------------------------------------------------------------
    def frame_pose(self, poses: Mapping[str, torch.Tensor], i: int) -> Dict[str, torch.Tensor]:
        """row i of a pose dict: what one ``forward(..., gt_a_smpl=...)`` call of the plugin takes"""
        return {k: (v if k == "betas" else v[i:i + 1]) for k, v in poses.items()}

    def joint_mats(self, poses: Mapping[str, torch.Tensor]) -> torch.Tensor:
        """cano2live joint transforms [F,55,4,4] of all frames in one launch (what ``SMPLGuidance.joint_mats`` gives per frame)"""
        g = self.guidance
        pose, transl, expr, betas = self._keys_of(poses)
        F = pose.shape[0]
        return g._jt.hip(torch.cat([betas.expand(F, -1), expr], dim=1), pose, transl, right=g.inv_mats[0])

    @torch.no_grad()
    def render(self, poses: Mapping[str, torch.Tensor], camera, bg: Optional[torch.Tensor] = None, chunk: int = 8,
               normal_as_rgb: bool = False) -> Dict[str, torch.Tensor]:
        """``poses``: a pose dict of F frames (``turntable`` / ``resample``); ``camera``: a ``renderer.cameras.Camera``; ``bg`` [3] on
        the device (white when None) -> ``rgb``, ``normal``, ``occ``: uint8 [F,H,W,4] and ``mask``: uint8 [F,H,W] on the device
        (``playback_finish`` states the conversion).  The frames are rendered ``chunk`` (1..8) at a time; the last chunk may be
        shorter."""
        from .rasterizer import GaussianRasterizationSettings
        from .renderer.fused_view import render_step_views
        if not 1 <= int(chunk) <= 8:
            raise ValueError(f"render: chunk must be in 1..8, the batched path's limit (got {chunk})")
        pc, rnd = self.geometry, self.renderer
        points, rot = pc.get_xyz, pc.get_rotation
        _need_hip(points, "the geometry")
        dev = points.device
        bg = torch.ones(3, dtype=torch.float32, device=dev) if bg is None else bg
        # once per playback: the field and the blend weights read canonical positions only; the joint chain of all frames is one launch
        fields = pc.attribute_field(points.detach(), z=None)
        explicit = bool(rnd.cfg.use_explicit)
        colors, scale = (pc.get_colors, pc.get_scaling) if explicit else (fields["shs"], fields["scales"])
        offsets = fields["offsets"] if rnd.cfg.offset else None
        w = pc.smpl_guidance.blend_weights(points)
        mats = self.joint_mats(poses)
        F = mats.shape[0]
        H, W = int(camera.image_height), int(camera.image_width)
        rs = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(camera.FoVx * 0.5), tanfovy=math.tan(camera.FoVy * 0.5), bg=bg,
            scale_modifier=1.0, viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform,
            patch_bbox=camera.random_patch(float("inf"), float("inf")), prcppoint=camera.prcppoint, sh_degree=pc.active_sh_degree,
            campos=camera.camera_center, prefiltered=False, render_front=False, sort_descending=False, debug=False, config=pc.config)
        carrier = torch.zeros((points.shape[0], 3), dtype=torch.float32, device=dev)       # (no gradient is ever asked of it)
        out = {"rgb": torch.empty((F, H, W, 4), dtype=torch.uint8, device=dev), "normal": torch.empty((F, H, W, 4), dtype=torch.uint8, device=dev),
               "occ": torch.empty((F, H, W, 4), dtype=torch.uint8, device=dev), "mask": torch.empty((F, H, W), dtype=torch.uint8, device=dev)}
        for f0 in range(0, F, int(chunk)):
            f1 = min(f0 + int(chunk), F)
            views = [{"weights": w, "joint_mats": mats[i], "offsets": offsets, "axis_perm": None, "settings": [rs], "cameras": [camera],
                      "backs": [False], "means2D": [carrier]} for i in range(f0, f1)]
            outs = render_step_views(points, rot, colors, scale, pc.get_occ, views, capacity=rnd._binning_capacity())
            img = lambda k: _batch([o[0][k] for o in outs])                                # o[0]: the pose's one view
            playback_finish(img(0), img(1), img(4), img(5), normal_as_rgb=normal_as_rgb, out={k: v[f0:f1] for k, v in out.items()})
        return out

    def play(self, poses: Mapping[str, torch.Tensor], camera, out_dir: str, bg: Optional[torch.Tensor] = None, chunk: int = 8,
             normal_as_rgb: bool = False, video=None, device_png: bool = False) -> Dict[str, torch.Tensor]:
        """``render``, then ``out_dir/{rgb,normal,occ,mask}/{i:05d}.png``: RGBA PNGs (the image with the mask as alpha, as the reference's
        ``save_image(torch.cat([image, mask]))`` writes them) and the greyscale mask.  -> what ``render`` returned.  Where the reference
        writes ``video.mp4`` with imageio, ``video=True`` or ``video=dict(fps=25, quality=90, subsampling="420")`` (``video.MjpegWriter``'s
        keywords) also writes ``out_dir/{rgb,normal,occ}/video.avi``: Motion-JPEG, encoded on the device ``chunk`` frames at a time from
        the byte images, the alpha channel dropped (``rgb`` is composited over ``bg`` already).  Without ``video`` nothing changes.
        ``device_png=True`` makes the PNG files on the device too (``png.write_png_files``, ``chunk`` images per call): the same names,
        pixels and modes, other bytes, and only compressed bytes are copied to the host."""
        from PIL import Image
        res = self.render(poses, camera, bg=bg, chunk=chunk, normal_as_rgb=normal_as_rgb)
        if video is not None and video is not False:
            from .video import video_options, write_video
            for k in ("rgb", "normal", "occ"):
                os.makedirs(os.path.join(out_dir, k), exist_ok=True)
                write_video(os.path.join(out_dir, k, "video.avi"), res[k], chunk=chunk, **video_options(video))
        for k, t in res.items():
            folder = os.path.join(out_dir, k)
            os.makedirs(folder, exist_ok=True)
            if device_png:
                from .png import write_png_files
                write_png_files([os.path.join(folder, f"{i:05d}.png") for i in range(t.shape[0])], t, chunk=chunk)
                continue
            for i, img in enumerate(t.cpu().numpy()):                   # [H,W,4] bytes -> "RGBA", [H,W] -> "L"
                Image.fromarray(img).save(os.path.join(folder, f"{i:05d}.png"))
        return res
