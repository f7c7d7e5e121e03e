"""SMPLify fit inspection: per frame a strip of five panels -- target keypoints (green) and fitted keypoints (red), the body's normal
render over the photograph, and the body from the camera, turned by 120 and by 240 degrees about the camera's up axis -- what the
reference's ``SMPLify.visualize_params`` (preproc/utils.py:687-791) shows its user, with the image stage in HIP (csrc/fitviz.hip) so
that only finished uint8 strips leave the device.

* ``yaw_matrices(w2c, n_views)`` / ``yaw_views(verts, pivot, w2c, n_views)``: the turned copies of the body; view 0 is ``verts``.
* ``draw_strips(target_px, fit_px, kp_mask, prior, mask, imgs=...)``: drawing, compositing and packing -> ``[N,H,5W,3]`` uint8.
* ``fit_residuals(fit_px, target_px, conf, kp_mask)``: per frame the count, mean and maximum pixel distance of the confident keypoints.
* ``fit_strips(rig, body, topo, params, Ks, w2c, img_wh, target_kps, imgs=...)``: the whole stage, in chunks of frames.
* ``save_strips`` / ``FitVisualizer``: a folder of PNGs per call, and the object ``SMPLify.fit(..., visual=...)`` takes.

Every keypoint is a filled disc, as in the reference (its ``draw_pose`` draws a skeleton only for 135 keypoints and is fed 137); a
skeleton is opt-in: pass ``limbs=OPENPOSE_BODY25_LIMBS[0], limb_rgb=OPENPOSE_BODY25_LIMBS[1]``.  The coverage rules are this
project's own definitions: they are not measured against OpenCV's rasterizer, and the normal renders are those of
``prior.render_normal_priors`` (9n), not of the reference's ``render_mesh``.  Where the reference writes an ``.mp4`` per call, a
folder of PNGs is written and, with ``video=``, a Motion-JPEG ``video.avi`` encoded on the device (soar_amd/video.py).  HIP only: CPU
tensors are refused, there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from . import hip_lib
from .hip_lib import _stream, check, ptr
from .prior import MeshTopology, full_pose, render_normal_priors

MAX_KEYPOINTS = MAX_LIMBS = 512          # soar_fitviz_strip
HALF_ABOVE = 2048                        # the reference halves its strips when max(img_wh) is larger

# OpenPose's BODY_25 pairs and colours (the limb's colour is its second keypoint's), for ``draw_strips(limbs=..., limb_rgb=...)``
_BODY25_PAIRS = ((1, 8), (1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (8, 9), (9, 10), (10, 11), (8, 12), (12, 13), (13, 14),
                 (1, 0), (0, 15), (15, 17), (0, 16), (16, 18), (14, 19), (19, 20), (14, 21), (11, 22), (22, 23), (11, 24))
_BODY25_RGB = ((255, 0, 85), (255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 255, 0), (170, 255, 0), (85, 255, 0), (0, 255, 0),
               (255, 0, 0), (0, 255, 85), (0, 255, 170), (0, 255, 255), (0, 170, 255), (0, 85, 255), (0, 0, 255), (255, 0, 170),
               (170, 0, 255), (255, 0, 255), (85, 0, 255), (0, 0, 255), (0, 0, 255), (0, 0, 255), (0, 255, 255), (0, 255, 255),
               (0, 255, 255))
OPENPOSE_BODY25_LIMBS = (np.array(_BODY25_PAIRS, np.int32), np.array([_BODY25_RGB[b] for _, b in _BODY25_PAIRS], np.uint8))


def _hip(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name} is on '{where}': soar_amd.fitviz runs on HIP devices only; there is no CPU fallback")


def yaw_matrices(w2c, n_views: int = 3) -> np.ndarray:
    """``[n_views,3,3]`` float32: Rodrigues matrices of ``-w2c[:3,1]`` (normalised) times ``2 pi k / n_views`` -- the reference's
    ``rotvec_to_rotmat(-w2c[:3,1] * linspace(0, 2 pi, n_views + 1)[:n_views])``, worked out in float64 and rounded once."""
    w = np.asarray(w2c.detach().cpu() if isinstance(w2c, torch.Tensor) else w2c, dtype=np.float64)
    if w.shape != (4, 4):
        raise ValueError(f"yaw_matrices: w2c must be [4,4] (got {w.shape})")
    if not 1 <= int(n_views) <= 16:
        raise ValueError(f"yaw_matrices: n_views must be 1 .. 16 (got {n_views})")
    axis = -w[:3, 1]
    norm = float(np.linalg.norm(axis))
    if not norm > 0.0 or not math.isfinite(norm):
        raise ValueError("yaw_matrices: w2c[:3,1] is zero or not finite")
    x, y, z = axis / norm
    K = np.array([[0.0, -z, y], [z, 0.0, -x], [-y, x, 0.0]])
    out = np.empty((int(n_views), 3, 3), np.float64)
    for k in range(int(n_views)):
        t = 2.0 * math.pi * k / int(n_views)
        out[k] = np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)
    return out.astype(np.float32)


@torch.no_grad()
def yaw_views(verts: torch.Tensor, pivot: torch.Tensor, w2c, n_views: int = 3) -> torch.Tensor:
    """``verts [N,V,3]`` float32 (any strides), ``pivot [N,3]`` -> ``[N,n_views,V,3]``: view 0 is ``verts`` bit for bit, view k is
    ``R_k (v - pivot) + pivot`` with ``R = yaw_matrices(w2c, n_views)``."""
    _hip(verts, "verts")
    _hip(pivot, "pivot")
    if verts.dim() != 3 or verts.shape[2] != 3 or verts.dtype != torch.float32 or verts.shape[1] < 1:
        raise ValueError(f"yaw_views: verts must be float32 [N,V,3] (got {verts.dtype} {tuple(verts.shape)})")
    N, V = verts.shape[:2]
    if tuple(pivot.shape) != (N, 3):
        raise ValueError(f"yaw_views: pivot must be [{N},3] (got {tuple(pivot.shape)})")
    dev = verts.device
    R = torch.from_numpy(yaw_matrices(w2c, n_views)[1:].copy()).to(dev)
    pivot = pivot.detach().to(dev, torch.float32).contiguous()
    out = torch.empty((N, int(n_views), V, 3), dtype=torch.float32, device=dev)
    if N:
        verts = verts.detach()
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_fitviz_yaw_views(N, V, int(n_views), verts.data_ptr(), (C.c_int64 * 3)(*verts.stride()),
                                                      pivot.data_ptr(), ptr(R), out.data_ptr(), _stream(dev)), "soar_fitviz_yaw_views")
    return out


def _rgb(v, name):
    t = tuple(int(x) for x in v)
    if len(t) != 3 or not all(0 <= x <= 255 for x in t):
        raise ValueError(f"draw_strips: {name} must be three values in 0 .. 255 (got {v})")
    return (C.c_uint8 * 4)(*t, 0)


@torch.no_grad()
def draw_strips(target_px: torch.Tensor, fit_px: torch.Tensor, kp_mask, prior: torch.Tensor, mask: torch.Tensor, imgs=None,
                limbs=None, limb_rgb=None, radius: int = 3, thickness: int = 4, half: Optional[bool] = None,
                target_rgb=(0, 255, 0), fit_rgb=(255, 0, 0)) -> torch.Tensor:
    """``target_px``, ``fit_px`` ``[N,K,2]`` float32 pixels; ``kp_mask [K]``; ``prior`` / ``mask`` as ``render_normal_priors`` leaves
    them for the ``3 N`` bodies of ``yaw_views`` (``[3N,2,3,H,W]`` / ``[3N,2,H,W]``, or with the leading axes split); ``imgs
    [N,H,W,3]`` uint8 (any strides) or None; ``limbs [L,2]`` keypoint pairs with ``limb_rgb [L,3]``, or None for discs alone.
    Returns ``[N,H,5W,3]`` uint8, or ``[N,H//2,(5W)//2,3]`` with ``half`` (default: ``max(W, H) > 2048``, the reference's rule).
    The rules are those of include/soar_hip.h."""
    _hip(target_px, "target_px")
    _hip(fit_px, "fit_px")
    _hip(prior, "prior")
    _hip(mask, "mask")
    dev = prior.device
    if target_px.dim() != 3 or target_px.shape[2] != 2 or fit_px.shape != target_px.shape:
        raise ValueError(f"draw_strips: target_px and fit_px must both be [N,K,2] (got {tuple(target_px.shape)}, {tuple(fit_px.shape)})")
    N, K = target_px.shape[:2]
    if K > MAX_KEYPOINTS:
        raise ValueError(f"draw_strips: at most {MAX_KEYPOINTS} keypoints are supported (got {K})")
    if not 1 <= int(radius) <= 8 or not 1 <= int(thickness) <= 64:
        raise ValueError(f"draw_strips: radius must be 1 .. 8 and thickness 1 .. 64 (got {radius}, {thickness})")
    if prior.dim() < 4 or prior.dtype != torch.float32 or mask.dtype != torch.uint8:
        raise ValueError(f"draw_strips: prior must be float32 and mask uint8 (got {prior.dtype} {tuple(prior.shape)}, {mask.dtype})")
    H, W = prior.shape[-2:]
    if prior.numel() != N * 18 * H * W or mask.numel() != N * 6 * H * W or tuple(mask.shape[-2:]) != (H, W):
        raise ValueError(f"draw_strips: prior must hold [{N},3,2,3,H,W] and mask [{N},3,2,H,W] (got {tuple(prior.shape)}, {tuple(mask.shape)})")
    f = lambda x: x.detach().to(dev, torch.float32).contiguous()
    target_px, fit_px, prior, mask = f(target_px), f(fit_px), prior.detach().contiguous(), mask.detach().contiguous()
    km = torch.as_tensor(kp_mask).detach().to(dev)
    if km.shape != (K,):
        raise ValueError(f"draw_strips: kp_mask must be [{K}] (got {tuple(km.shape)})")
    km = (km != 0).to(torch.uint8).contiguous()
    L, lt, lc = 0, None, None
    if (limbs is None) != (limb_rgb is None):
        raise ValueError("draw_strips: limbs and limb_rgb come together")
    if limbs is not None:
        ln = np.asarray(limbs.detach().cpu() if isinstance(limbs, torch.Tensor) else limbs)
        cn = np.asarray(limb_rgb.detach().cpu() if isinstance(limb_rgb, torch.Tensor) else limb_rgb)
        if ln.ndim != 2 or ln.shape[1] != 2 or ln.dtype.kind not in "iu" or cn.shape != (ln.shape[0], 3):
            raise ValueError(f"draw_strips: limbs must be integer [L,2] and limb_rgb [L,3] (got {ln.shape} {ln.dtype}, {cn.shape})")
        L = ln.shape[0]
        if L > MAX_LIMBS:
            raise ValueError(f"draw_strips: at most {MAX_LIMBS} limbs are supported (got {L})")
        if L and (int(ln.min()) < 0 or int(ln.max()) >= K):
            raise ValueError(f"draw_strips: a limb names a keypoint outside [0, {K})")
        if L and (cn.min() < 0 or cn.max() > 255):
            raise ValueError("draw_strips: limb_rgb must be 0 .. 255")
        lt = torch.from_numpy(np.ascontiguousarray(ln, np.int32)).to(dev)
        lc = torch.from_numpy(np.ascontiguousarray(cn).astype(np.uint8)).to(dev)
    if imgs is not None:
        _hip(imgs, "imgs")
        if tuple(imgs.shape) != (N, H, W, 3) or imgs.dtype != torch.uint8:
            raise ValueError(f"draw_strips: imgs must be uint8 [{N},{H},{W},3] (got {imgs.dtype} {tuple(imgs.shape)})")
        imgs = imgs.detach()
    half = max(W, H) > HALF_ABOVE if half is None else bool(half)
    if half and H < 2:
        raise ValueError("draw_strips: a halved strip needs H >= 2")
    out = torch.empty((N, H // 2, 5 * W // 2, 3) if half else (N, H, 5 * W, 3), dtype=torch.uint8, device=dev)
    if N:
        a = hip_lib.SoarFitvizStripArgs()
        a.N, a.H, a.W, a.K, a.L, a.radius, a.thickness, a.half = N, H, W, K, L, int(radius), int(thickness), int(half)
        a.target_px, a.fit_px, a.kp_mask, a.limbs, a.limb_rgb = ptr(target_px), ptr(fit_px), ptr(km), ptr(lt), ptr(lc)
        if imgs is not None:
            a.imgs = imgs.data_ptr()
            a.imgs_stride = (C.c_int64 * 4)(*imgs.stride())
        a.prior, a.mask, a.out = prior.data_ptr(), mask.data_ptr(), out.data_ptr()
        a.target_rgb, a.fit_rgb = _rgb(target_rgb, "target_rgb"), _rgb(fit_rgb, "fit_rgb")
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_fitviz_strip(C.byref(a), _stream(dev)), "soar_fitviz_strip")
    return out


@torch.no_grad()
def fit_residuals(fit_px: torch.Tensor, target_px: torch.Tensor, conf: torch.Tensor, kp_mask, thresh: float = 0.3) -> torch.Tensor:
    """``[N,3]`` float32: per frame the number of keypoints with ``kp_mask``, confidence above ``thresh`` (the selection
    ``target_scales`` uses) and finite coordinates, then the mean and the maximum pixel distance between fit and target over
    them; zeros for a frame with none."""
    _hip(fit_px, "fit_px")
    _hip(target_px, "target_px")
    _hip(conf, "conf")
    if fit_px.dim() != 3 or fit_px.shape[2] != 2 or target_px.shape != fit_px.shape or tuple(conf.shape) != tuple(fit_px.shape[:2]):
        raise ValueError(f"fit_residuals: fit_px and target_px must be [N,K,2] and conf [N,K] (got {tuple(fit_px.shape)}, "
                         f"{tuple(target_px.shape)}, {tuple(conf.shape)})")
    N, K = fit_px.shape[:2]
    if K > MAX_KEYPOINTS:
        raise ValueError(f"fit_residuals: at most {MAX_KEYPOINTS} keypoints are supported (got {K})")
    dev = fit_px.device
    f = lambda x: x.detach().to(dev, torch.float32).contiguous()
    fit_px, target_px, conf = f(fit_px), f(target_px), f(conf)
    km = torch.as_tensor(kp_mask).detach().to(dev)
    if km.shape != (K,):
        raise ValueError(f"fit_residuals: kp_mask must be [{K}] (got {tuple(km.shape)})")
    km = (km != 0).to(torch.uint8).contiguous()
    out = torch.empty((N, 3), dtype=torch.float32, device=dev)
    if N:
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_fitviz_residuals(N, K, ptr(fit_px), ptr(target_px), ptr(conf), ptr(km), float(thresh),
                                                      out.data_ptr(), _stream(dev)), "soar_fitviz_residuals")
    return out


def _six_d(params: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The parameter dict ``project_keypoints`` takes (6-D rotations, one row of betas) from rotation vectors as ``SMPLify.fit``
    returns them."""
    from .smplify import POSE_KEYS, rotation_6d_from_rotvec
    out = {}
    for k, v in params.items():
        if k in POSE_KEYS:
            v = rotation_6d_from_rotvec(v.reshape(v.shape[0], -1, 3))
        out[k] = v
    out["betas"] = out["betas"].reshape(-1, out["betas"].shape[-1])[:1]
    return out


@torch.no_grad()
def fit_strips(rig, body, topo: MeshTopology, params: Mapping[str, torch.Tensor], Ks, w2c, img_wh, target_kps, imgs=None,
               pose_mean=None, chunk: int = 4, **draw) -> Dict[str, torch.Tensor]:
    """The whole stage for N fitted frames.  ``rig``: the ``KeypointRig`` of the fit; ``body`` / ``topo``: what ``smplx_vertices`` and
    ``render_normal_priors`` take; ``params``: rotation vectors as ``SMPLify.fit`` returns them; ``Ks [N,3,3]``, ``w2c [4,4]``,
    ``img_wh = (W, H)``; ``target_kps [N,137,3]`` normalised as ``SMPLify.fit`` takes it (it is multiplied by ``img_wh`` once, here);
    ``imgs [N,H,W,3]`` uint8 or None; ``pose_mean`` as ``prior.full_pose`` takes it; ``draw``: ``draw_strips``' keywords.  Per chunk
    of ``chunk`` frames: the projected keypoints, the body's vertices, the pelvis (rest joint 0 of the shaped body plus ``transl``,
    which the pose does not move) as the pivot, the yaw views, one renderer call on the ``3 chunk`` bodies (the float normal images
    are about 100 bytes a pixel and body: hence the chunks), the strips.  Returns dict(``strips`` uint8, ``residuals [N,3]``)."""
    from .body import smplx_vertices
    from .smplify import project_keypoints
    if chunk < 1:
        raise ValueError(f"fit_strips: chunk must be >= 1 (got {chunk})")
    dev = rig.device
    f = lambda x: torch.as_tensor(x).detach().to(dev, torch.float32)
    params = {k: f(v) for k, v in params.items()}
    _hip(params["transl"], "params")
    N = params["transl"].shape[0]
    W, H = (int(x) for x in img_wh)
    target = f(target_kps)
    if target.dim() != 3 or target.shape[0] != N or target.shape[2] != 3:
        raise ValueError(f"fit_strips: target_kps must be [{N},K,3] (got {tuple(target.shape)})")
    Ks, w2c = f(Ks), f(w2c)
    if Ks.shape != (N, 3, 3) or w2c.shape != (4, 4):
        raise ValueError(f"fit_strips: Ks must be [{N},3,3] and w2c [4,4] (got {tuple(Ks.shape)}, {tuple(w2c.shape)})")
    target_px = (target[..., :2] * torch.tensor([float(W), float(H)], device=dev)).contiguous()
    conf = target[..., 2].contiguous()
    six = _six_d(params)
    betas = params["betas"].reshape(-1, params["betas"].shape[-1])[:1]
    coef = torch.cat([betas.expand(N, -1), params["expression"].reshape(N, -1)], dim=1)
    pose = full_pose(params, pose_mean)
    pelvis = rig.J_template[0] + torch.einsum("kl,nl->nk", rig.J_dirs[0], coef) + params["transl"]
    strips, residuals = [], torch.empty((N, 3), dtype=torch.float32, device=dev)
    for i in range(0, N, chunk):
        j = min(i + chunk, N)
        sl = {k: (v if k == "betas" else v[i:j]) for k, v in six.items()}
        fit_px = project_keypoints(rig, sl, Ks[i:j], w2c)
        verts = smplx_vertices(body, coef[i:j], pose[i:j], params["transl"][i:j])
        views = yaw_views(verts, pelvis[i:j], w2c, 3)
        pr = render_normal_priors(topo, views.reshape(3 * (j - i), -1, 3), w2c, Ks[i:j].repeat_interleave(3, dim=0), (W, H))
        strips.append(draw_strips(target_px[i:j], fit_px, rig.kp_mask, pr["prior"], pr["mask"], None if imgs is None else imgs[i:j], **draw))
        residuals[i:j] = fit_residuals(fit_px, target_px[i:j], conf[i:j], rig.kp_mask)
    if not strips:
        strips = [draw_strips(target_px, target_px, rig.kp_mask, torch.empty((0, 2, 3, H, W), device=dev),
                              torch.empty((0, 2, H, W), dtype=torch.uint8, device=dev), **draw)]
    return dict(strips=torch.cat(strips, dim=0), residuals=residuals)


def save_strips(strips: torch.Tensor, folder: str, video=None, device_png: bool = False) -> None:
    """``<folder>/<frame:05d>.png`` for every strip of ``[N,h,w,3]`` uint8.  Where the reference writes one ``.mp4``, ``video=True`` or
    ``video=dict(fps=..., quality=..., subsampling=...)`` (``video.MjpegWriter``'s keywords) also writes ``<folder>/video.avi``:
    Motion-JPEG, encoded on the device from the strips (which must then be on a HIP device).  ``device_png=True`` makes the PNG files
    on the device as well (``png.write_png_files``): the same names and pixels, and only compressed bytes are copied to the host."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    if video is not None and video is not False:
        from .video import video_options, write_video
        write_video(os.path.join(folder, "video.avi"), strips.detach(), **video_options(video))
    if device_png:
        from .png import write_png_files
        write_png_files([os.path.join(folder, f"{n:05d}.png") for n in range(strips.shape[0])], strips.detach())
        return
    host = strips.detach().cpu().numpy()
    for n in range(host.shape[0]):
        Image.fromarray(host[n]).save(os.path.join(folder, f"{n:05d}.png"))


class FitVisualizer:
    """What ``SMPLify.fit(..., visual=...)`` calls at the reference's moments: ``visual(name, params, Ks, w2c, img_wh, target_kps)``
    runs ``fit_strips``, writes the strips under ``out_dir/name`` and keeps ``residuals[name]`` (a host ``[N,3]`` array).
    ``debug=True`` asks ``fit`` for every fifth step instead of the stages' last; ``video``: what ``save_strips`` takes."""

    def __init__(self, rig, body, topo: MeshTopology, out_dir: str, imgs=None, debug: bool = False, pose_mean=None, video=None, **draw):
        self.rig, self.body, self.topo, self.out_dir, self.imgs, self.debug = rig, body, topo, out_dir, imgs, bool(debug)
        self.pose_mean, self.video, self.draw = pose_mean, video, draw
        self.residuals: Dict[str, np.ndarray] = {}

    def __call__(self, name: str, params, Ks, w2c, img_wh, target_kps) -> None:
        out = fit_strips(self.rig, self.body, self.topo, params, Ks, w2c, img_wh, target_kps, imgs=self.imgs,
                         pose_mean=self.pose_mean, **self.draw)
        save_strips(out["strips"], os.path.join(self.out_dir, name), video=self.video)
        self.residuals[name] = out["residuals"].cpu().numpy()
