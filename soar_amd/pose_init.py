"""SMPL-X initialisation from keypoints alone: a pose search and a shortest path in HIP (csrc/pose_init.hip).

``SMPLify.fit`` needs a per-frame SMPL-X estimate and intrinsics to start from.  The reference gets both by shelling out to
SMPLer-X (``preproc/compute_smplx.py:36-53``), a ViT-H regressor with licensed weights that this project cannot rebuild.

**This module stands in for that step and is a different algorithm**: the classical SMPLify start.  **The bank of hypotheses, the
intrinsics rule and the defaults (``conf_min``, ``z_min``, ``min_points``, ``rot_weight``, ``switch_cost``, ``prior_weight``) are this
project's definitions.  The defaults are not tuned on real video.  Nothing was compared with SMPLer-X or with the licensed SMPL-X
model, because neither was available.  A pose far from every bank entry, such as sitting or lying, starts badly; the remedy is the
caller's ``base_poses``.**

* ``search``: N frames x S = B x H hypotheses (B base poses, H root rotations about the pelvis) in one launch: per (frame, state)
  the closed-form camera translation (a 3 x 3 system from seven weighted sums, in float64) and the fit's own keypoint term as the
  cost, so that what the search minimises is what the fit minimises next.
* ``viterbi`` / ``viterbi_path``: the shortest path through the frames in one launch, so that a sequence does not flip between
  look-alike hypotheses; frames without evidence are bridged and their translation interpolated.
* ``transition_cost``, ``rotation_bank``, ``base_poses``, ``default_intrinsics``: the bank and the rules (torch, plumbing).
* ``init_from_keypoints``: ``search`` then ``viterbi_path`` -> a dict in ``load_smplerx``'s keys and shapes.
* ``fit_from_keypoints``: that, a short low-prior fit, and the reference's fit -- ``SMPLify`` as it is.

HIP only; there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, NamedTuple, Optional, Sequence

import torch

from . import hip_lib, smplify
from .hip_lib import _stream, check
from .smplify import N_KEYPOINTS, PARAM_KEYS, POSE_KEYS, KeypointRig, SMPLify, _hip

MAX_STATES = 1024                   # pose_init.hip
# this project's definitions, not tuned on real video (module docstring)
CONF_MIN, Z_MIN, MIN_POINTS = 0.1, 0.1, 6
ROT_WEIGHT, SWITCH_COST, PRIOR_WEIGHT = 100.0, 100.0, 1.0
L_SHOULDER, R_SHOULDER = 16, 17     # SMPL-X joints; body_pose holds joints 1 .. 21


class SearchResult(NamedTuple):
    cost: torch.Tensor      # [N,S] float32, +inf for an invalid state
    transl: torch.Tensor    # [N,S,3] float32, world translation of every state (0 for an invalid one)
    valid: torch.Tensor     # [N] bool: any state of the frame is finite


class ViterbiResult(NamedTuple):
    path: torch.Tensor          # [N] int64
    total: torch.Tensor         # 0-d float32
    transl_path: torch.Tensor   # [N,3] float32


class InitInfo(NamedTuple):
    path: torch.Tensor      # [N] int64: state b * H + h of every frame
    valid: torch.Tensor     # [N] bool
    cost: torch.Tensor      # [N] float32: the chosen state's cost (+inf where the frame is not valid)


class FitResult(NamedTuple):
    params: Dict[str, torch.Tensor]     # what ``save_params`` takes, with Ks, w2c, img_wh
    Ks: torch.Tensor
    w2c: torch.Tensor
    img_wh: tuple
    info: InitInfo


def _f32(t, name: str, dev) -> torch.Tensor:
    _hip(t, name)
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


@torch.no_grad()
def search(points0, pivot, rotations, rig: KeypointRig, target_kps, Ks, w2c, img_wh, scales, sigma: float = 100.0,
           conf_min: float = CONF_MIN, z_min: float = Z_MIN, min_points: int = MIN_POINTS) -> SearchResult:
    """Score every (frame, state) and solve its camera translation; one launch, nothing read back.

    ``points0 [B,P,3]``: ``smplify.model_points`` of B base poses with identity ``global_orient`` and zero ``transl``;
    ``pivot [B,3]``: joint 0 of each; ``rotations [H,3,3]``.  State ``s = b * H + h`` is base pose b turned by ``rotations[h]`` about its
    pivot.  ``target_kps [N,137,3]`` (x / w, y / h, confidence), ``Ks [N,3,3]`` upper triangular (skew honoured), ``w2c [4,4]``,
    ``scales [N]`` (``smplify.target_scales``).  The weights are ``confidence * kp_mask`` with the hands (rows ``25:-70``), confidences
    below ``conf_min`` and a rig's contour keypoints at zero; a frame needs ``min_points`` positive ones.  A state whose system
    has no positive determinant or whose smallest camera depth is below ``z_min`` is invalid: cost ``+inf``, transl 0.  Strided inputs
    are made contiguous.  A frame's outputs are the same bits alone, in any batch and in any order."""
    dev = rig.device
    points0, pivot, rotations = _f32(points0, "points0", dev), _f32(pivot, "pivot", dev), _f32(rotations, "rotations", dev)
    target, Ks, w2c, scales = _f32(target_kps, "target_kps", dev), _f32(Ks, "Ks", dev), _f32(w2c, "w2c", dev), _f32(scales, "scales", dev)
    if points0.dim() != 3 or points0.shape[2] != 3 or pivot.shape != (points0.shape[0], 3) or rotations.dim() != 3 or rotations.shape[1:] != (3, 3):
        raise ValueError(f"points0 must be [B,P,3], pivot [B,3] and rotations [H,3,3] (got {tuple(points0.shape)}, {tuple(pivot.shape)}, "
                         f"{tuple(rotations.shape)})")
    B, PA, H = points0.shape[0], points0.shape[1], rotations.shape[0]
    if PA != rig.PA:
        raise ValueError(f"points0 holds {PA} points per pose; the rig's model_points has {rig.PA}")
    S = B * H
    if not 1 <= S <= MAX_STATES:
        raise ValueError(f"{B} base poses x {H} rotations = {S} states; 1 .. {MAX_STATES} are supported")
    N = target.shape[0]
    if N <= 0:
        raise ValueError("no frames")
    if target.shape != (N, N_KEYPOINTS, 3) or Ks.shape != (N, 3, 3) or w2c.shape != (4, 4) or scales.shape != (N,):
        raise ValueError(f"target_kps must be [{N},{N_KEYPOINTS},3], Ks [{N},3,3], w2c [4,4] and scales [{N}] (got {tuple(target.shape)}, "
                         f"{tuple(Ks.shape)}, {tuple(w2c.shape)}, {tuple(scales.shape)})")
    if int(min_points) < 1:
        raise ValueError("min_points must be at least 1")
    src = rig.src_inds.to(torch.int32).to(dev)
    dst = rig.dst_inds.to(torch.int32).to(dev)
    cost = torch.empty(N, S, dtype=torch.float32, device=dev)
    transl = torch.empty(N, S, 3, dtype=torch.float32, device=dev)
    valid = torch.empty(N, dtype=torch.uint8, device=dev)
    a = hip_lib.SoarPoseSearch()
    a.N, a.B, a.H, a.PA, a.P, a.min_points = N, B, H, PA, src.numel(), int(min_points)
    a.points0, a.pivot, a.rotations = points0.data_ptr(), pivot.data_ptr(), rotations.data_ptr()
    a.src_inds, a.dst_inds = (src.data_ptr(), dst.data_ptr()) if src.numel() else (None, None)
    a.kp_mask, a.target_kps, a.Ks, a.w2c, a.scales = rig.kp_mask.data_ptr(), target.data_ptr(), Ks.data_ptr(), w2c.data_ptr(), scales.data_ptr()
    a.img_w, a.img_h, a.sigma, a.conf_min, a.z_min = float(img_wh[0]), float(img_wh[1]), float(sigma), float(conf_min), float(z_min)
    a.cost, a.transl, a.valid = cost.data_ptr(), transl.data_ptr(), valid.data_ptr()
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_pose_init_search(C.byref(a), _stream(dev)), "soar_pose_init_search")
    return SearchResult(cost, transl, valid.bool())


def _viterbi(unary, trans, transl, valid):
    _hip(unary, "unary")
    dev = unary.device
    U, T = _f32(unary, "unary", dev), _f32(trans, "trans", dev)
    if U.dim() != 2 or T.shape != (U.shape[1], U.shape[1]):
        raise ValueError(f"unary must be [N,S] and trans [S,S] (got {tuple(U.shape)} and {tuple(T.shape)})")
    N, S = U.shape
    if N <= 0:
        raise ValueError("no frames")
    if not 1 <= S <= MAX_STATES:
        raise ValueError(f"{S} states; 1 .. {MAX_STATES} are supported")
    backptr = torch.empty(N, S, dtype=torch.int32, device=dev)         # the kernel's scratch
    path = torch.empty(N, dtype=torch.int64, device=dev)
    total = torch.empty(1, dtype=torch.float32, device=dev)
    tp = tr = vd = None
    if transl is not None:
        tr = _f32(transl, "transl", dev)
        _hip(valid, "valid")
        vd = valid.detach().to(device=dev, dtype=torch.uint8).contiguous()
        if tr.shape != (N, S, 3) or vd.shape != (N,):
            raise ValueError(f"transl must be [{N},{S},3] and valid [{N}] (got {tuple(tr.shape)} and {tuple(vd.shape)})")
        tp = torch.empty(N, 3, dtype=torch.float32, device=dev)
    p = lambda t: t.data_ptr() if t is not None else None
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_pose_init_viterbi(N, S, U.data_ptr(), T.data_ptr(), backptr.data_ptr(), path.data_ptr(), total.data_ptr(),
                                                   p(tr), p(vd), p(tp), _stream(dev)), "soar_pose_init_viterbi")
    return path, total[0], tp


@torch.no_grad()
def viterbi(unary, trans):
    """``(path [N] int64, total)``: the shortest path through ``unary [N,S]`` with transition costs ``trans [S,S]`` (from row to
    column), one launch of one workgroup, S <= 1024.  ``D[0] = U[0]``, ``D[n,s] = (min_s' (D[n-1,s'] + T[s',s])) + U[n,s]`` in
    float32 in exactly that order; ties go to the lowest ``s'`` and the final minimum to the lowest ``s``.  A frame whose unary
    row is all ``+inf`` counts as a row of zeros: it carries no evidence, and the path bridges it."""
    path, total, _ = _viterbi(unary, trans, None, None)
    return path, total


@torch.no_grad()
def viterbi_path(unary, trans, transl, valid) -> ViterbiResult:
    """``viterbi`` and, in the same launch, the path's translations ``[N,3]`` out of ``transl [N,S,3]``: for frames where ``valid [N]``
    is false, interpolated linearly between the nearest valid frames on either side and held at the ends."""
    return ViterbiResult(*_viterbi(unary, trans, transl, valid))


def transition_cost(rotations: torch.Tensor, B: int, rot_weight: float = ROT_WEIGHT, switch_cost: float = SWITCH_COST) -> torch.Tensor:
    """``T [S,S]``, ``S = B * H``: ``rot_weight * angle(R_h'^T R_h)^2 + switch_cost * [b != b']`` for the step from state
    ``b' H + h'`` to ``b H + h`` (torch, on the rotations' device)."""
    R = rotations.to(torch.float32)
    H = R.shape[0]
    M = R.transpose(1, 2)[:, None] @ R[None]                           # [H',H,3,3]
    a = 0.5 * torch.stack((M[..., 2, 1] - M[..., 1, 2], M[..., 0, 2] - M[..., 2, 0], M[..., 1, 0] - M[..., 0, 1]), -1)
    c = 0.5 * (M[..., 0, 0] + M[..., 1, 1] + M[..., 2, 2] - 1.0)
    angle = torch.atan2(torch.linalg.norm(a, dim=-1), c)
    base = torch.arange(B, device=R.device)
    switch = (base[:, None] != base[None]).to(torch.float32) * float(switch_cost)          # [B',B]
    return (float(rot_weight) * (angle * angle)[None, :, None, :] + switch[:, None, :, None]).reshape(B * H, B * H).contiguous()


def default_intrinsics(N: int, img_wh, focal: Optional[float] = None, device="cpu") -> torch.Tensor:
    """``Ks [N,3,3]``: the focal length defaults to the image diagonal in pixels, the principal point is the centre.  **This project's
    definition: SMPLer-X's ``meta/`` files are not reproduced.**"""
    w, h = float(img_wh[0]), float(img_wh[1])
    f = float(focal) if focal is not None else math.hypot(w, h)
    K = torch.tensor([[f, 0.0, 0.5 * w], [0.0, f, 0.5 * h], [0.0, 0.0, 1.0]], dtype=torch.float32, device=device)
    return K[None].repeat(N, 1, 1)


def rotation_bank(yaws: int = 24, pitches: Sequence[float] = (0.0,), device="cpu") -> torch.Tensor:
    """``[len(pitches) * yaws, 3, 3]``: ``R_y(2 pi i / yaws) R_x(pitch)``, the pitch outermost in the order of the rows."""
    out = []
    for p in pitches:
        cp, sp = math.cos(p), math.sin(p)
        Rx = torch.tensor([[1.0, 0.0, 0.0], [0.0, cp, -sp], [0.0, sp, cp]], dtype=torch.float64)
        for i in range(int(yaws)):
            y = 2.0 * math.pi * i / int(yaws)
            Ry = torch.tensor([[math.cos(y), 0.0, math.sin(y)], [0.0, 1.0, 0.0], [-math.sin(y), 0.0, math.cos(y)]], dtype=torch.float64)
            out.append(Ry @ Rx)
    return torch.stack(out).to(device=device, dtype=torch.float32)


def base_poses(rig: Optional[KeypointRig] = None, arm_angles: Sequence[float] = (0.0, 1.1)) -> torch.Tensor:
    """``[B,63]`` body poses (rotation vectors): per angle the T-pose with the two shoulder joints turned about z, the left by
    ``-angle`` and the right by ``+angle`` (0: the T-pose, 1.1: an A-pose).  On the rig's device when one is given."""
    out = torch.zeros(len(arm_angles), 21, 3)
    for b, ang in enumerate(arm_angles):
        out[b, L_SHOULDER - 1, 2], out[b, R_SHOULDER - 1, 2] = -float(ang), float(ang)
    return out.reshape(len(arm_angles), 63).to(rig.device if rig is not None else "cpu")


def _base_params(rig: KeypointRig, poses: torch.Tensor, num_betas: int) -> Dict[str, torch.Tensor]:
    """The 6-D parameter dict of the B base poses: identity global_orient, zero transl, zero betas, expression and hand offsets."""
    B, dev = poses.shape[0], rig.device
    eye6 = lambda J: torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0], device=dev).repeat(B, J, 1)
    z = lambda *s: torch.zeros(*s, device=dev)
    return {"global_orient": eye6(1), "body_pose": smplify.rotation_6d_from_rotvec(poses.to(dev, torch.float32).reshape(B, 21, 3)),
            "left_hand_pose": eye6(15), "right_hand_pose": eye6(15), "betas": z(1, num_betas), "transl": z(B, 3), "jaw_pose": z(B, 3),
            "leye_pose": z(B, 3), "reye_pose": z(B, 3), "expression": z(B, rig.NB - num_betas)}


@torch.no_grad()
def init_from_keypoints(rig: KeypointRig, target_kps, img_wh, Ks=None, w2c=None, rotations=None, poses=None, num_betas: int = 10,
                        sigma: float = 100.0, conf_min: float = CONF_MIN, z_min: float = Z_MIN, min_points: int = MIN_POINTS,
                        rot_weight: float = ROT_WEIGHT, switch_cost: float = SWITCH_COST):
    """``(init_params, Ks, info)``: a start for ``SMPLify.fit`` from keypoints alone (module docstring: **not SMPLer-X**).

    ``init_params`` has ``load_smplerx``'s keys and shapes with rotation vectors: zero ``betas [N,num_betas]`` and ``expression``, the
    chosen base pose, ``global_orient`` from the chosen rotation, the path's translations, the hands at the rig's mean (zero
    offsets).  ``Ks`` defaults to ``default_intrinsics``, ``w2c`` to the identity, ``rotations [H,3,3]`` to ``rotation_bank()``,
    ``poses [B,63]`` to ``base_poses()``.  ``info`` is an ``InitInfo``."""
    dev = rig.device
    _hip(target_kps, "target_kps")
    target = target_kps.detach().to(device=dev, dtype=torch.float32).contiguous()
    N = target.shape[0]
    if not 1 <= num_betas <= rig.NB:
        raise ValueError(f"num_betas={num_betas}: the rig has {rig.NB} shape and expression directions")
    Ks = default_intrinsics(N, img_wh, device=dev) if Ks is None else _f32(Ks, "Ks", dev)
    w2c = torch.eye(4, device=dev) if w2c is None else _f32(w2c, "w2c", dev)
    rotations = rotation_bank(device=dev) if rotations is None else _f32(rotations, "rotations", dev)
    poses = base_poses(rig) if poses is None else _f32(poses, "poses", dev)
    if poses.dim() != 2 or poses.shape[1] != 63:
        raise ValueError(f"poses must be [B,63] rotation vectors (got {tuple(poses.shape)})")
    B, H = poses.shape[0], rotations.shape[0]
    points0 = smplify.model_points(rig, _base_params(rig, poses, num_betas))
    scales = smplify.target_scales(target, img_wh)
    res = search(points0, points0[:, 0].contiguous(), rotations, rig, target, Ks, w2c, img_wh, scales, sigma, conf_min, z_min, min_points)
    vit = viterbi_path(res.cost, transition_cost(rotations, B, rot_weight, switch_cost), res.transl, res.valid)
    b, h = vit.path // H, vit.path % H
    z = lambda *s: torch.zeros(*s, device=dev)
    init = {"global_orient": smplify.rotmat_to_rotvec(rotations[h]), "body_pose": poses[b].clone(), "left_hand_pose": z(N, 45),
            "right_hand_pose": z(N, 45), "betas": z(N, num_betas), "transl": vit.transl_path, "jaw_pose": z(N, 3), "leye_pose": z(N, 3),
            "reye_pose": z(N, 3), "expression": z(N, rig.NB - num_betas)}
    cost = torch.gather(res.cost, 1, vit.path[:, None])[:, 0]
    return init, Ks, InitInfo(vit.path, res.valid, cost)


def fit_from_keypoints(rig: KeypointRig, target_kps, img_wh, Ks=None, w2c=None, prior_weight: float = PRIOR_WEIGHT, prior_fit=None, fit=None,
                       make_fit: Optional[Callable[..., SMPLify]] = None, **init_kw) -> FitResult:
    """``extract keypoints -> fit`` without SMPLer-X: ``init_from_keypoints``; then ``SMPLify(rig, hand_steps=0,
    preserve_weight=prior_weight).fit`` -- with a low weight the existing preserve term is the pose prior towards the searched pose;
    then ``SMPLify(rig).fit`` with the reference's defaults.  ``prior_fit`` / ``fit``: keyword arguments for the two ``SMPLify``
    objects (step counts, say).  ``make_fit(**kw)`` builds them (default ``SMPLify(rig, **kw)``): tests drive the same stages by a
    restated objective.  Returns a ``FitResult``: ``save_params(path, r.params, r.Ks, r.w2c, r.img_wh)``."""
    make = make_fit if make_fit is not None else (lambda **kw: SMPLify(rig, **kw))
    init, Ks, info = init_from_keypoints(rig, target_kps, img_wh, Ks, w2c, **init_kw)
    w2c = torch.eye(4, device=rig.device) if w2c is None else w2c
    first = make(**{"hand_steps": 0, "preserve_weight": prior_weight, **(prior_fit or {})})
    mid = first.fit(init, Ks, w2c, img_wh, target_kps)
    second = make(**(fit or {}))
    out = second.fit(mid, Ks, w2c, img_wh, target_kps)
    return FitResult(out, Ks, w2c, tuple(img_wh), info)


__all__ = ["SearchResult", "ViterbiResult", "InitInfo", "FitResult", "search", "viterbi", "viterbi_path", "transition_cost",
           "default_intrinsics", "rotation_bank", "base_poses", "init_from_keypoints", "fit_from_keypoints", "PARAM_KEYS", "POSE_KEYS"]
