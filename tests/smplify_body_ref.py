"""Torch restatement, in any dtype, of the SMPLify objective for the body model the reference creates (``use_face_contour=True``,
``flat_hand_mean=False``): tests/smplify_ref.py with the two things ``SMPLX.forward`` adds (body_models.py:1306-1383).

* The pose mean: every rotation becomes a rotation vector, ``pose_mean`` is added, and ``batch_rodrigues`` (with its ``+ 1e-8``)
  makes the matrix ``lbs()`` sees.  ``detour=True`` sends all 52 optimised joints that way, as the reference does;
  ``detour=False`` only the joints whose mean row is non-zero, as the kernel does (for the others the detour is the identity map).
* The contour landmarks: per frame the row of ``dynamic_lmk_faces_idx`` / ``dynamic_lmk_bary_coords`` chosen by
  ``find_dynamic_lmk_idx_and_bcoords`` (lbs.py:82-99) from the neck's world rotation, appended to the static landmarks.  The row
  is an integer: no gradient passes through it.

The body ``m`` is ``smplify_ref``'s namespace plus ``dynamic_lmk_faces_idx [79,LD]``, ``dynamic_lmk_bary_coords [79,LD,3]``,
``neck_kin_chain`` (neck first, root last) and ``pose_mean [165]``; a body without the table keeps static landmarks, one
without a mean adds none.  ``rotmat_to_rotvec`` is this project's (``roma`` is absent where it is built), as in ``smplify_ref``."""
import math
import types

import numpy as np
import torch

import smplify_ref as sr
from soar_amd import smplx_joints as sj

POSE_KEYS, GRAD_KEYS, FIXED_KEYS, PARAM_KEYS = sr.POSE_KEYS, sr.GRAD_KEYS, sr.FIXED_KEYS, sr.PARAM_KEYS
ORDER = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")


def contour_row(R):
    """``R [N,3,3]`` (the neck's world rotation) -> the table's row, int64 ``[N]``: rot_mat_to_euler, the clamp at 39, torch.round
    (half to even) and the fold of the negative angles."""
    e = torch.atan2(-R[:, 2, 0], torch.sqrt(R[:, 0, 0] * R[:, 0, 0] + R[:, 1, 0] * R[:, 1, 0]))
    y = torch.round(torch.clamp(-e * 180.0 / np.pi, max=39)).to(torch.long)
    return torch.where(y >= 0, y, torch.where(y < -39, torch.full_like(y, 78), 39 - y))


def yaw_degrees(R):
    """What ``contour_row`` rounds, before the clamp."""
    return -torch.atan2(-R[:, 2, 0], torch.sqrt(R[:, 0, 0] * R[:, 0, 0] + R[:, 1, 0] * R[:, 1, 0])) * 180.0 / np.pi


def neck_rotation(m, R):
    """root . ... . neck of ``R [N,55,3,3]``."""
    chain = [int(j) for j in torch.as_tensor(m.neck_kin_chain).reshape(-1).tolist()]
    out = R[:, chain[0]]
    for j in chain[1:]:
        out = R[:, j] @ out
    return out


def full_rotations(params, pose_mean=None, detour=True):
    """[N,55,3,3] in the body model's joint order, the mean included."""
    N = params["transl"].shape[0]
    dt, dev = params["transl"].dtype, params["transl"].device
    mean = torch.zeros(55, 3, dtype=dt, device=dev) if pose_mean is None else torch.as_tensor(pose_mean).to(device=dev, dtype=dt).reshape(55, 3)
    out, j0 = [], 0
    for k in ORDER:
        x = params[k]
        if k in POSE_KEYS:
            Rk = sr.rotation_6d_to_matrix(x.reshape(N, -1, 6))
            nj = Rk.shape[1]
            mk = mean[j0:j0 + nj]
            through = sj.batch_rodrigues((sr.rotmat_to_rotvec(Rk) + mk[None]).reshape(-1, 3)).reshape(N, nj, 3, 3)
            if detour:
                Rk = through
            else:
                Rk = torch.where((mk != 0).any(-1)[None, :, None, None], through, Rk)
        else:
            nj = 1
            Rk = sj.batch_rodrigues(x.reshape(N, 3) + mean[j0][None]).reshape(N, 1, 3, 3)
        out.append(Rk)
        j0 += nj
    return torch.cat(out, 1)


def frame_model(m, row):
    """``m`` with the contour table's row ``row`` appended to the static landmarks: the body one frame sees."""
    d = dict(vars(m))
    d["lmk_faces_idx"] = torch.cat([torch.as_tensor(m.lmk_faces_idx).long(), torch.as_tensor(m.dynamic_lmk_faces_idx).long()[row]])
    d["lmk_bary_coords"] = torch.cat([torch.as_tensor(m.lmk_bary_coords), torch.as_tensor(m.dynamic_lmk_bary_coords)[row].to(m.lmk_bary_coords)])
    return types.SimpleNamespace(**d)


def keypoints(m, tables, params, Ks, w2c, detour=True, with_rows=False):
    """[N,137,2]: the projected OpenPose keypoints; with ``with_rows`` also the contour rows (None for a body without a table)."""
    src, dst, _ = tables
    N = Ks.shape[0]
    coef = torch.cat([params["betas"].mean(0, keepdim=True).expand(N, -1), params["expression"]], -1)
    R = full_rotations(params, getattr(m, "pose_mean", None), detour)
    rows = None
    if getattr(m, "dynamic_lmk_faces_idx", None) is not None:
        rows = contour_row(neck_rotation(m, R.detach()))
        pts = torch.cat([sr.model_points(frame_model(m, int(rows[f])), R[f:f + 1], coef[f:f + 1], params["transl"][f:f + 1]) for f in range(N)])
    else:
        pts = sr.model_points(m, R, coef, params["transl"])
    kps = sr.project(sr.convert_kps(pts, list(src), list(dst)), Ks, w2c)
    return (kps, rows) if with_rows else kps


def losses(m, tables, params, init_params, Ks, w2c, img_wh, target_kps, scales, weights=(100.0, 60.0, 10000.0), sigma=100.0,
           ignore_hands=False, detour=True, norm_frames=None):
    """``smplify_ref.losses`` on the keypoints above; the preserve and smooth terms read the 6-D parameters, without the mean."""
    N = Ks.shape[0]
    scale_n = 1.0 if norm_frames is None else float(N) / float(norm_frames)
    pred = keypoints(m, tables, params, Ks, w2c, detour)
    tgt = target_kps[..., :2] * target_kps.new_tensor(img_wh)
    conf = target_kps[..., 2:] * torch.as_tensor(tables[2]).to(target_kps)[:, None]
    if ignore_hands:
        conf = conf.clone()
        conf[:, 25:-70] = 0.0
    kp = (sr.gmof((pred - tgt) / scales[:, None, None] * 200.0, sigma) * conf).mean() * scale_n
    preserve = 0.0
    for k in params:
        term = torch.linalg.norm(params[k] - init_params[k], dim=-1).mean()
        preserve = preserve + (term if k == "betas" else term * scale_n)
    smooth = sr._sum_loop(sr.smooth_loss(params[k]) for k in ("body_pose", "global_orient", "left_hand_pose", "right_hand_pose"))
    return {"kp": weights[0] * kp, "preserve": weights[1] * preserve, "smooth": weights[2] * smooth}


def objective(m, tables, params, init_params, Ks, w2c, img_wh, target_kps, scales, dtype=torch.float64, device="cpu", **kw):
    """-> (losses {name: 0-d tensor}, grads {key: tensor}) of the summed objective in ``dtype`` on ``device``."""
    c = lambda x: torch.as_tensor(x).detach().to(device=device, dtype=dtype)
    p = {k: c(v).requires_grad_(k in GRAD_KEYS) for k, v in params.items()}
    p0 = {k: c(v) for k, v in init_params.items()}
    ls = losses(m, tables, p, p0, c(Ks), c(w2c), img_wh, c(target_kps), c(scales), **kw)
    sum(ls.values()).backward()
    return ({k: v.detach() for k, v in ls.items()}, {k: (p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])) for k in GRAD_KEYS})


def y_rotation(deg, dtype=torch.float64):
    """[len(deg),3,3]: rotations about y by ``deg`` degrees."""
    a = torch.as_tensor(deg, dtype=dtype) * (math.pi / 180.0)
    o, z = torch.ones_like(a), torch.zeros_like(a)
    return torch.stack((torch.cos(a), z, torch.sin(a), z, o, z, -torch.sin(a), z, torch.cos(a)), -1).reshape(-1, 3, 3)


# ---- the golden file ---------------------------------------------------------------------------------------------------------------

def golden_model(g, dynamic=True, mean=True):
    """The seeded body of tests/golden/smplify_body.npz; ``dynamic=False`` drops the contour table (the rig then appends its
    frontal row), ``mean=False`` the mean."""
    t = lambda k: torch.from_numpy(g[k])
    m = sr.golden_model(g)
    m.dynamic_lmk_faces_idx, m.dynamic_lmk_bary_coords = (t("dynamic_lmk_faces_idx"), t("dynamic_lmk_bary_coords")) if dynamic else (None, None)
    m.neck_kin_chain = t("neck_kin_chain")
    m.pose_mean = t("pose_mean") if mean else torch.zeros(165)
    return m


def static_model(m, row=0):
    """``m`` with row ``row`` of its contour table as 17 further static landmarks and no table: what the static rig sees."""
    s = frame_model(m, row)
    s.dynamic_lmk_faces_idx = s.dynamic_lmk_bary_coords = None
    return s
