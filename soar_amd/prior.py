"""The SMPL-X normal priors: the fitted body of every frame drawn as a normal map into the crop's camera, from the front and from
behind -- the ``prior_F`` / ``prior_B`` (the reference's ``T_normal_F`` / ``T_normal_B``) that the normal networks take, on a
triangle-mesh rasterizer in HIP (csrc/prior.hip).

* ``MeshTopology(faces, num_verts)``: the static part, checked on the host: ``faces`` and the vertex-to-corner CSR table the vertex
  normals are summed from.
* ``render_normal_priors(topo, verts, w2c, Ks)``: three launches for all N frames -> ``prior [N,2,3,H,W]`` (unit normals on the body,
  exact zeros off it), ``mask [N,2,H,W]`` uint8, ``face [N,2,H,W]`` int32 (-1 off the body); view 0 is the front, view 1 the rear.
* ``body_normal_priors(body, params, normal_Ks, w2c, topo)``: ``smplx_vertices`` on fitted parameters, then the renderer.
* ``estimate_normals_from_body(net, images, masks, Ks, verts, topo, w2c)``: the whole stage -- crop, priors, networks, bytes -- in
  chunks; its result is what ``normals.save_normals`` writes.

The renderer is this project's own definition: the reference draws its priors with a ``soar.rendering.render_mesh``
that is not part of its tree, so **the axis convention, the area weighting and the hard mask cannot be checked against the
reference's renderer**.  Vertices are snapped to 1/256 pixel and coverage is exact integer arithmetic with a top-left rule; there is
no back-face culling (the rear view needs the faces that point away), no clipping (a face with a vertex at ``z <= 1e-6`` or more
than 2^20 pixels from the origin is skipped whole) and no antialiasing.  Normals are area-weighted vertex normals, interpolated
perspective-correctly.  ``space="opengl"`` gives ``(x, -y, -z)`` of the OpenCV camera frame (y up, +z toward the viewer) in both
views; ``space="opencv"`` leaves the camera frame's axes.  Every output is deterministic, and a frame's output depends neither on
N nor on its place in the batch.  HIP only: CPU tensors are refused, there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from . import hip_lib
from .hip_lib import _stream, check, ptr

SPACES = {"opencv": 0, "opengl": 1}
MAX_SIDE = 4096                      # soar_prior_raster
INVALID = -(1 << 31)                 # snapped x / y of a vertex behind the camera or past the guard band


def _hip(t, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name} is on '{where}': soar_amd.prior runs on HIP devices only; there is no CPU fallback")


class MeshTopology:
    """``faces [F,3]`` (any integer type, host or device) of a mesh of ``num_verts`` vertices.  Every index is checked on the host;
    ``csr_offsets [V+1]`` / ``csr_corners [3F]`` list, per vertex, the corners ``3 face + corner`` that name it, ascending (a vertex
    no face uses has an empty row).  ``faces`` and the table are kept as int32 tensors on ``device`` (default: where ``faces`` is)."""

    def __init__(self, faces, num_verts: int, device=None):
        if isinstance(faces, torch.Tensor):
            if device is None:
                device = faces.device
            f = faces.detach().cpu().numpy()
        else:
            f = np.asarray(faces)
        if f.ndim != 2 or f.shape[1] != 3:
            raise ValueError(f"MeshTopology: faces must be [F,3] (got {tuple(f.shape)})")
        if f.dtype.kind not in "iu":
            raise ValueError(f"MeshTopology: faces must hold integers (got {f.dtype})")
        V = int(num_verts)
        if not 1 <= V <= 1 << 24 or f.shape[0] > 1 << 24:
            raise ValueError(f"MeshTopology: need 1 <= num_verts <= 2^24 and at most 2^24 faces (got {V}, {f.shape[0]})")
        f = f.astype(np.int64)
        bad = np.argwhere((f < 0) | (f >= V))
        if bad.size:
            i, c = (int(x) for x in bad[0])
            raise ValueError(f"MeshTopology: face {i} corner {c} has vertex index {int(f[i, c])}, outside [0, {V}) "
                             f"({bad.shape[0]} such corners)")
        flat = f.reshape(-1)
        corners = np.argsort(flat, kind="stable").astype(np.int32)           # ascending vertex, then ascending 3 face + corner
        offsets = np.zeros(V + 1, np.int64)
        np.cumsum(np.bincount(flat, minlength=V), out=offsets[1:])
        self.num_verts, self.num_faces = V, int(f.shape[0])
        dev = torch.device("cpu" if device is None else device)
        self.faces = torch.from_numpy(f.astype(np.int32)).to(dev)
        self.csr_offsets = torch.from_numpy(offsets.astype(np.int32)).to(dev)
        self.csr_corners = torch.from_numpy(corners).to(dev)

    @property
    def device(self) -> torch.device:
        return self.faces.device

    def to(self, device) -> "MeshTopology":
        self.faces, self.csr_offsets, self.csr_corners = (t.to(device) for t in (self.faces, self.csr_offsets, self.csr_corners))
        return self


def _check_call(topo, verts, w2c, Ks, img_wh, space):
    if not isinstance(topo, MeshTopology):
        raise TypeError(f"render_normal_priors: topo must be a MeshTopology (got {type(topo).__name__})")
    if space not in SPACES:
        raise ValueError(f"render_normal_priors: space must be one of {sorted(SPACES)} (got {space!r})")
    if not isinstance(verts, torch.Tensor) or verts.dim() != 3 or tuple(verts.shape[1:]) != (topo.num_verts, 3):
        raise ValueError(f"render_normal_priors: verts must be [N,{topo.num_verts},3] (got {tuple(getattr(verts, 'shape', ()))})")
    _hip(verts, "verts")
    if verts.dtype != torch.float32:
        raise TypeError(f"render_normal_priors: verts must be float32 (got {verts.dtype})")
    if topo.device != verts.device:
        raise RuntimeError(f"render_normal_priors: the topology is on '{topo.device}', verts on '{verts.device}': move it with "
                           ".to(device); there is no CPU fallback")
    N = verts.shape[0]
    W, H = (int(x) for x in img_wh)
    if not (1 <= W <= MAX_SIDE and 1 <= H <= MAX_SIDE):
        raise ValueError(f"render_normal_priors: img_wh must be 1 .. {MAX_SIDE} each (got {tuple(img_wh)})")
    if N > 65535:
        raise ValueError(f"render_normal_priors: at most 65535 frames per call (got {N})")
    w2c = torch.as_tensor(w2c)
    if tuple(w2c.shape) not in ((4, 4), (N, 4, 4)):
        raise ValueError(f"render_normal_priors: w2c must be [4,4] or [{N},4,4] (got {tuple(w2c.shape)})")
    Ks = torch.as_tensor(Ks)
    if tuple(Ks.shape) not in ((3, 3), (N, 3, 3)):
        raise ValueError(f"render_normal_priors: Ks must be [{N},3,3] or [3,3] (got {tuple(Ks.shape)})")
    return N, H, W, w2c, Ks


@torch.no_grad()
def render_normal_priors(topo: MeshTopology, verts: torch.Tensor, w2c, Ks, img_wh=(512, 512), space: str = "opengl",
                         debug: bool = False) -> Dict[str, torch.Tensor]:
    """``verts`` float32 ``[N,V,3]`` (any strides), ``w2c`` ``[4,4]`` or ``[N,4,4]`` (OpenCV camera: x right, y down, z forward),
    ``Ks`` ``[N,3,3]`` pixel intrinsics (fx, fy, cx, cy are read), ``img_wh = (W, H)`` -> dict(``prior [N,2,3,H,W]``,
    ``mask [N,2,H,W]``, ``face [N,2,H,W]``, and the views ``prior_F = prior[:, 0]``, ``prior_B = prior[:, 1]`` in the layout
    ``NormalNet`` takes).  ``debug=True`` adds what the vertex launch left: ``snapped [N,V,2]`` int32 (1/256 pixel; ``INVALID`` for
    a vertex that is skipped), ``inv_z [N,V]``, ``vertex_normals [N,V,3]`` (camera space) and ``face_boxes [N,F,4]`` int16 (first / last pixel column, first / last
    row a face's bounding box holds a sample of; an empty box for a face that draws nothing)."""
    N, H, W, w2c, Ks = _check_call(topo, verts, w2c, Ks, img_wh, space)
    dev = verts.device
    V, F = topo.num_verts, topo.num_faces
    prior = torch.empty((N, 2, 3, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((N, 2, H, W), dtype=torch.uint8, device=dev)
    face = torch.empty((N, 2, H, W), dtype=torch.int32, device=dev)
    snapped = torch.empty((N, V, 2), dtype=torch.int32, device=dev)
    inv_z = torch.empty((N, V), dtype=torch.float32, device=dev)
    vnrm = torch.empty((N, V, 3), dtype=torch.float32, device=dev)
    boxes = torch.empty((N, F, 4), dtype=torch.int16, device=dev)
    if N:
        verts = verts.detach()
        w2c = w2c.detach().to(dev, torch.float32).contiguous()
        Ks = Ks.detach().to(dev, torch.float32)
        Ks = (Ks.expand(N, 3, 3) if Ks.dim() == 2 else Ks).contiguous()
        L = hip_lib.lib()
        with torch.cuda.device(dev):
            s = _stream(dev)
            check(L.soar_prior_vertex_setup(N, V, F, verts.data_ptr(), (C.c_int64 * 3)(*verts.stride()), w2c.data_ptr(),
                                            int(w2c.dim() == 3), Ks.data_ptr(), ptr(topo.faces), topo.csr_offsets.data_ptr(),
                                            ptr(topo.csr_corners), snapped.data_ptr(), inv_z.data_ptr(), vnrm.data_ptr(), s),
                  "soar_prior_vertex_setup")
            check(L.soar_prior_face_boxes(N, V, F, ptr(topo.faces), snapped.data_ptr(), ptr(boxes), s), "soar_prior_face_boxes")
            check(L.soar_prior_raster(N, V, F, H, W, SPACES[space], ptr(topo.faces), snapped.data_ptr(), inv_z.data_ptr(),
                                      vnrm.data_ptr(), ptr(boxes), prior.data_ptr(), mask.data_ptr(), face.data_ptr(), s),
                  "soar_prior_raster")
    out = dict(prior=prior, mask=mask, face=face, prior_F=prior[:, 0], prior_B=prior[:, 1])
    if debug:
        out.update(snapped=snapped, inv_z=inv_z, vertex_normals=vnrm, face_boxes=boxes)
    return out


def full_pose(params: Mapping[str, torch.Tensor], pose_mean=None) -> torch.Tensor:
    """``[N,165]`` rotation vectors in SMPL-X joint order (global, 21 body, jaw, two eyes, 15 + 15 hand joints) from the parameter
    dict ``SMPLify.fit`` returns and ``save_params`` writes.  ``pose_mean [165]``: the body model's mean pose, added as
    ``SMPLX.forward`` adds it (the parameters are offsets from it)."""
    N = params["body_pose"].shape[0]
    keys = ("global_orient", "body_pose", "jaw_pose", "leye_pose", "reye_pose", "left_hand_pose", "right_hand_pose")
    pose = torch.cat([params[k].reshape(N, -1) for k in keys], dim=1)
    return pose if pose_mean is None else pose + torch.as_tensor(pose_mean).reshape(1, -1).to(pose)


@torch.no_grad()
def body_normal_priors(body, params: Mapping[str, torch.Tensor], normal_Ks, w2c, topo: MeshTopology, img_wh=(512, 512),
                       space: str = "opengl", pose_mean=None) -> Dict[str, torch.Tensor]:
    """The priors of N fitted frames: ``params`` as ``SMPLify.fit`` returns them (rotation vectors, ``betas [1|N,NBS]``,
    ``expression [N,NE]``, ``transl [N,3]``; device tensors), ``body`` as ``body.smplx_vertices`` takes it, ``normal_Ks [N,3,3]`` of
    ``crop_frames``, ``pose_mean`` as ``full_pose`` takes it.  Returns ``render_normal_priors``' dict plus ``verts [N,V,3]``."""
    from .body import smplx_vertices
    pose = full_pose(params, pose_mean)
    _hip(pose, "params")
    N = pose.shape[0]
    betas = params["betas"].reshape(-1, params["betas"].shape[-1])
    betas = torch.cat([betas.expand(N, -1), params["expression"].reshape(N, -1)], dim=1)
    verts = smplx_vertices(body, betas, pose, params["transl"])
    out = render_normal_priors(topo, verts, w2c, normal_Ks, img_wh, space)
    out["verts"] = verts
    return out


@torch.no_grad()
def estimate_normals_from_body(net, images, masks, Ks, verts: torch.Tensor, topo: MeshTopology, w2c, batch: int = 4,
                               space: str = "opengl") -> Dict[str, torch.Tensor]:
    """The preprocessing stage for a whole sequence with the priors drawn from the body: per chunk of ``batch`` frames the crop, the
    two priors in the crop's camera (the chunk's ``normal_Ks``), the networks and the bytes -> dict(normal_F, normal_B uint8
    ``[N,512,512,3]``, normal_mask uint8 ``[N,512,512]``, normal_Ks float32 ``[N,3,3]``), as ``normals.estimate_normals`` gives it.
    The priors of a chunk live only for that chunk; nothing is read back between the chunks: the masks' status words are looked at
    once, at the end."""
    from . import normals as nm
    images, masks = nm._frames(images, masks, "estimate_normals_from_body")
    N = images.shape[0]
    if batch < 1:
        raise ValueError(f"estimate_normals_from_body: batch must be >= 1 (got {batch})")
    if not isinstance(verts, torch.Tensor) or verts.dim() != 3 or verts.shape[0] != N:
        raise ValueError(f"estimate_normals_from_body: verts must be [{N},V,3] (got {tuple(getattr(verts, 'shape', ()))})")
    dev = images.device
    w2c = torch.as_tensor(w2c).to(dev, torch.float32)
    if tuple(w2c.shape) not in ((4, 4), (N, 4, 4)):
        raise ValueError(f"estimate_normals_from_body: w2c must be [4,4] or [{N},4,4] (got {tuple(w2c.shape)})")
    Ks = torch.as_tensor(Ks, dtype=torch.float32).to(dev)
    Ks = (Ks.expand(N, 3, 3) if Ks.dim() == 2 else Ks).contiguous()
    S = nm.CROP
    out = dict(normal_F=torch.empty((N, S, S, 3), dtype=torch.uint8, device=dev),
               normal_B=torch.empty((N, S, S, 3), dtype=torch.uint8, device=dev),
               normal_mask=torch.empty((N, S, S), dtype=torch.uint8, device=dev),
               normal_Ks=torch.empty((N, 3, 3), dtype=torch.float32, device=dev))
    status = torch.zeros((N,), dtype=torch.int32, device=dev)
    for i in range(0, N, batch):
        j = min(i + batch, N)
        image, mask, nKs, _, st = nm._crop_launch(images[i:j], masks[i:j], Ks[i:j])
        pr = render_normal_priors(topo, verts[i:j], w2c if w2c.dim() == 2 else w2c[i:j], nKs, (S, S), space)
        nF, nB = net(image, pr["prior_F"], pr["prior_B"])
        bF, bB, bM = nm.normal_bytes(nF, nB, mask)
        out["normal_F"][i:j], out["normal_B"][i:j], out["normal_mask"][i:j], out["normal_Ks"][i:j] = bF, bB, bM, nKs
        status[i:j] = st
    nm._raise_on_status(status)
    return out
