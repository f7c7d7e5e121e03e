"""Avatar initialisation: SMPL-X vertices, midpoint subdivision, vertex normals and surfel frames (csrc/body.hip).

What the reference's ``"smpl-guidance"`` gets from ``smplx``, ``trimesh`` and ``pytorch3d`` in its ``configure``
(TS/utils/smpl.py:179-547) before any training step runs:

* ``smplx_vertices``: the body model's ``lbs()`` (TS/utils/smplx/lbs.py:197-241) plus ``transl`` for B frames in one launch --
  shape blend, pose-corrective blend shapes and skinning.  Forward only: the reference does not optimise SMPL parameters.
* ``subdivide``: what ``trimesh.remesh.subdivide`` does to a triangle mesh (``init_xyz_on_mesh``, :89-96): one new vertex per
  unique edge, four faces per face.  The new vertices follow the old ones **in ascending order of the edge key
  ``(min << 32) | max``**; this order is this project's own (``trimesh``'s is not reproduced: the points are an unordered cloud).
  Children of ``(a, b, c)``, at rows ``4 f .. 4 f + 3``: ``(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)``.
* ``vertex_normals`` and ``surfel_frames``: the vertex normals and the quaternions ``init_q`` of ``init_qso_on_mesh``
  (:99-120).  ``init_s`` / ``init_o`` are not ported: the reference throws them away (:412-424).

Every output is deterministic: the same input gives the same tensors bit for bit.  HIP only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check, ptr

WEIGHTINGS = {"angle": 0, "area": 1, "uniform": 2}       # SOAR_NORMALS_*


class Mesh(NamedTuple):
    vertices: torch.Tensor   # [V,3] float32
    faces: torch.Tensor      # [F,3] int32


def _hip(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name} is on '{where}': soar_amd.body runs on HIP devices only; there is no CPU fallback")


def _mesh_workspace(F: int, device: torch.device) -> Tuple[torch.Tensor, int]:
    nb = _bytes(hip_lib.lib().soar_mesh_workspace_bytes, "soar_mesh_workspace_bytes", int(F))
    return _workspace(nb, device), nb


def _mesh_args(verts: torch.Tensor, faces: torch.Tensor):
    _hip(verts, "verts")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"verts must be [V,3] and faces [F,3] (got {tuple(verts.shape)} / {tuple(faces.shape)})")
    return verts.detach().to(torch.float32).contiguous(), faces.detach().to(verts.device, torch.int32).contiguous()


# ---- the body model's vertices -----------------------------------------------------------------------------------------------

_joint_cache = {}


def _joint_transformer(body, dev):
    """One JointTransformer per body object and device (its regressed joint template does not change between calls)."""
    from .smplx_joints import JointTransformer
    key = (id(body), str(dev))
    hit = _joint_cache.get(key)
    if hit is None or hit[0] is not body:
        if len(_joint_cache) >= 8:
            _joint_cache.clear()
        hit = _joint_cache[key] = (body, JointTransformer(body.v_template, body.shapedirs, body.J_regressor, body.parents).to(dev))
    return hit[1]


@torch.no_grad()
def smplx_vertices(body, betas: torch.Tensor, full_pose: torch.Tensor, transl: Optional[torch.Tensor] = None,
                   joint_transformer=None) -> torch.Tensor:
    """Vertices [B,V,3] of the body model for B frames, in two launches (the joint chain, then C: soar_smplx_vertices).

    ``body``: an object with ``v_template [V,3], shapedirs [V,3,NB], posedirs [(J-1)*9, V*3], J_regressor [J,V], parents [J],
    lbs_weights [V,J]`` (what ``SMPLGuidance`` takes, plus ``posedirs``).  ``betas [1|B,NB]`` (shape and expression
    coefficients concatenated), ``full_pose [B,J*3]`` axis-angle with the global orientation first (any strides: it is made
    contiguous), ``transl [B,3]`` or None.  ``transl`` is added to the finished vertices as the reference does, not folded into
    the joint transforms.  A frame computed alone equals the same frame inside a batch bit for bit."""
    _hip(full_pose, "full_pose")
    if getattr(body, "posedirs", None) is None:
        raise ValueError("smplx_vertices needs body.posedirs [(J-1)*9, V*3]")
    dev = full_pose.device
    f = lambda x: None if x is None else x.detach().to(device=dev, dtype=torch.float32).contiguous()
    jt = joint_transformer if joint_transformer is not None else _joint_transformer(body, dev)
    consts = getattr(jt, "_body_consts", None)
    if consts is None or consts[0] is not body or consts[1].device != dev:
        consts = jt._body_consts = (body, f(body.v_template), f(body.shapedirs), f(body.posedirs), f(body.lbs_weights))
    _, vt, sd, pd, lw = consts
    V, J, NB = vt.shape[0], lw.shape[1], sd.shape[2]
    pose, be, tr = f(full_pose).reshape(-1, J * 3), f(betas).reshape(-1, NB), f(transl)
    B = pose.shape[0]
    if pd.shape != ((J - 1) * 9, V * 3) or sd.shape != (V, 3, NB) or lw.shape != (V, J):
        raise ValueError(f"bad body model: posedirs {tuple(pd.shape)}, shapedirs {tuple(sd.shape)}, lbs_weights {tuple(lw.shape)} "
                         f"for V={V}, J={J}")
    if be.shape[0] not in (1, B) or (tr is not None and tr.shape != (B, 3)):
        raise ValueError(f"bad shapes: betas {tuple(be.shape)}, transl {None if tr is None else tuple(tr.shape)} for B={B}")
    out = torch.empty(B, V, 3, dtype=torch.float32, device=dev)
    if B == 0 or V == 0:
        return out
    A = jt.hip(be, pose, None)                              # [B,J,4,4], without transl
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_smplx_vertices(B, V, J, NB, ptr(be), be.shape[0], ptr(vt), ptr(sd), ptr(pd), ptr(lw), ptr(pose),
                                                ptr(A), ptr(tr), ptr(out), _stream(dev)), "soar_smplx_vertices")
    return out


# ---- meshes ----------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def subdivide(verts: torch.Tensor, faces: torch.Tensor, levels: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """``levels`` midpoint subdivisions of an index triangle mesh -> (verts [V',3] float32, faces [F',3] int32).

    Any index mesh: open, non-manifold, with unused vertices.  Per level V' = V + E (E unique edges, read back once: this is
    set-up code) and F' = 4 F; a midpoint is ``(a + b) * 0.5`` in float32.  See the module docstring for the vertex order."""
    v, f = _mesh_args(verts, faces)
    dev = v.device
    L = hip_lib.lib()
    for _ in range(int(levels)):
        V, F = int(v.shape[0]), int(f.shape[0])
        if F == 0:
            break
        ws, nb = _mesh_workspace(F, dev)
        E = C.c_int64(0)
        with torch.cuda.device(dev):
            st = _stream(dev)
            check(L.soar_mesh_subdivide_edges(V, F, f.data_ptr(), ws.data_ptr(), nb, C.byref(E), st), "soar_mesh_subdivide_edges")
            vo = torch.empty(V + int(E.value), 3, dtype=torch.float32, device=dev)
            fo = torch.empty(4 * F, 3, dtype=torch.int32, device=dev)
            check(L.soar_mesh_subdivide(V, F, int(E.value), v.data_ptr(), f.data_ptr(), ws.data_ptr(), nb, vo.data_ptr(),
                                        fo.data_ptr(), st), "soar_mesh_subdivide")
        v, f = vo, fo
    return v, f


@torch.no_grad()
def vertex_normals(verts: torch.Tensor, faces: torch.Tensor, weighting: str = "angle") -> torch.Tensor:
    """Vertex normals [V,3]: the normalised sum, over the faces of a vertex, of ``weight * unit_face_normal``.

    ``weighting="angle"`` (the default) weights a face by its interior angle at the vertex.  This is what current ``trimesh``
    computes for ``Trimesh.vertex_normals`` **as far as its behaviour is remembered**: ``trimesh`` is not available where this
    project is built, so the correspondence could not be checked against the library.  ``"area"`` weights by the face's area
    and ``"uniform"`` by 1.  ``normalize`` is ``x / max(|x|, 1e-12)``: a zero-area face adds nothing and a vertex no face uses
    gets ``(0, 0, 0)``.  The faces of a vertex are added in ascending (face, corner) order without atomics."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting must be one of {sorted(WEIGHTINGS)} (got {weighting!r})")
    v, f = _mesh_args(verts, faces)
    dev = v.device
    V, F = int(v.shape[0]), int(f.shape[0])
    if V == 0 or F == 0:
        return torch.zeros(V, 3, dtype=torch.float32, device=dev)
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    ws, nb = _mesh_workspace(F, dev)
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_mesh_vertex_normals(V, F, v.data_ptr(), f.data_ptr(), WEIGHTINGS[weighting], ws.data_ptr(), nb,
                                                     out.data_ptr(), _stream(dev)), "soar_mesh_vertex_normals")
    return out


@torch.no_grad()
def surfel_frames(normals: torch.Tensor, rand_dir: Optional[torch.Tensor] = None,
                  generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Quaternions [P,4] (real part first) of the surfel frames of ``init_qso_on_mesh`` (TS/utils/smpl.py:115-120):
    ``ux = normalize(uz x rand_dir)``, ``uy = normalize(uz x ux)``, columns ``[ux, uy, uz]``, then ``matrix_to_quaternion``
    in pytorch3d's convention, with a non-negative real part and a final normalisation (the identity up to rounding for a
    rotation matrix; a degenerate frame -- a zero normal, ``rand_dir`` parallel to it -- still gives a finite unit quaternion).

    ``rand_dir [P,3]`` defaults to standard normal draws from ``generator`` (a CPU or device ``torch.Generator``; the global
    generator of the normals' device when None)."""
    _hip(normals, "normals")
    dev = normals.device
    n = normals.detach().to(torch.float32).contiguous()
    if n.dim() != 2 or n.shape[1] != 3:
        raise ValueError(f"normals must be [P,3] (got {tuple(n.shape)})")
    P = int(n.shape[0])
    if rand_dir is None:
        gdev = dev if generator is None else generator.device
        rand_dir = torch.randn(P, 3, generator=generator, device=gdev)
    rd = rand_dir.detach().to(dev, torch.float32).contiguous()
    if rd.shape != n.shape:
        raise ValueError(f"rand_dir must have the shape of normals (got {tuple(rd.shape)})")
    out = torch.empty(P, 4, dtype=torch.float32, device=dev)
    if P == 0:
        return out
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_mesh_vertex_frames(P, n.data_ptr(), rd.data_ptr(), out.data_ptr(), _stream(dev)),
              "soar_mesh_vertex_frames")
    return out
