"""Mesh export of a surfel avatar: TSDF fusion of rendered depth, marching cubes, small-component removal (csrc/mesh.hip),
decimation to a face budget (csrc/mesh_simplify.hip).

Replaces the exporter behind every SOAR configuration (``exporter_type: "gaussiandreamer-mesh-exporter"`` ->
``geometry.extract_mesh()``).  The reference samples a 3-D Gaussian density built from ``get_scaling`` on a 128^3 grid
(TS/geometry/gaussian_io.py:176-262) -- not the footprint the surfel renderer draws -- and runs marching cubes and the
clean-up on the CPU (mcubes, pymeshlab).  Here the avatar is rendered as the renderer sees it, from ``n_views`` cameras on a
sphere, the depth is fused into a truncated signed-distance volume and its zero level set is extracted, all on the device.

* ``fuse_depth``: the kernel's TSDF integration (field sum / weight: positive outside, negative inside, weight 0 unobserved).
* ``marching_cubes``: welded, crack-free, outward-facing triangles in index coordinates (like ``mcubes.marching_cubes``).
* ``filter_components``: drops components with fewer than 64 faces or a bounding-box diagonal below 20 % of the mesh's
  (the reference's ``clean_mesh(min_f=64, min_d=20)``, geometry/mesh_utils.py:91-150).
* ``simplify`` / ``decimate``: quadric vertex clustering at a cell size / at the cell size a face budget asks for, in place of
  the reference's ``decimate_mesh`` (pymeshlab's quadric edge collapse, geometry/mesh_utils.py:45-88).  A different algorithm
  with the same purpose: no output is comparable bit for bit with pymeshlab's.
* ``extract_mesh``: the whole path, from the rasterizer's inputs to a world-space ``Mesh``.  A POSED mesh: warp the canonical
  surfels first (``soar_amd.lbs.lbs_warp(xyz, rot, weights, joint_mats)``) and pass the warped positions and rotations.
* ``vertex_attributes`` / ``prune_by_quality`` / ``adjacency`` / ``smooth`` (csrc/mesh_attr.hip): the colour of a vertex from its
  k nearest surfels, the squared distance to the nearest as its quality, pruning by that quality and Laplacian smoothing -- the
  reference's ``poisson_mesh`` refinement (utils/general_utils.py:269-302) ("Colour, smoothing, skinning").
* ``close_holes`` / ``open_border_edges`` (csrc/mesh_holes.hip): caps every simple border loop of at most ``max_hole_edges`` edges
  with a fan around its centroid, the place of ``meshing_close_holes(maxholesize=300)`` in that refinement -- a deterministic loop
  search, not MeshLab's ear cutting ("Closing holes") --, and the number of border edges of a mesh.
* ``repair_manifold`` / ``manifold_report`` (csrc/mesh_repair.hip): on every edge with more than two faces the smallest faces go
  until two are left, and every vertex whose faces form several fans is split -- the two repair filters of the reference's
  ``clean_mesh`` made order-free ("Repairing non-manifold edges and vertices"); ``repair=True`` of ``decimate``,
  ``extract_mesh`` and ``export_avatar`` runs it behind the clustering and the pruning.
* ``skin_weights`` / ``pose_mesh``: SMPL-X blend weights of the mesh vertices (the rule ``query_weights_smpl`` applies to surfels)
  and the mesh in any number of poses with the existing warp and normal kernels: one export, many frames.
* ``export_avatar``: all of it in the reference's order, from canonical surfels to mesh, colours, quality, normals and weights;
  ``save_obj`` / ``save_ply`` / ``save_skinned`` write them.
* ``build_atlas`` / ``bake_texture`` / ``save_textured_obj`` (soar_amd/texture.py, csrc/mesh_texture.hip): a per-face texture atlas baked
  from the surfels' colours, and the OBJ + MTL + PNG writer; ``export_avatar(texture_size=...)`` runs them ("Texture atlas").

Every output is deterministic: the same input gives the same tensors bit for bit.  HIP only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check

TSDF_MAX_VIEWS = 64          # views per soar_tsdf_integrate call
ZNEAR = 0.2                  # znear of the export cameras: voxels nearer than this to a camera are not observed by it
MIN_OPACITY = 0.5            # a pixel below this opacity is free space
TRUNC_VOXELS = 3.0           # truncation of the signed distance, in voxels
MIN_FACES, MIN_DIAG_FRAC = 64, 0.2


class Mesh(NamedTuple):
    vertices: torch.Tensor   # [V,3] float32, world space
    faces: torch.Tensor      # [F,3] int32, counter-clockwise seen from outside


def _hip(t: torch.Tensor, name: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on '{t.device}': soar_amd.mesh runs on HIP devices only; there is no CPU fallback")


def fuse_depth(depth: torch.Tensor, opac: torch.Tensor, viewmatrix: torch.Tensor, projmatrix: torch.Tensor, prcppoint: torch.Tensor,
               origin: Sequence[float], voxel: float, dims: Sequence[int],
               acc: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, trunc: Optional[float] = None, znear: float = ZNEAR,
               min_opacity: float = MIN_OPACITY) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fuse N rendered depth / opacity planes [N,H,W] (views with world_view_transform / full_proj_transform [N,4,4] and
    prcppoint [N,2]) into the TSDF of the grid [X,Y,Z] whose voxel (x,y,z) sits at origin + voxel * (x,y,z).

    Returns ``(sum, weight)`` [X,Y,Z]; ``acc`` = a previous ``(sum, weight)`` is accumulated into in place.  The field is
    sum / weight where weight > 0.  ``trunc`` defaults to 3 voxels."""
    _hip(depth, "depth")
    dev = depth.device
    if depth.dim() != 3 or opac.shape != depth.shape:
        raise ValueError(f"depth / opac must both be [N,H,W] (got {tuple(depth.shape)} / {tuple(opac.shape)})")
    N, H, W = depth.shape
    X, Y, Z = (int(d) for d in dims)
    f32 = lambda t: t.to(dev, torch.float32).contiguous()
    depth, opac = f32(depth), f32(opac)
    viewmatrix, projmatrix, prcppoint = f32(viewmatrix).reshape(N, 16), f32(projmatrix).reshape(N, 16), f32(prcppoint).reshape(N, 2)
    if acc is None:
        s = torch.zeros(X, Y, Z, device=dev)
        w = torch.zeros(X, Y, Z, device=dev)
    else:
        s, w = acc
        if s.shape != (X, Y, Z) or w.shape != (X, Y, Z) or s.dtype != torch.float32 or w.dtype != torch.float32 \
                or not (s.is_contiguous() and w.is_contiguous()) or s.device != dev or w.device != dev:
            raise ValueError("acc must be two contiguous float32 [X,Y,Z] tensors on the depth's device")
    t = TRUNC_VOXELS * float(voxel) if trunc is None else float(trunc)
    L = hip_lib.lib()
    with torch.cuda.device(dev):
        for k0 in range(0, N, TSDF_MAX_VIEWS):
            k1 = min(N, k0 + TSDF_MAX_VIEWS)
            check(L.soar_tsdf_integrate(k1 - k0, H, W, depth[k0].data_ptr(), opac[k0].data_ptr(), viewmatrix[k0].data_ptr(),
                                        projmatrix[k0].data_ptr(), prcppoint[k0].data_ptr(), float(origin[0]), float(origin[1]),
                                        float(origin[2]), float(voxel), X, Y, Z, t, float(znear), float(min_opacity),
                                        s.data_ptr(), w.data_ptr(), _stream(dev)), "soar_tsdf_integrate")
    return s, w


def marching_cubes(values: torch.Tensor, level: float = 0.0, valid: Optional[torch.Tensor] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Iso-surface of a dense [X,Y,Z] field at ``level`` -> (verts [V,3] float32 in index coordinates, faces [F,3] int32).

    Inside is ``value < level``; triangles face the values above level.  ``valid`` [X,Y,Z] (bool): edges carry vertices only
    between valid corners, cells emit triangles only when all 8 corners are valid.  Vertices that no face uses (at the edge
    of the valid region) are kept; ``filter_components`` drops them."""
    _hip(values, "values")
    dev = values.device
    if values.dim() != 3:
        raise ValueError(f"values must be [X,Y,Z] (got {tuple(values.shape)})")
    X, Y, Z = values.shape
    v = values.to(torch.float32).contiguous()
    m = None
    if valid is not None:
        if valid.shape != values.shape:
            raise ValueError("valid must have the shape of values")
        m = valid.to(dev, torch.bool).contiguous()
    L = hip_lib.lib()
    nb = _bytes(L.soar_mc_workspace_bytes, "soar_mc_workspace_bytes", X, Y, Z)
    ws = _workspace(nb, dev)
    counts = (C.c_int64 * 2)()
    mp = None if m is None else m.data_ptr()
    with torch.cuda.device(dev):
        st = _stream(dev)
        check(L.soar_mc_count(X, Y, Z, v.data_ptr(), mp, float(level), ws.data_ptr(), nb, counts, st), "soar_mc_count")
        verts = torch.empty(int(counts[0]), 3, device=dev)
        faces = torch.empty(int(counts[1]), 3, dtype=torch.int32, device=dev)
        if counts[0] > 0:
            check(L.soar_mc_emit(X, Y, Z, v.data_ptr(), mp, float(level), ws.data_ptr(), nb, verts.data_ptr(),
                                 faces.data_ptr() if counts[1] > 0 else verts.data_ptr(), st), "soar_mc_emit")
    return verts, faces


def filter_components(verts: torch.Tensor, faces: torch.Tensor, min_faces: int = MIN_FACES, min_diag_frac: float = MIN_DIAG_FRAC
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Drop the connected components with fewer than ``min_faces`` faces or a bounding-box diagonal below ``min_diag_frac``
    times the whole mesh's, and the vertices no face uses.  Kept vertices and faces stay in their input order."""
    _hip(verts, "verts")
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V == 0 or F == 0:
        return verts.new_zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32, device=dev)
    vv = verts.to(torch.float32).contiguous()
    ff = faces.to(dev, torch.int32).contiguous()
    L = hip_lib.lib()
    nb = _bytes(L.soar_mesh_filter_bytes, "soar_mesh_filter_bytes", V, F)
    ws = _workspace(nb, dev)
    vo = torch.empty(V, 3, device=dev)
    fo = torch.empty(F, 3, dtype=torch.int32, device=dev)
    counts = (C.c_int64 * 2)()
    with torch.cuda.device(dev):
        check(L.soar_mesh_filter_components(V, F, vv.data_ptr(), ff.data_ptr(), int(min_faces), float(min_diag_frac), ws.data_ptr(),
                                            nb, vo.data_ptr(), fo.data_ptr(), counts, _stream(dev)),
              "soar_mesh_filter_components")
    return vo[:int(counts[0])].clone(), fo[:int(counts[1])].clone()


# ---- decimation ------------------------------------------------------------------------------------------------------

DECIMATE_TARGET = 100_000    # the reference's extract_mesh(decimate_target=1e5)


def _f32(x: float) -> float:
    """x rounded to float32 (for a quotient of two float32 values: the float32 quotient)"""
    return C.c_float(x).value


def _mesh_tensors(mesh) -> Tuple[torch.Tensor, torch.Tensor]:
    verts, faces = mesh
    _hip(verts, "vertices")
    _hip(faces, "faces")
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError(f"vertices must be [V,3] float32 (got {tuple(verts.shape)} {verts.dtype})")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32 or faces.device != verts.device:
        raise ValueError(f"faces must be [F,3] int32 on the vertices' device (got {tuple(faces.shape)} {faces.dtype} on {faces.device})")
    return verts.contiguous(), faces.contiguous()


class _Simplifier:
    """The workspace and the two calls of one mesh (``decimate`` probes many cell sizes with one workspace)."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor):
        self.verts, self.faces = verts, faces
        self.V, self.F = int(verts.shape[0]), int(faces.shape[0])
        self.lib = hip_lib.lib()
        self.nb = _bytes(self.lib.soar_mesh_simplify_bytes, "soar_mesh_simplify_bytes", self.V, self.F)
        self.ws = _workspace(self.nb, verts.device)
        self.fptr = faces.data_ptr() if self.F > 0 else verts.data_ptr()

    def count(self, cell: float) -> Tuple[int, int]:
        counts = (C.c_int64 * 2)()
        with torch.cuda.device(self.verts.device):
            check(self.lib.soar_mesh_simplify_count(self.V, self.F, self.verts.data_ptr(), self.fptr, cell, self.ws.data_ptr(), self.nb,
                                                    counts, _stream(self.verts.device)), "soar_mesh_simplify_count")
        return int(counts[0]), int(counts[1])

    def run(self, cell: float) -> Mesh:
        dev = self.verts.device
        vo = torch.empty(self.V, 3, device=dev)
        fo = torch.empty(max(self.F, 1), 3, dtype=torch.int32, device=dev)
        counts = (C.c_int64 * 2)()
        with torch.cuda.device(dev):
            check(self.lib.soar_mesh_simplify(self.V, self.F, self.verts.data_ptr(), self.fptr, cell, self.ws.data_ptr(), self.nb,
                                              vo.data_ptr(), fo.data_ptr(), counts, _stream(dev)), "soar_mesh_simplify")
        return Mesh(vo[:int(counts[0])].clone(), fo[:int(counts[1])].clone())


def simplify(mesh: Mesh, cell: float) -> Mesh:
    """One pass of quadric vertex clustering (Lindstrom 2000) at cell size ``cell``: the vertices inside one cell of the uniform
    grid over the bounding box become one vertex, placed where the summed quadrics of the faces around them are least; faces
    that lose a corner this way, and repeated faces, go.  Surviving faces keep their order and winding.  DESIGN.md 9b states
    the computation; it is deterministic bit for bit.  Where two sheets of the surface pass through one cell the result has
    non-manifold edges: ``repair_manifold`` removes them (``manifold_report`` counts them; ``decimate(..., repair=True)`` does both
    steps)."""
    verts, faces = _mesh_tensors(mesh)
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError(f"cell must be positive and finite (got {cell})")
    if verts.shape[0] == 0:
        return Mesh(verts.new_zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32, device=verts.device))
    return _Simplifier(verts, faces).run(cell)


def _decimate_cells(count, target_faces: int, max_cells: int) -> int:
    """The search of ``decimate``: ``count(R)`` = faces left at ``R`` cells along the longest axis.  R doubles from 1 until
    count(R) > target_faces or R == max_cells; then a bisection under count(lo) <= target_faces < count(hi) -> lo."""
    lo, hi, R = 1, None, 1
    while True:
        if count(R) > target_faces:
            hi = R
            break
        lo = R
        if R >= max_cells:
            return lo
        R = min(2 * R, max_cells)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if count(mid) <= target_faces:
            lo = mid
        else:
            hi = mid
    return lo


def decimate(mesh: Mesh, target_faces: int = DECIMATE_TARGET, max_cells: int = 4096, repair: bool = False) -> Mesh:
    """``mesh`` with at most ``target_faces`` faces: ``simplify`` at cell = L / R (float32), L the longest extent of the
    bounding box, R the integer ``_decimate_cells`` finds (about two dozen counting passes, two int64 read back from each).  A
    mesh within the budget comes back as it is, the same tensors.  The face count is not exactly monotone in R, so R is what
    the search finds, not a proven maximum.  (One cell, R = 1, leaves no face: every budget >= 0 can be met.)

    The clustering leaves non-manifold edges where two sheets of the surface share a cell (fingers, an arm at the torso).  ``repair``:
    False (the default) returns the clustered mesh as it is; True returns ``repair_manifold`` of it, the mesh alone (the repair only
    removes faces, so the budget still holds)."""
    target_faces, max_cells = int(target_faces), int(max_cells)
    if target_faces < 0 or max_cells < 1:
        raise ValueError(f"need target_faces >= 0 and max_cells >= 1 (got {target_faces}, {max_cells})")
    verts, faces = _mesh_tensors(mesh)
    if faces.shape[0] <= target_faces:
        return repair_manifold(mesh)[0] if repair else mesh
    L = float((verts.max(0).values - verts.min(0).values).max())
    if not (L > 0.0 and math.isfinite(L)):
        raise ValueError(f"the mesh's bounding box has the longest extent {L}")
    s = _Simplifier(verts, faces)
    R = _decimate_cells(lambda r: s.count(_f32(L / r))[1], target_faces, max_cells)
    out = s.run(_f32(L / R))
    return repair_manifold(out)[0] if repair else out


# ---- the whole path --------------------------------------------------------------------------------------------------

def export_grid(means3D: torch.Tensor, scales: torch.Tensor, resolution: int):
    """-> (origin [3] float64 list, voxel, dims): the surfels' bounding box padded by the largest surfel radius (3 sigma of the
    in-plane scales) plus twice the truncation, ``resolution`` cubic voxels along the longest axis."""
    lo = means3D.min(0).values.double().cpu()
    hi = means3D.max(0).values.double().cpu()
    rmax = 3.0 * float(scales[:, :2].max())
    pad = 2.0 * TRUNC_VOXELS                                   # 2t, in voxels
    ext = (hi - lo) + 2.0 * rmax
    voxel = float(ext.max()) / (resolution - 1 - 2.0 * pad)
    dims = [int(min(resolution, math.ceil(float(e) / voxel + 2.0 * pad) + 1)) for e in ext]
    centre = (lo + hi) / 2.0
    origin = [float(centre[k] - 0.5 * (dims[k] - 1) * voxel) for k in range(3)]
    return origin, voxel, dims


def export_cameras(origin, voxel, dims, n_views: int, image_size: int, fov_deg: float = 40.0):
    """``n_views`` cameras on a Fibonacci sphere around the grid's centre, each far enough away for the grid's bounding sphere
    to fit its square field of view, znear = 0.2 -> [(world_view_transform, full_proj_transform, camera_center)], fov."""
    from .synthetic import camera_from_c2w
    centre = torch.tensor([origin[k] + 0.5 * (dims[k] - 1) * voxel for k in range(3)], dtype=torch.float64)
    radius = 0.5 * voxel * math.sqrt(sum((d - 1) ** 2 for d in dims))
    fov = math.radians(fov_deg)
    dist = max(radius / math.sin(0.5 * fov), radius + 2.0 * ZNEAR)
    golden = math.pi * (3.0 - math.sqrt(5.0))
    cams = []
    for i in range(n_views):
        y = 1.0 - 2.0 * (i + 0.5) / n_views
        r = math.sqrt(max(0.0, 1.0 - y * y))
        d = torch.tensor([r * math.cos(golden * i), y, r * math.sin(golden * i)], dtype=torch.float64)
        zc = d                                                          # OpenGL camera: looks along -z, so +z points back at it
        up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64) if abs(y) < 0.99 else torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
        xc = torch.nn.functional.normalize(torch.linalg.cross(up, zc), dim=0)
        yc = torch.linalg.cross(zc, xc)
        c2w = torch.eye(4, dtype=torch.float64)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = xc, yc, zc, centre + dist * d
        cams.append(camera_from_c2w(c2w, fov, fov, znear=ZNEAR, zfar=dist + radius + 1.0))
    return cams, fov


@torch.no_grad()
def render_depth(means3D, rotations, scales, opacities, cams, fov, image_size: int):
    """Depth and opacity planes [n,S,S] of the cameras ``cams`` (config (1,1,1,0): per-pixel surfel depth normalised by the
    opacity), rendered with the batched rasterizer."""
    from .rasterizer import GaussianRasterizationSettings, rasterize_views
    dev = means3D.device
    S = int(image_size)
    cfg = torch.tensor([1.0, 1.0, 1.0, 0.0], device=dev)
    bg = torch.zeros(3, device=dev)
    patch = torch.tensor([0.0, 0.0, S, S], device=dev)
    prcp = torch.tensor([0.5, 0.5], device=dev)
    tan = math.tan(0.5 * fov)
    colors = torch.zeros_like(means3D)
    means2D = torch.zeros_like(means3D)
    settings, inputs = [], []
    for wv, full, center in cams:
        settings.append(GaussianRasterizationSettings(S, S, tan, tan, bg, 1.0, wv.to(dev), full.to(dev), patch, prcp, 0, center.to(dev),
                                                      False, False, False, False, cfg))
        inputs.append(dict(means3D=means3D, means2D=means2D, opacities=opacities, colors_precomp=colors, scales=scales,
                           rotations=rotations))
    outs = rasterize_views(settings, inputs)
    depth = torch.stack([o[2].reshape(S, S) for o in outs])
    opac = torch.stack([o[3].reshape(S, S) for o in outs])
    return depth, opac


@torch.no_grad()
def extract_mesh(means3D: torch.Tensor, rotations: torch.Tensor, scales: torch.Tensor, opacities: torch.Tensor, resolution: int = 256,
                 n_views: int = 48, image_size: int = 1024, group: int = 8, decimate_target: Optional[int] = None,
                 repair: bool = False) -> Mesh:
    """World-space mesh of the surfels (rasterizer conventions: scales [P,3] with z = -1e10, opacities [P,1]).

    Renders ``n_views`` depth maps of ``image_size``^2 in groups of ``group`` views (one group's planes alive at a time), fuses
    them into a TSDF of ``resolution`` voxels along the longest axis, extracts the zero level set of the observed voxels and
    removes small components.  For a posed mesh, warp the surfels with ``soar_amd.lbs`` first -- or, for many poses of one
    avatar, export the canonical surfels once (``export_avatar``) and pose the mesh (``pose_mesh``).

    ``decimate_target``: None (the default) returns that mesh; a number runs ``decimate`` on it, the face budget of the
    reference's ``extract_mesh(decimate_target=1e5)`` (by vertex clustering, not pymeshlab's edge collapse).

    ``repair``: False (the default) changes nothing; True runs ``repair_manifold`` after the clustering (``decimate(..., repair=True)``;
    without a ``decimate_target``, on the filtered mesh), the two repair filters of the reference's ``clean_mesh``."""
    _hip(means3D, "means3D")
    dev = means3D.device
    f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
    means3D, rotations, scales, opacities = f32(means3D), f32(rotations), f32(scales), f32(opacities).reshape(-1, 1)
    origin, voxel, dims = export_grid(means3D, scales, resolution)
    cams, fov = export_cameras(origin, voxel, dims, n_views, image_size)
    acc = None
    prcp = torch.tensor([0.5, 0.5]).expand(len(cams), 2)
    for g0 in range(0, len(cams), group):
        sub = cams[g0:g0 + group]
        depth, opac = render_depth(means3D, rotations, scales, opacities, sub, fov, image_size)
        acc = fuse_depth(depth, opac, torch.stack([c[0] for c in sub]), torch.stack([c[1] for c in sub]), prcp[g0:g0 + len(sub)],
                         origin, voxel, dims, acc=acc)
        del depth, opac
    s, w = acc
    valid = w > 0
    field = torch.where(valid, s / w.clamp_min(1.0), torch.ones_like(s))
    del s, w
    verts, faces = marching_cubes(field, 0.0, valid)
    del field, valid
    verts, faces = filter_components(verts, faces)
    if decimate_target is not None:
        verts, faces = decimate(Mesh(verts, faces), int(decimate_target), repair=bool(repair))
    elif repair:
        verts, faces = repair_manifold(Mesh(verts, faces))[0]
    org = torch.tensor(origin, dtype=torch.float32, device=dev)
    return Mesh(verts * voxel + org, faces)


# ---- colour, quality, smoothing (csrc/mesh_attr.hip) -------------------------------------------------------------------------

ATTR_K, ATTR_MAX_K = 4, 8    # the reference's knn_points(K=4) (utils/general_utils.py:270); the kernel's upper bound
SMOOTH_STEPS = 3             # apply_coord_laplacian_smoothing(stepsmoothnum=3) (:301)


@torch.no_grad()
def vertex_attributes(vertices: torch.Tensor, means3D: torch.Tensor, colors: torch.Tensor, k: int = ATTR_K
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Colour and quality of mesh vertices [V,3] from the surfels (centres ``means3D`` [N,3], ``colors`` [N,3]) ->
    ``(color [V,3], quality [V], idx [V,k])``.

    ``idx``: the k nearest centres of every vertex (1 <= k <= 8, k <= N), from the exact grid search that also skins the surfels
    (``soar_lbs_knn_build_grid`` / ``_query``), nearest first, ties to the lower index.  ``color``: the float32 mean of their colours
    added in that order, clamped to [0,1].  ``quality``: the SQUARED distance to the nearest one, as pytorch3d's ``knn_points``
    returns it and the reference thresholds it (utils/general_utils.py:270-292)."""
    _hip(vertices, "vertices")
    _hip(means3D, "means3D")
    _hip(colors, "colors")
    dev = vertices.device
    f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
    v, pts, col = f32(vertices), f32(means3D), f32(colors)
    k = int(k)
    V, N = int(v.shape[0]), int(pts.shape[0])
    if v.dim() != 2 or v.shape[1] != 3 or pts.dim() != 2 or pts.shape[1] != 3 or col.shape != pts.shape:
        raise ValueError(f"need vertices [V,3], means3D [N,3] and colors [N,3] (got {tuple(v.shape)}, {tuple(pts.shape)}, {tuple(col.shape)})")
    if not (1 <= k <= ATTR_MAX_K and k <= N):
        raise ValueError(f"need 1 <= k <= min({ATTR_MAX_K}, N) (k={k}, N={N})")
    color = torch.empty(V, 3, device=dev)
    quality = torch.empty(V, device=dev)
    idx = torch.empty(V, k, dtype=torch.int32, device=dev)
    if V == 0:
        return color, quality, idx
    L = hip_lib.lib()
    grid = _workspace(_bytes(L.soar_lbs_knn_grid_bytes, "soar_lbs_knn_grid_bytes", N), dev)
    qws = _workspace(_bytes(L.soar_lbs_knn_query_bytes, "soar_lbs_knn_query_bytes", V), dev)
    tws = _workspace(_bytes(L.soar_mesh_attr_transfer_bytes, "soar_mesh_attr_transfer_bytes", V, k), dev)
    blend = torch.empty(V, 3, device=dev)      # the query's own output (the inverse-distance blend of the colours): not used
    with torch.cuda.device(dev):
        st = _stream(dev)
        # the colours ride as the grid's "skinning rows" (J = 3): the query needs some, and only its indices are kept
        check(L.soar_lbs_knn_build_grid(pts.data_ptr(), N, col.data_ptr(), 3, grid.data_ptr(), st), "soar_lbs_knn_build_grid")
        check(L.soar_lbs_knn_query(grid.data_ptr(), N, col.data_ptr(), 3, v.data_ptr(), V, k, blend.data_ptr(), idx.data_ptr(),
                                   qws.data_ptr(), qws.numel(), st), "soar_lbs_knn_query")
        check(L.soar_mesh_attr_transfer(V, N, k, v.data_ptr(), pts.data_ptr(), col.data_ptr(), idx.data_ptr(), tws.data_ptr(), tws.numel(),
                                        color.data_ptr(), quality.data_ptr(), None, st), "soar_mesh_attr_transfer")
    return color, quality, idx


@torch.no_grad()
def prune_by_quality(mesh: Mesh, quality: torch.Tensor, thresh: float) -> Tuple[Mesh, torch.Tensor]:
    """Drop the vertices with ``quality > thresh`` and every face that touches one (the reference's
    ``compute_selection_by_condition_per_vertex("q>thrsh")`` + ``meshing_remove_selected_vertices``) -> ``(Mesh, keep)``, ``keep``
    [V'] int32 the old index of every vertex left.  Kept vertices and faces stay in their order.  The holes this leaves are
    ``close_holes``' to close."""
    verts, faces = _mesh_tensors(mesh)
    _hip(quality, "quality")
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    q = quality.detach().to(dev, torch.float32).contiguous()
    if q.shape != (V,):
        raise ValueError(f"quality must be [{V}] (got {tuple(q.shape)})")
    thresh = float(thresh)
    if math.isnan(thresh):
        raise ValueError("thresh is not a number")
    if V == 0:
        return Mesh(verts, faces), torch.zeros(0, dtype=torch.int32, device=dev)
    L = hip_lib.lib()
    nb = _bytes(L.soar_mesh_prune_bytes, "soar_mesh_prune_bytes", V, F)
    ws = _workspace(nb, dev)
    vo = torch.empty(V, 3, device=dev)
    fo = torch.empty(max(F, 1), 3, dtype=torch.int32, device=dev)
    keep = torch.empty(V, dtype=torch.int32, device=dev)
    counts = (C.c_int64 * 2)()
    with torch.cuda.device(dev):
        check(L.soar_mesh_prune(V, F, verts.data_ptr(), faces.data_ptr() if F else None, q.data_ptr(), thresh, ws.data_ptr(), nb,
                                vo.data_ptr(), fo.data_ptr(), keep.data_ptr(), counts, _stream(dev)), "soar_mesh_prune")
    nv, nf = int(counts[0]), int(counts[1])
    return Mesh(vo[:nv].clone(), fo[:nf].clone()), keep[:nv].clone()


@torch.no_grad()
def adjacency(mesh: Mesh) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Vertex adjacency in CSR form -> ``(row_start [V+1] int32, nbr [6F] int32, border [V] bool)``.  Row i holds the two other
    corners of every face at vertex i, ascending: a neighbour across an edge of m faces stands m times.  ``border``: the vertex has
    an edge that belongs to exactly one face.  A face that names a vertex twice is refused."""
    verts, faces = _mesh_tensors(mesh)
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    row_start = torch.zeros(V + 1, dtype=torch.int32, device=dev)
    nbr = torch.empty(6 * F, dtype=torch.int32, device=dev)
    border = torch.zeros(V, dtype=torch.uint8, device=dev)
    if V > 0:
        L = hip_lib.lib()
        nb = _bytes(L.soar_mesh_adjacency_bytes, "soar_mesh_adjacency_bytes", V, F)
        ws = _workspace(nb, dev)
        with torch.cuda.device(dev):
            check(L.soar_mesh_adjacency(V, F, faces.data_ptr() if F else None, ws.data_ptr(), nb, row_start.data_ptr(),
                                        nbr.data_ptr() if F else None, border.data_ptr(), _stream(dev)), "soar_mesh_adjacency")
    return row_start, nbr, border.bool()


@torch.no_grad()
def smooth(mesh: Mesh, steps: int = SMOOTH_STEPS) -> Mesh:
    """``steps`` Jacobi steps of Laplacian smoothing with the uniform umbrella operator, the role of the reference's
    ``apply_coord_laplacian_smoothing(stepsmoothnum=3, boundary=True)`` ("Colour, smoothing, skinning" states the
    operator; it is this project's definition, not a bit copy of pymeshlab's).  A vertex moves to ``(P + S) / (n + 1)``: S sums, over every face at the vertex,
    that face's two other corners; a border vertex sums only its neighbours across border edges, so a border slides along itself;
    a vertex without neighbours stays.  Faces are unchanged.  Deterministic bit for bit."""
    verts, faces = _mesh_tensors(mesh)
    steps = int(steps)
    if steps < 0:
        raise ValueError(f"steps must be >= 0 (got {steps})")
    V = int(verts.shape[0])
    if V == 0 or steps == 0:
        return Mesh(verts.clone(), faces)
    dev = verts.device
    row_start, nbr, border = adjacency(Mesh(verts, faces))
    border = border.to(torch.uint8)
    L = hip_lib.lib()
    nb = _bytes(L.soar_mesh_smooth_bytes, "soar_mesh_smooth_bytes", V)
    ws = _workspace(nb, dev)
    out = torch.empty_like(verts)
    with torch.cuda.device(dev):
        check(L.soar_mesh_smooth(V, int(nbr.shape[0]), verts.data_ptr(), row_start.data_ptr(), nbr.data_ptr() if nbr.numel() else None,
                                 border.data_ptr(), steps, ws.data_ptr(), nb, out.data_ptr(), _stream(dev)), "soar_mesh_smooth")
    return Mesh(out, faces)


# ---- hole closing (csrc/mesh_holes.hip) -----------------------------------------------------------------------------------------

MAX_HOLE_EDGES = 300         # meshing_close_holes(maxholesize=300) (utils/general_utils.py:296)
HOLE_EDGES_RANGE = (3, 65535)


def _close_holes(verts: torch.Tensor, faces: torch.Tensor, max_hole_edges: int):
    """-> (verts_out, faces_out, loop_edges, counts[4]) of soar_mesh_close_holes, the outputs at their full capacity"""
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    L = hip_lib.lib()
    nb = _bytes(L.soar_mesh_close_holes_bytes, "soar_mesh_close_holes_bytes", V, F)
    ws = _workspace(nb, dev)
    vo = torch.empty(V + (3 * F) // 4, 3, device=dev)
    fo = torch.empty(max(4 * F, 1), 3, dtype=torch.int32, device=dev)
    loops = torch.empty(max(F, 1), dtype=torch.int32, device=dev)
    counts = (C.c_int64 * 4)()
    with torch.cuda.device(dev):
        check(L.soar_mesh_close_holes(V, F, verts.data_ptr(), faces.data_ptr() if F else None, int(max_hole_edges), ws.data_ptr(), nb,
                                      vo.data_ptr(), fo.data_ptr(), loops.data_ptr(), counts, _stream(dev)), "soar_mesh_close_holes")
    return vo, fo, loops, [int(c) for c in counts]


@torch.no_grad()
def close_holes(mesh: Mesh, max_hole_edges: int = MAX_HOLE_EDGES) -> Tuple[Mesh, torch.Tensor]:
    """Cap the holes of at most ``max_hole_edges`` border edges -> ``(Mesh, closed)``, ``closed`` [L] int32 the edge count of every
    loop that was closed, in output order.  The place of the reference's ``meshing_close_holes(maxholesize=300)``; the definition is
    this project's ("Closing holes"), a loop search with a centroid fan and not MeshLab's minimum-weight ear cutting.

    A border edge belongs to exactly one face (``adjacency``'s rule).  A border loop is closed when it has 3 .. ``max_hole_edges``
    edges, every vertex on it has exactly one border edge arriving and one leaving (two holes that touch in a vertex stay open, as
    MeshLab leaves non-manifold borders; ``repair_manifold`` first splits such a vertex, and both holes then close) and it is not the
    rim of a lone triangle.  A loop of three gets one face; a longer one a
    new vertex at the mean of its ring (summed in float64 in ring order) and one face per edge, each with the border edge reversed,
    so the patch continues the surface's orientation.  The rim of a small open component is a loop like any other.  The input's
    vertices and faces come first, unchanged; new vertices and faces follow loop by loop.  Deterministic bit for bit."""
    max_hole_edges = int(max_hole_edges)
    if not HOLE_EDGES_RANGE[0] <= max_hole_edges <= HOLE_EDGES_RANGE[1]:
        raise ValueError(f"need {HOLE_EDGES_RANGE[0]} <= max_hole_edges <= {HOLE_EDGES_RANGE[1]} (got {max_hole_edges})")
    verts, faces = _mesh_tensors(mesh)
    if verts.shape[0] == 0:
        return Mesh(verts.clone(), faces.clone()), torch.zeros(0, dtype=torch.int32, device=verts.device)
    vo, fo, loops, (nv, nf, nl, _) = _close_holes(verts, faces, max_hole_edges)
    return Mesh(vo[:nv].clone(), fo[:nf].clone()), loops[:nl].clone()


@torch.no_grad()
def open_border_edges(mesh: Mesh) -> int:
    """The number of border edges (edges of exactly one face) of ``mesh``: 0 for a watertight one.  ``soar_mesh_close_holes``' fourth
    count at the smallest ``max_hole_edges`` with the loops it closes added back, so nothing new is computed for it."""
    verts, faces = _mesh_tensors(mesh)
    if verts.shape[0] == 0 or faces.shape[0] == 0:
        return 0
    _, _, loops, (_, _, nl, still_open) = _close_holes(verts, faces, HOLE_EDGES_RANGE[0])
    return still_open + 3 * nl


# ---- repair of non-manifold edges and vertices (csrc/mesh_repair.hip) ----------------------------------------------------------

REPAIR_COUNTS = ("vertices", "faces", "non_manifold_edges", "faces_removed", "null_faces", "vertex_copies", "unreferenced_vertices",
                 "same_direction_edges", "border_edges")


class _Repairer:
    """The workspace and the two calls of one mesh with V >= 1 and F >= 1."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor):
        self.verts, self.faces = verts, faces
        self.V, self.F = int(verts.shape[0]), int(faces.shape[0])
        self.lib = hip_lib.lib()
        self.nb = _bytes(self.lib.soar_mesh_repair_workspace_size, "soar_mesh_repair_workspace_size", self.V, self.F)
        self.ws = _workspace(self.nb, verts.device)

    def count(self) -> dict:
        counts = (C.c_int64 * len(REPAIR_COUNTS))()
        dev = self.verts.device
        with torch.cuda.device(dev):
            check(self.lib.soar_mesh_repair_count(self.V, self.F, self.verts.data_ptr(), self.faces.data_ptr(), self.ws.data_ptr(), self.nb,
                                                  counts, _stream(dev)), "soar_mesh_repair_count")
        return dict(zip(REPAIR_COUNTS, (int(c) for c in counts)))

    def run(self, info: dict) -> Tuple[Mesh, torch.Tensor, dict]:
        dev = self.verts.device
        vo = torch.empty(max(info["vertices"], 1), 3, device=dev)
        fo = torch.empty(max(info["faces"], 1), 3, dtype=torch.int32, device=dev)
        src = torch.empty(max(info["vertices"], 1), dtype=torch.int32, device=dev)
        counts = (C.c_int64 * len(REPAIR_COUNTS))()
        with torch.cuda.device(dev):
            check(self.lib.soar_mesh_repair(self.V, self.F, self.verts.data_ptr(), self.faces.data_ptr(), self.ws.data_ptr(), self.nb,
                                            vo.data_ptr(), fo.data_ptr(), src.data_ptr(), counts, _stream(dev)), "soar_mesh_repair")
        got = dict(zip(REPAIR_COUNTS, (int(c) for c in counts)))
        if got != info:
            raise RuntimeError(f"soar_mesh_repair reports {got} after soar_mesh_repair_count reported {info} for the same mesh")
        return Mesh(vo[:info["vertices"]], fo[:info["faces"]]), src[:info["vertices"]], got


def _repair_empty(V: int) -> dict:
    info = dict.fromkeys(REPAIR_COUNTS, 0)
    info["unreferenced_vertices"] = V
    return info


@torch.no_grad()
def manifold_report(mesh: Mesh) -> dict:
    """What ``repair_manifold`` would do to ``mesh``, from the analysis alone: a dict of the nine counts ``REPAIR_COUNTS``; no output
    mesh is allocated or written.  The three to read: ``non_manifold_edges`` (edges of more than two faces), ``vertex_copies``
    (fans beyond the first at a vertex: bow-tie vertices) and ``border_edges`` (edges of one face in the repaired mesh).  A mesh with
    0 / 0 there, no ``null_faces`` and no ``unreferenced_vertices`` is one that ``repair_manifold`` returns as it is."""
    verts, faces = _mesh_tensors(mesh)
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V == 0 or F == 0:
        return _repair_empty(V)
    return _Repairer(verts, faces).count()


@torch.no_grad()
def repair_manifold(mesh: Mesh) -> Tuple[Mesh, torch.Tensor, dict]:
    """Remove the non-manifold edges and split the non-manifold vertices of ``mesh`` -> ``(Mesh, source, info)``: ``source`` [V']
    int32 the input vertex every output vertex came from (use it as ``prune_by_quality``'s keep map is used: ``color[source]``),
    ``info`` the nine counts ``REPAIR_COUNTS``.  The place of the reference's ``meshing_repair_non_manifold_edges(method=0)`` and
    ``meshing_repair_non_manifold_vertices(vertdispratio=0)`` (geometry/mesh_utils.py, ``clean_mesh``); the definition is this
    project's, MeshLab's rules made independent of any order ("Repairing non-manifold edges and vertices").

    A face that names a vertex twice goes.  On every edge with k > 2 faces the k - 2 smallest go (by the bits of the float32 squared
    area, ties by face index), in one pass: afterwards no edge has more than two faces.  Then, around every vertex, the faces that
    hang together through edges of exactly two faces form a fan; the fan with the least corner index keeps the vertex and every other
    fan gets a copy of it at the same place.  Kept vertices come first in their order (a vertex no surviving face names is dropped),
    then the copies; surviving faces keep their order and winding.  Inconsistent winding is counted (``same_direction_edges``) and
    not changed; nothing is re-oriented, merged or remeshed.  Running it on its own output changes nothing; a mesh that needs nothing
    comes back with equal bits and ``source == arange(V)``.  An empty mesh, or one without faces, gives empty results.  A face that
    names a vertex outside [0, V) is refused.  Deterministic bit for bit."""
    verts, faces = _mesh_tensors(mesh)
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if V == 0 or F == 0:
        return (Mesh(verts.new_zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32, device=dev)),
                torch.zeros(0, dtype=torch.int32, device=dev), _repair_empty(V))
    r = _Repairer(verts, faces)
    return r.run(r.count())                                   # the counts size the outputs; a refused mesh is refused before any is made


# ---- the rig -------------------------------------------------------------------------------------------------------------------

@torch.no_grad()
def skin_weights(mesh: Mesh, smpl_vertices: torch.Tensor, lbs_weights: torch.Tensor, K: int = 30) -> torch.Tensor:
    """Blend weights [V,J] of the mesh vertices: ``soar_amd.lbs.knn_blend_weights`` on them, the inverse-distance blend of the
    skinning rows of the K nearest canonical SMPL-X vertices that ``query_weights_smpl`` gives the surfels
    (TS/utils/smpl.py:618-637).  The mesh must be in the canonical space of ``smpl_vertices`` [Vs,3] / ``lbs_weights`` [Vs,J]."""
    from . import lbs
    verts, _ = _mesh_tensors(mesh)
    _hip(smpl_vertices, "smpl_vertices")
    return lbs.knn_blend_weights(verts, smpl_vertices, lbs_weights, K=int(K))


@torch.no_grad()
def pose_mesh(mesh: Mesh, weights: torch.Tensor, joint_mats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The canonical mesh in B poses -> ``(vertices [B,V,3], normals [B,V,3])``.  ``weights`` [V,J] from ``skin_weights``,
    ``joint_mats`` [B,J,4,4] (cano2live).  The positions are those of ``soar_lbs_warp_forward`` pose by pose (one batched launch,
    unit quaternions for the rotations it also warps); the normals are ``soar_mesh_vertex_normals`` (angle-weighted) of every
    posed mesh.  The faces do not change."""
    from . import body
    verts, faces = _mesh_tensors(mesh)
    _hip(weights, "weights")
    _hip(joint_mats, "joint_mats")
    dev = verts.device
    V = int(verts.shape[0])
    w = weights.detach().to(dev, torch.float32).contiguous()
    A = joint_mats.detach().to(dev, torch.float32).contiguous()
    if A.dim() != 4 or A.shape[2:] != (4, 4) or w.shape != (V, A.shape[1]):
        raise ValueError(f"need weights [V,J] and joint_mats [B,J,4,4] (got {tuple(w.shape)}, {tuple(A.shape)}; V={V})")
    B, J = int(A.shape[0]), int(A.shape[1])
    out = torch.empty(B, V, 3, device=dev)
    normals = torch.zeros(B, V, 3, device=dev)
    if B == 0 or V == 0:
        return out, normals
    rot = torch.zeros(V, 4, device=dev)
    rot[:, 0] = 1.0
    rot_out = torch.empty(B, V, 4, device=dev)
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_lbs_warp_forward_batch(verts.data_ptr(), rot.data_ptr(), w.data_ptr(), A.data_ptr(), B, V, J, out.data_ptr(),
                                                        rot_out.data_ptr(), _stream(dev)), "soar_lbs_warp_forward_batch")
    for b in range(B):
        normals[b] = body.vertex_normals(out[b], faces)
    return out, normals


def _surfel_tensors(model_or_tensors, use_explicit: bool):
    """-> (means3D, rotations, scales [P,3], opacities, colors) as the renderer hands them to the rasterizer.

    A 5-tuple or a dict with those names is taken as it is.  Anything else is a ``GaussianSurfelModel``, read as
    ``renderer/diff_gaussian.py`` reads it: scales [P,1] and colours [P,3] are the attribute field's ``scales`` and ``shs`` at the
    surfel centres, or, with ``use_explicit``, the leaves ``get_scaling`` / ``get_colors``; the scale is repeated to three columns
    and the third set to -1e10, the rasterizer's flat axis."""
    m = model_or_tensors
    if isinstance(m, dict):
        return tuple(m[k] for k in ("means3D", "rotations", "scales", "opacities", "colors"))
    if isinstance(m, (tuple, list)):
        if len(m) != 5:
            raise ValueError("need (means3D, rotations, scales, opacities, colors)")
        return tuple(m)
    xyz = m.get_xyz
    _hip(xyz, "get_xyz")
    if use_explicit:
        scale, colors = m.get_scaling, m.get_colors
    else:
        if getattr(m, "attribute_field", None) is None:
            raise ValueError("the model has no attribute_field: pass use_explicit=True to export its explicit scales and colours")
        fields = m.attribute_field(xyz.detach())
        scale, colors = fields["scales"], fields["shs"]
    if scale.dim() != 2 or scale.shape != (xyz.shape[0], 1):
        raise ValueError(f"the model's scale must be [{int(xyz.shape[0])},1] (got {tuple(scale.shape)})")
    scales = scale.detach().repeat(1, 3)
    scales[:, 2] = -1e10
    return xyz, m.get_rotation, scales, m.get_opacity, colors


def _check_surfels(means3D, rotations, scales, opacities, colors) -> None:
    """The rasterizer reads these buffers by the surfel count alone: every shape is checked before anything is launched."""
    P = int(means3D.shape[0]) if means3D.dim() == 2 else -1
    want = (("means3D", means3D, ((P, 3),)), ("rotations", rotations, ((P, 4),)), ("scales", scales, ((P, 3),)),
            ("opacities", opacities, ((P, 1), (P,))), ("colors", colors, ((P, 3),)))
    for name, t, shapes in want:
        if not isinstance(t, torch.Tensor) or P < 1 or tuple(t.shape) not in shapes:
            raise ValueError(f"{name} must be {' or '.join(str(list(s)) for s in shapes)} with P >= 1 "
                             f"(got {tuple(getattr(t, 'shape', ()))}; P is means3D's row count)")


@torch.no_grad()
def export_avatar(model_or_tensors, smpl_vertices: torch.Tensor, lbs_weights: torch.Tensor, resolution: int = 256,
                  decimate_target: Optional[int] = DECIMATE_TARGET, quality_thresh: Optional[float] = None,
                  smooth_steps: int = SMOOTH_STEPS, k: int = ATTR_K, K: int = 30, n_views: int = 48, image_size: int = 1024,
                  group: int = 8, use_explicit: bool = False, max_hole_edges: Optional[int] = None,
                  texture_size: Optional[int] = None, repair: bool = False) -> dict:
    """A coloured, animatable mesh from CANONICAL-space surfels in one call -> ``dict(mesh, color, quality, normals, weights)``.

    ``model_or_tensors``: the tuple ``(means3D [P,3], rotations [P,4], scales [P,3] with z = -1e10, opacities [P,1], colors [P,3]
    in [0,1])`` (or a dict with those names), or a ``GaussianSurfelModel``.  Of a model, scales and colours are what its renderer
    draws: the attribute field's outputs at the surfel centres, as every SOAR configuration has it (``use_explicit: false``), or
    the explicit leaves with ``use_explicit=True`` (the renderer's switch of that name).  Any other shape is refused.

    The steps in the reference's order (utils/general_utils.py:263-302): ``extract_mesh`` (with ``decimate_target``),
    ``vertex_attributes``, ``prune_by_quality`` when ``quality_thresh`` is given, ``close_holes`` when ``max_hole_edges`` is given,
    ``smooth``, then ``vertex_attributes`` again on the moved vertices (the colours and qualities returned), angle-weighted vertex
    normals and ``skin_weights`` against ``smpl_vertices`` / ``lbs_weights``.  ``pose_mesh(out["mesh"], out["weights"], joint_mats)``
    then gives any pose.

    ``max_hole_edges``: None (the default) closes nothing and returns exactly what this function returned before it had the
    argument.  A number closes the holes of at most that many edges that the pruning (or the extraction) left, before the smoothing,
    and the dict gains ``closed`` (``close_holes``' second result); 300 is recommended, the reference's ``maxholesize``.

    ``repair``: False (the default) changes nothing.  True runs ``repair_manifold`` twice: on ``extract_mesh``'s result, clustered
    or not, and again after ``prune_by_quality`` (which leaves bow-tie vertices), before ``close_holes``, so that holes that touch
    in a vertex can be closed; the dict gains ``repair``, the two ``info`` dicts in that order (the second is None without a
    ``quality_thresh``).  Colours, qualities and weights are computed after the repair, as they are after the pruning.

    ``texture_size``: None (the default) returns exactly that dict.  A power of two adds ``atlas`` (``build_atlas`` of the final,
    smoothed mesh) and ``texture`` (``bake_texture`` from the same surfel colours and ``k`` as the vertex colours), for
    ``save_textured_obj``; the texture belongs to the faces, so it rides along with every ``pose_mesh`` pose.  A size that is not a
    power of two in [16, 16384] is refused before anything runs.  Whether the size holds the mesh (``F <= T^2 / 8``: 1024 for the
    default budget of 100 000 faces) is known only once the mesh exists: the ``ValueError`` then names the smallest size that does
    and carries the finished dict, without ``atlas`` and ``texture``, as its ``result``, so that ``build_atlas`` can be called on
    ``result["mesh"]`` with that size instead of exporting again."""
    from . import body
    if texture_size is not None:
        texture._check_size(texture_size)                     # a malformed size is refused before the export, not after it
    means3D, rotations, scales, opacities, colors = _surfel_tensors(model_or_tensors, bool(use_explicit))
    _check_surfels(means3D, rotations, scales, opacities, colors)
    for t, name in ((means3D, "means3D"), (rotations, "rotations"), (scales, "scales"), (opacities, "opacities"), (colors, "colors")):
        _hip(t, name)
    dev = means3D.device
    f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
    means3D, colors = f32(means3D), f32(colors)
    m = extract_mesh(means3D, rotations, scales, opacities, resolution=resolution, n_views=n_views, image_size=image_size, group=group,
                     decimate_target=decimate_target)
    repaired = None
    if repair:
        m, _, first = repair_manifold(m)                      # on the world-space mesh, for its counts
        repaired = [first, None]
    if quality_thresh is not None:
        _, quality, _ = vertex_attributes(m.vertices, means3D, colors, k)
        m, _ = prune_by_quality(m, quality, quality_thresh)
        if repair:
            m, _, repaired[1] = repair_manifold(m)
    closed = None
    if max_hole_edges is not None:
        m, closed = close_holes(m, max_hole_edges)
    m = smooth(m, smooth_steps)
    color, quality, _ = vertex_attributes(m.vertices, means3D, colors, k)
    normals = body.vertex_normals(m.vertices, m.faces)
    weights = skin_weights(m, smpl_vertices.to(dev), lbs_weights.to(dev), K)
    out = dict(mesh=m, color=color, quality=quality, normals=normals, weights=weights)
    if closed is not None:
        out["closed"] = closed
    if repaired is not None:
        out["repair"] = repaired
    if texture_size is not None:
        try:
            out["atlas"] = build_atlas(m, texture_size)
        except ValueError as e:                               # too many faces for this size: known only now; the export is not lost
            err = ValueError(f"{e}; the export itself is done: this exception's `result` is the dict without atlas and texture")
            err.result = out
            raise err from e
        out["texture"] = bake_texture(m, out["atlas"], means3D, colors, k)
    return out


# ---- writers -------------------------------------------------------------------------------------------------------------------

def _host(t: Optional[torch.Tensor], rows: int, cols: Optional[int], name: str) -> Optional[torch.Tensor]:
    if t is None:
        return None
    h = t.detach().cpu().to(torch.float32)
    if h.shape != ((rows,) if cols is None else (rows, cols)):
        raise ValueError(f"{name} must be [{rows}{'' if cols is None else ',' + str(cols)}] (got {tuple(h.shape)})")
    return h.contiguous()


def save_obj(path: str, mesh: Mesh, colors: Optional[torch.Tensor] = None) -> None:
    """Wavefront OBJ: ``v x y z`` lines (float32 round-trip precision), then ``f a b c`` lines with 1-based indices.  With
    ``colors`` [V,3] the vertex lines are ``v x y z r g b``, the extension MeshLab reads and the reference's ``save_obj_mesh``
    writes."""
    v = mesh.vertices.detach().cpu().to(torch.float32).tolist()
    f = mesh.faces.detach().cpu().to(torch.int64).tolist()
    c = _host(colors, len(v), 3, "colors")
    with open(path, "w") as fh:
        if c is None:
            fh.writelines(f"v {a:.9g} {b:.9g} {c:.9g}\n" for a, b, c in v)
        else:
            fh.writelines(f"v {x:.9g} {y:.9g} {z:.9g} {r:.9g} {g:.9g} {b:.9g}\n" for (x, y, z), (r, g, b) in zip(v, c.tolist()))
        fh.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)


def save_ply(path: str, mesh: Mesh, colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
             quality: Optional[torch.Tensor] = None) -> None:
    """PLY, ``binary_little_endian 1.0``.  Vertex: float ``x y z``, then float ``nx ny nz`` with ``normals`` [V,3], uchar ``red green
    blue`` with ``colors`` [V,3] (floor(255 c + 0.5) of the colour clamped to [0,1]), float ``quality`` with ``quality`` [V].
    Face: ``list uchar int vertex_indices``."""
    import numpy as np
    v = _host(mesh.vertices, int(mesh.vertices.shape[0]), 3, "vertices")
    V = int(v.shape[0])
    f = mesh.faces.detach().cpu().to(torch.int32).contiguous().numpy()
    n, c, q = _host(normals, V, 3, "normals"), _host(colors, V, 3, "colors"), _host(quality, V, None, "quality")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if n is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if c is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if q is not None:
        fields += [("quality", "<f4")]
    rec = np.zeros(V, dtype=np.dtype(fields))
    for k, name in enumerate("xyz"):
        rec[name] = v[:, k].numpy()
    if n is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            rec[name] = n[:, k].numpy()
    if c is not None:
        c8 = torch.floor(c.clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).numpy()
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = c8[:, k]
    if q is not None:
        rec["quality"] = q.numpy()
    frec = np.zeros(len(f), dtype=np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    frec["n"] = 3
    frec["v"] = f
    kinds = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {V}"]
    header += [f"property {kinds[t]} {name}" for name, t in fields]
    header += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
        fh.write(frec.tobytes())


def save_skinned(path_npz: str, mesh: Mesh, weights: torch.Tensor, colors: torch.Tensor) -> None:
    """The rigged asset as an uncompressed ``.npz`` that ``numpy.load`` reads: ``vertices`` [V,3] float32, ``faces`` [F,3] int32,
    ``weights`` [V,J] float32, ``colors`` [V,3] float32.  ``pose_mesh`` (or any linear-blend skinning) poses it with [J,4,4] joint
    transforms.  The archive's members carry a fixed date (``numpy.savez`` stamps the time of writing): the same asset gives the
    same bytes."""
    import io
    import zipfile

    import numpy as np
    V = int(mesh.vertices.shape[0])
    w = weights.detach().cpu().to(torch.float32).contiguous()
    if w.dim() != 2 or w.shape[0] != V:
        raise ValueError(f"weights must be [{V},J] (got {tuple(w.shape)})")
    arrays = dict(vertices=_host(mesh.vertices, V, 3, "vertices").numpy(),
                  faces=mesh.faces.detach().cpu().to(torch.int32).contiguous().numpy(), weights=w.numpy(),
                  colors=_host(colors, V, 3, "colors").numpy())
    with zipfile.ZipFile(path_npz, "w", zipfile.ZIP_STORED) as zf:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


# ---- texture atlas (soar_amd/texture.py, csrc/mesh_texture.hip) -------------------------------------------------------------------

from . import texture  # noqa: E402
from .texture import Atlas, bake_texture, build_atlas, save_textured_obj  # noqa: E402,F401

assert (texture.ATTR_K, texture.ATTR_MAX_K) == (ATTR_K, ATTR_MAX_K)
