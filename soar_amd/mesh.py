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

Every output is deterministic: the same input gives the same tensors bit for bit.  HIP only; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import hip_lib
from .hip_lib import check

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


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    if buf.data_ptr() % 256:
        raise RuntimeError("device allocation is not 256-byte aligned")
    return buf


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
    nb = C.c_size_t(0)
    check(L.soar_mc_workspace_bytes(X, Y, Z, C.byref(nb)), "soar_mc_workspace_bytes")
    ws = _workspace(nb.value, dev)
    counts = (C.c_int64 * 2)()
    mp = None if m is None else m.data_ptr()
    with torch.cuda.device(dev):
        st = _stream(dev)
        check(L.soar_mc_count(X, Y, Z, v.data_ptr(), mp, float(level), ws.data_ptr(), nb.value, counts, st), "soar_mc_count")
        verts = torch.empty(int(counts[0]), 3, device=dev)
        faces = torch.empty(int(counts[1]), 3, dtype=torch.int32, device=dev)
        if counts[0] > 0:
            check(L.soar_mc_emit(X, Y, Z, v.data_ptr(), mp, float(level), ws.data_ptr(), nb.value, verts.data_ptr(),
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
    nb = C.c_size_t(0)
    check(L.soar_mesh_filter_bytes(V, F, C.byref(nb)), "soar_mesh_filter_bytes")
    ws = _workspace(nb.value, dev)
    vo = torch.empty(V, 3, device=dev)
    fo = torch.empty(F, 3, dtype=torch.int32, device=dev)
    counts = (C.c_int64 * 2)()
    with torch.cuda.device(dev):
        check(L.soar_mesh_filter_components(V, F, vv.data_ptr(), ff.data_ptr(), int(min_faces), float(min_diag_frac), ws.data_ptr(),
                                            nb.value, vo.data_ptr(), fo.data_ptr(), counts, _stream(dev)),
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
        nb = C.c_size_t(0)
        check(self.lib.soar_mesh_simplify_bytes(self.V, self.F, C.byref(nb)), "soar_mesh_simplify_bytes")
        self.nb = nb.value
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
    non-manifold edges, and nothing repairs them."""
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


def decimate(mesh: Mesh, target_faces: int = DECIMATE_TARGET, max_cells: int = 4096) -> Mesh:
    """``mesh`` with at most ``target_faces`` faces: ``simplify`` at cell = L / R (float32), L the longest extent of the
    bounding box, R the integer ``_decimate_cells`` finds (about two dozen counting passes, two int64 read back from each).  A
    mesh within the budget comes back as it is, the same tensors.  The face count is not exactly monotone in R, so R is what
    the search finds, not a proven maximum.  (One cell, R = 1, leaves no face: every budget >= 0 can be met.)"""
    target_faces, max_cells = int(target_faces), int(max_cells)
    if target_faces < 0 or max_cells < 1:
        raise ValueError(f"need target_faces >= 0 and max_cells >= 1 (got {target_faces}, {max_cells})")
    verts, faces = _mesh_tensors(mesh)
    if faces.shape[0] <= target_faces:
        return mesh
    L = float((verts.max(0).values - verts.min(0).values).max())
    if not (L > 0.0 and math.isfinite(L)):
        raise ValueError(f"the mesh's bounding box has the longest extent {L}")
    s = _Simplifier(verts, faces)
    R = _decimate_cells(lambda r: s.count(_f32(L / r))[1], target_faces, max_cells)
    return s.run(_f32(L / R))


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
                 n_views: int = 48, image_size: int = 1024, group: int = 8, decimate_target: Optional[int] = None) -> Mesh:
    """World-space mesh of the surfels (rasterizer conventions: scales [P,3] with z = -1e10, opacities [P,1]).

    Renders ``n_views`` depth maps of ``image_size``^2 in groups of ``group`` views (one group's planes alive at a time), fuses
    them into a TSDF of ``resolution`` voxels along the longest axis, extracts the zero level set of the observed voxels and
    removes small components.  For a posed mesh, warp the surfels with ``soar_amd.lbs`` first.

    ``decimate_target``: None (the default) returns that mesh; a number runs ``decimate`` on it, the face budget of the
    reference's ``extract_mesh(decimate_target=1e5)`` (by vertex clustering, not pymeshlab's edge collapse)."""
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
        verts, faces = decimate(Mesh(verts, faces), int(decimate_target))
    org = torch.tensor(origin, dtype=torch.float32, device=dev)
    return Mesh(verts * voxel + org, faces)


def save_obj(path: str, mesh: Mesh) -> None:
    """Wavefront OBJ: ``v x y z`` lines (float32 round-trip precision), then ``f a b c`` lines with 1-based indices."""
    v = mesh.vertices.detach().cpu().to(torch.float32).tolist()
    f = mesh.faces.detach().cpu().to(torch.int64).tolist()
    with open(path, "w") as fh:
        fh.writelines(f"v {a:.9g} {b:.9g} {c:.9g}\n" for a, b, c in v)
        fh.writelines(f"f {a + 1} {b + 1} {c + 1}\n" for a, b, c in f)
