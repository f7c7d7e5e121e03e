"""Texture atlas of the exported mesh (csrc/mesh_texture.hip): MeshLab's "trivial per-triangle parametrization" and "transfer vertex
attributes to texture", on the device, deterministic, without pymeshlab or xatlas.  ``soar_amd.mesh`` re-exports everything here.

* ``build_atlas``: every face gets half of a square cell of ``s`` texels a side, ``s`` a power of two that follows the face's area;
  the cells stand largest first along the Z-order curve of the image, so they are aligned and disjoint by construction.
* ``bake_texture``: the colour of every owned texel is ``vertex_attributes``' rule at the texel's 3-D point, then bytes as ``save_ply``
  makes them.  Bilinear filtering never mixes two faces ("Texture atlas"); mip-mapping is out of scope.
* ``save_textured_obj``: OBJ + MTL + PNG.

Every output is deterministic bit for bit.  HIP only; there is no CPU path (the writer works on host tensors).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import torch

from . import hip_lib
from .hip_lib import check

ATTR_K, ATTR_MAX_K = 4, 8        # soar_amd.mesh's (vertex_attributes)
MIN_SIZE, MAX_SIZE = 16, 16384
CHUNK_TEXELS = 1 << 20

# The ladder of face areas: LADDER_N float32 thresholds, eight to the octave, th[i] = M[i % 8] * 2^(i // 8 - LADDER_OCTAVES) with
# M[r] = float32(2^(r / 8)) given by its bits, so the table is the same wherever it is built.  A face's level is the number of
# thresholds <= its float32 area: a comparison, no logarithm.
LADDER_OCTAVES = 32
LADDER_N = 16 * LADDER_OCTAVES + 1
MANTISSA_BITS = (0x3F800000, 0x3F8B95C2, 0x3F9837F0, 0x3FA5FED7, 0x3FB504F3, 0x3FC5672A, 0x3FD744FD, 0x3FEAC0C7)
STEP_MIN = 15 - LADDER_N         # at this step even the highest level has floor((level + step) / 8) < 2: every side is 4


class Atlas(NamedTuple):
    uv: torch.Tensor         # [3F,2] float32, OBJ convention (v = 0 at the bottom); corners sit on texel centres
    uv_faces: torch.Tensor   # [F,3] int32: row f is 3f, 3f+1, 3f+2
    cell: torch.Tensor       # [F,4] int32: x0, y0 (image texels, row 0 at the top), s, half (0 lower, 1 upper)
    scale_step: int          # the ladder step that was picked
    size: int                # T


def _check_size(texture_size) -> int:
    T = texture_size
    if isinstance(T, bool) or not isinstance(T, int) or not (MIN_SIZE <= T <= MAX_SIZE) or T & (T - 1):
        raise ValueError(f"texture_size must be a power of two in [{MIN_SIZE}, {MAX_SIZE}] (got {texture_size!r})")
    return T


def ladder() -> torch.Tensor:
    """The LADDER_N thresholds, float32 on the host."""
    i = torch.arange(LADDER_N)
    mant = torch.tensor(MANTISSA_BITS, dtype=torch.int64).to(torch.int32).view(torch.float32)
    return torch.ldexp(mant[i % 8], (i // 8 - LADDER_OCTAVES).to(torch.int32))            # times a power of two: exact


def _units(hist, step: int, T: int) -> int:
    """4 x 4 texel units that the cells take at ``step``: per side s, ceil(faces / 2) cells of (s / 4)^2 units.  ``hist``: faces per
    level 0 .. LADDER_N, then the faces without an area (side 4)."""
    top = T.bit_length() - 2                                                  # log2(T / 2)
    per_side = [0] * (top + 1)
    for level in range(LADDER_N + 1):
        if hist[level]:
            per_side[min(max((level + step) // 8, 2), top)] += hist[level]
    per_side[2] += hist[LADDER_N + 1]
    return sum(((per_side[L] + 1) // 2) << (2 * (L - 2)) for L in range(2, top + 1))


def pick_step(hist, T: int) -> int:
    """The largest step in [STEP_MIN, 8 log2(T / 2)] whose cells fit the (T / 4)^2 units, in exact integers.  (The unit count is not
    monotone in the step -- two odd sizes that merge save a cell -- so every step is tried, from the top.)"""
    F = sum(hist)
    for step in range(8 * (T.bit_length() - 2), STEP_MIN - 1, -1):
        if _units(hist, step, T) <= (T // 4) ** 2:
            return step
    need = MIN_SIZE
    while F > need * need // 8:
        need *= 2
    raise ValueError(f"texture_size={T} cannot hold {F} faces (two to a cell of 4 x 4 texels at the least): the smallest that can is {need}")


@torch.no_grad()
def build_atlas(mesh, texture_size: int) -> Atlas:
    """One chart per face: ``Atlas(uv, uv_faces, cell, scale_step, size)`` for a ``T x T`` texture, ``T = texture_size`` a power of two
    in [16, 16384].

    Every face gets half of a square cell of side ``s`` texels, ``s`` a power of two in [4, T/2]; two faces share a cell.
    ``s = clamp(2^floor((level + scale_step) / 8), 4, T/2)``: ``level`` counts the thresholds of an eighth-octave ladder that the
    face's float32 area reaches, ``scale_step`` is the one global step, the largest at which everything fits, so texel density is
    within a factor 2 in ``s`` across the mesh.  A face whose area is zero or not finite gets ``s = 4``.  Faces ordered by
    decreasing ``s``, then index, pair up (lower half, upper half; an odd last one keeps its cell) and the cells follow each other
    on the Z-order curve of the image's 4 x 4 texel units.  Local texels ``(a, b)``, ``m = s - 3``: the lower half has its corners
    at the centres of (0,0), (m,0), (0,m) and owns ``a + b <= s - 1``; the upper half at (s-1,s-1), (s-1-m,s-1), (s-1,s-1-m) and
    owns ``a + b >= s``.  Integer arithmetic throughout: the same mesh gives the same atlas bit for bit.  One histogram of the
    levels is read back; ``scale_step`` is chosen on the host.  More than ``T^2 / 8`` faces are refused."""
    from . import mesh as M
    T = _check_size(texture_size)
    verts, faces = M._mesh_tensors(mesh)
    dev = verts.device
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if F == 0:
        return Atlas(torch.zeros(0, 2, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev),
                     torch.zeros(0, 4, dtype=torch.int32, device=dev), 8 * (T.bit_length() - 2), T)
    L = hip_lib.lib()
    nb = M._bytes(L.soar_mesh_atlas_bytes, "soar_mesh_atlas_bytes", F)
    ws = M._workspace(nb, dev)
    th = ladder().to(dev)
    hist = (C.c_int64 * (LADDER_N + 2))()
    uv = torch.empty(3 * F, 2, device=dev)
    uv_faces = torch.empty(F, 3, dtype=torch.int32, device=dev)
    cell = torch.empty(F, 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = M._stream(dev)
        check(L.soar_mesh_atlas_levels(V, F, verts.data_ptr(), faces.data_ptr(), th.data_ptr(), LADDER_N, ws.data_ptr(), nb, hist, st),
              "soar_mesh_atlas_levels")
        step = pick_step(list(hist), T)
        check(L.soar_mesh_atlas_place(F, T, LADDER_N, step, ws.data_ptr(), nb, uv.data_ptr(), uv_faces.data_ptr(), cell.data_ptr(), st),
              "soar_mesh_atlas_place")
    return Atlas(uv, uv_faces, cell, step, T)


@torch.no_grad()
def bake_texture(mesh, atlas: Atlas, means3D: torch.Tensor, colors: torch.Tensor, k: int = ATTR_K, chunk_texels: int = CHUNK_TEXELS,
                 return_debug: bool = False):
    """The surfels' colours baked into ``atlas`` -> ``texture`` [T,T,3] uint8, row 0 at the top (as PIL writes it).

    Every owned texel gets barycentrics in UV space from the integers of its cell (lower half: ``b1 = a/m``, ``b2 = b/m``,
    ``b0 = 1 - b1 - b2``, the upper half mirrored; the gutter texels outside the triangle have their negative weight clamped to 0 and
    the three renormalised), the 3-D point ``b0 v0 + b1 v1 + b2 v2``, and as its colour exactly ``vertex_attributes``' rule at that
    point: the float32 mean of the ``k`` nearest surfels' colours from the same grid search, in the same order, clamped, then
    ``floor(255 c + 0.5)`` as in ``save_ply``.  The grid is built once; the texels are visited ``chunk_texels`` at a time, and the
    workspace is bounded by that, not by ``T^2``.  Unowned texels are (0,0,0).  A texel whose point is not finite (its face has
    such a vertex) has no nearest surfel -- ``vertex_attributes`` refuses such a query -- and is (0,0,0) too.

    ``return_debug=True`` -> ``(texture, dict(owner [T,T] int32 (face, -1 unowned), bary [T,T,3], position [T,T,3], color [T,T,3]
    the floats behind the bytes))``.  Runs on the current stream; no float atomics: two runs give the same bytes."""
    from . import mesh as M
    k, chunk_texels = int(k), int(chunk_texels)
    if not 1 <= k <= ATTR_MAX_K:
        raise ValueError(f"need 1 <= k <= {ATTR_MAX_K} (k={k})")
    if chunk_texels < 1:
        raise ValueError(f"chunk_texels must be >= 1 (chunk_texels={chunk_texels})")
    if not isinstance(atlas, Atlas):
        raise TypeError("atlas must be the Atlas that build_atlas returns")
    T = _check_size(atlas.size)
    verts, faces = M._mesh_tensors(mesh)
    for t, name in ((atlas.cell, "atlas.cell"), (means3D, "means3D"), (colors, "colors")):
        M._hip(t, name)
    dev = verts.device
    f32 = lambda t: t.detach().to(dev, torch.float32).contiguous()
    pts, col = f32(means3D), f32(colors)
    V, F, N = int(verts.shape[0]), int(faces.shape[0]), int(pts.shape[0]) if pts.dim() == 2 else -1
    if pts.dim() != 2 or pts.shape[1] != 3 or col.shape != pts.shape:
        raise ValueError(f"need means3D [N,3] and colors [N,3] (got {tuple(pts.shape)}, {tuple(col.shape)})")
    if k > N:
        raise ValueError(f"need k <= N (k={k}, N={N})")
    cell = atlas.cell.to(dev)
    if cell.shape != (F, 4) or cell.dtype != torch.int32:
        raise ValueError(f"atlas.cell must be [{F},4] int32, one row per face of the mesh (got {tuple(cell.shape)} {cell.dtype})")
    cell = cell.contiguous()
    texture = torch.zeros(T, T, 3, dtype=torch.uint8, device=dev)
    debug = None
    if return_debug:
        debug = dict(owner=torch.full((T, T), -1, dtype=torch.int32, device=dev), bary=torch.zeros(T, T, 3, device=dev),
                     position=torch.zeros(T, T, 3, device=dev), color=torch.zeros(T, T, 3, device=dev))
    if F == 0:
        return (texture, debug) if return_debug else texture
    L = hip_lib.lib()
    nb = M._bytes(L.soar_mesh_texels_bytes, "soar_mesh_texels_bytes", F)
    ws = M._workspace(nb, dev)
    total = C.c_int64(0)
    dbg = [debug[name].data_ptr() if debug else None for name in ("owner", "bary", "position", "color")]
    with torch.cuda.device(dev):
        st = M._stream(dev)
        check(L.soar_mesh_texel_offsets(V, F, T, faces.data_ptr(), cell.data_ptr(), ws.data_ptr(), nb, C.byref(total), st),
              "soar_mesh_texel_offsets")
        n_max = min(chunk_texels, int(total.value))
        grid = M._workspace(M._bytes(L.soar_lbs_knn_grid_bytes, "soar_lbs_knn_grid_bytes", N), dev)
        qws = M._workspace(M._bytes(L.soar_lbs_knn_query_bytes, "soar_lbs_knn_query_bytes", n_max), dev)
        tws = M._workspace(M._bytes(L.soar_mesh_attr_transfer_bytes, "soar_mesh_attr_transfer_bytes", n_max, k), dev)
        pos = torch.empty(n_max, 3, device=dev)
        addr = torch.empty(n_max, dtype=torch.int32, device=dev)
        idx = torch.empty(n_max, k, dtype=torch.int32, device=dev)
        blend = torch.empty(n_max, 3, device=dev)          # the query's own output, not used (see vertex_attributes)
        color = torch.empty(n_max, 3, device=dev)
        quality = torch.empty(n_max, device=dev)
        check(L.soar_lbs_knn_build_grid(pts.data_ptr(), N, col.data_ptr(), 3, grid.data_ptr(), st), "soar_lbs_knn_build_grid")
        for first in range(0, int(total.value), n_max):
            n = min(n_max, int(total.value) - first)
            check(L.soar_mesh_texels(V, F, T, verts.data_ptr(), faces.data_ptr(), cell.data_ptr(), ws.data_ptr(), nb, first, n,
                                     pos.data_ptr(), addr.data_ptr(), dbg[0], dbg[1], dbg[2], st), "soar_mesh_texels")
            check(L.soar_lbs_knn_query(grid.data_ptr(), N, col.data_ptr(), 3, pos.data_ptr(), n, k, blend.data_ptr(), idx.data_ptr(),
                                       qws.data_ptr(), qws.numel(), st), "soar_lbs_knn_query")
            check(L.soar_mesh_attr_transfer(n, N, k, pos.data_ptr(), pts.data_ptr(), col.data_ptr(), idx.data_ptr(), tws.data_ptr(),
                                            tws.numel(), color.data_ptr(), quality.data_ptr(), None, st), "soar_mesh_attr_transfer")
            check(L.soar_mesh_texture_write(n, T, addr.data_ptr(), color.data_ptr(), texture.data_ptr(), dbg[3], st),
                  "soar_mesh_texture_write")
    return (texture, debug) if return_debug else texture


def save_textured_obj(path: str, mesh, atlas: Atlas, texture: torch.Tensor, device_png: bool = False) -> None:
    """Three files: the Wavefront OBJ at ``path`` (``mtllib``, ``v x y z`` at float32 round-trip precision, the 3F ``vt u v`` lines,
    ``usemtl``, ``f a/ta b/tb c/tc`` with 1-based indices), ``<stem>.mtl`` next to it with ``map_Kd <stem>.png``, and that PNG
    (``texture`` [T,T,3] uint8, row 0 at the top).  Works on host copies of the tensors; ``device_png=True`` makes the PNG on the
    device instead (``png.save_png``; ``texture`` must then be on a HIP device): the same pixels, and only compressed bytes are copied."""
    import numpy as np
    from PIL import Image
    vertices, faces = mesh
    v = vertices.detach().cpu().to(torch.float32).tolist()
    f = faces.detach().cpu().to(torch.int64).tolist()
    uv = atlas.uv.detach().cpu().to(torch.float32)
    ft = atlas.uv_faces.detach().cpu().to(torch.int64)
    tex = texture.detach().cpu()
    T = int(atlas.size)
    if uv.shape != (3 * len(f), 2) or ft.shape != (len(f), 3):
        raise ValueError(f"atlas.uv / atlas.uv_faces must be [{3 * len(f)},2] / [{len(f)},3] (got {tuple(uv.shape)} / {tuple(ft.shape)})")
    if tex.shape != (T, T, 3) or tex.dtype != torch.uint8:
        raise ValueError(f"texture must be [{T},{T},3] uint8 (got {tuple(tex.shape)} {tex.dtype})")
    stem = os.path.splitext(os.path.basename(path))[0]
    folder = os.path.dirname(path)
    with open(path, "w") as fh:
        fh.write(f"mtllib {stem}.mtl\n")
        fh.writelines(f"v {a:.9g} {b:.9g} {c:.9g}\n" for a, b, c in v)
        fh.writelines(f"vt {a:.9g} {b:.9g}\n" for a, b in uv.tolist())
        fh.write("usemtl atlas\n")
        fh.writelines(f"f {a + 1}/{ta + 1} {b + 1}/{tb + 1} {c + 1}/{tc + 1}\n" for (a, b, c), (ta, tb, tc) in zip(f, ft.tolist()))
    with open(os.path.join(folder, stem + ".mtl"), "w") as fh:
        fh.write(f"newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd {stem}.png\n")
    if device_png:
        from .png import save_png
        save_png(os.path.join(folder, stem + ".png"), texture.detach())
        return
    Image.fromarray(np.ascontiguousarray(tex.numpy())).save(os.path.join(folder, stem + ".png"))
