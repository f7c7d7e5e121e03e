"""Time the mesh decimation (soar_amd/mesh.py: simplify, decimate) on the 256^3 marching-cubes mesh of an analytic capsule or
sphere, on one GPU, in one process after warm-up.

    python scripts/mesh_simplify_time.py [--shape capsule|sphere] [--resolution 256] [--iters 10] [--out profiles/mesh_simplify_time.json]

  * `simplify` alone at the cell size `decimate` ends on, wall clock around a device synchronise (the call itself reads its
    bounding box and its totals back: two synchronisations inside);
  * `decimate` to 100k faces: the counting passes of the search plus that one `simplify`;
  * the bytes the computation has to move at the least (the input mesh read once, the output mesh written once) over the time of
    `simplify`, next to the 8 TB/s roofline.  The sorts, scans and the (cluster, face) stream move several times that; the share
    says how far the whole call is from a single streaming pass, not how well any one kernel runs.
There is no earlier path in this tree to compare with and pymeshlab is not installed: the figures stand alone, no bar is set."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from soar_amd import mesh  # noqa: E402

HBM_ROOFLINE = 8.0e12


def wall(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def analytic_field(shape, n, dev):
    a = torch.arange(n, dtype=torch.float32, device=dev)
    g = torch.stack(torch.meshgrid(a, a, a, indexing="ij"), -1)
    c = torch.tensor([0.497, 0.503, 0.501], device=dev) * (n - 1)
    if shape == "sphere":
        return (g - c).norm(dim=-1) - 0.42 * n
    p0, p1 = c - torch.tensor([0.0, 0.28 * n, 0.0], device=dev), c + torch.tensor([0.0, 0.28 * n, 0.0], device=dev)
    ab = p1 - p0
    t = (((g - p0) * ab).sum(-1) / (ab * ab).sum()).clamp(0, 1)
    return (g - (p0 + t[..., None] * ab)).norm(dim=-1) - 0.17 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("capsule", "sphere"), default="capsule")
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target", type=int, default=mesh.DECIMATE_TARGET)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_simplify_time.py needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    v, f = mesh.marching_cubes(analytic_field(args.shape, args.resolution, dev))
    m = mesh.Mesh(v, f)
    V, F = int(v.shape[0]), int(f.shape[0])
    res = {"device": torch.cuda.get_device_name(0), "shape": args.shape, "resolution": args.resolution, "iters": args.iters,
           "vertices": V, "faces": F, "target_faces": args.target}

    probes = []
    L = float((v.max(0).values - v.min(0).values).max())
    s = mesh._Simplifier(v, f)

    def count_faces(r):
        probes.append(r)
        return s.count(mesh._f32(L / r))[1]

    R = mesh._decimate_cells(count_faces, args.target, 4096)
    cell = mesh._f32(L / R)
    out = mesh.simplify(m, cell)
    res.update(cells_along_longest_axis=R, cell=cell, counting_passes=len(probes), out_vertices=int(out.vertices.shape[0]),
               out_faces=int(out.faces.shape[0]), workspace_bytes=s.nb)

    res["simplify_ms"], res["simplify_min_ms"] = wall(lambda: mesh.simplify(m, cell), args.iters)
    res["decimate_ms"], res["decimate_min_ms"] = wall(lambda: mesh.decimate(m, args.target), args.iters)
    res["count_ms"], res["count_min_ms"] = wall(lambda: s.count(cell), args.iters)
    least = 12 * (V + F) + 12 * (res["out_vertices"] + res["out_faces"])
    res["simplify_least_bytes"] = least
    res["simplify_bytes_per_s"] = least / (res["simplify_ms"] * 1e-3)
    res["simplify_share_of_8TBs_roofline"] = res["simplify_bytes_per_s"] / HBM_ROOFLINE
    again = mesh.decimate(m, args.target)
    res["bit_reproducible"] = bool(torch.equal(again.vertices, out.vertices) and torch.equal(again.faces, out.faces))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
