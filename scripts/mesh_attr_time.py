"""Time the stages that colour, smooth and prune the exported mesh (soar_amd/mesh.py: vertex_attributes, adjacency, smooth,
prune_by_quality; csrc/mesh_attr.hip) on the 256^3 marching-cubes mesh of the analytic capsule of scripts/mesh_simplify_time.py
(171k faces) with 100k surfels, on one GPU, in one process after warm-up.

    python scripts/mesh_attr_time.py [--resolution 256] [--surfels 100000] [--iters 10] [--out profiles/mesh_attr_time.json]

Every stage is timed with device events around the whole Python call (allocations, the calls' own read-backs and stream
synchronisations included: that is what a user waits for) and, next to it, a plain torch composition of the same stage on the same
device: chunked ``cdist`` + ``topk`` for the transfer, ``index_add_`` over the directed edges for the smoothing (every edge of a
closed mesh has two faces, so no border rule is needed -- ``border_vertices`` in the result is the number ``adjacency`` found, and
``smooth_max_diff_to_torch`` means something only where it is 0), boolean masks for the pruning.  The adjacency has no torch counterpart of
its own: the torch smoothing builds its edge list inside its time, as ``smooth`` builds its rows inside its own
(``smooth_steps_only_ms`` is the steps alone, through the C call).  The two sides are compared on the way: same neighbours, same
kept vertices, smoothed positions to 1e-5.  No bar is set.  The result is printed as one JSON line and written to ``--out``
(default ``profiles/mesh_attr_time.json`` of the repository)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from soar_amd import mesh  # noqa: E402
from mesh_simplify_time import analytic_field  # noqa: E402


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)


def torch_transfer(v, pts, col, k, chunk=4096):
    idx, d2 = [], []
    for i in range(0, v.shape[0], chunk):
        d = torch.cdist(v[i:i + chunk], pts).square()
        dk, ik = torch.topk(d, k, dim=1, largest=False)
        idx.append(ik)
        d2.append(dk[:, 0])
    idx = torch.cat(idx)
    return col[idx].mean(1).clamp(0, 1), torch.cat(d2), idx


def torch_smooth(v, faces, steps):
    f = faces.long()
    src = f[:, [0, 0, 1, 1, 2, 2]].reshape(-1)
    dst = f[:, [1, 2, 2, 0, 0, 1]].reshape(-1)
    n = torch.zeros(v.shape[0], device=v.device).index_add_(0, src, torch.ones(src.shape[0], device=v.device))
    for _ in range(steps):
        s = torch.zeros_like(v).index_add_(0, src, v[dst])
        v = torch.where(n[:, None] > 0, (v + s) / (n[:, None] + 1), v)
    return v


def torch_prune(v, faces, q, thresh):
    kv = ~(q > thresh)
    new = torch.cumsum(kv.int(), 0) - 1
    kf = kv[faces.long()].all(1)
    return v[kv], new[faces.long()[kf]].int(), kv.nonzero()[:, 0].int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--surfels", type=int, default=100_000)
    ap.add_argument("--k", type=int, default=mesh.ATTR_K)
    ap.add_argument("--steps", type=int, default=mesh.SMOOTH_STEPS)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_attr_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_attr_time.py needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    v, f = mesh.marching_cubes(analytic_field("capsule", args.resolution, dev))
    v = v / (args.resolution - 1)                                      # the unit cube
    m = mesh.Mesh(v, f)
    V, F = int(v.shape[0]), int(f.shape[0])
    gen = torch.Generator(device="cpu").manual_seed(0)
    # surfels: mesh vertices drawn at random, pushed off the surface by up to half a voxel, random colours
    pick = torch.randint(0, V, (args.surfels,), generator=gen).to(dev)
    pts = (v[pick] + (torch.rand(args.surfels, 3, generator=gen).to(dev) - 0.5) / args.resolution).contiguous()
    col = torch.rand(args.surfels, 3, generator=gen).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "resolution": args.resolution, "iters": args.iters, "vertices": V, "faces": F,
           "surfels": args.surfels, "k": args.k, "smooth_steps": args.steps}

    color, quality, idx = mesh.vertex_attributes(v, pts, col, args.k)
    tcolor, tq, tidx = torch_transfer(v, pts, col, args.k)
    res["transfer_same_neighbour_sets"] = float((idx.long().sort(1).values == tidx.sort(1).values).all(1).float().mean())
    res["transfer_max_color_diff"] = float((color - tcolor).abs().max())
    thresh = float(quality.median())
    pm, keep = mesh.prune_by_quality(m, quality, thresh)
    tv, tf, tkeep = torch_prune(v, f, quality, thresh)
    res["prune_equal"] = bool(torch.equal(pm.vertices, tv) and torch.equal(pm.faces, tf) and torch.equal(keep, tkeep))
    res["pruned_vertices"], res["pruned_faces"] = int(pm.vertices.shape[0]), int(pm.faces.shape[0])
    res["border_vertices"] = int(mesh.adjacency(m)[2].sum())            # the torch smoothing below has no border rule
    sm = mesh.smooth(m, args.steps)
    res["smooth_max_diff_to_torch"] = float((sm.vertices - torch_smooth(v, f, args.steps)).abs().max())
    res["smooth_bit_reproducible"] = bool(torch.equal(mesh.smooth(m, args.steps).vertices, sm.vertices))

    # the smoothing steps alone, over an adjacency built before (mesh.smooth builds it inside its time)
    import ctypes as C
    from soar_amd import hip_lib
    L = hip_lib.lib()
    row_start, nbr, border = mesh.adjacency(m)
    border8 = border.to(torch.uint8)
    nb = C.c_size_t(0)
    hip_lib.check(L.soar_mesh_smooth_bytes(V, C.byref(nb)), "soar_mesh_smooth_bytes")
    ws, out = mesh._workspace(nb.value, dev), torch.empty_like(v)

    def steps_only():
        hip_lib.check(L.soar_mesh_smooth(V, int(nbr.shape[0]), v.data_ptr(), row_start.data_ptr(), nbr.data_ptr(), border8.data_ptr(),
                                         args.steps, ws.data_ptr(), nb.value, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                      "soar_mesh_smooth")

    res["smooth_steps_only_ms"], res["smooth_steps_only_min_ms"] = timed(steps_only, args.iters)
    for name, hip, ref in (
            ("transfer", lambda: mesh.vertex_attributes(v, pts, col, args.k), lambda: torch_transfer(v, pts, col, args.k)),
            ("adjacency", lambda: mesh.adjacency(m), None),
            ("smooth", lambda: mesh.smooth(m, args.steps), lambda: torch_smooth(v, f, args.steps)),
            ("prune", lambda: mesh.prune_by_quality(m, quality, thresh), lambda: torch_prune(v, f, quality, thresh))):
        res[name + "_ms"], res[name + "_min_ms"] = timed(hip, args.iters)
        if ref is not None:
            res[name + "_torch_ms"], res[name + "_torch_min_ms"] = timed(ref, args.iters)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
