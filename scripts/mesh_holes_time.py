"""Time the hole closing (soar_amd/mesh.py: close_holes; csrc/mesh_holes.hip) on the 256^3 marching-cubes mesh of the analytic
capsule of scripts/mesh_simplify_time.py (171k faces) from which a fixed-seed set of vertex rings has been pruned, on one GPU, in
one process after warm-up.

    python scripts/mesh_holes_time.py [--resolution 256] [--rings 2000] [--radius 2] [--iters 10] [--out profiles/mesh_holes_time.json]

``--rings`` vertices are drawn with a fixed seed; they and everything within ``--radius`` edges of them get quality 1, the rest 0,
and ``prune_by_quality`` at 0.5 cuts them out: holes of a few dozen edges, some of them merged where two rings met.  ``close_holes``
is timed with device events around the whole Python call (the allocations, the call's read-back and stream synchronisation
included: that is what a user waits for), next to the NumPy restatement of the same definition on the host
(tests/mesh_holes_ref.py, plain Python loops, once; the download of the mesh is not in its time).  The two results are compared bit
for bit on the way.  No bar is set.  The result is printed as one JSON line and written to ``--out``."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from soar_amd import mesh  # noqa: E402
from mesh_simplify_time import analytic_field  # noqa: E402
import mesh_holes_ref as H  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--rings", type=int, default=2000)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--max-hole-edges", type=int, default=mesh.MAX_HOLE_EDGES)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_holes_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_holes_time.py needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    v, f = mesh.marching_cubes(analytic_field("capsule", args.resolution, dev))
    v = v / (args.resolution - 1)                                      # the unit cube
    whole = mesh.Mesh(v, f)
    V = int(v.shape[0])
    gen = torch.Generator(device="cpu").manual_seed(0)
    q = torch.zeros(V, device=dev)
    q[torch.randperm(V, generator=gen)[:args.rings].to(dev)] = 1.0
    src, dst = f.long()[:, [0, 1, 2]].reshape(-1), f.long()[:, [1, 2, 0]].reshape(-1)
    for _ in range(args.radius):                                       # grow the marked set by one edge
        grown = q.clone()
        grown.index_put_((dst,), q[src], accumulate=True)
        grown.index_put_((src,), q[dst], accumulate=True)
        q = (grown > 0).float()
    m, _ = mesh.prune_by_quality(whole, q, 0.5)
    res = {"device": torch.cuda.get_device_name(0), "resolution": args.resolution, "iters": args.iters, "rings": args.rings,
           "radius": args.radius, "max_hole_edges": args.max_hole_edges, "whole_vertices": V, "whole_faces": int(f.shape[0]),
           "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0]), "border_edges": mesh.open_border_edges(m)}

    got, closed = mesh.close_holes(m, args.max_hole_edges)
    hv, hf = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    t0 = time.perf_counter()
    want = H.close_holes(hv, hf, args.max_hole_edges)
    res["numpy_host_ms"] = 1e3 * (time.perf_counter() - t0)
    res["loops_closed"], res["longest_loop_closed"] = int(closed.numel()), int(closed.max()) if closed.numel() else 0
    res["border_edges_left"] = mesh.open_border_edges(got)
    res["equal_to_numpy_bit_for_bit"] = bool(
        got.faces.shape == want.faces.shape and (got.faces.cpu().numpy() == want.faces).all()
        and got.vertices.shape == want.verts.shape and (got.vertices.cpu().numpy().view("u4") == want.verts.view("u4")).all()
        and (closed.cpu().numpy() == want.closed).all() and res["border_edges_left"] == want.open_left)
    res["close_holes_ms"], res["close_holes_min_ms"] = timed(lambda: mesh.close_holes(m, args.max_hole_edges), args.iters)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
