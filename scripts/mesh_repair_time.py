"""Time the repair of non-manifold edges and vertices (soar_amd/mesh.py: repair_manifold, manifold_report; csrc/mesh_repair.hip)
on the clustered two-sheet case at about 100k faces, on one GPU, in one process after warm-up.

    python scripts/mesh_repair_time.py [--level 7] [--inner 0.99] [--rough 0.002] [--target 100000] [--iters 10]
                                       [--out profiles/mesh_repair_time.json]

Two nested rough icospheres of ``--level`` (328k faces each at 7), the inner one scaled by ``--inner``, are decimated together to
``--target`` faces: where both sheets pass through one cell of the clustering the result has edges with more than two faces.
``repair_manifold`` (the counting call, the allocation of the outputs, the full call, both read-backs and synchronisations: what a
user waits for) and ``manifold_report`` (the counting call alone) are timed with device events around the whole Python call, next
to the NumPy restatement of the same definition on the host (tests/mesh_repair_ref.py, plain Python loops, once; the download of
the mesh is not in its time).  The two results are compared bit for bit on the way.  No bar is set.  The result is printed as one
JSON line and written to ``--out``."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "tests")]

from soar_amd import mesh  # noqa: E402
from mesh_holes_time import timed  # noqa: E402
import mesh_repair_ref as R  # noqa: E402
import mesh_simplify_ref as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=7)
    ap.add_argument("--inner", type=float, default=0.99)
    ap.add_argument("--rough", type=float, default=0.002)
    ap.add_argument("--target", type=int, default=mesh.DECIMATE_TARGET)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_repair_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("mesh_repair_time.py needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    v0, f0 = S.icosphere(args.level, seed=1, rough=args.rough)
    v1, f1 = S.icosphere(args.level, seed=2, rough=args.rough, scale=args.inner)
    whole = mesh.Mesh(torch.from_numpy(np.concatenate([v0, v1])).to(dev), torch.from_numpy(np.concatenate([f0, f1 + len(v0)])).to(dev))
    m = mesh.decimate(whole, args.target)
    res = {"device": torch.cuda.get_device_name(0), "level": args.level, "inner": args.inner, "rough": args.rough, "target": args.target,
           "iters": args.iters, "whole_vertices": int(whole.vertices.shape[0]), "whole_faces": int(whole.faces.shape[0]),
           "vertices": int(m.vertices.shape[0]), "faces": int(m.faces.shape[0])}

    got, source, info = mesh.repair_manifold(m)
    res["report"] = info
    hv, hf = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
    t0 = time.perf_counter()
    want = R.repair(hv, hf)
    res["numpy_host_ms"] = 1e3 * (time.perf_counter() - t0)
    res["equal_to_numpy_bit_for_bit"] = bool(
        tuple(info.values()) == want.counts and got.faces.shape == want.faces.shape and (got.faces.cpu().numpy() == want.faces).all()
        and got.vertices.shape == want.verts.shape and (got.vertices.cpu().numpy().view("u4") == want.verts.view("u4")).all()
        and (source.cpu().numpy() == want.source).all())
    res["report_after"] = mesh.manifold_report(got)
    res["repair_manifold_ms"], res["repair_manifold_min_ms"] = timed(lambda: mesh.repair_manifold(m), args.iters)
    res["manifold_report_ms"], res["manifold_report_min_ms"] = timed(lambda: mesh.manifold_report(m), args.iters)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
