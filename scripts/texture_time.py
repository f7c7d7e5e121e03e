"""Time the texture atlas (soar_amd/texture.py: build_atlas, bake_texture; csrc/mesh_texture.hip) on the analytic capsule of
scripts/mesh_simplify_time.py (256^3 marching cubes) decimated to 100k faces, with 100k surfels, at texture sizes 2048 and 4096, on
one GPU, in one process after warm-up.

    python scripts/texture_time.py [--sizes 2048 4096] [--surfels 100000] [--iters 5] [--out profiles/texture_time.json]

Per size: ``build_atlas`` and ``bake_texture`` (default chunk), medians of repeated regions timed with device events around the
whole Python call (allocations, read-backs and stream synchronisations included: what a user waits for), and as the yardstick
``vertex_attributes`` on the very points the bake queries (the owned texels' positions, in one call): the floor the grid search
sets, since the bake runs that search and transfer chunk by chunk.  ``bake_over_vertex_attributes`` is their ratio.  Those points
are in image (row-major) order; ``vertex_attributes_face_order_ms`` is the same call on the same points face after face, the order
the bake queries them in, so the two ratios separate the order of the queries from the chunking.  No bar is set."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

from soar_amd import mesh  # noqa: E402
from mesh_attr_time import timed  # noqa: E402
from mesh_simplify_time import analytic_field  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--target", type=int, default=mesh.DECIMATE_TARGET)
    ap.add_argument("--surfels", type=int, default=100_000)
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 4096])
    ap.add_argument("--k", type=int, default=mesh.ATTR_K)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("texture_time.py needs a GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    v, f = mesh.marching_cubes(analytic_field("capsule", args.resolution, dev))
    m = mesh.decimate(mesh.Mesh(v / (args.resolution - 1), f), args.target)           # the unit cube
    V, F = int(m.vertices.shape[0]), int(m.faces.shape[0])
    gen = torch.Generator(device="cpu").manual_seed(0)
    # surfels: mesh vertices drawn at random, pushed off the surface by up to half a voxel, random colours
    pick = torch.randint(0, V, (args.surfels,), generator=gen).to(dev)
    pts = (m.vertices[pick] + (torch.rand(args.surfels, 3, generator=gen).to(dev) - 0.5) / args.resolution).contiguous()
    col = torch.rand(args.surfels, 3, generator=gen).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "resolution": args.resolution, "iters": args.iters, "vertices": V, "faces": F,
           "surfels": args.surfels, "k": args.k, "sizes": {}}
    for T in args.sizes:
        atlas = mesh.build_atlas(m, T)
        tex, dbg = mesh.bake_texture(m, atlas, pts, col, args.k, return_debug=True)
        owned = dbg["owner"] >= 0
        queries = dbg["position"][owned].contiguous()
        want, _, _ = mesh.vertex_attributes(queries, pts, col, args.k)
        r = {"scale_step": atlas.scale_step, "sides": sorted(set(atlas.cell[:, 2].tolist())), "owned_texels": int(owned.sum()),
             "owned_share": float(owned.float().mean()),
             "colours_equal_vertex_attributes": bool(torch.equal(dbg["color"][owned], want)),
             "bit_reproducible": bool(torch.equal(mesh.bake_texture(m, atlas, pts, col, args.k), tex))}
        # the same points face after face (stable by owner: image order inside a face), close to the order the bake queries them in
        by_face = queries[torch.argsort(dbg["owner"][owned], stable=True)].contiguous()
        del dbg, owned, want
        r["build_atlas_ms"], r["build_atlas_min_ms"] = timed(lambda: mesh.build_atlas(m, T), args.iters)
        r["bake_texture_ms"], r["bake_texture_min_ms"] = timed(lambda: mesh.bake_texture(m, atlas, pts, col, args.k), args.iters)
        r["vertex_attributes_ms"], r["vertex_attributes_min_ms"] = timed(lambda: mesh.vertex_attributes(queries, pts, col, args.k), args.iters)
        r["bake_over_vertex_attributes"] = r["bake_texture_ms"] / r["vertex_attributes_ms"]
        r["vertex_attributes_face_order_ms"], r["vertex_attributes_face_order_min_ms"] = timed(
            lambda: mesh.vertex_attributes(by_face, pts, col, args.k), args.iters)
        r["bake_over_vertex_attributes_face_order"] = r["bake_texture_ms"] / r["vertex_attributes_face_order_ms"]
        res["sizes"][str(T)] = r
        del queries, by_face, tex
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
