"""Time the three launches of the normal priors (soar_amd/prior.py, csrc/prior.hip) on one GPU, in one process after warm-up.

    python scripts/prior_time.py [--iters 20] [--reps 5] [--frames 1 4 64] [--out profiles/prior_time.json]

The body is ``synthetic.make_body_model()`` (V = 10 475, the one scripts/smplify_time.py builds) posed by
``synthetic.make_pose_sequence``.  It is a point sample of a surface and has no faces, so 20 908 are made here: every vertex
joins its 1st and 2nd, and its 3rd and 4th, nearest neighbours in the rest pose (the first 20 908 of these) -- triangles of the
right number and size that overlap like a sheet, not a closed manifold.  The camera puts the body into a 512 x 512 crop as
``crop_frames`` would (1.1 x its longer side).  The script reports the mean snapped area of the faces in pixels and the covered
share of the image next to the times.

A timed region is ``reps`` calls of one C entry point between two device events; the figure is the median over ``iters`` regions
divided by ``reps``.  There is no other renderer to compare with: the times stand next to the networks' own from
profiles/normals_time.json (both generators, one call), with each launch's share of the stage's time without the crop and the bytes = networks + the
three launches."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from soar_amd import hip_lib, prior  # noqa: E402
from soar_amd import synthetic as syn  # noqa: E402
from soar_amd.body import smplx_vertices  # noqa: E402

N_FACES = 20908
SIDE = 512


def region(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps           # microseconds per call


def median_us(fn, iters, reps, warmup=3):
    for _ in range(warmup):
        region(fn, reps)
    ts = [region(fn, reps) for _ in range(iters)]
    return statistics.median(ts), min(ts)


def make_faces(v_template):
    v = v_template.cuda()
    nn = torch.empty((v.shape[0], 4), dtype=torch.int64, device="cuda")
    for i in range(0, v.shape[0], 2048):                                 # k nearest neighbours, in blocks (set-up code)
        d = torch.cdist(v[i:i + 2048], v)
        nn[i:i + 2048] = d.topk(5, dim=1, largest=False).indices[:, 1:]
    me = torch.arange(v.shape[0], device="cuda")
    faces = torch.stack([torch.stack([me, nn[:, 0], nn[:, 1]], 1), torch.stack([me, nn[:, 2], nn[:, 3]], 1)], 1).reshape(-1, 3)
    return faces[:N_FACES].cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 4, 64])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    body = syn.make_body_model(0)
    topo = prior.MeshTopology(make_faces(body.v_template), body.v_template.shape[0], device=dev)
    V, F = topo.num_verts, topo.num_faces
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.0, 0.1, 3.5])
    w2c = w2c.to(dev)
    with open(os.path.join(ROOT, "profiles", "normals_time.json")) as fh:
        nets = {int(k.strip("[]").split(",")[0]): v["hip"] for k, v in json.load(fh)["shapes"].items()}
    res = {"device": torch.cuda.get_device_name(0), "V": V, "F": F, "image": [SIDE, SIDE], "reps_per_region": args.reps, "regions": args.iters,
           "unit": "us per launch (median, min)", "networks_ms_per_call": nets, "library": os.path.basename(hip_lib.LIB_PATH)}
    L = hip_lib.lib()
    for N in args.frames:
        seq = syn.make_pose_sequence(N, 0)
        verts = smplx_vertices(body, torch.cat([seq["betas"].expand(N, -1), seq["expression"]], 1).to(dev), seq["full_pose"].to(dev),
                               seq["transl"].to(dev))
        # the crop's camera: the body's box x 1.1 fills the image
        cam = verts @ w2c[:3, :3].T + w2c[:3, 3]
        uv = cam[..., :2] / cam[..., 2:]
        lo, hi = uv.amin(1), uv.amax(1)
        f = SIDE / (1.1 * (hi - lo).amax(1))
        c = SIDE / 2 - f[:, None] * (lo + hi) / 2
        Ks = torch.zeros((N, 3, 3), device=dev)
        Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2], Ks[:, 2, 2] = f, f, c[:, 0], c[:, 1], 1.0
        out = prior.render_normal_priors(topo, verts, w2c, Ks, (SIDE, SIDE), debug=True)
        sn = out["snapped"][0].double() / 256
        tri = sn[topo.faces.long()]
        area = 0.5 * ((tri[:, 1, 0] - tri[:, 0, 0]) * (tri[:, 2, 1] - tri[:, 0, 1]) - (tri[:, 1, 1] - tri[:, 0, 1]) * (tri[:, 2, 0] - tri[:, 0, 0])).abs()
        s = torch.cuda.current_stream(dev).cuda_stream
        st = (C.c_int64 * 3)(*verts.stride())
        o = out

        def setup():
            hip_lib.check(L.soar_prior_vertex_setup(N, V, F, verts.data_ptr(), st, w2c.data_ptr(), 0, Ks.data_ptr(), topo.faces.data_ptr(),
                                                    topo.csr_offsets.data_ptr(), topo.csr_corners.data_ptr(), o["snapped"].data_ptr(),
                                                    o["inv_z"].data_ptr(), o["vertex_normals"].data_ptr(), s), "soar_prior_vertex_setup")

        def boxes():
            hip_lib.check(L.soar_prior_face_boxes(N, V, F, topo.faces.data_ptr(), o["snapped"].data_ptr(), o["face_boxes"].data_ptr(), s),
                          "soar_prior_face_boxes")

        def raster():
            hip_lib.check(L.soar_prior_raster(N, V, F, SIDE, SIDE, 1, topo.faces.data_ptr(), o["snapped"].data_ptr(), o["inv_z"].data_ptr(),
                                              o["vertex_normals"].data_ptr(), o["face_boxes"].data_ptr(), o["prior"].data_ptr(),
                                              o["mask"].data_ptr(), o["face"].data_ptr(), s), "soar_prior_raster")

        t_setup, t_boxes, t_raster = (median_us(fn, args.iters, args.reps) for fn in (setup, boxes, raster))
        t_both = median_us(lambda: prior.render_normal_priors(topo, verts, w2c, Ks, (SIDE, SIDE)), args.iters, args.reps)
        r = {"vertex_setup_us": t_setup[0], "vertex_setup_min_us": t_setup[1], "face_boxes_us": t_boxes[0], "face_boxes_min_us": t_boxes[1], "raster_us": t_raster[0], "raster_min_us": t_raster[1],
             "render_normal_priors_us": t_both[0], "raster_us_per_frame": t_raster[0] / N,
             "mean_face_area_px": float(area.mean()), "covered_share": float(out["mask"][:, 0].float().mean()),
             "faces_with_a_sample_share": float((out["face_boxes"][..., 0] <= out["face_boxes"][..., 1]).float().mean())}
        if N in nets:
            stage = nets[N] * 1e3 + t_setup[0] + t_boxes[0] + t_raster[0]
            r.update(networks_us=nets[N] * 1e3, vertex_setup_share_of_stage=t_setup[0] / stage, face_boxes_share_of_stage=t_boxes[0] / stage, raster_share_of_stage=t_raster[0] / stage,
                     raster_over_networks=t_raster[0] / (nets[N] * 1e3))
        res[f"N{N}"] = r
        print(json.dumps({f"N{N}": r}), flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
