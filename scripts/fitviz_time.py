"""Time the SMPLify fit inspection (soar_amd/fitviz.py, csrc/fitviz.hip) on one GPU, in one process after warm-up.

    python scripts/fitviz_time.py [--frames 64] [--baseline-frames 8] [--iters 5] [--out profiles/fitviz_time.json]

The workload: ``--frames`` frames of 1080 x 1920, the 10 475-vertex synthetic body of scripts/smplify_time.py with the faces of
scripts/prior_time.py, K = 137 keypoints, photographs of random bytes.

* ``fit_strips`` as a whole (keypoints, vertices, yaw views, the renderer on three bodies a frame, the strips, the residuals), in
  chunks of 4 frames: wall time per call between two synchronisations, median of ``--iters``.
* ``draw_strips`` alone on one chunk's images: microseconds per call between two device events, and the bytes it reads and writes
  per second (13 bytes of normal image and mask per pixel of panels 2 - 4 and again for panel 1, 3 bytes of photograph for panels 0
  and 1, 15 bytes of strip written).
* the baseline: the same strips with the image stage on the host -- the same device calls up to the renderer, the float normal
  images and masks copied to the host, then the NumPy restatement of tests/fitviz_ref.py -- on the first
  ``--baseline-frames`` frames, one frame at a time; the bytes must equal ``fit_strips``'.
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import fitviz_ref as fr  # noqa: E402
import prior_time  # noqa: E402
import smplify_time  # noqa: E402
from soar_amd import fitviz, prior  # noqa: E402
from soar_amd import smplify as S  # noqa: E402
from soar_amd.body import smplx_vertices  # noqa: E402

W, H = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--baseline-frames", type=int, default=8)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N = args.frames
    m, tables = smplify_time.make_model(dev)
    rig = S.KeypointRig.from_body_model(m, *tables, device=dev)
    topo = prior.MeshTopology(prior_time.make_faces(m.v_template), m.v_template.shape[0], device=dev)
    start, _, Ks, w2c, img_wh, target = smplify_time.make_inputs(m, tables, N, dev)
    assert tuple(img_wh) == (W, H)
    params = {k: v.to(dev) for k, v in start.items()}
    params["betas"] = params["betas"][:1]
    imgs = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(9)).to(dev)
    call = lambda: fitviz.fit_strips(rig, m, topo, params, Ks, w2c, img_wh, target, imgs=imgs, chunk=args.chunk)

    out = call()
    torch.cuda.synchronize()
    res = {"device": torch.cuda.get_device_name(0), "frames": N, "image_wh": [W, H], "V": topo.num_verts, "F": topo.num_faces, "K": 137,
           "chunk": args.chunk, "strip_bytes_per_frame": int(out["strips"][0].numel()),
           "mean_residual_px": float(out["residuals"][:, 1].mean())}

    # the pieces of one chunk, for draw_strips alone
    c = args.chunk
    six = fitviz._six_d({k: (v if k == "betas" else v[:c]) for k, v in params.items()})
    fit_px = S.project_keypoints(rig, six, Ks[:c], w2c)
    target_px = (target[:c, :, :2] * torch.tensor([float(W), float(H)], device=dev)).contiguous()
    coef = torch.cat([params["betas"].expand(c, -1), params["expression"][:c]], 1)
    pose = prior.full_pose({k: v[:c] if k != "betas" else v for k, v in params.items()})
    verts = smplx_vertices(m, coef, pose, params["transl"][:c])
    pelvis = rig.J_template[0] + torch.einsum("kl,nl->nk", rig.J_dirs[0], coef) + params["transl"][:c]
    views = fitviz.yaw_views(verts, pelvis, w2c, 3)
    pr = prior.render_normal_priors(topo, views.reshape(3 * c, -1, 3), w2c, Ks[:c].repeat_interleave(3, dim=0), (W, H))
    draw = lambda: fitviz.draw_strips(target_px, fit_px, rig.kp_mask, pr["prior"], pr["mask"], imgs[:c])

    gc.collect()
    gc.freeze()
    walls = []
    for _ in range(args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    res["fit_strips_s"], res["fit_strips_min_s"] = statistics.median(walls), min(walls)
    res["fit_strips_ms_per_frame"] = res["fit_strips_s"] * 1e3 / N
    med, lo = prior_time.median_us(draw, 20, 5)
    moved = c * H * W * (4 * 13 + 2 * 3 + 15)
    res.update(draw_strips_us=med, draw_strips_min_us=lo, draw_strips_frames=c, draw_strips_bytes=moved,
               draw_strips_GB_per_s=moved / med * 1e-3)

    # the baseline: the parent's device calls, the float images on the host, NumPy
    nb = min(args.baseline_frames, N)
    mask_host = rig.kp_mask.cpu().numpy()
    walls = []
    for n in range(nb):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        one = {k: (v if k == "betas" else v[n:n + 1]) for k, v in params.items()}
        f_px = S.project_keypoints(rig, fitviz._six_d(one), Ks[n:n + 1], w2c)
        cf = torch.cat([params["betas"], params["expression"][n:n + 1]], 1)
        vs = smplx_vertices(m, cf, prior.full_pose(one), params["transl"][n:n + 1])
        pv = rig.J_template[0] + torch.einsum("kl,nl->nk", rig.J_dirs[0], cf) + params["transl"][n:n + 1]
        turned = fitviz.yaw_views(vs, pv, w2c, 3)[0]
        p = prior.render_normal_priors(topo, turned, w2c, Ks[n:n + 1].expand(3, 3, 3), (W, H))
        t_px = (target[n:n + 1, :, :2] * torch.tensor([float(W), float(H)], device=dev))
        strip = fr.strips(t_px.cpu().numpy(), f_px.cpu().numpy(), mask_host, p["prior"].cpu().numpy()[None], p["mask"].cpu().numpy()[None],
                          imgs=imgs[n:n + 1].cpu().numpy())
        walls.append(time.perf_counter() - t0)
        assert np.array_equal(strip[0], out["strips"][n].cpu().numpy()), f"frame {n}: the baseline's bytes differ"
    res.update(baseline_frames=nb, baseline_s_per_frame=statistics.median(walls), baseline_equal_bytes=True,
               speedup_per_frame=statistics.median(walls) / (res["fit_strips_s"] / N))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
