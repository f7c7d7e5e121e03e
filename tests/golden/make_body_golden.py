"""Generate ``smplx_vertices.npz`` by RUNNING the reference's own ``lbs()`` where the reference tree is present.

Run once:  ``python tests/golden/make_body_golden.py <path to soar/threestudio-soar>``.  Only inputs and outputs (data) are written; no reference source is copied.

``lbs()`` of the vendored SMPL-X (soar/threestudio-soar/utils/smplx/lbs.py:147-246) on a seeded SMPL-X-shaped model (V = 96,
J = 55, NB = 20, B = 4) with NON-ZERO pose correctives, once in float32 and once in float64 on the same (float32) inputs, each
followed by ``+ transl`` (body_models.py).  ``posedirs = U @ Wt`` has rank 8 and is stored as its two factors
(``tests/body_ref.posedirs_from_factors`` rebuilds it bit for bit).  Poses: random, the rest pose, a near-pi root rotation.
"""
import math
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(OUT, "..", ".."), os.path.join(OUT, "..")]


def main(ref):
    sys.path.insert(0, os.path.join(ref, "utils"))
    import smplx.lbs as ref_lbs                                    # the vendored SMPL-X lbs module
    import body_ref
    from soar_amd import synthetic as syn

    g = torch.Generator().manual_seed(4321)
    V, J, NB, B, RANK = 96, 55, 20, 4, 8
    v_template, _ = syn.sample_capsule_surface(V, g)
    shapedirs = torch.randn(V, 3, NB, generator=g) * 5e-3
    U = torch.randn((J - 1) * 9, RANK, generator=g) * 0.1
    Wt = torch.randn(RANK, V * 3, generator=g) * 0.05
    posedirs = torch.from_numpy(body_ref.posedirs_from_factors(U.numpy(), Wt.numpy()))
    jr = torch.rand(J, V, generator=g) ** 8
    J_regressor = jr / jr.sum(1, keepdim=True)
    parents = torch.tensor(syn.SMPLX_PARENTS)
    lbs_weights = torch.softmax(2.0 * torch.randn(V, J, generator=g), dim=1)
    betas = torch.randn(B, NB, generator=g) * 0.7
    pose = torch.randn(B, J * 3, generator=g) * 0.4
    pose[1] = 0.0                                                   # rest pose: exercises |v + 1e-8|
    pose[2, :3] = torch.tensor([0.0, math.pi - 1e-3, 0.0])          # near-pi rotation of the root
    transl = torch.randn(B, 3, generator=g)
    out = {}
    with torch.no_grad():
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            c = lambda t: t.to(dt)
            verts, _ = ref_lbs.lbs(c(betas), c(pose), c(v_template)[None].expand(B, -1, -1), c(shapedirs), c(posedirs),
                                   c(J_regressor), parents, c(lbs_weights), pose2rot=True)
            out[f"verts_{name}"] = (verts + c(transl).unsqueeze(1)).numpy()
    np.savez_compressed(os.path.join(OUT, "smplx_vertices.npz"), v_template=v_template.numpy(), shapedirs=shapedirs.numpy(),
                        posedirs_U=U.numpy(), posedirs_Wt=Wt.numpy(), J_regressor=J_regressor.numpy(), parents=parents.numpy(),
                        lbs_weights=lbs_weights.numpy(), betas=betas.numpy(), pose=pose.numpy(), transl=transl.numpy(), **out)
    print("wrote smplx_vertices.npz", {k: (v.shape, v.dtype) for k, v in out.items()},
          "posedirs max", float(posedirs.abs().max()), "f32 vs f64 worst", float(np.abs(out["verts_f32"] - out["verts_f64"]).max()))


if __name__ == "__main__":
    main(sys.argv[1])
