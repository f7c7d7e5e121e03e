"""GPU tests of the geometry model (soar_amd/geometry.py, csrc/geometry.hip): the two per-surfel passes against the float64
restatement (tests/geometry_ref.py) with bars derived from torch's own float32 distance on the same inputs, bitwise reproducibility,
the renderer plugin on the model against the duck-typed stub, the one-launch Adam against torch.optim.Adam, densification against
``SurfelDensifier`` driven by hand, checkpoints, and a 30-step end-to-end run."""
import math
import types

import numpy as np
import pytest
import torch
from torch import nn

import geometry_ref as gr
from soar_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SIZES = (1, 63, 64, 65, 100003)
FLOOR, TORCH_CAP = 1e-6, 1e-4


def bar_check(name, hip, f32, f64, report):
    """The bar of HIP: 4 x the distance of torch-float32 from float64 on the same inputs, never below 1e-6 (relative L2; the worst
    element over the largest magnitude likewise); torch-float32 itself is capped at 1e-4 so that a broken restatement fails."""
    d_hip, d_t = gr.rel_l2(hip, f64), gr.rel_l2(f32, f64)
    w_hip, w_t = gr.worst(hip, f64), gr.worst(f32, f64)
    report.append(f"{name}: rel-L2 hip {d_hip:.3e} torch {d_t:.3e} | worst hip {w_hip:.3e} torch {w_t:.3e}")
    print(report[-1])
    assert d_t <= TORCH_CAP and w_t <= TORCH_CAP, (name, d_t, w_t)
    assert d_hip <= max(4 * d_t, FLOOR), (name, d_hip, d_t)
    assert w_hip <= max(4 * w_t, FLOOR), (name, w_hip, w_t)


def leaves(P, S, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    rot, sc, op, occ, col = r(P, 4), r(P, S) * 3, r(P, 1) * 3, r(P, 1) * 3, r(P, 3) * 3
    # the corners: a zero quaternion (the 1e-12 floor), a tiny one below the floor, |opacity logit| of 30, scaling logits of +-20
    rot[0] = 0
    if P > 3:
        rot[1] = torch.tensor([3e-13, 0, -2e-13, 1e-13])
        op[2], op[3] = 30.0, -30.0
        occ[2], col[3] = -30.0, 30.0
        sc[2], sc[3] = 20.0, -20.0
    return [t.to(DEV) for t in (rot, sc, op, occ, col)]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("P", SIZES)
def test_activations_and_gradients_against_float64(P, S):
    from soar_amd.geometry import surfel_activations
    raw = leaves(P, S, seed=P + S)
    g = torch.Generator().manual_seed(7)
    ups = [torch.randn(t.shape, generator=g).to(DEV) for t in raw]
    res = {}
    for kind in ("hip", "f32", "f64"):
        dt = torch.float64 if kind == "f64" else torch.float32
        ins = [t.detach().to(dt).requires_grad_(True) for t in raw]
        outs = surfel_activations(*ins) if kind == "hip" else gr.activations(*ins)
        sum((o * u.to(dt)).sum() for o, u in zip(outs, ups)).backward()
        res[kind] = ([o.detach() for o in outs], [t.grad for t in ins])
    report = []
    names = ("rotation", "scaling", "opacity", "occ", "colors")
    for k, n in enumerate(names):
        bar_check(f"P={P} S={S} {n}", res["hip"][0][k], res["f32"][0][k], res["f64"][0][k], report)
        bar_check(f"P={P} S={S} d{n}", res["hip"][1][k], res["f32"][1][k], res["f64"][1][k], report)
    # the floor: a zero quaternion stays zero and passes its gradient through 1 / eps, as F.normalize does
    assert torch.equal(res["hip"][0][0][0], torch.zeros(4, device=DEV))
    assert torch.equal(res["hip"][1][0][0], res["f32"][1][0][0])
    # an output nobody uses costs nothing and yields None; partial use works
    ins = [t.detach().clone().requires_grad_(True) for t in raw]
    outs = surfel_activations(*ins)
    (outs[2].sum() + outs[0].sum()).backward()
    assert ins[1].grad is None and ins[3].grad is None and ins[4].grad is None and ins[2].grad is not None


def reg_inputs(P, S, K, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    xyz, pos = r(P, 3), None
    pos = xyz + r(P, 3) * 0.01
    lo, hi = P // 4, max(P // 2, 1)
    pos[lo:hi] = xyz[lo:hi]                                  # rows that have not moved: clones, and every row at initialisation
    if P > 8:
        xyz[5] = 0
    scaling, opacity, scales = torch.exp(r(P, S)), torch.sigmoid(r(P, 1) * 2), torch.sigmoid(r(P, K)) * 2e-2
    return [t.to(DEV) for t in (xyz, pos, scaling, opacity, scales)], (lo, hi)


ALL = {"lambda_position": 0.3, "lambda_delta": 1.0, "lambda_opacity": 0.02, "lambda_sparsity": 0.7, "lambda_scales": 0.1}


@pytest.mark.parametrize("S,K", [(1, 1), (3, 3), (3, 1)])
@pytest.mark.parametrize("P", SIZES)
def test_regularizers_and_gradients_against_float64(P, S, K):
    from soar_amd.geometry import LAMBDAS, surfel_regularizers
    raw, (lo, hi) = reg_inputs(P, S, K, seed=P + S + K)
    report = []
    for lambdas in [{k: ALL[k]} for k in LAMBDAS] + [ALL]:
        res = {}
        for kind in ("hip", "f32", "f64"):
            dt = torch.float64 if kind == "f64" else torch.float32
            ins = [t.detach().to(dt) for t in raw]
            for k in (0, 2, 3, 4):
                ins[k].requires_grad_(True)
            loss, terms = (surfel_regularizers(*ins, lambdas) if kind == "hip" else gr.regularizers(*ins, lambdas))
            (loss * 1.7).backward()
            res[kind] = (loss.detach(), torch.stack([t for t in terms]) if kind != "hip" else terms, [ins[k].grad for k in (0, 2, 3, 4)])
        tag = f"P={P} S={S} K={K} {'+'.join(k[7:] for k in lambdas)}"
        bar_check(tag + " loss", res["hip"][0], res["f32"][0], res["f64"][0], report)
        bar_check(tag + " terms", res["hip"][1], res["f32"][1], res["f64"][1], report)
        for k, n in zip((0, 2, 3), ("dxyz", "dopacity", "dscales")):
            a, b, c = res["hip"][2][k], res["f32"][2][k], res["f64"][2][k]
            if c is None or float(c.abs().max()) == 0.0:
                assert a is None or float(a.abs().max()) == 0.0, (tag, n)           # a term that is off contributes no gradient
                continue
            bar_check(f"{tag} {n}", a, b, c, report)
        assert res["hip"][2][1] is None or float(res["hip"][2][1].abs().max()) == 0.0          # scaling: detached in the opacity term
        for k, name in enumerate(LAMBDAS):                                                 # a term that is off is reported as 0
            if name not in lambdas:
                assert float(res["hip"][1][k]) == 0.0
        if "lambda_delta" in lambdas and len(lambdas) == 1 and hi > lo and P > 1:
            assert float(res["hip"][2][0][lo:hi].abs().max()) == 0.0                         # exactly zero where xyz == original_pos
            assert res["hip"][2][0].abs().max() > 0 or P < 4


def test_regularizers_upstream_scalar_and_missing_weights():
    from soar_amd.geometry import surfel_regularizers
    raw, _ = reg_inputs(5000, 1, 1, seed=2)
    outs = []
    for scale in (None, 0.25, torch.tensor(0.25, device=DEV)):
        ins = [t.detach().clone() for t in raw]
        ins[0].requires_grad_(True)
        ins[3].requires_grad_(True)
        loss, terms = surfel_regularizers(*ins, {"lambda_delta": 1.0, "lambda_sparsity": 0.5, "lambda_position": 0.0}, grad_scale=scale)
        loss.backward()
        outs.append((loss.detach(), ins[0].grad, ins[3].grad))
        assert float(terms[0]) == 0.0 and float(terms[4]) == 0.0
    assert torch.equal(outs[1][1], outs[2][1]) and torch.equal(outs[0][0], outs[1][0])
    torch.testing.assert_close(outs[1][1], outs[0][1] * 0.25, rtol=2e-7, atol=0)
    torch.testing.assert_close(outs[1][2], outs[0][2] * 0.25, rtol=2e-7, atol=0)


def test_regularizers_backward_twice_and_cache_follows_in_place_writes(world):
    from soar_amd.geometry import surfel_regularizers
    raw, _ = reg_inputs(3000, 1, 1, seed=9)
    ins = [t.detach().clone() for t in raw]
    ins[0].requires_grad_(True)
    loss, _ = surfel_regularizers(*ins, {"lambda_delta": 1.0, "lambda_position": 0.5})
    (loss * 3.0).backward(retain_graph=True)
    first = ins[0].grad.clone()
    ins[0].grad = None
    (loss * 3.0).backward()
    assert torch.equal(first, ins[0].grad)                   # the precomputed gradients are not scaled in place
    m = make_model(world, P=500, seed=5)
    a = m.get_opacity
    assert m.get_opacity is a
    with torch.no_grad():
        m._opacity.fill_(1.5)                                # an in-place write: no invalidate() needed
    assert m.get_opacity is not a and torch.equal(m.get_opacity.detach(), torch.sigmoid(m._opacity.detach()).clone()) or \
        gr.rel_l2(m.get_opacity, torch.sigmoid(m._opacity.detach())) < 1e-6


def test_bitwise_reproducible_split_invariant_and_graph_replay():
    from soar_amd.geometry import surfel_activations, surfel_regularizers
    P = 100003
    raw = leaves(P, 3, seed=5)
    a, b = surfel_activations(*raw), surfel_activations(*raw)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    h = P // 2
    lo, hi = surfel_activations(*[t[:h].contiguous() for t in raw]), surfel_activations(*[t[h:].contiguous() for t in raw])
    for x, l, u in zip(a, lo, hi):
        assert torch.equal(x, torch.cat([l, u]))
    # ... and the gradients of the elementwise pass
    def grads(ts, ups):
        ins = [t.detach().clone().requires_grad_(True) for t in ts]
        sum((o * u).sum() for o, u in zip(surfel_activations(*ins), ups)).backward()
        return [t.grad for t in ins]
    g = torch.Generator().manual_seed(1)
    ups = [torch.randn(t.shape, generator=g).to(DEV) for t in raw]
    full = grads(raw, ups)
    parts = (grads([t[:h].contiguous() for t in raw], [u[:h].contiguous() for u in ups]), grads([t[h:].contiguous() for t in raw], [u[h:].contiguous() for u in ups]))
    for x, l, u in zip(full, *parts):
        assert torch.equal(x, torch.cat([l, u]))
    for x, y in zip(full, grads(raw, ups)):
        assert torch.equal(x, y)
    # the sums: two runs, and eager against a captured graph's replay
    ins, _ = reg_inputs(P, 3, 1, seed=6)
    run = lambda: surfel_regularizers(*ins, ALL)
    (l0, t0), (l1, t1) = run(), run()
    assert torch.equal(l0, l1) and torch.equal(t0, t1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lg, tg = run()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(lg, l0) and torch.equal(tg, t0)


# ---- the model ---------------------------------------------------------------------------------------------------------------
P0, W, H, FRAMES = 3000, 160, 120, 6


def _smpl_parms(poses):
    fp = poses["full_pose"]
    return {"betas": poses["betas"], "expression": poses["expression"], "global_orient": fp[:, :3], "body_pose": fp[:, 3:66],
            "jaw_pose": fp[:, 66:69], "leye_pose": fp[:, 69:72], "reye_pose": fp[:, 72:75], "left_hand_pose": fp[:, 75:120],
            "right_hand_pose": fp[:, 120:165], "transl": poses["transl"]}


class StubModel:
    """The duck-typed geometry of tests/test_plugin_gpu.py (``SurfelModel``), holding the ACTIVATED tensors as its leaves, so that
    it can be given a model's values bit for bit."""

    def __init__(self, xyz, rot, scale, color, opacity, occ, guidance, field, config=(1.0, 1.0, 1.0, 0.0)):
        d = lambda t: t.detach().clone().contiguous().requires_grad_(True)
        self._xyz, self._rot, self._scale, self._color, self._opacity, self._occ = d(xyz), d(rot), d(scale), d(color), d(opacity), d(occ)
        self.smpl_guidance, self.active_sh_degree, self._field = guidance, 0, field
        self.config = torch.tensor(config, dtype=torch.float32, device=DEV)

    get_xyz = property(lambda s: s._xyz)
    get_rotation = property(lambda s: s._rot)
    get_opacity = property(lambda s: s._opacity)
    get_occ = property(lambda s: s._occ)
    get_scaling = property(lambda s: s._scale)
    get_colors = property(lambda s: s._color)

    def attribute_field(self, x, z=0):
        return self._field(x, z)


@pytest.fixture(scope="module")
def world():
    from soar_amd.renderer import cameras
    from soar_amd.smpl_guidance import SMPLGuidance
    import soar_amd.renderer  # noqa: F401
    body = syn.make_body_model(0)
    poses = syn.make_pose_sequence(FRAMES, 0)
    guide = SMPLGuidance(body, _smpl_parms(poses), device=DEV)
    surf = syn.make_surfels(P0, 0)
    spec = syn.make_camera(W, H, distance=3.0, elevation=0.1, azimuth=0.4)
    cam = cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(DEV), image_width=W, image_height=H,
                         world_view_transform=spec.world_view_transform.to(DEV), full_proj_transform=spec.full_proj_transform.to(DEV),
                         prcppoint=spec.prcppoint.to(DEV))
    return types.SimpleNamespace(body=body, poses=poses, guide=guide, surf=surf, cam=cam, spec=spec)


def make_model(w, cfg=None, P=None, seed=0):
    from soar_amd.geometry import GaussianSurfelModel
    surf = w.surf if P is None else syn.make_surfels(P, seed)
    m = GaussianSurfelModel(dict(cfg or {}))
    m.create_from_pcd(surf.xyz, surf.colors.clamp(0.02, 0.98), 10, smpl_guidance=w.guide)
    with torch.no_grad():                         # the synthetic body's orientations and sizes instead of identity / neighbour distance
        m._rotation.copy_(surf.rot.to(DEV))
        m._scaling.copy_(torch.log(surf.scales[:, :1].to(DEV)))
    m.invalidate()
    return m


def test_create_from_pcd_and_cached_properties(world):
    from soar_amd import lbs
    from soar_amd.field import HashMLPField
    from soar_amd.geometry import GaussianSurfelModel
    w = world
    m = GaussianSurfelModel({})
    pts, col = w.surf.xyz, w.surf.colors.clamp(0.02, 0.98)
    m.create_from_pcd(pts.numpy(), col.numpy(), 10, smpl_guidance=w.guide)
    P = pts.shape[0]
    assert torch.equal(m._xyz.detach().cpu(), pts) and torch.equal(m.original_pos.cpu(), pts) and float(m.get_delta_xyz.detach().abs().max()) == 0
    want = torch.log(torch.sqrt(torch.clamp_min(lbs.dist2_knn3(pts.to(DEV)), 1e-7)))[:, None]
    assert torch.equal(m._scaling.detach(), want) and m._scaling.shape == (P, 1)
    assert torch.equal(m._rotation.detach(), torch.tensor([1.0, 0, 0, 0], device=DEV).expand(P, 4))           # no init_q: identity
    torch.testing.assert_close(m.get_opacity, torch.full((P, 1), 0.1, device=DEV), rtol=1e-6, atol=0)
    torch.testing.assert_close(m.get_occ, torch.full((P, 1), 0.01, device=DEV), rtol=1e-6, atol=0)
    torch.testing.assert_close(m.get_colors.detach().cpu(), col, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(m._features_dc.detach().cpu()[:, 0], (col - 0.5) / 0.28209479177387814)
    assert m._features_rest.shape == (P, 0, 3) and m.get_features.shape == (P, 1, 3) and m.latent_pose.shape == (FRAMES, 2)
    box = torch.stack([pts.min(0).values, pts.max(0).values]).to(DEV)
    c = box.mean(0)
    torch.testing.assert_close(m.aabb, (box - c) * 1.5 + c)
    assert isinstance(m.attribute_field, HashMLPField) and m.radius == 0.1 and m.max_radii2D.shape == (P,)
    n = m.get_normal
    torch.testing.assert_close(n, torch.tensor([0.0, 0, 1], device=DEV).expand(P, 3))
    # a guidance with init_q and canonical query points is used
    g2 = types.SimpleNamespace(init_q=torch.nn.functional.normalize(torch.randn(P, 4)), query_points=pts[None] * 2, smpl_parms=w.guide.smpl_parms)
    m2 = GaussianSurfelModel({})
    m2.create_from_pcd(pts, col, 10, smpl_guidance=g2)
    assert torch.equal(m2._rotation.detach().cpu(), g2.init_q)
    torch.testing.assert_close(m2.aabb, ((box - c) * 1.5 + c) * 2)
    # one node, cached: a second read returns the same tensors; a step (or any replaced leaf) drops them
    a = (m.get_rotation, m.get_scaling, m.get_opacity, m.get_occ, m.get_colors)
    b = (m.get_rotation, m.get_scaling, m.get_opacity, m.get_occ, m.get_colors)
    assert all(x is y for x, y in zip(a, b)) and len({x.grad_fn for x in a}) == 1 and a[0].grad_fn is not None
    m.training_setup()
    sum(x.sum() for x in a).backward()
    assert all(t.grad is not None for t in (m._rotation, m._scaling, m._opacity, m._occ, m._colors))
    before = m.get_opacity.detach().clone()
    m.optimizer.step()
    assert m.get_opacity is not a[2] and not torch.equal(m.get_opacity.detach(), before)
    with torch.no_grad():
        assert m.get_opacity.requires_grad is False
    assert m.get_opacity.requires_grad is True


def _sds_batch(bs=3):
    c2w = torch.stack([syn.make_c2w(2.5, 0.1 * i, 0.7 * i, target=(0.0, 0.0, 0.0)) for i in range(bs)])
    return dict(c2w=c2w, fovy=torch.full((bs,), 0.8), width=W, height=H, rays_d=torch.zeros(bs, H, W, 3, device=DEV), gt_index=2)


def _gt_batch(w, res=96):
    nf = 2 * math.atan(0.5 / 1.1)
    return dict(gt_fovx=w.spec.fovx, gt_fovy=w.spec.fovy, gt_c2w=syn.make_c2w(3.0, 0.1, 0.4)[None], gt_normal_fovx=nf, gt_normal_fovy=nf,
                gt_normal_res=res, gt_normal_cx=torch.tensor([res / 2.0]), gt_normal_cy=torch.tensor([res / 2.0]),
                gt_cx=torch.tensor([W / 2.0]), gt_cy=torch.tensor([H / 2.0]), gt_width=W, gt_height=H,
                rand_bg_color=torch.tensor([0.2, 0.5, 0.7], device=DEV), gt_index=3)


def _render_groups(w, pc, use_explicit):
    """One SDS view group and one video-frame group through the plugin; -> (outputs, gradients of what the renderer read)."""
    from soar_amd.renderer import registry
    renderer = registry.find("gaussiansurfel-rasterizer")({"use_explicit": use_explicit}, geometry=pc)
    renderer.background = lambda dirs: torch.full(dirs.shape, 0.3, device=DEV)
    read = [pc.get_xyz, pc.get_rotation, pc.get_scaling, pc.get_colors, pc.get_opacity, pc.get_occ]
    for t in read:
        if not t.is_leaf:
            t.retain_grad()
    outs = {}
    a, b = renderer.batch_forward(_sds_batch()), renderer.gt_forward(_gt_batch(w))
    loss = 0
    for tag, o in (("sds", a), ("gt", b)):
        for k, v in o.items():
            if torch.is_tensor(v) and v.is_floating_point():
                outs[f"{tag}/{k}"] = v.detach().clone()
                if v.requires_grad:
                    loss = loss + v.square().mean() + v.mean()
    loss.backward()
    return outs, [None if t.grad is None else t.grad.detach().clone() for t in read]


# The bar of the rasterizer's gradients between two evaluations that differ only in the order of its float atomics: the one this
# project already holds the same kernels to wherever two such evaluations are compared (tests/test_plugin_gpu.py: fused against
# composed view, one call against three, batched against per-pose): worst element within 2e-4 of the largest magnitude.
ATOMIC_ORDER_BAR = 2e-4
NAMES = ("xyz", "rotation", "scaling", "colors", "opacity", "occ")


@pytest.mark.parametrize("use_explicit", [True, False])
def test_plugin_renders_the_model_like_the_stub(world, use_explicit):
    """Forward: the same bits as the stub, every image of both groups.

    Backward, in three parts, because "the same bits" is not defined for the whole of it: the rasterizer's backward adds the
    per-pixel contributions with float atomics (csrc/rast_render_bwd.hip), so the stub does not reproduce its OWN gradient bits
    from one run to the next (measured on an MI355X: d xyz differs by 3e-8 .. 4e-8 between two stub runs at a largest value of 0.15).
    (1) What is deterministic is asserted bit for bit: the gradients at the model's leaves are exactly what
        ``soar_surfel_activations_backward`` makes of the gradients that arrived at the model's five activated tensors (retained;
        ``get_xyz`` is the leaf itself), and they meet the float64 restatement of that backward on the same gradients.
    (2) Whenever two runs of the stub give the same bits for a tensor, the model must give those bits too.
    (3) Otherwise model and stub are held to the fixed bar this project uses for two evaluations of these kernels that differ in
        atomic order (ATOMIC_ORDER_BAR), not to a sampled spread."""
    from soar_amd.geometry import surfel_activations
    w = world
    m = make_model(w)
    with torch.no_grad():
        m._opacity.fill_(30.0)                         # the stub's constant opacity of one: sigmoid(30) rounds to 1
        m._occ.copy_(torch.logit(torch.rand(P0, 1, generator=torch.Generator().manual_seed(4)).clamp(0.01, 0.99)).to(DEV))
    color, scale = m.get_colors.detach().clone(), m.get_scaling.detach().clone()
    field = lambda x, z=0: {"shs": color, "scales": scale, "offsets": torch.zeros_like(x)}
    m.attribute_field = field
    m.config = torch.tensor([1.0, 1.0, 1.0, 0.0], device=DEV)
    assert float(m.get_opacity.min()) == 1.0
    mk = lambda: StubModel(m._xyz, m.get_rotation, m.get_scaling, m.get_colors, m.get_opacity, m.get_occ, w.guide, field)
    o_model, g_model = _render_groups(w, m, use_explicit)
    o_stub, g_stub = _render_groups(w, mk(), use_explicit)
    _, g_stub2 = _render_groups(w, mk(), use_explicit)
    assert set(o_model) == set(o_stub) and len(o_model) >= 10
    for k in o_stub:
        assert torch.equal(o_model[k], o_stub[k]), k
    # (1) the model's own node, bit for bit on the gradients that reached it
    g_xyz, g_rot, g_sc, g_col, g_op, g_occ = g_model
    ins = [t.detach().clone().requires_grad_(True) for t in (m._rotation, m._scaling, m._opacity, m._occ, m._colors)]
    outs = surfel_activations(*ins)
    pairs = [(o, g) for o, g in zip(outs, (g_rot, g_sc, g_op, g_occ, g_col)) if g is not None]
    assert len(pairs) >= 2
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    for leaf, twin, g, name in zip((m._rotation, m._scaling, m._opacity, m._occ, m._colors), ins, (g_rot, g_sc, g_op, g_occ, g_col),
                                   ("rotation", "scaling", "opacity", "occ", "colors")):
        if g is None:
            assert leaf.grad is None and twin.grad is None, name
            continue
        assert leaf.grad is not None and torch.equal(leaf.grad, twin.grad), name
        assert torch.isfinite(leaf.grad).all(), name
    # ... and against the float64 restatement of the activations' backward on those same gradients (the bar of the node's own test)
    ins64 = [t.detach().double().requires_grad_(True) for t in (m._rotation, m._scaling, m._opacity, m._occ, m._colors)]
    outs64 = gr.activations(*ins64)
    sel = [(o, g.double()) for o, g in zip(outs64, (g_rot, g_sc, g_op, g_occ, g_col)) if g is not None]
    torch.autograd.backward([o for o, _ in sel], [g for _, g in sel])
    assert gr.rel_l2(m._rotation.grad, ins64[0].grad) <= 1e-6 and gr.rel_l2(m._occ.grad, ins64[3].grad) <= 1e-6
    # (2), (3) model against stub at the tensors the renderer read
    seen = 0
    for a, b, c, name in zip(g_model, g_stub, g_stub2, NAMES):
        assert (a is None) == (b is None), name
        if b is None:
            continue
        seen += 1
        big = float(b.abs().max())
        spread, dist = float((b - c).abs().max()), float((a - b).abs().max())
        print(f"use_explicit={use_explicit} d{name}: model-stub {dist:.3e}, stub-stub {spread:.3e}, largest {big:.3e}")
        assert big > 0 and torch.isfinite(a).all(), name
        if torch.equal(b, c):
            assert torch.equal(a, b), name
        assert dist <= ATOMIC_ORDER_BAR * big, (name, dist, big)
    assert seen >= 3


def _groups_for_torch(m):
    return [{"params": list(g["params"]), "lr": g["lr"], "name": g["name"]} for g in m.optimizer.param_groups]


@pytest.mark.parametrize("P", [2000, 1997, 1998, 1999])
def test_one_launch_adam_matches_torch_adam_over_all_groups(world, P):
    """(P past 2000: surfel counts that are no multiple of four -- the leaves' rows end inside a float4 of the wide table's kernel)"""
    w = world
    m = make_model(w, dict(position_lr_init=1.6e-5, position_lr_final=1.6e-6, position_lr_max_steps=1000), P=P, seed=1)
    m.training_setup()
    ours = [p for g in m.optimizer.param_groups for p in g["params"]]
    assert len(ours) == 27
    ref = [p.detach().clone().requires_grad_(True) for p in ours]
    it = iter(ref)
    tgroups = [{"params": [next(it) for _ in g["params"]], "lr": g["lr"], "name": g["name"]} for g in m.optimizer.param_groups]
    tadam = torch.optim.Adam(tgroups, lr=0.0, eps=1e-15)
    gen = torch.Generator().manual_seed(0)
    for step in range(10):
        lr = m.update_learning_rate(step + 1)
        assert lr == pytest.approx(gr.expon_lr(step + 1, 1.6e-4, 1.6e-5, 0, 0.01, 1000), rel=1e-12) and m.optimizer.param_groups[0]["lr"] == lr
        tadam.param_groups[0]["lr"] = lr
        for a, b in zip(ours, ref):
            grad = (torch.randn(a.shape, generator=gen) * (10.0 ** ((step % 5) - 2))).to(DEV)      # drawn once on the host, fed to both
            a.grad, b.grad = grad, grad.clone()
        m.optimizer.step()
        tadam.step()
        for k, (a, b) in enumerate(zip(ours, ref)):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=3e-5, atol=5e-7, msg=lambda s: f"step {step} tensor {k}: {s}")
    assert m.optimizer.steps == 10 and int(m.optimizer._dev_state[0]) == 10
    m.optimizer.zero_grad()
    assert all(p.grad is None for p in ours)


def _force_stats(m, seed=0):
    """Statistics that prune some rows, clone some and split some."""
    P = m.num_points
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m._opacity.copy_(torch.where(torch.rand(P, 1, generator=g) < 0.2, -4.0, 2.0).to(DEV))           # sigmoid(-4) < 0.1: pruned
        big = (torch.rand(P, 1, generator=g) < 0.4).to(DEV)
        m._scaling.copy_(torch.where(big, math.log(0.004), math.log(0.0004)))                             # percent_dense * extent = 0.001
    m.invalidate()
    d = m.densifier
    d.accum.zero_()
    d.accum[4] = 1.0
    d.accum[0] = torch.where(torch.rand(P, generator=g) < 0.5, 1e-3, 0.0).to(DEV)                         # threshold 1e-4
    m.max_radii2D = torch.rand(P, generator=g).to(DEV) * 7
    m.original_pos = (m._xyz.detach() + 0.01 * torch.randn(P, 3, generator=g).to(DEV)).contiguous()


def test_update_states_prunes_and_densifies_every_per_row_tensor(world):
    from soar_amd.densify import PARAMS, SurfelDensifier
    w = world
    cfg = dict(densify_from_iter=0, prune_from_iter=0, densification_interval=5, densify_grad_threshold=1e-4, opacity_reset_interval=100000)
    m = make_model(w, cfg, P=4000, seed=2)
    m.training_setup()
    ours = [p for g in m.optimizer.param_groups for p in g["params"]]
    gen = torch.Generator().manual_seed(3)
    for _ in range(2):                                   # moments that are not zero
        for p in ours:
            p.grad = torch.randn(p.shape, generator=gen).to(DEV)
        m.optimizer.step()
    _force_stats(m)
    P = m.num_points
    field_state = {p: (m.optimizer.state[p]["exp_avg"].clone(), p.detach().clone()) for g in m.optimizer.param_groups if "attribute" in g["name"] for p in g["params"]}
    # the densifier by hand on copies of the same tensors, with torch's Adam holding copies of the moments
    attr = dict(__import__("soar_amd.geometry", fromlist=["LEAVES"]).LEAVES)
    hand = {k: nn.Parameter(getattr(m, attr[k]).detach().clone()) for k in PARAMS}
    hand["scaling"] = nn.Parameter(hand["scaling"].detach().repeat(1, 3).contiguous())
    hand["f_rest"] = nn.Parameter(torch.zeros(P, 1, 3, device=DEV))          # degree 0: [P,0,3] is not a row the kernels take
    opt = torch.optim.Adam([{"params": [hand[k]], "lr": 1e-3, "name": k} for k in PARAMS], lr=0.0, eps=1e-15)
    for k in PARAMS:
        st = m.optimizer.state[getattr(m, attr[k])]
        wide = (lambda t: t.repeat(1, 3).contiguous()) if k == "scaling" else (lambda t: torch.zeros(P, 1, 3, device=DEV)) if k == "f_rest" else (lambda t: t.clone())
        opt.state[hand[k]] = {"step": torch.tensor(2.0), "exp_avg": wide(st["exp_avg"]), "exp_avg_sq": wide(st["exp_avg_sq"])}
    d = SurfelDensifier(hand, opt, percent_dense=m.percent_dense, surface=True)
    d.accum.copy_(m.densifier.accum)
    flags = d.flags(True, True, 0.1, m.radius, 1e-4)
    pruned, clone, split = (flags & 1) > 0, (flags & 2) > 0, (flags & 4) > 0
    assert int(pruned.sum()) > 100 and int(clone.sum()) > 100 and int(split.sum()) > 100
    noise = torch.randn(2 * int(split.sum()), 3, generator=gen).to(DEV)
    old = {k: getattr(m, attr[k]).detach().clone() for k in attr}
    old_m = {k: m.optimizer.state[getattr(m, attr[k])]["exp_avg"].clone() for k in attr}
    old_pos, old_r = m.original_pos.clone(), m.max_radii2D.clone()
    act_before = m.get_opacity
    r_hand = d.prune_and_densify(0.1, 1e-4, m.radius, noise=noise)
    # update_states at an iteration on the interval: the view's statistics are empty (radii 0), the forced ones decide
    radii = [torch.zeros(P, dtype=torch.int32, device=DEV)]
    r = m.update_states(5, [radii[0] > 0], radii, [torch.zeros(P, 3, device=DEV)], noise=noise)
    assert r == r_hand and r["cloned"] == int(clone.sum()) and r["split"] == int(split.sum())
    Pn = r["num_points"]
    assert Pn == r["kept"] + r["cloned"] + 2 * r["split"] and Pn != P
    for k in attr:
        assert getattr(m, attr[k]).shape[0] == Pn and getattr(m, attr[k]).requires_grad, k
        st = m.optimizer.state[getattr(m, attr[k])]
        assert st["exp_avg"].shape == getattr(m, attr[k]).shape and st["exp_avg_sq"].shape == getattr(m, attr[k]).shape, k
        g = [g for g in m.optimizer.param_groups if g["name"] == k][0]
        assert g["params"][0] is getattr(m, attr[k])
    assert m.original_pos.shape == (Pn, 3) and m.max_radii2D.shape == (Pn,) and m.densifier.accum.shape == (5, Pn)
    # row for row the hand-driven densifier's model (the one-column scaling is its first column) and its moments
    for k in PARAMS:
        want, wm = d.params[k].detach(), opt.state[d.params[k]]
        sel = (lambda t: t[:, :1]) if k == "scaling" else (lambda t: t[:, :0]) if k == "f_rest" else (lambda t: t)
        assert torch.equal(getattr(m, attr[k]).detach(), sel(want)), k
        st = m.optimizer.state[getattr(m, attr[k])]
        assert torch.equal(st["exp_avg"], sel(wm["exp_avg"])) and torch.equal(st["exp_avg_sq"], sel(wm["exp_avg_sq"])), k
    # kept rows: unchanged bit for bit, everything that follows the rows included
    stay = ~pruned & ~split
    nk = int(stay.sum())
    assert nk == r["kept"]
    assert torch.equal(m.original_pos[:nk], old_pos[stay]) and torch.equal(m.max_radii2D[:nk], old_r[stay])
    for k in attr:
        assert torch.equal(getattr(m, attr[k]).detach()[:nk], old[k][stay]), k
        assert torch.equal(m.optimizer.state[getattr(m, attr[k])]["exp_avg"][:nk], old_m[k][stay]), k
        assert float(m.optimizer.state[getattr(m, attr[k])]["exp_avg"][nk:].abs().sum()) == 0.0, k
    # new rows: no displacement, no radius; the occlusion value of the row they were made from
    assert torch.equal(m.original_pos[nk:], m._xyz.detach()[nk:]) and float(m.max_radii2D[nk:].abs().sum()) == 0.0
    assert float(m.get_delta_xyz.detach()[nk:].abs().max()) == 0.0
    src = torch.cat([torch.nonzero(clone)[:, 0], torch.nonzero(split)[:, 0].repeat(2)])
    assert torch.equal(m._occ.detach()[nk:], old["occ"][src]) and torch.equal(m._colors.detach()[nk:], old["color"][src])
    # the field's groups keep their tensors and their state
    for p, (mom, val) in field_state.items():
        assert torch.equal(m.optimizer.state[p]["exp_avg"], mom) and torch.equal(p.detach(), val)
    # the cached activations are fresh, and the next step runs
    assert m.get_opacity is not act_before and m.get_opacity.shape == (Pn, 1)
    assert torch.equal(m.get_opacity.detach(), torch.sigmoid(m._opacity.detach())) or gr.rel_l2(m.get_opacity, torch.sigmoid(m._opacity.detach())) < 1e-6
    loss, _ = m.regularizers({"lambda_delta": 1.0, "lambda_scales": 0.1, "lambda_sparsity": 0.1})
    (loss + m.get_rotation.sum() + m.get_colors.sum() + m.get_occ.sum()).backward()
    before = m._opacity.detach().clone()
    m.optimizer.step()
    assert not torch.equal(before, m._opacity.detach()) and all(torch.isfinite(getattr(m, a)).all() for a in attr.values())
    # prune_points and reset_opacity keep the bookkeeping consistent
    mask = torch.zeros(Pn, dtype=torch.bool, device=DEV)
    mask[::3] = True
    keep_pos = m.original_pos[~mask].clone()
    m.prune_points(mask)
    assert m.num_points == Pn - int(mask.sum()) and torch.equal(m.original_pos, keep_pos) and m._occ.shape[0] == m.num_points
    m.reset_opacity(0.12)
    assert float(m.get_opacity.max()) <= 0.1201 and float(m.optimizer.state[m._opacity]["exp_avg"].abs().sum()) == 0.0


def _drive(m, steps, seed):
    gen = torch.Generator().manual_seed(seed)
    ours = [p for g in m.optimizer.param_groups for p in g["params"]]
    for s in range(steps):
        m.update_learning_rate(m.optimizer.steps + 1)
        for p in ours:
            p.grad = (torch.randn(p.shape, generator=gen) * 0.1).to(DEV)
        m.optimizer.step()


def test_capture_restore_continues_bit_for_bit_and_ply_round_trip_renders_the_same(world, tmp_path):
    from soar_amd.geometry import LEAVES, GaussianSurfelModel
    w = world
    cfg = dict(position_lr_init=1.6e-5, position_lr_final=1.6e-6, position_lr_max_steps=1000)
    a = make_model(w, cfg, P=1500, seed=3)
    a.training_setup()
    _drive(a, 3, seed=1)
    snap = a.capture()
    b = GaussianSurfelModel(cfg)
    b.smpl_guidance = w.guide
    b.restore(snap)
    assert b.optimizer.steps == 3 and [g["lr"] for g in b.optimizer.param_groups] == [g["lr"] for g in a.optimizer.param_groups]
    _drive(a, 1, seed=2)
    _drive(b, 1, seed=2)
    for name, attr in LEAVES:
        assert torch.equal(getattr(a, attr).detach(), getattr(b, attr).detach()), name
        assert torch.equal(a.optimizer.state[getattr(a, attr)]["exp_avg_sq"], b.optimizer.state[getattr(b, attr)]["exp_avg_sq"]), name
    for pa, pb in zip(a.attribute_field.parameters(), b.attribute_field.parameters()):
        assert torch.equal(pa.detach(), pb.detach())
    assert torch.equal(a.latent_pose.detach(), b.latent_pose.detach()) and torch.equal(a.original_pos, b.original_pos)
    # the checkpoint did not move with the model
    assert not torch.equal(snap[1], a._xyz.detach())
    # PLY: the six leaves of the file, into a model made from the same point cloud
    path = str(tmp_path / "avatar.ply")
    a.save_ply(path)
    c = make_model(w, cfg, P=1500, seed=3)
    c.load_ply(path)
    for attr in ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation"):
        assert torch.equal(getattr(a, attr).detach(), getattr(c, attr).detach()) and getattr(c, attr).is_cuda, attr
    with torch.no_grad():
        c._colors.copy_(a._colors)
        c._occ.copy_(a._occ)
    c.attribute_field, c.config = a.attribute_field, a.config
    from soar_amd.renderer import registry
    imgs = []
    for pc in (a, c):
        r = registry.find("gaussiansurfel-rasterizer")({"use_explicit": False}, geometry=pc)
        with torch.no_grad():
            imgs.append(r(w.cam, torch.tensor([0.2, 0.5, 0.7], device=DEV), gt=True, gt_index=3))
    for k in ("render", "normal", "depth", "mask", "occ"):
        assert torch.equal(imgs[0][k], imgs[1][k]), k
    assert float(imgs[0]["mask"].mean()) > 0.01


def test_thirty_training_steps_end_to_end(world):
    """model + plugin + avatar_stage_loss + regularizers + update_states: the loss of the last step is strictly below the first and
    every leaf is finite.  It shows that the parts are connected, not how well they train."""
    from soar_amd.geometry import LEAVES
    from soar_amd.losses import avatar_stage_loss
    from soar_amd.renderer import registry
    w = world
    cfg = dict(position_lr_init=1.6e-5, position_lr_final=1.6e-6, position_lr_max_steps=1000, feature_lr=0.01, opacity_lr=0.01, field_lr=0.01,
               rotation_lr=0.001, occ_lr=0.1, densify_from_iter=5, prune_from_iter=5, densification_interval=15, densify_grad_threshold=1e-4)
    m = make_model(w, cfg)
    m.training_setup()
    renderer = registry.find("gaussiansurfel-rasterizer")({"use_explicit": False}, geometry=m)
    bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
    # the target: the synthetic body itself, rendered with its own colours through the explicit path
    with torch.no_grad():
        tgt = registry.find("gaussiansurfel-rasterizer")({"use_explicit": True}, geometry=m)(w.cam, bg, gt=True, gt_index=3)
    gt_rgb, gt_mask, gt_normal = tgt["render"].clone(), tgt["mask"].clone(), tgt["normal"].clone()
    sel = gt_mask[0] > 0.5
    losses, changed = [], None
    for it in range(1, 31):
        m.update_learning_rate(it)
        out = renderer(w.cam, bg, gt=True, gt_index=3)
        scales = m.attribute_field(m.get_xyz)["scales"]
        reg, terms = m.regularizers({"lambda_delta": 1.0, "lambda_scales": 0.1}, scales=scales)
        loss = avatar_stage_loss(out, gt_rgb, gt_mask, gt_normal, sel) + reg
        m.optimizer.zero_grad()
        loss.backward()
        losses.append(float(loss))
        m.optimizer.step()
        if it == 15:
            changed = m.update_states(it, [out["visibility_filter"]], [out["radii"]], [out["viewspace_points"]])
    print("losses", losses[0], losses[-1], "densification", changed)
    assert changed is not None and changed["num_points"] == m.num_points
    assert losses[-1] < losses[0], losses
    for name, attr in LEAVES:
        assert torch.isfinite(getattr(m, attr)).all(), name
    assert all(torch.isfinite(p).all() for p in m.attribute_field.parameters())
