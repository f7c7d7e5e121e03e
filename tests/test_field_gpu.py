"""GPU tests of the attribute field (csrc/field.hip, soar_amd/field.py) against the float64 restatement (tests/field_ref.py):
outputs and gradients for the renderer's, all five, the reset loss's and the position's upstream gradients, reproducibility,
sizes, frozen parameters, the renderer plugin with ``use_explicit: False``, and ``reset_field``."""
import types

import pytest
import torch

import field_ref as R
from soar_amd import synthetic as syn
from soar_amd.field import HashMLPField

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P = 100_000


def _aabb(cano):
    """as surfel_base.py:570-574 builds it from the canonical points"""
    aabb = torch.stack([cano.min(dim=0)[0], cano.max(dim=0)[0]])
    center = aabb.mean(dim=0)
    return (aabb - center) * 1.5 + center


def _field(aabb, seed=0):
    torch.manual_seed(seed)
    f = HashMLPField(aabb)
    with torch.no_grad():              # the offsets head starts at zero: give it weights, so that its backward carries something
        f.mlp_base_offsets.layers[-1].weight.normal_(0, 0.1)
        f.mlp_base_offsets.layers[-1].bias.normal_(0, 0.1)
        f.encoding.hash_table.mul_(100)   # tables that carry a signal past the first layer
        f.quat_encoding.hash_table.mul_(100)
    return f.to(DEV)


@pytest.fixture(scope="module")
def world():
    surf = syn.make_surfels(P, 0)
    aabb = _aabb(surf.xyz)
    f = _field(aabb)
    lo, hi = aabb[0], aabb[1]
    mid = (lo + hi) / 2
    extra = [hi + 0.1, lo - 0.2, torch.stack([hi[0] + 1, mid[1], mid[2]])]                 # outside the box
    for d in range(3):                                                                      # exactly on its faces
        for v in (lo[d], hi[d]):
            x = mid.clone()
            x[d] = v
            extra.append(x)
    xyz = torch.cat([surf.xyz, torch.stack(extra)]).to(DEV).contiguous()
    return types.SimpleNamespace(surf=surf, aabb=aabb, f=f, xyz=xyz)


def _lattice_points():
    """normalised points on the lattices of several levels (0.5: every even resolution; 0.25: 16, 80, 212, 776, 1072)"""
    g = torch.Generator().manual_seed(5)
    v = torch.tensor([0.25, 0.5, 0.75, 0.125, 0.0625])
    pts = v[torch.randint(0, 5, (300, 3), generator=g)]
    return torch.cat([pts, torch.rand(300, 3, generator=g)]).to(DEV)


def _upstream(kind, n, seed=7):
    g = torch.Generator().manual_seed(seed)
    G = {h: torch.randn(n, o, generator=g).to(DEV) for h, o in (("shs", 3), ("scales", 1), ("quats", 4), ("offsets", 3),
                                                                  ("opacities", 1))}
    gt_shs = torch.full((n, 3), 0.5, device=DEV)
    gt_scales = (torch.rand(n, 1, generator=g) * 2e-2).to(DEV)
    gt_quats = torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1).to(DEV)

    def loss(out):
        if kind == "renderer":
            return sum((out[h].float() * G[h].to(out[h].dtype)).sum() for h in ("shs", "scales", "offsets"))
        if kind == "reset":
            mse = torch.nn.functional.mse_loss
            return (((out["shs"] - gt_shs.to(out["shs"].dtype)) ** 2).mean() + 1000 * mse(out["scales"], gt_scales.to(out["shs"].dtype))
                    + mse(out["quats"], gt_quats.to(out["shs"].dtype)))
        return sum((out[h] * G[h].to(out[h].dtype)).sum() for h in G)
    return loss


def _run_hip(f, xyz, z, loss, xyz_grad):
    f.zero_grad(set_to_none=True)
    x = xyz.clone().requires_grad_(xyz_grad)
    out = f(x, z=z)
    loss(out).backward()
    grads = {n: p.grad for n, p in f.named_parameters()}
    grads["xyz"] = x.grad
    grads["z"] = None if z is None else z.grad
    return out, grads


def _names(f):
    return [n for n, _ in f.named_parameters()]


def _run_ref(f, xyz, z, loss, xyz_grad, dtype, is_normalized=False):
    return R.run(f, xyz, z, loss, xyz_grad, dtype, is_normalized, res=R.resolutions(), T=2 ** 18)


def _check_outputs(out, r64, r32):
    for h in R.HEADS:
        a, b, c = out[h].detach().double(), r64[h].detach(), r32[h].detach().double()
        err, err32 = float((a - b).abs().max()), float((c - b).abs().max())
        scale = max(1.0, float(b.abs().max()))
        print(f"{h}: max err {err:.2e} (float32 restatement {err32:.2e})")
        assert err <= 1e-5 * scale, (h, err, err32)
        assert err <= max(2 * err32, 1e-6), (h, err, err32)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


def _check_grads(g, g64, g32, names):
    measured = {}
    for n in names:
        if g64[n] is None:
            assert g[n] is None, n
            continue
        assert g[n] is not None, n
        if float(g64[n].abs().max()) == 0:
            assert float(g[n].abs().max()) == 0, n
            continue
        rel, rel32 = _rel(g[n], g64[n]), _rel(g32[n], g64[n])
        measured[n] = (rel, rel32)
        assert rel <= 1e-5, (n, rel, rel32)
        assert rel <= max(2 * rel32, 1e-6), (n, rel, rel32)
    return measured


@pytest.mark.parametrize("kind", ["renderer", "all", "reset", "xyz_z"])
def test_outputs_and_gradients_match_float64(world, kind):
    f, xyz = world.f, world.xyz
    n = xyz.shape[0]
    loss = _upstream("all" if kind == "xyz_z" else kind, n)
    xyz_grad = kind == "xyz_z"
    z = torch.tensor([0.4, -0.3], device=DEV, requires_grad=True) if kind == "xyz_z" else None
    out, g = _run_hip(f, xyz, z, loss, xyz_grad)
    r64, g64 = _run_ref(f, xyz, z, loss, xyz_grad, torch.float64)
    r32, g32 = _run_ref(f, xyz, z, loss, xyz_grad, torch.float32)
    _check_outputs(out, r64, r32)
    names = _names(f) + (["xyz", "z"] if xyz_grad else [])
    measured = _check_grads(g, g64, g32, names)
    print(kind, {k: f"{v[0]:.2e}/{v[1]:.2e}" for k, v in measured.items()})
    if kind == "renderer":
        assert g["quat_encoding.hash_table"] is None and g["mlp_base_opacities.layers.0.weight"] is None
    # points outside the box and on its faces are encoded at the origin
    p0 = R.field(torch.zeros(1, 3, device=DEV), None, *R.params_of(f, torch.float64, requires_grad=False), None, R.resolutions(),
                 2 ** 18, True, torch.float64)
    assert torch.allclose(out["shs"][P:].double(), p0["shs"].expand(xyz.shape[0] - P, -1), atol=1e-6)


def test_spatial_order_scatter_matches_float64(world):
    """points in Morton order: neighbouring lanes share the coarse levels' rows, and the scatter sums those runs in the wave
    before its atomics"""
    f = world.f
    xyz = syn.sort_surfels_spatially(world.surf).xyz.to(DEV).contiguous()
    loss = _upstream("all", xyz.shape[0])
    out, g = _run_hip(f, xyz, None, loss, False)
    r64, g64 = _run_ref(f, xyz, None, loss, False, torch.float64)
    r32, g32 = _run_ref(f, xyz, None, loss, False, torch.float32)
    _check_outputs(out, r64, r32)
    measured = _check_grads(g, g64, g32, _names(f))
    print("spatial", {k: f"{v[0]:.2e}/{v[1]:.2e}" for k, v in measured.items() if "hash" in k})


def test_lattice_points_normalized(world):
    f = world.f
    xyz = _lattice_points()
    loss = _upstream("all", xyz.shape[0])
    f.zero_grad(set_to_none=True)
    out = f(xyz, is_normalized=True)
    loss(out).backward()
    g = {n: p.grad for n, p in f.named_parameters()}
    r64, g64 = _run_ref(f, xyz, None, loss, False, torch.float64, is_normalized=True)
    r32, g32 = _run_ref(f, xyz, None, loss, False, torch.float32, is_normalized=True)
    _check_outputs(out, r64, r32)
    _check_grads(g, g64, g32, _names(f))


def test_reproducible(world):
    f, xyz = world.f, world.xyz
    loss = _upstream("all", xyz.shape[0])
    z = torch.tensor([0.1, 0.2], device=DEV, requires_grad=True)
    o1, g1 = _run_hip(f, xyz, z, loss, True)
    g1 = {k: (None if v is None else v.clone()) for k, v in g1.items()}
    z.grad = None
    o2, g2 = _run_hip(f, xyz, z, loss, True)
    for h in R.HEADS:
        assert torch.equal(o1[h], o2[h]), h
    for n in g1:
        if "hash_table" in n:
            assert _rel(g2[n], g1[n]) <= 1e-5, n
        else:
            assert torch.equal(g1[n], g2[n]), n


@pytest.mark.parametrize("n", [0, 1, 255, 257])
def test_sizes_and_frozen_parameters(world, n):
    f = _field(world.aabb, seed=3)
    f.quat_encoding.hash_table.requires_grad_(False)
    for p in f.mlp_base_shs.parameters():
        p.requires_grad_(False)
    xyz = world.xyz[:n].contiguous()
    loss = _upstream("all", n)
    out, g = _run_hip(f, xyz, None, loss, False)
    assert all(out[h].shape == (n, o) for h, o in (("shs", 3), ("scales", 1), ("quats", 4), ("offsets", 3), ("opacities", 1)))
    assert g["quat_encoding.hash_table"] is None and g["mlp_base_shs.layers.0.weight"] is None
    assert g["mlp_base_shs.layers.1.bias"] is None
    assert g["encoding.hash_table"] is not None and g["mlp_base_quats.layers.0.weight"] is not None
    if n == 0:
        assert float(g["encoding.hash_table"].abs().max()) == 0 and float(g["mlp_base_scales.layers.1.bias"].abs().max()) == 0
        return
    r64, g64 = _run_ref(f, xyz, None, loss, False, torch.float64)
    r32, g32 = _run_ref(f, xyz, None, loss, False, torch.float32)
    _check_outputs(out, r64, r32)
    frozen = {"quat_encoding.hash_table"} | {n_ for n_ in _names(f) if n_.startswith("mlp_base_shs")}
    _check_grads(g, g64, g32, [n_ for n_ in _names(f) if n_ not in frozen])


def test_reset_field_tracks_the_restatement(world):
    surf = world.surf
    f = _field(world.aabb, seed=4)
    ref = R.RefField(f).to(DEV)
    rots = torch.nn.functional.normalize(surf.rot)
    normal = torch.stack([2 * (rots[:, 1] * rots[:, 3] + rots[:, 0] * rots[:, 2]), 2 * (rots[:, 2] * rots[:, 3] - rots[:, 0] * rots[:, 1]),
                          1 - 2 * (rots[:, 1] ** 2 + rots[:, 2] ** 2)], -1)
    pts = torch.cat([surf.xyz, surf.xyz + 0.001 * normal]).to(DEV)
    colors = torch.full((2 * P, 3), 0.5, device=DEV)
    scales = torch.cat([surf.scales[:, :1]] * 2).to(DEV)
    quats = torch.cat([rots] * 2).to(DEV)
    ours = f.reset_field(pts, colors, scales, quats, iterations=200)
    theirs = HashMLPField.reset_field(ref, pts, colors, scales, quats, iterations=200)
    print("reset_field losses", ours, theirs)
    assert len(ours) == len(theirs) == 10
    for a, b in zip(ours, theirs):
        assert abs(a - b) <= 0.02 * abs(b), (a, b)
    assert ours[-1] < ours[0]


def test_plugin_with_attribute_field():
    """the renderer plugin with ``use_explicit: False`` and this field, against the same geometry whose field is the float32
    restatement with identical parameters"""
    import test_plugin_gpu as TP
    from soar_amd.renderer import cameras, registry
    from soar_amd.smpl_guidance import SMPLGuidance
    import soar_amd.renderer  # noqa: F401

    body = syn.make_body_model(0)
    poses = syn.make_pose_sequence(TP.FRAMES, 0)
    guide = SMPLGuidance(body, TP._smpl_parms(poses), device=DEV)
    surf = syn.make_surfels(TP.P, 0)
    aabb = _aabb(guide.cano_vertices.detach().cpu()[0] if guide.cano_vertices.dim() == 3 else guide.cano_vertices.detach().cpu())
    field = _field(aabb, seed=6)
    ref = R.RefField(field).to(DEV)
    results = []
    for fld in (field, ref):
        pc = TP.SurfelModel(surf, guide)
        pc.attribute_field = fld
        renderer = registry.find("gaussiansurfel-rasterizer")({"use_explicit": False}, geometry=pc)
        cams = []
        for az in (0.4, 2.0, -1.5):
            spec = syn.make_camera(TP.W, TP.H, distance=3.0, elevation=0.1, azimuth=az)
            cams.append(cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(DEV), image_width=TP.W,
                                       image_height=TP.H, world_view_transform=spec.world_view_transform.to(DEV),
                                       full_proj_transform=spec.full_proj_transform.to(DEV), prcppoint=spec.prcppoint.to(DEV)))
        bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
        fld.zero_grad(set_to_none=True)
        one = renderer(cams[0], bg, gt=True, gt_index=3)
        views = renderer.forward_views([{"camera": c, "bg_color": bg} for c in cams], gt=True, gt_index=2)
        imgs = [one["render"], one["mask"]] + [v["render"] for v in views] + [v["normal"] for v in views]
        g = torch.Generator().manual_seed(11)
        loss = sum((im * torch.randn(im.shape, generator=g).to(DEV)).sum() for im in imgs)
        loss.backward()
        grads = {_name_of(n): (None if p.grad is None else p.grad.clone()) for n, p in fld.named_parameters()}
        results.append(([im.detach() for im in imgs], grads))
    (ia, ga), (ib, gb) = results
    for a, b in zip(ia, ib):
        assert float((a - b).abs().max()) <= 1e-5
    assert set(ga) == set(gb)
    print({n: None if ga[n] is None else f"{_rel(ga[n], gb[n]):.2e}" for n in ga})
    assert ga["encoding.hash_table"] is not None and ga["mlp_base_shs.layers.0.weight"] is not None
    for n in ga:
        assert (ga[n] is None) == (gb[n] is None), n
        if ga[n] is not None:
            assert _rel(ga[n], gb[n]) <= 1e-4, n


def _name_of(n):
    """a RefField parameter's name as HashMLPField names it"""
    if n == "table":
        return "encoding.hash_table"
    if n == "qtable":
        return "quat_encoding.hash_table"
    if n.startswith("heads."):
        h, i = n[len("heads."):].rsplit("_", 1)
        return f"mlp_base_{h}." + ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias")[int(i)]
    return n


def test_bad_z_and_inputs_are_refused(world):
    f, xyz = world.f, world.xyz[:100]
    with pytest.raises(ValueError):
        f(xyz, z=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError):
        f(xyz, z=torch.zeros(1, 2, device=DEV))
    with pytest.raises(RuntimeError):
        f(xyz, z=torch.zeros(2))                               # z on the CPU, xyz on the GPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(xyz.cpu())
    with pytest.raises(ValueError):
        f(xyz[:, :2])
