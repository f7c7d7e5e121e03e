"""GPU tests of the avatar initialisation (soar_amd/body.py, csrc/body.hip): the vertex forward against the golden vertices of
the reference's lbs() and, at SMPL-X size, against the float64 restatement; subdivision against the numpy restatement bit for bit;
normals and frames against float64; the guidance's opt-in attributes into GaussianSurfelModel.create_from_pcd and one rendered view.

The bar: HIP against float64 at most 4 x (float32 against float64), floor 1e-6 of the largest magnitude."""
import types

import numpy as np
import pytest
import torch

import body_ref as br
from test_body_cpu import golden_body
from soar_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _smpl_parms(poses):
    fp = poses["full_pose"]
    return {"betas": poses["betas"], "expression": poses["expression"], "global_orient": fp[:, :3], "body_pose": fp[:, 3:66],
            "jaw_pose": fp[:, 66:69], "leye_pose": fp[:, 69:72], "reye_pose": fp[:, 72:75], "left_hand_pose": fp[:, 75:120],
            "right_hand_pose": fp[:, 120:165], "transl": poses["transl"]}


def test_vertices_against_the_reference_golden():
    from soar_amd import body
    g, gb = golden_body()
    t = lambda k: torch.from_numpy(g[k]).to(DEV)
    v = body.smplx_vertices(gb, t("betas"), t("pose"), t("transl"))
    assert v.shape == (4, 96, 3) and v.dtype == torch.float32
    br.bar_check("golden vertices", v, g["verts_f32"], g["verts_f64"])
    # without transl: the same vertices minus transl, up to the rounding of that one addition
    v0 = body.smplx_vertices(gb, t("betas"), t("pose"))
    assert torch.equal(v0 + t("transl")[:, None], v)


@pytest.fixture(scope="module")
def full():
    body = syn.make_body_model(0)
    g = torch.Generator().manual_seed(11)
    B = 64
    pose = torch.randn(B, 165, generator=g) * 0.4
    pose[1] = 0.0
    pose[2, :3] = torch.tensor([0.0, np.pi - 1e-3, 0.0])
    betas = torch.randn(B, 20, generator=g) * 0.7
    transl = torch.randn(B, 3, generator=g)
    f64 = br.lbs_vertices(body, betas, pose, transl, torch.float64).numpy()
    f32 = br.lbs_vertices(body, betas, pose, transl, torch.float32, DEV).cpu().numpy()
    return types.SimpleNamespace(body=body, pose=pose.to(DEV), betas=betas.to(DEV), transl=transl.to(DEV), f64=f64, f32=f32)


@pytest.mark.parametrize("B", [1, 7, 64])
def test_vertices_at_size(full, B):
    from soar_amd import body
    w = full
    v = body.smplx_vertices(w.body, w.betas[:B], w.pose[:B], w.transl[:B])
    assert v.shape == (B, 10475, 3)
    br.bar_check(f"vertices V=10475 B={B}", v, w.f32[:B], w.f64[:B])
    assert torch.equal(v, body.smplx_vertices(w.body, w.betas[:B], w.pose[:B], w.transl[:B]))         # two runs
    # a frame alone equals the frame inside the batch, wherever it sits
    for k in sorted({0, B // 2, B - 1}):
        one = body.smplx_vertices(w.body, w.betas[k:k + 1], w.pose[k:k + 1], w.transl[k:k + 1])
        assert torch.equal(one[0], v[k]), k
    # one betas row for all frames
    vb = body.smplx_vertices(w.body, w.betas[:1], w.pose[:B], w.transl[:B])
    assert torch.equal(vb[0], v[0])
    br.bar_check(f"vertices shared betas B={B}", vb, br.lbs_vertices(w.body, w.betas[:1].cpu(), w.pose[:B].cpu(), w.transl[:B].cpu(),
                                                                     torch.float32).numpy(),
                 br.lbs_vertices(w.body, w.betas[:1].cpu(), w.pose[:B].cpu(), w.transl[:B].cpu()).numpy())


def test_vertices_accept_a_strided_pose(full):
    from soar_amd import body
    w = full
    wide = torch.zeros(7, 330, device=DEV)
    wide[:, ::2] = w.pose[:7]
    assert not wide[:, ::2].is_contiguous()
    assert torch.equal(body.smplx_vertices(w.body, w.betas[:7], wide[:, ::2], w.transl[:7]),
                       body.smplx_vertices(w.body, w.betas[:7], w.pose[:7], w.transl[:7]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        body.smplx_vertices(w.body, w.betas[:7], w.pose[:7].cpu(), w.transl[:7])


def test_pose_correctives_and_the_unchanged_default():
    from soar_amd.smpl_guidance import SMPLGuidance
    body = syn.make_body_model(0)
    parms = _smpl_parms(syn.make_pose_sequence(6, 0))
    guide = SMPLGuidance(body, parms, device=DEV)
    assert not any(hasattr(guide, a) for a in ("query_points", "init_q", "cano_mesh"))
    # the parent commit's three lines
    betas0 = guide._betas(guide.smpl_parms, 0)
    cpose = torch.zeros(1, 165, device=DEV)
    cpose[:, 5], cpose[:, 8] = 30.0 / 180 * np.pi, -30.0 / 180 * np.pi
    A_cano = guide._jt(betas0, cpose, guide.cano_transl)
    v_shaped = body.v_template.to(DEV) + torch.einsum("bl,mkl->bmk", betas0, body.shapedirs.to(DEV))[0]
    Tm = torch.einsum("vj,jxy->vxy", guide.ori_lbs[0], A_cano[0])
    want = (torch.einsum("vxy,vy->vx", Tm[:, :3, :3], v_shaped) + Tm[:, :3, 3]).contiguous()
    assert torch.equal(guide.cano_vertices, want)
    assert torch.equal(guide.inv_mats, torch.linalg.inv(A_cano))

    pc = SMPLGuidance(body, parms, device=DEV, pose_correctives=True)
    args = (body, betas0.cpu(), cpose.cpu(), guide.cano_transl.cpu())
    f64 = br.lbs_vertices(*args).numpy()[0]
    br.bar_check("cano_vertices with correctives", pc.cano_vertices, br.lbs_vertices(*args, torch.float32).numpy()[0], f64)
    assert 1e-4 < float((pc.cano_vertices - guide.cano_vertices).abs().max()) < 1e-2        # the correctives are there, and small
    assert torch.equal(pc.inv_mats, guide.inv_mats)
    # live vertices of stored frames
    live = guide.vertices([0, 3, 5])
    sel = [guide._select(None, i, False) for i in (0, 3, 5)]
    cat = [torch.cat([s[k] for s in sel]).cpu() for k in range(3)]
    br.bar_check("live vertices", live, br.lbs_vertices(body, *cat, torch.float32).numpy(), br.lbs_vertices(body, *cat).numpy())
    assert torch.equal(guide.vertices(3)[0], live[1])


MESHES = {"closed": lambda: br.icosphere(5), "open": br.open_strip, "nonmanifold": br.nonmanifold}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_subdivision_equals_the_restatement(name):
    from soar_amd import body
    v, f = MESHES[name]()
    if name == "closed":
        assert v.shape[0] == 10242
        v = (v * np.array([0.31, 0.87, 0.23], np.float32) + np.array([0.1, -0.3, 0.05], np.float32)).astype(np.float32)   # no symmetric floats
    wv, wf = v, f
    for _ in range(2):
        wv, wf = br.subdivide_np(wv, wf)
    gv, gf = body.subdivide(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), levels=2)
    assert gf.dtype == torch.int32 and gv.dtype == torch.float32
    assert np.array_equal(gf.cpu().numpy(), wf)
    assert np.array_equal(gv.cpu().numpy().view(np.uint32), wv.view(np.uint32))
    gv2, gf2 = body.subdivide(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), levels=2)
    assert torch.equal(gv, gv2) and torch.equal(gf, gf2)
    # int64 faces are taken too; a face out of range is refused
    a, b = body.subdivide(torch.from_numpy(v).to(DEV), torch.from_numpy(f).long().to(DEV), levels=1)
    w1v, w1f = br.subdivide_np(v, f)
    assert np.array_equal(a.cpu().numpy(), w1v) and np.array_equal(b.cpu().numpy(), w1f)
    from soar_amd.hip_lib import SoarHipError
    bad = torch.from_numpy(f).to(DEV).clone()
    bad[-1, 1] = v.shape[0]
    with pytest.raises(SoarHipError, match="outside"):
        body.subdivide(torch.from_numpy(v).to(DEV), bad)
    with pytest.raises(SoarHipError, match="outside"):
        body.vertex_normals(torch.from_numpy(v).to(DEV), bad)


@pytest.mark.parametrize("weighting", ["angle", "area", "uniform"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_normals_and_frames(name, weighting):
    from soar_amd import body
    v, f = MESHES[name]()
    if name == "closed":
        v = (v * np.array([0.31, 0.87, 0.23], np.float32)).astype(np.float32)
        f = np.concatenate([f, [[5, 5, 9], [7, 8, 8]]]).astype(np.int32)                   # two zero-area faces
    tv, tf = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    n = body.vertex_normals(tv, tf, weighting)
    n64 = br.vertex_normals_np(v, f, weighting, np.float64)
    br.bar_check(f"normals {name} {weighting}", n, br.vertex_normals_np(v, f, weighting, np.float32), n64)
    assert torch.equal(n, body.vertex_normals(tv, tf, weighting))
    if name == "open":
        assert torch.equal(n[-2:], torch.zeros(2, 3, device=DEV))                           # vertices no face uses
    P = v.shape[0]
    rd = torch.randn(P, 3, generator=torch.Generator().manual_seed(5))
    rd[0] = 2.0 * n[0].cpu()                                                                 # parallel to the normal
    rd[1] = 0.0
    q = body.surfel_frames(n, rd.to(DEV))
    assert q.shape == (P, 4) and bool(torch.isfinite(q).all())
    assert float((q.norm(dim=1) - 1).abs().max()) <= 1e-6
    assert torch.equal(q, body.surfel_frames(n, rd.to(DEV)))
    # the matrix of each quaternion is the frame the restatement builds from the SAME (float32) normals
    ncpu = n.cpu().numpy()
    M64 = br.frames_np(ncpu, rd.numpy(), np.float64)
    M32 = br.frames_np(ncpu, rd.numpy(), np.float32)
    ok = np.abs(np.linalg.det(M64) - 1) < 1e-6                                              # proper frames (not the degenerate rows)
    assert ok.sum() >= P - 4 - (2 if name == "open" else 0)
    Mq = br.quat_to_mat_np(q.cpu().numpy())
    br.bar_check(f"frames {name} {weighting}", Mq[ok], M32[ok], M64[ok])
    br.bar_check(f"frame normals {name} {weighting}", Mq[ok][:, :, 2], ncpu[ok], ncpu[ok].astype(np.float64))
    # degenerate rows: zero in-plane axes in the restatement (normalize's epsilon), a finite unit quaternion here
    assert np.array_equal(M64[0][:, :2], np.zeros((3, 2))) and np.array_equal(M64[1][:, :2], np.zeros((3, 2)))
    # default rand_dir: drawn from the generator, reproducible
    qa = body.surfel_frames(n, generator=torch.Generator().manual_seed(9))
    qb = body.surfel_frames(n, generator=torch.Generator().manual_seed(9))
    assert torch.equal(qa, qb) and not torch.equal(qa, q)


def test_guidance_initialises_a_model_end_to_end():
    from soar_amd import body as body_ops
    from soar_amd.geometry import GaussianSurfelModel
    from soar_amd.renderer import cameras, registry
    from soar_amd.smpl_guidance import SMPLGuidance
    import soar_amd.renderer  # noqa: F401
    V = 2562
    sv, sf = br.icosphere(4)
    body = syn.make_body_model(0, V=V)
    # a closed surface with the body model's vertex count: the capsule samples carry no faces, so the template is the sphere,
    # squeezed to the body's proportions
    body.v_template = torch.from_numpy(sv * np.array([0.25, 0.8, 0.2], np.float32)).contiguous()
    parms = _smpl_parms(syn.make_pose_sequence(4, 0))
    guide = SMPLGuidance(body, parms, device=DEV, faces=torch.from_numpy(sf), num_subdiv=1, pose_correctives=True,
                         generator=torch.Generator().manual_seed(3))
    again = SMPLGuidance(body, parms, device=DEV, faces=torch.from_numpy(sf), num_subdiv=1, pose_correctives=True,
                         generator=torch.Generator().manual_seed(3))
    P = V + 3 * sf.shape[0] // 2
    assert guide.query_points.shape == (1, P, 3) and guide.init_q.shape == (P, 4) and guide.cano_mesh.faces.shape == (4 * sf.shape[0], 3)
    assert torch.equal(guide.query_points, again.query_points) and torch.equal(guide.init_q, again.init_q)
    assert torch.equal(guide.query_points[0, :V], guide.cano_vertices)
    m = GaussianSurfelModel({})
    m.create_from_pcd(guide.query_points[0], torch.full((P, 3), 0.5), 10, smpl_guidance=guide)
    assert torch.equal(m._rotation.detach(), guide.init_q)
    q = guide.query_points[0]
    box = torch.stack([q.min(0).values, q.max(0).values])
    c = box.mean(0)
    assert torch.equal(m.aabb, (box - c) * 1.5 + c)
    # the model's normals are the vertex normals that went into init_q: the third column of each quaternion's matrix.  The
    # yardstick is the normals themselves (distance 0), so the floor of the bar decides: 1e-6 of a unit vector.  (The skinned test
    # sphere is crumpled -- its skinning weights belong to another surface -- so the normals' own float32 error is not small here;
    # test_normals_and_frames holds them against float64 on well-shaped meshes.)
    normals = body_ops.vertex_normals(*guide.cano_mesh)
    br.bar_check("model normals", m.get_normal.detach(), normals, normals.double())
    m.training_setup()           # as the reference does after create_from_pcd: the renderer reads the config it completes
    assert torch.equal(m._rotation.detach(), guide.init_q)
    root, mats, scale = guide(m.get_xyz.detach(), idx=0)
    assert mats.shape == (1, P, 4, 4) and bool(torch.isfinite(mats).all())
    spec = syn.make_camera(160, 120, distance=3.0, elevation=0.1, azimuth=0.4)
    cam = cameras.Camera(FoVx=spec.fovx, FoVy=spec.fovy, camera_center=spec.camera_center.to(DEV), image_width=160, image_height=120,
                         world_view_transform=spec.world_view_transform.to(DEV), full_proj_transform=spec.full_proj_transform.to(DEV),
                         prcppoint=spec.prcppoint.to(DEV))
    with torch.no_grad():
        out = registry.find("gaussiansurfel-rasterizer")({"use_explicit": True}, geometry=m)(cam, torch.zeros(3, device=DEV), gt=True,
                                                                                             gt_index=0)
    assert bool(torch.isfinite(out["mask"]).all()) and float((out["mask"] > 0.01).sum()) > 10      # opacities start at 0.1
