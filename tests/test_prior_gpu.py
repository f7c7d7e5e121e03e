"""GPU tests of the normal priors (csrc/prior.hip, soar_amd/prior.py) against the NumPy restatement of
tests/prior_ref.py: the projection, visibility bit for bit outside the near-tie set, shading against float64 under the project's
bar (4 x the float32 restatement's own error, floor 1e-6), reproducibility, and the whole stage.

Measured on an MI355X (worst element over the largest magnitude; the HIP path and the float32 restatement give the same figure to
the digits shown, and the same snapped vertices; the bar is 4 x that figure, floor 1e-6):
  case               snapped       inv_z     vertex normals   prior front / rear    | |n| - 1 |
  torus16x10_33x47   0.500 units   6.2e-08   1.2e-07          9.8e-08 / 9.8e-08     1.0e-07
  torus24x12_96x80   0.499 units   6.7e-08   1.6e-07          1.4e-07 / 1.0e-07     1.1e-07
  torus48x24_48x40   0.500 units   7.0e-08   2.7e-07          1.1e-07 / 1.0e-07     1.1e-07
  capsule_130x70     0.499 units   6.8e-08   2.8e-07          1.2e-07 / 1.1e-07     1.1e-07
Near-ties (best and second-best q within 1e-5 relative): 0 of 1551 / 7680 / 1920 / 9100 covered pixels in both views, and 0 of 2130
without the quad; no pixel's face differs from the oracle's.
"""
import numpy as np
import pytest
import torch

import prior_cases as pc
import prior_ref as pr
from soar_amd import prior

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


_cache = {}


def _case(name, dev, quad=True):
    """inputs, the HIP outputs, and the oracle fed with the GPU's own snapped vertices in float64 and float32: computed once, shared,
    left unchanged"""
    key = (name, quad)
    if key not in _cache:
        c = pc.make_case(name, quad)
        c["topo"] = prior.MeshTopology(torch.from_numpy(c["faces"]), c["verts"].shape[0], device=dev)
        c["tv"] = torch.from_numpy(c["verts"])[None].to(dev)
        c["tK"], c["tw2c"] = torch.from_numpy(c["K"])[None].to(dev), torch.from_numpy(c["w2c"]).to(dev)
        out = prior.render_normal_priors(c["topo"], c["tv"], c["tw2c"], c["tK"], (c["W"], c["H"]), debug=True)
        torch.cuda.synchronize()
        c["out"] = out
        c["hip"] = {k: v[0].cpu().numpy() for k, v in out.items()}
        c["v64"] = pr.vertex_setup(c["verts"], c["faces"], c["w2c"], c["K"], np.float64)
        c["v32"] = pr.vertex_setup(c["verts"], c["faces"], c["w2c"], c["K"], np.float32)
        sn = c["hip"]["snapped"].astype(np.int64)
        c["r64"] = pr.rasterize(sn, c["v64"]["inv_z"], c["v64"]["normals"], c["faces"], c["H"], c["W"], np.float64)
        c["r32"] = pr.rasterize(sn, c["v32"]["inv_z"], c["v32"]["normals"], c["faces"], c["H"], c["W"], np.float32)
        _cache[key] = c
    return _cache[key]


def _visibility(c, name):
    """mask bit for bit; face on every pixel outside the near-tie set; at most 0.5 % of the covered pixels left out"""
    hip, r64 = c["hip"], c["r64"]
    assert hip["mask"].dtype == np.uint8 and hip["face"].dtype == np.int32 and hip["prior"].dtype == np.float32
    assert (hip["mask"] == r64["mask"]).all(), name
    ties = pr.near_ties(r64)
    agree = np.ones(ties.shape, bool)
    for view in (0, 1):
        covered, n = int((r64["face"][view] >= 0).sum()), int(ties[view].sum())
        differ = int((hip["face"][view] != r64["face"][view]).sum())
        print(f"{name} view {view}: {n} near-ties of {covered} covered pixels; {differ} pixels differ in face")
        assert n <= 0.005 * covered, (name, view, n, covered)
        agree[view] = ~ties[view] & (hip["face"][view] == r64["face"][view])
        assert (hip["face"][view][~ties[view]] == r64["face"][view][~ties[view]]).all(), (name, view)
    assert ((hip["face"] >= 0) == (hip["mask"] == 1)).all()
    return agree


@pytest.mark.parametrize("name", list(pc.CASES))
def test_projection(name, dev):
    c = _case(name, dev)
    hip, v64, v32 = c["hip"], c["v64"], c["v32"]
    ok = v64["valid"]
    assert ((hip["snapped"][:, 0] != prior.INVALID) == ok).all() and int((~ok).sum()) == 2
    assert (hip["snapped"][~ok] == prior.INVALID).all() and (hip["inv_z"][~ok] == 0).all()
    err = np.abs(hip["snapped"][ok].astype(np.float64) - v64["xy"][ok] * 256)
    print(f"{name}: snapped within {err.max():.3f} units of float64; {int((hip['snapped'] != v32['snapped']).sum())} differ from the float32 restatement")
    assert err.max() <= 1.0
    pr.bar_check(f"{name} inv_z", hip["inv_z"], v32["inv_z"], v64["inv_z"])
    boxes = pr.face_boxes(hip["snapped"].astype(np.int64), c["faces"])
    assert hip["face_boxes"].dtype == np.int16 and (hip["face_boxes"] == boxes).all()
    assert (boxes[:, 0] > boxes[:, 1]).sum() >= 4 and boxes[:, 0].min() < 0                       # empty ones; columns left of the image
    well = v64["well"]                                           # all but the collinear face's and the needle's vertices (test_prior_cpu.py)
    pr.bar_check(f"{name} vertex normals", hip["vertex_normals"][well], v32["normals"][well], v64["normals"][well])
    assert (np.abs(np.linalg.norm(hip["vertex_normals"].astype(np.float64), axis=1) - 1) <= 1e-6).sum() >= well.sum() - 2     # unit; 0 for the two vertices only the repeated-vertex face names


@pytest.mark.parametrize("name", list(pc.CASES))
def test_visibility(name, dev):
    c = _case(name, dev)
    _visibility(c, name)
    # copies of faces come last and never win; their originals do
    front = set(np.unique(c["hip"]["face"][0]).tolist())
    assert max(front) < c["first_copy"] and len(front & set(c["copies_of"])) >= 3
    assert c["hip"]["face"][1].max() < c["first_copy"]


def test_front_and_rear_differ(dev):
    c = _case("torus24x12_96x80", dev, quad=False)
    _visibility(c, "torus24x12_96x80 without the quad")
    hip, r64 = c["hip"], c["r64"]
    on = hip["mask"][0] == 1
    assert (hip["mask"][0] == hip["mask"][1]).all() and 0.2 < on.mean() < 0.9
    assert (hip["face"][0][on] != hip["face"][1][on]).mean() > 0.9
    # the rear view's winner is the farthest layer: the oracle's smallest q over all faces that cover the pixel
    assert (r64["q"][1][on] <= r64["q"][0][on]).all() and (hip["face"][1][on] == r64["face"][1][on]).all()


@pytest.mark.parametrize("name", list(pc.CASES))
def test_shading(name, dev):
    c = _case(name, dev)
    agree = _visibility(c, name)
    hip, r64, r32 = c["hip"], c["r64"], c["r32"]
    for view in (0, 1):
        sel = agree[view] & (r32["face"][view] == r64["face"][view])
        assert sel.sum() >= 0.995 * (r64["face"][view] >= 0).sum()
        pr.bar_check(f"{name} prior view {view}", hip["prior"][view][:, sel], r32["prior"][view][:, sel], r64["prior"][view][:, sel])
    off, on = hip["mask"] == 0, hip["mask"] == 1
    p = np.moveaxis(hip["prior"], 1, -1)                         # [2,H,W,3]
    assert (p[off] == 0).all()
    norm = np.sqrt((p[on].astype(np.float64) ** 2).sum(-1))
    print(f"{name}: |n| - 1 within {np.abs(norm - 1).max():.3e}")
    assert np.abs(norm - 1).max() <= 1e-6
    cv = prior.render_normal_priors(c["topo"], c["tv"], c["tw2c"], c["tK"], (c["W"], c["H"]), space="opencv")
    flip = torch.tensor([1.0, -1.0, -1.0], device=dev).view(1, 1, 3, 1, 1)
    want = c["out"]["prior"] * flip
    assert torch.equal(cv["prior"].view(torch.int32) & 0x7FFFFFFF, want.view(torch.int32) & 0x7FFFFFFF)          # magnitudes bit for bit
    assert torch.equal(cv["prior"], want) and torch.equal(cv["face"], c["out"]["face"]) and torch.equal(cv["mask"], c["out"]["mask"])


def test_off_the_body_is_exactly_zero(dev):
    c = _case("torus24x12_96x80", dev, quad=False)
    off = c["hip"]["mask"] == 0
    assert off.any() and (np.moveaxis(c["hip"]["prior"], 1, -1)[off] == 0).all() and (c["hip"]["face"][off] == -1).all()
    assert (np.signbit(np.moveaxis(c["hip"]["prior"], 1, -1)[off]) == False).all()      # noqa: E712  (+0, under both conventions)


def test_reproducibility(dev):
    c = _case("torus24x12_96x80", dev)
    topo, W, H = c["topo"], c["W"], c["H"]
    keys = ("prior", "mask", "face", "snapped", "inv_z", "vertex_normals", "face_boxes")
    again = prior.render_normal_priors(topo, c["tv"], c["tw2c"], c["tK"], (W, H), debug=True)
    assert all(torch.equal(again[k], c["out"][k]) for k in keys)
    # a frame alone against the same frame at position 2 of a batch of 3 with other vertices and other Ks in front of it
    g = torch.Generator().manual_seed(3)
    verts = torch.cat([c["tv"] + 0.02 * torch.randn(2, *c["tv"].shape[1:], generator=g).to(dev), c["tv"]])
    Ks = c["tK"].repeat(3, 1, 1)
    Ks[0, 0, 0] *= 1.2
    Ks[1, :2, 2] += 3.25
    batch = prior.render_normal_priors(topo, verts, c["tw2c"], Ks, (W, H), debug=True)
    assert all(torch.equal(batch[k][2], c["out"][k][0]) for k in keys)
    assert not torch.equal(batch["face"][0], batch["face"][2]) and not torch.equal(batch["face"][1], batch["face"][2])
    # a strided view against its contiguous copy
    wide = torch.zeros((3, verts.shape[1], 7), device=dev)
    wide[:, :, 1:7:2] = verts
    view = wide[:, :, 1:7:2]
    assert not view.is_contiguous() and view.stride() == (7 * verts.shape[1], 7, 2)
    strided = prior.render_normal_priors(topo, view, c["tw2c"], Ks, (W, H), debug=True)
    assert all(torch.equal(strided[k], batch[k]) for k in keys)
    # one w2c against the same matrix per frame
    per = prior.render_normal_priors(topo, verts, c["tw2c"][None].repeat(3, 1, 1), Ks, (W, H), debug=True)
    assert all(torch.equal(per[k], batch[k]) for k in keys)
    # and a w2c of its own per frame is read per frame
    w2 = c["tw2c"][None].repeat(3, 1, 1)
    w2[1, 0, 3] += 0.1
    per2 = prior.render_normal_priors(topo, verts, w2, Ks, (W, H))
    assert torch.equal(per2["face"][2], batch["face"][2]) and not torch.equal(per2["face"][1], batch["face"][1])


def test_no_frames_no_launch(dev, monkeypatch):
    c = _case("torus16x10_33x47", dev)
    from soar_amd import hip_lib

    def refuse():
        raise AssertionError("the library was asked for with N = 0")
    monkeypatch.setattr(hip_lib, "lib", refuse)
    out = prior.render_normal_priors(c["topo"], c["tv"][:0], c["tw2c"], c["tK"][:0], (c["W"], c["H"]), debug=True)
    assert out["prior"].shape == (0, 2, 3, c["H"], c["W"]) and out["mask"].shape == out["face"].shape == (0, 2, c["H"], c["W"])
    assert out["prior_F"].shape == out["prior_B"].shape == (0, 3, c["H"], c["W"]) and out["snapped"].shape == (0, c["verts"].shape[0], 2)
    assert out["prior"].is_cuda and out["mask"].dtype == torch.uint8 and out["face"].dtype == torch.int32


def test_a_mesh_without_faces_and_a_mesh_off_the_image(dev):
    topo = prior.MeshTopology(np.zeros((0, 3), np.int64), 3, device=dev)
    v = torch.tensor([[[0.0, 0.0, 2.0], [1.0, 0.0, 2.0], [0.0, 1.0, 2.0]]], device=dev)
    K = torch.tensor([[[10.0, 0.0, 4.0], [0.0, 10.0, 4.0], [0.0, 0.0, 1.0]]], device=dev)
    out = prior.render_normal_priors(topo, v, torch.eye(4, device=dev), K, (9, 7))
    assert out["mask"].sum().item() == 0 and (out["face"] == -1).all() and (out["prior"] == 0).all()
    topo = prior.MeshTopology(torch.tensor([(0, 1, 2)]), 3, device=dev)
    out = prior.render_normal_priors(topo, v + torch.tensor([50.0, 0.0, 0.0], device=dev), torch.eye(4, device=dev), K, (9, 7))
    assert out["mask"].sum().item() == 0
    out = prior.render_normal_priors(topo, v, torch.eye(4, device=dev), K, (9, 7))
    # (4, 4), (9, 4), (4, 9) in pixels: the samples with x, y >= 4.5 and x + y < 13, inside 9 x 7
    want = torch.zeros((7, 9), dtype=torch.uint8)
    for i in range(7):
        for j in range(9):
            want[i, j] = int(j >= 4 and i >= 4 and (j + 0.5) + (i + 0.5) <= 13)
    assert torch.equal(out["mask"][0, 0].cpu(), want) and torch.equal(out["mask"][0, 1].cpu(), want)
    # a needle to pixel column 40004: its box is clamped to int16 and it still covers its part of the image
    far = v.clone()
    far[0, 1, 0] = 8000.0
    out = prior.render_normal_priors(topo, far, torch.eye(4, device=dev), K, (9, 7), debug=True)
    assert out["face_boxes"][0, 0].tolist() == [4, 32767, 4, 8]
    want = torch.zeros((7, 9), dtype=torch.uint8)
    want[4:, 4:] = 1
    assert torch.equal(out["mask"][0, 0].cpu(), want)
    out = prior.render_normal_priors(topo, v, torch.eye(4, device=dev), K, (9, 7))
    # the face looks along -z of the camera (its cross product is +z, away from the viewer): (0, 0, 1) in OpenCV, (0, 0, -1) in OpenGL
    assert torch.equal(out["prior"][0, 0, :, 5, 5].cpu(), torch.tensor([0.0, -0.0, -1.0]))


def test_the_stage(dev):
    import normalnet_ref as nref
    from soar_amd import normals
    images, masks, Ks = (t.to(dev) for t in nref.make_frames())
    images = torch.cat([images, images[:2].flip(2)]).contiguous()
    masks = torch.cat([masks, masks[:2].flip(2)]).contiguous()
    Ks = torch.cat([Ks, Ks[:2]])
    net = normals.NormalNet(nref.random_state_dict(8, 2, 1, seed=21, device=dev), 8, 2, 1).to(dev)
    v, f = pc.capsule()
    topo = prior.MeshTopology(f, v.shape[0], device=dev)
    g = torch.Generator().manual_seed(8)
    verts = (torch.from_numpy(v)[None] * 0.4 + 0.01 * torch.randn(5, v.shape[0], 3, generator=g)).to(dev)
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.0, 0.0, 2.0])
    w2c = w2c.to(dev)
    res = prior.estimate_normals_from_body(net, images, masks, Ks, verts, topo, w2c, batch=2)
    image, mask, nKs, _ = normals.crop_frames(images, masks, Ks)
    pri = prior.render_normal_priors(topo, verts, w2c, nKs)
    assert pri["prior_F"].shape == (5, 3, 512, 512) and 0.01 < pri["mask"].float().mean().item() < 0.9
    want = normals.estimate_normals(net, images, masks, Ks, pri["prior_F"], pri["prior_B"], batch=2)
    assert set(res) == set(want)
    for k in want:
        assert torch.equal(res[k], want[k]), k
    # the priors matter: without them the result differs
    zero = torch.zeros_like(pri["prior_F"])
    assert not torch.equal(normals.estimate_normals(net, images, masks, Ks, zero, zero, batch=2)["normal_F"], want["normal_F"])
    m = masks.clone()
    m[3] = 0
    with pytest.raises(ValueError, match="frame 3 has an empty mask"):
        prior.estimate_normals_from_body(net, images, m, Ks, verts, topo, w2c, batch=2)


def test_body_normal_priors(dev):
    from soar_amd import synthetic as syn
    from soar_amd.body import smplx_vertices
    body = syn.make_body_model(0, V=512)
    seq = syn.make_pose_sequence(2, 0)
    fp = seq["full_pose"].to(dev)
    params = {"global_orient": fp[:, :3], "body_pose": fp[:, 3:66], "jaw_pose": fp[:, 66:69], "leye_pose": fp[:, 69:72], "reye_pose": fp[:, 72:75],
              "left_hand_pose": fp[:, 75:120], "right_hand_pose": fp[:, 120:165], "betas": seq["betas"].to(dev),
              "expression": seq["expression"].to(dev), "transl": seq["transl"].to(dev)}
    assert torch.equal(prior.full_pose(params), fp)
    g = torch.Generator().manual_seed(2)
    topo = prior.MeshTopology(torch.stack([torch.randperm(512, generator=g)[:3] for _ in range(300)]), 512, device=dev)
    w2c = torch.eye(4)
    w2c[:3, 3] = torch.tensor([0.0, 0.0, 3.0])
    K = torch.tensor([[40.0, 0.0, 24.0], [0.0, 40.0, 32.0], [0.0, 0.0, 1.0]]).repeat(2, 1, 1)
    out = prior.body_normal_priors(body, params, K.to(dev), w2c.to(dev), topo, img_wh=(48, 64))
    verts = smplx_vertices(body, torch.cat([params["betas"].expand(2, -1), params["expression"]], 1), fp, params["transl"])
    assert torch.equal(out["verts"], verts)
    direct = prior.render_normal_priors(topo, verts, w2c.to(dev), K.to(dev), (48, 64))
    assert torch.equal(out["prior"], direct["prior"]) and out["mask"].float().mean().item() > 0.05
