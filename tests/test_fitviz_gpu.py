"""GPU tests of the fit inspection (soar_amd/fitviz.py, csrc/fitviz.hip) against the NumPy restatement of
tests/fitviz_ref.py.  The strips are compared bit for bit: the kernels use integers and un-contracted float32 only.  The shapes are
the smallest that reach every edge: W = 70, H = 45 is a multiple of no tile (64 x 16) and of no store word (a row of the strip is
1050 bytes, a panel 210), two tiles wide and three high."""
import os
import types

import numpy as np
import pytest
import torch

import fitviz_ref as fr
from test_smplify_cpu import golden, golden_call

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
W, H, N = 70, 45, 3


def dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV, dtype)


@pytest.fixture(scope="module")
def scene():
    """Hand-placed keypoints (frame 0), random ones (frames 1, 2), random normal images and photographs."""
    gen = np.random.default_rng(11)
    nan = np.nan
    target0 = [(1, 1), (0, 5), (W - 1, 20), (W + 2, 30), (W + 3, 40), (-5, 10), (nan, 10), (1e9, 10), (30, 30), (64, 16),
               (20, 35), (40, 35), (33.9, 8.2), (50, 44), (12, 0.5), (63, 31)]
    fit0 = [(8, 12), (5, 0), (W - 1, 24), (W + 2, 33), (10, -1e9), (6, 40), (25, nan), (10, np.inf), (30, 31), (55, 25),
            (20, 35), (43, 35), (34.1, 9.9), (52, 47), (1, 44), (65, 32)]
    K = len(target0)
    target = np.stack([np.array(target0, np.float32)] + [gen.uniform(-8, W + 8, (K, 2)).astype(np.float32) for _ in range(2)])
    fit = np.stack([np.array(fit0, np.float32)] + [target[n] + gen.normal(0, 3, (K, 2)).astype(np.float32) for n in (1, 2)])
    target[1:, :, 1] *= np.float32(H / W)
    fit[1:, :, 1] *= np.float32(H / W)
    kp_mask = np.ones(K, np.float32)
    kp_mask[8] = 0                                                          # (30, 30) / (30, 31): masked out
    prior = gen.uniform(-1, 1, (N, 3, 2, 3, H, W)).astype(np.float32)
    prior[0, 0, 0, :, 0, :4] = np.array([1.0, -1.0, 0.0, 1e-8], np.float32)
    mask = (gen.uniform(0, 1, (N, 3, 2, H, W)) > 0.4).astype(np.uint8)
    mask[0, 0, 0, 0, :4] = 1
    imgs = gen.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    # limbs: one of length 0 (a keypoint with itself), one leaving the image (keypoint 3 lies right of it), one with an end that is
    # not drawn (keypoint 1: x = 0), one masked out, long diagonals, and two ends with one centre in the fit set (10)
    limbs = np.array([[9, 9], [10, 3], [10, 1], [8, 11], [0, 13], [2, 14], [10, 11], [12, 15]], np.int32)
    limb_rgb = gen.integers(1, 256, (len(limbs), 3)).astype(np.uint8)
    return types.SimpleNamespace(K=K, target=target, fit=fit, kp_mask=kp_mask, prior=prior, mask=mask, imgs=imgs, limbs=limbs,
                                 limb_rgb=limb_rgb, d_target=dev(target), d_fit=dev(fit), d_prior=dev(prior), d_mask=dev(mask),
                                 d_imgs=dev(imgs))


def hip_strips(s, sl=slice(None), imgs=None, **kw):
    from soar_amd import fitviz
    out = fitviz.draw_strips(s.d_target[sl], s.d_fit[sl], dev(s.kp_mask), s.d_prior[sl], s.d_mask[sl], imgs=imgs, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def assert_same(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} bytes differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


CASES = {
    "plain": dict(),
    "imgs": dict(with_imgs=True),
    "limbs": dict(limbs=True),
    "limbs_imgs_thick": dict(limbs=True, with_imgs=True, thickness=7, radius=5),
    "radius_1": dict(radius=1, thickness=1, limbs=True),
    "radius_8": dict(radius=8),
    "half": dict(half=True, with_imgs=True, limbs=True),
    "colours": dict(target_rgb=(7, 200, 255), fit_rgb=(255, 255, 1)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_strips_equal_the_restatement(scene, case):
    s, kw = scene, dict(CASES[case])
    with_imgs, limbs = kw.pop("with_imgs", False), kw.pop("limbs", False)
    if limbs:
        kw.update(limbs=s.limbs, limb_rgb=s.limb_rgb)
    kw.setdefault("half", False)
    got = hip_strips(s, imgs=s.d_imgs if with_imgs else None, **kw)
    want = fr.strips(s.target, s.fit, s.kp_mask, s.prior, s.mask, imgs=s.imgs if with_imgs else None, **kw)
    assert want.shape == ((N, H // 2, 5 * W // 2, 3) if kw["half"] else (N, H, 5 * W, 3))
    assert_same(got, want, case)


def test_the_hand_placed_facts_of_frame_zero(scene):
    """What the restatement is checked for on the host, read off the kernel's own strip."""
    got = hip_strips(scene, half=False)[0]
    p0, p1 = got[:, :W], got[:, W:2 * W]
    green, red = np.array([0, 255, 0]), np.array([255, 0, 0])
    is_green, is_red = (p0 == green).all(-1), (p0 == red).all(-1)
    assert is_green[1, 1] and is_green[0, 0] and is_green[4, 1] and not is_green[5, 1]              # (1, 1): drawn, clipped
    assert not (is_green | is_red)[6:9, 0:4].any()                                                   # (0, 5) draws nothing
    assert is_green[17:21, W - 1].all() and is_green[20, W - 4] and is_red[21:28, W - 1].all()       # (W - 1, 20) under (W - 1, 24)
    assert is_green[29:32, W - 1].all() and not is_green[29:32, W - 2].any()                         # (W + 2, 30): column W - 1 only
    assert not (is_green | is_red)[37:44, W - 4:].any()                                              # (W + 3, 40): nothing
    assert not (is_green | is_red)[27:35, 27:34].any()                                               # the masked keypoint
    assert is_green[16, 61:68].all() and is_green[13, 63:66].all() and is_green[19, 63:66].all()     # across both tile edges
    assert is_red[35, 17:24].all() and not is_green[32:39, 17:24].any()                              # red over green, offset 0
    assert is_red[35, 40:47].all() and is_green[35, 37:40].all()                                     # ... offset 3
    assert is_red[44, 51:54].all() and not is_red[44, 50] and not is_red[43, 52]                     # (52, 47): its top row only
    # the discs at x = W - 1 leave panel 1's first columns as the normal render has them
    want = fr.normal_bytes(scene.prior[0, 0, 0], scene.mask[0, 0, 0])
    assert np.array_equal(p1, want)
    assert want[0, :4, 0].tolist() == [255, 0, 127, 127]


def test_a_strided_photograph(scene):
    s = scene
    big = torch.zeros((N, H + 2, W + 3, 4), dtype=torch.uint8, device=DEV)
    view = big[:, 1:H + 1, 2:W + 2, 1:]
    view.copy_(s.d_imgs)
    assert not view.is_contiguous()
    assert_same(hip_strips(s, imgs=view), fr.strips(s.target, s.fit, s.kp_mask, s.prior, s.mask, imgs=s.imgs), "strided imgs")
    flipped = s.d_imgs.flip(-1)                                             # (a copy: flip is no view)
    bgr = torch.empty((N, 3, H, W), dtype=torch.uint8, device=DEV).copy_(flipped.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert bgr.stride(3) == H * W
    assert_same(hip_strips(s, imgs=bgr, half=True), fr.strips(s.target, s.fit, s.kp_mask, s.prior, s.mask, imgs=s.imgs[..., ::-1], half=True),
                "planar imgs, halved")


def test_a_frame_alone_equals_the_frame_in_the_batch(scene):
    s = scene
    kw = dict(limbs=s.limbs, limb_rgb=s.limb_rgb)
    for half in (False, True):
        batch = hip_strips(s, imgs=s.d_imgs, half=half, **kw)
        alone = hip_strips(s, slice(1, 2), imgs=s.d_imgs[1:2], half=half, **kw)
        assert_same(alone[0], batch[1], f"frame 1 alone, half={half}")


@pytest.mark.parametrize("w,h,half", [(70, 45, False), (35, 9, True), (129, 17, True), (64, 16, False), (1, 2, True), (3, 1, False)])
def test_137_random_keypoints(w, h, half):
    """K = 137 (two culling chunks of 256 primitives with limbs), odd widths whose 2 x 2 blocks straddle two panels, a width of
    exactly one tile, and the smallest images."""
    from soar_amd import fitviz
    gen = np.random.default_rng(w * 100 + h)
    K, n = 137, 2
    target = gen.uniform(-6, max(w, h) + 6, (n, K, 2)).astype(np.float32)
    target[..., 1] = gen.uniform(-6, h + 6, (n, K)).astype(np.float32)
    fit = target + gen.normal(0, 2.5, (n, K, 2)).astype(np.float32)
    kp_mask = (gen.uniform(0, 1, K) > 0.1).astype(np.float32)
    prior = gen.uniform(-1, 1, (n, 3, 2, 3, h, w)).astype(np.float32)
    mask = (gen.uniform(0, 1, (n, 3, 2, h, w)) > 0.5).astype(np.uint8)
    imgs = gen.integers(0, 256, (n, h, w, 3)).astype(np.uint8)
    limbs = gen.integers(0, K, (200, 2)).astype(np.int32)
    limb_rgb = gen.integers(0, 256, (200, 3)).astype(np.uint8)
    got = fitviz.draw_strips(dev(target), dev(fit), dev(kp_mask), dev(prior), dev(mask), imgs=dev(imgs), limbs=limbs, limb_rgb=limb_rgb,
                             thickness=2, half=half)
    want = fr.strips(target, fit, kp_mask, prior, mask, imgs=imgs, limbs=limbs, limb_rgb=limb_rgb, thickness=2, half=half)
    assert_same(got.cpu().numpy(), want, f"K=137 {w}x{h} half={half}")


def test_the_python_side_refuses(scene):
    from soar_amd import fitviz
    s = scene
    big = torch.zeros((1, 513, 2), device=DEV)
    with pytest.raises(ValueError, match="512"):
        fitviz.draw_strips(big, big, torch.ones(513), s.d_prior[:1], s.d_mask[:1])
    with pytest.raises(ValueError, match="radius"):
        fitviz.draw_strips(s.d_target, s.d_fit, dev(s.kp_mask), s.d_prior, s.d_mask, radius=0)
    with pytest.raises(ValueError, match="outside"):
        fitviz.draw_strips(s.d_target, s.d_fit, dev(s.kp_mask), s.d_prior, s.d_mask, limbs=[[0, s.K]], limb_rgb=[[1, 1, 1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fitviz.draw_strips(s.d_target.cpu(), s.d_fit, dev(s.kp_mask), s.d_prior, s.d_mask)
    empty = fitviz.draw_strips(s.d_target[:0], s.d_fit[:0], dev(s.kp_mask), s.d_prior[:0], s.d_mask[:0])
    assert empty.shape == (0, H, 5 * W, 3)


# ---- yaw views ---------------------------------------------------------------------------------------------------------------------

def tilted_camera():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smplify.npz"))
    return g["w2c"].astype(np.float32)


def test_yaw_views():
    from soar_amd import fitviz
    gen = np.random.default_rng(3)
    n, V = 3, 301                                                           # more than one block of 256
    verts = (gen.normal(size=(n, V, 3)) * [0.4, 0.8, 0.3] + [0.1, -0.2, 3.0]).astype(np.float32)
    pivot = (verts.mean(1) + gen.normal(size=(n, 3)) * 0.05).astype(np.float32)
    w2c = tilted_camera()
    R = fitviz.yaw_matrices(w2c, 3)
    d_verts = dev(verts)
    out = fitviz.yaw_views(d_verts, dev(pivot), w2c, 3)
    assert out.shape == (n, 3, V, 3) and torch.equal(out[:, 0], d_verts)    # view 0: bit for bit
    got = out.cpu().numpy()
    want = fr.yaw_views(verts, pivot, R)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    bound = 8 * 2.0 ** -23 * max(1.0, float(np.abs(verts).max()), float(np.abs(pivot).max()))
    err = float(np.abs(got - fr.yaw_views64(verts, pivot, R)).max())
    print(f"yaw views against float64: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    assert float(np.abs(got[:, 1] - got[:, 0]).max()) > 0.1                 # the views do turn
    # strided vertices, other view counts, and a frame alone
    wide = torch.zeros((n, V, 5), device=DEV)
    wide[..., 1:4] = d_verts
    assert torch.equal(fitviz.yaw_views(wide[..., 1:4], dev(pivot), w2c, 3), out)
    assert torch.equal(fitviz.yaw_views(d_verts[1:2], dev(pivot[1:2]), w2c, 3)[0], out[1])
    four = fitviz.yaw_views(d_verts, dev(pivot), w2c, 4).cpu().numpy()
    assert np.array_equal(four, fr.yaw_views(verts, pivot, fitviz.yaw_matrices(w2c, 4)))
    one = fitviz.yaw_views(d_verts, dev(pivot), w2c, 1)
    assert one.shape == (n, 1, V, 3) and torch.equal(one[:, 0], d_verts)


def icosahedron():
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
                  (-t, 0, -1), (-t, 0, 1)], np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int32)
    return v / np.linalg.norm(v[0]), f


def test_the_normal_panels_are_the_renderer_on_the_yaw_views():
    """Panels 1 - 4 against ``render_normal_priors`` run here on ``yaw_views``' own output, pushed through the restatement's byte
    rule: the same float images go in both ways, so there is no tolerance."""
    from soar_amd import fitviz, prior
    v, f = icosahedron()
    n = 2
    verts = np.stack([v * [0.5, 0.9, 0.5] + [0.05, -0.1, 3.0], v * 0.7 + [-0.3, 0.2, 3.4]]).astype(np.float32)
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, :3] = tilted_camera()[:3, :3]
    Ks = np.array([[[60.0, 0, 35.0], [0, 60.0, 22.5], [0, 0, 1]], [[75.0, 0, 30.0], [0, 70.0, 25.0], [0, 0, 1]]], np.float32)
    topo = prior.MeshTopology(f, 12, device=DEV)
    pivot = dev(verts.mean(1))
    views = fitviz.yaw_views(dev(verts), pivot, w2c, 3)
    pr = prior.render_normal_priors(topo, views.reshape(3 * n, 12, 3), dev(w2c), dev(Ks).repeat_interleave(3, dim=0), (W, H))
    gen = np.random.default_rng(4)
    imgs = gen.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    none = torch.zeros((n, 0, 2), device=DEV)
    p, m = pr["prior"].cpu().numpy(), pr["mask"].cpu().numpy()
    assert m.reshape(n, 3, 2, H, W)[:, :, 0].reshape(n * 3, -1).sum(1).min() > 100          # every view shows the body
    for photo in (None, imgs):
        got = fitviz.draw_strips(none, none, torch.ones(0), pr["prior"], pr["mask"], imgs=None if photo is None else dev(photo)).cpu().numpy()
        want = fr.strips(np.zeros((n, 0, 2), np.float32), np.zeros((n, 0, 2), np.float32), np.ones(0), p, m, imgs=photo)
        assert_same(got, want, "normal panels")
        for k in range(3):
            assert_same(got[:, :, (2 + k) * W:(3 + k) * W], np.stack([fr.normal_bytes(p.reshape(n, 3, 2, 3, H, W)[i, k, 0],
                        m.reshape(n, 3, 2, H, W)[i, k, 0]) for i in range(n)]), f"panel {2 + k}")
        if photo is None:
            assert np.array_equal(got[:, :, W:2 * W], got[:, :, 2 * W:3 * W]) and not got[:, :, :W].any()
        assert not np.array_equal(got[:, :, 2 * W:3 * W], got[:, :, 3 * W:4 * W])


# ---- residuals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [137, 512, 5])
def test_fit_residuals(K):
    from soar_amd import fitviz
    gen = np.random.default_rng(K)
    n = 4
    f, t = gen.uniform(0, 1900, (n, K, 2)).astype(np.float32), gen.uniform(0, 1900, (n, K, 2)).astype(np.float32)
    conf = gen.uniform(0, 1, (n, K)).astype(np.float32)
    conf[2] = 0.3                                                           # not above the threshold: a frame with none
    conf[0, 1] = 0.9
    f[0, 1, 0] = np.nan
    t[0, 2, 1] = np.inf
    mask = np.ones(K, np.float32)
    mask[4] = 0
    got = fitviz.fit_residuals(dev(f), dev(t), dev(conf), dev(mask)).cpu().numpy()
    r32, r64 = fr.residuals(f, t, conf, mask), fr.residuals64(f, t, conf, mask)
    assert got.shape == (n, 3) and got.dtype == np.float32
    assert np.array_equal(got[:, 0], r64[:, 0]) and got[2].tolist() == [0.0, 0.0, 0.0] and got[0, 0] > 0
    rel = np.abs(got[:, 1] - r64[:, 1]) / np.maximum(r64[:, 1], 1e-30)
    ulps = np.abs(got[:, 2].astype(np.float64) - r64[:, 2]) / np.spacing(r64[:, 2].astype(np.float32)).astype(np.float64)
    print(f"K={K}: mean rel {rel.max():.3e} (bound {16 * 2.0 ** -24:.3e}), max {ulps.max():.2f} ulps")
    assert rel[[0, 1, 3]].max() <= 16 * 2.0 ** -24
    assert ulps[[0, 1, 3]].max() <= 2.0
    assert np.array_equal(got.view(np.uint32), r32.view(np.uint32))         # the header's order of additions
    alone = fitviz.fit_residuals(dev(f[1:2]), dev(t[1:2]), dev(conf[1:2]), dev(mask)).cpu().numpy()
    assert np.array_equal(alone[0], got[1])


# ---- the whole stage -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fitted():
    """The rig and body of the smplify tests, three of the golden frames as fitted parameters, a quarter-size image."""
    from soar_amd import prior, smplify
    g, m, p, i, tables = golden()
    rig = smplify.KeypointRig.from_body_model(m, *tables, device=DEV)
    c = golden_call(g)
    sel = [0, 1, 2]
    params = smplify.SMPLify._rotvec_params({k: (v if k == "betas" else v[sel]).to(DEV) for k, v in p.items()})
    Ks = c["Ks"][sel].clone()
    Ks[:, :2] *= 0.25
    topo = prior.MeshTopology(m.faces_tensor, m.v_template.shape[0], device=DEV)
    imgs = torch.randint(0, 256, (3, 120, 160, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(DEV)
    return types.SimpleNamespace(rig=rig, body=m, topo=topo, params=params, Ks=Ks.to(DEV), w2c=c["w2c"].to(DEV), img_wh=(160, 120),
                                 target=c["target_kps"][sel].to(DEV), imgs=imgs)


def test_fit_strips_in_chunks(fitted):
    from soar_amd import fitviz, smplify
    w = fitted
    call = lambda **kw: fitviz.fit_strips(w.rig, w.body, w.topo, w.params, w.Ks, w.w2c, w.img_wh, w.target, imgs=w.imgs, **kw)
    two, three = call(chunk=2), call(chunk=3)
    assert two["strips"].shape == (3, 120, 800, 3) and two["strips"].dtype == torch.uint8
    assert torch.equal(two["strips"], three["strips"]) and torch.equal(two["residuals"], three["residuals"])
    assert torch.equal(call(chunk=1)["strips"], three["strips"])
    # the strip is made of what it says: the projected keypoints, the target times img_wh, the renderer on the yaw views
    six = fitviz._six_d(w.params)
    fit_px = smplify.project_keypoints(w.rig, six, w.Ks, w.w2c).cpu().numpy()
    t = w.target.cpu().numpy()
    target_px = (t[..., :2] * np.array([160.0, 120.0], np.float32)).astype(np.float32)
    res = fr.residuals(fit_px, target_px, t[..., 2], w.rig.kp_mask.cpu().numpy())
    assert np.array_equal(three["residuals"].cpu().numpy(), res) and res[:, 0].min() > 0
    strips = three["strips"].cpu().numpy()
    bare = fitviz.fit_strips(w.rig, w.body, w.topo, w.params, w.Ks, w.w2c, w.img_wh, w.target)["strips"].cpu().numpy()
    want0 = np.stack([fr.keypoint_panel(120, 160, target_px[n], fit_px[n], w.rig.kp_mask.cpu().numpy()) for n in range(3)])
    assert_same(bare[:, :, :160], want0, "panel 0 of fit_strips")
    assert_same(strips[:, :, :160], fr.blend(want0, w.imgs.cpu().numpy()), "panel 0 of fit_strips over the photograph")
    for k in range(3):
        assert (bare[:, :, (2 + k) * 160:(3 + k) * 160].reshape(3, -1) != 0).sum(1).min() > 50, k        # the body shows in every view
    assert np.array_equal(bare[:, :, 160:320], bare[:, :, 320:480])
    halved = call(half=True)["strips"].cpu().numpy()
    assert_same(halved, np.stack([fr.halve(x) for x in strips]), "halved fit_strips")


def test_the_visualizer_writes_what_it_drew(fitted, tmp_path):
    from PIL import Image
    from soar_amd import fitviz
    w = fitted
    vis = fitviz.FitVisualizer(w.rig, w.body, w.topo, str(tmp_path), imgs=w.imgs, chunk=2)
    assert vis.debug is False
    vis("1_000", w.params, w.Ks, w.w2c, w.img_wh, w.target)
    want = fitviz.fit_strips(w.rig, w.body, w.topo, w.params, w.Ks, w.w2c, w.img_wh, w.target, imgs=w.imgs)
    names = sorted(os.listdir(tmp_path / "1_000"))
    assert names == ["00000.png", "00001.png", "00002.png"]
    for n, name in enumerate(names):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "1_000" / name)), want["strips"][n].cpu().numpy())
    assert np.array_equal(vis.residuals["1_000"], want["residuals"].cpu().numpy())


def test_fit_calls_the_visualizer(fitted, tmp_path):
    """One short fit on the HIP objective with a FitVisualizer: the names of the reference, and the same parameters as an unwatched fit."""
    from soar_amd import fitviz, smplify
    w = fitted
    start = {k: v.clone() for k, v in w.params.items()}
    start["betas"] = start["betas"].expand(3, -1)
    steps = dict(body_steps=1, hand_steps=1, max_iters=2)
    vis = fitviz.FitVisualizer(w.rig, w.body, w.topo, str(tmp_path))
    watched = smplify.SMPLify(w.rig, **steps).fit(start, w.Ks, w.w2c, w.img_wh, w.target, visual=vis)
    plain = smplify.SMPLify(w.rig, **steps).fit(start, w.Ks, w.w2c, w.img_wh, w.target)
    assert sorted(os.listdir(tmp_path)) == ["1_000", "2_000"] == list(vis.residuals)       # ("1_000" before and after step 0)
    for k in plain:
        assert torch.equal(plain[k], watched[k]), k
