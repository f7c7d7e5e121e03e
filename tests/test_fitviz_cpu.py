"""CPU tests of the fit inspection (soar_amd/fitviz.py, csrc/fitviz.hip): the NumPy restatement of tests/fitviz_ref.py
against facts worked out by hand, the yaw matrices, the exported symbols and their argument checks, and the ``visual`` hook of
``SMPLify.fit`` on a CPU objective.  Nothing is launched."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import fitviz_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GREEN, RED = (0, 255, 0), (255, 0, 0)


def px(*pts):
    return np.array(pts, np.float32).reshape(-1, 2)


def count(img):
    return int((img != 0).any(-1).sum())


def test_the_disc_of_radius_three_is_37_pixels():
    img = fr.keypoint_panel(21, 21, px((10, 10)), px((-5, -5)), np.ones(1))
    assert count(img) == 37
    assert [(int((img[y] != 0).any(-1).sum())) for y in range(7, 14)] == [3, 5, 7, 7, 7, 5, 3]
    assert (img[img.any(-1)] == GREEN).all()
    # truncation toward zero: 10.99 is 10, and the target's confidence plays no part
    assert np.array_equal(img, fr.keypoint_panel(21, 21, px((10.99, 10.5)), px((np.nan, 3)), np.ones(1)))


def test_a_limb_of_ten_pixels_and_thickness_four_is_63_pixels():
    img = np.zeros((21, 31, 3), np.uint8)
    fr.paint_limb(img, (10, 10), (20, 10), 4, (9, 9, 9))
    assert count(img) == 63 == 11 * 5 + 2 * 4
    assert img[8:13, 10:21].all()                                          # the 11 x 5 block
    for x, ys in ((9, (9, 10, 11)), (8, (10,)), (21, (9, 10, 11)), (22, (10,))):
        assert [y for y in range(21) if img[y, x].any()] == list(ys)
    # a limb of length 0 is its end test: 4 |p - a|^2 <= 16
    z = np.zeros((21, 31, 3), np.uint8)
    fr.paint_limb(z, (10, 10), (10, 10), 4, (9, 9, 9))
    want = np.array([[4 * ((x - 10) ** 2 + (y - 10) ** 2) <= 16 for x in range(31)] for y in range(21)])
    assert np.array_equal(z.any(-1), want) and count(z) == 13


def test_centres_at_the_border():
    ones = np.ones(1)
    off = px((-9, -9))
    assert count(fr.keypoint_panel(12, 12, px((0, 5)), off, ones)) == 0     # x = 0: the reference's "> EPS" on integers
    assert count(fr.keypoint_panel(12, 12, px((0.99, 5)), off, ones)) == 0
    assert count(fr.keypoint_panel(12, 12, px((5, 0)), off, ones)) == 0
    img = fr.keypoint_panel(12, 12, px((1, 1)), off, ones)                  # drawn, clipped: rows 0 .. 4 of the disc's 7
    assert [int(img[y].any(-1).sum()) for y in range(6)] == [5, 5, 5, 4, 3, 0]
    assert count(fr.keypoint_panel(12, 12, px((5, 5)), off, np.zeros(1))) == 0
    for bad in ((np.nan, 5), (5, np.inf), (1e9, 5), (-4, 5), (float(1 << 20), 5)):
        assert count(fr.keypoint_panel(12, 12, px(bad), off, ones)) == 0, bad
    W = 12
    assert count(fr.keypoint_panel(12, W, px((W + 2, 5)), off, ones)) == 3  # only column W - 1, rows 4 .. 6
    assert count(fr.keypoint_panel(12, W, px((W + 3, 5)), off, ones)) == 0


def test_red_over_green():
    same = fr.keypoint_panel(21, 21, px((10, 10)), px((10, 10)), np.ones(1))
    assert count(same) == 37 and (same[same.any(-1)] == RED).all()
    shifted = fr.keypoint_panel(21, 21, px((10, 10)), px((13, 10)), np.ones(1))
    assert (shifted[10, 10:17] == RED).all() and (shifted[10, 7:10] == GREEN).all()
    # order with limbs: the fit's limb lies over the target's disc, the fit's disc over its own limb
    two = fr.keypoint_panel(21, 31, px((5, 10), (15, 10)), px((5, 10), (15, 10)), np.ones(2), limbs=[[0, 1]], limb_rgb=[[1, 2, 3]])
    assert tuple(two[10, 10]) == (1, 2, 3) and tuple(two[10, 5]) == RED and not (two == GREEN).all(-1).any()


def test_blend_rounds_half_to_even():
    c, img = np.array([255, 0, 5, 5, 255], np.uint8), np.array([0, 255, 0, 5, 255], np.uint8)
    assert fr.blend(c, img).tolist() == [153, 102, 3, 5, 255]
    # half-way cases: the rounding itself, and every pair of bytes whose float32 sum is a tie
    assert np.rint(np.float32(2.5)) == 2 and np.rint(np.float32(3.5)) == 4
    ties = [(a, b) for a in range(256) for b in range(256)
            if float(np.float32(0.6) * np.float32(a) + np.float32(0.4) * np.float32(b)) % 1.0 == 0.5]
    for a, b in ties[:8]:
        s = float(np.float32(0.6) * np.float32(a) + np.float32(0.4) * np.float32(b))
        assert int(fr.blend(np.array([a], np.uint8), np.array([b], np.uint8))[0]) == 2 * round(s / 2)


def test_normal_bytes_and_halving():
    prior = np.array([1.0, -1.0, 0.0, 0.5], np.float32).reshape(1, 1, 4).repeat(3, 0)
    b = fr.normal_bytes(prior, np.array([[1, 1, 1, 0]], np.uint8))
    assert b[0, :, 0].tolist() == [255, 0, 127, 0]                          # 127.5 is truncated; off the body 0
    blk = np.array([[1, 2], [2, 2]], np.uint8)[..., None].repeat(3, -1)
    assert fr.halve(blk).tolist() == [[[2, 2, 2]]]
    odd = np.arange(3 * 5 * 3, dtype=np.uint8).reshape(3, 5, 3)
    assert fr.halve(odd).shape == (1, 2, 3)


def test_yaw_matrices():
    from soar_amd import fitviz
    w2c = np.eye(4)
    R = fitviz.yaw_matrices(w2c, 3)
    assert R.shape == (3, 3, 3) and R.dtype == np.float32 and np.array_equal(R[0], np.eye(3, dtype=np.float32))
    gen = np.random.default_rng(5)
    q, _ = np.linalg.qr(gen.normal(size=(3, 3)))
    tilted = np.eye(4)
    tilted[:3, :3] = q
    for w in (w2c, tilted):
        R = fitviz.yaw_matrices(w, 3).astype(np.float64)
        for k in range(3):
            assert np.abs(R[k] @ R[k].T - np.eye(3)).max() <= 1e-6 and abs(np.linalg.det(R[k]) - 1) <= 1e-6
        assert np.abs(R[1] @ R[1] @ R[1] - np.eye(3)).max() <= 1e-5
        assert np.abs(R[1] @ R[1] - R[2]).max() <= 1e-6
        axis = -w[:3, 1] / np.linalg.norm(w[:3, 1])
        assert np.abs(R[1] @ axis - axis).max() <= 1e-6
    # the identity camera: a rotation by 120 degrees about (0, -1, 0)
    c, s = np.cos(2 * np.pi / 3), np.sin(2 * np.pi / 3)
    assert np.abs(fitviz.yaw_matrices(np.eye(4), 3)[1] - np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])).max() <= 1e-6
    assert fitviz.yaw_matrices(np.eye(4), 4).shape == (4, 3, 3)
    with pytest.raises(ValueError):
        fitviz.yaw_matrices(np.zeros((4, 4)))


def test_yaw_restatement_keeps_view_zero_and_follows_float64():
    from soar_amd import fitviz
    gen = np.random.default_rng(1)
    v, p = gen.normal(size=(2, 7, 3)).astype(np.float32), gen.normal(size=(2, 3)).astype(np.float32)
    R = fitviz.yaw_matrices(np.eye(4), 3)
    out = fr.yaw_views(v, p, R)
    assert np.array_equal(out[:, 0], v)
    bound = 8 * 2.0 ** -23 * max(1.0, np.abs(v).max(), np.abs(p).max())
    assert np.abs(out - fr.yaw_views64(v, p, R)).max() <= bound


def test_residuals_restatement():
    gen = np.random.default_rng(2)
    f, t = gen.uniform(0, 500, (3, 137, 2)).astype(np.float32), gen.uniform(0, 500, (3, 137, 2)).astype(np.float32)
    conf = gen.uniform(0, 1, (3, 137)).astype(np.float32)
    conf[1] = 0.1
    f[0, 3] = np.nan
    mask = np.ones(137)
    mask[5] = 0
    r32, r64 = fr.residuals(f, t, conf, mask), fr.residuals64(f, t, conf, mask)
    assert np.array_equal(r32[:, 0], r64[:, 0]) and r32[1].tolist() == [0, 0, 0] and r32[0, 0] == ((conf[0] > 0.3).sum() - (conf[0, 3] > 0.3) - (conf[0, 5] > 0.3))
    assert np.abs(r32[:, 1] - r64[:, 1]).max() <= 16 * 2.0 ** -24 * r64[:, 1].max()


def test_symbols_are_exported_and_refuse_bad_arguments():
    from soar_amd import build, fitviz, hip_lib
    build.build()
    L = hip_lib.lib()
    header = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    for name in ("soar_fitviz_yaw_views", "soar_fitviz_strip", "soar_fitviz_residuals"):
        assert name in hip_lib.SIGNATURES and name in header and hasattr(L, name)
    assert "fitviz.hip" in build.SOURCES and build.EXTRA_FLAGS["fitviz.hip"] == ["-ffp-contract=off"]
    assert hip_lib.ABI_VERSION == 8 == L.soar_abi_version()
    for name in ("yaw_matrices", "yaw_views", "draw_strips", "fit_residuals", "fit_strips", "save_strips", "FitVisualizer",
                 "OPENPOSE_BODY25_LIMBS"):
        assert hasattr(fitviz, name)
    limbs, rgb = fitviz.OPENPOSE_BODY25_LIMBS
    assert limbs.shape == (24, 2) and rgb.shape == (24, 3) and limbs.min() == 0 and limbs.max() == 24 and rgb.dtype == np.uint8
    assert C.sizeof(hip_lib.SoarFitvizStripArgs) == 8 * 4 + 6 * 8 + 4 * 8 + 2 * 8 + 8 + 8

    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)            # any non-NULL address: nothing reads it before the checks fail
    stride = (C.c_int64 * 3)(3, 3, 1)
    assert L.soar_fitviz_yaw_views(2, 5, 3, None, stride, p, p, p, None) == 1 and "NULL" in hip_lib.last_error()
    assert L.soar_fitviz_yaw_views(2, 5, 3, p, stride, p, p, None, None) == 1 and "NULL" in hip_lib.last_error()
    assert L.soar_fitviz_yaw_views(2, 5, 0, p, stride, p, p, p, None) == 1 and "n_views" in hip_lib.last_error()
    assert L.soar_fitviz_yaw_views(0, 5, 3, None, None, None, None, None, None) == 0

    def strip_args(**kw):
        a = hip_lib.SoarFitvizStripArgs()
        a.N, a.H, a.W, a.K, a.L, a.radius, a.thickness = 1, 8, 8, 4, 0, 3, 4
        for k in ("target_px", "fit_px", "kp_mask", "prior", "mask", "out"):
            setattr(a, k, p)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.soar_fitviz_strip(None, None) == 1 and "NULL" in hip_lib.last_error()
    assert L.soar_fitviz_strip(C.byref(strip_args(K=513)), None) == 1 and "513" in hip_lib.last_error()
    assert L.soar_fitviz_strip(C.byref(strip_args(L=513)), None) == 1 and "513" in hip_lib.last_error()
    assert L.soar_fitviz_strip(C.byref(strip_args(radius=0)), None) == 1 and "radius" in hip_lib.last_error()
    assert L.soar_fitviz_strip(C.byref(strip_args(radius=9)), None) == 1
    assert L.soar_fitviz_strip(C.byref(strip_args(thickness=0)), None) == 1
    assert L.soar_fitviz_strip(C.byref(strip_args(W=5000)), None) == 1
    for k in ("target_px", "fit_px", "kp_mask", "prior", "mask", "out"):
        assert L.soar_fitviz_strip(C.byref(strip_args(**{k: None})), None) == 1 and "NULL" in hip_lib.last_error(), k
    assert L.soar_fitviz_strip(C.byref(strip_args(L=2)), None) == 1 and "NULL" in hip_lib.last_error()       # limbs without a table
    empty = hip_lib.SoarFitvizStripArgs()
    empty.H, empty.W, empty.radius, empty.thickness = 8, 8, 3, 4
    assert L.soar_fitviz_strip(C.byref(empty), None) == 0                                                      # N == 0

    assert L.soar_fitviz_residuals(2, 4, None, p, p, p, 0.3, p, None) == 1 and "NULL" in hip_lib.last_error()
    assert L.soar_fitviz_residuals(2, 4, p, p, p, p, 0.3, None, None) == 1
    assert L.soar_fitviz_residuals(2, 513, p, p, p, p, 0.3, p, None) == 1 and "K=513" in hip_lib.last_error()
    assert L.soar_fitviz_residuals(0, 4, None, None, None, None, 0.3, None, None) == 0


def test_cpu_tensors_are_refused():
    from soar_amd import fitviz
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fitviz.yaw_views(torch.zeros(1, 4, 3), torch.zeros(1, 3), torch.eye(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fitviz.draw_strips(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), torch.ones(4), torch.zeros(3, 2, 3, 8, 8), torch.zeros(3, 2, 8, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fitviz.fit_residuals(torch.zeros(1, 4, 2), torch.zeros(1, 4, 2), torch.zeros(1, 4), torch.ones(4))


# ---- the hook of SMPLify.fit ------------------------------------------------------------------------------------------------------

def quadratic_objective(rig, params, init, Ks, w2c, img_wh, target, scales, weights, sigma, ignore_hands):
    """A convex stand-in for the objective, on the CPU: the distance to the start plus a pull of every parameter toward 0.1."""
    from soar_amd import smplify
    loss, grads = torch.zeros(()), {}
    for k in smplify.GRAD_KEYS:
        d = params[k].detach() - 0.1
        hands = ignore_hands and k in ("left_hand_pose", "right_hand_pose")
        grads[k] = torch.zeros_like(d) if hands else 2.0 * d
        loss = loss + (0.0 if hands else (d * d).sum())
    return types.SimpleNamespace(losses=torch.stack([loss, torch.zeros(()), torch.zeros(())]), grads=grads)


def start_params(N=3):
    gen = torch.Generator().manual_seed(3)
    rn = lambda *s: 0.2 * torch.randn(*s, generator=gen)
    return {"global_orient": rn(N, 3), "body_pose": rn(N, 63), "left_hand_pose": rn(N, 45), "right_hand_pose": rn(N, 45), "jaw_pose": rn(N, 3),
            "leye_pose": rn(N, 3), "reye_pose": rn(N, 3), "betas": rn(N, 10), "expression": rn(N, 10), "transl": rn(N, 3)}


def cpu_fit(**kw):
    from soar_amd import smplify
    return smplify.SMPLify(types.SimpleNamespace(device=torch.device("cpu")), objective=quadratic_objective,
                           scales=lambda t, img_wh: torch.ones(t.shape[0]), **kw)


class Stub:
    def __init__(self, debug=False):
        self.debug, self.names, self.seen = debug, [], []

    def __call__(self, name, params, Ks, w2c, img_wh, target_kps):
        self.names.append(name)
        self.seen.append({k: v.clone() for k, v in params.items()})
        assert not torch.is_grad_enabled() or all(not v.requires_grad for v in params.values())
        for v in params.values():
            v.fill_(7.0)                                  # copies: scribbling on them must not reach the fit


def test_fit_without_a_visualizer_is_bit_for_bit_the_fit_of_before():
    """``visual=None`` against a call without the argument, and against a fit that is watched: the same parameters, bit for bit (the
    visualizer is handed copies and touches neither ``.grad`` nor the optimizer)."""
    start, args = start_params(), (torch.eye(3).expand(3, 3, 3), torch.eye(4), (64, 48), torch.rand(3, 137, 3))
    steps = dict(body_steps=3, hand_steps=4, max_iters=4)
    plain, none, stub = cpu_fit(**steps), cpu_fit(**steps), cpu_fit(**steps)
    a = plain.fit(start, *args)
    b = none.fit(start, *args, visual=None)
    watcher = Stub(debug=False)
    c = stub.fit(start, *args, visual=watcher)
    assert plain.evaluations == none.evaluations == stub.evaluations > 0
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), k
    assert watcher.names == ["1_000", "1_002", "2_003"]
    first = watcher.seen[0]
    assert first["global_orient"].shape == (3, 3) and first["body_pose"].shape == (3, 63) and first["betas"].shape == (1, 10)
    assert float((first["body_pose"] - start["body_pose"]).abs().max()) < 1e-4          # "1_000" shows the start
    assert float((watcher.seen[-1]["left_hand_pose"] - a["left_hand_pose"]).abs().max()) == 0.0


@pytest.mark.parametrize("debug", [False, True])
def test_the_names_of_the_reference(debug):
    watcher = Stub(debug=debug)
    fit = cpu_fit(max_iters=2)
    assert (fit.body_steps, fit.hand_steps) == (20, 40)
    fit.fit(start_params(2), torch.eye(3).expand(2, 3, 3), torch.eye(4), (64, 48), torch.rand(2, 137, 3), visual=watcher)
    if debug:
        assert watcher.names == ["1_000"] + [f"1_{i:03d}" for i in (4, 9, 14, 19)] + [f"2_{i:03d}" for i in range(4, 40, 5)]
    else:
        assert watcher.names == ["1_000", "1_019", "2_039"]
