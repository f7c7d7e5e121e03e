"""CPU tests of the initialisation from keypoints (soar_amd/pose_init.py, csrc/pose_init.hip): the float64 restatement of
tests/pose_init_ref.py recovers a planted state, its path equals brute force, and the entry points refuse bad arguments through the
C ABI before any launch.  Nothing is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pose_init_ref as pr
from test_smplify_cpu import golden, golden_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z_MIN = 0.1


def test_the_restatement_recovers_a_planted_state():
    g, m, p, i, tables = golden()
    c = golden_call(g)
    sc = pr.planted_scene(m, tables, c)
    out = pr.search(sc["points0"], sc["points0"][:, 0], sc["R"], tables, sc["targets"], c["Ks"].double(), c["w2c"].double(), c["img_wh"],
                    sc["scales"], z_min=Z_MIN)
    assert out["valid"].all() and np.isfinite(out["cost"]).all()
    for n in range(5):
        order = np.argsort(out["cost"][n])
        print(f"frame {n}: best {order[0]} cost {out['cost'][n, order[0]]:.3e} runner-up {order[1]} cost {out['cost'][n, order[1]]:.3e} "
              f"cond {out['cond'][n]:.1f} smallest depth {out['zmin'][n].min():.3f}")
        assert order[0] == sc["s_true"][n]
        assert out["cost"][n, order[0]] < 1e-20 and out["cost"][n, order[1]] > 7e3
        assert np.abs(out["transl"][n, order[0]] - sc["transl_true"][n]).max() <= 1e-13
        assert out["cond"][n] < 1e3
    assert np.abs(out["zmin"] - Z_MIN).min() > 0.1                        # no state sits near the depth limit
    # the float32 composition finds the same states
    o32 = pr.search(sc["points0"], sc["points0"][:, 0], sc["R"], tables, sc["targets"].float(), c["Ks"], c["w2c"], c["img_wh"],
                    sc["scales"].float(), z_min=Z_MIN, dtype=torch.float32)
    assert (o32["cost"].argmin(1) == sc["s_true"]).all()


@pytest.mark.parametrize("yaws", [12, 24])
@pytest.mark.parametrize("b", [0, 1])
def test_an_off_bank_yaw_goes_to_a_bracketing_bank_entry(yaws, b):
    g, m, p, i, tables = golden()
    c = golden_call(g)
    sc = pr.offbank_scene(m, tables, c, yaws, b)
    pts = pr.points_of(m, pr.base_params(pr.golden_base_poses(), 10, 10), torch.float64)
    import smplify_ref as sr
    out = pr.search(pts, pts[:, 0], pr.yaw_bank(yaws), tables, sc["targets"], sc["Ks"].double(), c["w2c"].double(), c["img_wh"],
                    sr.target_scales(sc["targets"], c["img_wh"]))
    best = out["cost"].argmin(1)
    from soar_amd import pose_init
    path, _, _ = pr.viterbi(out["cost"].astype(np.float32), pr.transition_cost(pr.yaw_bank(yaws), 2, pose_init.ROT_WEIGHT, pose_init.SWITCH_COST))
    for n in range(6):
        assert best[n] // yaws == b and best[n] % yaws in sc["brackets"][n], (n, best[n], sc["brackets"][n])
        assert path[n] // yaws == b and path[n] % yaws in sc["brackets"][n], (n, path[n], sc["brackets"][n])      # the default path too
        second = np.sort(out["cost"][n])[1]
        print(f"yaws {yaws} base {b} frame {n}: best {best[n]} {out['cost'][n, best[n]]:.1f}, runner-up {np.argsort(out['cost'][n])[1]} {second:.1f}")


def test_the_restated_path_equals_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(20):
        U = rng.integers(0, 9, (4, 3)).astype(np.float32)
        T = rng.integers(0, 5, (3, 3)).astype(np.float32)
        path, total, _ = pr.viterbi(U, T)
        bpath, btotal = pr.brute_force(U, T)
        assert float(total) == btotal
        assert float(sum(U[n, path[n]] for n in range(4)) + sum(T[path[n - 1], path[n]] for n in range(1, 4))) == btotal
    # a frame without evidence is a row of zeros, and the lowest index wins ties
    U = np.array([[1, 0, 2], [np.inf] * 3, [5, 5, 0]], np.float32)
    T = (4.0 * (1 - np.eye(3))).astype(np.float32)
    path, total, _ = pr.viterbi(U, T)
    zeroed = np.where(np.isinf(U), np.float32(0), U)
    bpath, btotal = pr.brute_force(zeroed, T)
    assert path.tolist() == bpath.tolist() == pr.viterbi(zeroed, T)[0].tolist() == [2, 2, 2] and float(total) == btotal == 2.0
    path, total, _ = pr.viterbi(np.zeros((3, 4), np.float32), np.zeros((4, 4), np.float32))
    assert path.tolist() == [0, 0, 0] and float(total) == 0.0
    tr = np.arange(5 * 2 * 3, dtype=np.float32).reshape(5, 2, 3)
    got = pr.fill(tr, np.array([0, 1, 1, 0, 1]), np.array([0, 1, 0, 0, 1], bool))
    assert np.array_equal(got[0], tr[1, 1]) and np.array_equal(got[4], tr[4, 1])
    assert np.allclose(got[2], tr[1, 1] + (tr[4, 1] - tr[1, 1]) / 3.0) and np.allclose(got[3], tr[1, 1] + (tr[4, 1] - tr[1, 1]) * (2.0 / 3.0))


def test_symbols_are_exported_and_refuse_bad_arguments():
    from soar_amd import build, hip_lib
    build.build()
    L = hip_lib.lib()
    header = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    for name in ("soar_smplify_model_points", "soar_pose_init_search", "soar_pose_init_viterbi"):
        assert name in hip_lib.SIGNATURES and name in header and hasattr(L, name)
    assert "pose_init.hip" in build.SOURCES and hip_lib.ABI_VERSION == 8 == L.soar_abi_version()
    assert not [n for n in hip_lib.SIGNATURES if "pose_init" in n and (n.endswith("_bytes") or n.endswith("_floats"))]
    assert C.sizeof(hip_lib.SoarPoseSearch) == 6 * 4 + 10 * 8 + 6 * 4 + 3 * 8
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)                               # any non-NULL address: nothing reads it before the checks fail

    def search_args(**kw):
        a = hip_lib.SoarPoseSearch()
        a.N, a.B, a.H, a.PA, a.P, a.min_points = 4, 2, 12, 144, 123, 6
        for k in ("points0", "pivot", "rotations", "src_inds", "dst_inds", "kp_mask", "target_kps", "Ks", "w2c", "scales", "cost", "transl", "valid"):
            setattr(a, k, p)
        a.img_w, a.img_h, a.sigma, a.conf_min, a.z_min = 640.0, 480.0, 100.0, 0.1, 0.1
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, word):
        assert L.soar_pose_init_search(C.byref(a), None) == 1 and word in hip_lib.last_error(), hip_lib.last_error()
    assert L.soar_pose_init_search(None, None) == 1 and "NULL" in hip_lib.last_error()
    refused(search_args(N=0), "N >= 1")
    refused(search_args(N=-3), "N >= 1")
    refused(search_args(B=5, H=205), "1024")
    refused(search_args(H=0), "H >= 1")
    refused(search_args(P=138), "P <= 137")
    refused(search_args(min_points=0), "min_points")
    refused(search_args(sigma=0.0), "sigma")
    for k in ("points0", "pivot", "rotations", "src_inds", "kp_mask", "target_kps", "Ks", "w2c", "scales", "cost", "transl", "valid"):
        refused(search_args(**{k: None}), "NULL pointer")
    V = L.soar_pose_init_viterbi
    assert V(0, 3, p, p, p, p, p, None, None, None, None) == 1 and "N >= 1" in hip_lib.last_error()
    assert V(3, 1025, p, p, p, p, p, None, None, None, None) == 1 and "1024" in hip_lib.last_error()
    assert V(3, 0, p, p, p, p, p, None, None, None, None) == 1
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert V(3, 4, *args, None, None, None, None) == 1 and "NULL pointer" in hip_lib.last_error()
    assert V(3, 4, p, p, p, p, p, p, None, None, None) == 1 and "come together" in hip_lib.last_error()
    assert V(3, 4, p, p, p, p, p, p, p, None, None) == 1 and "come together" in hip_lib.last_error()
    # model_points: the rig's limits, N <= 0, NULL tables
    M = L.soar_smplify_model_points
    assert M(None, None, None, 144, None, None, None, None) == 1 and "NULL" in hip_lib.last_error()
    rig, args = hip_lib.SoarSmplifyRig(), hip_lib.SoarSmplifyArgs()
    rig.J, rig.NBS, rig.NE, rig.VS = 55, 10, 10, 300
    assert M(C.byref(rig), None, C.byref(args), 144, p, p, p, None) == 1 and "VS" in hip_lib.last_error()
    rig.VS = 77
    assert M(C.byref(rig), None, C.byref(args), 144, p, p, p, None) == 1 and "N >= 1" in hip_lib.last_error()
    args.N = 3
    assert M(C.byref(rig), None, C.byref(args), 54, p, p, p, None) == 1 and "PA >= 55" in hip_lib.last_error()
    assert M(C.byref(rig), None, C.byref(args), 144, p, p, p, None) == 1 and "NULL rig table" in hip_lib.last_error()


def test_the_python_api_refuses_cpu_tensors_and_builds_the_bank():
    import types
    from soar_amd import pose_init, smplify
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose_init.viterbi(torch.zeros(2, 3), torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose_init.viterbi_path(torch.zeros(2, 3), torch.zeros(3, 3), torch.zeros(2, 3, 3), torch.ones(2, dtype=torch.bool))
    rig = types.SimpleNamespace(device=torch.device("cpu"), PA=144)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose_init.search(torch.zeros(2, 144, 3), torch.zeros(2, 3), torch.eye(3)[None], rig, torch.zeros(1, 137, 3), torch.eye(3)[None],
                         torch.eye(4), (640, 480), torch.ones(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pose_init.init_from_keypoints(rig, torch.zeros(1, 137, 3), (640, 480))
    # the bank and the rules are plain torch
    K = pose_init.default_intrinsics(3, (640, 480))
    assert K.shape == (3, 3, 3) and float(K[0, 0, 0]) == 800.0 == float(K[2, 1, 1]) and K[1, :2, 2].tolist() == [320.0, 240.0]
    assert float(pose_init.default_intrinsics(1, (640, 480), focal=500.0)[0, 0, 0]) == 500.0
    R = pose_init.rotation_bank(12, (0.0, 0.3))
    assert R.shape == (24, 3, 3) and torch.allclose(R @ R.transpose(1, 2), torch.eye(3).expand(24, 3, 3), atol=1e-6)
    assert torch.allclose(R[:12].double(), pr.yaw_bank(12), atol=1e-7)
    assert torch.allclose(pose_init.base_poses().double(), pr.golden_base_poses(), atol=1e-7) and pose_init.base_poses().shape == (2, 63)
    T = pose_init.transition_cost(R[:12], 2, 100.0, 7.0)
    assert T.shape == (24, 24) and np.allclose(T.numpy(), pr.transition_cost(R[:12], 2, 100.0, 7.0), rtol=1e-4, atol=1e-3)
    assert float(T[0, 0]) < 1e-3 and abs(float(T[0, 12]) - 7.0) < 1e-3 and abs(float(T[0, 1]) - 100.0 * (np.pi / 6) ** 2) < 1e-2
    assert abs(float(T[0, 6]) - 100.0 * np.pi ** 2) < 0.5
    for name in pose_init.__all__:
        assert hasattr(pose_init, name)
    assert hasattr(smplify, "model_points")
