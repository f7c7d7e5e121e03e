"""CPU tests of soar_amd/pose.py: the configuration read back from a state dict, the refusals, the ABI's new symbols, the
JSON round trip, and the restatement of tests/pose_ref.py itself on constructed scenes.

On the scenes' bound: the position of a peak is a centroid over a 7 x 7 window round the largest pixel, so for a blob wider than
the window it tends to that pixel's centre and its error to the place's offset from the centre: up to 0.5 per axis, 0.71 in distance,
whatever computes it.  The scenes therefore put their parts at sub-pixel places within 0.2 of a pixel centre per axis (0.28 in
distance); the restatement then has to find every part within 0.5 net pixels, the bound the definition can meet."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch

import pose_ref as R
from soar_amd import hip_lib, masks, pose, smplify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("cfg", [R.TINY, R.TINY_1, R.SHIPPED], ids=["tiny", "tiny_1_1", "shipped"])
def test_configuration_is_read_from_shapes_and_keys(cfg):
    if cfg is R.SHIPPED:
        sd = {}
        for conv, prelu, shape in pose.layer_keys(cfg):                     # shapes only: the shipped weights are 200 MB
            sd[f"{conv}.weight"] = torch.empty(shape, device="meta")
            sd[f"{conv}.bias"] = torch.empty(shape[:1], device="meta")
            if prelu:
                sd[f"{prelu}.weight"] = torch.empty(shape[:1], device="meta")
        got = pose.read_config(sd)
    else:
        sd = R.make_state_dict(cfg, seed=1)
        net = pose.PoseNet(sd)
        got = net.cfg
        assert net.tensor_keys == [k for conv, prelu, _ in pose.layer_keys(cfg) for k in
                                   [f"{conv}.weight", f"{conv}.bias"] + ([f"{prelu}.weight"] if prelu else [])]
        assert set(net.tensor_keys) == set(sd)
    want = dict(cfg)
    if cfg["n_paf"] == 1 and cfg["n_heat"] == 1:
        want["w1"], want["m1"] = want["w0"], want["m0"]                      # no later stage to read them from
    assert got == want
    keys = pose.layer_keys(cfg)
    assert len(keys) == 12 + 17 * (cfg["n_paf"] + cfg["n_heat"])
    first = {k: s for k, _, s in keys}
    F = cfg["feat"]
    assert first["Mconv1_stage0_L2_0"][1] == F and first["Mconv1_stage0_L1_0"][1] == F + 52
    if cfg["n_paf"] > 1:
        assert first["Mconv1_stage1_L2_0"][1] == F + 52 and first["Mconv1_stage1_L1_0"][1] == F + 26 + 52


def test_the_tables():
    assert len(pose.PARTS) == 25 and len(pose.PAIRS) == 26 and len(pose.PAF_CHANNELS) == 26
    assert sorted(c for xy in pose.PAF_CHANNELS for c in xy) == list(range(52)) and all(y == x + 1 and x % 2 == 0 for x, y in pose.PAF_CHANNELS)
    assert all(0 <= a < 25 and 0 <= b < 25 and a != b for a, b in pose.PAIRS) and len(set(pose.PAIRS)) == 26
    # every part hangs on the neck through the limbs
    reach = {1}
    for _ in range(26):
        reach |= {b for a, b in pose.PAIRS if a in reach} | {a for a, b in pose.PAIRS if b in reach}
    assert reach == set(range(25))


def test_refusals():
    sd = R.make_state_dict(R.TINY, seed=2)
    with pytest.raises(KeyError, match="Mprelu3_stage1_L1_2.weight"):
        pose.PoseNet({k: v for k, v in sd.items() if k != "Mprelu3_stage1_L1_2.weight"})
    with pytest.raises(KeyError, match="conv4_3_CPM.weight"):
        pose.PoseNet({k: v for k, v in sd.items() if k != "conv4_3_CPM.weight"})
    with pytest.raises(KeyError, match="stages 0 .. n - 1 of branch L2"):
        pose.PoseNet({k: v for k, v in sd.items() if not k.startswith("Mconv7_stage0_L2")})
    for key, rows in (("Mconv7_stage1_L2", 50), ("Mconv7_stage0_L1", 25)):
        bad = dict(sd)
        bad[f"{key}.weight"], bad[f"{key}.bias"] = sd[f"{key}.weight"][:rows], sd[f"{key}.bias"][:rows]
        with pytest.raises(ValueError, match=rf"{key}.weight' has shape \[{rows}, "):
            pose.PoseNet(bad)
    bad = dict(sd)
    bad["conv1_1.weight"] = torch.zeros(12, 3, 3, 3)
    with pytest.raises(ValueError, match="multiple of 8"):
        pose.PoseNet(bad)
    for nh in (0, 8, 40, 369, 368.0):
        with pytest.raises(ValueError, match="net_height must be a multiple of 16"):
            pose.net_size(1080, 1920, nh)
    assert pose.net_size(1080, 1920) == (368, 656) and pose.net_size(1080, 1920, 32) == (32, 64) and pose.net_size(100, 100, 48) == (48, 48)
    net = pose.PoseNet(sd)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        net(torch.zeros(1, 3, 32, 48))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        pose.pose_peaks(torch.zeros(1, 4, 6, 26))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        pose.PoseNet.preprocess(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 32)


def test_symbols_sources_and_header():
    from soar_amd import build
    new = {"soar_pose_weights_size", "soar_pose_workspace_size", "soar_pose_pack_weights", "soar_pose_preprocess", "soar_pose_forward",
           "soar_pose_peaks", "soar_pose_assemble", "soar_pose_scale", "soar_selftest_conv_gemm_slope"}
    assert new <= set(hip_lib.SIGNATURES)
    assert "pose.hip" in build.SOURCES and build.EXTRA_FLAGS["pose.hip"] == ["-ffp-contract=off"]
    header = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    assert all(f"int {name}(" in header for name in new) and "#define SOAR_HIP_ABI_VERSION 8" in header
    assert "typedef struct SoarPoseConfig {" in header and "typedef struct SoarPoseAssembleArgs {" in header
    L = hip_lib.lib()                                                       # binds every declared symbol
    assert all(hasattr(L, name) for name in new)
    # the sizing calls answer without a device, and refuse what the kernels cannot run
    cfg = pose._c_config(R.TINY)
    nb, count = C.c_size_t(0), C.c_int32(0)
    assert L.soar_pose_weights_size(C.byref(cfg), C.byref(nb), C.byref(count)) == 0
    n_prelu = sum(1 for _, p, _ in pose.layer_keys(R.TINY) if p)
    assert count.value == 2 * len(pose.layer_keys(R.TINY)) + n_prelu and nb.value % 256 == 0 and nb.value > 0
    assert L.soar_pose_workspace_size(C.byref(cfg), 2, 32, 48, C.byref(nb)) == 0 and nb.value % 256 == 0
    assert L.soar_pose_workspace_size(C.byref(cfg), 2, 32, 40, C.byref(nb)) != 0 and "multiples of 16" in hip_lib.last_error()
    cfg.w1 = 12
    assert L.soar_pose_weights_size(C.byref(cfg), C.byref(nb), None) != 0 and "multiple of 8" in hip_lib.last_error()
    assert "soar_amd.pose" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import workspace_guard
    assert "soar_amd.pose" in {m.__name__ for m in workspace_guard.modules_with_workspace()}
    # the post-processing's refusals
    assert L.soar_pose_peaks(1, 4, 6, None, 0.05, 33, None, None, None) != 0 and "max_peaks" in hip_lib.last_error()
    assert L.soar_pose_peaks(1, 4, 300, None, 0.05, 4, None, None, None) != 0
    assert L.soar_pose_peaks(1, 4, 6, None, 0.05, 4, None, None, None) != 0 and "NULL" in hip_lib.last_error()
    assert L.soar_pose_peaks(0, 4, 6, None, 0.05, 4, None, None, None) == 0
    a = hip_lib.SoarPoseAssembleArgs()
    a.B, a.h, a.w, a.max_peaks, a.max_people = 1, 4, 6, 4, 2
    assert L.soar_pose_assemble(C.byref(a), None) != 0 and "pair 0" in hip_lib.last_error()


def test_the_shared_gemm_refuses_a_slope_with_an_activation():
    L = hip_lib.lib()
    a = hip_lib.SoarConvGemmArgs()
    tile = C.c_int32(0)
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16
    a.x = a.y = p
    a.ldx = a.ldy = 8
    a.alpha = 1.0
    a.N, a.Hg, a.Wg, a.Hin, a.Win, a.Cin, a.Cout, a.stride, a.dil, a.Wout, a.os, a.nph = 1, 1, 1, 1, 1, 8, 1, 1, 1, 1, 1, 1
    a.ph[0].w, a.ph[0].ldw, a.ph[0].ntaps = p, 8, 1
    for wtype in (0, 1, 2):
        for act in (1, 2):
            assert L.soar_selftest_conv_gemm_slope(C.byref(a), wtype, act, p, C.byref(tile), None) != 0
            assert "slope (PReLU) goes with act == 0 only" in hip_lib.last_error()
    assert L.soar_selftest_conv_gemm_slope(C.byref(a), 0, 3, None, C.byref(tile), None) != 0 and "act must be" in hip_lib.last_error()
    assert L.soar_selftest_conv_gemm_slope(None, 0, 0, p, C.byref(tile), None) != 0 and "NULL" in hip_lib.last_error()


def test_json_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    people = (rng.random((3, 2, 25, 3)) * 700).astype(np.float32)
    people[0, 0, 7] = 0                                                      # a missing part
    n_people = np.array([2, 0, 1], np.int32)
    stems = ["00002", "00000", "00001"]                                      # load_keypoints sorts by name
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pose.save_keypoints(str(tmp_path), torch.from_numpy(people), torch.from_numpy(n_people), stems)
    assert len(w) == 1 and "'00000'" in str(w[0].message)
    doc = json.load(open(tmp_path / "00002_keypoints.json"))
    assert set(doc) == {"version", "people"} and len(doc["people"]) == 2
    assert [len(doc["people"][1][k]) for k in ("pose_keypoints_2d", "face_keypoints_2d", "hand_left_keypoints_2d", "hand_right_keypoints_2d")] == [75, 210, 63, 63]
    assert len(json.load(open(tmp_path / "00000_keypoints.json"))["people"]) == 1   # nobody: one all-zero person, still readable
    kp = smplify.load_keypoints(str(tmp_path))
    assert kp.shape == (3, 137, 3) and kp.dtype == np.float32
    assert np.array_equal(kp[2, :25], people[0, 0]) and np.array_equal(kp[1, :25], people[2, 0]) and not kp[0].any()
    assert not kp[:, 25:].any()
    prompts = masks.keypoint_prompts(kp)
    assert len(prompts) == 3 and prompts[0][0].shape == (0, 2)
    assert np.array_equal(prompts[2][0], people[0, 0][people[0, 0, :, 2] > 0.5, :2])


SCENES = {"close": (R.person(70.4, 100.6), R.person(92.7, 118.3)), "outside": (R.person(70.4, 100.6), R.person(222.4, 104.7))}


@pytest.mark.parametrize("name", list(SCENES))
def test_the_restatement_finds_two_constructed_people(name):
    """close: the necks are 28.5 pixels apart, nearer than either neck is to its own hip (50), knee or ankle; outside: the second person's
    left side lies behind the right edge"""
    h, w = 28, 30
    heat, paf, seen = R.scene(h, w, SCENES[name])
    assert len(seen[0]) == 25 and len(seen[1]) == (25 if name == "close" else 15)
    if name == "close":
        a, b = SCENES[name]
        assert np.hypot(a[1][0] - b[1][0], a[1][1] - b[1][1]) < np.hypot(a[1][0] - a[8][0], a[1][1] - a[8][1])
    assert all(max(abs(x % 1 - 0.5), abs(y % 1 - 0.5)) <= 0.2 + 1e-9 for who in seen for x, y in who.values())
    peaks, counts = R.peaks_ref(heat)
    assert counts[25] == 0 and all(counts[p] == sum(p in who for who in seen) for p in range(25))
    people, n = R.assemble_ref(peaks, counts, paf)
    assert n == 2 and not people[2:].any()
    for who in seen:
        k = int(np.argmin([np.hypot(*(people[q, 1, :2] - np.array(who[1]))) for q in range(2)]))
        for p in range(25):
            if p in who:
                d = float(np.hypot(*(people[k, p, :2] - np.array(who[p]))))
                assert d <= 0.5 and people[k, p, 2] > 0.9, (name, p, d)
            else:
                assert not people[k, p].any()


def test_restated_upsampling_interpolates_and_a_plateau_has_no_peak():
    """the cubic weights sum to one, mirror each other and reproduce a constant (a = -0.75 does not reproduce a ramp: only -0.5 would);
    a blob exactly between two pixels is a tie: no peak"""
    tab = R._cubic_table()
    assert np.abs(tab.sum(axis=1) - 1).max() <= 2e-7
    assert np.array_equal(R.upsample8(np.full((3, 4), 0.375, np.float32)), np.full((24, 32), 0.375, np.float32))
    assert np.abs(tab - tab[::-1, ::-1]).max() <= 2e-7
    t = 1 / 16                                                              # phase 0, by the closed form of the kernel with a = -0.75
    assert np.abs(tab[0] - [-0.75 * (t + 1) ** 3 + 3.75 * (t + 1) ** 2 - 6 * (t + 1) + 3, 1.25 * t ** 3 - 2.25 * t ** 2 + 1,
                            1.25 * (1 - t) ** 3 - 2.25 * (1 - t) ** 2 + 1, -0.75 * (2 - t) ** 3 + 3.75 * (2 - t) ** 2 - 6 * (2 - t) + 3]).max() <= 2e-7
    heat, _, _ = R.scene(6, 10, [{0: (40.0, 24.0)}])
    assert R.peaks_ref(heat)[1][0] == 0
    heat, _, _ = R.scene(6, 10, [{0: (40.4, 24.6)}])
    assert R.peaks_ref(heat)[1][0] == 1
