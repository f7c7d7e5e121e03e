"""CPU tests of soar_amd/pose_parts.py: the restatement of tests/pose_parts_ref.py anchored on torch's own operators and
on hand-worked numbers, the configuration read back from a state dict, the refusals, the ABI's new symbols and the JSON round trip.

On the tolerances: the network in float64 differs from ``F.conv2d`` only in the order of seven partial sums per output (1e-12 of values
of order one).  The crop's value is at most 1 in magnitude (a byte / 256 - 0.5): its float32 coordinate carries about 53 x 6e-8 = 3e-6
pixels of rounding at these sizes, times a slope of at most one per pixel, and its interpolation a few 6e-8: 1e-5.  The upsampling sums
sixteen products of values below one: 1e-5."""
import ctypes as C
import json
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pose_parts_ref as R
import pose_ref
from soar_amd import hip_lib, pose, pose_parts, smplify

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"soar_cpm_weights_size", "soar_cpm_workspace_size", "soar_cpm_pack_weights", "soar_cpm_forward", "soar_part_boxes", "soar_part_crop",
       "soar_part_keypoints"}
f32 = np.float32


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the restatement, anchored ----
@pytest.mark.parametrize("cfg", [R.HAND, R.FACE], ids=["hand", "face"])
def test_the_rowwise_network_is_conv2d_in_float64(cfg):
    sd = R.make_state_dict(cfg, seed=3, dtype=torch.float64)
    x = torch.randn(2, 3, 32, 32, generator=_gen(4), dtype=torch.float64) * 0.4
    f_row, s_row = R.RefCpmNet(sd)(x)
    f_one, s_one = R.RefCpmNet(sd, rowwise=False)(x)
    assert len(s_row) == cfg["n_stages"] and all(s.shape == (2, cfg["n_maps"], 4, 4) for s in s_row) and f_row.shape == (2, 8, 4, 4)
    assert torch.equal(f_row, f_one)                                        # (the front has no 7 x 7 layer)
    for a, b in zip(s_row, s_one):
        assert float((a - b).abs().max()) <= 1e-12 and float(b.abs().max()) > 1e-3
    assert not torch.equal(s_row[-1], s_one[-1]) or cfg["n_stages"] == 1     # ... and the order of summation is another


def _grid_sample_crop(img, box, S, mirrored):
    """the same affine grid through torch's bilinear sampler, in float64"""
    H, W, _ = img.shape
    x0, y0, side = (float(v) for v in box[:3])
    s = float(f32(side) / f32(S))
    u = torch.arange(S, dtype=torch.float64)
    xs = x0 + ((S - 1 - u) if mirrored else u) * s
    ys = y0 + u * s
    grid = torch.stack(torch.broadcast_tensors(2 * xs[None, :] / (W - 1) - 1, 2 * ys[:, None] / (H - 1) - 1), dim=-1)[None]
    src = torch.from_numpy(img[:, :, ::-1].copy()).permute(2, 0, 1)[None].double()
    out = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    return (out[0] / 256 - 0.5).numpy()


CROP_BOXES = {"inside": (10.3, 8.6, 20.0), "left": (-6.5, 10.2, 18.0), "right": (40.2, 5.5, 19.0), "top": (12.1, -7.3, 17.0),
              "bottom": (9.7, 25.4, 16.5), "small": (20.4, 14.2, 5.0), "large": (-20.0, -30.0, 90.0)}


@pytest.mark.parametrize("S", [16, 32])
@pytest.mark.parametrize("name", list(CROP_BOXES))
def test_the_crop_is_grid_sample(name, S):
    img = np.random.default_rng(5).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    box = np.array(CROP_BOXES[name] + (1.0,), f32)
    for mirrored in (False, True):
        got = R.crop_one(img, box, S, mirrored)
        want = _grid_sample_crop(img, box, S, mirrored)
        assert got.dtype == np.float32 and got.shape == (3, S, S) and np.abs(got - want).max() <= 1e-5, (name, np.abs(got - want).max())
        assert got.std() > 0.05
    assert np.array_equal(R.crop_one(img, box, S, True), R.crop_one(img, box, S, False)[:, :, ::-1])
    assert np.array_equal(R.crop_one(img, np.zeros(4, f32), S, False), np.full((3, S, S), -0.5, f32))
    assert np.array_equal(R.crop_one(img, np.array([60, 5, 12, 1], f32), S, False), np.full((3, S, S), -0.5, f32))     # wholly outside


def test_an_integer_box_copies_pixels():
    """side == S at an integer corner: every sample is a pixel centre"""
    img = np.random.default_rng(6).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    got = R.crop_one(img, np.array([7, 5, 16, 1], f32), 16, False)
    assert np.array_equal(got, img[5:21, 7:23, ::-1].transpose(2, 0, 1).astype(f32) / f32(256) - f32(0.5))


@pytest.mark.parametrize("hw", [(2, 2), (4, 4), (6, 6)])
def test_the_upsampling_is_torch_bicubic(hw):
    m = torch.rand(1, 1, *hw, generator=_gen(7))
    want = F.interpolate(m, scale_factor=8, mode="bicubic", align_corners=False)[0, 0].numpy()
    got = pose_ref.upsample8(m[0, 0].numpy())
    assert got.shape == want.shape and np.abs(got - want).max() <= 1e-5


# ---- the rectangles: hand-worked numbers ----
def _person(**joints):
    J = np.zeros((25, 3), f32)
    for k, v in joints.items():
        J[int(k[1:])] = v
    return J


def test_hand_boxes_by_hand():
    # right arm: shoulder (100, 100), elbow (100, 140), wrist (130, 180): |wrist - elbow| = 50, 0.9 |elbow - shoulder| = 36
    J = _person(j2=(100, 100, 0.9), j3=(100, 140, 0.8), j4=(130, 180, 0.7))
    x0, y0, side, valid = R.hand_box(J, left=False)
    assert valid == 1 and side == 75 and x0 == f32(130) + f32(0.33) * f32(30) - f32(37.5) and y0 == f32(180) + f32(0.33) * f32(40) - f32(37.5)
    assert abs(float(x0) - 102.4) < 1e-4 and abs(float(y0) - 155.7) < 1e-4
    assert R.hand_box(J, left=True) == (0, 0, 0, 0)                          # the left arm was not seen
    # the upper arm decides: |wrist - elbow| = 10, 0.9 x 100 = 90
    J = _person(j5=(200, 50, 0.5), j6=(200, 150, 0.5), j7=(200, 160, 0.5))
    assert R.hand_box(J, left=True) == (f32(200) - f32(67.5), f32(160) + f32(0.33) * f32(10) - f32(67.5), 135, 1)
    # one joint at the threshold: "greater than" fails
    for j in (5, 6, 7):
        K = J.copy()
        K[j, 2] = f32(0.03)
        assert R.hand_box(K, left=True) == (0, 0, 0, 0)
        K[j, 2] = f32(0.031)
        assert R.hand_box(K, left=True)[3] == 1
    # the area limit: side = 1.5 d, side^2 > 10 from d = 2.11 on
    for d, ok in ((2.10, False), (2.12, True)):
        J = _person(j5=(10, 10, 1), j6=(10, 10, 1), j7=(10 + d, 10, 1))
        assert bool(R.hand_box(J, left=True)[3]) is ok


FACES = {
    # neck (100, 200), nose (100, 150): |neck - nose| = 50; eyes 20 apart, ears 40 apart
    "frontal": (dict(j1=(100, 200, 1), j0=(100, 150, 1), j15=(90, 140, 1), j16=(110, 140, 1), j17=(80, 145, 1), j18=(120, 145, 1)),
                ((100 + 100 + 100) / 3, (175 + 140 + 145) / 3, (100 + 60 + 80) / 3)),
    # left profile: the left eye and ear only; |nose - eye| = 10, |nose - ear| = 50, |neck - nose| = 50
    "left profile": (dict(j1=(100, 200, 1), j0=(100, 150, 1), j16=(110, 150, 1), j18=(150, 150, 1)),
                     (120.0, 150.0, 0.85 * 110)),
    "right profile": (dict(j1=(100, 200, 1), j0=(100, 150, 1), j15=(90, 150, 1), j17=(50, 150, 1)),
                      (80.0, 150.0, 0.85 * 110)),
    "eyes only": (dict(j15=(90, 140, 1), j16=(110, 140, 1)), (100.0, 140.0, 60.0)),
    "ears only": (dict(j17=(80, 145, 1), j18=(120, 145, 1)), (100.0, 145.0, 80.0)),
    "nothing": (dict(j1=(100, 200, 0.25), j0=(100, 150, 1), j15=(90, 140, 0.2)), None),
}


@pytest.mark.parametrize("name", list(FACES))
def test_face_boxes_by_hand(name):
    joints, want = FACES[name]
    got = R.face_box(_person(**joints))
    if want is None:
        assert got == (0, 0, 0, 0)
        return
    cx, cy, size = want
    assert got[3] == 1
    # (the hand-worked values in double; the float32 chain is within a few ulp of them)
    assert np.allclose([float(got[0]), float(got[1]), float(got[2])], [cx - size / 2, cy - size / 2, size], rtol=0, atol=2e-4)
    if name == "eyes only":
        assert got[:3] == (70, 110, 60)                                      # exact where every step is
    if name == "ears only":
        assert got[:3] == (60, 105, 80)


def test_the_face_area_limit_and_the_batch():
    for d, ok in ((2.10, False), (2.12, True)):                             # eyes only: side = 3 d, side^2 > 40 from d = 2.109 on
        assert bool(R.face_box(_person(j15=(50, 50, 1), j16=(50 + d, 50, 1)))[3]) is ok
    people = np.zeros((2, 3, 25, 3), f32)
    people[:, :] = _person(**FACES["frontal"][0])
    boxes = R.boxes_ref(people, np.array([1, 0], np.int32), part_people=2)
    assert boxes.shape == (2, 2, 3, 4) and boxes[0, 0, 2, 3] == 1 and not boxes[0, 1].any() and not boxes[1].any()
    assert not boxes[0, 0, :2].any()                                         # (no arms in that person)


def test_restated_keypoints_map_back_through_the_box():
    heat = np.zeros((2, 4, 4, 3), f32)
    heat[0, 1, 2, 0] = heat[1, 1, 2, 0] = 0.8
    heat[:, :, :, 1] = -0.1
    heat[:, :, :, 2] = np.nan                                                # the background is not read
    boxes = np.array([[[[10, 20, 64, 1], [100, 20, 32, 1], [0, 0, 0, 0]]]], f32)
    kp = R.keypoints_ref(heat, boxes, "hands")
    U = pose_ref.upsample8(heat[0, :, :, 0])
    Y, X = divmod(int(np.argmax(U)), 32)
    assert (Y, X) in ((11, 19), (11, 20), (12, 19), (12, 20))
    assert kp[0, 0].tolist() == [10 + (31 - X) * 2.0, 20 + Y * 2.0, float(U[Y, X])] and kp[1, 0].tolist() == [100 + X * 1.0, 20 + Y * 1.0, float(U[Y, X])]
    assert not kp[:, 1].any()
    assert not R.keypoints_ref(heat[:1], boxes, "face").any()                # rectangle 2 is invalid


# ---- the module ----
@pytest.mark.parametrize("cfg", [R.HAND, R.FACE, R.SHIPPED_HAND], ids=["hand", "face", "shipped"])
def test_configuration_is_read_from_shapes_and_keys(cfg):
    if cfg is R.SHIPPED_HAND:
        sd = {}
        for name, shape in pose_parts.layer_keys(cfg):                      # shapes only
            sd[f"{name}.weight"] = torch.empty(shape, device="meta")
            sd[f"{name}.bias"] = torch.empty(shape[:1], device="meta")
        assert sd["Mconv1_stage2.weight"].shape == (128, 22 + 128, 7, 7) and sd["conv6_1_CPM.weight"].shape == (512, 128, 1, 1)
        got = pose_parts.read_config(sd)
    else:
        sd = R.make_state_dict(cfg, seed=1)
        net = pose_parts.CpmNet(sd)
        got = net.cfg
        assert net.tensor_keys == [k for name, _ in pose_parts.layer_keys(cfg) for k in (f"{name}.weight", f"{name}.bias")]
        assert set(net.tensor_keys) == set(sd) and net.n_maps == cfg["n_maps"]
    assert got == cfg and len(got["width"]) == 17 + 7 * (cfg["n_stages"] - 1)
    assert pose_parts.STAGE_INPUT == ("maps", "features") and pose_parts.POOL_AFTER == ("conv1_2", "conv2_2", "conv3_4")
    c = pose_parts._c_config(cfg)
    assert c.pool_mask == 0b10001010 and c.maps_first == 1 and c.n_layers == len(cfg["width"])


def test_refusals():
    sd = R.make_state_dict(R.HAND, seed=2)
    with pytest.raises(KeyError, match="Mconv3_stage2.bias"):
        pose_parts.CpmNet({k: v for k, v in sd.items() if k != "Mconv3_stage2.bias"})
    with pytest.raises(KeyError, match="conv5_3_CPM.weight"):
        pose_parts.CpmNet({k: v for k, v in sd.items() if k != "conv5_3_CPM.weight"})
    with pytest.raises(KeyError, match="stages 2 .. n"):
        pose_parts.CpmNet({k: v for k, v in sd.items() if not k.startswith("Mconv7_stage2")})
    bad = dict(sd)
    bad["Mconv7_stage3.weight"], bad["Mconv7_stage3.bias"] = sd["Mconv7_stage3.weight"][:21], sd["Mconv7_stage3.bias"][:21]
    with pytest.raises(ValueError, match=r"Mconv7_stage3.weight' has shape \[21, "):
        pose_parts.CpmNet(bad)
    bad = dict(sd)
    bad["conv1_1.weight"] = torch.zeros(12, 3, 3, 3)
    with pytest.raises(ValueError, match="multiple of 8"):
        pose_parts.CpmNet(bad)
    for k in (5, 9):
        bad = dict(sd)
        bad["Mconv2_stage2.weight"] = torch.zeros(8, 8, k, k)
        with pytest.raises(ValueError, match="kernel side must be 1, 3 or 7"):
            pose_parts.CpmNet(bad)
    net = pose_parts.CpmNet(sd)
    msg = "soar_amd.pose_parts runs on HIP devices only; there is no CPU fallback"
    with pytest.raises(RuntimeError, match=msg):
        net(torch.zeros(1, 3, 32, 32))
    with pytest.raises(RuntimeError, match=msg):
        pose_parts.part_boxes(torch.zeros(1, 8, 25, 3), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match=msg):
        pose_parts.crop_parts(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 1, 3, 4), 16)
    with pytest.raises(RuntimeError, match=msg):
        pose_parts.part_keypoints(torch.zeros(2, 2, 2, 22), torch.zeros(1, 1, 3, 4), "hands", 16)
    with pytest.raises(RuntimeError, match=msg):
        pose_parts.detect_parts(net, None, torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 25, 3), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="a CpmNet of 71 maps"):
        pose_parts.detect_parts(None, net, torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 25, 3), torch.zeros(1, dtype=torch.int32))


def test_symbols_sources_and_header():
    from soar_amd import build
    assert NEW <= set(hip_lib.SIGNATURES)
    assert not any(n.endswith("_bytes") or n.endswith("_floats") for n in NEW)
    assert hip_lib.ABI_VERSION == 8
    assert "pose_parts.hip" in build.SOURCES and build.EXTRA_FLAGS["pose_parts.hip"] == ["-ffp-contract=off"]
    header = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    assert all(f"int {name}(" in header for name in NEW) and "#define SOAR_HIP_ABI_VERSION 8" in header
    assert all(f"typedef struct {s} {{" in header for s in ("SoarCpmConfig", "SoarCpmArgs", "SoarPartBoxArgs"))
    assert f"#define SOAR_CPM_FRONT {hip_lib.CPM_FRONT}\n" in header and f"#define SOAR_CPM_MAX_STAGES {hip_lib.CPM_MAX_STAGES}\n" in header
    assert hip_lib.CPM_FRONT == len(pose_parts.FRONT)
    L = hip_lib.lib()                                                       # binds every declared symbol
    assert all(hasattr(L, name) for name in NEW)
    assert "soar_amd.pose_parts" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    import workspace_guard
    assert "soar_amd.pose_parts" in {m.__name__ for m in workspace_guard.modules_with_workspace()}


def test_the_sizing_calls_answer_without_a_device_and_refuse():
    L = hip_lib.lib()
    nb, count = C.c_size_t(0), C.c_int32(0)
    for cfg in (R.HAND, R.FACE, R.SHIPPED_FACE):
        c = pose_parts._c_config(cfg)
        assert L.soar_cpm_weights_size(C.byref(c), C.byref(nb), C.byref(count)) == 0
        assert count.value == 2 * len(cfg["width"]) and nb.value % 256 == 0
        # at least the padded weights: the first layer's 3 channels as 8, the maps' rows and columns as 24 / 72
        assert nb.value >= 4 * sum(np.prod(s) for _, s in pose_parts.layer_keys(cfg))
        assert L.soar_cpm_workspace_size(C.byref(c), 2, 32, C.byref(nb)) == 0 and nb.value % 256 == 0 and nb.value > 0
    c = pose_parts._c_config(R.HAND)
    for S in (0, 4, 36, 370):
        assert L.soar_cpm_workspace_size(C.byref(c), 2, S, C.byref(nb)) != 0 and "multiple of 8" in hip_lib.last_error()
    assert L.soar_cpm_workspace_size(C.byref(c), -1, 32, C.byref(nb)) != 0

    def refused(text, **change):
        c = pose_parts._c_config(R.HAND)
        for k, v in change.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        assert L.soar_cpm_weights_size(C.byref(c), C.byref(nb), None) != 0 and text in hip_lib.last_error(), hip_lib.last_error()
        assert L.soar_cpm_workspace_size(C.byref(c), 1, 32, C.byref(nb)) != 0 and text in hip_lib.last_error()

    refused("multiple of 8", width=(3, 12))
    refused("multiple of 8", width=(17, 4))
    refused("n_maps = 22", width=(16, 24))
    refused("1, 3 or 7", side=(18, 5))
    refused("1, 3 or 7", side=(18, 9))
    refused("n_maps must be", n_maps=1)
    refused("stages", n_stages=9)
    refused("stages", n_layers=30)
    refused("pool_mask", pool_mask=0b1010)
    refused("pool_mask", pool_mask=0b100000000001010)
    assert L.soar_cpm_weights_size(None, C.byref(nb), None) != 0 and "NULL" in hip_lib.last_error()
    # the part kernels' refusals
    a = hip_lib.SoarPartBoxArgs()
    a.B, a.max_people, a.part_people = 1, 8, 0
    assert L.soar_part_boxes(C.byref(a), None) != 0 and "part_people" in hip_lib.last_error()
    a.part_people = 1
    assert L.soar_part_boxes(C.byref(a), None) != 0 and "NULL" in hip_lib.last_error()
    a.B = 0
    assert L.soar_part_boxes(C.byref(a), None) == 0
    assert L.soar_part_crop(1, 8, 8, 1, 0, None, None, None, None, None) != 0
    assert L.soar_part_crop(1, 8, 8, 1, 16, None, None, None, None, None) != 0 and "NULL" in hip_lib.last_error()
    assert L.soar_part_crop(0, 8, 8, 1, 16, None, None, None, None, None) == 0
    assert L.soar_part_keypoints(2, 4, 6, 22, None, None, 0, None, None) != 0 and "h == w" in hip_lib.last_error()
    assert L.soar_part_keypoints(2, 120, 120, 22, None, None, 0, None, None) != 0
    assert L.soar_part_keypoints(3, 4, 4, 22, None, None, 0, None, None) != 0
    assert L.soar_part_keypoints(2, 4, 4, 1, None, None, 0, None, None) != 0
    assert L.soar_part_keypoints(2, 4, 4, 22, None, None, 2, None, None) != 0
    assert L.soar_part_keypoints(2, 4, 4, 22, None, None, 0, None, None) != 0 and "NULL" in hip_lib.last_error()
    assert L.soar_part_keypoints(0, 4, 4, 22, None, None, 1, None, None) == 0


# ---- the files ----
def _write(tmp_path, name, people, n_people, stems, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pose.save_keypoints(str(tmp_path / name), people, n_people, stems, **kw)
    return {s: open(tmp_path / name / f"{s}_keypoints.json", "rb").read() for s in stems}


def test_json_round_trip_with_parts_and_the_bytes_without(tmp_path):
    rng = np.random.default_rng(5)
    people = (rng.random((3, 2, 25, 3)) * 700).astype(f32)
    n_people = np.array([2, 0, 1], np.int32)
    stems = ["00000", "00001", "00002"]
    hands = (rng.random((3, 1, 2, 21, 3)) * 700).astype(f32)
    face = (rng.random((3, 1, 70, 3)) * 700).astype(f32)
    hands[1], face[1] = 0, 0
    # without the new arguments: the bytes of the writer as it was
    plain = _write(tmp_path, "plain", people, n_people, stems)
    zeros = lambda n: [0.0] * (3 * n)
    for i, s in enumerate(stems):
        n = int(n_people[i])
        rows = people[i, :n] if n else np.zeros((1, 25, 3), f32)
        doc = {"version": 1.3, "people": [{"person_id": [-1], "pose_keypoints_2d": [float(v) for v in row.reshape(-1)],
                                           "face_keypoints_2d": zeros(70), "hand_left_keypoints_2d": zeros(21),
                                           "hand_right_keypoints_2d": zeros(21)} for row in rows]}
        assert plain[s] == json.dumps(doc).encode()
    assert _write(tmp_path, "none", people, n_people, stems, hands=None, face=None) == plain
    # with them: read back bit for bit
    full = _write(tmp_path, "full", torch.from_numpy(people), torch.from_numpy(n_people), stems, hands=torch.from_numpy(hands), face=face)
    kp = smplify.load_keypoints(str(tmp_path / "full"))
    assert kp.shape == (3, 137, 3) and kp.dtype == np.float32
    for i in (0, 2):
        assert np.array_equal(kp[i, :25], people[i, 0]) and np.array_equal(kp[i, 25:46], hands[i, 0, 0]) and np.array_equal(kp[i, 46:67], hands[i, 0, 1])
        assert np.array_equal(kp[i, 67:], face[i, 0])
    assert not kp[1].any() and kp[0, 25:].all()
    doc = json.loads(full["00000"])
    assert len(doc["people"]) == 2 and not any(doc["people"][1]["hand_left_keypoints_2d"]) and not any(doc["people"][1]["face_keypoints_2d"])
    assert [len(doc["people"][0][k]) for k in ("pose_keypoints_2d", "face_keypoints_2d", "hand_left_keypoints_2d", "hand_right_keypoints_2d")] == [75, 210, 63, 63]
    only_face = _write(tmp_path, "face", people, n_people, stems, face=face)
    kp = smplify.load_keypoints(str(tmp_path / "face"))
    assert not kp[:, 25:67].any() and np.array_equal(kp[2, 67:], face[2, 0]) and only_face != plain
    with pytest.raises(ValueError, match=r"hands \[N,P,2,21,3\]"):
        pose.save_keypoints(str(tmp_path / "bad"), people, n_people, stems, hands=hands[:, :, :, :20])
