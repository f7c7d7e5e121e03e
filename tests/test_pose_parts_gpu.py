"""GPU tests of soar_amd/pose_parts.py (csrc/pose_parts.hip) against tests/pose_parts_ref.py.

* The networks: every stage and the features within FACTOR = 4 times the float32 restatement's own distance from the float64 one (the
  bar, the helper and the print format of tests/test_pose_gpu.py), with the real map counts (22 -> 24 and 71 -> 72 padded channels), at
  4 x 4 and 6 x 6 maps, where the 7 x 7 kernel overhangs every border; batches against single calls bit for bit.
* Rectangles, crops and maxima: bit for bit against the NumPy float32 restatement; the mapping back to the image once more against a
  planted blob, without the restatement.
* The stage composed, the sequence in ragged chunks, its files; the workspace between guard bands over zeros, 0xFF and noise."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import pose_parts_ref as R
import pose_ref
import test_pose_parts_cpu as CPU
import workspace_guard as W
from soar_amd import hip_lib, pose, pose_parts

pytestmark = pytest.mark.gpu
FACTOR = 4.0
f32 = np.float32
_cache = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the networks ----
CFGS = {"hand": R.HAND, "face": R.FACE}
SIZES = (32, 48)


def rel(a, b):
    """worst element of a - b over b's RMS (b: float64)"""
    return float((a.double().cpu() - b).abs().max() / b.pow(2).mean().sqrt())


def within(name, got, ref64, ref32):
    e32 = rel(ref32, ref64)
    err = rel(got, ref64)
    print(f"{name}: err {err:.3g}  e32 {e32:.3g}  ratio {err / e32 if e32 else float('inf'):.2f}")
    assert err <= FACTOR * e32, f"{name}: {err:.3g} from float64, float32 restatement {e32:.3g}: ratio {err / e32:.2f} > {FACTOR}"


def _net_case(cname, S, dev):
    """the net, a batch of three and the restatement's stages in float64 and float32 (NHWC), computed once"""
    if (cname, S) not in _cache:
        cfg = CFGS[cname]
        sd = R.make_state_dict(cfg, seed=11)
        x = torch.randn(3, 3, S, S, generator=_gen(12)) * 0.4
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
        refs = {}
        for dt in (torch.float64, torch.float32):
            f, st = R.RefCpmNet({k: v.to(dt) for k, v in sd.items()})(x.to(dt))
            refs[dt] = (nhwc(f), [nhwc(s) for s in st])
        net = pose_parts.CpmNet(sd).to(dev)
        xd = x.to(dev)
        _cache[cname, S] = dict(cfg=cfg, sd=sd, x=xd, net=net, r64=refs[torch.float64], r32=refs[torch.float32],
                                hip=net(xd, return_stages=True))
    return _cache[cname, S]


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("cname", list(CFGS))
def test_network_against_float64(cname, S, M, dev):
    c = _net_case(cname, S, dev)
    cfg = c["cfg"]
    heat, features, stages = c["hip"] if M == 3 else c["net"](c["x"][:1], return_stages=True)
    h = S // 8
    assert cfg["n_maps"] in (22, 71) and cfg["n_stages"] == (3 if cname == "hand" else 2) and len(stages) == cfg["n_stages"]
    assert features.shape == (M, h, h, 8) and heat.shape == (M, h, h, cfg["n_maps"]) and heat.is_contiguous()
    f64, s64 = c["r64"]
    f32_, s32 = c["r32"]
    tag = f"cpm {cname} S={S} M={M}"
    within(f"{tag} features", features, f64[:M], f32_[:M])
    for s, got in enumerate(stages):
        within(f"{tag} stage {s + 1}", got, s64[s][:M], s32[s][:M])
    assert torch.equal(heat, stages[-1]) and bool(torch.isfinite(heat).all())


@pytest.mark.parametrize("cname,S", [("hand", 32), ("face", 48)])
def test_a_crop_in_a_batch_is_bit_equal_to_the_single_call(cname, S, dev):
    c = _net_case(cname, S, dev)
    flat = lambda out: (out[0], out[1], *out[2])
    again = flat(c["net"](c["x"], return_stages=True))
    batch = flat(c["hip"])
    for i in range(3):
        one = flat(c["net"](c["x"][i:i + 1], return_stages=True))
        for got, b, rep in zip(one, batch, again):
            assert torch.equal(_bits(got[0]), _bits(b[i])) and torch.equal(_bits(rep), _bits(b))
    assert torch.equal(c["net"](c["x"]), c["hip"][0])


def test_strided_input_is_bit_equal_and_the_empty_batch(dev):
    c = _net_case("hand", 32, dev)
    cl = c["x"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl.is_contiguous()
    assert torch.equal(_bits(c["net"](cl)), _bits(c["hip"][0]))
    wide = torch.zeros(3, 3, 40, 60, device=dev)
    wide[:, :, 3:35, 5:37] = c["x"]
    assert torch.equal(_bits(c["net"](wide[:, :, 3:35, 5:37])), _bits(c["hip"][0]))
    heat = c["net"](c["x"][:0])
    assert heat.shape == (0, 4, 4, 22) and heat.is_cuda
    heat, features, stages = c["net"](c["x"][:0], return_stages=True)
    assert features.shape == (0, 4, 4, 8) and len(stages) == 3
    with pytest.raises(ValueError, match="multiple of 8"):
        c["net"](torch.zeros(1, 3, 36, 36, device=dev))
    with pytest.raises(ValueError, match=r"\[M,3,S,S\]"):
        c["net"](torch.zeros(1, 3, 32, 40, device=dev))


def test_packed_weights_are_kept_repacked_and_refused(dev):
    net = pose_parts.CpmNet(R.make_state_dict(R.HAND, seed=31)).to(dev)
    x = (torch.randn(1, 3, 16, 16, generator=_gen(32)) * 0.4).to(dev)
    first = net(x)
    assert first.abs().sum().item() > 0
    packed = net._packed(dev)
    assert net._packed(dev) is packed and torch.equal(net(x), first)
    net.t0[0].neg_()                                                       # one output channel of conv1_1
    assert net._packed(dev) is not packed
    assert not torch.equal(net(x), first)
    net.cpu()
    with pytest.raises(RuntimeError, match=r"CpmNet: weights are not on cuda:\d+: move the module with \.to"):
        net(x)


def test_a_3x3_and_1x1_stage_is_the_same_machine(dev):
    """every side the launcher takes, in one net: 3 x 3 in the later stages goes through the single launch with the fused ReLU"""
    cfg = R.make_cfg(22, 2, stage_side=3)
    cfg["side"][R.N_FRONT - 1] = 7                                          # ... and a 7 x 7 that writes the stage row's feature slice
    cfg["side"][R.N_FRONT + 1] = 7                                          # ... and one that writes the padded maps, without a ReLU
    sd = R.make_state_dict(cfg, seed=41)
    x = torch.randn(2, 3, 32, 32, generator=_gen(42)) * 0.4
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    f64, s64 = R.RefCpmNet({k: v.double() for k, v in sd.items()})(x.double())
    f32_, s32 = R.RefCpmNet(sd)(x)
    heat, features, stages = pose_parts.CpmNet(sd).to(dev)(x.to(dev), return_stages=True)
    within("cpm mixed sides features", features, nhwc(f64), nhwc(f32_))
    for s in range(2):
        within(f"cpm mixed sides stage {s + 1}", stages[s], nhwc(s64[s]), nhwc(s32[s]))
    assert bool((stages[0] < 0).any())                                      # the maps carry no ReLU


# ---- part_boxes ----
def _box_people():
    """[B,8,25,3] and n_people: the CPU test's persons and the edge cases, one frame each"""
    persons = [CPU._person(**j) for j, _ in CPU.FACES.values()]
    arm = CPU._person(j2=(100, 100, 0.9), j3=(100, 140, 0.8), j4=(130, 180, 0.7), j5=(200, 50, 0.5), j6=(200, 150, 0.5), j7=(200, 160, 0.5))
    persons.append(arm)
    for j in (5, 6, 7):
        k = arm.copy()
        k[j, 2] = f32(0.03)
        persons.append(k)
    neg = arm.copy()
    neg[:, :2] -= f32(400.25)                                               # negative coordinates
    neg[[0, 1, 15, 16], :] = [(-30.5, -80.25, 1), (-30.5, -20.75, 1), (-40.5, -90.25, 1), (-20.5, -90.5, 1)]
    persons.append(neg)
    for d in (2.10, 2.108, 2.109, 2.12):                                    # just under and just over either area limit
        persons.append(CPU._person(j5=(10, 10, 1), j6=(10, 10, 1), j7=(10 + d, 10, 1), j15=(50, 50, 1), j16=(50 + d, 50, 1)))
    rng = np.random.default_rng(8)
    for _ in range(6):
        p = (rng.random((25, 3)) * [300, 200, 1]).astype(f32)
        p[rng.random(25) < 0.3, 2] = 0
        persons.append(p)
    B = len(persons)
    people = np.zeros((B, 8, 25, 3), f32)
    people[:, 0] = persons
    people[:, 1] = persons[::-1]
    n_people = np.full((B,), 2, np.int32)
    n_people[-1], n_people[-2], n_people[-3] = 0, 1, 9                       # nobody; one person; more than the rows hold
    return people, n_people


@pytest.mark.parametrize("part_people", [1, 2, 3])
def test_part_boxes_bit_for_bit(part_people, dev):
    people, n_people = _box_people()
    want = R.boxes_ref(people, n_people, part_people)
    got = pose_parts.part_boxes(torch.from_numpy(people).to(dev), torch.from_numpy(n_people).to(dev), part_people)
    assert got.shape == want.shape and _same_bits(got.cpu().numpy(), want), np.argwhere(got.cpu().numpy() != want)[:5]
    valid = want[..., 3]
    assert set(np.unique(valid)) == {0.0, 1.0} and valid[:, 0].sum() > 10 and not want[valid == 0].any()
    assert not want[-1].any() and (part_people < 2 or (not want[-2, 1].any() and want[-4, 1].any()))
    if part_people == 3:
        assert not want[:, 2].any()                                         # person 2: beyond n_people everywhere but frame -3, whose row is zeros
    assert (want[valid == 1][:, 0] < 0).any()
    # the thresholds are arguments
    kw = dict(hand_min_conf=0.6, min_hand_area=3000.0, face_min_conf=0.5, min_face_area=5000.0)
    want2 = R.boxes_ref(people, n_people, part_people, **kw)
    got2 = pose_parts.part_boxes(torch.from_numpy(people).to(dev), torch.from_numpy(n_people).to(dev), part_people, **kw)
    assert _same_bits(got2.cpu().numpy(), want2) and 0 < want2[..., 3].sum() < valid.sum()
    empty = pose_parts.part_boxes(torch.zeros(0, 8, 25, 3, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), part_people)
    assert empty.shape == (0, part_people, 3, 4)


# ---- crop_parts ----
def _crop_case():
    """frames of 37 x 53 and boxes [B,2,3,4]: inside, over each side, wholly outside, smaller and larger than the crop, invalid"""
    if "crop" not in _cache:
        img = np.random.default_rng(5).integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)
        rows = [v + (1.0,) for v in CPU.CROP_BOXES.values()] + [(60.0, 5.0, 12.0, 1.0), (-40.0, -50.0, 30.0, 1.0), (0.0, 0.0, 0.0, 0.0),
                                                                  (7.0, 5.0, 16.0, 1.0), (3.25, 2.5, 32.0, 1.0)]
        rows = rows + rows[:18 - len(rows)]
        boxes = np.array(rows, f32).reshape(3, 2, 3, 4)
        _cache["crop"] = (img, boxes)
    return _cache["crop"]


@pytest.mark.parametrize("S", [16, 32])
def test_crop_parts_bit_for_bit(S, dev):
    img, boxes = _crop_case()
    want_h, want_f = R.crop_ref(img, boxes, S)
    d_img, d_boxes = torch.from_numpy(img).to(dev), torch.from_numpy(boxes).to(dev)
    hands, faces = pose_parts.crop_parts(d_img, d_boxes, S)
    assert hands.shape == (12, 3, S, S) and faces.shape == (6, 3, S, S)
    assert _same_bits(hands.cpu().numpy(), want_h) and _same_bits(faces.cpu().numpy(), want_f)
    flat = boxes.reshape(-1, 4)
    # what the cases are: wholly outside and invalid are all -0.5, the others are pictures; a left hand is the mirror image
    for k, b in enumerate(flat):
        frame, q, which = k // 6, (k // 3) % 2, k % 3
        crop = (want_h[(frame * 2 + q) * 2 + which] if which < 2 else want_f[frame * 2 + q])
        outside = b[3] == 0 or b[0] >= 53 or b[1] >= 37 or b[0] + b[2] <= -1 or b[1] + b[2] <= -1
        assert bool((crop == -0.5).all()) == bool(outside), (k, b)
        if which == 0 and not outside:
            assert np.array_equal(crop, R.crop_one(img[frame], b, S, False)[:, :, ::-1])
    assert sum(1 for b in flat if b[3] and b[2] < S) and sum(1 for b in flat if b[2] > S)
    # a frame in a batch equals the single call, and either output by itself
    one_h, one_f = pose_parts.crop_parts(d_img[1:2], d_boxes[1:2], S)
    assert torch.equal(_bits(one_h), _bits(hands[4:8])) and torch.equal(_bits(one_f), _bits(faces[2:4]))
    only_h, none = pose_parts.crop_parts(d_img, d_boxes, S, faces=False)
    assert none is None and torch.equal(_bits(only_h), _bits(hands))
    none, only_f = pose_parts.crop_parts(d_img, d_boxes, S, hands=False)
    assert none is None and torch.equal(_bits(only_f), _bits(faces))
    eh, ef = pose_parts.crop_parts(d_img[:0], d_boxes[:0], S)
    assert eh.shape == (0, 3, S, S) and ef.shape == (0, 3, S, S)


# ---- part_keypoints ----
def _blob(h, cx, cy, s=0.9):
    gy, gx = np.mgrid[0:h, 0:h].astype(np.float64)
    return np.exp(-((gx - cx) ** 2 + (gy - cy) ** 2) / (2 * s * s)).astype(f32)


def _keypoint_case(h):
    """heat [8,h,h,5] for the hands of two frames of two persons (the first four: their faces), boxes [2,2,3,4]: a blob, a corner maximum, two equal maxima, an
    all-negative map; the background NaN"""
    heat = np.zeros((8, h, h, 5), f32)
    rng = np.random.default_rng(h)
    for m in range(8):
        heat[m, :, :, 0] = _blob(h, 0.3 * h + 0.2 * m, 0.6 * h - 0.1 * m)
        heat[m, :, :, 1] = 0.1 * rng.random((h, h), dtype=f32)
        heat[m, (0, h - 1)[m & 1], (0, h - 1)[(m >> 1) & 1], 1] = 0.9             # the maximum in a corner cell: clamped borders
        if h == 6:
            # two exactly equal maxima: columns (a, b, a, a, b, a) give the cells 1 and 4 the same four-tap windows in every phase
            col_a, col_b = 0.05 + 0.01 * rng.random(h, dtype=f32), 0.3 + 0.4 * _blob(h, 0, 2.3 + 0.2 * m)[:, 0]
            heat[m, :, :, 2] = col_a[:, None]
            heat[m, :, 1, 2] = heat[m, :, 4, 2] = col_b
        else:
            # ... or many: a map that is constant along x repeats every 8 pixels
            heat[m, :, :, 2] = (0.2 + 0.5 * rng.random(h, dtype=f32))[:, None]
        heat[m, :, :, 3] = -0.5 - 0.1 * rng.random((h, h), dtype=f32)   # (far enough below 0 for the cubic's overshoot)
    heat[..., 4] = np.nan
    boxes = np.array([[[[10.5, 20.25, 60.0, 1], [100.0, -20.0, 33.3, 1], [40.0, 40.0, 90.0, 1]],
                       [[-30.0, 5.0, 12.0, 1], [0, 0, 0, 0], [7.0, 9.0, 20.0, 1]]],
                      [[[0, 0, 0, 0], [300.0, 200.0, 150.0, 1], [0, 0, 0, 0]],
                       [[1.0, 2.0, 3.0, 1], [5.0, 6.0, 700.0, 1], [50.0, 60.0, 64.0, 1]]]], f32)
    return heat, boxes


@pytest.mark.parametrize("which", ["hands", "face"])
@pytest.mark.parametrize("h", [2, 4, 6])
def test_part_keypoints_bit_for_bit(h, which, dev):
    heat, boxes = _keypoint_case(h)
    if which == "face":
        heat = heat[:4]                                                     # faces are rectangle 2: one crop a person
    want = R.keypoints_ref(heat, boxes, which)
    got = pose_parts.part_keypoints(torch.from_numpy(heat).to(dev), torch.from_numpy(boxes).to(dev), which, 8 * h)
    assert got.shape == (heat.shape[0], 4, 3) and _same_bits(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    flat = boxes.reshape(-1, 3, 4)
    for m in range(heat.shape[0]):
        box = flat[m // 2, m % 2] if which == "hands" else flat[m, 2]
        if box[3] == 0:
            assert not want[m].any()                                        # an invalid box
            continue
        assert (want[m, :3, 2] > 0).all() and not want[m, 3].any()          # an all-negative map
        s, WW = box[2] / f32(8 * h), 8 * h
        # the corner: the winner lies in that corner's cell; the tie: the first in raster order
        Y, X = ((WW - 1) * (c > 0) for c in np.argwhere(heat[m, :, :, 1] == f32(0.9))[0])
        left = which == "hands" and m % 2 == 0
        U = pose_ref.upsample8(heat[m, :, :, 1])
        Yw, Xw = divmod(int(np.argmax(U)), WW)
        assert abs(Xw - X) < 8 and abs(Yw - Y) < 8 and (U == U.max()).sum() == 1
        assert want[m, 1, 0] == box[0] + f32(WW - 1 - Xw if left else Xw) * s and want[m, 1, 1] == box[1] + f32(Yw) * s
        U = pose_ref.upsample8(heat[m, :, :, 2])
        ties = np.argwhere(U == U.max())
        assert len(ties) >= 2 and (h != 6 or (ties[0][0], ties[0][1] + 24) in set(map(tuple, ties)))
        Yw, Xw = ties[0]
        assert want[m, 2, 0] == box[0] + f32(WW - 1 - Xw if left else Xw) * s and want[m, 2, 1] == box[1] + f32(Yw) * s
    # a crop in a batch equals the single frame's call
    mine = slice(4, 8) if which == "hands" else slice(2, 4)                 # frame 1's crops
    one = pose_parts.part_keypoints(torch.from_numpy(heat[mine]).to(dev), torch.from_numpy(boxes[1:2]).to(dev), which, 8 * h)
    assert torch.equal(_bits(one), _bits(got[mine]))
    empty = pose_parts.part_keypoints(torch.zeros(0, h, h, 5, device=dev), torch.zeros(0, 2, 3, 4, device=dev), which, 8 * h)
    assert empty.shape == (0, 4, 3)


@pytest.mark.parametrize("cy,cx", [(0, 0), (2, 3), (5, 1), (3, 5)])
def test_a_planted_blob_maps_back_to_the_image(cy, cx, dev):
    """independent of the restatement: cell (cy, cx) of a 6 x 6 map covers crop pixels 8 c .. 8 c + 7, centre 8 c + 3.5; the keypoint lies
    within 4 s of that place in the image, for a left hand at the mirrored column"""
    gy, gx = np.mgrid[0:6, 0:6].astype(np.float64)
    heat = np.zeros((2, 6, 6, 22), f32)
    heat[:, :, :, 7] = np.exp(-((gx - cx) ** 2 + (gy - cy) ** 2) / 2).astype(f32)[None]
    boxes = np.array([[[[100.0, 50.0, 96.0, 1], [300.0, 20.0, 24.0, 1], [10.0, 10.0, 144.0, 1]]]], f32)
    kp = pose_parts.part_keypoints(torch.from_numpy(heat).to(dev), torch.from_numpy(boxes).to(dev), "hands", 48).cpu().numpy()
    face = pose_parts.part_keypoints(torch.from_numpy(heat[:1]).to(dev), torch.from_numpy(boxes).to(dev), "face", 48).cpu().numpy()
    for got, (x0, y0, side, _), col in ((kp[0, 7], boxes[0, 0, 0], 5 - cx), (kp[1, 7], boxes[0, 0, 1], cx), (face[0, 7], boxes[0, 0, 2], cx)):
        s = side / 48
        want = (x0 + (8 * col + 3.5) * s, y0 + (8 * cy + 3.5) * s)
        assert np.hypot(got[0] - want[0], got[1] - want[1]) <= 4 * s and got[2] > 0.9, (got, want, s)
    assert not kp[:, :7].any() and not kp[:, 8:].any()


# ---- the stage ----
LOOSE = dict(threshold=0.0, inter_threshold=-100.0, min_above=-1.0, min_score=-1e9, min_parts=2)


@pytest.fixture(scope="module")
def stage(dev):
    """a body net, a hand net and a face net with random weights, five frames, and people put where the rectangles hold picture"""
    body = pose.PoseNet(pose_ref.make_state_dict(pose_ref.TINY, seed=61)).to(dev)
    hand = pose_parts.CpmNet(R.make_state_dict(R.HAND, seed=63)).to(dev)
    face = pose_parts.CpmNet(R.make_state_dict(R.FACE, seed=64)).to(dev)
    img = torch.randint(0, 256, (5, 45, 72, 3), generator=_gen(62), dtype=torch.uint8).to(dev)
    return body, hand, face, img


def _people_for(img, dev):
    B = img.shape[0]
    person = CPU._person(j1=(36, 30, 1), j0=(36, 18, 1), j15=(32, 15, 1), j16=(40, 15, 1), j17=(28, 17, 1), j18=(44, 17, 1),
                         j2=(24, 30, 0.9), j3=(18, 38, 0.8), j4=(14, 44, 0.7), j5=(48, 30, 0.9), j6=(54, 37, 0.8), j7=(80, 40, 0.7))
    people = np.zeros((B, 8, 25, 3), f32)
    people[:, 0] = person
    people[:, 1] = person
    people[:, 1, :, :2] *= f32(0.75)                                        # a second, smaller person
    people[:, :, :, :2] += np.arange(B, dtype=f32)[:, None, None, None]
    n_people = np.array(([2, 1, 0, 2, 1] * B)[:B], np.int32)
    return torch.from_numpy(people).to(dev), torch.from_numpy(n_people).to(dev)


@pytest.mark.parametrize("part_people", [1, 2])
def test_detect_parts_is_the_stages_composed(stage, part_people, dev):
    _, hand, face, img = stage
    people, n_people = _people_for(img, dev)
    hands, fc = pose_parts.detect_parts(hand, face, img, people, n_people, part_people, net_side=32)
    P = part_people
    assert hands.shape == (5, P, 2, 21, 3) and fc.shape == (5, P, 70, 3)
    boxes = pose_parts.part_boxes(people, n_people, P)
    xh, xf = pose_parts.crop_parts(img, boxes, 32)
    want_h = pose_parts.part_keypoints(hand(xh), boxes, "hands", 32).view(5, P, 2, 21, 3)
    want_f = pose_parts.part_keypoints(face(xf), boxes, "face", 32).view(5, P, 70, 3)
    assert torch.equal(_bits(hands), _bits(want_h)) and torch.equal(_bits(fc), _bits(want_f))
    # ... and every stage on the device's data is the restatement's
    b = boxes.cpu().numpy()
    assert _same_bits(b, R.boxes_ref(people.cpu().numpy(), n_people.cpu().numpy(), P))
    rh, rf = R.crop_ref(img.cpu().numpy(), b, 32)
    assert _same_bits(xh.cpu().numpy(), rh) and _same_bits(xf.cpu().numpy(), rf)
    assert _same_bits(want_h.cpu().numpy().reshape(-1, 21, 3), R.keypoints_ref(hand(xh).cpu().numpy(), b, "hands"))
    assert _same_bits(want_f.cpu().numpy().reshape(-1, 70, 3), R.keypoints_ref(face(xf).cpu().numpy(), b, "face"))
    # the content: persons that exist have keypoints in all three parts (random maps have positive maxima), the others none
    nh = n_people.cpu().numpy()
    for i in range(5):
        for q in range(P):
            there = q < nh[i]
            assert bool(b[i, q, :, 3].all()) == there
            assert bool(hands[i, q, :, :, 2].any()) == there and bool(fc[i, q, :, 2].any()) == there
    # either net may be missing: its rows are zeros, the other's the same bits
    only_h, zf = pose_parts.detect_parts(hand, None, img, people, n_people, P, net_side=32)
    zh, only_f = pose_parts.detect_parts(None, face, img, people, n_people, P, net_side=32)
    assert torch.equal(_bits(only_h), _bits(hands)) and torch.equal(_bits(only_f), _bits(fc)) and not zf.any() and not zh.any()
    # a frame in a batch equals the single call
    one_h, one_f = pose_parts.detect_parts(hand, face, img[3:4], people[3:4], n_people[3:4], P, net_side=32)
    assert torch.equal(_bits(one_h[0]), _bits(hands[3])) and torch.equal(_bits(one_f[0]), _bits(fc[3]))


def test_detect_sequence_with_part_nets_in_ragged_chunks_and_its_files(stage, dev, tmp_path):
    from soar_amd import smplify
    body, hand, face, img = stage
    kw = dict(net_height=32, hand_net=hand, face_net=face, part_net_side=32, **LOOSE)
    whole = pose.detect_sequence(body, img, chunk=5, **kw)
    ragged = pose.detect_sequence(body, img.cpu(), chunk=2, device=dev, **kw)
    assert whole.shape == (5, 137, 3) and whole.dtype == np.float32 and _same_bits(whole, ragged)
    plain = pose.detect_sequence(body, img, chunk=5, net_height=32, **LOOSE)
    assert _same_bits(whole[:, :25], plain[:, :25]) and not plain[:, 25:].any() and plain[:, :25, 2].any()
    # the rows are detect_parts' of the first person
    people, n_people = pose.detect(body, img, net_height=32, **LOOSE)
    hands, fc = pose_parts.detect_parts(hand, face, img, people, n_people, 1, net_side=32)
    assert _same_bits(whole[:, 25:46], hands[:, 0, 0].cpu().numpy()) and _same_bits(whole[:, 46:67], hands[:, 0, 1].cpu().numpy())
    assert _same_bits(whole[:, 67:], fc[:, 0].cpu().numpy())
    only = pose.detect_sequence(body, img, chunk=3, net_height=32, face_net=face, part_net_side=32, **LOOSE)
    assert _same_bits(only[:, 67:], whole[:, 67:]) and not only[:, 25:67].any()
    # the files: hands and face written and read back bit for bit
    pose.save_keypoints(str(tmp_path / "kp"), people, n_people, [f"{i:05d}" for i in range(5)], hands=hands, face=fc)
    assert _same_bits(smplify.load_keypoints(str(tmp_path / "kp")), whole)
    # a random body net's people need not have arms and a head the rules accept: the rows' content is planted below
    planted, n_planted = _people_for(img, dev)
    n_planted[:] = 1
    hands, fc = pose_parts.detect_parts(hand, face, img, planted, n_planted, 1, net_side=32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pose.save_keypoints(str(tmp_path / "planted"), planted, n_planted, [f"{i:05d}" for i in range(5)], hands=hands, face=fc)
    kp = smplify.load_keypoints(str(tmp_path / "planted"))
    assert _same_bits(kp[:, :25], planted[:, 0].cpu().numpy()) and _same_bits(kp[:, 25:67], hands[:, 0].reshape(5, 42, 3).cpu().numpy())
    assert _same_bits(kp[:, 67:], fc[:, 0].cpu().numpy())
    assert all((kp[:, a:b, 2] > 0).any(axis=1).all() for a, b in ((25, 46), (46, 67), (67, 137)))     # non-zero rows in every part of every frame


def test_a_frame_with_nobody_in_it_is_all_zeros(stage, dev):
    body, hand, face, img = stage
    tight = dict(LOOSE, min_parts=26)                                       # nobody has 26 parts
    kp = pose.detect_sequence(body, img[:3], chunk=2, net_height=32, hand_net=hand, face_net=face, part_net_side=32, **tight)
    assert kp.shape == (3, 137, 3) and not kp.any()


# ---- the workspace contract ----
def test_workspace_contract(dev):
    """CpmNet's two allocations (the packed weights, the forward's workspace) between guard bands over every fill: the bands intact,
    the sizes exactly the sizing calls', the outputs finite and the same bits as outside any context; the part kernels take no workspace"""
    sds = {"hand": R.make_state_dict(R.HAND, seed=71), "face": R.make_state_dict(R.FACE, seed=72)}
    x = (torch.randn(2, 3, 32, 32, generator=_gen(73)) * 0.4).to(dev)
    img = torch.randint(0, 256, (2, 40, 75, 3), generator=_gen(74), dtype=torch.uint8).to(dev)
    people, n_people = _people_for(img, dev)

    def run():
        out = []
        nets = {}
        for name, sd in sds.items():
            nets[name] = pose_parts.CpmNet(sd).to(dev)
            heat, features, stages = nets[name](x, return_stages=True)
            out += [heat, features, *stages]
        out += pose_parts.detect_parts(nets["hand"], nets["face"], img, people, n_people, 1, net_side=48)
        return out

    plain = run()
    L = hip_lib.lib()
    sizes = []
    for cfg in (R.HAND, R.FACE):
        c = pose_parts._c_config(cfg)
        nb = C.c_size_t(0)
        hip_lib.check(L.soar_cpm_weights_size(C.byref(c), C.byref(nb), None), "soar_cpm_weights_size")
        sizes += [nb.value, hip_lib._bytes(L.soar_cpm_workspace_size, "soar_cpm_workspace_size", C.byref(c), 2, 32)]
    sizes += [hip_lib._bytes(L.soar_cpm_workspace_size, "soar_cpm_workspace_size", C.byref(pose_parts._c_config(R.HAND)), 4, 48),
              hip_lib._bytes(L.soar_cpm_workspace_size, "soar_cpm_workspace_size", C.byref(pose_parts._c_config(R.FACE)), 2, 48)]
    for fill in W.FILLS:
        with W.guarded(fill) as g:
            got = run()
            g.check()
            asked = [(nbytes, who) for _, nbytes, who, _ in g.buffers]
            assert asked == [(s, "soar_amd.pose_parts") for s in sizes], asked
            for a, b in zip(got, plain):
                assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), fill
