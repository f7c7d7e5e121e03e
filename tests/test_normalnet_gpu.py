"""GPU tests of the normal-map preprocessing (csrc/normalnet.hip, csrc/normal_io.hip, soar_amd/normals.py) against the
restatement of tests/normalnet_ref.py: the networks against float64 on the device, with torch-float32 (MIOpen) as the yardstick of
what float32 can reach; the crop, the bytes and the whole stage."""
import math

import pytest
import torch

import normalnet_ref as ref
from soar_amd import normals

pytestmark = pytest.mark.gpu

# Measured on an MI355X: distance to the float64 restatement, (worst element, relative L2), of the HIP path and of the
# same network composed from torch-float32 on the same inputs.  The bars are twice the larger of the two, rounded up to one digit
# (the margin is for box-to-box differences in MIOpen's own order of summation); torch-float32's own distance is capped as well, so
# a broken oracle fails.
#   case: side F / B: (HIP worst, HIP L2, torch worst, torch L2)
MEASURED = {
    "bottom2x2": ((2.9525e-05, 4.1236e-06, 2.1720e-05, 4.5307e-06), (4.9657e-05, 9.8635e-06, 6.8109e-05, 1.5113e-05)),
    "offtile": ((5.6153e-05, 2.6283e-06, 2.0951e-05, 1.6183e-06), (3.1068e-05, 3.6929e-06, 1.9687e-05, 2.2544e-06)),
    "workload": ((3.4403e-04, 4.3120e-06, 2.3062e-04, 2.9038e-06), (1.0134e-04, 4.0219e-06, 7.7820e-05, 2.8411e-06)),
    "tiles128": ((5.5390e-05, 2.1829e-06, 3.8569e-05, 1.8367e-06), (6.2726e-05, 1.7549e-06, 5.0641e-05, 1.5899e-06)),
}


def _bar(v):
    """twice v, rounded up to one digit"""
    d = 10.0 ** math.floor(math.log10(2 * v))
    return math.ceil(2 * v / d) * d


# (worst element, relative L2): bottom2x2 2e-4, 4e-5; offtile 2e-4, 8e-6; workload 7e-4, 9e-6; tiles128 2e-4, 5e-6
BARS = {name: (_bar(max(max(s[0], s[2]) for s in sides)), _bar(max(max(s[1], s[3]) for s in sides))) for name, sides in MEASURED.items()}
assert [f"{b:.0e}" for name in ("bottom2x2", "offtile", "workload", "tiles128") for b in BARS[name]] == ["2e-04", "4e-05", "2e-04", "8e-06", "7e-04", "9e-06",
                                                                                                       "2e-04", "5e-06"]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


_cache = {}


def _case(name, dev):
    """inputs, the module, its output, the float64 and the float32 restatement: computed once, shared, left unchanged"""
    if name not in _cache:
        c = ref.make_case(name, dev)
        net = normals.NormalNet(c["sd"], *c["cfg"]).to(dev)
        c["net"] = net
        c["hip"] = net(c["image"], c["prior_F"], c["prior_B"])
        sd64 = {k: v.double() for k, v in c["sd"].items()}
        c["f64"] = ref.normalnet(c["image"], c["prior_F"], c["prior_B"], sd64, *c["cfg"], dtype=torch.float64)
        c["f32"] = ref.normalnet(c["image"], c["prior_F"], c["prior_B"], c["sd"], *c["cfg"], dtype=torch.float32)
        c["inside"] = c["image"].abs().sum(dim=1, keepdim=True) != 0
        _cache[name] = c
    return _cache[name]


def _distances(got, want, raw, inside):
    keep = (inside & (raw >= ref.NORM_FLOOR)).expand_as(want)
    worst = (got.double() - want)[keep].abs().max().item()
    rel = (torch.norm(got.double() - want) / torch.norm(want)).item()
    return worst, rel


@pytest.mark.parametrize("name", list(ref.CASES))
def test_network_against_float64(name, dev):
    c = _case(name, dev)
    inside = c["inside"]
    for side in (0, 1):
        want, raw = c["f64"][side], c["f64"][2 + side]
        short = ((raw < ref.NORM_FLOOR) & inside).sum().item()
        assert short <= 1e-3 * inside.sum().item()
        hip = _distances(c["hip"][side], want, raw, inside)
        t32 = _distances(c["f32"][side], want, raw, inside)
        print(f"normalnet {name} {'FB'[side]}: HIP worst {hip[0]:.3e} relL2 {hip[1]:.3e} | torch-f32 worst {t32[0]:.3e} relL2 {t32[1]:.3e}")
        bar_w, bar_l = BARS[name]
        assert t32[0] <= bar_w and t32[1] <= bar_l, "the torch-float32 oracle itself is off"
        assert hip[0] <= bar_w and hip[1] <= bar_l


@pytest.mark.parametrize("name", list(ref.CASES))
def test_zero_outside_and_unit_inside(name, dev):
    c = _case(name, dev)
    inside = c["inside"]
    assert inside.any() and (~inside).any()
    for side in (0, 1):
        n = c["hip"][side]
        assert n.shape == c["image"].shape and n.dtype == torch.float32 and n.is_contiguous()
        assert torch.all(n[~inside.expand_as(n)] == 0)
        assert (torch.norm(n.double(), dim=1, keepdim=True)[inside] - 1).abs().max().item() <= 1e-6


# at tiles128 the batch runs in 128 x 128 tiles and the single frames in 64 x 64 ones: the order of every sum is the same
@pytest.mark.parametrize("name", ["offtile", "tiles128"])
def test_batch_is_bit_equal_to_single_calls_and_runs_repeat(name, dev):
    c = _case(name, dev)
    net = c["net"]
    again = net(c["image"], c["prior_F"], c["prior_B"])
    assert torch.equal(again[0], c["hip"][0]) and torch.equal(again[1], c["hip"][1])
    for i in range(2):
        one = net(c["image"][i:i + 1], c["prior_F"][i:i + 1], c["prior_B"][i:i + 1])
        assert torch.equal(one[0][0], c["hip"][0][i]) and torch.equal(one[1][0], c["hip"][1][i])


def test_channels_last_view_is_bit_equal(dev):
    c = _case("offtile", dev)
    cl = [t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for t in (c["image"], c["prior_F"], c["prior_B"])]
    assert not cl[0].is_contiguous()
    got = c["net"](*cl)
    assert torch.equal(got[0], c["hip"][0]) and torch.equal(got[1], c["hip"][1])


def test_zero_prior_and_empty_batch(dev):
    c = _case("bottom2x2", dev)
    z = torch.zeros_like(c["prior_F"])
    got = c["net"](c["image"], z, z)
    sd64 = {k: v.double() for k, v in c["sd"].items()}
    want = ref.normalnet(c["image"], z, z, sd64, *c["cfg"], dtype=torch.float64)
    for side in (0, 1):
        d = _distances(got[side], want[side], want[2 + side], c["inside"])
        print(f"normalnet bottom2x2, zero prior, {'FB'[side]}: HIP worst {d[0]:.3e} relL2 {d[1]:.3e}")
        assert d[0] <= BARS["bottom2x2"][0] and d[1] <= BARS["bottom2x2"][1]
    e = c["image"][:0]
    nF, nB = c["net"](e, e, e)
    assert nF.shape == nB.shape == (0, 3, 32, 32) and nF.dtype == torch.float32 and nF.is_cuda


def test_packed_weights_are_kept_repacked_and_refused(dev):
    """hip_lib.PackedWeights, which the four nets share, on the smallest net: the packed buffers are kept from call to call, a weight
    written in place is packed again and changes the output, and weights left on another device raise the module's own error."""
    sd = ref.random_state_dict(8, 1, 0, seed=31, device=dev)
    net = normals.NormalNet(sd, 8, 1, 0).to(dev)
    image, pF, pB = (t.to(dev) for t in ref.make_inputs(1, 16, 16, 131))
    first = net(image, pF, pB)
    assert first[0].abs().sum().item() > 0 and first[1].abs().sum().item() > 0
    packed = net._packed(dev)
    again = net._packed(dev)
    assert again[0] is packed[0] and again[1] is packed[1]
    kept = net(image, pF, pB)
    assert torch.equal(kept[0], first[0]) and torch.equal(kept[1], first[1])
    net.netF_w0[0].neg_()                                       # one output channel of the front net's first convolution
    fresh = net._packed(dev)
    assert fresh[0] is not packed[0] and fresh[1] is not packed[1]
    after = net(image, pF, pB)
    assert not torch.equal(after[0], first[0]) and torch.equal(after[1], first[1])
    net.cpu()
    with pytest.raises(RuntimeError, match=r"NormalNet: weights are not on cuda:\d+: move the module with \.to"):
        net(image, pF, pB)


@pytest.fixture(scope="module")
def frames(dev):
    images, masks, Ks = (t.to(dev) for t in ref.make_frames())
    want = ref.crop(images, masks, Ks, S=512, dtype=torch.float64)
    return images, masks, Ks, want


def test_crop_against_the_restatement(frames):
    images, masks, Ks, (w_img, w_msk, w_K, w_box) = frames
    H, W = masks.shape[1:]
    assert (w_box[0, 0] >= 0) and (w_box[0, 3] <= H) and (w_box[1, 1] < 0) and (w_box[1, 2] > W)      # inside; leaving on two sides
    assert ((masks[2] > 0) & (masks[2] < 255)).any()                                                  # soft
    image, mask, nK, boxes = normals.crop_frames(images, masks, Ks)
    assert image.shape == (3, 3, 512, 512) and mask.shape == (3, 1, 512, 512) and nK.shape == (3, 3, 3) and boxes.shape == (3, 4)
    assert image.dtype == mask.dtype == nK.dtype == boxes.dtype == torch.float32
    assert ((boxes.double() - w_box).abs() <= 1e-6 * w_box.abs()).all()
    assert ((nK.double() - w_K).abs() <= 1e-6 * w_K.abs()).all()
    print(f"crop: image {(image.double() - w_img).abs().max().item():.3e} mask {(mask.double() - w_msk).abs().max().item():.3e}")
    assert (image.double() - w_img).abs().max().item() <= 1e-6
    assert (mask.double() - w_msk).abs().max().item() <= 1e-6
    # an RGBA array serves as both, without a copy
    rgba = torch.cat([images, masks[..., None]], dim=-1)
    again = normals.crop_frames(rgba, None, Ks)
    assert all(torch.equal(a, b) for a, b in zip(again, (image, mask, nK, boxes)))


def test_empty_mask_raises(frames):
    images, masks, Ks, _ = frames
    m = masks.clone()
    m[1] = 0
    with pytest.raises(ValueError, match="frame 1 has an empty mask"):
        normals.crop_frames(images, m, Ks)


def test_bytes(dev):
    c = _case("bottom2x2", dev)
    g = torch.Generator().manual_seed(4)
    mask = torch.rand((1, 1, 32, 32), generator=g).to(dev)
    mask[0, 0, :4] = 0
    mask[0, 0, 4:8] = 1
    nF, nB = c["hip"][0], c["hip"][1]
    bF, bB, bM = normals.normal_bytes(nF, nB, mask)
    assert bF.shape == bB.shape == (1, 32, 32, 3) and bM.shape == (1, 32, 32) and bF.dtype == bM.dtype == torch.uint8
    for got, n in ((bF, nF), (bB, nB)):
        want, want_m = ref.to_bytes(n, mask)
        assert torch.equal(got, want) and torch.equal(bM, want_m)
    for got, side in ((bF, 0), (bB, 1)):
        o64, _ = ref.to_bytes(c["f64"][side], mask.double())
        assert (got.int() - o64.int()).abs().max().item() <= 1


def test_estimate_normals_in_ragged_chunks(frames, dev):
    images, masks, Ks, _ = frames
    images = torch.cat([images, images[:2].flip(2)]).contiguous()
    masks = torch.cat([masks, masks[:2].flip(2)]).contiguous()
    Ks = torch.cat([Ks, Ks[:2]])
    sd = ref.random_state_dict(8, 4, 1, seed=21, device=dev)
    net = normals.NormalNet(sd, 8, 4, 1).to(dev)
    g = torch.Generator().manual_seed(6)
    low = torch.rand((2, 5, 3, 4, 4), generator=g) * 2 - 1
    pF, pB = (torch.nn.functional.interpolate(t, size=(512, 512), mode="bilinear").to(dev) for t in low)
    res = normals.estimate_normals(net, images, masks, Ks, pF, pB, batch=2)
    assert res["normal_F"].shape == res["normal_B"].shape == (5, 512, 512, 3) and res["normal_mask"].shape == (5, 512, 512)
    assert res["normal_F"].dtype == res["normal_B"].dtype == res["normal_mask"].dtype == torch.uint8
    assert res["normal_Ks"].shape == (5, 3, 3) and res["normal_Ks"].dtype == torch.float32
    for i in range(5):
        image, mask, nK, _ = normals.crop_frames(images[i:i + 1], masks[i:i + 1], Ks[i:i + 1])
        nF, nB = net(image, pF[i:i + 1], pB[i:i + 1])
        bF, bB, bM = normals.normal_bytes(nF, nB, mask)
        assert torch.equal(res["normal_F"][i], bF[0]) and torch.equal(res["normal_B"][i], bB[0])
        assert torch.equal(res["normal_mask"][i], bM[0]) and torch.equal(res["normal_Ks"][i], nK[0])
    assert res["normal_mask"].max().item() == 255 and res["normal_F"].float().std().item() > 1
    from soar_amd.data import FrameStore
    smpl = dict(betas=torch.zeros(10), body_pose=torch.zeros(5, 63), global_orient=torch.zeros(5, 3), transl=torch.zeros(5, 3))
    store = FrameStore.from_arrays(images, masks, res["normal_F"], res["normal_B"], res["normal_mask"], Ks, res["normal_Ks"], torch.eye(4),
                                   smpl, device=dev)
    assert store.n_frames == 5 and torch.equal(store.normal_F, res["normal_F"]) and torch.equal(store.normal_Ks, res["normal_Ks"])
