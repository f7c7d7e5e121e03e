"""GPU tests of soar_amd/pose.py (csrc/pose.hip, the shared convolution's PReLU) against tests/pose_ref.py.

* The shared GEMM with ``slope``: the exact-integer scheme of tests/test_conv_gemm_gpu.py (x, w, res integers in -2 .. 2, bias and slopes
  multiples of 0.25: every value is a multiple of 1/16 far below 2^24, so the comparison has no tolerance), at the three operand types
  and both tile sizes.
* The network: every stage output within FACTOR = 4 times the float32 restatement's own distance from the float64 one (the bar and the
  print format of tests/test_sam_gpu.py), batches against single calls bit for bit.
* The post-processing: bit for bit against the NumPy float32 restatement.
* The workspace: between guard bands, over zeros, 0xFF and noise."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_gemm_ref as cref
import pose_ref as R
import workspace_guard as W
from soar_amd import hip_lib, pose

pytestmark = pytest.mark.gpu
FACTOR = 4.0
CANARY = cref.CANARY
_cache = {}


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(dev, *shape, seed):
    return torch.randint(-2, 3, shape, generator=_gen(seed)).float().to(dev)


def _quarters(dev, n, seed):
    return (torch.randint(-8, 9, (n,), generator=_gen(seed)).float() * 0.25).to(dev)


def _bits(t):
    return t.view(torch.int32)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- the shared GEMM with slope ----
SLOPE_CASES = {64: dict(N=3, H=5, W=10, Cin=8, Cout=65), 128: dict(N=2, H=91, W=90, Cin=24, Cout=136)}
WTYPES = {"f32": (0, torch.float32), "bf16": (1, torch.bfloat16), "f16": (2, torch.float16)}


@pytest.mark.parametrize("prec", list(WTYPES))
@pytest.mark.parametrize("tile", [64, 128])
def test_conv_gemm_slope_is_exact(tile, prec, dev):
    """3 x 3, zero padding, bias, res and alpha = 0.5; Cout off the tile (65: a column tile of one; 136: one of 8); the output is a slice
    of rows 5 floats wider (ldy > Cout) that sit in a canary, the input in NaN"""
    N, H, Wd, Cin, Cout = SLOPE_CASES[tile].values()
    d = cref.conv3x3(N, H, Wd, Cin, Cout)
    d.alpha = 0.5
    w = _ints(dev, Cout, 9, Cin, seed=701)
    b = cref.guarded(d, _ints(dev, N, H, Wd, Cin, seed=700), [w], bias=_quarters(dev, Cout, 702), res=_ints(dev, N, H, Wd, Cout, seed=703))
    slope = _quarters(dev, Cout, 704)
    assert b.d.ldy == Cout + 5 and bool((slope < 0).any()) and bool((slope > 0).any())
    pre, written = cref.run(b.d, b.x.double(), b.w.double(), b.bias[:Cout].double(), None, b.y.double())
    assert bool((pre[written] < 0).any()) and bool((pre[written] > 0).any())
    chan = (torch.arange(pre.numel(), device=dev) - b.d.y_off) % b.d.ldy
    want = pre.clone()
    s = slope.double()[chan[written]]
    want[written] = torch.where(pre[written] > 0, pre[written], s * pre[written]) + b.res.double()[written]
    wtype, dt = WTYPES[prec]
    a = cref.c_args(b.d, b.x.data_ptr(), b.w.data_ptr(), b.bias.data_ptr(), b.res.data_ptr(), b.y.data_ptr())
    if wtype:
        w16 = w.to(dt).contiguous()
        assert torch.equal(w16.float(), w)
        a.ph[0].w, a.ph[0].ldw = w16.data_ptr(), 9 * Cin
    for per_image in ((0, 1) if tile == 64 else (0,)):
        y = torch.full_like(b.y, CANARY)
        a.y, a.per_image = y.data_ptr() + 4 * b.d.y_off, per_image
        got_tile = C.c_int32(0)
        hip_lib.check(hip_lib.lib().soar_selftest_conv_gemm_slope(C.byref(a), wtype, 0, slope.data_ptr(), C.byref(got_tile),
                                                                  torch.cuda.current_stream().cuda_stream), "selftest_conv_gemm_slope")
        assert got_tile.value == tile
        assert torch.equal(_bits(y[~written]), _bits(b.y[~written])), "the canary round the output slice died"
        assert torch.equal(y.double(), want), f"{(y.double() != want).sum().item()} elements differ"
    # slope = NULL is the plain epilogue
    y = torch.full_like(b.y, CANARY)
    a.y, a.per_image = y.data_ptr() + 4 * b.d.y_off, 0
    hip_lib.check(hip_lib.lib().soar_selftest_conv_gemm_slope(C.byref(a), wtype, 0, None, C.byref(got_tile), torch.cuda.current_stream().cuda_stream),
                  "selftest_conv_gemm_slope")
    plain = pre.clone()
    plain[written] = pre[written] + b.res.double()[written]
    assert torch.equal(y.double(), plain)


# ---- the network ----
CFGS = {"2+2": R.TINY, "1+1": R.TINY_1}
SIZES = {"4x6": (32, 48), "6x10": (48, 80)}


def rel(a, b):
    """worst element of a - b over b's RMS (b: float64)"""
    return float((a.double().cpu() - b).abs().max() / b.pow(2).mean().sqrt())


def within(name, got, ref64, ref32):
    e32 = rel(ref32, ref64)
    err = rel(got, ref64)
    print(f"{name}: err {err:.3g}  e32 {e32:.3g}  ratio {err / e32 if e32 else float('inf'):.2f}")
    assert err <= FACTOR * e32, f"{name}: {err:.3g} from float64, float32 restatement {e32:.3g}: ratio {err / e32:.2f} > {FACTOR}"


def _net_case(cname, sname, dev):
    """the net, a batch of three and the restatement's stages in float64 and float32 (NHWC), computed once"""
    if (cname, sname) not in _cache:
        cfg, (H, Wd) = CFGS[cname], SIZES[sname]
        sd = R.make_state_dict(cfg, seed=11)
        x = torch.randn(3, 3, H, Wd, generator=_gen(12)) * 0.4
        nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
        refs = {}
        for dt in (torch.float64, torch.float32):
            f, st = R.RefNet({k: v.to(dt) for k, v in sd.items()})(x.to(dt))
            refs[dt] = (nhwc(f), [nhwc(s) for s in st])
        net = pose.PoseNet(sd).to(dev)
        xd = x.to(dev)
        _cache[cname, sname] = dict(cfg=cfg, sd=sd, x=xd, net=net, r64=refs[torch.float64], r32=refs[torch.float32],
                                    hip=net(xd, return_stages=True))
    return _cache[cname, sname]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("sname", list(SIZES))
@pytest.mark.parametrize("cname", list(CFGS))
def test_network_against_float64(cname, sname, B, dev):
    c = _net_case(cname, sname, dev)
    cfg = c["cfg"]
    heat, paf, features, stages = c["hip"] if B == 3 else c["net"](c["x"][:1], return_stages=True)
    h, w = SIZES[sname][0] // 8, SIZES[sname][1] // 8
    assert (h, w) in ((4, 6), (6, 10)) and features.shape == (B, h, w, cfg["feat"]) and len(stages) == cfg["n_paf"] + cfg["n_heat"]
    assert heat.shape == (B, h, w, 26) and paf.shape == (B, h, w, 52) and heat.is_contiguous() and paf.is_contiguous()
    f64, s64 = c["r64"]
    f32, s32 = c["r32"]
    tag = f"pose {cname} {sname} B={B}"
    within(f"{tag} features", features, f64[:B], f32[:B])
    for s, got in enumerate(stages):
        branch = f"L2 stage {s}" if s < cfg["n_paf"] else f"L1 stage {s - cfg['n_paf']}"
        within(f"{tag} {branch}", got, s64[s][:B], s32[s][:B])
    assert torch.equal(heat, stages[-1]) and torch.equal(paf, stages[cfg["n_paf"] - 1])
    out = torch.cat([heat, paf], dim=-1)                                   # (last heat maps 26, last PAF 52)
    within(f"{tag} output 78", out, torch.cat([s64[-1], s64[cfg["n_paf"] - 1]], -1)[:B], torch.cat([s32[-1], s32[cfg["n_paf"] - 1]], -1)[:B])
    assert bool(torch.isfinite(out).all())


@pytest.mark.parametrize("cname,sname", [("2+2", "4x6"), ("1+1", "6x10")])
def test_a_frame_in_a_batch_is_bit_equal_to_the_single_call(cname, sname, dev):
    c = _net_case(cname, sname, dev)
    again = c["net"](c["x"], return_stages=True)
    for i in range(3):
        one = c["net"](c["x"][i:i + 1], return_stages=True)
        for got, batch, rep in zip((one[0], one[1], one[2], *one[3]), (c["hip"][0], c["hip"][1], c["hip"][2], *c["hip"][3]),
                                   (again[0], again[1], again[2], *again[3])):
            assert torch.equal(_bits(got[0]), _bits(batch[i])) and torch.equal(_bits(rep), _bits(batch))
    plain = c["net"](c["x"])
    assert torch.equal(plain[0], c["hip"][0]) and torch.equal(plain[1], c["hip"][1])


def test_strided_input_is_bit_equal_and_the_empty_batch(dev):
    c = _net_case("2+2", "4x6", dev)
    cl = c["x"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not cl.is_contiguous()
    got = c["net"](cl)
    assert torch.equal(_bits(got[0]), _bits(c["hip"][0])) and torch.equal(_bits(got[1]), _bits(c["hip"][1]))
    wide = torch.zeros(3, 3, 40, 60, device=dev)
    wide[:, :, 3:35, 5:53] = c["x"]
    got = c["net"](wide[:, :, 3:35, 5:53])
    assert torch.equal(_bits(got[0]), _bits(c["hip"][0])) and torch.equal(_bits(got[1]), _bits(c["hip"][1]))
    heat, paf = c["net"](c["x"][:0])
    assert heat.shape == (0, 4, 6, 26) and paf.shape == (0, 4, 6, 52) and heat.is_cuda
    with pytest.raises(ValueError, match="multiples of 16"):
        c["net"](torch.zeros(1, 3, 32, 40, device=dev))


def test_packed_weights_are_kept_repacked_and_refused(dev):
    sd = R.make_state_dict(R.TINY_1, seed=31)
    net = pose.PoseNet(sd).to(dev)
    x = (torch.randn(1, 3, 16, 16, generator=_gen(32)) * 0.4).to(dev)
    first = net(x)
    assert first[0].abs().sum().item() > 0 and first[1].abs().sum().item() > 0
    packed = net._packed(dev)
    assert net._packed(dev) is packed
    kept = net(x)
    assert torch.equal(kept[0], first[0]) and torch.equal(kept[1], first[1])
    net.t0[0].neg_()                                                       # one output channel of conv1_1
    fresh = net._packed(dev)
    assert fresh is not packed
    after = net(x)
    assert not torch.equal(after[0], first[0]) and not torch.equal(after[1], first[1])
    net.cpu()
    with pytest.raises(RuntimeError, match=r"PoseNet: weights are not on cuda:\d+: move the module with \.to"):
        net(x)


def test_preprocess(dev):
    """BGR, Pillow's bilinear resize on bytes (jpeg.resize_images, tested against Pillow by itself), v / 256 - 0.5"""
    from soar_amd.jpeg import resize_images
    img = torch.randint(0, 256, (2, 45, 80, 3), generator=_gen(40), dtype=torch.uint8).to(dev)
    x = pose.PoseNet.preprocess(img, 32)
    assert x.shape == (2, 3, 32, 64) and x.dtype == torch.float32 and not x.is_contiguous()
    small = resize_images(img, 32, 64, filter="bilinear")
    want = small.flip(-1).permute(0, 3, 1, 2).float() / 256 - 0.5
    assert torch.equal(x, want)
    with pytest.raises(ValueError, match="multiple of 16"):
        pose.PoseNet.preprocess(img, 40)


# ---- pose_peaks ----
def _blob(h, w, x0, y0, s=1.1):
    gy, gx = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.exp(-((gx - x0) ** 2 + (gy - y0) ** 2) / (2 * s * s)).astype(np.float32)


def _ring_map(h, w):
    """rises away from the top edge, with a bump in the middle of the top row: the upsampled map has a strict local maximum in row 0"""
    m = np.tile((0.2 + 0.1 * np.arange(h, dtype=np.float32))[:, None], (1, w))
    m[0, w // 2] += 0.05
    m[0, w // 2 + 1] += 0.02
    return m


def _peaks_cases():
    if "peaks" in _cache:
        return _cache["peaks"]
    cases = {}
    for h, w in ((4, 6), (6, 10)):
        # two people of three parts at sub-pixel places, the same parts 2.5 cells apart
        a = {0: (8 * w * 0.30 + 0.4, 8 * h * 0.35 + 0.6), 1: (8 * w * 0.25 + 0.3, 8 * h * 0.55 + 0.4), 8: (8 * w * 0.30 + 0.7, 8 * h * 0.75 + 0.3)}
        b = {p: (x + 8 * w * 0.45, y - 2.0) for p, (x, y) in a.items()}
        heat, _, _ = R.scene(h, w, [a, b], sigma=0.6, margin=3.0)
        cases[f"scene {h}x{w}"] = (heat[None], 32, {p: 2 for p in (0, 1)})
        z = np.zeros((1, h, w, 26), np.float32)
        # a blob centred beyond an edge peaks one pixel inside it: the four borders on four parts, a corner (a clipped window) on a fifth
        m = z.copy()
        m[0, :, :, 0], m[0, :, :, 1] = _blob(h, w, w / 2 - 0.2, -0.8), _blob(h, w, w / 2 + 0.3, h - 0.3)
        m[0, :, :, 2], m[0, :, :, 3] = _blob(h, w, -0.7, h / 2 - 0.4), _blob(h, w, w - 0.4, h / 2 + 0.2)
        m[0, :, :, 4] = _blob(h, w, -0.6, -0.6)
        m[0, :, :, 5] = _ring_map(h, w)
        cases[f"borders {h}x{w}"] = (m, 32, {0: 1, 1: 1, 2: 1, 3: 1, 4: 1})
    h, w = 6, 10
    z = np.zeros((1, h, w, 26), np.float32)
    m = z.copy()
    m[0, :, :, 0] = 0.5                                                     # a constant map
    m[0, :, :, 1] = R.scene(h, w, [{1: (40.0, 24.0)}])[0][:, :, 1]          # a blob exactly between four pixels
    cases["plateaus"] = (m, 32, {0: 0, 1: 0})
    m = z.copy()
    m[0, :, :, 3] = 0.04 * _blob(h, w, 4.3, 2.6)
    cases["below threshold"] = (m, 32, {p: 0 for p in range(25)})
    m = z.copy()
    m[0, :, :, 2] = sum(_blob(h, w, x, y, 0.45) for x, y in ((1.2, 1.1), (4.4, 0.9), (7.9, 1.3), (1.4, 4.2), (4.9, 3.8), (8.1, 4.4)))
    m[0, :, :, 7] = np.random.default_rng(3).random((h, w), dtype=np.float32)
    cases["over capacity"] = (m, 4, {2: 6})
    # three frames with different maps, the background all NaN
    rng = np.random.default_rng(4)
    m = np.stack([cases["scene 6x10"][0][0], (rng.random((h, w, 26), dtype=np.float32) - 0.3), cases["borders 6x10"][0][0]])
    m[:, :, :, 25] = np.nan
    cases["batch of three"] = (m, 32, {})
    _cache["peaks"] = cases
    return cases


PEAK_CASES = ["scene 4x6", "scene 6x10", "borders 4x6", "borders 6x10", "plateaus", "below threshold", "over capacity", "batch of three"]


@pytest.mark.parametrize("name", PEAK_CASES)
def test_pose_peaks_bit_for_bit(name, dev):
    heat, max_peaks, expect = _peaks_cases()[name]
    B, h, w, _ = heat.shape
    want_p, want_c = R.peaks_ref_batch(heat, 0.05, max_peaks, fill=CANARY)
    for p, n in expect.items():
        assert want_c[0, p] == n, (name, p, want_c[0])
    # the canary lies under every row and behind the last one
    flat = torch.full((B * 26 * max_peaks * 3 + 64,), CANARY, device=dev)
    peaks = flat[:B * 26 * max_peaks * 3].view(B, 26, max_peaks, 3)
    counts = torch.full((B, 26), -7, dtype=torch.int32, device=dev)
    pose.pose_peaks(torch.from_numpy(heat).to(dev), 0.05, max_peaks, out=(peaks, counts))
    got_c, got_p = counts.cpu().numpy(), peaks.cpu().numpy()
    assert np.array_equal(got_c, want_c), (got_c, want_c)
    assert _same_bits(got_p, want_p), np.argwhere(got_p.view(np.int32) != want_p.view(np.int32))[:5]
    assert bool((flat[B * 26 * max_peaks * 3:] == CANARY).all())
    assert (got_c[:, 25] == 0).all()
    fresh_p, fresh_c = pose.pose_peaks(torch.from_numpy(heat).to(dev), 0.05, max_peaks)
    zero_p, _ = R.peaks_ref_batch(heat, 0.05, max_peaks, fill=0.0)
    assert _same_bits(fresh_p.cpu().numpy(), zero_p) and np.array_equal(fresh_c.cpu().numpy(), want_c)
    if name.startswith("borders"):
        HH, WW = 8 * h, 8 * w
        px = [R.peak_pixels(R.upsample8(heat[0, :, :, p]))[0] for p in range(5)]          # (Y, X) of each map's only peak
        assert px[0][0] == 1 and px[1][0] == HH - 2 and px[2][1] == 1 and px[3][1] == WW - 2 and tuple(px[4]) == (1, 1)
        U = R.upsample8(heat[0, :, :, 5])
        X = int(np.argmax(U[0]))
        assert 0 < X < WW - 1 and U[0, X] > 0.05 and U[0, X] > max(U[0, X - 1], U[0, X + 1], U[1, X - 1:X + 2].max())
        assert not any(Y == 0 for Y, _ in R.peak_pixels(U))                                # ... which is no peak
    if name == "over capacity":
        assert want_c[0, 7] > 4 and (got_p[0, 2, :4, 2] > 0.05).all()
        big_p, big_c = R.peaks_ref(heat[0], 0.05, 32)
        assert _same_bits(got_p[0, 2], big_p[2, :4]) and _same_bits(got_p[0, 7], big_p[7, :4])     # the first four in raster order
    if name == "batch of three":
        for i in range(3):
            one_p, one_c = pose.pose_peaks(torch.from_numpy(heat[i:i + 1]).to(dev), 0.05, max_peaks)
            assert _same_bits(one_p.cpu().numpy()[0], zero_p[i]) and np.array_equal(one_c.cpu().numpy()[0], want_c[i])
        assert want_c[1].max() > 4


# ---- pose_assemble ----
def _from_scene(h, w, persons, **kw):
    heat, paf, _ = R.scene(h, w, persons, **kw)
    peaks, counts = R.peaks_ref(heat)
    return peaks[None], counts[None], paf[None]


def _empty(h, w, max_peaks=32):
    return np.zeros((1, 26, max_peaks, 3), np.float32), np.zeros((1, 26), np.int32), np.zeros((1, h, w, 52), np.float32)


def _assemble_cases():
    if "assemble" in _cache:
        return _cache["assemble"]
    cases = {}
    A = R.person(70.4, 100.6)
    close, outside = _from_scene(28, 30, [A, R.person(92.7, 118.3)]), _from_scene(28, 30, [A, R.person(222.4, 104.7)])
    cases["two scenes"] = (tuple(np.concatenate([a, b]) for a, b in zip(close, outside)), {}, [2, 2])
    # neck and hip of the second person at the same place: a candidate of length zero
    p, c, f = (t.copy() for t in close)
    p[0, 8, 1, :2] = p[0, 1, 1, :2]
    cases["zero length"] = ((p, c, f), {}, None)
    # four collinear peaks in a uniform field: every neck -> hip candidate scores exactly 1, (a, b) order decides
    p, c, f = _empty(12, 24)
    f[..., 0], f[..., 7] = 1.0, 1.0                                         # limb (1, 8) along x, limb (8, 9) along y
    p[0, 1, :2] = [(20.5, 40.5, 0.9), (60.5, 40.5, 0.8)]
    p[0, 8, :2] = [(140.5, 40.5, 0.7), (100.5, 40.5, 0.9)]
    p[0, 9, :2] = [(140.5, 80.5, 0.6), (100.5, 80.5, 0.9)]
    c[0, [1, 8, 9]] = 2
    cases["tie"] = ((p, c, f), {}, [2])
    # two toes and nothing else: a person of two parts
    cases["two parts"] = (_from_scene(12, 16, [{19: (40.4, 50.6), 20: (70.6, 52.4)}, R.person(60.4, 70.6, {1: (0, -40), 8: (0, 10), 9: (-12, 10)})]), {}, [1])
    # no neck: arms and head start as three persons and merge over the shoulder -> ear limbs
    head = {k: R.TEMPLATE[k] for k in (0, 2, 3, 5, 6, 15, 16, 17, 18)}
    cases["merge"] = (_from_scene(16, 16, [R.person(64.4, 90.6, head)]), {}, [1])
    # ten sticks of three parts, eight places
    sticks = [R.person(30.4 + 30 * i, 50.6, {1: (0, -30), 8: (0, 10), 9: (-10, 30)}) for i in range(10)]
    cases["over capacity"] = (_from_scene(12, 40, sticks), dict(max_people=8), [10])
    cases["capacity of one"] = (_from_scene(12, 40, sticks[:3]), dict(max_people=1, min_parts=2), [3])
    cases["nothing"] = (_empty(6, 10), {}, [0])
    _cache["assemble"] = cases
    return cases


ASSEMBLE_CASES = ["two scenes", "zero length", "tie", "two parts", "merge", "over capacity", "capacity of one", "nothing"]


@pytest.mark.parametrize("name", ASSEMBLE_CASES)
def test_pose_assemble_bit_for_bit(name, dev):
    (peaks, counts, paf), kw, n_want = _assemble_cases()[name]
    want_p, want_n = R.assemble_ref_batch(peaks, counts, paf, **kw)
    if n_want is not None:
        assert want_n.tolist() == n_want, want_n
    got_p, got_n = pose.pose_assemble(*(torch.from_numpy(t).to(dev) for t in (peaks, counts, paf)), **kw)
    assert got_n.dtype == torch.int32 and np.array_equal(got_n.cpu().numpy(), want_n), (got_n, want_n)
    assert _same_bits(got_p.cpu().numpy(), want_p)
    parts = (want_p[..., 2] > 0).sum(-1)
    if name == "two scenes":
        assert parts[0, :2].tolist() == [25, 25] and sorted(parts[1, :2].tolist()) == [15, 25] and not parts[:, 2:].any()
        for i in range(2):
            one_p, one_n = pose.pose_assemble(*(torch.from_numpy(t[i:i + 1]).to(dev) for t in (peaks, counts, paf)))
            assert _same_bits(one_p.cpu().numpy()[0], want_p[i]) and int(one_n[0]) == want_n[i]
    if name == "zero length":
        assert R._score(peaks[0, 1, 1], peaks[0, 8, 1], paf[0], 0, 1, np.float32(0.05), np.float32(0.95)) is None
        assert not any(np.array_equal(q[1], peaks[0, 1, 1]) and np.array_equal(q[8], peaks[0, 8, 1]) for q in want_p[0])
    if name == "tie":
        # (0, 0) first, then (1, 1), although hip 1 is the nearer one to neck 0
        assert np.array_equal(want_p[0, 0, [1, 8, 9], 0], [20.5, 140.5, 140.5]) and np.array_equal(want_p[0, 1, [1, 8, 9], 0], [60.5, 100.5, 100.5])
    if name == "two parts":
        assert parts[0, 0] == 3 and not want_p[0, 0, 19].any()
    if name == "merge":
        assert parts[0, 0] == 9 and want_p[0, 0, 1, 2] == 0
    if name == "over capacity":
        assert (parts[0] == 3).all() and want_p.shape[1] == 8
    if name == "capacity of one":
        assert parts[0].tolist() == [3] and want_p.shape[1] == 1


def test_scale_keypoints(dev):
    people = (torch.rand(2, 3, 25, 3, generator=_gen(50)) * 600).to(dev)
    got = pose.scale_keypoints(people, (1080, 1920), (368, 656))
    assert _same_bits(got.cpu().numpy(), R.scale_ref(people.cpu().numpy(), (1080, 1920), (368, 656))) and got.data_ptr() != people.data_ptr()


# ---- the stage ----
LOOSE = dict(threshold=0.0, inter_threshold=-100.0, min_above=-1.0, min_score=-1e9, min_parts=2)


@pytest.fixture(scope="module")
def frames(dev):
    net = pose.PoseNet(R.make_state_dict(R.TINY, seed=61)).to(dev)
    img = torch.randint(0, 256, (5, 45, 72, 3), generator=_gen(62), dtype=torch.uint8)
    return net, img.to(dev)


def test_detect_is_the_stages_composed(frames, dev):
    """a random net's maps mean nothing: the thresholds are opened until its peaks do assemble, so that the comparison has content"""
    net, img = frames
    people, n_people = pose.detect(net, img[:3], net_height=32, **LOOSE)
    x = net.preprocess(img[:3], 32)
    assert x.shape == (3, 3, 32, 64)
    heat, paf = net(x)
    peaks, counts = pose.pose_peaks(heat, 0.0, 32)
    kw = {k: v for k, v in LOOSE.items() if k != "threshold"}
    raw, n = pose.pose_assemble(peaks, counts, paf, **kw)
    want = pose.scale_keypoints(raw, (45, 72), (32, 64))
    assert torch.equal(_bits(people), _bits(want)) and torch.equal(n_people, n)
    assert int(n.min()) > 0 and people.shape == (3, 8, 25, 3)
    # ... and the post-processing of the device's maps is the restatement's, scaling included
    rp, rc = R.peaks_ref_batch(heat.cpu().numpy(), 0.0, 32)
    assert _same_bits(peaks.cpu().numpy(), rp) and np.array_equal(counts.cpu().numpy(), rc)
    ra, rn = R.assemble_ref_batch(rp, rc, paf.cpu().numpy(), **kw)
    assert _same_bits(people.cpu().numpy(), R.scale_ref(ra, (45, 72), (32, 64))) and np.array_equal(n.cpu().numpy(), rn)


def test_detect_sequence_in_ragged_chunks_and_its_files(frames, dev, tmp_path):
    from soar_amd import smplify
    net, img = frames
    whole = pose.detect_sequence(net, img, chunk=5, net_height=32, **LOOSE)
    ragged = pose.detect_sequence(net, img.cpu(), chunk=2, device=dev, net_height=32, **LOOSE)
    assert whole.shape == (5, 137, 3) and whole.dtype == np.float32 and _same_bits(whole, ragged)
    assert whole[:, :25, 2].any() and not whole[:, 25:].any()
    people, n_people = pose.detect(net, img, net_height=32, **LOOSE)
    assert _same_bits(whole[:, :25], people[:, 0].cpu().numpy())
    pose.save_keypoints(str(tmp_path / "kp"), people, n_people, [f"{i:05d}" for i in range(5)])
    assert _same_bits(smplify.load_keypoints(str(tmp_path / "kp")), whole)
    # ... and from picture files (PNG is lossless: the same frames), decoded on the device chunk by chunk
    from soar_amd import png
    files = [str(tmp_path / f"{i:05d}.png") for i in range(5)]
    png.write_png_files(files, img)
    assert _same_bits(pose.detect_sequence(net, files, chunk=2, device=dev, net_height=32, **LOOSE), whole)
    with pytest.raises(ValueError, match="jpg"):
        pose.detect_sequence(net, ["a.bmp"], device=dev)


# ---- the workspace contract ----
def test_workspace_contract(dev):
    """PoseNet's two allocations (the packed weights, the forward's workspace) between guard bands over every fill: the bands intact,
    the sizes exactly the sizing calls', the outputs finite and the same bits as outside any context; the post-processing takes no
    workspace"""
    sd = R.make_state_dict(R.TINY, seed=71)
    x = (torch.randn(2, 3, 32, 48, generator=_gen(72)) * 0.4).to(dev)
    img = torch.randint(0, 256, (2, 40, 75, 3), generator=_gen(73), dtype=torch.uint8).to(dev)
    assert pose.net_size(40, 75, 32) == (32, 64)

    def run():
        net = pose.PoseNet(sd).to(dev)
        heat, paf, features, stages = net(x, return_stages=True)
        people, n = pose.detect(net, img, net_height=32, **LOOSE)
        return [heat, paf, features, *stages, people, n]

    plain = run()
    L = hip_lib.lib()
    cfg = pose._c_config(R.TINY)
    nb = C.c_size_t(0)
    hip_lib.check(L.soar_pose_weights_size(C.byref(cfg), C.byref(nb), None), "soar_pose_weights_size")
    sizes = [nb.value, hip_lib._bytes(L.soar_pose_workspace_size, "soar_pose_workspace_size", C.byref(cfg), 2, 32, 48),
             hip_lib._bytes(L.soar_pose_workspace_size, "soar_pose_workspace_size", C.byref(cfg), 2, 32, 64)]
    for fill in W.FILLS:
        with W.guarded(fill) as g:
            got = run()
            g.check()
            asked = [(nbytes, who) for _, nbytes, who, _ in g.buffers]
            assert asked == [(s, "soar_amd.pose") for s in sizes], asked
            for a, b in zip(got, plain):
                assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b), fill
