"""Float64 functional restatement of LPIPS-VGG (lpips 0.1, net='vgg', eval mode, spatial=False), written from the definition in
DESIGN.md 9e with F.conv2d / F.relu / F.max_pool2d and the head -- the oracle of tests/test_lpips_*.py.  Where a tap's features
are all zero at a pixel the norm's gradient is taken as 0 (torch's sqrt would give inf there, and inf * 0 = NaN before the ReLU
mask drops it): the input gradient is then a finite 0, as the kernels give it."""
import torch
import torch.nn.functional as F

CONV_CH = [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512),
           (512, 512), (512, 512), (512, 512), (512, 512), (512, 512)]
FEATURE_INDEX = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
TAP_LAYERS = (1, 3, 6, 9, 12)          # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
POOL_AFTER = (1, 3, 6, 9)
TAP_CH = [64, 128, 256, 512, 512]
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10


def random_weights(seed=0, dead_layer=None):
    """Seeded VGG-shaped weights (He-scaled, so that activations neither vanish nor blow up over 13 layers) and non-negative lin
    weights -> dict with 'conv_w' [13], 'conv_b' [13], 'lin' [5], 'shift', 'scale' (float32, CPU).  dead_layer: that layer's biases
    are -1e3, so its ReLU output is zero everywhere."""
    g = torch.Generator().manual_seed(seed)
    w = {"conv_w": [], "conv_b": [], "lin": []}
    for i, (cin, cout) in enumerate(CONV_CH):
        w["conv_w"].append(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
        b = torch.randn(cout, generator=g) * 0.05
        w["conv_b"].append(torch.full_like(b, -1e3) if i == dead_layer else b)
    for c in TAP_CH:
        w["lin"].append(torch.rand(c, generator=g) * 0.1)
    w["shift"], w["scale"] = torch.tensor(SHIFT), torch.tensor(SCALE)
    return w


def lpips_state_dict(w):
    """w in the key layout of lpips.LPIPS(net='vgg').state_dict() (with the lins.* duplicates)"""
    sd = {}
    for i, fi in enumerate(FEATURE_INDEX):
        s = 1 if fi < 4 else 2 if fi < 9 else 3 if fi < 16 else 4 if fi < 23 else 5
        sd[f"net.slice{s}.{fi}.weight"] = w["conv_w"][i].clone()
        sd[f"net.slice{s}.{fi}.bias"] = w["conv_b"][i].clone()
    for k, lw in enumerate(w["lin"]):
        sd[f"lin{k}.model.1.weight"] = lw.reshape(1, -1, 1, 1).clone()
        sd[f"lins.{k}.model.1.weight"] = lw.reshape(1, -1, 1, 1).clone()
    sd["scaling_layer.shift"] = w["shift"].reshape(1, 3, 1, 1).clone()
    sd["scaling_layer.scale"] = w["scale"].reshape(1, 3, 1, 1).clone()
    return sd


def torchvision_state_dict(w):
    """w as torchvision's vgg16().state_dict() (a classifier included) merged with lpips' v0.1 lin weights"""
    g = torch.Generator().manual_seed(99)
    sd = {}
    for i, fi in enumerate(FEATURE_INDEX):
        sd[f"features.{fi}.weight"] = w["conv_w"][i].clone()
        sd[f"features.{fi}.bias"] = w["conv_b"][i].clone()
    sd["classifier.0.weight"] = torch.randn(8, 16, generator=g)
    sd["classifier.0.bias"] = torch.randn(8, generator=g)
    for k, lw in enumerate(w["lin"]):
        sd[f"lin{k}.model.1.weight"] = lw.reshape(1, -1, 1, 1).clone()
    return sd


def weights_of(module, dtype=torch.float64, device=None):
    """the weights of a soar_amd.lpips.LPIPSVGG as the dict random_weights returns, in dtype on device"""
    cast = lambda t: t.detach().to(device=device or t.device, dtype=dtype)          # noqa: E731
    return {"conv_w": [cast(getattr(module, f"conv{i}_weight")) for i in range(13)],
            "conv_b": [cast(getattr(module, f"conv{i}_bias")) for i in range(13)],
            "lin": [cast(getattr(module, f"lin{k}")) for k in range(5)],
            "shift": cast(module.shift), "scale": cast(module.scale)}


def cast_weights(w, dtype, device=None):
    f = lambda t: t.to(device=device or t.device, dtype=dtype)                     # noqa: E731
    return {"conv_w": [f(t) for t in w["conv_w"]], "conv_b": [f(t) for t in w["conv_b"]], "lin": [f(t) for t in w["lin"]],
            "shift": f(w["shift"]), "scale": f(w["scale"])}


def pool_f32_ties(x):
    """2 x 2 max pool (floor) whose window winner is chosen as torch's max_pool2d chooses it, on x rounded to float32: in a
    constant image region every window holds equal values, which a float64 convolution may not compute bit-equal from position to
    position (its summation order differs between output tiles) -- the last bit would decide where the whole gradient goes.  The
    value and gradient are those of the float64 element chosen."""
    _, idx = F.max_pool2d(x.detach().float(), 2, 2, return_indices=True)
    N, C = x.shape[:2]
    return x.flatten(2).gather(2, idx.flatten(2)).view(N, C, *idx.shape[2:])


def features(x, w, f32_ties=False):
    """the five taps of x [N, 3, H, W]; f32_ties: pool windows decided at float32 resolution (pool_f32_ties)"""
    x = (x - w["shift"].view(1, 3, 1, 1)) / w["scale"].view(1, 3, 1, 1)       # torch pads x', not x
    taps = []
    for i in range(13):
        x = F.relu(F.conv2d(x, w["conv_w"][i], w["conv_b"][i], padding=1))
        if i in TAP_LAYERS:
            taps.append(x)
        if i in POOL_AFTER:
            x = pool_f32_ties(x) if f32_ties else F.max_pool2d(x, 2, 2)
    return taps


def normalize(f):
    """f / (sqrt(sum_c f_c^2) + eps), with a finite gradient where the sum is 0"""
    ss = (f * f).sum(1, keepdim=True)
    pos = ss > 0
    n = torch.where(pos, ss.clamp_min(torch.finfo(ss.dtype).tiny).sqrt(), torch.zeros_like(ss))
    return f / (n + EPS)


def lpips(in0, in1, w, taps=range(5), f32_ties=False):
    """-> [N, 1, 1, 1]: sum over the taps of the spatial mean of sum_c lin_k[c] (u0_c - u1_c)^2"""
    t0, t1 = features(in0, w, f32_ties), features(in1, w, f32_ties)
    val = 0
    for k in taps:
        d = normalize(t0[k]) - normalize(t1[k])
        s = (d * d * w["lin"][k].view(1, -1, 1, 1)).sum(1, keepdim=True)
        val = val + s.mean(dim=(2, 3), keepdim=True)
    return val


def normal_images(N, H, W, seed):
    """(normal * mask - 0.5) * 2-style inputs: a smooth random normal map inside an ellipse, a constant -1 outside, so that large
    areas are constant and many ReLUs are dead"""
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(N, 3, max(2, H // 16), max(2, W // 16), generator=g)
    n = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=False)
    n = n / n.norm(dim=1, keepdim=True).clamp_min(1e-6)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    cy, cx = (torch.rand(2, generator=g) - 0.5) * 0.3
    mask = (((yy - cy) / 0.8) ** 2 + ((xx - cx) / 0.6) ** 2 < 1).to(torch.float32)
    return ((n * 0.5 + 0.5) * mask - 0.5) * 2
