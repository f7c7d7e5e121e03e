"""GPU tests of the VAE encoder's 16-bit precisions (csrc/vae.hip through soar_vae_*16, soar_amd/sds.py LatentEncoder(precision=
"bf16" / "f16")), the real ch = 128 network with vae_ref.random_weights.  Every case runs at bf16 and at f16.

The bar is DESIGN.md 9y's, measured against the restatement and never against the code under test: ``e16`` is the distance of the
float64 chain with 16-bit operands (tests/vae_half_ref.py) from the plain float64 chain (tests/vae_ref.py) on the same inputs --
what rounding the operands costs whoever does it; HIP's distance from the plain chain must be at most 4 e16 in each measure
(latents / mean / logvar: relative L2 and worst element over max |ref|; the image gradient: relative L2 and worst element over
max |g|).  HIP's distance from the 16-bit restatement itself is printed, without a bar.  At f16 every product of the restatement is
also held to tests/test_sds_half_cpu.py's caps (hardly any gradient operand below 2^-14, none above 2^12), or the yardstick itself
would be off the type's range.

Then: a peaked attention; the whole chain through MultiviewSDS; the same with the loss times 1e-4 (the weight must reach no 16-bit
product); the float32 path's bit-equalities per precision at image_size 72 and 40; the workspace contract; precision 0 through the
new entry points against the old ones."""
import ctypes as C

import pytest
import torch

import vae_half_ref as HR
import vae_ref as R
from soar_amd import hip_lib, sds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
CODES = {"f32": 0, "bf16": 1, "f16": 2}
PRECS = ["bf16", "f16"]
FACTOR = 4.0                   # DESIGN.md 9y's and 9z's: the largest ratio measured there is 2.58
SHARE_CAP, LARGEST_CAP = 1e-3, 2.0 ** 12          # test_sds_half_cpu.py's


@pytest.fixture(scope="module")
def weights():
    return R.random_weights(0)


_encoders = {}


def _encoder(weights, prec, key=0):
    """one module per (weights, precision), shared by the file"""
    if (key, prec) not in _encoders:
        _encoders[key, prec] = sds.LatentEncoder(weights, precision=prec).to(DEV)
    return _encoders[key, prec]


@pytest.fixture(scope="module")
def encs(weights):
    return {p: _encoder(weights, p) for p in ("f32", "bf16", "f16")}


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def _worst(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max())


def _inputs(N, H, W, S, seed):
    x = R.images(N, H, W, seed).to(DEV)
    g = torch.Generator().manual_seed(seed + 1)
    eps = torch.randn(N, 4, S // 8, S // 8, generator=g).to(DEV)
    gw = torch.randn(N, 4, S // 8, S // 8, generator=g).to(DEV)
    return x, eps, gw


def _hip(enc, x, S, eps, gw, grad_scale=None):
    xv = x.detach().clone().requires_grad_(True)
    lat = enc(xv, S, posterior_noise=eps, grad_scale=grad_scale)
    (lat * gw).sum().backward()
    torch.cuda.synchronize()
    return lat.detach(), xv.grad


# ---- the restatements, computed once per (weights, case, type) on the device and left unchanged ----
_oracle = {}


def _restated(weights, key, N, H, W, S, prec):
    """-> ((latents, gradient, mean, logvar) plain float64, the same with 16-bit operands, the Stats of that run)"""
    w64 = None
    for p in (None, prec):
        if (key, N, H, W, S, p) in _oracle:
            continue
        if w64 is None:
            w64 = R.cast(weights, torch.float64, DEV)
        x, eps, gw = _inputs(N, H, W, S, seed=H)
        st = HR.Stats()
        out = HR.latents_and_grad(x.double(), w64, S, eps.double(), gw.double(), DTYPES[p] if p else None, st)
        _oracle[key, N, H, W, S, p] = (out, st)
    plain, half = _oracle[key, N, H, W, S, None], _oracle[key, N, H, W, S, prec]
    return plain[0], half[0], half[1]


def _measures(got, ref):
    """(latents, gradient, mean, logvar) against the plain chain's: relative L2 and worst element over the largest, each"""
    names = ("latents", "grad", "mean", "logvar")
    out = {}
    for n, a, b in zip(names, got, ref):
        out[n + " L2"], out[n + " worst"] = _rel(a, b), _worst(a, b)
    return out


def _check(enc, weights, key, N, H, W, S, prec, layout="nchw", unread=False):
    x, eps, gw = _inputs(N, H, W, S, seed=H)
    if layout == "nhwc":
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)       # comp_rgb.permute(0, 3, 1, 2)
        assert not x.is_contiguous()
    lat, g = _hip(enc, x, S, eps, gw)
    mean, logvar = enc.encode(x, S)
    assert lat.shape == (N, 4, S // 8, S // 8) and g.shape == x.shape and g.stride() == x.stride()
    assert all(bool(torch.isfinite(t).all()) for t in (lat, g, mean, logvar))
    plain, half, st = _restated(weights, key, N, H, W, S, prec)
    assert float(plain[1].abs().max()) > 0
    e16 = _measures(half, plain)
    hip = _measures((lat, g, mean, logvar), plain)
    own = _measures((lat, g, mean, logvar), half)
    ratios = {k: hip[k] / e16[k] for k in hip}
    print(f"\n{prec} {N}x{H}x{W}->{S} {layout}")
    for k in hip:
        print(f"   {k:14s} e16 {e16[k]:.2e}  HIP {hip[k]:.2e}  ratio {ratios[k]:.2f}   HIP from the 16-bit restatement {own[k]:.2e}")
    if prec == "f16":
        print(f"   f16 restatement: worst share of gradient operands below 2^-14 {st.worst_share():.2e}, largest {st.largest():.1f}")
        assert len(st.per_product) == 29
        assert st.worst_share() <= SHARE_CAP and st.largest() <= LARGEST_CAP, st.per_product
    assert all(v > 0 for v in e16.values()), e16                 # the rounding moved every output: the yardstick is not zero
    assert all(hip[k] <= FACTOR * e16[k] for k in hip), {k: (hip[k], e16[k]) for k in hip if hip[k] > FACTOR * e16[k]}
    if unread:
        # input pixels that no resized pixel reads get an exact 0, and only they: the set is the float64 oracle's
        z64 = plain[1] == 0
        share = float(z64.double().mean())
        print(f"   grad == 0 share {share:.3f}")
        assert share > 0.5, share
        assert torch.equal(g == 0, z64), int(((g == 0) != z64).sum())


# one token in a padded tile, the stride-2 data gradient on 2 x 2 and 1 x 1; 9 tokens; partial tiles and T_pad = 128, also as a
# permuted view; the dyadic resize with unread input pixels
CASES = [(2, 8, 8, 8, "nchw"), (3, 30, 22, 24, "nchw"), (2, 50, 90, 72, "nchw"), (2, 50, 90, 72, "nhwc"), (1, 8, 200, 40, "nchw")]
UNREAD = {(1, 8, 200, 40)}


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("N,H,W,S,layout", CASES)
def test_within_four_times_the_roundings_own_error(encs, weights, N, H, W, S, layout, prec):
    _check(encs[prec], weights, 0, N, H, W, S, prec, layout, unread=(N, H, W, S) in UNREAD)


@pytest.mark.parametrize("prec", PRECS)
def test_peaked_attention(prec):
    """image_size 24 with test_sds_gpu.py's gain for it: a softmax with a dominant key per row, which 16-bit q and k move most"""
    N, H, W, S, gain = 3, 30, 22, 24, 1.5
    w = R.random_weights(0, attn_gain=gain)
    x, _, _ = _inputs(N, H, W, S, seed=H)
    with torch.no_grad():
        rowmax = float(R.attention_probs(x.double(), R.cast(w, torch.float64, DEV), S).max(dim=2).values.mean())
    print(f"\n{S}: gain {gain} mean row-max probability {rowmax:.3f}")
    assert 0.3 <= rowmax <= 0.8, rowmax
    _check(_encoder(w, prec, key=gain), w, gain, N, H, W, S, prec)


def test_the_16_bit_paths_run(encs):
    """the three precisions give three different results, close to each other"""
    S = 40
    x, eps, gw = _inputs(1, 8, 200, S, seed=3)
    out = {p: _hip(encs[p], x, S, eps, gw) for p in ("f32", "bf16", "f16")}
    for a, b in (("f32", "bf16"), ("f32", "f16"), ("bf16", "f16")):
        assert not torch.equal(out[a][0], out[b][0]) and not torch.equal(out[a][1], out[b][1])
    assert _rel(out["bf16"][0], out["f32"][0]) < 0.05 and _rel(out["f16"][0], out["f32"][0]) < 0.01


def test_the_default_is_f32(weights, encs):
    S = 40
    x, eps, gw = _inputs(2, 45, 52, S, seed=5)
    default = sds.LatentEncoder(weights).to(DEV)
    assert default.precision == "f32"
    ld, gd = _hip(default, x, S, eps, gw)
    lf, gf = _hip(encs["f32"], x, S, eps, gw)
    assert torch.equal(ld, lf) and torch.equal(gd, gf)
    for p in ("bf16", "f16"):
        assert encs[p].weights.dtype == torch.float32 and torch.equal(encs[p].weights, default.weights)


# ---- the whole chain ----
def _eps_fn(x, t):
    """test_sds_gpu.py's deterministic stand-in for the UNet: two affine maps of the noisy latents, t-dependent"""
    B = x.shape[0] // 2
    s = 1e-3 * t.to(x.dtype).view(-1, 1, 1, 1)
    return torch.cat([0.7 * x[:B] + 0.1 + s[:B], 0.4 * x[B:] - 0.05 * x[B:].flip(1) - s[B:]])


def _chain64(weights, x, eps, noise, t, S, dtype, stats=None):
    """the float64 chain through the loss tail (recon loss, std rescale 0.2), plain or with 16-bit operands in the encoder"""
    import contextlib
    w = R.cast(weights, torch.float64, DEV)
    tb = {k: v.to(DEV) for k, v in R.tables(R.ldm_alphas_cumprod()).items()}
    B = x.shape[0]
    with (HR.half(dtype, stats) if dtype is not None else contextlib.nullcontext()):
        x64 = x.double().clone().requires_grad_(True)
        lat = R.latents(x64, w, S, eps.double())
        x_in = R.q_sample(lat.detach(), t, noise.double(), tb)
        eps_pred = _eps_fn(torch.cat([x_in, x_in]), t.expand(2 * B))
        loss, gn, dlat = R.loss_tail(lat, noise.double(), eps_pred, t, tb, 5.0, 4, True, 0.2)
        (lat * dlat).sum().backward()
    return float(loss), float(gn), x64.grad.permute(0, 2, 3, 1)


def _sds_inputs(B, H, W, S, seed):
    x, eps, _ = _inputs(B, H, W, S, seed=seed)
    noise = torch.randn(B, 4, S // 8, S // 8, generator=torch.Generator().manual_seed(9)).to(DEV)
    return x, eps, noise, torch.tensor([500], device=DEV)


@pytest.mark.parametrize("prec", PRECS)
def test_whole_chain_through_multiview_sds(encs, weights, prec):
    B, S = 4, 64
    x, eps, noise, t = _sds_inputs(B, 80, 72, S, seed=5)
    m = sds.MultiviewSDS(encs[prec], guidance_scale=5.0, n_view=4, recon_loss=True, recon_std_rescale=0.2, image_size=S).to(DEV)
    xv = x.permute(0, 2, 3, 1).contiguous().requires_grad_(True)           # [B, H, W, 3]
    out = m(xv, _eps_fn, t=t, noise=noise, posterior_noise=eps)
    out["loss_sds"].backward()
    torch.cuda.synchronize()
    st = HR.Stats()
    l64, n64, g64 = _chain64(weights, x, eps, noise, t, S, None)
    l16, n16, g16 = _chain64(weights, x, eps, noise, t, S, DTYPES[prec], st)
    e16 = (abs(l16 / l64 - 1), abs(n16 / n64 - 1), _rel(g16, g64), _worst(g16, g64))
    hip = (abs(float(out["loss_sds"].detach()) / l64 - 1), abs(float(out["grad_norm"]) / n64 - 1), _rel(xv.grad, g64), _worst(xv.grad, g64))
    own = (abs(float(out["loss_sds"].detach()) / l16 - 1), abs(float(out["grad_norm"]) / n16 - 1), _rel(xv.grad, g16), _worst(xv.grad, g16))
    print(f"\n{prec} whole chain, loss {l64:.5g}: loss / grad_norm / grad L2 / grad worst")
    print("   e16   " + " ".join(f"{v:.2e}" for v in e16))
    print("   HIP   " + " ".join(f"{v:.2e}" for v in hip) + "   ratios " + " ".join(f"{h / e:.2f}" for h, e in zip(hip, e16)))
    print("   HIP from the 16-bit restatement " + " ".join(f"{v:.2e}" for v in own))
    if prec == "f16":
        print(f"   f16 restatement: worst share below 2^-14 {st.worst_share():.2e}, largest operand {st.largest():.1f}")
    assert l64 > 0 and float(g64.abs().max()) > 0 and all(v > 0 for v in e16)
    assert all(h <= FACTOR * e for h, e in zip(hip, e16)), (hip, e16)
    assert not out["grad_norm"].requires_grad


@pytest.mark.parametrize("prec", PRECS)
def test_the_loss_weight_reaches_no_16_bit_product(encs, prec):
    """The same call with the incoming gradient times 1e-4 (lambda_sds): the image gradient is 1e-4 times the unscaled one to
    float32 rounding, 2^-22 relative, element by element.  At 64 x 64 -> 64 the resize's data gradient is the identity (weights
    1 and 0), so behind the scale's place -- conv_in's data gradient -- nothing sums: the scaled gradient is one float32 multiply
    of the unscaled one, as torch's is.  A weight that entered a 16-bit operand would move the elements by the type's 2^-8 / 2^-11
    (and at f16, below 2^-14, by far more)."""
    B, S = 4, 64
    x, eps, noise, t = _sds_inputs(B, S, S, S, seed=7)
    m = sds.MultiviewSDS(encs[prec], guidance_scale=5.0, n_view=4, recon_loss=True, recon_std_rescale=0.2, image_size=S).to(DEV)
    grads = []
    for weight in (None, 1e-4):
        xv = x.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        loss = m(xv, _eps_fn, t=t, noise=noise, posterior_noise=eps)["loss_sds"]
        (loss if weight is None else loss * weight).backward()
        grads.append(xv.grad)
    torch.cuda.synchronize()
    g, gs = grads[0].double(), grads[1].double()
    want = g * float(torch.tensor(1e-4, dtype=torch.float32))
    nz = want != 0
    assert float(nz.double().mean()) > 0.9 and torch.equal(gs == 0, ~nz)
    err = ((gs - want).abs()[nz] / want.abs()[nz]).max().item()
    print(f"\n{prec}: worst relative distance of the 1e-4 gradient from 1e-4 x the unscaled one {err:.2e} (2^-22 = {2.0 ** -22:.2e})")
    assert err <= 2.0 ** -22


# ---- the float32 path's promises, per precision: image_size 72 pads the attention (T = 81, T_pad = 128), 40 has partial tiles ----
OFF_GRID = [(72, 50, 90), (40, 45, 52)]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S,H,W", OFF_GRID)
def test_two_runs_and_batch_splits_are_bit_equal(encs, S, H, W, prec):
    enc = encs[prec]
    x, eps, gw = _inputs(4, H, W, S, seed=23)
    lat, g = _hip(enc, x, S, eps, gw)
    lat2, g2 = _hip(enc, x, S, eps, gw)
    assert torch.equal(lat, lat2) and torch.equal(g, g2)
    for n in range(4):
        ln, gn = _hip(enc, x[n:n + 1], S, eps[n:n + 1], gw[n:n + 1])
        assert torch.equal(lat[n:n + 1], ln) and torch.equal(g[n:n + 1], gn), n


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S,H,W", OFF_GRID)
def test_an_image_gives_the_same_bits_first_and_last_in_a_batch(encs, S, H, W, prec):
    enc = encs[prec]
    x, eps, gw = _inputs(5, H, W, S, seed=29)
    first, last = [0, 1, 2], [3, 4, 0]
    lf, gf = _hip(enc, x[first], S, eps[first], gw[first])
    ll, gl = _hip(enc, x[last], S, eps[last], gw[last])
    assert not torch.equal(x[1], x[3]) and float(gf[0].abs().max()) > 0
    assert torch.equal(lf[0], ll[2]) and torch.equal(gf[0], gl[2])


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S,H,W", OFF_GRID)
def test_permuted_view_is_bit_equal_to_its_copy(encs, S, H, W, prec):
    enc = encs[prec]
    x, eps, gw = _inputs(2, H, W, S, seed=13)
    view = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    lv, gv = _hip(enc, view, S, eps, gw)
    lc, gc = _hip(enc, view.contiguous(), S, eps, gw)
    assert gv.stride() == view.stride() and gc.is_contiguous() and not view.is_contiguous()
    assert torch.equal(lv, lc) and torch.equal(gv, gc)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S,H,W", OFF_GRID)
def test_grad_scale_equals_a_torch_multiply(encs, S, H, W, prec):
    enc = encs[prec]
    x, eps, gw = _inputs(2, H, W, S, seed=15)
    occ = torch.rand(2, H, W, 1, generator=torch.Generator().manual_seed(3)).to(DEV)
    scale = torch.exp(-3 * occ)
    _, g = _hip(enc, x, S, eps, gw)
    _, gs = _hip(enc, x, S, eps, gw, grad_scale=scale)
    _, gs3 = _hip(enc, x, S, eps, gw, grad_scale=scale[..., 0])
    assert float(g.abs().max()) > 0
    assert torch.equal(gs, g * scale[..., 0].unsqueeze(1)) and torch.equal(gs, gs3)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("S,H,W", OFF_GRID)
def test_graph_capture_replays_equal_to_eager(encs, S, H, W, prec):
    """forward and backward captured: no host synchronisation and no allocation inside the calls; at 72 the padded attention's two
    memsets are nodes of the graph"""
    enc = encs[prec]
    x, eps, gw = _inputs(2, H, W, S, seed=31)
    xv = x.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            xv.grad = None
            (enc(xv, S, posterior_noise=eps) * gw).sum().backward()
    torch.cuda.current_stream().wait_stream(s)
    xv.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lat = enc(xv, S, posterior_noise=eps)
        (lat * gw).sum().backward()
    with torch.no_grad():
        xv.copy_(x * 0.5 + 0.25)
    graph.replay()
    torch.cuda.synchronize()
    le, ge = _hip(enc, x * 0.5 + 0.25, S, eps, gw)
    assert torch.equal(lat.detach(), le) and torch.equal(xv.grad, ge)


# ---- the C ABI ----
GUARD = 64 * 1024
GUARD_BYTE = 0xA5


def _workspace_bytes(N, H, W, S):
    nb = C.c_size_t(0)
    hip_lib.check(hip_lib.lib().soar_vae_workspace_bytes(N, H, W, S, C.byref(nb)), "soar_vae_workspace_bytes")
    return nb.value


def _abi_args(packed, scale_factor, x, S, eps, gw):
    N, _, H, W = x.shape
    h = S // 8
    lat, mean, logvar = (torch.full((N, 4, h, h), float("nan"), device=x.device) for _ in range(3))
    g = torch.full_like(x, float("nan"))
    a = hip_lib.SoarVaeArgs()
    a.N, a.H, a.W, a.image_size = N, H, W, S
    a.x = x.data_ptr()
    for i, st in enumerate(x.stride()):
        a.x_stride[i] = st
    a.weights = packed.data_ptr()
    a.scale_factor = scale_factor
    a.latents, a.eps, a.mean, a.logvar = lat.data_ptr(), eps.data_ptr(), mean.data_ptr(), logvar.data_ptr()
    a.g_latents, a.g_x = gw.data_ptr(), g.data_ptr()
    for i, st in enumerate(g.stride()):
        a.g_x_stride[i] = st
    return a, (lat, mean, logvar, g)


def _abi_forward_backward(packed, scale_factor, code, x, S, eps, gw, ws, old_entries=False):
    """soar_vae_forward16 + soar_vae_backward16 at precision code (old_entries: soar_vae_forward + soar_vae_backward) on the caller's
    workspace; the outputs start as NaN so that an element no kernel wrote is seen"""
    L = hip_lib.lib()
    a, outs = _abi_args(packed, scale_factor, x, S, eps, gw)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if old_entries:
        hip_lib.check(L.soar_vae_forward(C.byref(a), ws.data_ptr(), ws.numel(), stream), "soar_vae_forward")
        hip_lib.check(L.soar_vae_backward(C.byref(a), ws.data_ptr(), ws.numel(), stream), "soar_vae_backward")
    else:
        hip_lib.check(L.soar_vae_forward16(C.byref(a), code, ws.data_ptr(), ws.numel(), stream), "soar_vae_forward16")
        hip_lib.check(L.soar_vae_backward16(C.byref(a), code, ws.data_ptr(), ws.numel(), stream), "soar_vae_backward16")
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("prec", PRECS)
def test_workspace_contract(encs, prec):
    """image_size 72: the workspace is exactly soar_vae_workspace_bytes -- the float32 path's size -- between two guard bands.
    Whether it held zeros or 0xFF bytes (NaN as floats and as doubles) before the forward, the outputs are the same bits, the
    module's too, and the bands keep their pattern; one byte short is refused by both entries before anything is launched."""
    N, H, W, S = 2, 50, 90, 72
    enc = encs[prec]
    x, eps, gw = _inputs(N, H, W, S, seed=37)
    need = _workspace_bytes(N, H, W, S)
    packed = enc._packed(DEV)
    buf = torch.full((need + 2 * GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    ws = buf[GUARD:GUARD + need]
    assert ws.data_ptr() % 256 == 0
    results = []
    for fill in (0, 0xFF):
        ws.fill_(fill)
        out = _abi_forward_backward(packed, enc.scale_factor, CODES[prec], x, S, eps, gw, ws)
        assert all(bool(torch.isfinite(t).all()) for t in out), fill
        results.append(out)
        assert bool((buf[:GUARD] == GUARD_BYTE).all()) and bool((buf[GUARD + need:] == GUARD_BYTE).all()), fill
    assert float(results[0][3].abs().max()) > 0
    for name, a, b in zip(("latents", "mean", "logvar", "grad"), *results):
        assert torch.equal(a, b), name
    lat, g = _hip(enc, x, S, eps, gw)
    assert torch.equal(lat, results[0][0]) and torch.equal(g, results[0][3])
    a, outs = _abi_args(packed, enc.scale_factor, x, S, eps, gw)
    L = hip_lib.lib()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for entry in (L.soar_vae_forward16, L.soar_vae_backward16):
        assert entry(C.byref(a), CODES[prec], ws.data_ptr(), need - 1, stream) != 0
        assert f"workspace of {need - 1} bytes, need {need} (soar_vae_workspace_bytes)" in hip_lib.last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs)         # nothing was launched


def test_precision_0_through_the_new_entries_is_the_old_entries_bits(encs):
    enc = encs["f32"]
    L = hip_lib.lib()
    N, H, W, S = 2, 50, 90, 72
    x, eps, gw = _inputs(N, H, W, S, seed=41)
    nb, nb_old = C.c_size_t(0), C.c_size_t(0)
    hip_lib.check(L.soar_vae_weights_bytes16(0, C.byref(nb)), "soar_vae_weights_bytes16")
    hip_lib.check(L.soar_vae_weights_bytes(C.byref(nb_old)), "soar_vae_weights_bytes")
    assert nb.value == nb_old.value == enc._packed(DEV).numel()
    new = torch.full((nb.value,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    ref = torch.full((nb.value,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    w = enc.weights
    hip_lib.check(L.soar_vae_pack_weights16(w.data_ptr(), w.numel(), new.data_ptr(), new.numel(), 0, stream), "soar_vae_pack_weights16")
    hip_lib.check(L.soar_vae_pack_weights(w.data_ptr(), w.numel(), ref.data_ptr(), ref.numel(), stream), "soar_vae_pack_weights")
    torch.cuda.synchronize()
    assert torch.equal(new, ref)
    ws = torch.empty(_workspace_bytes(N, H, W, S), dtype=torch.uint8, device=DEV)
    a = _abi_forward_backward(new, enc.scale_factor, 0, x, S, eps, gw, ws)
    b = _abi_forward_backward(ref, enc.scale_factor, 0, x, S, eps, gw, ws, old_entries=True)
    for name, u, v in zip(("latents", "mean", "logvar", "grad"), a, b):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v), name
    # ... and the module's
    lat, g = _hip(enc, x, S, eps, gw)
    assert torch.equal(lat, a[0]) and torch.equal(g, a[3])


@pytest.mark.parametrize("prec", PRECS)
def test_the_packed_16_bit_tensors_are_the_rounded_weights(encs, weights, prec):
    """the packed copy starts with the raw float32 array, bit for bit, and is smaller than the float32 one by half of the B
    operands; a packed buffer of the float32 size is refused at a 16-bit precision"""
    enc = encs[prec]
    packed = enc._packed(DEV)
    raw = enc.weights
    assert torch.equal(packed[:raw.numel() * 4].view(torch.float32), raw)
    assert packed.numel() < encs["f32"]._packed(DEV).numel()
    L = hip_lib.lib()
    big = torch.empty(encs["f32"]._packed(DEV).numel(), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    assert L.soar_vae_pack_weights16(raw.data_ptr(), raw.numel(), big.data_ptr(), big.numel(), CODES[prec], stream) != 0
    assert f"at precision {CODES[prec]}" in hip_lib.last_error()
    # the first 16-bit region, 256-byte aligned behind the raw copy: down.0.block.0.conv1 as [Cout][tap][Cin]
    off = (raw.numel() * 4 + 255) // 256 * 256
    w = weights["encoder.down.0.block.0.conv1.weight"].to(DEV)
    want = w.reshape(128, 128, 9).permute(0, 2, 1).to(DTYPES[prec]).contiguous()
    got = packed[off:off + want.numel() * 2].view(DTYPES[prec]).view(128, 9, 128)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # ... and its data-gradient form right behind it: [Cin][8 - tap][Cout]
    off2 = off + want.numel() * 2
    wantr = w.reshape(128, 128, 9).flip(-1).permute(1, 2, 0).to(DTYPES[prec]).contiguous()
    gotr = packed[off2:off2 + wantr.numel() * 2].view(DTYPES[prec]).view(128, 9, 128)
    assert torch.equal(gotr.view(torch.int16), wantr.view(torch.int16))
