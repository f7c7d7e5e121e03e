"""GPU tests of LPIPS-VGG (csrc/lpips.hip, soar_amd/lpips.py) against the float64 restatement (tests/lpips_ref.py) on the device:
values and input gradients at 16 x 16, 67 x 45 and 512 x 512, the gradient of in1, strided inputs, batching, reproducibility, a
dead tap, graph capture, empty batches and the refusals."""
import pytest
import torch

import lpips_ref as R
from soar_amd.lpips import LPIPSVGG

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# fixed bars (the measured margins).  At 512 x 512 float32 and float64 open a few ReLU / pool gates differently
# (values within rounding of 0 or of a tie); the float32 torch evaluation lands at the same distance (measured: HIP 2.7e-3 / 2.4e-2,
# torch 2.1e-3 / 6.9e-2), hence the wider gradient bars there
VALUE_REL = 2e-5
GRAD_L2 = 1e-4
GRAD_WORST = 1e-3
BARS_512 = (VALUE_REL, 1e-2, 1e-1)
# a float32 evaluation by torch (MIOpen) must itself be this close to float64, or the oracle is broken
TORCH32_VALUE_CAP, TORCH32_GRAD_CAP = 1e-3, 1e-2


@pytest.fixture(scope="module")
def model():
    return LPIPSVGG(R.lpips_state_dict(R.random_weights(0))).to(DEV)


def _pair(N, H, W, seed):
    a = R.normal_images(N, H, W, seed)
    b = (a + 0.3 * R.normal_images(N, H, W, seed + 100)).clamp(-1, 1)      # a target close to the prediction
    return a.to(DEV), b.to(DEV)


def _hip(m, a, b, gw, grad0=True, grad1=False):
    x, y = a.clone().requires_grad_(grad0), b.clone().requires_grad_(grad1)
    v = m(x, y)
    (v.view(-1) * gw).sum().backward()
    torch.cuda.synchronize()
    return v.detach().view(-1), x.grad, y.grad


def _torch(w, a, b, gw, dtype):
    # the float64 oracle decides pool windows at float32 resolution: exact ties fill the constant (masked) regions
    x = a.to(dtype).clone().requires_grad_(True)
    v = R.lpips(x, b.to(dtype), w, f32_ties=dtype == torch.float64)
    (v.view(-1) * gw.to(dtype)).sum().backward()
    return v.detach().view(-1).double(), x.grad.double()


def _errs(v, g, v_ref, g_ref):
    g, g_ref = g.double(), g_ref.double()
    return (float((v.double() - v_ref).abs().max() / v_ref.abs().max()),
            float((g - g_ref).norm() / g_ref.norm()),
            float((g - g_ref).abs().max() / g_ref.abs().max()))


@pytest.mark.parametrize("N,H,W", [(1, 16, 16), (2, 67, 45), (1, 512, 512)])
def test_matches_float64(model, N, H, W):
    a, b = _pair(N, H, W, seed=H)
    gw = torch.rand(N, generator=torch.Generator().manual_seed(N)).add(0.5).to(DEV)
    v, g, _ = _hip(model, a, b, gw)
    assert v.shape == (N,) and g.shape == a.shape and torch.isfinite(g).all()
    w64 = R.weights_of(model, torch.float64)
    v64, g64 = _torch(w64, a, b, gw, torch.float64)
    v32, g32 = _torch(R.weights_of(model, torch.float32), a, b, gw, torch.float32)
    hip, t32 = _errs(v, g, v64, g64), _errs(v32, g32, v64, g64)
    print(f"\n{N}x{H}x{W} value {float(v64[0]):.6f}  HIP value/gradL2/gradworst {hip[0]:.2e} {hip[1]:.2e} {hip[2]:.2e}"
          f"  torch-f32 {t32[0]:.2e} {t32[1]:.2e} {t32[2]:.2e}  dead ReLU share at relu1_2 "
          f"{float((R.features(a.double(), w64)[0] == 0).double().mean()):.2f}")
    assert t32[0] < TORCH32_VALUE_CAP and t32[1] < TORCH32_GRAD_CAP, t32
    assert float(v64.min()) > 0 and float(g64.abs().max()) > 0
    bars = BARS_512 if H == 512 else (VALUE_REL, GRAD_L2, GRAD_WORST)
    assert hip[0] <= bars[0] and hip[1] <= bars[1] and hip[2] <= bars[2], hip


def test_in1_gradient_is_in0s_of_the_swapped_call(model):
    a, b = _pair(2, 40, 36, 7)
    gw = torch.tensor([0.7, 1.3], device=DEV)
    v, _, g1 = _hip(model, a, b, gw, grad0=False, grad1=True)
    vs, gs0, _ = _hip(model, b, a, gw)
    assert torch.equal(v, vs) and torch.equal(g1, gs0)
    # both at once: each as when asked alone
    v2, g0b, g1b = _hip(model, a, b, gw, grad0=True, grad1=True)
    _, g0a, _ = _hip(model, a, b, gw)
    assert torch.equal(v2, v) and torch.equal(g1b, g1) and torch.equal(g0b, g0a)


def test_channels_last_view_is_bit_equal_to_its_contiguous_copy(model):
    a, b = _pair(2, 48, 40, 9)
    base = a.permute(0, 2, 3, 1).contiguous().requires_grad_(True)             # [N, H, W, 3], as the renderer keeps images
    view = base.permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    grads = []
    view.register_hook(lambda g: grads.append(g))
    v = model(view, b)
    v.sum().backward()
    c = base.detach().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    vc = model(c, b)
    vc.sum().backward()
    assert torch.equal(v, vc)
    assert torch.equal(base.grad.permute(0, 3, 1, 2), c.grad)
    assert grads[0].stride() == view.stride()                                  # the gradient of the view, in its own layout


def test_batch_of_two_is_bit_equal_to_two_calls(model):
    a, b = _pair(2, 67, 45, 11)
    gw = torch.tensor([1.0, 2.0], device=DEV)
    v, g, _ = _hip(model, a, b, gw)
    for n in range(2):
        vn, gn, _ = _hip(model, a[n:n + 1], b[n:n + 1], gw[n:n + 1])
        assert torch.equal(v[n:n + 1], vn) and torch.equal(g[n:n + 1], gn)


def test_two_runs_are_bit_equal(model):
    a, b = _pair(1, 128, 96, 13)
    gw = torch.ones(1, device=DEV)
    r1, r2 = _hip(model, a, b, gw), _hip(model, a, b, gw)
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1])


def test_dead_tap_is_finite_and_matches(model):
    m = LPIPSVGG(R.lpips_state_dict(R.random_weights(0, dead_layer=6))).to(DEV)
    a, b = _pair(2, 67, 45, 15)
    gw = torch.ones(2, device=DEV)
    w64 = R.weights_of(m, torch.float64)
    t = R.features(a.double(), w64)
    assert float(t[2].abs().max()) == 0 and float(t[0].abs().max()) > 0 and float(t[1].abs().max()) > 0
    v, g, _ = _hip(m, a, b, gw)
    assert torch.isfinite(v).all() and not torch.isnan(g).any() and torch.isfinite(g).all()
    v64, g64 = _torch(w64, a, b, gw, torch.float64)
    e = _errs(v, g, v64, g64)
    print("\ndead tap", e)
    assert e[0] <= VALUE_REL and e[1] <= GRAD_L2 and e[2] <= GRAD_WORST, e


def test_graph_capture_replays_equal_to_eager(model):
    a, b = _pair(1, 64, 64, 17)
    x = a.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            x.grad = None
            model(x, b).sum().backward()
    torch.cuda.current_stream().wait_stream(s)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        v = model(x, b)
        v.sum().backward()
    with torch.no_grad():
        x.copy_(a * 0.5)
    graph.replay()
    torch.cuda.synchronize()
    ve, ge, _ = _hip(model, a * 0.5, b, torch.ones(1, device=DEV))
    assert torch.equal(v.detach().view(-1), ve) and torch.equal(x.grad, ge)


def test_empty_batch_and_no_grad(model):
    z = torch.zeros(0, 3, 32, 32, device=DEV, requires_grad=True)
    v = model(z, torch.zeros(0, 3, 32, 32, device=DEV))
    assert v.shape == (0, 1, 1, 1)
    v.sum().backward()
    assert z.grad.shape == z.shape
    a, b = _pair(1, 32, 32, 19)
    with torch.no_grad():
        vn = model(a.clone().requires_grad_(True), b)
    assert not vn.requires_grad and torch.equal(vn.view(-1), _hip(model, a, b, torch.ones(1, device=DEV))[0])


def test_refusals(model):
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="N, 3, H, W"):
        model(torch.zeros(1, 1, 32, 32, device=DEV), torch.zeros(1, 1, 32, 32, device=DEV))
    with pytest.raises(ValueError, match="N, 3, H, W"):
        model(torch.zeros(3, 32, 32, device=DEV), torch.zeros(3, 32, 32, device=DEV))
    with pytest.raises(ValueError, match="same shape"):
        model(x, torch.zeros(2, 3, 32, 32, device=DEV))
    with pytest.raises(TypeError, match="float32"):
        model(x.double(), x.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(x, x.cpu())
    with pytest.raises(ValueError, match=">= 16"):
        model(torch.zeros(1, 3, 15, 64, device=DEV), torch.zeros(1, 3, 15, 64, device=DEV))
    cpu_model = LPIPSVGG(R.lpips_state_dict(R.random_weights(1)))
    with pytest.raises(RuntimeError, match="move the module"):
        cpu_model(x, x)
