"""The environment-map background's specification restated in torch: tiny-cuda-nn's SphericalHarmonics of
degree 3 on ``(dirs + 1) / 2`` and threestudio's VanillaMLP without bias, then sigmoid.

The round trip ``u = (d + 1) / 2``, ``x = u * 2 - 1`` is evaluated in float32, as torch and tiny-cuda-nn evaluate it; the basis,
the layers and the sigmoid in ``dtype`` (float64 by default).  With ``gates32`` the ReLUs open where a float32 evaluation in the
kernels' order opens them (the GPU tests): a pre-activation within float32 rounding of zero would otherwise switch a whole
pixel's gradient on in one evaluation and off in the other, and the comparison measures the arithmetic, not those few pixels."""
import torch
import torch.nn.functional as F

C0 = 0.28209479177387814
C1 = 0.48860251190291987
C2 = 1.0925484305920792
C20 = 0.94617469575755997
C20b = 0.31539156525251999
C22 = 0.54627421529603959


def round_trip(dirs):
    """float32 d -> float32 x = ((d + 1) / 2) * 2 - 1, component-wise"""
    u = (dirs.to(torch.float32) + 1.0) / 2.0
    return u * 2.0 - 1.0


def basis(v):
    """the 9 values of tcnn's SphericalHarmonics (degree 3) at v [..., 3], in v's dtype"""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    return torch.stack([torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x, C2 * x * y, -C2 * y * z, C20 * z * z - C20b,
                        -C2 * x * z, C22 * x * x - C22 * y * y], -1)


def encode(dirs, dtype=torch.float64):
    return basis(round_trip(dirs).to(dtype))


def mlp(e, w1, w2, w3, gates=None):
    if gates is None:
        return F.linear(F.relu(F.linear(F.relu(F.linear(e, w1)), w2)), w3)
    zero = e.new_zeros(())
    h1 = torch.where(gates[0], F.linear(e, w1), zero)
    h2 = torch.where(gates[1], F.linear(h1, w2), zero)
    return F.linear(h2, w3)


def _basis32(x):
    """the basis in float32 in the kernels' order of operations (products of the coordinates first)"""
    f = torch.float32
    c = {k: torch.tensor(v, dtype=f).item() for k, v in (("c1", C1), ("c2", C2), ("c20", C20), ("c20b", C20b), ("c22", C22))}
    X, Y, Z = x[..., 0], x[..., 1], x[..., 2]
    return torch.stack([torch.full_like(X, C0), -c["c1"] * Y, c["c1"] * Z, -c["c1"] * X, c["c2"] * (X * Y), -c["c2"] * (Y * Z),
                        c["c20"] * (Z * Z) - c["c20b"], -c["c2"] * (X * Z), c["c22"] * (X * X) - c["c22"] * (Y * Y)], -1)


def _matvec32(x, w):
    """x [..., K] @ w.T in float32: each product rounded, then added in input order from 0"""
    s = x.new_zeros(x.shape[:-1] + (w.shape[0],))
    for k in range(w.shape[1]):
        s = s + x[..., k:k + 1] * w[:, k]
    return s


def gates32(dirs, w1, w2):
    """the ReLU decisions (pre-activation > 0) of layers 1 and 2 in a float32 evaluation in the kernels' order"""
    w1, w2 = w1.detach().to(torch.float32), w2.detach().to(torch.float32)
    s1 = _matvec32(_basis32(round_trip(dirs)), w1)
    s2 = _matvec32(torch.clamp_min(s1, 0), w2)
    return s1 > 0, s2 > 0


def background(dirs, w1, w2, w3, dtype=torch.float64, gates32_=False):
    """-> [B, H, W, 3] in dtype"""
    gates = gates32(dirs, w1, w2) if gates32_ else None
    return torch.sigmoid(mlp(encode(dirs, dtype), w1.to(dtype), w2.to(dtype), w3.to(dtype), gates))


def weights_of(module, dtype=torch.float64, requires_grad=True):
    return [module.network.layers[k].weight.detach().to(dtype).clone().requires_grad_(requires_grad) for k in (0, 2, 4)]


def composite(renders, masks, bg, n_comp):
    """the renderer's composite: renders + (1 - masks) * bg[:n_comp] in NCHW"""
    return renders + (1 - masks) * bg[:n_comp].permute(0, 3, 1, 2)


class RefBackground(torch.nn.Module):
    """The restatement as a background with its own float32 weights (the torch form the timing script measures)."""

    def __init__(self, module, dtype=torch.float32):
        super().__init__()
        self.dtype = dtype
        self.w = torch.nn.ParameterList([torch.nn.Parameter(w) for w in weights_of(module, dtype)])

    def forward(self, dirs):
        return background(dirs, *self.w, dtype=self.dtype)
