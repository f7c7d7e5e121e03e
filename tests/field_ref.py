"""The attribute field's specification restated in torch (DESIGN.md "Attribute field"), in float64 or float32.

Vectorised as nerfstudio's torch fallback is: all levels at once, eight gathers by advanced indexing, ``F.linear`` heads.  The
cells (ceil / floor) and the selector always come from the float32 evaluation, so that a float64 restatement and the kernels
agree on the cell; the offsets o, the weights and everything after them are evaluated in ``dtype``.  With ``value32`` the
offsets also take their value from the float32 q (the GPU tests: what float32 input rounding does to o at level 15, ~2e-4,
is then the same on both sides, and the comparison measures the arithmetic after it)."""
import numpy as np
import torch
import torch.nn.functional as F

HEADS = ("shs", "scales", "quats", "offsets", "opacities")
PRIMES = (1, 2654435761, 805459861)


def resolutions(num_levels=16, base_res=16, max_res=2048):
    g = np.exp((np.log(max_res) - np.log(base_res)) / (num_levels - 1))
    return torch.floor(base_res * g ** torch.arange(num_levels))          # float32, as nerfstudio computes it


_PRIMES = {}


def hash_slots(coords, T):
    """coords int [..., 3] -> slot in [0, T): int64 products, xor, then % T (nerfstudio's hash_fn)."""
    if coords.device not in _PRIMES:
        _PRIMES[coords.device] = torch.tensor(PRIMES, dtype=torch.int64, device=coords.device)
    c = coords.to(torch.int64) * _PRIMES[coords.device]
    return torch.bitwise_xor(torch.bitwise_xor(c[..., 0], c[..., 1]), c[..., 2]) % T


def normalise(xyz, aabb, is_normalized, dtype):
    """-> (p in dtype, p in float32) [N, 3]"""
    x = xyz.reshape(-1, 3)
    if is_normalized:
        return x.to(dtype), x.detach().to(torch.float32)
    if dtype == torch.float32:                      # one evaluation, as nerfstudio's fallback makes
        p = (x - aabb[0]) / (aabb[1] - aabb[0])
        p = p * ((p > 0) & (p < 1)).all(dim=-1, keepdim=True)
        return p, p.detach()
    x32, a32 = x.detach().to(torch.float32), aabb.to(torch.float32)
    p32 = (x32 - a32[0]) / (a32[1] - a32[0])
    sel = ((p32 > 0) & (p32 < 1)).all(dim=-1, keepdim=True)
    a = aabb.to(dtype)
    p = (x.to(dtype) - a[0]) / (a[1] - a[0])
    return p * sel.to(dtype), p32 * sel


_CORNER_BITS = {}


def _corner_bits(device):
    """[8, 1, 3] bool: corner k takes the ceiling on axis d where bit d of k is set (built once per device)"""
    if device not in _CORNER_BITS:
        _CORNER_BITS[device] = torch.tensor([[(k >> d) & 1 for d in range(3)] for k in range(8)], dtype=torch.bool,
                                            device=device)[:, None, :]
    return _CORNER_BITS[device]


def corner_terms(p, p32, res, T, value32=False):
    """the eight corners' (rows [N, L] into a [L*T, 2] table, weights [N, L, 1] in p's dtype), in corner order; then the float32
    cells (ceil, floor) [N, L, 3] int32 that they were taken from"""
    L = res.shape[0]
    res = res.to(p.device)
    if p.dtype == torch.float32:
        q = p[:, None, :] * res[None, :, None]                              # [N, L, 3]
        q32 = q.detach()
    else:
        q32 = p32[:, None, :] * res[None, :, None]                          # float32: the cells
        q = p[:, None, :] * res.to(p.dtype)[None, :, None]
        if value32:
            q = q32.to(p.dtype) + (q - q.detach())
    c, f = torch.ceil(q32).to(torch.int32), torch.floor(q32).to(torch.int32)
    o = q - f.to(p.dtype)
    off = (torch.arange(L, device=p.device) * T)[None, :]
    bits = _corner_bits(p.device)
    terms = []
    for k in range(8):
        corner = torch.where(bits[k], c, f)
        w = torch.where(bits[k], o, 1 - o).prod(dim=-1, keepdim=True)       # [N, L, 1]
        terms.append((hash_slots(corner, T) + off, w))
    return terms, (c, f)


def encode(p, p32, table, res, T, value32=False):
    """-> [N, 2L] level-major; table [L*T, 2] in p's dtype.  value32: q takes its VALUE from the float32 product (the kernels'
    input) and its derivative from p, so that a float64 restatement measures the arithmetic after the input's rounding"""
    enc = 0
    for rows, w in corner_terms(p, p32, res, T, value32)[0]:
        enc = enc + w * table[rows]
    return enc.reshape(p.shape[0], 2 * res.shape[0])


def heads(e, qe, z, W):
    """W: {head: (w1, b1, w2, b2)} in e's dtype"""
    def mlp(h, x):
        w1, b1, w2, b2 = W[h]
        return F.linear(F.relu(F.linear(x, w1, b1)), w2, b2)
    zz = torch.zeros(e.shape[0], 2, dtype=e.dtype, device=e.device) if z is None else z.to(e.dtype)[None].expand(e.shape[0], -1)
    return {"shs": torch.sigmoid(mlp("shs", e)), "scales": torch.sigmoid(mlp("scales", e)) * 2e-2,
            "quats": F.normalize(mlp("quats", qe), p=2, dim=-1), "offsets": mlp("offsets", torch.cat([e, zz], -1)),
            "opacities": torch.sigmoid(mlp("opacities", e))}


def field(xyz, z, table, qtable, W, aabb, res, T, is_normalized=False, dtype=torch.float64, value32=False):
    p, p32 = normalise(xyz, aabb, is_normalized, dtype)
    return heads(encode(p, p32, table, res, T, value32), encode(p, p32, qtable, res, T, value32), z, W)


def params_of(module, dtype, device=None, requires_grad=True):
    """leaf copies of a HashMLPField's parameters: (table, qtable, {head: (w1, b1, w2, b2)})"""
    def leaf(t):
        return t.detach().to(device or t.device, dtype).clone().requires_grad_(requires_grad)
    W = {}
    for h in HEADS:
        m = getattr(module, f"mlp_base_{h}")
        W[h] = tuple(leaf(t) for t in (m.layers[0].weight, m.layers[0].bias, m.layers[1].weight, m.layers[1].bias))
    return leaf(module.encoding.hash_table), leaf(module.quat_encoding.hash_table), W


PARAM_NAMES = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias")


def run(module, xyz, z, loss, xyz_grad, dtype, is_normalized=False, res=None, T=None, value32=True, device=None):
    """The restatement on leaf copies of ``module``'s parameters, then ``loss(out).backward()``: -> (out, grads), the gradients
    under the names of ``module.named_parameters()`` plus "xyz" and "z".  ``res`` / ``T`` default to the module's own levels and
    table size."""
    table, qtable, W = params_of(module, dtype, device)
    x = xyz.detach().to(table.device, dtype).clone().requires_grad_(xyz_grad)
    zz = None if z is None else z.detach().to(table.device, dtype).clone().requires_grad_(z.requires_grad)
    if res is None:
        res = module.encoding.scalings.clone()
    if T is None:
        T = 2 ** int(module.log2_hashmap_size)
    aabb = None if module.aabb is None else module.aabb.to(table.device)
    out = field(x, zz, table, qtable, W, aabb, res, T, is_normalized, dtype, value32=value32)
    loss(out).backward()
    grads = {"encoding.hash_table": table.grad, "quat_encoding.hash_table": qtable.grad, "xyz": x.grad,
             "z": None if zz is None else zz.grad}
    for h in HEADS:
        for i, nm in enumerate(PARAM_NAMES):
            grads[f"mlp_base_{h}.{nm}"] = W[h][i].grad
    return out, grads


class RefField(torch.nn.Module):
    """The restatement as a module with its own float32 parameters (a stand-in field for the plugin and reset_field)."""

    def __init__(self, module, dtype=torch.float32):
        super().__init__()
        self.dtype = dtype
        self.register_buffer("aabb", module.aabb.detach().clone())
        table, qtable, W = params_of(module, dtype)
        self.table, self.qtable = torch.nn.Parameter(table), torch.nn.Parameter(qtable)
        self.heads = torch.nn.ParameterDict({f"{h}_{i}": torch.nn.Parameter(t) for h in HEADS for i, t in enumerate(W[h])})
        self.register_buffer("res", resolutions(int(module.num_levels), 16, int(module.max_res)))
        self.T = 2 ** int(module.log2_hashmap_size)

    def forward(self, xyzs, pose=None, z=None, is_normalized=False):
        W = {h: tuple(self.heads[f"{h}_{i}"] for i in range(4)) for h in HEADS}
        return field(xyzs, z, self.table, self.qtable, W, self.aabb, self.res, self.T, is_normalized, self.dtype)
