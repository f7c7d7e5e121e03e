"""CPU tests of the attribute field (soar_amd/field.py): the specification's constants, the float64 restatement
(tests/field_ref.py) against autograd, the module's parameters, and argument checks that stop before any GPU work."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_ref as R
from soar_amd import field as FLD

RES = [16, 22, 30, 42, 58, 80, 111, 153, 212, 294, 406, 561, 776, 1072, 1482, 2047]


def test_level_resolutions_end_at_2047():
    assert FLD.level_resolutions().tolist() == RES
    assert R.resolutions().tolist() == RES
    assert FLD.level_resolutions().dtype == torch.float32


def test_u32_hash_equals_int64_modulo():
    g = torch.Generator().manual_seed(0)
    c = torch.randint(-5000, 5001, (20000, 3), generator=g, dtype=torch.int32)
    T = 2 ** 18
    u = c.numpy().astype(np.uint32)
    with np.errstate(over="ignore"):
        slot = (u[:, 0] ^ (u[:, 1] * np.uint32(2654435761)) ^ (u[:, 2] * np.uint32(805459861))) & np.uint32(T - 1)
    assert np.array_equal(slot.astype(np.int64), R.hash_slots(c, T).numpy())
    assert (c < 0).any()


def _small(seed=0, T=64):
    g = torch.Generator().manual_seed(seed)
    W = {}
    for h, out in FLD.HEAD_OUT.items():
        i = 34 if h == "offsets" else 32
        W[h] = tuple((torch.rand(s, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
                     for s in ((64, i), (64,), (out, 64), (out,)))
    table = ((torch.rand(16 * T, 2, generator=g, dtype=torch.float64) - 0.5) * 0.5).requires_grad_(True)
    qtable = ((torch.rand(16 * T, 2, generator=g, dtype=torch.float64) - 0.5) * 0.5).requires_grad_(True)
    return W, table, qtable


def test_restatement_passes_gradcheck():
    T = 64
    res = R.resolutions(16, 2, 64)
    aabb = torch.tensor([[-1.0, -0.5, -0.8], [1.0, 0.7, 0.9]], dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    cand = aabb[0] + (aabb[1] - aabb[0]) * (0.05 + 0.9 * torch.rand(200, 3, generator=g, dtype=torch.float64))
    p = ((cand - aabb[0]) / (aabb[1] - aabb[0])).float()
    q = p[:, None, :] * res[None, :, None]
    far = ((q - q.round()).abs() > 0.05).reshape(200, -1).all(1)          # away from every level's cell boundaries
    xyz = cand[far][:3].clone().requires_grad_(True)
    assert xyz.shape[0] == 3
    W, table, qtable = _small()
    z = torch.tensor([0.3, -0.2], dtype=torch.float64, requires_grad=True)
    names = list(R.HEADS)
    flat = [t for h in names for t in W[h]]

    def fn(xyz, z, table, qtable, *ws):
        Wd = {h: tuple(ws[4 * k: 4 * k + 4]) for k, h in enumerate(names)}
        out = R.field(xyz, z, table, qtable, Wd, aabb, res, T)
        return tuple(out[h] for h in names)

    assert torch.autograd.gradcheck(fn, (xyz, z, table, qtable, *flat), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_weights_sum_to_one_and_lattice_points_read_a_row():
    T = 2 ** 10
    res = R.resolutions()
    g = torch.Generator().manual_seed(2)
    ones = torch.ones(16 * T, 2, dtype=torch.float64)
    p = torch.rand(500, 3, generator=g)
    e = R.encode(p.double(), p, ones, res, T)
    assert torch.allclose(e, torch.ones_like(e), atol=1e-12)
    table = torch.randn(16 * T, 2, generator=g, dtype=torch.float64)
    lat = torch.tensor([[0.5, 0.25, 0.75], [0.0, 0.5, 0.5]])               # lattice points of level 0 (res 16)
    e = R.encode(lat.double(), lat, table, res, T)
    for i in range(2):
        cell = (lat[i] * 16).to(torch.int64)
        assert torch.equal(e[i, :2], table[R.hash_slots(cell, T)])


def test_module_parameters_init_and_param_groups():
    torch.manual_seed(0)
    aabb = torch.tensor([[-1.0, -1.2, -0.5], [1.0, 0.9, 0.6]])
    f = FLD.HashMLPField(aabb)
    shapes = {n: tuple(p.shape) for n, p in f.named_parameters()}
    T = 2 ** 18
    want = {"encoding.hash_table": (16 * T, 2), "quat_encoding.hash_table": (16 * T, 2)}
    for h, out in FLD.HEAD_OUT.items():
        i = 34 if h == "offsets" else 32
        want.update({f"mlp_base_{h}.layers.0.weight": (64, i), f"mlp_base_{h}.layers.0.bias": (64,),
                     f"mlp_base_{h}.layers.1.weight": (out, 64), f"mlp_base_{h}.layers.1.bias": (out,)})
    assert shapes == want
    for t in (f.encoding.hash_table, f.quat_encoding.hash_table):
        assert t.abs().max() <= 1e-3 and t.abs().max() > 0.9e-3 and abs(float(t.mean())) < 1e-5
    assert f.mlp_base_offsets.layers[-1].weight.abs().max() == 0 and f.mlp_base_offsets.layers[-1].bias.abs().max() == 0
    assert f.mlp_base_shs.layers[0].weight.abs().max() <= 1 / np.sqrt(32) and f.mlp_base_shs.layers[1].weight.abs().max() > 0
    assert {n for n, _ in f.named_buffers()} == {"aabb", "max_res", "num_levels", "log2_hashmap_size"}
    assert int(f.max_res) == 2048 and int(f.num_levels) == 16 and int(f.log2_hashmap_size) == 18
    f.mlp_base_offsets.layers[-1].weight.data.zero_()                       # the reference's zero-init line
    groups = [{"params": f.encoding.parameters(), "lr": 1e-2, "name": "attribute_field_encoding"},
              {"params": f.quat_encoding.parameters(), "lr": 1e-2, "name": "attribute_field_quat_encoding"},
              {"params": f.mlp_base_shs.parameters(), "lr": 1e-2, "name": "attribute_field_shs"},
              {"params": f.mlp_base_quats.parameters(), "lr": 1e-2, "name": "attribute_field_quats"},
              {"params": f.mlp_base_scales.parameters(), "lr": 1e-1, "name": "attribute_field_scales"},
              {"params": f.mlp_base_offsets.parameters(), "lr": 1e-4, "name": "attribute_field_offests"}]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    assert [len(g["params"]) for g in opt.param_groups] == [1, 1, 4, 4, 4, 4]


def test_refusals():
    aabb = torch.tensor([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
    for kw in ({"num_layers": 3}, {"hidden_dim": 32}, {"features_per_level": 4}, {"log2_hashmap_size": 25}, {"num_levels": 8}):
        with pytest.raises(NotImplementedError):
            FLD.HashMLPField(aabb, **kw)
    with pytest.raises(NotImplementedError):
        FLD.HashMLPField(aabb, use_linear=True)
    f = FLD.HashMLPField(aabb, log2_hashmap_size=8, implementation="torch", device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(torch.zeros(4, 3))
    with pytest.raises(ValueError):
        f(torch.zeros(4, 2))
    with pytest.raises(ValueError):
        f.get_attributes(torch.zeros(4, 4))


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_c_entries_check_arguments(lib):
    from soar_amd import hip_lib
    n = C.c_size_t(0)
    assert lib.soar_field_workspace_bytes(100000, C.byref(n)) == 0 and n.value >= 5 * 100000 * 32 * 4 and n.value % 256 == 0
    assert lib.soar_field_workspace_bytes(-1, C.byref(n)) != 0 and "N=-1" in hip_lib.last_error()
    a = hip_lib.SoarFieldArgs()
    a.N, a.log2_T = 10, 18
    for l, r in enumerate(RES):
        a.res[l] = r
    assert lib.soar_field_forward(C.byref(a), None) != 0 and "NULL table" in hip_lib.last_error()
    a.table = a.qtable = 0x1000
    a.xyz, a.aabb = 0x1000, 0x1000
    assert lib.soar_field_forward(C.byref(a), None) != 0 and "weight of head 0" in hip_lib.last_error()
    for k in range(5):
        a.head[k].w1 = a.head[k].b1 = a.head[k].w2 = a.head[k].b2 = 0x1000
    assert lib.soar_field_forward(C.byref(a), None) != 0 and "enc" in hip_lib.last_error()
    a.enc = a.qenc = 0x1000
    assert lib.soar_field_forward(C.byref(a), None) != 0 and "NULL output" in hip_lib.last_error()
    assert lib.soar_field_backward(C.byref(a), None, 0, None) != 0 and "workspace" in hip_lib.last_error()
    a.log2_T = 25
    assert lib.soar_field_forward(C.byref(a), None) != 0 and "log2_T" in hip_lib.last_error()
    a.log2_T, a.N = 18, 1 << 27
    assert lib.soar_field_backward(C.byref(a), None, 0, None) != 0 and "N <=" in hip_lib.last_error()
    a.N, a.res[15] = 10, 0.0
    assert lib.soar_field_forward(C.byref(a), None) != 0 and "resolution 15" in hip_lib.last_error()
