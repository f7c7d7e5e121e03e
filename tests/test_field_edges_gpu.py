"""GPU tests of the attribute field (csrc/field.hip) at its edges, on the scenes of tests/field_cases.py.

**Bit for bit.**  On the exact scenes (dyadic inputs, summed magnitudes below 2^23 grid units: tests/test_field_cases_cpu.py
holds them to that) no order of summation rounds, so the offsets output, the table gradient (float atomics after ``wave_add``'s
segmented scan, or after the block's LDS sums at 32 rows per level or fewer), dL/dz and the offsets head's four gradients must
``torch.equal`` the float64 restatement cast to float32: every
point order at log2_T 1, 4, 10 and N in 1 .. 777, one scene each at 2^18 and 2^19, levels 2 .. 64, and the box with points on and
outside its faces.  A lost, doubled or misplaced contribution of one lane changes an element by at least one grid unit.

The quaternion table has no exact scene: its head divides by |y|, which is a float32 number only where y is an integer
quadruple with an integer norm, and a y that does not move with the encoding sends nothing to the table.  The quats table is held
per element below instead.

**Per element**, on the random real-valued field: HIP against float64 at most 4 x (float32 restatement against float64), floor 1e-6
of the tensor's largest magnitude, for every output and every gradient, at log2_T 1, 4, 12 (hundreds to
thousands of contributions per table element), at lattice points and normalised points outside [0, 1] for dL/dxyz, at the quaternion norm's
floor, and under saturated sigmoids.

Measured on an MI355X (worst element over the tensor's largest magnitude: HIP / float32 restatement on the device; a range is
the spread over runs, the atomics' arrival order differing from run to run):

=================  =======================  ===================  ===================  =================  ====================
scene              outputs (worst head)     d encoding table     d quats table        d xyz              heads' gradients, d z
=================  =======================  ===================  ===================  =================  ====================
T=2^1 random       3.9e-7 / 1.4e-7 (quats)  8.9-9.3e-7 / 1.2e-6  3.4-6.1e-7 / 6.4e-7  5.4e-7 / 4.7e-7    <= 3.7e-7 / 4.4e-6
T=2^1 spatial      3.9e-7 / 1.4e-7          4.9-6.3e-7 / 7.5e-7  2.6-3.6e-7 / 4.6e-7  4.4e-7 / 3.3e-7    <= 3.7e-7 / 4.4e-6
T=2^4 random       3.4e-7 / 9.7e-8 (offs.)  2.0-2.1e-7 / 2.5e-7  2.3-2.6e-7 / 2.9e-7  2.2e-7 / 2.3e-7    <= 2.6e-7 / 3.0e-6
T=2^4 spatial      3.4e-7 / 9.7e-8          2.5-3.2e-7 / 3.7e-7  2.8e-7 / 2.9e-7      3.1e-7 / 2.4e-7    <= 4.7e-6 / 1.1e-5
T=2^12 random      4.5e-7 / 1.2e-7 (offs.)  2.3-2.5e-7 / 1.4e-7  2.5-3.3e-7 / 2.5e-7  2.1e-7 / 1.7e-7    <= 1.8e-7 / 2.8e-7
T=2^12 spatial     4.5e-7 / 1.2e-7          1.2-1.6e-7 / 1.1e-7  1.9-2.4e-7 / 1.3e-7  1.7e-7 / 1.8e-7    <= 3.2e-7 / 4.2e-7
lattice + outside  3.9e-7 / 9.3e-8 (offs.)  1.1-1.3e-7 / 1.1e-7  2.4-2.8e-7 / 2.1e-7  2.7e-7 / 1.7e-7    <= 3.2e-7 / 2.9e-7
quats at 0, 1e-13  4.4e-7 / 1.1e-7 (offs.)  2.1-4.4e-7 / 1.5e-7  0 / 0                1.5e-7 / 2.6e-7    <= 2.2e-7 / 4.7e-6
saturated          1.3e-4 / 9.9e-5 (shs)    1.3e-4 / 3.7e-4      2.9-3.1e-7 / 1.9e-7  1.6e-4 / 7.9e-5    <= 9.8e-5 / 8.2e-5
=================  =======================  ===================  ===================  =================  ====================

**What these tests found.**  With one float atomic per run of a wave, the table gradients at 2 and 16 rows per level sat on the
bar and missed it in some runs: 2.0-3.3e-6 (T = 2) and 0.9-1.5e-6 (T = 16) against bars of 1.0-4.6e-6, over three runs.  No
contribution was lost (the exact scenes at those sizes were bit-exact): one float collected 1 500 to 12 000 adds one after the
other, and the same float64 contributions rounded to float32 and added one at a time on the CPU landed in the same place
(2.1-2.8e-6, 0.8-1.7e-6).  ``field_scatter_kernel`` now sums tables of at most 32 rows per level per block in LDS and adds each
element to HBM once per block; the rows T=2^1 and T=2^4 above are measured with it.  Tables of 2 and 16 rows therefore take that
path in every test here, and ``wave_add`` is exercised from 2^10 rows on, where ``one_point`` makes all 64 lanes one run.
"""
import copy

import pytest
import torch

import field_cases as FC
import field_ref as R
from smplify_ref import bar_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_REAL = 3000
_dev_fields = {}


def _on_device(f):
    """a device copy of a shared CPU field (the copy is shared too: tests that change weights take their own)"""
    if id(f) not in _dev_fields:
        _dev_fields[id(f)] = (f, copy.deepcopy(f).to(DEV))
    return _dev_fields[id(f)][1]


def _run_hip(f, xyz, z, loss, xyz_grad, is_normalized=False):
    f.zero_grad(set_to_none=True)
    x = xyz.to(DEV).clone().requires_grad_(xyz_grad)
    out = f(x, z=z, is_normalized=is_normalized)
    loss(out).backward()
    grads = {n: p.grad for n, p in f.named_parameters()}
    grads["xyz"] = x.grad
    grads["z"] = None if z is None else z.grad
    return out, grads


def _all_plus_zero(t):
    return not bool((t.contiguous().view(torch.int32) != 0).any())


def _names(f):
    return [n for n, _ in f.named_parameters()]


# ---- bit for bit ---------------------------------------------------------------------------------------------------------------

def _run_exact(scene, f=None, xyz_grad=False):
    f = _on_device(scene.field) if f is None else f
    z = scene.z.to(DEV).requires_grad_(True)
    return _run_hip(f, scene.points, z, FC.offsets_loss(scene.g), xyz_grad, scene.normalized)


def _assert_exact(scene, tag, xyz_grad=False):
    out, g = _run_exact(scene, xyz_grad=xyz_grad)
    ref = FC.restate(scene, torch.float64)
    got = {"offsets": out["offsets"].detach()}
    got.update({n: g[n] for n in FC.EXACT_NAMES})
    for n, want in ref.items():
        assert got[n] is not None, (tag, n)
        a, b = got[n].cpu(), want.to(torch.float32)
        assert torch.equal(b.double(), want), (tag, n)                        # the cast itself is exact
        if not torch.equal(a, b):
            bad = torch.nonzero((a != b).reshape(a.shape[0], -1).any(dim=1)).flatten()
            raise AssertionError(f"{tag} {n}: {int((a != b).sum())} elements differ from float64, largest difference "
                                 f"{float((a.double() - want).abs().max()) / scene.grid:.1f} grid units, first rows {bad[:8].tolist()}")
    for n in _names(scene.field):
        if n not in FC.EXACT_NAMES:
            assert g[n] is None, (tag, n)                                     # no upstream gradient reaches them
    return out, g


@pytest.mark.parametrize("log2_T", FC.EXACT_LOG2_T)
@pytest.mark.parametrize("order", FC.ORDERS)
def test_exact_scenes_equal_float64(order, log2_T):
    for N in FC.SIZES:
        unselected = order == "box_edges"
        _, g = _assert_exact(FC.exact_case(order, log2_T, N), (order, log2_T, N), xyz_grad=unselected)
        if unselected:
            assert _all_plus_zero(g["xyz"])                                   # exactly +0: nothing is selected


@pytest.mark.parametrize("order,log2_T,N", [c for c in FC.exact_cases() if c[1] > 12])
def test_exact_scenes_at_large_tables(order, log2_T, N):
    _assert_exact(FC.exact_case(order, log2_T, N), (order, log2_T, N))


def test_exact_at_coinciding_and_odd_levels():
    """levels 2, 2, 3, 4, 5, 6, 8, ... 64 under the quarter-lattice runs: neighbouring levels coincide, some are odd"""
    res = R.resolutions(16, **FC.COARSE).tolist()
    assert res[0] == res[1] and any(int(r) % 2 for r in res)
    for log2_T in (4, 10):                                # the block's LDS sums, and wave_add
        for N in FC.SIZES:
            _assert_exact(FC.exact_scene(log2_T, FC.runs(N), **FC.COARSE), ("runs at levels 2..64", log2_T, N))


@pytest.mark.parametrize("log2_T", [1, 10])
def test_exact_in_the_box_with_points_on_its_faces(log2_T):
    """aabb mode, lo = -1, hi = 3: runs of selected points between points outside the box and on its faces.  The unselected are
    encoded at the origin: their outputs are the origin's, bit for bit, and their rows of dL/dxyz are +0"""
    for N in (65, 130, 777):
        pts, inside = FC.box_mixed(N)
        scene = FC.exact_scene(log2_T, pts, normalized=False, aabb=FC.BOX)
        out, g = _assert_exact(scene, ("box", log2_T, N), xyz_grad=True)
        with torch.no_grad():
            origin = _on_device(scene.field)(torch.zeros(1, 3, device=DEV), z=scene.z.to(DEV), is_normalized=True)
        off = ~inside.to(DEV)
        for h in R.HEADS:
            assert torch.equal(out[h][off], origin[h].expand(int(off.sum()), -1)), h
        assert _all_plus_zero(g["xyz"][off])
        assert float(g["xyz"][~off].abs().max()) > 0


def test_exact_table_gradient_is_reproducible():
    """where no sum can round, the atomics' arrival order cannot show: two runs give the same bits (test_field_gpu.py's
    test_reproducible allows the real-valued field 1e-5)"""
    for order, log2_T in (("runs", 4), ("alternating", 1), ("coarse_shared", 10)):
        scene = FC.exact_case(order, log2_T, 777)
        first = _run_exact(scene)[1]["encoding.hash_table"].clone()
        second = _run_exact(scene)[1]["encoding.hash_table"]
        assert torch.equal(first, second), (order, log2_T)
        assert float(first.abs().max()) > 0


# ---- per element, real-valued -----------------------------------------------------------------------------------------------------

def _check_all(tag, f, f_cpu, xyz, z_val, loss, is_normalized):
    """outputs and gradients of one call under the bar, element-wise: every tensor is measured and printed, then the misses are
    raised together; -> (out, grads)"""
    z = None if z_val is None else torch.tensor(z_val, device=DEV, requires_grad=True)
    out, g = _run_hip(f, xyz, z, loss, True, is_normalized)
    r64, g64 = R.run(f_cpu, xyz, z, loss, True, torch.float64, is_normalized, device=DEV)
    r32, g32 = R.run(f_cpu, xyz, z, loss, True, torch.float32, is_normalized, device=DEV)
    todo = [(h, out[h], r32[h], r64[h]) for h in R.HEADS]
    for n in _names(f) + ["xyz"] + ([] if z is None else ["z"]):
        if g64[n] is None:
            assert g[n] is None, (tag, n)
            continue
        assert g[n] is not None, (tag, n)
        todo.append((f"d_{n}", g[n], g32[n], g64[n]))
    missed = []
    for n, a, b, c in todo:
        try:
            bar_check(f"{tag} {n}", a, b, c)
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, missed
    return out, g


_real = {}


def _real_scene(log2_T):
    if log2_T not in _real:
        _real[log2_T] = FC.real_scene(log2_T, N_REAL)
    return _real[log2_T]


@pytest.mark.parametrize("order", ["random", "spatial"])
@pytest.mark.parametrize("log2_T", [1, 4, 12])
def test_every_element_matches_float64(log2_T, order):
    s = _real_scene(log2_T)
    _check_all(f"T=2^{log2_T} {order}", _on_device(s.field), s.field, s.xyz[order], (0.4, -0.3), FC.upstream(N_REAL), False)


def test_position_gradient_on_the_lattice_and_outside():
    """normalised points on the lattices of several levels (o == 0, ceil == floor), random ones, and ones outside [0, 1], whose
    negative cells go through the u32 hash"""
    s = _real_scene(12)
    g = torch.Generator().manual_seed(5)
    v = torch.tensor([0.25, 0.5, 0.75, 0.125, 0.0625])
    lattice = v[torch.randint(0, 5, (300, 3), generator=g)]
    beyond = torch.rand(300, 3, generator=g) * 3 - 1
    beyond[:, 0] = torch.where(torch.arange(300) % 2 == 0, -torch.rand(300, generator=g), 1 + torch.rand(300, generator=g))
    lattice_out = torch.tensor([[-0.25, 0.5, 1.5], [1.25, -0.5, 0.75], [-1.0, 2.0, 0.0]])
    xyz = torch.cat([lattice, torch.rand(300, 3, generator=g), beyond, lattice_out])
    _check_all("lattice", _on_device(s.field), s.field, xyz, (0.4, -0.3), FC.upstream(xyz.shape[0]), True)


@pytest.mark.parametrize("bias", [0.0, 1e-13])
def test_quaternion_head_at_the_norm_floor(bias):
    """second layer of the quats head zero: y = 0, output exactly 0 and dL/dy = g / 1e-12; bias 1e-13: |y| = 2e-13, below eps, the
    output is 0.1 per component"""
    s = _real_scene(12)
    f_cpu = copy.deepcopy(s.field)
    with torch.no_grad():
        f_cpu.mlp_base_quats.layers[1].weight.zero_()
        f_cpu.mlp_base_quats.layers[1].bias.fill_(bias)
    f = copy.deepcopy(f_cpu).to(DEV)
    out, g = _check_all(f"quats bias {bias:g}", f, f_cpu, s.xyz["random"], None, FC.upstream(N_REAL), False)
    q = out["quats"].detach()
    if bias == 0.0:
        assert float(q.abs().max()) == 0
    else:
        assert float((q - 0.1).abs().max()) <= 1e-6
    for n, t in g.items():
        assert t is None or bool(torch.isfinite(t).all()), n
    assert float(g["mlp_base_quats.layers.1.bias"].abs().max()) > 1e11        # the divisor is the floor, 1e-12
    assert float(g["quat_encoding.hash_table"].abs().max()) == 0               # nothing passes a zero second layer


def test_saturated_sigmoids():
    """|y| past 100 on about half of the points of the shs and opacities heads: outputs in [0, 1], gradients under the bar, and
    rows of the table that only saturated points touch get exactly 0 (float32's sigmoid is 0 or 1 there, s (1 - s) = 0)"""
    s = FC.real_scene(16, N_REAL, seed=2)
    f_cpu, xyz = s.field, s.xyz["random"]
    FC.saturate(f_cpu, xyz)
    f = copy.deepcopy(f_cpu).to(DEV)
    out, _ = _check_all("saturated", f, f_cpu, xyz, None, FC.upstream(N_REAL), False)
    for h in ("shs", "opacities"):
        o = out[h].detach()
        assert bool(torch.isfinite(o).all()) and float(o.min()) >= 0 and float(o.max()) <= 1, h
        assert float(o.min()) == 0 and float(o.max()) == 1, h
    # upstream on the two sigmoid heads alone: a point is saturated when every one of its four outputs is past 101
    y = torch.cat([FC.second_layer_outputs(f_cpu, xyz, h) for h in ("shs", "opacities")], dim=1)
    sat = y.abs().min(dim=1)[0] > 101
    assert 50 < int(sat.sum()) < N_REAL - 50
    _, g = _run_hip(f, xyz, None, FC.upstream(N_REAL, heads=("shs", "opacities")), False)
    keys, _, _ = FC.lane_keys(xyz, s.res, s.T, normalized=False, aabb=s.aabb)
    touched_by_others = torch.zeros(16 * s.T, dtype=torch.bool)
    touched_by_others[keys[~sat].reshape(-1)] = True
    only_saturated = torch.zeros(16 * s.T, dtype=torch.bool)
    only_saturated[keys[sat].reshape(-1)] = True
    only_saturated &= ~touched_by_others
    assert int(only_saturated.sum()) > 1000
    d = g["encoding.hash_table"].cpu()
    assert _all_plus_zero(d[only_saturated])
    assert float(d[touched_by_others].abs().max()) > 0
    assert g["quat_encoding.hash_table"] is None
