"""GPU tests of the skinning warp (csrc/lbs.hip, soar_amd/lbs.py) at its edges, against the float64 restatement of
tests/lbs_warp_ref.py under its comparison rule and the project's bar (HIP at most 4 x the float32 restatement's own distance from
float64, floor 1e-6, the restatement capped at 1e-4; tie window 1e-5): ties of matrix_to_quaternion's candidate table under
orthogonal and non-orthogonal transforms, half turns, quaternion scales, joint counts 1 .. 64 with joints that whole wavefronts
leave out, the gradient of the offsets, the per-point-matrix form, soar_lbs_warp_backward_views, the row tails of the all-frames
kernels, row independence, repeatability and inputs that start off the 16-byte grid.  The cases: tests/lbs_warp_cases.py.

Measured on an MI355X (worst element over the largest magnitude of the float64 tensor, under the rule; HIP / the float32 restatement;
dL/drot rows times |q|; the bar is 4 x the second figure, floor 1e-6):
  case                 positions           quaternions         dL/dxyz             dL/drot             several pairs / other pair
  random               1.4e-07 / 1.4e-07   1.4e-07 / 1.6e-07   1.0e-07 / 1.0e-07   2.3e-07 / 2.2e-07   0 of 3000 / 0
  random_T (and _off)  1.4e-07 / 1.4e-07   1.4e-07 / 1.8e-07   1.6e-07 / 1.6e-07   3.2e-07 / 2.7e-07   0 of 3000 / 0
  scales               1.4e-07 / 1.4e-07   1.8e-07 / 1.8e-07   9.3e-08 / 1.0e-07   2.0e-07 / 2.2e-07   0 of 3000 / 0
  ties_orthogonal      0 / 0               2.7e-07 / 3.1e-07   0 / 0               2.3e-07 / 2.6e-07   624 of 640 / 298
  ties_nonorthogonal   2.2e-08 / 2.2e-08   1.6e-07 / 1.8e-07   2.3e-08 / 2.3e-08   2.7e-07 / 2.8e-07   512 of 512 / 83
  half_turns           0 / 0               1.3e-07 / 1.1e-07   0 / 0               1.7e-07 / 1.3e-07   256 of 256 / 4
  half_turns_T         0 / 0               1.0e-07 / 9.5e-08   0 / 0               2.0e-07 / 1.8e-07   256 of 256 / 45
  joints J = 1         1.5e-07 / 1.5e-07   1.4e-07 / 1.6e-07   6.3e-08 / 8.8e-08   3.0e-07 / 3.6e-07   0 (worst of P = 63 .. 257, also below)
  joints J = 7         1.1e-07 / 1.1e-07   1.4e-07 / 1.9e-07   7.0e-08 / 9.9e-08   3.7e-07 / 4.7e-07   0
  joints J = 8         7.9e-08 / 7.9e-08   1.8e-07 / 1.5e-07   9.8e-08 / 1.1e-07   2.9e-07 / 2.6e-07   0
  joints J = 9         1.1e-07 / 1.1e-07   1.3e-07 / 1.5e-07   1.1e-07 / 1.1e-07   2.3e-07 / 3.1e-07   0
  joints J = 16        8.5e-08 / 6.6e-08   1.7e-07 / 1.3e-07   1.3e-07 / 1.3e-07   3.6e-07 / 2.4e-07   0
  joints J = 55        1.1e-07 / 9.6e-08   1.4e-07 / 1.6e-07   5.9e-08 / 6.2e-08   2.7e-07 / 3.1e-07   0
  joints J = 64        7.9e-08 / 7.9e-08   1.2e-07 / 1.7e-07   8.6e-08 / 1.0e-07   2.7e-07 / 3.9e-07   0
"several pairs": points at which the rule admits more than one (branch, sign) pair; "other pair": of those, the points at which the
kernel's result is closest to another pair than float64's own.  Compared naively, the tie and half-turn cases are off by 1.1 to 2.0
(q against -q, or another row of the table).  The exact rows (64 of ties_orthogonal, 128 of ties_nonorthogonal) are bit-equal to the
float32 restatement: the kernel takes the first maximal row.  offsets.grad is exact (0 / 0) with and without T: T permutes axes.
J = 64: the single-frame launches with 65536 bytes of dynamic LDS succeed and meet the bar like every other joint count.
"""
import numpy as np
import pytest
import torch

import lbs_warp_cases as wc
import lbs_warp_ref as wr
from body_ref import bar_check

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_prepared = {}


def _dev(t, grad=False):
    return None if t is None else t.to(DEV).requires_grad_(grad)


def _hip(c, offsets_grad=True, per_point=False):
    """one forward and backward through lbs.lbs_warp with the case's upstream gradients -> dict of float32 numpy arrays"""
    from soar_amd import lbs
    xyz, rot = _dev(c["xyz"], True), _dev(c["rot"], True)
    off = _dev(c["offsets"], offsets_grad)
    w, A, T = _dev(c["weights"]), _dev(c["mats"]), _dev(c["T"])
    if per_point:
        w, A = None, lbs.point_transforms(xyz, rot, w, A)
    p, q = lbs.lbs_warp(xyz, rot, w, A, off, T)
    ((p * c["gp"].to(DEV)).sum() + (q * c["gq"].to(DEV)).sum()).backward()
    n = lambda t: t.detach().cpu().numpy()
    return {"p": n(p), "q": n(q), "dxyz": n(xyz.grad), "drot": n(rot.grad), "doff": n(off.grad) if off is not None and offsets_grad else None}


def _bar(name):
    c = wc.make_case(name)
    if name not in _prepared:
        _prepared[name] = wr.admitted_pairs(c)
    got = _hip(c)
    wr.compare(name, got, c, _prepared[name])
    return c, got


@pytest.mark.parametrize("name", [n for n in wc.BAR_CASES if not n.startswith("joints_")])
def test_warp_meets_the_bar_under_the_rule(name):
    c, got = _bar(name)
    if "exact" in c:
        # an exact tie in exact arithmetic: the kernel takes the FIRST maximal row of the table, as argmax does
        f32 = wr.run(c, torch.float32)
        e = c["exact"]
        same = (got["q"][e] == f32["q"][e].astype(np.float32)).all(1)
        print(f"{name}: {int(same.sum())} of {int(e.sum())} exact rows bit-equal to the float32 restatement")
        assert same.all(), (name, np.flatnonzero(e)[~same][:8], got["q"][e][~same][:4], f32["q"][e][~same][:4])


@pytest.mark.parametrize("J", wc.JOINT_COUNTS)
def test_joint_counts_meet_the_bar(J):
    """J = 64 asks the single-frame kernels for 64 KB of dynamic LDS, the most a launch gets without an opt-in"""
    for P in wc.POINT_COUNTS:
        _bar(f"joints_J{J}_P{P}")


def test_joint_counts_outside_the_range_are_refused():
    """J = 65 through lbs.lbs_warp, and J = 65 and 0 with weights through the C entry points (tests/test_abi_cpu.py asks the same of
    every entry point without a device): refused with the existing message, nothing launched, nothing written"""
    from soar_amd import hip_lib, lbs
    L, ptr = hip_lib.lib(), hip_lib.ptr
    c = wc.make_case("joints_J9_P65")
    xyz, rot = _dev(c["xyz"]), _dev(c["rot"])
    with pytest.raises(RuntimeError, match="bad sizes P=65 J=65"):
        lbs.lbs_warp(xyz, rot, torch.zeros(65, 65, device=DEV), torch.zeros(65, 4, 4, device=DEV))
    w, A = torch.zeros(65, 65, device=DEV), torch.zeros(65, 4, 4, device=DEV)
    p, q = torch.full((65, 3), 7.0, device=DEV), torch.full((65, 4), 7.0, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for J in (65, 0):
        assert L.soar_lbs_warp_forward(ptr(xyz), ptr(rot), ptr(w), ptr(A), None, None, 65, J, ptr(p), ptr(q), None, stream) != 0
        assert f"bad sizes P=65 J={J} (max J 64)" in hip_lib.last_error()
    torch.cuda.synchronize()
    assert bool((p == 7.0).all()) and bool((q == 7.0).all())


@pytest.mark.parametrize("use_T", [False, True])
def test_offsets_gradient(use_T):
    c = dict(wc.make_case("random_T_off"))
    if not use_T:
        c["T"] = None
    got = _hip(c)
    f64, f32 = wr.run(c, torch.float64), wr.run(c, torch.float32)
    bar_check(f"offsets.grad T={use_T}", got["doff"], f32["doff"], f64["doff"])
    # the offsets shift the position behind the blend: without them only the positions change, by the offsets under T
    without = _hip(dict(c, offsets=None))
    assert np.array_equal(without["q"], got["q"]) and np.array_equal(without["drot"], got["drot"]) and np.array_equal(without["dxyz"], got["dxyz"])


@pytest.mark.parametrize("P", [1, 255, 257])
def test_per_point_matrices_are_the_blend(P):
    """lbs_warp(xyz, rot, None, point_transforms(...)) -- the kernels' weights == NULL path, float4 loads of [P,4,4] -- is
    lbs_warp(xyz, rot, weights, joint_mats) bit for bit, forward and backward, with offsets and T"""
    from soar_amd import lbs
    full = wc.make_case("joints_J55_P257")
    sc = wc.make_case("random_T_off")
    c = {k: (full[k][:P].contiguous() if k in ("xyz", "rot", "weights", "gp", "gq") else full[k]) for k in full}
    c["offsets"], c["T"] = sc["offsets"][:P].contiguous(), sc["T"]
    a, b = _hip(c), _hip(c, per_point=True)
    for k in ("p", "q", "dxyz", "drot", "doff"):
        assert np.array_equal(a[k], b[k]) and np.isfinite(a[k]).all(), (P, k)
    xyz, rot, w, A = _dev(c["xyz"]), _dev(c["rot"]), _dev(c["weights"]), _dev(c["mats"])
    mats = lbs.point_transforms(xyz, rot, w, A)
    assert mats.shape == (P, 4, 4)
    with pytest.raises(ValueError, match="per-point matrices must be"):
        lbs.lbs_warp(xyz, rot, None, torch.cat([mats, mats[:1]]))
    with pytest.raises(ValueError, match="weights must be"):
        lbs.lbs_warp(xyz, rot, w[:, :-1], A)


def _extra_blocks(extras, P):
    sums = [torch.full((P, e.shape[2]), float("nan"), device=DEV) for e in extras]
    src = torch.tensor([e.data_ptr() for e in extras], dtype=torch.int64)
    dst = torch.tensor([e.data_ptr() for e in sums], dtype=torch.int64)
    width = torch.tensor([e.shape[2] for e in extras], dtype=torch.int32)
    return sums, src, dst, width


def _frame_order_sum(e):
    want = e[0].clone()
    for f in range(1, e.shape[0]):
        want = want + e[f]
    return want


@pytest.mark.parametrize("n", [1, 4, 6])
def test_backward_over_the_views_of_one_pose(n):
    """soar_lbs_warp_backward_views (one set of joint transforms, an axis permutation, two extra blocks) == the sum in view order of
    soar_lbs_warp_backward with the same T, bit for bit"""
    from soar_amd import hip_lib
    L, ptr = hip_lib.lib(), hip_lib.ptr
    c = wc.make_case("joints_J55_P257")
    P, J = c["weights"].shape
    g = torch.Generator().manual_seed(70 + n)
    xyz, rot, w, A = (c[k].to(DEV).contiguous() for k in ("xyz", "rot", "weights", "mats"))
    T = wc.make_case("random_T")["T"].to(DEV).contiguous()
    g_p, g_q = torch.randn(n, P, 3, generator=g).to(DEV), torch.randn(n, P, 4, generator=g).to(DEV)
    extras = [torch.randn(n, P, wd, generator=g).to(DEV) for wd in ((5, 4) if n != 4 else (7, 1))]
    sums, src, dst, width = _extra_blocks(extras, P)
    stream = torch.cuda.current_stream().cuda_stream
    d_p, d_q = torch.full((P, 3), float("nan"), device=DEV), torch.full((P, 4), float("nan"), device=DEV)
    assert L.soar_lbs_warp_backward_views(ptr(xyz), ptr(rot), ptr(w), ptr(A), ptr(T), n, P, J, ptr(g_p), ptr(g_q), ptr(d_p), ptr(d_q), 2,
                                          src.data_ptr(), dst.data_ptr(), width.data_ptr(), stream) == 0, hip_lib.last_error()
    want_p, want_q = torch.zeros(P, 3, device=DEV), torch.zeros(P, 4, device=DEV)
    for f in range(n):
        dp_f, dq_f = torch.empty(P, 3, device=DEV), torch.empty(P, 4, device=DEV)
        assert L.soar_lbs_warp_backward(ptr(xyz), ptr(rot), ptr(w), ptr(A), ptr(T), P, J, ptr(g_p[f]), ptr(g_q[f]), ptr(dp_f), ptr(dq_f),
                                        stream) == 0
        want_p, want_q = want_p + dp_f, want_q + dq_f
    torch.cuda.synchronize()
    assert torch.equal(d_p, want_p) and torch.equal(d_q, want_q) and torch.isfinite(d_q).all()
    for e, got in zip(extras, sums):
        assert torch.equal(got, _frame_order_sum(e))


@pytest.mark.parametrize("J,P", wc.TAIL_SHAPES)
def test_row_tails_of_the_all_frames_kernels(J, P):
    """rows * J mod 4 = 3, 2, 1, 0 floats behind the float4 copies of the last workgroup's weight rows; extra blocks of widths that
    fill one group of four columns, spill into a second, or neither: bit for bit the per-frame entry points"""
    from soar_amd import hip_lib
    L, ptr = hip_lib.lib(), hip_lib.ptr
    stream = torch.cuda.current_stream().cuda_stream
    for n in wc.TAIL_FRAMES:
        t = wc.tail_case(J, P, n)
        xyz, rot, w, mats, g_p, g_q = (t[k].to(DEV).contiguous() for k in ("xyz", "rot", "weights", "mats", "gp", "gq"))
        p_all, q_all = torch.full((n, P, 3), float("nan"), device=DEV), torch.full((n, P, 4), float("nan"), device=DEV)
        assert L.soar_lbs_warp_forward_batch(ptr(xyz), ptr(rot), ptr(w), ptr(mats), n, P, J, ptr(p_all), ptr(q_all), stream) == 0
        want_p, want_q = torch.zeros(P, 3, device=DEV), torch.zeros(P, 4, device=DEV)
        for f in range(n):
            p_f, q_f, dp_f, dq_f = (torch.empty(P, k, device=DEV) for k in (3, 4, 3, 4))
            assert L.soar_lbs_warp_forward(ptr(xyz), ptr(rot), ptr(w), ptr(mats[f]), None, None, P, J, ptr(p_f), ptr(q_f), None, stream) == 0
            assert torch.equal(p_all[f], p_f) and torch.equal(q_all[f], q_f) and torch.isfinite(q_f).all(), (n, f)
            assert L.soar_lbs_warp_backward(ptr(xyz), ptr(rot), ptr(w), ptr(mats[f]), None, P, J, ptr(g_p[f]), ptr(g_q[f]), ptr(dp_f),
                                            ptr(dq_f), stream) == 0
            want_p, want_q = want_p + dp_f, want_q + dq_f
        for pair in t["extras"]:
            extras = [e.to(DEV) for e in pair]
            sums, src, dst, width = _extra_blocks(extras, P)
            d_p, d_q = torch.full((P, 3), float("nan"), device=DEV), torch.full((P, 4), float("nan"), device=DEV)
            assert L.soar_lbs_warp_backward_sum(ptr(xyz), ptr(rot), ptr(w), ptr(mats), n, P, J, ptr(g_p), ptr(g_q), ptr(d_p), ptr(d_q), 2,
                                                src.data_ptr(), dst.data_ptr(), width.data_ptr(), stream) == 0
            torch.cuda.synchronize()
            assert torch.equal(d_p, want_p) and torch.equal(d_q, want_q), (n, [e.shape[2] for e in extras])
            for e, got in zip(extras, sums):
                assert torch.equal(got, _frame_order_sum(e)), (n, e.shape[2])


def test_rows_do_not_see_each_other():
    """a zero or NaN quaternion spoils its own row and no other: single-frame and all-frames, forward and backward"""
    from soar_amd import hip_lib
    L, ptr = hip_lib.lib(), hip_lib.ptr
    c = wc.make_case("joints_J55_P257")
    bad = [0, 63, 64, 130, 256]
    spoiled = dict(c, rot=c["rot"].clone())
    spoiled["rot"][bad[0]] = 0.0
    spoiled["rot"][bad[1]] = float("nan")
    spoiled["rot"][bad[2], 2] = float("nan")
    spoiled["rot"][bad[3]] = 0.0
    spoiled["rot"][bad[4], 0] = float("nan")
    keep = np.ones(257, bool)
    keep[bad] = False
    a, b = _hip(c), _hip(spoiled)
    assert (~np.isfinite(b["q"][bad])).any(1).all() and (~np.isfinite(b["drot"][bad])).any(1).all()
    for k in ("p", "q", "dxyz", "drot"):
        assert np.array_equal(a[k][keep], b[k][keep]) and np.isfinite(a[k]).all(), k
    assert np.array_equal(a["p"], b["p"])                          # positions do not read the quaternion
    # all frames in one launch
    n, P, J = 2, 257, 55
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(9)
    mats = torch.stack([c["mats"], c["mats"].flip(0)]).to(DEV).contiguous()
    g_p, g_q = torch.randn(n, P, 3, generator=g).to(DEV), torch.randn(n, P, 4, generator=g).to(DEV)
    outs = []
    for case in (c, spoiled):
        xyz, rot, w = (case[k].to(DEV).contiguous() for k in ("xyz", "rot", "weights"))
        p_all, q_all = torch.empty(n, P, 3, device=DEV), torch.empty(n, P, 4, device=DEV)
        d_p, d_q = torch.empty(P, 3, device=DEV), torch.empty(P, 4, device=DEV)
        assert L.soar_lbs_warp_forward_batch(ptr(xyz), ptr(rot), ptr(w), ptr(mats), n, P, J, ptr(p_all), ptr(q_all), stream) == 0
        assert L.soar_lbs_warp_backward_sum(ptr(xyz), ptr(rot), ptr(w), ptr(mats), n, P, J, ptr(g_p), ptr(g_q), ptr(d_p), ptr(d_q), 0, None,
                                            None, None, stream) == 0
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy() for t in (q_all, d_p, d_q)])
    (q0, dp0, dq0), (q1, dp1, dq1) = outs
    assert (~np.isfinite(q1[:, bad])).any(2).all() and np.isfinite(q0).all() and np.isfinite(dq0).all()
    assert np.array_equal(q0[:, keep], q1[:, keep]) and np.array_equal(dp0[keep], dp1[keep]) and np.array_equal(dq0[keep], dq1[keep])


def test_two_runs_are_bit_equal():
    for name in ("random_T_off", "ties_nonorthogonal", "joints_J64_P257"):
        c = wc.make_case(name)
        a, b = _hip(c), _hip(c)
        for k in ("p", "q", "dxyz", "drot"):
            assert np.array_equal(a[k], b[k]), (name, k)


def test_inputs_off_the_16_byte_grid_equal_their_aligned_clones():
    """a contiguous rot, or [P,4,4], that is a view at a 4-byte storage offset: lbs.lbs_warp hands the kernels (which read both as
    float4) an aligned copy, and the results are those of the aligned clone"""
    from soar_amd import lbs
    c = wc.make_case("joints_J55_P257")
    P = 257

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        assert lbs._f32(v).data_ptr() % 16 == 0 and torch.equal(lbs._f32(v), v)       # what the kernels are handed
        return v

    xyz, w, A = _dev(c["xyz"]), _dev(c["weights"]), _dev(c["mats"])
    gp, gq = c["gp"].to(DEV), c["gq"].to(DEV)
    mats = lbs.point_transforms(xyz, _dev(c["rot"]), w, A)
    outs = []
    for rot_in, mats_in in ((_dev(c["rot"]), mats.clone()), (shifted(_dev(c["rot"])), shifted(mats))):
        for ww, AA in ((w, A), (None, mats_in)):
            x, r = xyz.clone().requires_grad_(True), rot_in.detach().requires_grad_(True)
            p, q = lbs.lbs_warp(x, r, ww, AA)
            ((p * gp).sum() + (q * gq).sum()).backward()
            outs.append((p.detach(), q.detach(), x.grad, r.grad))
    for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):
        for s, t in zip(a, b):
            assert torch.equal(s, t) and torch.isfinite(s).all()
    assert outs[3][3].shape == (P, 4)
