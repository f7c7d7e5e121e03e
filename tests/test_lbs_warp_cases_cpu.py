"""CPU checks of the skinning warp's edge cases (tests/lbs_warp_cases.py) and of the restatement and comparison rule they are
measured with (tests/lbs_warp_ref.py): the float32 restatement is oracle.lbs_oracle.warp bit for bit, every case is what it says it
is (tie counts, flip counts, tails, joints left out by whole wavefronts, negative zeros), the restatement alone stays inside the bar
under the rule, and the rule still bites when a stand-in takes the wrong row of the candidate table or drops the sign."""
import numpy as np
import pytest
import torch

import lbs_warp_cases as wc
import lbs_warp_ref as wr
from oracle import lbs_oracle as lo

_prepared = {}


def _pairs(name):
    if name not in _prepared:
        _prepared[name] = wr.admitted_pairs(wc.make_case(name))
    return _prepared[name]


@pytest.mark.parametrize("name", ["random", "random_T_off", "scales", "ties_orthogonal", "ties_nonorthogonal", "half_turns", "half_turns_T",
                                  "joints_J9_P257", "joints_J64_P65"])
def test_float32_restatement_is_the_oracle_bit_for_bit(name):
    c = wc.make_case(name)
    leaves = lambda: [c[k].clone().requires_grad_(True) if c[k] is not None else None for k in ("xyz", "rot", "offsets")]
    a, b = leaves(), leaves()
    p0, q0, mat0 = lo.warp(a[0], a[1], c["weights"], c["mats"], a[2], c["T"])
    p1, q1, _ = wr.warp(b[0], b[1], c["weights"], c["mats"], b[2], c["T"])
    assert torch.equal(p0, p1) and torch.equal(q0, q1)
    for p, q in ((p0, q0), (p1, q1)):
        ((p * c["gp"]).sum() + (q * c["gq"]).sum()).backward()
    for x, y in zip(a, b):
        assert x is None or torch.equal(x.grad, y.grad)
    # ... and the per-point-matrix form is the same computation
    p2, q2, _ = wr.warp(c["xyz"], c["rot"], None, mat0[0], c["offsets"], c["T"])
    assert torch.equal(p2, p0.detach()) and torch.equal(q2, q0.detach())


@pytest.mark.parametrize("name", ["random", "random_T", "random_T_off"])
def test_random_scene_spreads_over_the_branches_and_meets_no_tie_or_flip(name):
    c = wc.make_case(name)
    nat, _, ok = _pairs(name)
    counts = np.bincount(nat["branch"], minlength=4)
    print(name, "branches", counts.tolist())
    assert c["xyz"].shape == (3000, 3) and c["weights"].shape == (3000, 55)
    assert (counts >= 600).all() and int((ok.sum(0) > 1).sum()) == 0
    n = c["rot"].norm(dim=1)
    assert 0.5 <= float(n.min()) < 0.55 and 1.45 < float(n.max()) <= 1.5 + 1e-6


def test_scales_span_six_decades():
    c = wc.make_case("scales")
    n = c["rot"].double().norm(dim=1)
    assert float(n.min()) < 2e-3 and float(n.max()) > 500 and float(n.min()) >= 0.99e-3 and float(n.max()) <= 1.01e3
    _, _, ok = _pairs("scales")
    assert int((ok.sum(0) > 1).sum()) <= wr.MULTI_CAP * n.numel()


def _f32_q_abs(c):
    return wr.warp(c["xyz"], c["rot"], c["weights"], c["mats"], c["offsets"], c["T"])[2]["q_abs"].numpy()


def test_orthogonal_ties_are_ties():
    c = wc.make_case("ties_orthogonal")
    kinds, eps, exact = np.array(c["kinds"]), c["eps"], c["exact"]
    assert c["rot"].shape[0] == 640 and sorted(set(kinds)) == ["four", "two", "two_third"] and int(exact.sum()) == 4 * 16
    assert sorted(set(eps.tolist())) == sorted(wc.PERTURBATIONS)
    qa = np.sort(_f32_q_abs(c), 1)[:, ::-1]
    # float32, unperturbed: all four q_abs are 1 (every operation exact), or the two largest are the same rounded sqrt(2)
    two = (kinds == "two") & (eps == 0)
    assert (qa[exact] == 1.0).all() and int(two.sum()) == 4 * 12
    assert (qa[two][:, 0] == qa[two][:, 1]).all() and (qa[two][:, 0] == np.sqrt(np.float32(2))).all() and (qa[two][:, 2] == 0).all()
    _, _, ok = _pairs("ties_orthogonal")
    branches = ok[0::2].sum(0)
    small = eps <= 1e-6
    assert (branches[small & (kinds == "four")] == 4).all() and (branches[small & (kinds != "four")] == 2).all()
    print("orthogonal ties: admitted branches per point", np.bincount(branches).tolist(), "flip candidates", int(ok[1::2].any(0).sum()))
    assert (branches >= 1).all() and int((branches > 1).sum()) >= 480


def test_nonorthogonal_ties_change_the_answer():
    c = wc.make_case("ties_nonorthogonal")
    exact = c["exact"]
    assert c["rot"].shape[0] == 512 and int(exact.sum()) == 128
    w8 = c["weights"] * 8
    assert torch.equal(w8, w8.round()) and (w8 >= 0).all() and torch.equal(w8.sum(1), torch.full((512,), 8.0))
    m32 = torch.einsum("nj,jxy->nxy", c["weights"], c["mats"])
    m64 = torch.einsum("nj,jxy->nxy", c["weights"].double(), c["mats"].double())
    assert torch.equal(m32.double(), m64) and (m64[:, :3, :3] == torch.diag_embed(torch.diagonal(m64[:, :3, :3], dim1=1, dim2=2))).all()
    assert (_f32_q_abs(c)[exact] == 1.0).all()                     # R' has a zero diagonal: every xs is 1
    _, runs, ok = _pairs("ties_nonorthogonal")
    assert (ok[0::2].sum(0)[exact] == 4).all()
    # the rows of the table are different quaternions here: a wrong tie rule is an error of order 1
    d = np.abs(runs[0]["q"] - runs[2]["q"]).max(1)
    d = np.minimum(d, np.abs(runs[0]["q"] + runs[2]["q"]).max(1))
    print("non-orthogonal ties: |q(row 0) - +-q(row 1)| median", float(np.median(d[exact])), "max", float(d[exact].max()))
    assert float(np.median(d[exact])) > 0.05 and float(d[exact].max()) > 0.5


@pytest.mark.parametrize("name", ["half_turns", "half_turns_T"])
def test_half_turns_are_flip_candidates(name):
    c = wc.make_case(name)
    nat, _, ok = _pairs(name)
    assert c["rot"].shape[0] == 256 and (c["T"] is not None) == name.endswith("_T")
    assert ok[1::2].any(0).all()                                    # every point admits the other sign
    assert float(np.abs(nat["real"]).max()) <= 1e-5
    if name == "half_turns":
        r = c["rot"][:, 0]
        assert int((r == 0).sum()) == 64 and int((r > 0).sum()) >= 64 and int((r < 0).sum()) >= 64
        assert torch.equal(c["rot"][:6, 1:], torch.tensor([[1., 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1]]))


@pytest.mark.parametrize("J", wc.JOINT_COUNTS)
def test_joint_count_cases(J):
    for P in wc.POINT_COUNTS:
        c = wc.make_case(f"joints_J{J}_P{P}")
        w = c["weights"]
        assert w.shape == (P, J) and c["mats"].shape == (J, 4, 4)
        used = w != 0
        nnz = used.sum(1)
        assert int(nnz.min()) >= 1 and int(nnz.max()) <= 4 and torch.allclose(w.sum(1), torch.ones(P), atol=1e-6)
        if J > 1:
            assert int(((w == 0) & torch.signbit(w)).sum()) >= 1                 # some of the zeros are -0.0
        det = torch.linalg.det(c["mats"][:, :3, :3]).abs() ** (1 / 3)
        assert 0.5 <= float(det.min()) and float(det.max()) <= 1.5 and (J < 7 or float(det.max() - det.min()) > 0.2)
        if J >= 3:
            waves = [used[s:s + 64].any(0) for s in range(0, P, 64)]
            for v, u in enumerate(waves):
                left_out = ~u
                assert left_out.any(), (J, P, v)                                 # a joint NO point of this wavefront follows ...
                if len(waves) > 1 and P >= 255:
                    others = torch.stack([x for k, x in enumerate(waves) if k != v]).any(0)
                    assert (left_out & others).any(), (J, P, v)                  # ... and points of another wavefront do
        _, _, ok = wr.admitted_pairs(c)
        assert int((ok.sum(0) > 1).sum()) <= wr.MULTI_CAP * P, (J, P)


def test_tail_shapes_reach_every_remainder():
    tails = [(min(64, P - 64 * ((P - 1) // 64)) * J) % 4 for J, P in wc.TAIL_SHAPES]
    assert tails == [3, 2, 1, 0, 1, 2, 3, 0]
    assert wc.TAIL_FRAMES == (1, 4, 5, 9) and wc.TAIL_EXTRAS == ((3, 1), (5, 4), (7, 1))
    t = wc.tail_case(55, 66, 5)
    assert t["weights"].shape == (66, 55) and t["mats"].shape == (5, 55, 4, 4) and [e.shape[2] for e in t["extras"][1]] == [5, 4]
    assert torch.allclose(t["weights"].sum(1), torch.ones(66), atol=1e-6)


@pytest.mark.parametrize("name", ["random_T_off", "scales", "ties_orthogonal", "ties_nonorthogonal", "half_turns", "half_turns_T"])
def test_the_restatement_alone_passes_under_the_rule(name):
    """torch float32 standing in for the kernel: a naive comparison is off by order 1 on the tie and flip cases, under the rule the
    restatement is within 1e-5 of float64"""
    c = wc.make_case(name)
    f32 = wr.run(c, torch.float32)
    nat = _pairs(name)[0]
    naive = float(np.abs(f32["q"] - nat["q"]).max())
    lines = wr.compare(name, f32, c, _pairs(name))
    print(name, "naive worst |dq|", naive)
    errs, _ = wr.rule_errors(c, f32, *_pairs(name))
    assert max(errs.values()) <= 1e-5, errs


def test_tensors_off_the_16_byte_grid_go_to_the_kernels_as_aligned_copies():
    """lbs._f32 (what every tensor passes on its way to the warp's entry points): a contiguous view at a 4-byte storage offset
    comes back as an equal, aligned copy; an aligned tensor comes back as it is"""
    from soar_amd import lbs
    buf = torch.arange(4 * 37 + 3, dtype=torch.float32)
    for shift in (1, 2, 3):
        v = buf[shift:shift + 4 * 37].view(37, 4)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4 * shift
        a = lbs._f32(v)
        assert a.data_ptr() % 16 == 0 and a.is_contiguous() and torch.equal(a, v) and a.data_ptr() != v.data_ptr()
    aligned = buf[:16].view(4, 4)
    assert lbs._f32(aligned).data_ptr() == aligned.data_ptr()
    assert lbs._f32(buf[4:20].view(4, 4)).data_ptr() == buf.data_ptr() + 16           # an offset ON the grid needs no copy
    assert lbs._f32(torch.empty(0, 4)).shape == (0, 4)


def test_the_rule_bites():
    # on an exact tie any row of the table is admitted, but not one row forward and another backward
    c = wc.make_case("ties_nonorthogonal")
    P = c["rot"].shape[0]
    f32 = wr.run(c, torch.float32)
    row1 = wr.run(c, torch.float32, branch=torch.ones(P, dtype=torch.int64))
    exact = c["exact"][:, None]
    assert (f32["branch"][c["exact"]] == 0).all()                 # argmax takes the first of equal rows
    wr.compare("row 1 on the exact ties", {k: np.where(exact, row1[k], f32[k]) for k in ("p", "q", "dxyz", "drot")}, c,
               _pairs("ties_nonorthogonal"))
    with pytest.raises(AssertionError):
        wr.compare("rows mixed", dict(f32, drot=np.where(exact, row1["drot"], f32["drot"])), c, _pairs("ties_nonorthogonal"))
    # forward with one pair, backward with another: the gradient without the standardisation's sign
    c = wc.make_case("half_turns")
    f32 = wr.run(c, torch.float32)
    flipped = wr.run(c, torch.float32, sign=torch.from_numpy(-np.where(f32["real"] < 0, -1.0, 1.0)))
    mixed = dict(f32, drot=flipped["drot"])
    with pytest.raises(AssertionError):
        wr.compare("mixed pairs", mixed, c, _pairs("half_turns"))
    # a wrong branch on a point that is no tie
    c = wc.make_case("random")
    f32 = wr.run(c, torch.float32)
    other = wr.run(c, torch.float32, branch=torch.from_numpy((f32["branch"] + 1) % 4))
    bad = {k: np.where(np.arange(3000)[:, None] == 17, other[k], f32[k]) for k in ("p", "q", "dxyz", "drot")}
    with pytest.raises(AssertionError):
        wr.compare("one wrong branch", bad, c, _pairs("random"))
