"""tests/optim_ref.py checked without a GPU: the float32 restatement of the Adam update against torch.optim.Adam on the CPU and
against float64, and the row builder of tests/test_optim_gpu.py -- the offsets it promises, guards that survive a round trip and
catch a stray write, rows that do not overlap."""
import numpy as np
import pytest
import torch

import optim_ref as orf


def _grad(gen, n, step):
    """The gradient scaling of test_optim_gpu.py::test_fused_adam_matches_torch_adam."""
    return torch.randn(n, generator=gen) * (10.0 ** ((step % 5) - 2))


@pytest.mark.parametrize("n", [1, 3, 5, 1025, 4099])
def test_float32_restatement_is_torch_adam_on_the_cpu(n):
    gen = torch.Generator().manual_seed(n)
    lr = 1e-2
    p0 = torch.randn(n, generator=gen)
    ref = torch.nn.Parameter(p0.clone())
    tadam = torch.optim.Adam([ref], lr=lr, eps=1e-15)
    z = np.zeros(n, np.float32)
    s32, s64 = (p0.numpy().copy(), z, z), (p0.numpy().astype(np.float64), z.astype(np.float64), z.astype(np.float64))
    gmax = np.zeros(n)
    for step in range(25):
        g = _grad(gen, n, step)
        gmax = np.maximum(gmax, g.abs().numpy())
        ref.grad = g.clone()
        tadam.step()
        s32 = orf.adam_step_f32(s32[0], g.numpy(), s32[1], s32[2], lr, step + 1)
        s64 = orf.adam_step_f64(s64[0], g.numpy(), s64[1], s64[2], lr, step + 1)
        assert all(a.dtype == np.float32 for a in s32) and all(a.dtype == np.float64 for a in s64)
        torch.testing.assert_close(torch.from_numpy(s32[0]), ref.detach(), rtol=3e-5, atol=5e-7, msg=lambda m: f"step {step}: {m}")
    # the moments: exp_avg is a sum of terms of either sign up to the largest gradient seen (a value left by cancellation carries the
    # rounding of its terms: 25 steps x 3 operations x 2^-24 of them, 1e-5 with room), exp_avg_sq a sum of positive terms
    state = tadam.state[ref]
    for m, v in ((s32[1], s32[2]), (state["exp_avg"].numpy(), state["exp_avg_sq"].numpy())):
        assert bool((np.abs(m - s64[1]) <= 1e-5 * gmax).all())
        np.testing.assert_allclose(v, s64[2], rtol=1e-5, atol=0)
    # the value: every step rounds it once (half an ulp, 2^-24 of its size) and adds an update of at most ~lr whose own relative
    # error is a few 2^-24 where exp_avg is well conditioned and, by the bound above, small in absolute terms where it is not
    bound = 25 * 2.0 ** -24 * np.maximum(np.abs(s64[0]), 1.0) + 25 * lr * 1e-5
    for got in (s32[0], ref.detach().numpy()):
        assert bool((np.abs(got - s64[0]) <= bound).all()), float(np.abs(got - s64[0]).max())


def test_restatement_rounds_the_constants_once():
    """1 - beta formed in double and rounded once (float(1 - 0.9) = 0.1, whereas 1.f - 0.9f = 0.100000024); bias corrections of large
    steps are exactly 1."""
    p, m, v = orf.adam_step_f32([1.0], [1.0], [0.0], [0.0], 1.0, 1)
    assert m[0] == np.float32(0.1) and m[0] != np.float32(1.0) - np.float32(0.9)
    assert v[0] == np.float32(1.0 - 0.999)
    for t in (10 ** 6, 2 ** 31 - 1):
        assert orf.bias_corrections(t) == (np.float32(1.0), np.float32(1.0))
    b1, b2 = orf.bias_corrections(1)
    assert b1 == np.float32(1.0 - 0.9) and b2 == np.float32(np.sqrt(1.0 - 0.999))


OFFSETS = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 2, 0, 0), (0, 0, 3, 0), (0, 0, 0, 1), (1, 2, 3, 0), (3, 1, 0, 2)]


@pytest.mark.parametrize("offsets", OFFSETS, ids=[str(o) for o in OFFSETS])
def test_make_rows_places_every_array_at_its_offset_between_guards(offsets):
    rows = orf.make_rows(orf.COUNTS, offsets, guard=8)
    tab = rows.table()
    spans = {k: [] for k in orf.KINDS}
    for r, n in enumerate(rows.counts):
        assert tab[r].count == n and tab[r].lr == np.float32(rows.lr[r])
        for ki, kind in enumerate(orf.KINDS):
            v = rows.view(kind, r)
            assert v.numel() == n and (n == 0 or v.data_ptr() % 16 == 4 * offsets[ki])
            assert getattr(tab[r], kind) == (v.data_ptr() if n else None)
            assert orf.same_bits(v, rows.initial[r][kind])
            s = rows.start[kind][r]
            words = rows.buf[kind].view(torch.int32).numpy().view(np.uint32)
            assert s >= 8 and (words[s - 8:s] == orf.GUARD_BITS).all() and (words[s + n:s + n + 8] == orf.GUARD_BITS).all()
            spans[kind].append((s, s + n))
    for kind, sp in spans.items():                    # rows of one buffer: disjoint, in order, at least a guard apart
        for (a0, a1), (b0, b1) in zip(sp, sp[1:]):
            assert a1 + 8 <= b0, kind
        assert len({b.data_ptr() for b in rows.buf.values()}) == 4
    rows.check_guards()


def test_rows_keep_their_values_wherever_they_are_placed():
    a, b = orf.make_rows(orf.COUNTS), orf.make_rows(orf.COUNTS, (1, 2, 3, 0))
    orf.assert_rows_equal(a, b)
    orf.assert_rows_equal(a, a.reference())
    lrs = {round(x, 9) for x in a.lr}
    assert len(lrs) == len(a.lr)


def test_guards_survive_a_round_trip_and_catch_a_stray_write():
    rows = orf.make_rows((3, 0, 1025), (1, 2, 3, 0), guard=8)
    for kind in orf.KINDS:                            # through a copy and back, as a device round trip does
        rows.buf[kind] = rows.buf[kind].clone().view(torch.int32).contiguous().view(torch.float32)
    rows.check_guards()
    for r in range(3):
        for kind in orf.KINDS:
            rows.view(kind, r).mul_(2.0)              # writing inside the rows is no violation
    rows.check_guards()
    for kind, r, where in (("param", 0, -1), ("exp_avg_sq", 2, 1025), ("grad", 1, 0)):
        rows = orf.make_rows((3, 0, 1025), (1, 2, 3, 0), guard=8)
        rows.buf[kind][rows.start[kind][r] + where] = 1.0
        with pytest.raises(AssertionError, match=kind):
            rows.check_guards()
    # a NaN of another payload is a violation too: the guards are compared as integers
    rows = orf.make_rows((3,), guard=8)
    rows.buf["param"].view(torch.int32)[0] = 0x7FC00000
    with pytest.raises(AssertionError, match="param"):
        rows.check_guards()
    out = orf.GuardedArray(7, torch.float32, "cpu", offset=1)
    assert out.data.data_ptr() % 16 == 4 and out.data.numel() == 7
    out.data.fill_(1.0)
    out.check_guards()
    out.buf[out.at + 7] = 0
    with pytest.raises(AssertionError):
        out.check_guards()


def test_step_reference_updates_the_named_rows_only():
    rows = orf.make_rows((5, 1025))
    state = rows.reference()
    orf.step_reference(state, rows.lr, 1, rows=[1])
    assert orf.same_bits(state[0]["param"], rows.initial[0]["param"]) and not orf.same_bits(state[1]["param"], rows.initial[1]["param"])
    assert orf.same_bits(state[1]["grad"], rows.initial[1]["grad"])
