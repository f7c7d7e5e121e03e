"""tests/densify_cases.py against the pinned restatement (oracle/densify_oracle.py), on every case tests/test_densify_layout_gpu.py
uses: the rows sit clear of the thresholds that go through exp / sigmoid, each decision takes a sizeable share, every designated
row gets the decision it was built for, and the reference's two-call form equals one pass over the original indices -- what the
fused plan of csrc/densify.hip relies on."""
import functools

import pytest
import torch

import densify_cases as dc
from oracle import densify_oracle as do

LAYOUT_CASES = ([("size", P, seed, 2, True) for P, seed in dc.SIZE_CASES] + [("ns",) + c for c in dc.NS_CASES]
                + [("uniform", P, seed, 2, kind) for P, seed, kind in dc.UNIFORM_CASES])
ALL_CASES = LAYOUT_CASES + [("stats", P, seed, 2, True) for P, seed in dc.STATS_CASES] + [("stride", P, seed, 2, s) for P, seed, s in dc.STRIDE_CASES]
ids = lambda cases: ["-".join(str(x) for x in c) for c in cases]


@functools.lru_cache(maxsize=None)
def build(key):
    what, P, seed, N, extra = key
    if what == "uniform":
        return dc.uniform_case(P, seed, extra)
    if what == "stats":
        return dc.make_case(P, seed, n_views=5, radii_low=-3)
    if what == "stride":
        return dc.make_case(P, seed, grad_stride=extra)
    return dc.make_case(P, seed, N=N, surface=extra)


def equal_with_nans(a, b):
    return a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) \
        and torch.equal(a.isnan(), b.isnan())


@pytest.mark.parametrize("key", ALL_CASES, ids=ids(ALL_CASES))
def test_rows_are_clear_of_the_thresholds_and_every_decision_has_its_share(key):
    case = build(key)
    worst = case.margins.min(1).values
    assert float(worst.min()) >= 1e-5, f"row {int(worst.argmin())} is within {float(worst.min()):.2e} of a threshold: change the seed"
    if key[0] in ("size", "ns") and case.P >= 255:
        pruned, clone, split = dc.two_calls(case, dc.accumulate(case, dc.oracle_state(case)))
        shares = dict(pruned=int(pruned.sum()) / case.P, cloned=int(clone.sum()) / case.P, split=int(split.sum()) / case.P)
        assert min(shares.values()) >= 0.05, shares
    if case.P >= 255:
        assert int(torch.stack([radii <= 0 for radii, _, _ in case.views]).all(0).sum()) >= 1          # points no view sees
    if case.P >= 64 and key[0] != "uniform":
        assert len(case.row_names) >= 24 and case.rows.unique().numel() == len(case.row_names)
        assert {i for i in (0, 255, 256, case.P - 1) if i < case.P} <= set(case.rows.tolist())


@pytest.mark.parametrize("do_prune", [True, False])
@pytest.mark.parametrize("key", LAYOUT_CASES, ids=ids(LAYOUT_CASES))
def test_designated_rows_get_their_decision_and_both_forms_agree(key, do_prune):
    case = build(key)
    st = dc.accumulate(case, dc.oracle_state(case))
    flags, params, m, v = dc.single_pass(case, st, do_prune=do_prune)
    got = dc.flags_of(*dc.two_calls(case, st, do_prune=do_prune))
    want = case.row_flags[0 if do_prune else 1]
    for j, name in enumerate(case.row_names if key[0] != "uniform" else []):
        assert int(got[case.rows[j]]) == int(want[j]), f"designated row '{name}' at {int(case.rows[j])}: flag {int(got[case.rows[j]])}, built for {int(want[j])}"
    assert torch.equal(got[case.rows], want)
    assert torch.equal(flags, got)
    for k in do.PARAMS:
        assert equal_with_nans(st["params"][k], params[k]), k
        assert torch.equal(st["m"][k], m[k]) and torch.equal(st["v"][k], v[k]), k


def test_prune_alone_keeps_the_survivors_in_order():
    case = build(("size", 4099, 16, 2, True))
    st = dc.accumulate(case, dc.oracle_state(case))
    flags, params, m, v = dc.single_pass(case, st, do_prune=True, do_densify=False)
    pruned = do.adaptive_prune(st, case.min_opacity, case.extent)
    assert torch.equal(flags, pruned.to(torch.uint8))
    for k in do.PARAMS:
        assert torch.equal(st["params"][k], params[k]) and torch.equal(st["m"][k], m[k]) and torch.equal(st["v"][k], v[k]), k
