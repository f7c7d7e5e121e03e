"""csrc/densify.hip and soar_amd/densify.py against the pinned restatement (oracle/densify_oracle.py) run on the CPU in the same
test, on the seeded cases of tests/densify_cases.py: row layout across workgroup and scan-block boundaries, every threshold hit on
purpose, N != 2, surface off, uniform decisions, the 21-bit counters at their limit, the statistics kernel's strides and negative
radii, the split noise's sources, and the optimizer surgery.

Bars (those of test_densify_gpu.py): flags, counts, moments, every tensor but xyz / scaling and every kept or cloned row bit-equal;
split children of xyz and scaling (expf / logf on the device against torch's CPU exp / log) rtol 2e-6, atol 2e-7; statistics
rtol 2e-6, atol 1e-12 with denom and max_radii2D bit-equal.  Each test prints its largest child error as a fraction of that bar."""
import copy
import ctypes as C

import pytest
import torch
from torch import nn

import densify_cases as dc
from oracle import densify_oracle as do

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHILD = dict(rtol=2e-6, atol=2e-7)


# ---- comparison helpers ----------------------------------------------------------------------------------------------------------
def assert_rows(got, want, name, first_row=0, rtol=0.0, atol=0.0):
    """got == want (NaNs in the same places count as equal), or within atol + rtol |want|; names the first row that is not.
    Returns the largest error as a fraction of the bar (0 for the bit-equal form)."""
    got = got.detach().to(want.device)
    assert got.shape == want.shape, f"{name}: shape {tuple(got.shape)}, expected {tuple(want.shape)}"
    if got.numel() == 0:
        return 0.0
    both_nan = got.isnan() & want.isnan()
    exact = rtol == 0.0 and atol == 0.0
    err = (got.double() - want.double()).abs()
    bar = atol + rtol * want.double().abs()
    bad = ~(((got == want) if exact else (err <= bar)) | both_nan)
    if bool(bad.any()):
        rows = bad.reshape(bad.shape[0], -1).any(1)
        r = int(torch.nonzero(rows)[0])
        raise AssertionError(f"{name}: row {first_row + r} differs ({int(rows.sum())} of {rows.numel()} rows do): "
                             f"got {got[r].flatten().tolist()}, expected {want[r].flatten().tolist()}")
    if exact:
        return 0.0
    frac = torch.where(both_nan | (err == 0), torch.zeros_like(err), err / bar)
    return float(frac.max())


def assert_flags(got, want, case, what):
    got = got.cpu()
    bad = torch.nonzero(got != want)[:, 0]
    if bad.numel():
        i = int(bad[0])
        hit = torch.nonzero(case.rows == i)[:, 0]
        name = f" (designated row '{case.row_names[int(hit[0])]}')" if hit.numel() else ""
        raise AssertionError(f"{what}: flags differ at row {i}{name}: got {int(got[i])}, expected {int(want[i])} ({bad.numel()} rows differ)")


def densifier(case, keys=do.PARAMS, extra_groups=()):
    """keys: the tensors the Adam holds state for (None: no optimizer)."""
    from soar_amd.densify import SurfelDensifier
    params = {k: nn.Parameter(case.params[k].clone().to(DEV)) for k in do.PARAMS}
    opt = None
    if keys is not None:
        opt = torch.optim.Adam([{"params": [params[k]], "lr": 1e-3, "name": k} for k in do.PARAMS] + list(extra_groups), lr=0.0, eps=1e-15)
        for k in keys:
            opt.state[params[k]] = {"step": torch.tensor(1.0), "exp_avg": case.m[k].clone().to(DEV), "exp_avg_sq": case.v[k].clone().to(DEV)}
    return SurfelDensifier(params, opt, percent_dense=case.percent_dense, surface=case.surface)


def compare_model(d, st, n_child, tag, keys=do.PARAMS):
    """The densifier's model and optimizer against the oracle's state, row for row; the last n_child rows are split children."""
    head = st["params"]["xyz"].shape[0] - n_child
    worst = {}
    for k in do.PARAMS:
        got, want = d.params[k].detach().cpu(), st["params"][k]
        assert got.shape == want.shape, f"{tag}: {k} has shape {tuple(got.shape)}, expected {tuple(want.shape)}"
        if k in ("xyz", "scaling"):
            assert_rows(got[:head], want[:head], f"{tag}: {k} (kept and cloned rows)")
            worst[k] = assert_rows(got[head:], want[head:], f"{tag}: {k} (split children)", first_row=head, **CHILD)
        else:
            assert_rows(got, want, f"{tag}: {k}")
        if d.optimizer is None:
            continue
        assert d._group(k)["params"][0] is d.params[k], f"{tag}: the optimizer's group {k} does not hold the new tensor"
        state = d.optimizer.state.get(d.params[k])
        if keys is not None and k in keys:
            assert_rows(state["exp_avg"], st["m"][k], f"{tag}: exp_avg of {k}")
            assert_rows(state["exp_avg_sq"], st["v"][k], f"{tag}: exp_avg_sq of {k}")
        else:
            assert not state, f"{tag}: {k} had no optimizer state and now has {sorted(state)}"
    assert d.accum.shape == (5, d.num_points) and d.max_radii2D.shape == (d.num_points,)
    assert float(d.accum.abs().sum()) == 0 and float(d.max_radii2D.abs().sum()) == 0, f"{tag}: statistics not reset"
    if n_child:
        print(f"{tag}: largest child error / bar: xyz {worst['xyz']:.3f}, scaling {worst['scaling']:.3f}")
    return worst


def run_stats(d, case, st):
    """Every view through the statistics kernel and through the oracle; the accumulators compared."""
    for radii, grad2d, sgrad in case.views:
        d.add_densification_stats(radii.to(DEV), grad2d.to(DEV), sgrad.to(DEV))
        do.add_densification_stats(st, radii, grad2d, sgrad)
    for row, k in enumerate(do.ACCUMS[:4]):
        assert_rows(d.accum[row], st[k][:, 0], f"statistics: {k}", rtol=2e-6, atol=1e-12)
    assert_rows(d.accum[4], st["denom"][:, 0], "statistics: denom")
    assert_rows(d.max_radii2D, st["max_radii2D"], "statistics: max_radii2D")


def prepared(case, keys=do.PARAMS):
    """A densifier whose statistics kernel has been checked and which then holds the oracle's accumulators with the designated
    rows pinned, the oracle's state before any decision, and a maker of further densifiers in that state."""
    st = dc.oracle_state(case)
    d = densifier(case, keys)
    run_stats(d, case, st)
    dc.pin_rows(case, st)
    acc = dc.accum_matrix(st).to(DEV)
    d.accum.copy_(acc)

    def again(keys=keys, extra_groups=()):
        d2 = densifier(case, keys, extra_groups)
        d2.accum.copy_(acc)
        return d2
    return d, st, acc, again


def oracle_run(case, st0, do_prune, noise=None):
    st = copy.deepcopy(st0)
    pruned, clone, split = dc.two_calls(case, st, do_prune=do_prune, noise=noise)
    return st, pruned, clone, split


def check_counts(r, case, pruned, clone, split):
    n_clone, n_split = int(clone.sum()), int(split.sum())
    kept = case.P - int(pruned.sum()) - n_split
    assert r == dict(kept=kept, cloned=n_clone, split=n_split, pruned=int(pruned.sum()), num_points=kept + n_clone + case.N * n_split), r


def step_and_check_finite(d):
    """One optimizer step with unit gradients; what was finite stays finite (a zero rotation's children are NaN by construction)."""
    before = {k: torch.isfinite(d.params[k].detach()) for k in do.PARAMS}
    for k in do.PARAMS:
        d.params[k].grad = torch.ones_like(d.params[k])
    d.optimizer.step()
    for k in do.PARAMS:
        assert bool(torch.isfinite(d.params[k].detach()[before[k]]).all()), k
        state = d.optimizer.state[d.params[k]]
        assert bool(torch.isfinite(state["exp_avg"]).all()) and bool(torch.isfinite(state["exp_avg_sq"]).all()), k


# ---- sizes: workgroup boundaries, the P * W tail, scan blocks ---------------------------------------------------------------------
@pytest.mark.parametrize("P,seed", dc.SIZE_CASES)
def test_layout_matches_the_restatement_at_every_size(P, seed):
    case = dc.make_case(P, seed)
    d, st0, acc, again = prepared(case)
    runs = {}
    for do_prune in (True, False):
        runs[do_prune] = oracle_run(case, st0, do_prune)
        flags = d.flags(do_prune, True, case.min_opacity, case.extent, case.max_grad)
        assert_flags(flags, dc.flags_of(*runs[do_prune][1:]), case, f"flags(do_prune={do_prune})")
    st, pruned, clone, split = runs[True]
    # the two calls of the reference
    st_p = copy.deepcopy(st0)
    do.adaptive_prune(st_p, case.min_opacity, case.extent)
    r = d.adaptive_prune(case.min_opacity, case.extent)
    assert r["pruned"] == int(pruned.sum()) and r["cloned"] == 0 and r["split"] == 0, r
    compare_model(d, st_p, 0, "adaptive_prune")
    d.accum.copy_(acc[:, (~pruned).to(DEV)])             # adaptive_prune keeps the survivors' accumulators
    r = d.adaptive_densify(case.max_grad, case.extent, noise=case.noise)
    assert r["cloned"] == int(clone.sum()) and r["split"] == int(split.sum()), r
    compare_model(d, st, case.N * int(split.sum()), "adaptive_prune, adaptive_densify")
    # both in one plan
    d = again()
    check_counts(d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=case.noise), case, pruned, clone, split)
    compare_model(d, st, case.N * int(split.sum()), "prune_and_densify")
    # densification alone
    st, pruned, clone, split = runs[False]
    d = again()
    check_counts(d.adaptive_densify(case.max_grad, case.extent, noise=case.noise), case, pruned, clone, split)
    compare_model(d, st, case.N * int(split.sum()), "adaptive_densify alone")


@pytest.mark.parametrize("P,seed,N,surface", dc.NS_CASES)
def test_children_per_split_and_the_last_scale_column(P, seed, N, surface):
    case = dc.make_case(P, seed, N=N, surface=surface)
    d, st0, acc, again = prepared(case)
    st, pruned, clone, split = oracle_run(case, st0, True)
    assert_flags(d.flags(True, True, case.min_opacity, case.extent, case.max_grad), dc.flags_of(pruned, clone, split), case, "flags")
    r = d._run(True, True, case.min_opacity, case.extent, case.max_grad, None, N=N, noise=case.noise)
    check_counts(r, case, pruned, clone, split)
    compare_model(d, st, N * int(split.sum()), f"N={N}, surface={surface}")


@pytest.mark.parametrize("P,seed,kind", dc.UNIFORM_CASES)
def test_uniform_decisions(P, seed, kind):
    case = dc.uniform_case(P, seed, kind)
    d0, st0, acc, again = prepared(case)
    for do_prune in (True, False):
        st, pruned, clone, split = oracle_run(case, st0, do_prune)
        assert torch.equal(dc.flags_of(pruned, clone, split), case.row_flags[0 if do_prune else 1])
        assert_flags(d0.flags(do_prune, True, case.min_opacity, case.extent, case.max_grad), case.row_flags[0 if do_prune else 1], case, kind)
        d = again()
        if do_prune:
            r = d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=case.noise)
        else:
            r = d.adaptive_densify(case.max_grad, case.extent, noise=case.noise)
        check_counts(r, case, pruned, clone, split)
        compare_model(d, st, case.N * int(split.sum()), f"{kind}, do_prune={do_prune}")
        if kind == "prune" and do_prune:
            assert d.num_points == 0 and d.params["f_rest"].shape == (0, 3, 3)
        step_and_check_finite(d)


# ---- the packed 21-bit counters at their limit -------------------------------------------------------------------------------------
def limit_model(scale):
    P = dc.LIMIT_P
    g = torch.Generator(device=DEV).manual_seed(5)
    mk = lambda *s: torch.randn(*s, device=DEV, generator=g)
    return dict(xyz=mk(P, 3), f_dc=mk(P, 1, 3), f_rest=mk(P, 3, 3), color=mk(P, 3), opacity=torch.full((P, 1), 2.0, device=DEV),
                scaling=torch.log(torch.tensor(scale)) + 0.1 * mk(P, 3).clamp_(-3, 3), rotation=mk(P, 4))


def limit_densifier(scale, xyz_accum, denom):
    from soar_amd.densify import SurfelDensifier
    base = limit_model(scale)
    d = SurfelDensifier(dict(base), None)
    d.accum[0] = xyz_accum
    d.accum[4] = denom
    return base, d


def test_counter_limit_every_point_cloned():
    P = dc.LIMIT_P
    base, d = limit_densifier(dc.SMALL, 1.0, 1.0)
    r = d.adaptive_densify(dc.MAX_GRAD, dc.EXTENT)
    assert r == dict(kept=P, cloned=P, split=0, pruned=0, num_points=2 * P), r
    for k in do.PARAMS:
        assert_rows(d.params[k], torch.cat([base[k], base[k]]), f"all cloned: {k}")
    del base, d
    torch.cuda.empty_cache()


def test_counter_limit_every_point_split():
    P, N = dc.LIMIT_P, 2
    base, d = limit_densifier(dc.BIG, 1.0, 1.0)
    noise = torch.randn(N * P, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(6)).clamp_(-3, 3)
    r = d.adaptive_densify(dc.MAX_GRAD, dc.EXTENT, noise=noise)
    assert r == dict(kept=0, cloned=0, split=P, pruned=0, num_points=N * P), r
    # the oracle on the tensors the children are computed from; the others stand in as a column of row numbers (exact below 2^24),
    # which shows that their closed form is cat([x, x])
    index = torch.arange(P, dtype=torch.float32)[:, None]
    real = {k: base[k].cpu() for k in ("xyz", "scaling", "rotation")}
    stand_in = {k: real.get(k, index) for k in do.PARAMS}
    zeros = {k: torch.zeros_like(t) for k, t in stand_in.items()}
    st = do.new_state(stand_in, zeros, zeros)
    st["xyz_gradient_accum"] += 1
    st["denom"] += 1
    masks = do.adaptive_densify(st, dc.MAX_GRAD, dc.EXTENT, dc.PERCENT_DENSE, True, noise.cpu(), N)
    assert bool(masks["split"].all()) and torch.equal(st["params"]["color"], torch.cat([index, index]))
    worst = {k: assert_rows(d.params[k], st["params"][k], f"all split: {k}", **CHILD) for k in ("xyz", "scaling")}
    print(f"all split at P = 2^21 - 1: largest child error / bar: xyz {worst['xyz']:.3f}, scaling {worst['scaling']:.3f}")
    for k in ("f_dc", "f_rest", "color", "opacity", "rotation"):
        assert_rows(d.params[k], torch.cat([base[k], base[k]]), f"all split: {k}")
    del base, d, noise
    torch.cuda.empty_cache()


def test_counter_limit_every_point_pruned_but_the_last():
    P = dc.LIMIT_P
    denom = torch.zeros(P, device=DEV)
    denom[-1] = 1.0
    base, d = limit_densifier(dc.SMALL, 0.0, denom)
    r = d.prune_and_densify(dc.MIN_OPACITY, dc.MAX_GRAD, dc.EXTENT)
    assert r == dict(kept=1, cloned=0, split=0, pruned=P - 1, num_points=1), r
    for k in do.PARAMS:
        assert_rows(d.params[k], base[k][-1:], f"all pruned but the last: {k}")
    del base, d
    torch.cuda.empty_cache()


def test_plan_refuses_two_to_the_21_points():
    from soar_amd import hip_lib
    rc = hip_lib.lib().soar_densify_plan(2 ** 21, None, None, None, 1, 1, 0.1, 0.65, 1e-8, 2e-4, 0.013, None, None, None)
    assert rc != 0 and "2^21" in hip_lib.last_error(), (rc, hip_lib.last_error())


# ---- the statistics kernel ------------------------------------------------------------------------------------------------------
def check_hidden_points(d, case):
    """Points no view saw (radii <= 0 throughout) accumulate nothing, and a view of negative radii changes nothing at all."""
    hidden = torch.stack([radii <= 0 for radii, _, _ in case.views]).all(0).to(DEV)
    assert int(hidden.sum()) > 0
    assert float(d.accum[:, hidden].abs().sum()) == 0 and float(d.max_radii2D[hidden].abs().sum()) == 0
    assert float(d.max_radii2D.min()) >= 0
    accum, radii = d.accum.clone(), d.max_radii2D.clone()
    nan = torch.full((case.P, 3), float("nan"), device=DEV)
    d.add_densification_stats(torch.full((case.P,), -5, dtype=torch.int32, device=DEV), nan, nan)
    assert torch.equal(d.accum, accum) and torch.equal(d.max_radii2D, radii)


@pytest.mark.parametrize("P,seed,stride", dc.STRIDE_CASES)
def test_statistics_read_two_columns_at_any_stride(P, seed, stride):
    case = dc.make_case(P, seed, grad_stride=stride)
    assert case.views[0][1].shape == (P, stride) and (stride < 4 or bool(case.views[0][1][:, 2:].isnan().all()))
    d = densifier(case, None)
    run_stats(d, case, dc.oracle_state(case))
    check_hidden_points(d, case)


@pytest.mark.parametrize("P,seed", dc.STATS_CASES)
def test_statistics_over_five_views_with_negative_radii(P, seed):
    case = dc.make_case(P, seed, n_views=5, radii_low=-3)
    assert len(case.views) == 5 and min(int(v[0].min()) for v in case.views) == -3
    d = densifier(case, None)
    run_stats(d, case, dc.oracle_state(case))
    check_hidden_points(d, case)


# ---- where the split noise comes from --------------------------------------------------------------------------------------------
def test_noise_from_a_seeded_generator_longer_than_needed_and_too_short():
    case = dc.make_case(4099, 16)
    d, st0, acc, again = prepared(case)
    st, pruned, clone, split = oracle_run(case, st0, True)
    n_child = case.N * int(split.sum())
    assert n_child > 0
    # drawn by the densifier from a seeded device generator: the same draw fed to the oracle
    r = d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, generator=torch.Generator(device=DEV).manual_seed(7))
    check_counts(r, case, pruned, clone, split)
    drawn = torch.randn(n_child, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7)).cpu()
    compare_model(d, oracle_run(case, st0, True, noise=drawn)[0], n_child, "noise drawn from the generator")
    # longer than needed: only the first N * split rows are read
    d = again()
    d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=torch.cat([case.noise[:n_child], torch.full((9, 3), float("nan"))]))
    compare_model(d, st, n_child, "noise with a NaN tail")
    # too short: refused, and the model is left as it was
    d = again()
    with pytest.raises(ValueError, match="noise must be"):
        d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=case.noise[: n_child - 1])
    assert d.num_points == case.P and d.generation == 0 and float(d.accum[4].sum()) == float(acc[4].sum())
    with pytest.raises(ValueError, match="noise must be"):
        d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=case.noise[:n_child].reshape(-1))


def test_apply_without_noise_puts_children_on_their_parents():
    from soar_amd import hip_lib
    from soar_amd.hip_lib import SoarDensifyRow, check, ptr
    case = dc.make_case(257, 15)
    d, st0, acc, again = prepared(case, None)
    st, pruned, clone, split = oracle_run(case, st0, True, noise=torch.zeros_like(case.noise))
    P, N, P_new = case.P, case.N, st["params"]["xyz"].shape[0]
    L, stream = hip_lib.lib(), torch.cuda.current_stream(DEV).cuda_stream
    nbytes = C.c_size_t(0)
    check(L.soar_densify_plan_bytes(P, C.byref(nbytes)), "plan_bytes")
    plan = torch.empty(int(nbytes.value), dtype=torch.uint8, device=DEV)
    counts = (C.c_int64 * 3)()
    scaling, rotation, xyz = [d.params[k].detach().contiguous() for k in ("scaling", "rotation", "xyz")]
    opacity = d.params["opacity"].detach().reshape(-1).contiguous()
    check(L.soar_densify_plan(P, ptr(acc), ptr(scaling), ptr(opacity), 1, 1, case.min_opacity, 0.5 * case.extent, 1e-8 * case.extent ** 2,
                              case.max_grad, case.percent_dense * case.extent, ptr(plan), counts, stream), "plan")
    n_split = int(counts[2])
    assert n_split == int(split.sum()) and int(counts[0]) + int(counts[1]) + N * n_split == P_new
    out = {k: torch.full((P_new, 3), 7.0, device=DEV) for k in ("xyz", "scaling")}
    rows = (SoarDensifyRow * 2)(SoarDensifyRow(ptr(xyz), ptr(out["xyz"]), 3, 2), SoarDensifyRow(ptr(scaling), ptr(out["scaling"]), 3, 3))
    check(L.soar_densify_apply(P, N, ptr(plan), 2, rows, ptr(scaling), ptr(rotation), None, 1, stream), "apply")
    torch.cuda.synchronize()
    head = P_new - N * n_split
    for k in ("xyz", "scaling"):
        assert_rows(out[k][:head], st["params"][k][:head], f"noise = NULL: {k} (kept and cloned rows)")
        assert_rows(out[k][head:], st["params"][k][head:], f"noise = NULL: {k} (split children)", first_row=head, **CHILD)
    # bit for bit the parent's position, wherever the parent's rotation can be normalised
    full = torch.zeros(P, dtype=torch.bool)
    full[~pruned] = split
    parents = case.params["xyz"][full].repeat(N, 1)
    ok = (case.params["rotation"][full].norm(dim=1) > 0).repeat(N)
    assert int(ok.sum()) >= N * (n_split - 1) and torch.equal(out["xyz"][head:].cpu()[ok], parents[ok])
    assert bool(out["xyz"][head:].cpu()[~ok].isnan().all())


# ---- optimizer surgery -----------------------------------------------------------------------------------------------------------
def test_optimizer_with_state_for_some_tensors_only():
    case = dc.make_case(257, 15)
    keys = ("xyz", "opacity", "rotation")
    d, st0, acc, again = prepared(case, keys)
    st, pruned, clone, split = oracle_run(case, st0, True)
    check_counts(d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=case.noise), case, pruned, clone, split)
    compare_model(d, st, case.N * int(split.sum()), "state for xyz, opacity, rotation only", keys=keys)
    assert len(d.optimizer.state) == len(keys)
    step_and_check_finite(d)


def test_attribute_groups_are_left_alone():
    case = dc.make_case(257, 15)
    field = nn.Parameter(torch.randn(10, 4, device=DEV))
    moments = {"step": torch.tensor(1.0), "exp_avg": torch.randn(10, 4, device=DEV), "exp_avg_sq": torch.rand(10, 4, device=DEV)}
    kept = {k: v.clone() for k, v in moments.items()}
    d, st0, acc, again = prepared(case)
    d = again(extra_groups=[{"params": [field], "lr": 1e-3, "name": "attribute_field"}])
    d.optimizer.state[field] = moments
    st, pruned, clone, split = oracle_run(case, st0, True)
    check_counts(d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=case.noise), case, pruned, clone, split)
    compare_model(d, st, case.N * int(split.sum()), "with an attribute_field group")
    group = d.optimizer.param_groups[-1]
    assert group["name"] == "attribute_field" and group["params"][0] is field and d.optimizer.state[field] is moments
    assert all(torch.equal(moments[k], kept[k]) for k in kept)
    field.grad = torch.ones_like(field)
    step_and_check_finite(d)
    assert bool(torch.isfinite(field).all())
