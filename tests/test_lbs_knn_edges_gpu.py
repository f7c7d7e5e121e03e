"""The K-nearest-vertex kernels of csrc/lbs_knn.hip off the body's surface, on sparse, flat and degenerate vertex sets: the full
search (knn_cell_kernel: box growth, brute-force fallback in one and in several staged chunks, clamped cells), the generic
kernel (knn_grid_kernel: any K <= 32, any J) and the follower (knn_certify_kernel / knn_blend_search_kernel), each against
brute force in float64 (oracle/lbs_oracle.py on float64 copies of the float32 inputs).  The cases come from tests/knn_cases.py;
tests/test_knn_cases_cpu.py proves that each reaches the branch it is named for.

Neighbour sets: a row equals the oracle's, or ``_rows_equal_or_proved_ties`` proves it a tie at the K-th place -- at most 1 % of a
case's rows, except where the case is built of ties (then the sorted distances must be the brute-force ones to 1e-7).  Weights:
rtol 1e-4, atol 1e-6 against the oracle (rows settled by the proof: against the oracle's blend of the kernel's own neighbour list);
every row sums to one within 1e-5.  The follower: bit-equal to KnnGrid.query at every step, which is itself held to the oracle."""
import numpy as np
import pytest
import torch

import knn_cases as kc
from oracle import lbs_oracle as lo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIE_CAP = 0.01


def check_against_oracle(label, w, idx, x, verts, weights, K=kc.KNN_K, ties=False):
    """w [P,J], idx [P,K] from a kernel; x, verts, weights the float32 CPU inputs.  -> the share of rows settled by the tie proof."""
    P, V = x.shape[0], verts.shape[0]
    x64, v64, w64 = x.double(), verts.double(), weights.double()
    d2_ref, i_ref = lo.knn_brute(x64, v64, K)
    w_ref = lo.query_weights(x64, v64, w64, K, knn=(d2_ref, i_ref))
    idx = idx.cpu().long()
    assert idx.shape == (P, K) and int(idx.min()) >= 0 and int(idx.max()) < V, label
    same = kc._rows_equal_or_proved_ties(idx.numpy(), i_ref.numpy(), x.numpy(), verts.numpy())
    settled = int((~same).sum())
    note = f"{label}: {settled} of {P} rows ({100.0 * settled / P:.2f} %) settled by the tie proof"
    print(note)
    own_d2 = ((v64[idx] - x64[:, None, :]) ** 2).sum(2)
    if ties:
        err = float((torch.sort(own_d2.sqrt(), 1).values - d2_ref.sqrt()).abs().max())
        assert err < 1e-7, f"{note}; distances off by {err:.3e}"
        assert all(len(set(r)) == K for r in idx.tolist()), note
    else:
        assert settled <= TIE_CAP * P, note
    got = w.cpu().double()
    same_t = torch.from_numpy(same)
    np.testing.assert_allclose(got[same_t].numpy(), w_ref[same_t].numpy(), rtol=1e-4, atol=1e-6, err_msg=note)
    if settled:
        own = lo.query_weights(x64[~same_t], v64, w64, K, knn=(own_d2[~same_t], idx[~same_t]))
        np.testing.assert_allclose(got[~same_t].numpy(), own.numpy(), rtol=1e-4, atol=1e-6, err_msg=note)
    row_sum = float((got.sum(1) - 1.0).abs().max())
    assert row_sum <= 1e-5, f"{note}; a row sums to 1 -+ {row_sum:.3e}"
    return settled / P


# ---- 1-9: the full search, K = 30, J = 55 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kc.FULL_SEARCH_CASES))
def test_full_search_matches_brute_force(name):
    from soar_amd import lbs
    case = kc.FULL_SEARCH_CASES[name]()
    v, vw, x = case.verts.to(DEV), case.weights.to(DEV), case.queries.to(DEV)
    grid = lbs.KnnGrid(v, vw)
    w, idx = grid.query(x, return_idx=True)
    assert torch.equal(grid.query(x), w), f"{case.name}: the weights depend on whether the indices are asked for"
    w_one, idx_one = lbs.knn_blend_weights(x, v, vw, return_idx=True)
    assert torch.equal(w_one, w) and torch.equal(idx_one, idx), f"{case.name}: grid built once != one-call form"
    assert torch.equal(lbs.knn_blend_weights(x, v, vw), w)
    check_against_oracle(case.name, w, idx, case.queries, case.verts, case.weights, ties=case.ties)
    if name == "far-from-origin":
        # the neighbour sets of the untranslated case, wherever the translation's rounding leaves them decided
        home = case.home
        i_home = lo.knn_brute(home.queries.double(), home.verts.double(), kc.KNN_K)[1].numpy()
        same = kc._rows_equal_or_proved_ties(idx.cpu().numpy().astype(np.int64), i_home, case.queries.numpy(), case.verts.numpy())
        print(f"{case.name}: {int((~same).sum())} of {len(same)} rows differ from the untranslated sets, each a proved tie")


# ---- 10: the generic kernel, K and J off the fast path ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kc.GENERIC_CASES))
@pytest.mark.parametrize("K,J", kc.GENERIC_KJ)
def test_generic_kernel_matches_brute_force(K, J, name):
    from soar_amd import lbs
    case = kc.GENERIC_CASES[name]()
    weights = case.weights if J == 55 else kc.random_rows(case.verts.shape[0], J, 1000 + J)
    v, vw = case.verts.to(DEV), weights.to(DEV)
    grid = lbs.KnnGrid(v, vw)
    for P in kc.GENERIC_P:
        queries = kc.generic_queries(case, P)
        x = queries.to(DEV)
        w, idx = grid.query(x, K=K, return_idx=True)
        assert w.shape == (P, J) and torch.equal(grid.query(x, K=K), w)
        w_one, idx_one = lbs.knn_blend_weights(x, v, vw, K=K, return_idx=True)
        assert torch.equal(w_one, w) and torch.equal(idx_one, idx)
        check_against_oracle(f"{case.name}, K={K} J={J} P={P}", w, idx, queries, case.verts, weights, K=K, ties=case.ties)


def test_generic_kernel_takes_every_vertex_at_k_32_of_32():
    from soar_amd import lbs
    case = kc.smallest(32)
    w, idx = lbs.KnnGrid(case.verts.to(DEV), case.weights.to(DEV)).query(case.queries.to(DEV), K=32, return_idx=True)
    assert (torch.sort(idx.cpu().long(), 1).values == torch.arange(32)).all()
    check_against_oracle(case.name + ", K=32", w, idx, case.queries, case.verts, case.weights, K=32)


# ---- 11-15: the follower ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kc.FOLLOWER_CASES))
def test_follower_is_the_full_search_and_the_full_search_is_exact(name):
    from soar_amd import lbs
    case = kc.FOLLOWER_CASES[name]()
    grid = lbs.KnnGrid(case.verts.to(DEV), case.weights.to(DEV))
    P = case.steps[0].shape[0]
    fol = lbs.KnnFollower(grid, P)
    before = 0
    for step, queries in enumerate(case.steps):
        x = queries.to(DEV)
        got = fol(x).clone()
        want, idx = grid.query(x, return_idx=True)
        worst = float((got - want).abs().max())
        assert torch.equal(got, want), f"{case.name}, step {step}: follower != full search (max difference {worst:.3e})"
        assert torch.equal(grid.query(x), want)
        n = int(fol.searched.item())
        searched, before = n - before, n
        print(f"{case.name}, step {step}: {searched} of {P} searched")
        assert 0 <= searched <= P, (case.name, step, searched)
        if step == 0:
            assert searched == 0                                # the full search
        if step == 1:
            assert searched == P                                # the first refresh after a full search measures every gap
        if step in case.still:
            assert searched <= P // 50, (case.name, step, searched)     # nothing moved: certified, but for near-ties at the K-th place
        check_against_oracle(f"{case.name}, step {step}", want, idx, queries, case.verts, case.weights)


def test_follower_refuses_as_many_vertices_as_it_keeps():
    """V = 32: the plain search serves it, the neighbour state (32 kept vertices and a gap BEHIND them) does not; V = 33 is case 11."""
    from soar_amd import lbs
    case = kc.smallest(32)
    grid = lbs.KnnGrid(case.verts.to(DEV), case.weights.to(DEV))
    x = case.queries.to(DEV)
    w, idx = grid.query(x, return_idx=True)
    check_against_oracle(case.name, w, idx, case.queries, case.verts, case.weights)
    fol = lbs.KnnFollower(grid, x.shape[0])
    with pytest.raises(RuntimeError, match="keeps 32 vertices"):
        fol(x)
