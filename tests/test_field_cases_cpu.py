"""CPU tests of the attribute field's edge scenes (tests/field_cases.py): the exact scenes are exact (the float32 restatement
in three point orders equals the float64 one bit for bit, and the summed magnitudes stay below 2^23 grid units), the point orders
put into a wave what they say, and a small table forces collisions."""
import pytest
import torch

import field_cases as FC
import field_ref as R

GROUPS = [(o, t) for o in FC.ORDERS for t in FC.EXACT_LOG2_T]
LARGE = [c for c in FC.exact_cases() if c[1] > 12]


def _sizes(order, log2_T):
    return [n for o, t, n in FC.exact_cases() if (o, t) == (order, log2_T)]


def _assert_exact(scene, tag):
    f64 = FC.restate(scene, torch.float64)
    N = scene.points.shape[0]
    perms = {"given": None, "reversed": torch.arange(N - 1, -1, -1), "shuffled": torch.randperm(N, generator=torch.Generator().manual_seed(N))}
    for how, perm in perms.items():
        f32 = FC.restate(scene, torch.float32, perm)
        for n in ("offsets",) + FC.EXACT_NAMES:
            assert f32[n].dtype == torch.float32 and f64[n].dtype == torch.float64
            assert torch.equal(f32[n].double(), f64[n]), (tag, how, n, float((f32[n].double() - f64[n]).abs().max()))
    return f64


@pytest.mark.parametrize("order,log2_T", GROUPS)
def test_exact_scenes_agree_bit_for_bit(order, log2_T):
    carried = 0
    for N in _sizes(order, log2_T):
        f64 = _assert_exact(FC.exact_case(order, log2_T, N), (order, log2_T, N))
        carried += int(f64["encoding.hash_table"].abs().sum() > 0 and f64["z"].abs().sum() > 0
                       and f64["mlp_base_offsets.layers.0.weight"].abs().sum() > 0)
    assert carried >= len(FC.SIZES) - 2, carried          # the scenes carry a gradient (a single point may sit on dead units)


@pytest.mark.parametrize("order,log2_T,N", LARGE)
def test_large_exact_scenes_agree_bit_for_bit(order, log2_T, N):
    scene = FC.exact_case(order, log2_T, N)
    _assert_exact(scene, (order, log2_T, N))
    assert FC.exactness_margin(scene) < 2 ** 23


@pytest.mark.parametrize("order,log2_T", GROUPS)
def test_margin_holds(order, log2_T):
    worst = 0.0
    for N in _sizes(order, log2_T):
        m = FC.exactness_margin(FC.exact_case(order, log2_T, N))
        worst = max(worst, m)
        assert m < 2 ** 23, (order, log2_T, N, m)
    print(f"{order} log2_T={log2_T}: largest sum of magnitudes {worst:.0f} grid units (2^{torch.log2(torch.tensor(worst)).item():.1f})")


def test_margin_sees_an_inexact_scene():
    """the condition can fail: the same scene on sixteenths of 2^-12 with 777 equal points is past 2^23 units"""
    scene = FC.exact_scene(4, torch.tensor([[0.0625, 0.5625, 0.3125]]).expand(777, 3), **FC.COARSE)
    assert scene.grid == 2.0 ** -12
    assert FC.exactness_margin(scene) >= 2 ** 23


def test_grids():
    assert FC.exact_case("runs", 4, 65).grid == 2.0 ** -6
    assert FC.exact_case("box_edges", 4, 65).grid == 2.0 ** -6
    assert FC.exact_case("coarse_shared", 4, 65).grid == 2.0 ** -9


def _waves(x):
    return [x[i:i + FC.WAVE] for i in range(0, x.shape[0], FC.WAVE)]


RES = R.resolutions()
T18 = 2 ** 18


def test_one_point_is_one_key_per_wave():
    keys, _, _ = FC.lane_keys(FC.one_point(257), RES, T18)
    for w in _waves(keys):
        assert bool((w == w[:1]).all())                   # one key per (level, corner) across the wave


def test_runs_holds_the_stated_lengths():
    for N in FC.SIZES:
        pts = FC.runs(N)
        keys, floor, _ = FC.lane_keys(pts, RES, T18)
        want = FC.run_lengths(N)
        assert sum(want) == N
        assert FC.run_lengths_of(floor[:, 0]) == want                              # level 0, by cell
        for k in range(8):
            assert FC.run_lengths_of(keys[:, 0, k]) == want, (N, k)                # and by the key that each corner's lanes compare
    got = FC.run_lengths(777)
    assert set(FC.RUN_LENGTHS) <= set(got)
    ends = torch.cumsum(torch.tensor(got), 0)
    starts = ends - torch.tensor(got)
    assert 64 in ends.tolist()                                                     # a run ends exactly on lane 63
    assert any(s < 128 <= e - 1 and s <= 127 for s, e in zip(starts.tolist(), ends.tolist()))    # lane 63 -> lane 0, across blocks
    assert any(s < 192 <= e - 1 for s, e in zip(starts.tolist(), ends.tolist()))   # ... and across the two waves of one block
    for N in (63, 127, 130):                                                       # the ragged sizes cut a run off at the last valid lane
        assert FC.run_lengths(N)[-1] > 1 and N % FC.WAVE != 0


def test_alternating_shares_rows_but_not_with_neighbours():
    keys, floor, _ = FC.lane_keys(FC.alternating(130), RES, T18)
    assert bool((keys[1:] != keys[:-1]).all())            # no corner of any level equals the neighbouring lane's
    assert bool((floor[1:] != floor[:-1]).any(dim=-1).all())
    assert bool((keys[2:] == keys[:-2]).all())            # yet every row comes back two lanes on


def test_coarse_shared_splits_at_the_fine_levels():
    res = R.resolutions(16, **FC.COARSE)
    assert res.tolist()[:2] == [2, 2] and res.tolist()[-1] == 64 and any(int(r) % 2 for r in res.tolist())
    assert any(a == b for a, b in zip(res.tolist(), res.tolist()[1:]))
    pts = FC.coarse_shared(777)
    keys, floor, _ = FC.lane_keys(pts, res, T18)
    n = torch.arange(776)
    same_group = (n // 16) == ((n + 1) // 16)
    assert bool((keys[1:, 0] == keys[:-1, 0]).all(dim=-1)[same_group].all())       # level 0: neighbours of a group share all 8 rows
    assert bool((floor[1:, 15] != floor[:-1, 15]).any(dim=-1).all())               # level 15: no two neighbours share a cell
    assert bool((keys[1:, 15, 0] != keys[:-1, 15, 0]).all())
    shared = (keys[1:] == keys[:-1]).all(dim=-1)[same_group].float().mean(dim=0)   # per level: share of neighbours with equal rows
    assert shared[0] == 1 and shared[15] == 0 and 0 < shared[4] < 1


def test_outside_reaches_negative_cells():
    pts = FC.outside(257)
    assert bool(((pts < 0) | (pts > 1)).any(dim=1).all())
    _, floor, _ = FC.lane_keys(pts, RES, T18)
    assert int(floor.min()) < 0 and int(floor.max()) > int(RES[-1])


def test_box_edges_selects_nothing():
    pts = FC.box_edges(257)
    _, _, sel = FC.lane_keys(pts, RES, T18, normalized=False, aabb=FC.BOX)
    assert not bool(sel.any())
    p = (pts + 1) / 4
    assert bool((p == 0).any()) and bool((p == 1).any()) and bool((p < 0).any()) and bool((p > 1).any())
    mixed, inside = FC.box_mixed(257)
    _, _, sel = FC.lane_keys(mixed, RES, T18, normalized=False, aabb=FC.BOX)
    assert torch.equal(sel, inside) and 100 < int(inside.sum()) < 157


def test_small_table_forces_collisions():
    for order in FC.ORDERS:
        scene = FC.exact_case(order, 1, 130)
        keys, _, _ = FC.lane_keys(scene.p, scene.res, 2)
        for l in range(16):
            rows = keys[:, l] - 2 * l
            assert int(rows.min()) >= 0 and int(rows.max()) <= 1            # at most two rows per level, for every corner of every point


def test_real_scene_follows_the_gpu_tests_field():
    s = FC.real_scene(4, 300, seed=1, base_res=2, max_res=64)
    f = s.field
    assert f.encoding.hash_table.shape == (16 * 16, 2) and f.encoding.scalings.tolist() == R.resolutions(16, 2, 64).tolist()
    assert float(f.encoding.hash_table.detach().abs().max()) > 0.05
    assert float(f.mlp_base_offsets.layers[1].weight.detach().abs().max()) > 0
    assert s.xyz["random"].shape == s.xyz["spatial"].shape == (300, 3)
    assert torch.equal(torch.sort(s.xyz["random"][:, 0])[0], torch.sort(s.xyz["spatial"][:, 0])[0])
    assert not torch.equal(s.xyz["random"], s.xyz["spatial"])
