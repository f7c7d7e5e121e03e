"""GPU tests of the initialisation from keypoints (soar_amd/pose_init.py, csrc/pose_init.hip; ``smplify.model_points``) against the
restatement of tests/pose_init_ref.py on the seeded body of tests/golden/smplify.npz (96 vertices, 144 model points, 123 mapped;
skewed intrinsics, a tilted w2c).

The bar (``smplify_ref.bar_check``): HIP against float64 at most 4 x (float32 restatement against float64), floor 1e-6 of the
tensor's largest magnitude.  The path is float32 additions and comparisons only: it must equal the NumPy restatement exactly.

The fit (N = 6, the low-prior stage 2 L-BFGS steps, then 1 + 2 steps, at most 8 iterations each; the float64 objective at each
drive's final parameters against the searched start; measured on an MI355X, from 1026.7): HIP 64.1321, float32 restatement
63.8508, float64 restatement 64.1343; 50 / 49 / 50 closure evaluations."""
import types

import numpy as np
import pytest
import torch

import pose_init_ref as pr
import smplify_ref as sr
from test_smplify_cpu import golden, golden_call

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Z_MIN, CONF_MIN, MIN_POINTS = 0.1, 0.1, 6


def to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


@pytest.fixture(scope="module")
def w():
    from soar_amd import pose_init, smplify
    g, m, p, i, tables = golden()
    rig = smplify.KeypointRig.from_body_model(m, *tables, device=DEV)
    assert (rig.PA, rig.P) == (144, 123)
    c = golden_call(g)
    base6 = pr.base_params(pr.golden_base_poses(), 10, 10)
    pts64 = pr.points_of(m, base6, torch.float64)
    pts32 = pr.points_of(m, base6, torch.float32)
    hip = smplify.model_points(rig, to_dev({k: v.float() for k, v in base6.items()}))
    return types.SimpleNamespace(g=g, m=m, p=p, i=i, tables=tables, rig=rig, c=c, smplify=smplify, pi=pose_init, pts64=pts64, pts32=pts32,
                                 pts=hip, cache={})


# ---- model_points -------------------------------------------------------------------------------------------------------------------

def ref_points(w, p, dtype):
    return pr.points_of(w.m, p, dtype)


@pytest.mark.parametrize("N", [5, 1])
def test_model_points_against_the_restatement(w, N):
    p = {k: (v if k == "betas" else v[:N]) for k, v in w.p.items()}
    Ks, w2c = w.c["Ks"][:N].to(DEV), w.c["w2c"].to(DEV)
    before = w.smplify.project_keypoints(w.rig, to_dev(p), Ks, w2c)
    got = w.smplify.model_points(w.rig, to_dev(p))
    assert got.shape == (N, 144, 3) and got.dtype == torch.float32
    sr.bar_check(f"model_points N={N}", got, ref_points(w, p, torch.float32), ref_points(w, p, torch.float64))
    assert torch.equal(got, w.smplify.model_points(w.rig, to_dev(p)))                     # two runs agree bit for bit
    assert torch.equal(before, w.smplify.project_keypoints(w.rig, to_dev(p), Ks, w2c))    # and the objective's kernel is as it was
    # the mapped points are what the objective's kernel scatters: through convert_kps and the camera they give its keypoints
    kps = sr.project(sr.convert_kps(got.double().cpu(), *w.tables[:2]), w.c["Ks"][:N].double(), w.c["w2c"].double())
    ok = (before.cpu().double() - kps).abs() <= 1e-3 * (1.0 + kps.abs())
    assert bool(ok[[n for n in range(N) if n != 3]].all())                                 # (frame 3 sits under the depth clamp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.smplify.model_points(w.rig, p)


def test_model_points_of_a_rig_with_a_contour_table_and_a_mean(w):
    """The static points only (55 + 21 + 51), the mean applied."""
    import smplify_body_ref as sb
    from test_smplify_body_cpu import golden as body_golden
    g, m, p, i, tables = body_golden()
    rig = w.smplify.KeypointRig.from_body_model(m, *tables, device=DEV, dynamic_contour=True, use_pose_mean=True)
    assert rig.PA == 55 + 21 + 51 and rig.LD == 17 and rig.mean_mask != 0
    got = w.smplify.model_points(rig, to_dev(p))

    def ref(dtype):
        q = {k: v.to(dtype) for k, v in p.items()}
        N = q["transl"].shape[0]
        coef = torch.cat([q["betas"].mean(0, keepdim=True).expand(N, -1), q["expression"]], -1)
        return sr.model_points(m, sb.full_rotations(q, m.pose_mean, detour=False), coef, q["transl"], gather=True)
    assert got.shape == ref(torch.float64).shape == (p["transl"].shape[0], 127, 3)
    sr.bar_check("model_points contour + mean", got, ref(torch.float32), ref(torch.float64))


# ---- search -------------------------------------------------------------------------------------------------------------------------

def hip_search(w, targets, Ks, R, pts=None, scales=None, rig=None, **kw):
    pts = w.pts if pts is None else pts
    t = targets.to(DEV)
    scales = w.smplify.target_scales(t, w.c["img_wh"]) if scales is None else scales.to(DEV)
    kw = {"conf_min": CONF_MIN, "z_min": Z_MIN, "min_points": MIN_POINTS, **kw}
    return w.pi.search(pts, pts[:, 0], R.to(DEV), rig or w.rig, t, Ks.to(DEV), w.c["w2c"].to(DEV), w.c["img_wh"], scales, **kw), scales


def ref_search(w, targets, Ks, R, scales, dtype, pts=None, tables=None, **kw):
    pts = (w.pts64 if dtype == torch.float64 else w.pts32) if pts is None else pts
    kw = {"conf_min": CONF_MIN, "z_min": Z_MIN, "min_points": MIN_POINTS, **kw}
    return pr.search(pts, pts[:, 0], R, tables or w.tables, targets.cpu(), Ks.cpu(), w.c["w2c"], w.c["img_wh"], scales.cpu(), dtype=dtype, **kw)


def check_search(tag, w, targets, Ks, R, max_left_out=0.02, **kw):
    """HIP against the float64 restatement under the bar over the states that are finite in float64; a state whose smallest depth
    lies within 1e-3 (relative) of z_min in float64 may be left out; validity must be equal everywhere else."""
    targets, R = targets.float(), R.float()
    got, scales = hip_search(w, targets, Ks, R, **kw)
    r64, r32 = (ref_search(w, targets, Ks, R, scales, dt, **{k: v for k, v in kw.items() if k != "scales"}) for dt in (torch.float64, torch.float32))
    cost, transl = got.cost.cpu().numpy().astype(np.float64), got.transl.cpu().numpy().astype(np.float64)
    z_min = kw.get("z_min", Z_MIN)
    near = np.abs(r64["zmin"] - z_min) <= 1e-3 * z_min
    assert near.mean() <= max_left_out, (tag, near.mean())
    fin = np.isfinite(r64["cost"])
    assert np.array_equal(np.isfinite(cost)[~near], fin[~near]), tag
    assert np.array_equal(got.valid.cpu().numpy(), np.isfinite(cost).any(1)), tag           # valid[n]: any state of the frame is finite
    assert bool((cost[~np.isfinite(cost)] == np.inf).all()) and bool((transl[~np.isfinite(cost)] == 0).all())
    sel = fin & ~near & np.isfinite(r32["cost"])
    if sel.any():
        sr.bar_check(f"{tag} cost", cost[sel], r32["cost"][sel], r64["cost"][sel])
        sr.bar_check(f"{tag} transl", transl[sel], r32["transl"][sel], r64["transl"][sel])
    return got, r64, near


def planted(w):
    if "planted" not in w.cache:
        w.cache["planted"] = pr.planted_scene(w.m, w.tables, w.c)
    return w.cache["planted"]


def test_search_finds_the_planted_state(w):
    sc = planted(w)
    got, r64, near = check_search("planted", w, sc["targets"], w.c["Ks"], sc["R"], max_left_out=0.0)
    assert got.cost.shape == (5, 24) and got.transl.shape == (5, 24, 3) and got.valid.dtype == torch.bool and bool(got.valid.all())
    assert not near.any()
    assert got.cost.argmin(1).tolist() == sc["s_true"].tolist() == r64["cost"].argmin(1).tolist()
    best = got.transl[torch.arange(5), got.cost.argmin(1)].cpu().numpy()
    assert np.abs(best - sc["transl_true"]).max() <= 1e-3                                   # float32 targets, metres
    again, _ = hip_search(w, sc["targets"].float(), w.c["Ks"], sc["R"].float())
    assert torch.equal(again.cost, got.cost) and torch.equal(again.transl, got.transl) and torch.equal(again.valid, got.valid)


@pytest.mark.parametrize("B,H,N", [(2, 5, 5), (5, 13, 2), (2, 12, 1)], ids=["S10", "S65", "N1"])
def test_search_at_other_state_counts(w, B, H, N):
    """S = 10 (fewer states than wavefronts), S = 65 (one state past 64 and past four rounds of sixteen wavefronts), N = 1."""
    sc = planted(w)
    angles = np.linspace(0.0, 1.1, B)
    poses = torch.zeros(B, 21, 3, dtype=torch.float64)
    poses[:, 15, 2], poses[:, 16, 2] = torch.from_numpy(-angles), torch.from_numpy(angles)
    base6 = pr.base_params(poses.reshape(B, 63), 10, 10)
    pts = w.smplify.model_points(w.rig, to_dev({k: v.float() for k, v in base6.items()}))
    targets, Ks, R = sc["targets"][:N].float(), w.c["Ks"][:N], pr.yaw_bank(H).float()
    got, scales = hip_search(w, targets, Ks, R, pts=pts)
    assert got.cost.shape == (N, B * H)
    r64, r32 = (ref_search(w, targets, Ks, R, scales, dt, pts=pr.points_of(w.m, base6, dt)) for dt in (torch.float64, torch.float32))
    fin = np.isfinite(r64["cost"])
    assert fin.all() and bool(torch.isfinite(got.cost).all())
    sr.bar_check(f"S={B * H} N={N} cost", got.cost, r32["cost"], r64["cost"])
    sr.bar_check(f"S={B * H} N={N} transl", got.transl, r32["transl"], r64["transl"])


def test_search_counts_the_usable_keypoints(w):
    """0, 1 and min_points - 1 usable keypoints: all +inf, valid false; exactly min_points: finite.  Usable: confidence at or above
    conf_min on a row the mask keeps, outside the hands."""
    sc = planted(w)
    rows = [k for k in range(137) if float(w.tables[2][k]) > 0 and not 25 <= k < 67 and float(sc["targets"][0, k, 2]) > 0][:: 9][:MIN_POINTS]
    assert len(rows) == MIN_POINTS
    frames = []
    for count in (0, 1, MIN_POINTS - 1, MIN_POINTS):
        t = sc["targets"][0].clone()
        t[:, 2] = 0.0
        t[rows[:count], 2] = 1.0
        t[30, 2] = 1.0                                                                      # a hand row never counts
        frames.append(t)
    targets = torch.stack(frames)
    Ks = w.c["Ks"][[0, 0, 0, 0]]
    got, r64, _ = check_search("usable", w, targets, Ks, sc["R"], scales=sc["scales"][[0, 0, 0, 0]].float())
    assert got.valid.tolist() == [False, False, False, True]
    assert bool(torch.isinf(got.cost[:3]).all()) and bool((got.cost[:3] > 0).all()) and bool((got.transl[:3] == 0).all())
    assert bool(torch.isfinite(got.cost[3, sc["s_true"][0]])) and got.cost[3].argmin().item() == sc["s_true"][0]


def test_search_edges_of_validity(w):
    sc = planted(w)
    R, Ks4 = sc["R"], w.c["Ks"][[0, 0, 0, 0]]
    scales = sc["scales"][[0, 0, 0, 0]].float()
    # every weighted keypoint at one pixel: the system is singular up to rounding.  The frame's sums are restated bit for bit, so the
    # determinant's sign is float64's; at this pixel it rounds to a non-positive value and every state is refused.  (Where it rounds
    # to a positive one the solve divides rounding errors and nothing can be asked of the states: DESIGN.md 9zc.)
    one = sc["targets"][0].clone()
    one[:, 0], one[:, 1] = 0.4371, 0.5129
    # a body behind the camera: its image is the planted one mirrored through the principal point
    cam_t = sc["cam_t"][:1] * np.array([1.0, 1.0, -1.0])
    behind = pr.plant(sc["points0"], sc["points0"][:, 0], R[[3]], np.array([1]), cam_t, w.tables, w.c["Ks"][:1], w.c["w2c"], w.c["img_wh"],
                      torch.ones(1, 137, dtype=torch.float64))[0]
    # confidences just below and at conf_min on one row
    k = 5
    below, at = sc["targets"][0].clone(), sc["targets"][0].clone()
    below[k, 2], at[k, 2] = float(np.nextafter(np.float32(CONF_MIN), np.float32(0))), float(np.float32(CONF_MIN))
    targets = torch.stack([one, behind, below, at])
    got, r64, near = check_search("edges", w, targets, Ks4, R, scales=scales, max_left_out=0.02)
    print("one pixel: finite states hip", int(torch.isfinite(got.cost[0]).sum()), "float64", int(np.isfinite(r64["cost"][0]).sum()))
    assert not np.isfinite(r64["cost"][1]).any() and bool(torch.isinf(got.cost[1]).all()) and not bool(got.valid[1])      # behind: invalid
    zeroed = sc["targets"][0].clone()
    zeroed[k, 2] = 0.0
    ref0, _ = hip_search(w, torch.stack([zeroed]).float(), Ks4[:1], R.float(), scales=scales[:1])
    assert torch.equal(got.cost[2], ref0.cost[0]) and torch.equal(got.transl[2], ref0.transl[0])                         # below: the row is out
    assert not torch.equal(got.cost[3], ref0.cost[0])                                                                     # at: it counts


def test_search_gives_contour_rows_weight_zero(w):
    import smplify_body_ref as sb
    from test_smplify_body_cpu import golden as body_golden
    g, m, p, i, tables = body_golden()
    flat = sb.golden_model(g, mean=False)
    rig = w.smplify.KeypointRig.from_body_model(flat, *tables, device=DEV, dynamic_contour=True)
    contour = [d for s, d in zip(tables[0], tables[1]) if s >= rig.PA]
    assert rig.PA == 127 and len(contour) >= 1
    base6 = pr.base_params(pr.golden_base_poses(), 10, 10)
    static = sb.golden_model(g, dynamic=False, mean=False)
    pts64, pts32 = (pr.points_of(static, base6, dt) for dt in (torch.float64, torch.float32))
    assert pts64.shape[1] == 127
    pts = w.smplify.model_points(rig, to_dev({k: v.float() for k, v in base6.items()}))
    R = pr.yaw_bank(12)
    c = golden_call(g)
    tgt = pr.plant(pts64, pts64[:, 0], R[[2, 7]], np.array([0, 1]), np.array([[0.1, 0.0, 3.0], [-0.2, 0.1, 4.0]]), tables, c["Ks"][:2], c["w2c"],
                   c["img_wh"], torch.ones(2, 137, dtype=torch.float64)).float()
    scales = sr.target_scales(tgt.double(), c["img_wh"]).float()
    run = lambda t: w.pi.search(pts, pts[:, 0], R.float().to(DEV), rig, t.to(DEV), c["Ks"][:2].to(DEV), c["w2c"].to(DEV), c["img_wh"],
                                scales.to(DEV), conf_min=CONF_MIN, z_min=Z_MIN, min_points=MIN_POINTS)
    got = run(tgt)
    r64, r32 = (pr.search(q, q[:, 0], R.float(), tables, tgt, c["Ks"][:2], c["w2c"], c["img_wh"], scales, dtype=dt) for q, dt in
                ((pts64, torch.float64), (pts32, torch.float32)))
    assert np.isfinite(r64["cost"]).all()
    sr.bar_check("contour rig cost", got.cost, r32["cost"], r64["cost"])
    sr.bar_check("contour rig transl", got.transl, r32["transl"], r64["transl"])
    assert got.cost.argmin(1).tolist() == [2, 12 + 7]
    moved = tgt.clone()
    moved[:, contour, :2] += 0.3                                        # whatever stands on the contour rows changes no bit
    other = run(moved)
    assert torch.equal(other.cost, got.cost) and torch.equal(other.transl, got.transl)


def test_a_frame_alone_equals_the_frame_in_the_batch(w):
    sc = planted(w)
    targets, R, Ks = sc["targets"].float(), sc["R"].float(), w.c["Ks"]
    batch, scales = hip_search(w, targets, Ks, R)
    for f in range(5):
        one, _ = hip_search(w, targets[f:f + 1], Ks[f:f + 1], R, scales=scales[f:f + 1])
        assert torch.equal(one.cost[0], batch.cost[f]) and torch.equal(one.transl[0], batch.transl[f]) and bool(one.valid[0]) == bool(batch.valid[f])
    perm = [3, 0, 4, 2, 1]
    shuffled, _ = hip_search(w, targets[perm], Ks[perm], R, scales=scales[perm])
    assert torch.equal(shuffled.cost, batch.cost[perm]) and torch.equal(shuffled.transl, batch.transl[perm])
    # strided target_kps and Ks
    wide = torch.zeros(5, 137, 6, device=DEV)
    wide[..., ::2] = targets.to(DEV)
    Kt = Ks.to(DEV).transpose(1, 2).contiguous().transpose(1, 2)
    assert not wide[..., ::2].is_contiguous() and not Kt.is_contiguous()
    strided, _ = hip_search(w, wide[..., ::2], Kt, R, scales=scales)
    assert torch.equal(strided.cost, batch.cost) and torch.equal(strided.transl, batch.transl)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w.pi.search(w.pts, w.pts[:, 0], R.to(DEV), w.rig, targets, Ks.to(DEV), w.c["w2c"].to(DEV), w.c["img_wh"], scales)
    with pytest.raises(ValueError, match="1024"):
        w.pi.search(w.pts, w.pts[:, 0], torch.eye(3, device=DEV).repeat(513, 1, 1), w.rig, targets.to(DEV), Ks.to(DEV), w.c["w2c"].to(DEV),
                    w.c["img_wh"], scales)


# ---- the path ---------------------------------------------------------------------------------------------------------------------

def check_path(w, U, T):
    path, total = w.pi.viterbi(torch.from_numpy(U).to(DEV), torch.from_numpy(T).to(DEV))
    rp, rt, _ = pr.viterbi(U, T)
    assert path.dtype == torch.int64 and path.tolist() == rp.tolist(), (path.tolist(), rp.tolist())
    assert np.float32(total.item()) == rt or (np.isinf(rt) and np.isinf(total.item()))
    return rp


@pytest.mark.parametrize("N,S", [(1, 7), (2, 7), (5, 1), (6, 65), (3, 1024)])
def test_viterbi_equals_the_restatement(w, N, S):
    rng = np.random.default_rng(N * 2000 + S)
    U = (rng.random((N, S)) * 10).astype(np.float32)
    T = (rng.random((S, S)) * 3).astype(np.float32)
    check_path(w, U, T)
    check_path(w, np.round(U), np.round(T))                              # many exact ties: the lowest index wins


def test_viterbi_ties_infinities_and_frames_without_evidence(w):
    rng = np.random.default_rng(5)
    S = 9
    T = (rng.random((S, S)) * 3).astype(np.float32)
    assert check_path(w, np.full((4, S), 2.5, np.float32), np.full((S, S), 1.25, np.float32)).tolist() == [0, 0, 0, 0]   # all equal
    U = (rng.random((6, S)) * 10).astype(np.float32)
    U[rng.random((6, S)) < 0.3] = np.inf
    assert np.isfinite(U).any(1).all()
    check_path(w, U, T)                                                  # some +inf entries
    for rows in ([2], [0], [5], [0, 2, 3, 5]):
        V = U.copy()
        V[rows] = np.inf
        zero = V.copy()
        zero[rows] = 0.0
        assert check_path(w, V, T).tolist() == pr.viterbi(zero, T)[0].tolist()      # a frame without evidence is a row of zeros
    # a near-tie: frame 2 prefers state 4 by less than the step there and back costs, so the path stays
    U = np.full((5, S), 50.0, np.float32)
    U[:, 1] = 1.0
    U[2, 4] = 0.5
    T = (2.0 * (1.0 - np.eye(S))).astype(np.float32)
    assert check_path(w, U, T).tolist() == [1, 1, 1, 1, 1]
    U[2, 4] = -3.5                                                       # ... and leaves once the gain beats 2 x 2
    assert check_path(w, U, T).tolist() == [1, 1, 4, 1, 1]
    with pytest.raises(ValueError, match="1024"):
        w.pi.viterbi(torch.zeros(2, 1025, device=DEV), torch.zeros(1025, 1025, device=DEV))


@pytest.mark.parametrize("valid", [[1, 0, 1, 0, 0, 1, 1], [0, 1, 1, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0, 0], [1] * 7, [0] * 7], ids=str)
def test_the_translation_fill(w, valid):
    """One-frame and two-frame gaps, both ends, a single valid frame, all and none."""
    rng = np.random.default_rng(9)
    N, S = 7, 5
    U, T = (rng.random((N, S)) * 10).astype(np.float32), (rng.random((S, S)) * 3).astype(np.float32)
    tr = rng.standard_normal((N, S, 3)).astype(np.float32)
    v = np.array(valid, bool)
    res = w.pi.viterbi_path(torch.from_numpy(U).to(DEV), torch.from_numpy(T).to(DEV), torch.from_numpy(tr).to(DEV), torch.from_numpy(v).to(DEV))
    rp, rt, _ = pr.viterbi(U, T)
    assert res.path.tolist() == rp.tolist() and np.float32(res.total.item()) == rt and res.transl_path.shape == (N, 3)
    f32, f64 = pr.fill(tr, rp, v, np.float32), pr.fill(tr, rp, v, np.float64)
    sr.bar_check(f"fill {valid}", res.transl_path, f32, f64)
    for n in np.nonzero(v)[0]:
        assert np.array_equal(res.transl_path[n].cpu().numpy(), tr[n, rp[n]])


# ---- end to end ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("yaws", [12, 24])
@pytest.mark.parametrize("b", [0, 1])
def test_init_from_keypoints_picks_a_bracketing_yaw(w, yaws, b, tmp_path):
    sc = pr.offbank_scene(w.m, w.tables, w.c, yaws, b)
    R = pr.yaw_bank(yaws).float()
    init, Ks, info = w.pi.init_from_keypoints(w.rig, sc["targets"].float().to(DEV), w.c["img_wh"], sc["Ks"].to(DEV), w.c["w2c"].to(DEV), rotations=R.to(DEV))
    assert bool(info.valid.all()) and bool(torch.isfinite(info.cost).all())
    for n, s in enumerate(info.path.tolist()):
        assert s // yaws == b and s % yaws in sc["brackets"][n], (n, s, sc["brackets"][n])
    # load_smplerx's keys and shapes, rotation vectors; through save_params unchanged
    shapes = {"betas": (6, 10), "global_orient": (6, 3), "body_pose": (6, 63), "left_hand_pose": (6, 45), "right_hand_pose": (6, 45),
              "jaw_pose": (6, 3), "leye_pose": (6, 3), "reye_pose": (6, 3), "expression": (6, 10), "transl": (6, 3)}
    assert {k: tuple(v.shape) for k, v in init.items()} == shapes
    assert torch.allclose(w.smplify.rotvec_to_rotmat(init["global_orient"]).cpu(), R[info.path.cpu() % yaws], atol=1e-5)
    assert torch.equal(init["body_pose"].cpu(), pr.golden_base_poses(torch.float32)[[b] * 6]) and not bool(init["betas"].any())
    w.smplify.save_params(str(tmp_path / "params.pth"), init, Ks, w.c["w2c"], w.c["img_wh"])
    back = torch.load(str(tmp_path / "params.pth"))
    assert set(back) == set(shapes) | {"Ks", "w2c", "img_wh"} and all(torch.equal(back[k], init[k].cpu()) for k in shapes)
    # without Ks the project's rule stands in
    _, K0, _ = w.pi.init_from_keypoints(w.rig, sc["targets"].float().to(DEV), w.c["img_wh"], rotations=R.to(DEV))
    assert torch.equal(K0.cpu(), w.pi.default_intrinsics(6, w.c["img_wh"]))


def fit_scene(w):
    sc = pr.offbank_scene(w.m, w.tables, w.c, 24, 1, step=0)
    return sc["targets"].float(), sc["Ks"], pr.yaw_bank(24).float()


def test_the_low_prior_stage_does_not_leave_the_searched_keypoint_loss(w):
    """After ``SMPLify(rig, hand_steps=0, preserve_weight=prior_weight).fit`` from the searched start the total objective is at most
    the keypoint loss at the searched parameters: the preserve term starts at 0 there and strong-Wolfe L-BFGS does not increase
    the objective."""
    target, Ks, R = fit_scene(w)
    wh, w2c = w.c["img_wh"], w.c["w2c"].to(DEV)
    init, Ks, info = w.pi.init_from_keypoints(w.rig, target.to(DEV), wh, Ks.to(DEV), w2c, rotations=R.to(DEV))
    fit = w.smplify.SMPLify(w.rig, hand_steps=0, preserve_weight=w.pi.PRIOR_WEIGHT, body_steps=2, max_iters=8)
    fit.fit(init, Ks, w2c, wh, target.to(DEV))
    init6 = {k: (w.smplify.rotation_6d_from_rotvec(v.reshape(6, -1, 3)) if k in sr.POSE_KEYS else v) for k, v in init.items()}
    init6["betas"] = init6["betas"].mean(0, keepdim=True)
    scales = w.smplify.target_scales(target.to(DEV), wh)
    weights = (100.0, w.pi.PRIOR_WEIGHT, 10000.0)
    start = w.smplify.smplify_objective(w.rig, init6, init6, Ks, w2c, wh, target.to(DEV), scales, weights, ignore_hands=True).losses
    end = w.smplify.smplify_objective(w.rig, fit.params_6d, init6, Ks, w2c, wh, target.to(DEV), scales, weights, ignore_hands=True).losses
    print(f"low-prior stage: start kp {float(start[0]):.6g} preserve {float(start[1]):.6g} smooth {float(start[2]):.6g}; "
          f"end kp {float(end[0]):.6g} preserve {float(end[1]):.6g} smooth {float(end[2]):.6g}; {fit.evaluations} evaluations")
    assert float(start[1]) == 0.0
    assert float(end.sum()) <= float(start[0])


def test_fit_from_keypoints_three_ways(w, tmp_path):
    """The same stages driven by the HIP objective and by the float32 and float64 restatements (the search is HIP in all three); the
    float64 objective against the searched start at each drive's final parameters.  The yardstick is the float32 drive, the margin
    twice the distance between the float32 and the float64 drive: what float32 arithmetic alone moves an L-BFGS trajectory.

    Measured on an MI355X (N = 6, 2 low-prior steps, then 1 + 2 steps, at most 8 iterations each; searched start 1026.7): HIP
    64.1321, float32 restatement 63.8508, float64 restatement 64.1343; 50 / 49 / 50 closure evaluations.  The HIP drive lies 0.281
    above the float32 drive; the margin is 2 x 0.2835 = 0.567."""
    target, Ks, R = fit_scene(w)
    wh, w2c = w.c["img_wh"], w.c["w2c"]
    steps = dict(prior_fit=dict(body_steps=2, max_iters=8), fit=dict(body_steps=1, hand_steps=2, max_iters=8))

    def restated(dtype, device):
        def objective(rig, params, init, Ks_, w2c_, img_wh, tk, scales, weights, sigma, ignore_hands):
            ls, gr = sr.objective(w.m, w.tables, params, init, Ks_, w2c_, img_wh, tk, scales, dtype=dtype, device=device, weights=weights,
                                  sigma=sigma, ignore_hands=ignore_hands)
            return types.SimpleNamespace(losses=torch.stack([ls[k] for k in ("kp", "preserve", "smooth")]), grads=gr)
        return lambda **kw: w.smplify.SMPLify(types.SimpleNamespace(device=torch.device(device)), objective=objective,
                                              scales=lambda t, img_wh: sr.target_scales(t, img_wh), dtype=dtype, **kw)

    makers = {"hip": lambda **kw: w.smplify.SMPLify(w.rig, **kw), "f32": restated(torch.float32, DEV), "f64": restated(torch.float64, "cpu")}
    init, _, _ = w.pi.init_from_keypoints(w.rig, target.to(DEV), wh, Ks.to(DEV), w2c.to(DEV), rotations=R.to(DEV))
    init6 = {k: (w.smplify.rotation_6d_from_rotvec(v.reshape(6, -1, 3)) if k in sr.POSE_KEYS else v).cpu() for k, v in init.items()}
    init6["betas"] = init6["betas"].mean(0, keepdim=True)
    scales = sr.target_scales(target.double(), wh)

    def f64_objective(six):
        ls, _ = sr.objective(w.m, w.tables, {k: v.cpu() for k, v in six.items()}, init6, Ks, w2c, wh, target, scales)
        return float(sum(ls.values()))

    final, evals = {}, {}
    for name, make in makers.items():
        made = []
        res = w.pi.fit_from_keypoints(w.rig, target.to(DEV), wh, Ks.to(DEV), w2c.to(DEV), rotations=R.to(DEV),
                                      make_fit=lambda **kw: (made.append(make(**kw)), made[-1])[1], **steps)
        assert len(made) == 2 and made[0].weights[1] == w.pi.PRIOR_WEIGHT and made[1].weights[1] == 60.0
        assert res.params["global_orient"].shape == (6, 3) and res.params["body_pose"].shape == (6, 63) and res.params["betas"].shape == (1, 10)
        final[name], evals[name] = f64_objective(made[1].params_6d), made[0].evaluations + made[1].evaluations
        if name == "hip":
            w.smplify.save_params(str(tmp_path / "params.pth"), res.params, res.Ks, res.w2c, res.img_wh)
            assert set(torch.load(str(tmp_path / "params.pth"))) == set(sr.PARAM_KEYS) | {"Ks", "w2c", "img_wh"}
    initial = f64_objective(init6)
    print(f"fit_from_keypoints: searched start {initial:.6g}; final hip {final['hip']:.6g} f32 {final['f32']:.6g} f64 {final['f64']:.6g} "
          f"(closure evaluations: {evals})")
    assert final["hip"] < initial
    assert final["hip"] - final["f32"] <= 2.0 * abs(final["f32"] - final["f64"])
