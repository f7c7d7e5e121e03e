"""Seeded densification cases for tests/test_densify_cases_cpu.py and tests/test_densify_layout_gpu.py.  CPU only.

``make_case`` builds a model of P surfels (the seven parameter tensors, Adam moments, views of statistics, thresholds, split noise)
whose random rows prune, clone and split a sizeable share each, and -- from P = 64 on -- overwrites a few dozen *designated rows*,
scattered through the index range, that each pin one decision of the plan kernel: a threshold hit exactly and one ulp either side,
``denom == 0``, NaN and negative accumulators, the scale-pruning branches, prune against clone / split, degenerate rotations.
The designated rows get their accumulators written directly, after the statistics pass (``accumulate``).

``single_pass`` restates the state machine over the *original* indices -- the form the fused plan of csrc/densify.hip uses -- next
to the reference's two-call form in oracle/densify_oracle.py; test_densify_cases_cpu.py holds the two together.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import densify_oracle as do

EXTENT, PERCENT_DENSE, MIN_OPACITY = 1.3, 0.01, 0.1
MAX_GRAD = 2.0 ** -12                      # exact in float32: rows can sit on it and one ulp either side
SMALL, BIG = 0.004, 0.02                   # exp(scaling) below / above percent_dense * extent = 0.013
KEEP, PRUNE, CLONE, SPLIT = 0, 1, 2, 4     # the plan's flag byte

# what the GPU file runs; the CPU file checks the builder on exactly these
SIZE_CASES = [(1, 11), (2, 12), (255, 13), (256, 14), (257, 15), (4099, 16), (70001, 17), (300007, 18)]           # (P, seed)
NS_CASES = [(4099, 20 + N + int(surface), N, surface) for N in (1, 3, 5) for surface in (True, False)]          # (P, seed, N, surface)
UNIFORM_CASES = [(513, 31, kind) for kind in ("keep", "clone", "split", "prune", "alternate")]                  # (P, seed, kind)
STATS_CASES = [(257, 41), (70001, 42)]                                                                          # five views, radii from -3
STRIDE_CASES = [(257, 50 + s, s) for s in (2, 3, 4)]                                                            # (P, seed, grad_stride)
LIMIT_P = 2 ** 21 - 1

_f32 = np.float32
_up = lambda x: float(np.nextafter(_f32(x), _f32(np.inf)))
_down = lambda x: float(np.nextafter(_f32(x), _f32(-np.inf)))
_UNIT = (1.0, 0.0, 0.0, 0.0)


def _designated_rows():
    """(name, exp(scaling) per column, opacity, rotation, (accum xyz, scale, opac, denom), flag with pruning, flag without)."""
    S, B, hot = (SMALL,) * 3, (BIG,) * 3, 4 * MAX_GRAD
    rows = []

    def add(name, scale, accum, with_prune, without, opacity=2.0, rot=_UNIT):
        rows.append((name, scale, opacity, rot, accum, with_prune, without))
    # 1. the positional gradient on max_grad (>=), one ulp below and above; denom = 1
    for tag, size, flag in (("small", S, CLONE), ("big", B, SPLIT)):
        add(f"gp == max_grad, {tag}", size, (MAX_GRAD, 0, 0, 1), flag, flag)
        add(f"gp one ulp below max_grad, {tag}", size, (_down(MAX_GRAD), 0, 0, 1), KEEP, KEEP)
        add(f"gp one ulp above max_grad, {tag}", size, (_up(MAX_GRAD), 0, 0, 1), flag, flag)
    # 2. the clone pre-mask: go <= 2 and gs <= float32(1e-7); neither holds a split back
    add("go == 2", S, (hot, 0, 2.0, 1), CLONE, CLONE)
    add("go one ulp above 2", S, (hot, 0, _up(2.0), 1), KEEP, KEEP)
    add("gs == float32(1e-7)", S, (hot, float(_f32(1e-7)), 0, 1), CLONE, CLONE)
    add("gs one ulp above float32(1e-7)", S, (hot, _up(1e-7), 0, 1), KEEP, KEEP)
    add("go and gs large, big point", B, (hot, 1.0, 5.0, 1), SPLIT, SPLIT)
    # 3. never visible: 0/0 -> 0, x/0 = inf stays
    add("denom 0, zero accumulators, small", S, (0, 0, 0, 0), PRUNE, KEEP)
    add("denom 0, zero accumulators, big", B, (0, 0, 0, 0), PRUNE, KEEP)
    add("denom 0, gp inf, go 0/0, small", S, (1.0, 0, 0, 0), PRUNE, CLONE)
    add("denom 0, gp inf, go inf, small", S, (1.0, 0, 1.0, 0), PRUNE, KEEP)
    add("denom 0, gp inf, big", B, (1.0, 0, 1.0, 0), PRUNE, SPLIT)
    # 4. NaN -> 0 before either test; a negative gradient clones (|gp|) but does not split (signed gp)
    add("NaN accumulator, small", S, (float("nan"), 0, 0, 1), KEEP, KEEP)
    add("NaN accumulator, big", B, (float("nan"), 0, 0, 1), KEEP, KEEP)
    add("negative accumulator, small", S, (-1e3, 0, 0, 1), CLONE, CLONE)
    add("negative accumulator, big", B, (-1e3, 0, 0, 1), KEEP, KEEP)
    # 5. pruned by scale (columns 0 and 1 only); 6. prune wins over clone and over split
    add("smax > 0.5 extent, cold", (0.7, BIG, BIG), (0, 0, 0, 1), PRUNE, KEEP)
    add("smax > 0.5 extent in column 1, split-flagged", (BIG, 0.7, BIG), (hot, 0, 0, 1), PRUNE, SPLIT)
    add("sx * sy < 1e-8 extent^2, cold", (1e-4, 1e-4, SMALL), (0, 0, 0, 1), PRUNE, KEEP)
    add("sx * sy < 1e-8 extent^2, clone-flagged", (1e-5, 1e-3, SMALL), (hot, 0, 0, 1), PRUNE, CLONE)
    add("large third column alone, hot", (SMALL, SMALL, 0.7), (hot, 0, 0, 1), SPLIT, SPLIT)
    add("large third column alone, cold", (SMALL, SMALL, 0.7), (0, 0, 0, 1), KEEP, KEEP)
    add("low opacity, clone-flagged", S, (hot, 0, 0, 1), PRUNE, CLONE, opacity=-4.0)
    add("low opacity, split-flagged", B, (hot, 0, 0, 1), PRUNE, SPLIT, opacity=-4.0)
    # 7. rotations far from unit length and all zero (0/0: NaN children in the reference and here)
    add("split, rotation of length 13", B, (hot, 0, 0, 1), SPLIT, SPLIT, rot=(3.0, -4.0, 12.0, 0.0))
    add("split, tiny rotation", (BIG, SMALL, BIG), (hot, 0, 0, 1), SPLIT, SPLIT, rot=(1e-3, 2e-3, -1e-3, 5e-4))
    add("split, zero rotation", B, (hot, 0, 0, 1), SPLIT, SPLIT, rot=(0.0, 0.0, 0.0, 0.0))
    add("clone, zero rotation", S, (hot, 0, 0, 1), CLONE, CLONE, rot=(0.0, 0.0, 0.0, 0.0))
    return rows


def _randn(g, *shape):
    return torch.randn(*shape, generator=g).clamp_(-3, 3)


def _margins(params):
    """float64 relative distance of every quantity that is thresholded after exp / sigmoid to its threshold, [P, 8]."""
    s = torch.exp(params["scaling"].double())
    op = torch.sigmoid(params["opacity"].double())[:, 0]
    smin, smax = s[:, :2].min(1).values, s[:, :2].max(1).values
    rel = lambda q, t: (q - t).abs() / t
    dense = PERCENT_DENSE * EXTENT
    return torch.stack([rel(op, MIN_OPACITY), rel(smax, 0.5 * EXTENT), rel(smin, 0.5 * EXTENT), rel(smin * smax, 1e-8 * EXTENT ** 2),
                        rel(s[:, 0], dense), rel(s[:, 1], dense), rel(s[:, 2], dense), rel(s.max(1).values, dense)], 1)


def make_case(P, seed, N=2, surface=True, n_views=3, grad_stride=3, radii_low=-1, designated=True):
    """A namespace with params, m, v (name -> tensor), views [(radii, grad2d [P, grad_stride], scaling_grad [P, 3])], noise [N P, 3],
    the thresholds, margins [P, 8] (see _margins) and the designated rows: rows (indices), row_names, row_accum [5, D] and
    row_flags [2, D] (the flag each row is built for, with pruning and without).  About one point in five is pruned (low opacity;
    3 % are in no view at all), two in five are big, three in four have a gradient above max_grad."""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *s: torch.rand(*s, generator=g)
    params = dict(xyz=0.5 * _randn(g, P, 3), f_dc=_randn(g, P, 1, 3), f_rest=_randn(g, P, 3, 3), color=_randn(g, P, 3),
                  opacity=torch.where(rand(P, 1) < 0.2, -4.0, 2.0) + 0.2 * _randn(g, P, 1),
                  scaling=torch.log(torch.where(rand(P, 1) < 0.4, BIG, SMALL)) + 0.1 * _randn(g, P, 3), rotation=_randn(g, P, 4))
    m = {k: 1e-3 * _randn(g, *t.shape) for k, t in params.items()}
    v = {k: 1e-6 * rand(*t.shape) for k, t in params.items()}
    hot, hidden = rand(P) < 0.75, rand(P) < 0.03          # hidden: in no view at all
    views = []
    for _ in range(n_views):
        radii = torch.randint(radii_low, 9, (P,), generator=g, dtype=torch.int32)
        radii[hidden] = radii[hidden].clamp(max=0)
        phi = 2 * np.pi * rand(P)
        norm = torch.where(hot, 3e-3, 1e-5) * (1 + 0.1 * _randn(g, P))
        grad2d = _randn(g, P, grad_stride)
        grad2d[:, 0], grad2d[:, 1] = norm * torch.cos(phi), norm * torch.sin(phi)
        if grad_stride > 3:
            grad2d[:, 2:] = float("nan")                 # never read
        views.append((radii, grad2d, 1e-3 * (rand(P, 3) - 0.65)))
    case = SimpleNamespace(P=P, seed=seed, N=N, surface=surface, params=params, m=m, v=v, views=views, noise=_randn(g, N * P, 3),
                           extent=EXTENT, percent_dense=PERCENT_DENSE, max_grad=MAX_GRAD, min_opacity=MIN_OPACITY,
                           rows=torch.zeros(0, dtype=torch.long), row_names=[], row_accum=torch.zeros(5, 0),
                           row_flags=torch.zeros(2, 0, dtype=torch.uint8))
    if designated and P >= 64:
        rows = _designated_rows()
        # first and last row and both sides of the first workgroup boundary, then a seeded scatter over the rest
        first = list(dict.fromkeys(i for i in (0, 255, 256, 511, 512, P - 1) if i < P))
        rest = [i for i in torch.randperm(P, generator=g).tolist() if i not in first]
        order = torch.randperm(len(rows), generator=g).tolist()
        _designate(case, (first + rest)[: len(rows)], [rows[j] for j in order])
    case.margins = _margins(params)
    return case


def _designate(case, index, rows):
    case.rows = torch.tensor(index, dtype=torch.long)
    case.row_names = [r[0] for r in rows]
    accum = torch.zeros(5, len(rows))
    for j, (_, scale, opacity, rot, (a_xyz, a_scale, a_opac, denom), _, _) in enumerate(rows):
        i = index[j]
        case.params["scaling"][i] = torch.log(torch.tensor(scale, dtype=torch.float64)).float()
        case.params["opacity"][i] = opacity
        case.params["rotation"][i] = torch.tensor(rot)
        accum[:, j] = torch.tensor([a_xyz, a_scale, 1.0, a_opac, denom])
    case.row_accum = accum
    case.row_flags = torch.tensor([[r[5] for r in rows], [r[6] for r in rows]], dtype=torch.uint8)


def uniform_case(P, seed, kind):
    """Every row designated: all kept, all cloned, all split, all pruned (never visible), or clone / split alternating."""
    case = make_case(P, seed, designated=False)
    S, B = (SMALL,) * 3, (BIG,) * 3
    row = {"keep": ("kept", S, 2.0, _UNIT, (0, 0, 0, 1), KEEP, KEEP), "clone": ("cloned", S, 2.0, _UNIT, (1.0, 0, 0, 1), CLONE, CLONE),
           "split": ("split", B, 2.0, _UNIT, (1.0, 0, 0, 1), SPLIT, SPLIT), "prune": ("never visible", S, 2.0, _UNIT, (0, 0, 0, 0), PRUNE, KEEP)}
    rotation = case.params["rotation"].clone()
    _designate(case, list(range(P)), [row[("clone", "split")[i % 2] if kind == "alternate" else kind] for i in range(P)])
    case.params["rotation"] = rotation                   # keep the random rotations: the children then differ from their parents
    case.margins = _margins(case.params)
    return case


# ---- the pinned restatement on a case ------------------------------------------------------------------------------------------
def oracle_state(case):
    return do.new_state(case.params, case.m, case.v)


def accumulate(case, st):
    """The statistics pass over the case's views, then the designated rows' accumulators written directly."""
    for radii, grad2d, sgrad in case.views:
        do.add_densification_stats(st, radii, grad2d, sgrad)
    return pin_rows(case, st)


def pin_rows(case, st):
    for a, k in enumerate(do.ACCUMS):
        st[k][case.rows, 0] = case.row_accum[a]
    return st


def accum_matrix(st):
    return torch.stack([st[k][:, 0] for k in do.ACCUMS])


def two_calls(case, st, do_prune=True, noise=None):
    """adaptive_prune (if do_prune) then adaptive_densify, as the reference calls them.  Returns the masks over the original rows
    (clone and split over the survivors) and, in st, the new model."""
    noise = case.noise if noise is None else noise
    pruned = do.adaptive_prune(st, case.min_opacity, case.extent) if do_prune else torch.zeros(case.P, dtype=torch.bool)
    masks = do.adaptive_densify(st, case.max_grad, case.extent, case.percent_dense, case.surface, noise, case.N)
    return pruned, masks["clone"], masks["split"]


def flags_of(pruned, clone, split):
    """The plan's flag byte per original row from the two-call form's masks."""
    f = pruned.to(torch.uint8) * PRUNE
    f[~pruned] = clone.to(torch.uint8) * CLONE + split.to(torch.uint8) * SPLIT
    return f


def single_pass(case, st, do_prune=True, do_densify=True, noise=None):
    """One pass over the original indices: decisions per row from its own accumulators, then the layout
    [kept and not split | clones | split children, repetition-major].  Returns (flags, params, m, v)."""
    noise = case.noise if noise is None else noise
    p, N = st["params"], case.N
    s = torch.exp(p["scaling"])
    denom = st["denom"][:, 0]
    prune = torch.zeros(s.shape[0], dtype=torch.bool)
    if do_prune:
        smin, smax = s[:, :2].min(1).values, s[:, :2].max(1).values
        prune = ((torch.sigmoid(p["opacity"])[:, 0] < case.min_opacity) | (denom == 0) | (smax > 0.5 * case.extent)
                 | (smin * smax < 1e-8 * case.extent ** 2))

    def ratio(k):
        r = st[k][:, 0] / denom
        r[r.isnan()] = 0.0
        return r
    clone = split = torch.zeros_like(prune)
    if do_densify:
        gp, gs, go = ratio("xyz_gradient_accum"), ratio("scale_gradient_accum"), ratio("opac_gradient_accum")
        big = s.max(1).values > case.percent_dense * case.extent
        clone = (gp.abs() >= case.max_grad) & ~big & (go <= 2) & (gs <= 1e-7) & ~prune
        split = (gp >= case.max_grad) & big & ~prune
    flags = prune.to(torch.uint8) * PRUNE + clone.to(torch.uint8) * CLONE + split.to(torch.uint8) * SPLIT
    keep_i, clone_i, split_i = [torch.nonzero(x)[:, 0] for x in (~prune & ~split, clone, split)]
    src = torch.cat([keep_i, clone_i, split_i.repeat(N)])
    out = {k: p[k][src] for k in do.PARAMS}
    n_child = N * split_i.numel()
    if n_child:
        samples = noise[:n_child] * s[split_i].repeat(N, 1)
        rots = do.build_rotation(p["rotation"][split_i]).repeat(N, 1, 1)
        out["xyz"][-n_child:] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p["xyz"][split_i].repeat(N, 1)
        out["scaling"][-n_child:] = torch.log(s[split_i].repeat(N, 1) / (0.8 * N))
        if case.surface:
            out["scaling"][-n_child:, -1] = -1e10
    new = src.numel() - keep_i.numel()
    moments = [{k: torch.cat([st[grp][k][keep_i], torch.zeros((new,) + tuple(p[k].shape[1:]))]) for k in do.PARAMS} for grp in ("m", "v")]
    return flags, out, moments[0], moments[1]
