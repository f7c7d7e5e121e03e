"""Scenes for the attribute field's edge tests (tests/test_field_edges_gpu.py; verified on the CPU by
tests/test_field_cases_cpu.py).  Everything here is built on the CPU and importable without a GPU.

**Exact scenes.**  Inputs on a dyadic grid, so that every product and every partial sum of the offsets head's forward and backward
is a float32 number: normalised points on quarters (or eighths), integer tables in [-4, 4], first-layer rows of the offsets head
with 4 entries of +-1, second-layer rows with 8, integer biases in [-2, 2], z = (0.5, -0.25) and integer upstream gradients on the
offsets head alone.  With points on 2^-a the corner weights lie on the grid 2^-3a (2^-6 for quarters, 2^-9 for eighths), and so
does everything summed from them.  As long as the summed magnitudes of an accumulated element stay below 2^23 grid units
(``exactness_margin``), no order of summation can round: the kernels, atomics included, must equal the float64 restatement bit
for bit.

**Point orders** steer what the lanes of a wave see in the scatter's ``wave_add`` (blocks of 128 threads = 2 waves; the head
backward takes chunks of 64 points, two per block): ``one_point``, ``runs``, ``alternating``, ``coarse_shared``, ``outside``,
``box_edges``.  ``coarse_shared`` needs neighbours less than a cell apart: points on eighths under levels 2 .. 64 (at the default
coarsest level, 16, dyadic points a quarter apart are four cells apart).  ``box_edges`` is in aabb mode, lo = -1, hi = 3, so that
p = (x + 1) / 4 is exact.

**Real scenes** (``real_scene``) are the random field of tests/test_field_gpu.py at any table size and level range."""
import types
import zlib

import torch

import field_ref as R
from soar_amd import synthetic as syn
from soar_amd.field import HashMLPField

SIZES = (1, 63, 64, 65, 127, 128, 129, 130, 257, 777)
EXACT_LOG2_T = (1, 4, 10)
ORDERS = ("one_point", "runs", "alternating", "coarse_shared", "outside", "box_edges")
RUN_LENGTHS = (1, 2, 3, 5, 31, 32, 33)
# 31 + 33 ends a run on lane 63 of the first wave; 1 + 2 + 3 + 5 + 32 = 43, so the next 33 runs over points 107 .. 139, from lane
# 63 of the second wave into lane 0 of the third; then RUN_LENGTHS over and over (the run 182 .. 213 crosses the two waves of a block)
RUN_LAYOUT_HEAD = (31, 33, 1, 2, 3, 5, 32, 33)
WAVE = 64
COARSE = dict(base_res=2, max_res=64)
BOX = ((-1.0, -1.0, -1.0), (3.0, 3.0, 3.0))
ORDER_CONFIG = {
    "one_point": dict(normalized=True), "runs": dict(normalized=True), "alternating": dict(normalized=True),
    "coarse_shared": dict(normalized=True, **COARSE), "outside": dict(normalized=True), "box_edges": dict(normalized=False, aabb=BOX),
}
ONE_POINT = (0.25, 0.75, 0.5)
ALTERNATING = ((0.25, 0.5, 0.75), (0.75, 0.25, 0.5))
Z = (0.5, -0.25)


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def quarter_pool():
    """[1331, 3]: every point k / 4 with k in -3 .. 7 on each axis"""
    k = torch.arange(-3, 8, dtype=torch.float32) / 4
    return torch.cartesian_prod(k, k, k)


def run_lengths(N):
    """the lengths of the runs of ``runs`` at N points (the last one cut off at N)"""
    out, total, i = [], 0, 0
    while total < N:
        n = RUN_LAYOUT_HEAD[i] if i < len(RUN_LAYOUT_HEAD) else RUN_LENGTHS[(i - len(RUN_LAYOUT_HEAD)) % len(RUN_LENGTHS)]
        n = min(n, N - total)
        out.append(n)
        total += n
        i += 1
    return out


def one_point(N, seed=0):
    return torch.tensor(ONE_POINT).expand(N, 3).contiguous()


def runs(N, seed=0):
    """runs of equal points, each run another point of the quarter lattice (so no two runs share a level-0 cell)"""
    pool = quarter_pool()
    lengths = run_lengths(N)
    pick = torch.randperm(pool.shape[0], generator=_gen("runs", seed))[:len(lengths)]
    return torch.repeat_interleave(pool[pick], torch.tensor(lengths), dim=0).contiguous()


def alternating(N, seed=0):
    return torch.tensor(ALTERNATING)[torch.arange(N) % 2].contiguous()


def coarse_shared(N, seed=0):
    """points on eighths, for levels 2 .. 64: groups of 16 neighbours inside one cell of the coarsest level (a / 8 with a in
    1 .. 3, or 5 .. 7, on every axis), no two neighbours equal on x"""
    g = _gen("coarse", seed)
    n = torch.arange(N)
    octant = torch.randint(0, 2, ((N + 15) // 16, 3), generator=g)[n // 16]
    a = torch.randint(1, 4, (N, 3), generator=g)
    a[:, 0] = 1 + n % 3
    return ((a + 4 * octant).to(torch.float32) / 8).contiguous()


def _beyond(closed):
    pool = quarter_pool()
    out = ((pool <= 0) | (pool >= 1)) if closed else ((pool < 0) | (pool > 1))
    return pool[out.any(dim=1)]


def outside(N, seed=0):
    """normalised points with a coordinate below 0 or above 1"""
    pool = _beyond(False)
    return pool[torch.randint(0, pool.shape[0], (N,), generator=_gen("outside", seed))].contiguous()


def box_edges(N, seed=0):
    """world points of the box lo = -1, hi = 3 that lie outside it or exactly on a face (p <= 0 or p >= 1 on some axis)"""
    pool = _beyond(True)
    return (4 * pool[torch.randint(0, pool.shape[0], (N,), generator=_gen("box", seed))] - 1).contiguous()


def box_mixed(N, seed=0):
    """``box_edges`` with every other group of 5 points replaced by one point strictly inside the box (a run of selected points
    between runs that are all encoded at the origin) -> (world points, selected)"""
    pool = quarter_pool()
    pool = pool[((pool > 0) & (pool < 1)).all(dim=1)]
    n = torch.arange(N)
    pick = torch.randint(0, pool.shape[0], ((N + 4) // 5,), generator=_gen("mixed", seed))
    inside = (n // 5) % 2 == 0
    return torch.where(inside[:, None], 4 * pool[pick[n // 5]] - 1, box_edges(N, seed)).contiguous(), inside


BUILDERS = dict(one_point=one_point, runs=runs, alternating=alternating, coarse_shared=coarse_shared, outside=outside,
                box_edges=box_edges)
_fields = {}


def _sparse_signs(rows, cols, per_row, g):
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:per_row]
        w[r, idx] = (torch.randint(0, 2, (per_row,), generator=g) * 2 - 1).to(torch.float32)
    return w


def exact_field(log2_T, base_res=16, max_res=2048, aabb=None, seed=0):
    """A CPU HashMLPField with integer tables in [-4, 4] and the offsets head's weights sparse +-1 (4 per first-layer row, 8 per
    second-layer row) with integer biases in [-2, 2].  The other heads keep their random initial weights: they get no upstream
    gradient in an exact scene.  Small fields are built once and shared: leave them unchanged."""
    key = (log2_T, base_res, max_res, aabb, seed)
    if key in _fields:
        return _fields[key]
    g = _gen("field", log2_T, base_res, max_res, seed)
    box = torch.tensor(aabb if aabb is not None else ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)))
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        f = HashMLPField(box, base_res=base_res, max_res=max_res, log2_hashmap_size=log2_T)
    rows = 16 * 2 ** log2_T
    with torch.no_grad():
        f.encoding.hash_table.copy_(torch.randint(-4, 5, (rows, 2), generator=g).float())
        f.quat_encoding.hash_table.copy_(torch.randint(-4, 5, (rows, 2), generator=g).float())
        m = f.mlp_base_offsets
        m.layers[0].weight.copy_(_sparse_signs(64, 34, 4, g))
        m.layers[0].bias.copy_(torch.randint(-2, 3, (64,), generator=g).float())
        m.layers[1].weight.copy_(_sparse_signs(3, 64, 8, g))
        m.layers[1].bias.copy_(torch.randint(-2, 3, (3,), generator=g).float())
    if log2_T <= 12:
        _fields[key] = f
    return f


def _grid_of(p):
    """points on 2^-a give corner weights, and everything summed from them, on 2^-3a (never coarser than 2^-6)"""
    for a in range(2, 5):
        if bool((p * 2 ** a == torch.round(p * 2 ** a)).all()):
            return 2.0 ** (-3 * a)
    raise ValueError("exact scenes take points on quarters, eighths or sixteenths")


def exact_scene(log2_T, points, normalized=True, base_res=16, max_res=2048, aabb=None, seed=0):
    """The dyadic scene: ``points`` [N, 3] float32 as the field is called with them (world points with ``aabb`` = (lo, hi) and
    ``normalized=False``).  -> field (CPU), points, z, g (the integer upstream gradient of the offsets head), loss, grid"""
    points = points.to(torch.float32).contiguous()
    f = exact_field(log2_T, base_res, max_res, aabb, seed)
    p = points if normalized else (points - f.aabb[0]) / (f.aabb[1] - f.aabb[0])
    N = points.shape[0]
    g = torch.randint(-2, 3, (N, 3), generator=_gen("upstream", seed, N)).float()
    return types.SimpleNamespace(field=f, points=points, normalized=normalized, log2_T=log2_T, T=2 ** log2_T, res=f.encoding.scalings.clone(),
                                 z=torch.tensor(Z), g=g, grid=_grid_of(p), p=p)


def exact_case(order, log2_T, N, seed=0):
    return exact_scene(log2_T, BUILDERS[order](N, seed), seed=seed, **ORDER_CONFIG[order])


def exact_cases():
    """every (order, log2_T, N) that the GPU tests run bit for bit, and the two large tables"""
    return [(o, t, n) for o in ORDERS for t in EXACT_LOG2_T for n in SIZES] + [("runs", 18, 777), ("alternating", 19, 257)]


def offsets_loss(g):
    return lambda out: (out["offsets"] * g.to(out["offsets"].device, out["offsets"].dtype)).sum()


EXACT_NAMES = ("encoding.hash_table", "z") + tuple(f"mlp_base_offsets.{n}" for n in R.PARAM_NAMES)


def restate(scene, dtype, perm=None, device=None):
    """the restatement of an exact scene in ``dtype`` -> {"offsets": the output, and the gradients of EXACT_NAMES}.  ``perm``
    runs the points (and their upstream gradients) in another order; the output comes back in the scene's."""
    N = scene.points.shape[0]
    perm = torch.arange(N) if perm is None else perm
    z = scene.z.clone().requires_grad_(True)
    out, grads = R.run(scene.field, scene.points[perm], z, offsets_loss(scene.g[perm]), False, dtype, scene.normalized, device=device)
    offs = torch.empty_like(out["offsets"].detach())
    offs[perm.to(offs.device)] = out["offsets"].detach()
    res = {"offsets": offs}
    res.update({n: grads[n] for n in EXACT_NAMES})
    return res


def exactness_margin(scene):
    """The largest sum of magnitudes that any accumulated element of the scene collects, in units of the scene's grid: the rows
    of the table gradient (sum over points and corners of |w| |dL/de|), the offsets head's weight and bias gradients, dL/dz, and
    the forward's own sums.  From the float64 restatement: dL/de and dL/dh by autograd with ``retain_grad``, the corner weights
    and rows as ``field_ref.encode`` takes them.  Below 2^23 no partial sum, in any order, needs more than float32's 24 bits."""
    f = scene.field
    table, _, W = R.params_of(f, torch.float64)
    w1, b1, w2, b2 = W["offsets"]
    p, p32 = R.normalise(scene.points, f.aabb, scene.normalized, torch.float64)
    terms, _ = R.corner_terms(p, p32, scene.res, scene.T)
    e = 0
    for rows, w in terms:
        e = e + w * table[rows]
    N = p.shape[0]
    e = e.reshape(N, 32)
    e.retain_grad()
    x = torch.cat([e, scene.z.double()[None].expand(N, -1)], -1)
    pre = x @ w1.T + b1
    pre.retain_grad()
    h = torch.relu(pre)
    y = h @ w2.T + b2
    (y * scene.g.double()).sum().backward()
    de, dh, dy = e.grad.abs(), pre.grad.abs(), scene.g.double().abs()
    acc = torch.zeros_like(table.detach())
    fwd_e = 0
    for rows, w in terms:
        w = w.detach().abs()
        acc.index_add_(0, rows.reshape(-1), (w * de.view(N, -1, 2)).reshape(-1, 2))
        fwd_e = fwd_e + w * table.detach()[rows].abs()
    xa, ha = x.detach().abs(), h.detach().abs()
    sums = [acc, dh.T @ xa, dh.sum(0), dy.T @ ha, dy.sum(0), dh.sum(0) @ w1.detach()[:, 32:].abs(),
            fwd_e, xa @ w1.detach().abs().T + b1.detach().abs(), ha @ w2.detach().abs().T + b2.detach().abs(),
            dy @ w2.detach().abs(), dh @ w1.detach().abs()]
    return max(float(s.max()) for s in sums) / scene.grid


# ---- what a wave sees ----------------------------------------------------------------------------------------------------------

def lane_keys(points, res, T, normalized=True, aabb=None):
    """-> (keys [N, L, 8] int64: the table row of every corner as the scatter's lanes hold them, from the float32 cells and
    ``hash_slots``; floor cells [N, L, 3] int32; the selector [N] bool)"""
    box = None if aabb is None else torch.as_tensor(aabb, dtype=torch.float32)
    p, p32 = R.normalise(points.to(torch.float32), box, normalized, torch.float32)
    terms, (_, f) = R.corner_terms(p, p32, res, T)
    sel = torch.ones(points.shape[0], dtype=torch.bool)
    if not normalized:
        q = (points.to(torch.float32) - box[0]) / (box[1] - box[0])
        sel = ((q > 0) & (q < 1)).all(dim=1)
    return torch.stack([rows for rows, _ in terms], dim=-1), f, sel


def run_lengths_of(keys):
    """lengths of the runs of equal neighbours in a 1-D (or row-wise compared 2-D) tensor"""
    k = keys.reshape(keys.shape[0], -1)
    starts = torch.ones(k.shape[0], dtype=torch.bool)
    starts[1:] = (k[1:] != k[:-1]).any(dim=1)
    idx = torch.nonzero(starts).flatten()
    return torch.diff(torch.cat([idx, torch.tensor([k.shape[0]])])).tolist()


# ---- the random real-valued field ----------------------------------------------------------------------------------------------

def box_of(cano):
    """the aabb as the reference builds it from the canonical points (tests/test_field_gpu.py)"""
    aabb = torch.stack([cano.min(dim=0)[0], cano.max(dim=0)[0]])
    center = aabb.mean(dim=0)
    return (aabb - center) * 1.5 + center


def real_scene(log2_T, N, seed=0, base_res=16, max_res=2048):
    """The random field as ``_field()`` of tests/test_field_gpu.py builds it (tables scaled by 100, weights on the offsets head)
    at any table size and level range, on the CPU, with N surfel positions in random order and in the order of
    ``synthetic.sort_surfels_spatially``."""
    surf = syn.make_surfels(N, seed)
    aabb = box_of(surf.xyz)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        f = HashMLPField(aabb, base_res=base_res, max_res=max_res, log2_hashmap_size=log2_T)
        with torch.no_grad():
            f.mlp_base_offsets.layers[-1].weight.normal_(0, 0.1)
            f.mlp_base_offsets.layers[-1].bias.normal_(0, 0.1)
            f.encoding.hash_table.mul_(100)
            f.quat_encoding.hash_table.mul_(100)
    xyz = {"random": surf.xyz.contiguous(), "spatial": syn.sort_surfels_spatially(surf).xyz.contiguous()}
    return types.SimpleNamespace(field=f, aabb=aabb, xyz=xyz, log2_T=log2_T, T=2 ** log2_T, res=f.encoding.scalings.clone())


def second_layer_outputs(f, xyz, head, is_normalized=False):
    """float64 y [N, out] of a head that takes the encoding alone, before its sigmoid or normalisation"""
    table, qtable, W = R.params_of(f, torch.float64, requires_grad=False)
    p, p32 = R.normalise(xyz, f.aabb, is_normalized, torch.float64)
    e = R.encode(p, p32, qtable if head == "quats" else table, f.encoding.scalings, 2 ** int(f.log2_hashmap_size), value32=True)
    w1, b1, w2, b2 = W[head]
    return torch.relu(e @ w1.T + b1) @ w2.T + b2


def saturate(f, xyz, heads=("shs", "opacities"), level=200.0):
    """centres every output of the heads' second layers on its median over ``xyz`` and scales the layer in place so that the
    median |y| is ``level``: most points then lie past +-100, on either side, where float32's sigmoid is exactly 0 or 1"""
    with torch.no_grad():
        for h in heads:
            m = getattr(f, f"mlp_base_{h}")
            m.layers[1].bias.sub_(second_layer_outputs(f, xyz, h).median(dim=0)[0].float())
            s = level / float(second_layer_outputs(f, xyz, h).abs().median())
            m.layers[1].weight.mul_(s)
            m.layers[1].bias.mul_(s)


HEAD_OUT = (("shs", 3), ("scales", 1), ("quats", 4), ("offsets", 3), ("opacities", 1))


def upstream(n, seed=7, heads=R.HEADS):
    """random upstream gradients on ``heads`` -> loss(out)"""
    g = torch.Generator().manual_seed(seed)
    G = {h: torch.randn(n, o, generator=g) for h, o in HEAD_OUT}
    return lambda out: sum((out[h] * G[h].to(out[h].device, out[h].dtype)).sum() for h in heads)
