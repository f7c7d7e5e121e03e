"""A reference of the Adam update of soar_amd/csrc/optim.hip and a builder of row tables for its tests.

``adam_step_f32`` restates the kernel's expressions in numpy float32, one rounding per operation and in the kernel's order.  The
kernel turns contraction off around the update, the library is built without a fast-math flag, and float add, multiply, divide and
square root are correctly rounded on both sides: the GPU result is expected to equal this one bit for bit.  ``adam_step_f64`` is the
same formula in float64, for reporting how far float32 is from the truth.

``make_rows`` carves the four arrays of every row out of larger float tensors at a chosen element offset (0-3 floats past a 16-byte
boundary) and fills everything around them with a fixed NaN bit pattern: what a kernel writes outside its rows is seen bit for bit."""
import math

import numpy as np
import torch

KINDS = ("param", "grad", "exp_avg", "exp_avg_sq")
BETAS, EPS = (0.9, 0.999), 1e-15
# a signalling NaN: loads, stores and copies keep its bits, every arithmetic operation returns it quietened (bit 22 set) -- an update
# that runs one element past a row changes the guard there although all of its inputs are guards
GUARD_BITS = 0x7FA0BEEF
# the counts of the direct tests: empty, below one float4, around one block of 1024, around two, and four blocks plus three
COUNTS = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 4099)
RAGGED = tuple(c for c in COUNTS if c % 4)            # 8 rows, none a multiple of four


def bias_corrections(t, betas=BETAS):
    """(1 - beta1^t, sqrt(1 - beta2^t)) formed in double and rounded once, as the host and the tick kernel do."""
    return np.float32(1.0 - math.pow(betas[0], float(t))), np.float32(math.sqrt(1.0 - math.pow(betas[1], float(t))))


def adam_step_f32(p, g, m, v, lr, t, betas=BETAS, eps=EPS):
    """One step of the kernel's update on float32 arrays; returns the new (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    omb1, omb2 = f(1.0 - betas[0]), f(1.0 - betas[1])
    bc1, bc2s = bias_corrections(t, betas)
    with np.errstate(all="ignore"):
        step_size = f(lr) / bc1
        m = m + (g - m) * omb1
        v = f(betas[1]) * v + omb2 * (g * g)
        denom = np.sqrt(v) / bc2s + f(eps)
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


def adam_step_f64(p, g, m, v, lr, t, betas=BETAS, eps=EPS):
    """The same formula in float64 (the learning rate as the float32 the row table carries)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    with np.errstate(all="ignore"):
        step_size = float(np.float32(lr)) / (1.0 - b1 ** t)
        m = m + (g - m) * (1.0 - b1)
        v = b2 * v + (1.0 - b2) * (g * g)
        p = p - step_size * (m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps))
    return p, m, v


def bits(a):
    """float32 array (numpy or torch) -> its int32 bit patterns as numpy."""
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


def row_data(r, n, seed=0):
    """The values of row r: they depend on the row and its count only, not on where make_rows places them."""
    rng = np.random.default_rng([seed, r, n])
    f = np.float32
    return {"param": rng.standard_normal(n).astype(f), "grad": (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(f),
            "exp_avg": (0.1 * rng.standard_normal(n)).astype(f), "exp_avg_sq": (0.01 * rng.random(n)).astype(f)}


def row_lr(r):
    return 1e-3 * (1.0 + 0.37 * r)


class Rows:
    """What make_rows returns: ``buf[kind]`` the four backing tensors, ``view(kind, r)`` the array of a row inside them,
    ``table(rows)`` the SoarAdamRow table of the given rows (all by default), ``check_guards()``."""

    def __init__(self, counts, offsets, guard, device, seed):
        self.counts, self.guard, self.device = [int(c) for c in counts], int(guard), torch.device(device)
        if offsets is None:
            offsets = (0, 0, 0, 0)
        if len(offsets) == 4 and all(isinstance(o, int) for o in offsets):
            offsets = [tuple(offsets)] * len(self.counts)
        assert len(offsets) == len(self.counts) and all(len(o) == 4 and all(0 <= k <= 3 for k in o) for o in offsets)
        self.offsets = [tuple(o) for o in offsets]
        self.lr = [row_lr(r) for r in range(len(self.counts))]
        lead = (self.guard + 3) // 4 * 4                                        # the guard in front of a row ends on a 16-byte boundary
        self.start = {k: [] for k in KINDS}
        self.initial = [row_data(r, n, seed) for r, n in enumerate(self.counts)]
        host = {}
        for ki, kind in enumerate(KINDS):
            at = 0
            for r, n in enumerate(self.counts):
                self.start[kind].append(at + lead + self.offsets[r][ki])
                at = (self.start[kind][r] + n + self.guard + 3) // 4 * 4
            words = np.full(at, GUARD_BITS, dtype=np.uint32).view(np.int32)
            for r, n in enumerate(self.counts):
                words[self.start[kind][r]:self.start[kind][r] + n] = self.initial[r][kind].view(np.int32)
            host[kind] = words
        self.is_guard = {}
        for kind in KINDS:
            mask = np.ones(host[kind].shape, dtype=bool)
            for r, n in enumerate(self.counts):
                mask[self.start[kind][r]:self.start[kind][r] + n] = False
            self.is_guard[kind] = mask
        # (moved as int32: a float copy may quieten or canonicalise a NaN)
        self.buf = {kind: torch.from_numpy(host[kind].copy()).to(self.device).view(torch.float32) for kind in KINDS}
        assert all(b.data_ptr() % 16 == 0 for b in self.buf.values())

    def view(self, kind, r):
        s = self.start[kind][r]
        return self.buf[kind][s:s + self.counts[r]]

    def host(self, kind, r):
        return self.view(kind, r).detach().cpu().numpy().copy()

    def table(self, rows=None):
        from soar_amd.hip_lib import SoarAdamRow
        rows = range(len(self.counts)) if rows is None else rows
        tab = (SoarAdamRow * max(len(rows), 1))()
        for k, r in enumerate(rows):
            for kind in KINDS:                                                 # an empty row carries NULL pointers
                setattr(tab[k], kind, self.view(kind, r).data_ptr() if self.counts[r] else None)
            tab[k].count, tab[k].lr = self.counts[r], self.lr[r]
        return tab

    def check_guards(self):
        for kind in KINDS:
            words = self.buf[kind].view(torch.int32).cpu().numpy()
            bad = np.flatnonzero((words.view(np.uint32) != GUARD_BITS) & self.is_guard[kind])
            assert bad.size == 0, f"{kind}: {bad.size} guard words overwritten, the first at float {int(bad[0])} (rows start at {self.start[kind]})"

    def reference(self):
        """A float32 copy of the rows' initial values for ``step_reference``."""
        return [{k: a.copy() for k, a in d.items()} for d in self.initial]


def make_rows(counts, offsets=None, guard=8, device="cpu", seed=0):
    """Rows of ``counts[r]`` floats.  ``offsets``: one (param, grad, exp_avg, exp_avg_sq) tuple of element offsets 0-3 for all rows or one
    per row -- array k of a row starts ``4 * offset`` bytes past a 16-byte boundary.  ``guard`` floats of GUARD_BITS (at least) lie
    on both sides of every array."""
    return Rows(counts, offsets, guard, device, seed)


def step_reference(state, lr, t, rows=None, betas=BETAS, eps=EPS, step=adam_step_f32):
    """Step t of the given rows (all by default) of ``Rows.reference()`` in place."""
    for r in (range(len(state)) if rows is None else rows):
        d = state[r]
        d["param"], d["exp_avg"], d["exp_avg_sq"] = step(d["param"], d["grad"], d["exp_avg"], d["exp_avg_sq"], lr[r], t, betas, eps)


def assert_rows_equal(rows, state, what=""):
    """Every array of every row of a ``Rows`` against the reference state (or another ``Rows``), bit for bit."""
    for r, n in enumerate(rows.counts):
        for kind in KINDS:
            want = state.host(kind, r) if isinstance(state, Rows) else state[r][kind]
            got = rows.host(kind, r)
            if not same_bits(got, want):
                bad = np.flatnonzero(bits(got) != bits(want))
                raise AssertionError(f"{what} row {r} (count {n}, offsets {rows.offsets[r]}) {kind}: {bad.size} of {n} differ, the first at {int(bad[0])}: "
                                     f"{got[bad[0]]!r} against {want[bad[0]]!r}")


class GuardedArray:
    """One array of `n` elements of `dtype` (float32 / int32) between guards, for outputs that are no Adam rows."""

    def __init__(self, n, dtype, device, guard=8, offset=0):
        self.n, self.at = n, (guard + 3) // 4 * 4 + offset
        words = np.full(self.at + n + guard, GUARD_BITS, dtype=np.uint32).view(np.int32)
        self.buf = torch.from_numpy(words.copy()).to(device)
        self.data = self.buf[self.at:self.at + n].view(dtype)

    def check_guards(self):
        words = self.buf.cpu().numpy().view(np.uint32)
        mask = np.ones(words.shape, dtype=bool)
        mask[self.at:self.at + self.n] = False
        assert bool((words[mask] == GUARD_BITS).all()), "guard words around an output were overwritten"
