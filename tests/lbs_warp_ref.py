"""Restatement of the skinning warp (soar_amd/lbs.py, csrc/lbs.hip) in torch, in any dtype: float64 is the yardstick, float32 the
composition a user without the kernel would run.  It follows oracle.lbs_oracle.warp operation by operation (blend einsum, position
plus offsets, R' = M3 R(q), optional T, matrix_to_quaternion, standardise, F.normalize) and, with neither control set, gives its
bits in float32.  Two controls the oracle lacks: ``branch=`` forces the row of the candidate table per point where the oracle takes
the argmax of q_abs, ``sign=`` forces the standardisation's sign per point.  Gradients come from autograd.

The comparison rule (``compare``) is made for the two places where matrix_to_quaternion is discontinuous: a tie of the candidate
table (two q_abs equal: another row is another formula, equal in exact arithmetic only for a rotation matrix) and the flip at a
real part of zero (q and -q).  There a kernel and a reference may rightly decide differently, and a naive comparison reports errors
of order 1.  Per point the rule admits every (branch, sign) pair the float64 run cannot tell apart -- branches whose q_abs is within
1e-5 relative of the largest, and the other sign where that branch's real part is within 1e-5 of zero -- and asks that ONE admitted
pair matches the kernel's quaternion, its dL/drot and its dL/dxyz at once.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import lbs_oracle as lo

FLOOR = 1e-6            # of the largest magnitude (the project's bar: tests/body_ref.py)
CAP = 1e-4              # the float32 restatement's own distance from float64
TIE = 1e-5              # window of a tie (relative, q_abs) and of a flip (absolute, real part of a quaternion of norm <= 1)
MULTI_CAP = 0.005       # share of points with more than one admitted pair, outside the cases built on ties and flips


def warp(points, rot, weights, mats, offsets=None, T=None, branch=None, sign=None, dtype=None):
    """points [P,3], rot [P,4], weights [P,J] + mats [J,4,4] -- or weights None and mats [P,4,4] per point -- -> (points' [P,3],
    rot' [P,4], info).  branch: int64 [P] or None (argmax of q_abs), sign: [P] of +-1 or None (non-negative real part).
    info: q_abs [P,4], real [P] (the real part of the chosen candidate before standardisation), branch [P] (the row taken)."""
    if dtype is not None:
        c = lambda t: None if t is None else t.to(dtype)
        points, rot, weights, mats, offsets, T = c(points), c(rot), c(weights), c(mats), c(offsets), c(T)
    if weights is None:
        mat = mats[None]
    else:
        mat = torch.einsum("bnj,bjxy->bnxy", weights[None], mats[None])
    pts = (torch.einsum("bnxy,bny->bnx", mat[..., :3, :3], points[None]) + mat[..., :3, 3])[0]
    if offsets is not None:
        pts = pts + offsets
    rot_mat = lo.quaternion_to_matrix(rot)
    rot_mat = torch.matmul(mat[..., :3, :3], rot_mat)
    if T is not None:
        pts = torch.matmul(pts, T)
        rot_mat = torch.matmul(T.T, rot_mat)
    # matrix_to_quaternion of the oracle, with the row of the table open to the caller
    batch_dim = rot_mat.shape[:-2]
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = torch.unbind(rot_mat.reshape(batch_dim + (9,)), dim=-1)
    q_abs = lo._sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22,
                                                1.0 - m00 - m11 + m22], dim=-1))
    quat_by_rijk = torch.stack([
        torch.stack([q_abs[..., 0] ** 2, m21 - m12, m02 - m20, m10 - m01], dim=-1),
        torch.stack([m21 - m12, q_abs[..., 1] ** 2, m10 + m01, m02 + m20], dim=-1),
        torch.stack([m02 - m20, m10 + m01, q_abs[..., 2] ** 2, m12 + m21], dim=-1),
        torch.stack([m10 - m01, m20 + m02, m21 + m12, q_abs[..., 3] ** 2], dim=-1)], dim=-2)
    flr = torch.tensor(0.1).to(dtype=q_abs.dtype)
    quat_candidates = quat_by_rijk / (2.0 * q_abs[..., None].max(flr))
    row = q_abs.argmax(dim=-1) if branch is None else branch.reshape(q_abs.shape[:-1])
    best = F.one_hot(row, num_classes=4) > 0.5
    out = quat_candidates[best, :].reshape(batch_dim + (4,))
    real = out[..., 0]
    if sign is None:
        out = torch.where(out[..., 0:1] < 0, -out, out)
    else:
        out = out * sign.to(out.dtype).reshape(batch_dim + (1,))
    q = F.normalize(out, p=2, dim=-1)[0]
    return pts, q, {"q_abs": q_abs[0].detach(), "real": real[0].detach(), "branch": row[0].detach()}


def run(case, dtype, branch=None, sign=None):
    """One forward and backward of a case (tests/lbs_warp_cases.py) with the case's upstream gradients -> dict of numpy float64
    arrays: p, q, dxyz, drot, doff (None without offsets), q_abs, real, branch."""
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)         # (the case's own tensors stay as they are)
    xyz, rot = leaf(case["xyz"]), leaf(case["rot"])
    off = case.get("offsets")
    off = leaf(off) if off is not None else None
    p, q, info = warp(xyz, rot, case.get("weights"), case["mats"], off, case.get("T"), branch, sign, dtype)
    ((p * case["gp"].to(dtype)).sum() + (q * case["gq"].to(dtype)).sum()).backward()
    n = lambda t: None if t is None else t.detach().double().numpy()
    return {"p": n(p), "q": n(q), "dxyz": n(xyz.grad), "drot": n(rot.grad), "doff": n(off.grad) if off is not None else None,
            "q_abs": n(info["q_abs"]), "real": n(info["real"]), "branch": info["branch"].numpy()}


def admitted_pairs(case):
    """The float64 runs of every (branch, sign) pair and which of them the rule admits per point -> (list of 8 run dicts, bool
    [8,P]).  Pair 2 b is branch b with its natural sign, pair 2 b + 1 the same branch with the other sign."""
    nat = run(case, torch.float64)
    P = nat["q"].shape[0]
    top = nat["q_abs"].max(1)
    runs, ok = [], np.zeros((8, P), bool)
    for b in range(4):
        rb = torch.full((P,), b, dtype=torch.int64)
        r = run(case, torch.float64, branch=rb)
        with np.errstate(invalid="ignore"):
            branch_ok = nat["q_abs"][:, b] >= (1.0 - TIE) * top
            natural = np.where(r["real"] < 0, -1.0, 1.0)
            flip_ok = branch_ok & (np.abs(r["real"]) <= TIE)
        runs.append(r)
        runs.append(run(case, torch.float64, branch=rb, sign=torch.from_numpy(-natural)))
        ok[2 * b], ok[2 * b + 1] = branch_ok, flip_ok
    return nat, runs, ok


def _scaled(case, name, a):
    """dL/drot rows times that row's |q|: the gradient scales as 1 / |q|, and the cases span scales"""
    if name != "drot":
        return a
    return a * np.linalg.norm(case["rot"].double().numpy(), axis=1, keepdims=True)


def rule_errors(case, got, nat, runs, ok):
    """Under the rule: per tensor (q, drot, dxyz) the worst element over the largest magnitude of the float64 tensor, every point
    measured against the ONE admitted pair that serves its three tensors best at once.  -> ({name: worst}, chosen pair [P])."""
    names = ("q", "drot", "dxyz")
    P = nat["q"].shape[0]
    scale = {k: max(float(np.abs(_scaled(case, k, nat[k])).max()), 1e-300) for k in names}
    err = np.full((8, P, 3), np.inf)
    for i, r in enumerate(runs):
        for t, k in enumerate(names):
            with np.errstate(invalid="ignore"):
                d = np.abs(_scaled(case, k, np.asarray(got[k], np.float64)) - _scaled(case, k, r[k])).max(1) / scale[k]
            d = np.where(np.isfinite(d), d, np.inf)
            err[i, :, t] = np.where(ok[i], d, np.inf)
    pick = err.max(2).argmin(0)                                   # the pair whose worst of the three is smallest
    chosen = err[pick, np.arange(P)]                              # [P,3]
    return {k: float(chosen[:, t].max()) for t, k in enumerate(names)}, pick


def compare(name, got, case, prepared=None, report=None):
    """The kernel's outputs of a case (dict: p, q, dxyz, drot as arrays) against float64 under the rule and the project's bar: HIP
    at most 4 x the float32 restatement's own distance under the same rule, floor 1e-6; the restatement itself capped at 1e-4.
    Positions do not depend on the pair: plain worst element.  Prints before it asserts.  -> the table's lines."""
    nat, runs, ok = prepared if prepared is not None else admitted_pairs(case)
    f32 = run(case, torch.float32)
    e_hip, pick = rule_errors(case, got, nat, runs, ok)
    e_f32, _ = rule_errors(case, f32, nat, runs, ok)
    pscale = max(float(np.abs(nat["p"]).max()), 1e-300)
    e_hip["p"] = float(np.abs(np.asarray(got["p"], np.float64) - nat["p"]).max() / pscale)
    e_f32["p"] = float(np.abs(f32["p"] - nat["p"]).max() / pscale)
    multi = int((ok.sum(0) > 1).sum())
    off_natural = int(((pick != 2 * nat["branch"]) & (ok.sum(0) > 1)).sum())
    lines = [f"{name}: {k:5s} hip {e_hip[k]:.3e} f32 {e_f32[k]:.3e}" for k in ("p", "q", "dxyz", "drot")]
    lines.append(f"{name}: {multi} of {ok.shape[1]} points admit more than one pair; the kernel sits on another pair than float64 at {off_natural}")
    for line in lines:
        print(line)
    if report is not None:
        report.extend(lines)
    for k in ("p", "q", "dxyz", "drot"):
        assert np.isfinite(np.asarray(got[k])).all(), (name, k)
        assert e_f32[k] <= CAP, (name, k, e_f32[k])
        assert e_hip[k] <= max(4 * e_f32[k], FLOOR), (name, k, e_hip[k], e_f32[k])
    if not case.get("on_ties", False):
        assert multi <= MULTI_CAP * ok.shape[1], (name, multi)
    return lines
