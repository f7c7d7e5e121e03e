"""The batched step plan's folded small launches against the launches they replace (soar_amd/step_plan.py):

* SOAR_PLAN_LOSS_IN_TAIL    -- the fixed-order sum of the frame loss's partials runs as extra workgroups of the epilogue's kernel
                               (soar_frames_geometry_warp_backward_losses) instead of as frame_loss_finish_kernel in the chain;
* SOAR_PLAN_GATHER_IN_ADAM  -- the gather of the step's joint transforms / target-set indices rides in the optimizer's launch
                               (soar_adam_step_at_gather); the first step, which has no optimizer launch, keeps the stand-alone gather.

`tiny` (5k Gaussians, 256 x 192), plans of 1, 4 and 5 frames (5: a second group of frames in the epilogue's kernel), two steps from the
same snapshot of the leaves, each switch alone and both together against the form with both off.  Losses, gathered inputs and
images are the same bits wherever the parameters they were computed from are: in the first step always, in the second when the
first step's gradients were.  Gradients and the parameters after the optimizer's update differ between two runs of the SAME form by
the order of the backward blend's float atomics; that distance (L2 norm of the difference, per leaf: a maximum over elements is one
element's luck, and Adam turns a gradient of the size of the order noise into +-lr either way) is measured here from two runs with
every switch off, and a folded form may be 2 x as far from the first of them.  At this size two runs of one form often repeat each
other bit for bit (measured distance 0) while a third differs in one element's last bit: two samples cannot resolve a noise that
small, so the allowance has a floor from the number format, not from any measurement -- gradients: float32 epsilon times the
leaf's gradient norm (every element half a bit off); parameters: 2 lr of the leaf (Adam moves ONE element whose gradient is of the
size of the order noise by +-lr either way).  With the order-insensitive backward (rasterizer.DETERMINISTIC_BACKWARD: float64
accumulation rows) there is no such noise: every distance must be exactly zero, and the second step is held to the same bits too.
"""
EPS32 = 2.0 ** -23
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LRS = {"xyz": 1.6e-5, "rot": 1e-3, "scales": 5e-5, "colors": 2.5e-3}
SWITCHES = ("SOAR_PLAN_LOSS_IN_TAIL", "SOAR_PLAN_GATHER_IN_ADAM")
STEPS = {1: ([3], [17]), 4: ([0, 1, 2, 3], [9, 2, 30, 17]), 5: ([0, 1, 2, 3, 4], [9, 2, 30, 17, 5])}


@pytest.fixture(scope="module")
def tiny():
    import bench
    from soar_amd import rasterizer
    from soar_amd.frame_dp import FlatGradBuffer
    seq, pool, _ = bench.build_sequence("tiny", DEV)
    bg = torch.tensor([0.2, 0.5, 0.7], device=DEV)
    bench.run_step(seq, pool, FlatGradBuffer(seq.leaves()), [0, 1, 2, 3], bg)
    leaves = seq.leaves()
    return seq, pool, bg, 2 * rasterizer.last_num_rendered, {n: leaves[n].detach().clone() for n in leaves}


def _two_steps(tiny, n, on, monkeypatch):
    """a fresh plan + optimizer on the snapshot's leaves, the switches in `on` set -> what its two steps left"""
    from soar_amd.frame_dp import FlatGradBuffer
    from soar_amd.optim import FusedAdam
    from soar_amd.step_plan import FrameStepPlan
    seq, pool, bg, cap, snap = tiny
    leaves = seq.leaves()
    with torch.no_grad():
        for name, t in snap.items():
            leaves[name].copy_(t)
    for s in SWITCHES:
        monkeypatch.setenv(s, "1" if s in on else "0")
    flat = FlatGradBuffer(leaves)
    plan = FrameStepPlan(seq, n, pool, bg, cap, flat, use_graphs=False)
    assert plan.batched and plan.fused_tail
    assert (plan.loss_in_tail, plan.gather_in_adam) == tuple(s in on for s in SWITCHES)
    plan.optimizer = FusedAdam(flat, lr=LRS)
    out = []
    for frames in STEPS[n] + (STEPS[n][0],):            # (a third call applies the second step's gradients: the parameters after it)
        losses = plan.run(frames).clone()
        torch.cuda.synchronize()
        assert all(o == 0 for _, o in plan.check())
        out.append(dict(losses=losses, mats=plan.mats.clone(), sel=plan.frame_sel.clone(), grads=flat.flat.clone(),
                        images=[{k: v[k].clone() for k in ("color", "normal", "depth", "opac", "occ", "radii")} for v in plan.views],
                        params={k: leaves[k].detach().clone() for k in LRS}))
    return out[:2] + [dict(params=out[2]["params"])]


@pytest.mark.parametrize("exact", [False, True], ids=["float32_atomics", "float64_rows"])
@pytest.mark.parametrize("n", [1, 4, 5])
def test_folded_launches_leave_what_the_separate_ones_leave(tiny, n, exact, monkeypatch):
    from soar_amd import rasterizer
    monkeypatch.setattr(rasterizer, "DETERMINISTIC_BACKWARD", exact)
    seq = tiny[0]
    parent, again = _two_steps(tiny, n, (), monkeypatch), _two_steps(tiny, n, (), monkeypatch)
    dist = lambda a, b: float((a.double() - b.double()).norm())
    P = int(seq.xyz.shape[0])
    slices = {"xyz": (0, 3 * P), "rot": (3 * P, 7 * P), "scales": (7 * P, 10 * P), "colors": (10 * P, 13 * P)}
    same_params = lambda a, b: all(torch.equal(a["params"][k], b["params"][k]) for k in LRS)
    assert torch.equal(parent[0]["losses"], again[0]["losses"])              # the form itself repeats these bits
    if exact:
        assert all(torch.equal(parent[k]["grads"], again[k]["grads"]) for k in range(2)) and same_params(parent[2], again[2])
    for on in ((SWITCHES[0],), (SWITCHES[1],), SWITCHES):
        got = _two_steps(tiny, n, on, monkeypatch)
        for step in range(2):
            a, b = parent[step], got[step]
            # (a step's parameters: the leaves as its forward saw them = what the optimizer left at the start of that call)
            comparable = same_params(a, b)
            assert comparable or (step > 0 and not exact), (on, step)
            assert torch.equal(a["mats"], b["mats"]) and torch.equal(a["sel"], b["sel"]), (on, step)
            want_ids = torch.tensor([f % seq.num_frames for f in STEPS[n][step]], device=DEV)
            assert torch.equal(b["mats"], seq.cano2live[want_ids].reshape(b["mats"].shape)), (on, step)
            assert torch.equal(b["sel"].long(), want_ids % int(tiny[1].shape[0])), (on, step)
            if not comparable:
                continue
            assert torch.isfinite(b["losses"]).all() and float(b["losses"].abs().min()) > 0
            assert torch.equal(a["losses"], b["losses"]), (on, step, a["losses"], b["losses"])
            for f, (va, vb) in enumerate(zip(a["images"], b["images"])):
                for name in va:
                    assert torch.equal(va[name], vb[name]), (on, step, f, name)
            for name, (lo, hi) in slices.items():
                d0, d = dist(a["grads"][lo:hi], again[step]["grads"][lo:hi]), dist(a["grads"][lo:hi], b["grads"][lo:hi])
                print(f"n={n} {on} step {step} grad {name}: parent-parent {d0:.3e}, folded-parent {d:.3e}")
                floor = 0.0 if exact else EPS32 * float(a["grads"][lo:hi].double().norm())
                assert float(b["grads"][lo:hi].abs().max()) > 0 and d <= max(2 * d0, floor), (on, step, name, d, d0, floor)
        for step in (1, 2):                              # after the update from the first / the second step's gradients
            for name in LRS:
                d0 = dist(parent[step]["params"][name], again[step]["params"][name])
                d = dist(parent[step]["params"][name], got[step]["params"][name])
                print(f"n={n} {on} params after update {step} {name}: parent-parent {d0:.3e}, folded-parent {d:.3e}")
                assert d <= max(2 * d0, 0.0 if exact else 2 * LRS[name]), (on, step, name, d, d0)
        assert not torch.equal(got[2]["params"]["xyz"], tiny[4]["xyz"])      # (the optimizer did move the model)
