"""soar_adam_step / optim.FusedAdam against torch.optim.Adam, the optimizer of the reference's Gaussian model
(TS/geometry/surfel_base.py:596-681: per-leaf learning rates, eps = 1e-15; TS/system/gaussian_surfel_mvdream.py:471-472), and the
entry points of csrc/optim.hip directly against the float32 restatement of the update (tests/optim_ref.py), bit for bit and between
guards: every count around the kernel's float4 and its block of 1024, every alignment of the four arrays, empty rows, full tables,
both step counters, a step in parts and the gather that rides in the launch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optim_ref as orf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the surfel counts of the flat-buffer test: 5000 as before, then counts that leave the buffer's slices (at 3P, 7P, 10P, 13P, 14P
# floats) off 16 bytes, rows below one float4, and 1023 / 1025 / 4999 around a block's and a float4's end
_FUSED_CASES = ([pytest.param(c, 5000, id=i) for c, i in ((False, "step kept by the host"), (True, "step kept on the device"))]
                + [pytest.param(c, P, id=f"{i}-P{P}") for P in (1, 2, 3, 5, 1023, 1025, 4999)
                   for c, i in ((False, "step kept by the host"), (True, "step kept on the device"))])


@pytest.mark.parametrize("device_counter,P", _FUSED_CASES)
def test_fused_adam_matches_torch_adam(device_counter, P):
    from soar_amd import frame_dp, optim
    g = torch.Generator().manual_seed(0)
    widths = dict(frame_dp.LEAVES)
    init = {n: torch.randn(P, w, generator=g) for n, w in widths.items()}
    ours = {n: t.clone().to(DEV).requires_grad_(True) for n, t in init.items()}
    ref = {n: t.clone().to(DEV).requires_grad_(True) for n, t in init.items()}
    flat = frame_dp.FlatGradBuffer(ours)
    # where the slices lie: leaf after leaf, so all but the first start off a 16-byte boundary unless (floats in front) % 4 == 0 --
    # at P % 4 != 0 that is rot, scales and opacity at every such P, colors and occ too at odd P (asserted: the scalar path's premise)
    at = 0
    for n, w in frame_dp.LEAVES:
        assert flat.views[n].data_ptr() == flat.flat.data_ptr() + 4 * at and flat.flat.data_ptr() % 16 == 0
        assert (flat.views[n].data_ptr() % 16 != 0) == ((at % 4) != 0), n
        at += P * w
    if P % 4:
        off = {n for n in widths if flat.views[n].data_ptr() % 16}
        assert {"rot", "scales", "opacity"} <= off and (P % 2 == 0 or off == set(widths) - {"xyz"}), off
    adam = optim.FusedAdam(flat)
    adam.device_counter = device_counter          # soar_adam_step_rows (a launch advances a counter) / soar_adam_step_at
    tadam = torch.optim.Adam([{"params": [ref[n]], "lr": optim.REFERENCE_LR[n]} for n in widths], lr=0.0, eps=1e-15)
    exact = {n: (init[n].numpy().reshape(-1).copy(), np.zeros(P * w, np.float32), np.zeros(P * w, np.float32)) for n, w in widths.items()}
    for step in range(25):
        for n, w in widths.items():
            grad_host = torch.randn(P, w, generator=g) * (10.0 ** ((step % 5) - 2))
            grad = grad_host.to(DEV)
            flat.views[n].copy_(grad)
            ref[n].grad = grad.clone()
            exact[n] = orf.adam_step_f32(exact[n][0], grad_host.numpy().reshape(-1), exact[n][1], exact[n][2], optim.REFERENCE_LR[n], step + 1)
        adam.step()
        tadam.step()
        for n in widths:
            torch.testing.assert_close(ours[n].detach(), ref[n].detach(), rtol=3e-5, atol=5e-7, msg=lambda m: f"step {step} leaf {n}: {m}")
            # ... and the float32 restatement of the kernel's expressions bit for bit
            for got, want, what in zip((ours[n], adam.exp_avg[n], adam.exp_avg_sq[n]), exact[n], ("value", "exp_avg", "exp_avg_sq")):
                assert orf.same_bits(got.reshape(-1), want), (step, n, what)
    assert (int(adam.state[0].item()) if device_counter else adam.steps) == 25


# ---- the entry points directly: rows from tests/optim_ref.make_rows, the reference from adam_step_f32 -------------------------------

_ENTRY_ROWS = {"at": 8, "rows": 8, "wide": 40}
_KINDS = orf.KINDS


def _mixed(n):
    """Every row with offsets of its own, the four arrays of a row never all alike."""
    return [((r + 1) % 4, (3 * r) % 4, (r + 2) % 4, (2 * r + 3) % 4) for r in range(n)]


# (b): all aligned; one array at a time moved by 1, 2 or 3 floats; all four at different offsets; every row on its own
_OFFSETS = ([(0, 0, 0, 0)] + [tuple(k if i == a else 0 for i in range(4)) for a in range(4) for k in (1, 2, 3)]
            + [(1, 2, 3, 0), (3, 1, 0, 2), "mixed"])


def _offsets(o, n):
    return _mixed(n) if o == "mixed" else o


def _lib():
    from soar_amd import hip_lib
    return hip_lib.lib()


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _state(step=0):
    st = torch.zeros(4, dtype=torch.int32, device=DEV)
    st[0] = step
    return st


def _call(entry, rows, idx, t=None, state=None, advance=1):
    b1, b2 = orf.BETAS
    idx = list(idx)
    tab = rows.table(idx) if idx else None
    if entry == "at":
        return _lib().soar_adam_step_at(len(idx), tab, b1, b2, orf.EPS, t, _stream())
    fn = _lib().soar_adam_step_rows if entry == "rows" else _lib().soar_adam_step_rows_wide
    return fn(len(idx), tab, b1, b2, orf.EPS, state.data_ptr(), advance, _stream())


def _parts(entry, n):
    """All rows in as few tables as the entry point takes: the first starts the step, the others belong to it."""
    m = _ENTRY_ROWS[entry]
    if n <= m:
        return [list(range(n))]
    k = -(-n // m)
    size = -(-n // k)
    return [list(range(a, min(a + size, n))) for a in range(0, n, size)]


def _run(entry, rows, parts=None, steps=3, first=1):
    from soar_amd import hip_lib
    parts = _parts(entry, len(rows.counts)) if parts is None else parts
    state = _state(first - 1)
    for t in range(first, first + steps):
        for k, idx in enumerate(parts):
            assert _call(entry, rows, idx, t=t, state=state, advance=1 if k == 0 else 0) == 0, hip_lib.last_error()
    torch.cuda.synchronize()
    return state


@functools.lru_cache(maxsize=None)
def _reference(counts, steps=3, first=1):
    rows = orf.make_rows(counts)                               # (the values of a row do not depend on its placement)
    state = rows.reference()
    for t in range(first, first + steps):
        orf.step_reference(state, rows.lr, t)
    return state


@functools.lru_cache(maxsize=None)
def _aligned_run(entry, counts):
    rows = orf.make_rows(counts, device=DEV)
    _run(entry, rows)
    return rows


def _check_state(state, t):
    """The device counter's three words: the step and its bias corrections, formed in double and rounded once."""
    words = state.cpu().numpy()
    bc1, bc2s = orf.bias_corrections(t)
    assert int(words[0]) == t and int(words[3]) == 0
    assert int(words[1]) == int(orf.bits(bc1)[0]) and int(words[2]) == int(orf.bits(bc2s)[0]), (words, bc1, bc2s)


@pytest.mark.parametrize("entry", ["at", "rows", "wide"])
def test_adam_entry_points_equal_the_float32_reference_at_every_count(entry):
    """(a) Rows of 0 to 4099 floats, each with its own learning rate, three steps, all arrays aligned: the 8-row entry points over
    two tables (the second belongs to the step the first started), the wide one over a single table.  Values, both moments and the
    untouched gradients bit for bit, every guard word intact."""
    rows = orf.make_rows(orf.COUNTS, device=DEV)
    parts = _parts(entry, len(orf.COUNTS))
    assert len(parts) == (1 if entry == "wide" else 2)
    state = _run(entry, rows, parts)
    rows.check_guards()
    orf.assert_rows_equal(rows, _reference(orf.COUNTS), entry)
    if entry != "at":
        _check_state(state, 3)


@pytest.mark.parametrize("entry", ["at", "wide"])
@pytest.mark.parametrize("offsets", _OFFSETS, ids=[str(o) for o in _OFFSETS])
def test_adam_result_does_not_depend_on_alignment(offsets, entry):
    """(b) The rows of (a) with their arrays moved off the 16-byte boundary: whole rows through the scalar loop, and -- in the aligned
    case -- the scalar fallback in the last block of a row whose count is no multiple of four.  Bit-equal to the aligned run and to
    the reference, guards intact."""
    n = len(orf.COUNTS)
    rows = orf.make_rows(orf.COUNTS, _offsets(offsets, n), device=DEV)
    for r in (5, n - 1):                                                       # the premise: the pointers really are where asked
        for ki, kind in enumerate(_KINDS):
            assert rows.view(kind, r).data_ptr() % 16 == 4 * rows.offsets[r][ki]
    _run(entry, rows)
    rows.check_guards()
    orf.assert_rows_equal(rows, _aligned_run(entry, orf.COUNTS), f"{entry} against the aligned run:")
    orf.assert_rows_equal(rows, _reference(orf.COUNTS), f"{entry} against the reference:")


_EMPTY_CASES = [(0, 5, 1025, 3), (5, 0, 1025, 3), (5, 1025, 3, 0), (5, 0, 0, 1025, 3), (0, 0, 1023, 0, 0, 2, 0)]


@pytest.mark.parametrize("entry", ["at", "rows", "wide"])
@pytest.mark.parametrize("counts", _EMPTY_CASES, ids=[str(c) for c in _EMPTY_CASES])
def test_adam_empty_rows_anywhere_in_the_table(counts, entry):
    """(c) Empty rows (NULL pointers, count 0) first, in the middle, last and next to each other: they own no block, the search
    for a block's row steps over them."""
    rows = orf.make_rows(counts, _mixed(len(counts)), device=DEV)
    tab = rows.table()
    assert all((tab[r].param is None) == (c == 0) for r, c in enumerate(counts))
    _run(entry, rows)
    rows.check_guards()
    orf.assert_rows_equal(rows, _reference(counts), entry)


@pytest.mark.parametrize("entry", ["at", "rows", "wide"])
def test_adam_all_rows_empty_is_no_launch(entry):
    """(c) Nothing to update: return code 0; the device counter moves where `advance` says so and only there."""
    from soar_amd import hip_lib
    rows = orf.make_rows((0, 0, 0), device=DEV)
    for idx in ([0, 1, 2], []):
        state = _state(4)
        assert _call(entry, rows, idx, t=7, state=state, advance=0) == 0, hip_lib.last_error()
        torch.cuda.synchronize()
        if entry != "at":
            assert state.cpu().tolist() == [4, 0, 0, 0]
            assert _call(entry, rows, idx, state=state, advance=1) == 0, hip_lib.last_error()
            torch.cuda.synchronize()
            _check_state(state, 5)
    rows.check_guards()


@pytest.mark.parametrize("offsets", ["aligned", "mixed"])
@pytest.mark.parametrize("entry", ["at", "rows", "wide"])
def test_adam_full_table_and_one_row_too_many(entry, offsets):
    """(c) 8 of 8 and 40 of 40 rows, the counts cycling through those of (a); one row more is refused and nothing is written."""
    from soar_amd import hip_lib
    m = _ENTRY_ROWS[entry]
    counts = tuple(orf.COUNTS[(r + 3) % len(orf.COUNTS)] for r in range(m + 1))
    rows = orf.make_rows(counts, _mixed(m + 1) if offsets == "mixed" else None, device=DEV)
    state = _state(0)
    assert _call(entry, rows, range(m + 1), t=1, state=state, advance=1) != 0
    assert "n_rows" in hip_lib.last_error()
    torch.cuda.synchronize()
    orf.assert_rows_equal(rows, rows.reference(), "refused:")
    assert state.cpu().tolist() == [0, 0, 0, 0]
    _run(entry, rows, [list(range(m))])
    rows.check_guards()
    want = _reference(counts)
    orf.assert_rows_equal(rows, want[:m] + rows.reference()[m:], entry)


_STEPS = [1, 2, 1000, 10 ** 6, 2 ** 31 - 1]


@pytest.mark.parametrize("entry", ["at", "rows", "wide"])
@pytest.mark.parametrize("t", _STEPS)
def test_adam_step_numbers(t, entry):
    """(d) The step number from the host (soar_adam_step_at) and from the device counter (step - 1 written into the state, advanced
    once): the bias corrections of step t, up to the last step an int32 holds."""
    rows = orf.make_rows(orf.COUNTS, _mixed(len(orf.COUNTS)), device=DEV)
    state = _run(entry, rows, steps=1, first=t)
    rows.check_guards()
    orf.assert_rows_equal(rows, _reference(orf.COUNTS, 1, t), f"{entry} step {t}:")
    if entry != "at":
        _check_state(state, t)


def _gather_args(ids, seq, fpf, n_sets, table, mats, sets):
    return (len(ids), seq, fpf, n_sets, (C.c_int32 * len(ids))(*ids), table.data_ptr(), mats.data.data_ptr(),
            sets.data.data_ptr() if sets is not None else None)


@pytest.mark.parametrize("gather", [False, True], ids=["step_at", "step_at_gather"])
@pytest.mark.parametrize("t", [2 ** 31, 2 ** 40, 0, -1], ids=["2^31", "2^40", "0", "-1"])
def test_adam_step_at_refuses_steps_outside_int32(t, gather):
    """(d) A step past INT32_MAX used to be truncated to a negative int32, every row skipped and 0 returned: now refused with a
    message, like a step below 1, and nothing is written."""
    from soar_amd import hip_lib
    rows = orf.make_rows(orf.RAGGED, _mixed(len(orf.RAGGED)), device=DEV)
    b1, b2 = orf.BETAS
    if gather:
        table = torch.randn(5 * 7, device=DEV)
        mats, sets = orf.GuardedArray(2 * 7, torch.float32, DEV), orf.GuardedArray(2, torch.int32, DEV)
        mats.data.fill_(-1.0)
        rc = _lib().soar_adam_step_at_gather(len(orf.RAGGED), rows.table(), b1, b2, orf.EPS, t, *_gather_args([1, 2], 5, 7, 3, table, mats, sets),
                                             _stream())
    else:
        rc = _lib().soar_adam_step_at(len(orf.RAGGED), rows.table(), b1, b2, orf.EPS, t, _stream())
    assert rc != 0 and "step" in hip_lib.last_error()
    if t > 0:
        assert str(t) in hip_lib.last_error() and "32-bit" in hip_lib.last_error()
    torch.cuda.synchronize()
    rows.check_guards()
    orf.assert_rows_equal(rows, rows.reference(), "refused:")
    if gather:
        assert bool((mats.data == -1.0).all())
        mats.check_guards(); sets.check_guards()


@pytest.mark.parametrize("offsets", [(0, 0, 0, 0), (0, 1, 0, 0), (1, 2, 3, 0), "mixed"], ids=str)
@pytest.mark.parametrize("entry,counts", [("rows", orf.RAGGED), ("wide", orf.COUNTS)], ids=["rows", "wide"])
def test_adam_step_in_parts_equals_the_step_in_one_call(entry, counts, offsets):
    """(e) advance = 1 on the first rows, advance = 0 on the rest: the same three steps as one call over all rows, bit for bit."""
    n = len(counts)
    whole = orf.make_rows(counts, _offsets(offsets, n), device=DEV)
    _run(entry, whole, [list(range(n))])
    orf.assert_rows_equal(whole, _reference(counts), "one call:")
    for split in (1, n // 2, n - 1):
        rows = orf.make_rows(counts, _offsets(offsets, n), device=DEV)
        state = _run(entry, rows, [list(range(split)), list(range(split, n))])
        rows.check_guards()
        _check_state(state, 3)
        orf.assert_rows_equal(rows, whole, f"split at {split}:")


_SEQ = 5                                                             # frames of the sequence table
# a negative id, the sequence length itself, one far beyond it, a repeat, the ends, a negative multiple of the length
_IDS = [-7, _SEQ, 1000003, 2, 2, 0, _SEQ - 1, -_SEQ]


@pytest.mark.parametrize("fpf", [7, 880], ids=["7-floats", "880-floats"])          # below one stride of 256 threads; 55 joints x 16
@pytest.mark.parametrize("n_frames", [1, 3, 8])
def test_adam_step_at_gather_is_the_step_and_the_gather(n_frames, fpf):
    """(f) soar_adam_step_at_gather: its n_frames workgroups behind the update's write what soar_gather_step_inputs_ids writes -- ids
    taken modulo the sequence length, negative ones fixed up -- between intact guards; the rows are those of soar_adam_step_at.
    With and without target sets and their output, and with no rows at all (the launch is the gather's workgroups alone)."""
    from soar_amd import hip_lib
    L = _lib()
    b1, b2 = orf.BETAS
    n = len(orf.RAGGED)
    table = torch.randn(_SEQ * fpf, generator=torch.Generator().manual_seed(fpf)).to(DEV)
    plain = orf.make_rows(orf.RAGGED, _mixed(n), device=DEV)
    assert L.soar_adam_step_at(n, plain.table(), b1, b2, orf.EPS, 3, _stream()) == 0, hip_lib.last_error()
    id_lists = [[i] for i in _IDS] if n_frames == 1 else [_IDS[:n_frames], _IDS[::-1][:n_frames]]
    for ids in id_lists:
        for n_sets in (0, 3):
            for with_sets in (True, False):
                for n_rows in (n, 0):
                    want_m, want_s = orf.GuardedArray(n_frames * fpf, torch.float32, DEV), orf.GuardedArray(n_frames, torch.int32, DEV)
                    assert L.soar_gather_step_inputs_ids(*_gather_args(ids, _SEQ, fpf, n_sets, table, want_m, want_s), _stream()) == 0
                    mats = orf.GuardedArray(n_frames * fpf, torch.float32, DEV, offset=n_frames % 4)
                    sets = orf.GuardedArray(n_frames, torch.int32, DEV, offset=1) if with_sets else None
                    rows = orf.make_rows(orf.RAGGED, _mixed(n), device=DEV)
                    rc = L.soar_adam_step_at_gather(n_rows, rows.table() if n_rows else None, b1, b2, orf.EPS, 3,
                                                    *_gather_args(ids, _SEQ, fpf, n_sets, table, mats, sets), _stream())
                    assert rc == 0, hip_lib.last_error()
                    torch.cuda.synchronize()
                    case = (ids, n_sets, with_sets, n_rows)
                    mats.check_guards(); rows.check_guards()
                    assert torch.equal(mats.data.view(torch.int32), want_m.data.view(torch.int32)), case
                    host = [i % _SEQ for i in ids]                               # (Python's % is already the fixed-up one)
                    assert torch.equal(mats.data, torch.cat([table[i * fpf:(i + 1) * fpf] for i in host])), case
                    if with_sets:
                        sets.check_guards()
                        assert torch.equal(sets.data, want_s.data), case
                        assert sets.data.cpu().tolist() == [i % n_sets if n_sets else 0 for i in host], case
                    orf.assert_rows_equal(rows, plain if n_rows else rows.reference(), str(case))
    orf.assert_rows_equal(plain, _reference(orf.RAGGED, 1, 3), "soar_adam_step_at:")


def test_rows_of_a_step_that_was_never_started_are_left_alone():
    """soar_adam_step_rows(advance=0) on a fresh, zeroed state: 1 - beta1^0 = 0 would make the step size infinite.  The rows are
    left untouched (parameters and moments); the first advancing call then is step 1."""
    from soar_amd import frame_dp, optim
    g = torch.Generator().manual_seed(1)
    P = 1000
    leaves = {n: torch.randn(P, w, generator=g).to(DEV).requires_grad_(True) for n, w in dict(frame_dp.LEAVES).items()}
    before = {n: t.detach().clone() for n, t in leaves.items()}
    flat = frame_dp.FlatGradBuffer(leaves)
    flat.flat.copy_(torch.randn(flat.flat.shape, generator=g).to(DEV))
    adam = optim.FusedAdam(flat)
    adam.device_counter = True
    adam.step(advance=False)
    torch.cuda.synchronize()
    for n in leaves:
        assert torch.equal(leaves[n].detach(), before[n]) and torch.isfinite(leaves[n]).all(), n
        assert not adam.exp_avg[n].any() and not adam.exp_avg_sq[n].any()
    assert int(adam.state[0].item()) == 0
    adam.step()
    assert int(adam.state[0].item()) == 1 and all(torch.isfinite(t).all() for t in leaves.values())
    assert not torch.equal(leaves["xyz"].detach(), before["xyz"])


def test_batched_launch_sites_refuse_frames_that_disagree():
    """soar_batch_begin / _frame / _end: every stage is launched once for all frames with the LAST frame's grid -- a frame of another
    size (or a frame whose call never came) must fail loudly instead of being launched with a stale or mis-sized argument block."""
    import ctypes as C
    from soar_amd import hip_lib
    from soar_amd.hip_lib import ptr
    L = hip_lib.lib()
    dev = torch.device("cuda:0")
    k = C.c_size_t(0)
    assert L.soar_image_loss_scratch_floats(C.byref(k)) == 0
    stream = torch.cuda.current_stream(dev).cuda_stream

    def l1(H, W):
        a, b = torch.rand(3, H, W, device=dev), torch.rand(3, H, W, device=dev)
        stats, scratch = torch.zeros(2, device=dev), torch.zeros(int(k.value), device=dev)
        keep.extend([a, b, stats, scratch])
        return L.soar_masked_l1(3, H, W, ptr(a), ptr(b), None, ptr(stats), ptr(scratch), stream), stats, (a - b).abs().mean()

    keep = []
    # two frames of one size: one launch, both right
    assert L.soar_batch_begin(2) == 0
    try:
        assert L.soar_batch_frame(0) == 0
        rc0, s0, want0 = l1(64, 96)
        assert L.soar_batch_frame(1) == 0
        rc1, s1, want1 = l1(64, 96)
    finally:
        L.soar_batch_end()
    torch.cuda.synchronize()
    assert rc0 == 0 and rc1 == 0
    torch.testing.assert_close(s0[0], want0, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(s1[0], want1, rtol=1e-5, atol=1e-7)
    # a second frame of another size: refused
    assert L.soar_batch_begin(2) == 0
    try:
        assert L.soar_batch_frame(0) == 0
        rc0, _, _ = l1(64, 96)
        assert L.soar_batch_frame(1) == 0
        rc1, _, _ = l1(256, 256)
    finally:
        L.soar_batch_end()
    torch.cuda.synchronize()
    assert rc0 == 0 and rc1 != 0 and "agree in size" in hip_lib.last_error()
