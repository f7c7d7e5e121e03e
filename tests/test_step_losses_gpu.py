"""GPU tests of the training step's image terms (csrc/step_terms.hip, soar_amd/step_losses.py).

The cosine and L1 terms are pinned on the library's own kernels (``losses.cos_loss`` / ``losses.masked_l1``) bit for bit: the
arithmetic is shared (csrc/loss_pixel.h) and the products commute, so no tolerance is involved.  The LPIPS inputs and the blended
target are pinned on the torch expression evaluated on the device, bit for bit (every operation rounds once; no contraction).  The
float64-summed means lie within 2 float32 ulps of the float64 restatement (tests/step_terms_ref.py): the double sum of fewer than
2^24 floats is exact to far below one float32 ulp, one division and one rounding to float32 follow.

Shapes: 1x1, 16x16, 37x53 (1961 pixels: a multiple of neither 4 nor 64, more than one workgroup) and 520x512 read from an odd base
(more workgroups than a walk has: the second trip of the grid-stride loop); B in {1, 2, 5, 8, 9} (9 crosses the chunk of 8)."""
import math

import pytest
import torch

import step_terms_ref as R
from soar_amd import losses as L
from soar_amd import step_losses as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
THR = math.pi / 10000
SHAPES = [(1, 1), (16, 16), (37, 53)]
AXES = torch.tensor([[1.0, 0.5, 0.5], [0.5, 1.0, 0.5], [0.5, 0.5, 1.0], [0.0, 0.5, 0.5]])      # unit normals (n + 1) / 2: cos = 1 exactly


def same(x, y):
    return x.shape == y.shape and torch.allclose(x, y, rtol=0.0, atol=0.0, equal_nan=True)


def ulp(x):
    x = x.abs().to(torch.float32)
    return torch.nextafter(x, torch.full_like(x, float("inf"))) - x


def quotient(a, b):
    """a / b in float32, rounded once (formed on the host: a device division by a number is a product with its reciprocal)"""
    return (torch.as_tensor(a).detach().cpu().to(torch.float32) / torch.tensor(float(b), dtype=torch.float32)).to(DEV)


def place(data, layout):
    """`data` [B,C,H,W] as a leaf in one of the layouts the nodes take without a copy"""
    B, C, H, W = data.shape
    n = C * H * W
    if layout == "planar":
        t = data.clone()
    elif layout == "permuted":                        # the plugin's [B,H,W,C]: a permuted view of planar memory
        t = data.clone().permute(0, 2, 3, 1)
    elif layout == "strided":                         # views of a larger allocation, a stride beyond their planes apart: an odd
        # number of floats where the planes take single pixels anyway, 8 where they take four (the cosine kernel walks the views
        # of a batch in one width: views of mixed alignment are refused by `losses.cos_loss`, so they have no oracle)
        pad = 8 if (H * W) % 4 == 0 else 5
        big = torch.zeros(B, n + pad, device=data.device)
        big[:, :n] = data.reshape(B, n)
        t = big[:, :n].view(B, C, H, W)
    elif layout == "offset":                          # a base that is only 4-byte aligned
        big = torch.zeros(B * n + 1, device=data.device)
        big[1:] = data.reshape(-1)
        t = big[1:].view(B, C, H, W)
        assert t.data_ptr() % 16 == 4
    return t.detach().requires_grad_(True)


def cf(t, layout):
    return t.permute(0, 3, 1, 2) if layout == "permuted" else t


def normal_pair(B, H, W, seed, empty_views=()):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(B, 3, H, W, generator=g)
    b = (a + 0.02 * torch.randn(B, 3, H, W, generator=g)).clamp(0, 1)
    # a quarter of the pixels: the same unit normal in both images (cos = 1: not selected)
    pick = torch.rand(B, H, W, generator=g) < 0.25
    axis = AXES[torch.randint(0, 4, (B, H, W), generator=g)].permute(0, 3, 1, 2)
    a = torch.where(pick[:, None], axis, a)
    b = torch.where(pick[:, None], axis, b)
    for v in empty_views:
        a[v] = axis[v]
        b[v] = axis[v]
    return a.to(DEV), b.to(DEV)


def check_consistency(B, H, W, layout, empty_views=(), seed=0, weight=1.0):
    a0, b0 = normal_pair(B, H, W, seed + 7 * B + H, empty_views)
    a, b = place(a0, layout), place(b0, layout)
    loss = S.consistency_loss(a, b, THR, weight)
    ga, gb = torch.autograd.grad(loss * 0.37, (a, b))
    want = L.cos_loss(cf(a, layout), cf(b, layout).detach(), None, THR, weight)
    wa, = torch.autograd.grad(want * 0.37, a)
    wb, = torch.autograd.grad(L.cos_loss(cf(b, layout), cf(a, layout).detach(), None, THR, weight) * 0.37, b)
    assert same(loss.detach(), want.detach()), (loss.item(), want.item())
    assert ga.shape == a.shape and gb.shape == b.shape
    assert same(ga, wa) and same(gb, wb)
    # again: the same bits
    loss2 = S.consistency_loss(a, b, THR, weight)
    ga2, gb2 = torch.autograd.grad(loss2 * 0.37, (a, b))
    assert same(loss2.detach(), loss.detach()) and same(ga2, ga) and same(gb2, gb)
    return loss.detach(), ga, gb


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("B", [1, 2, 5, 8, 9])
def test_consistency_equals_the_cosine_kernel_both_ways(shape, B):
    loss, ga, gb = check_consistency(B, *shape, "planar")
    if shape != (1, 1):
        assert torch.isfinite(loss) and ga.abs().max() > 0 and gb.abs().max() > 0 and (ga == 0).any()


@pytest.mark.parametrize("layout", ["permuted", "strided", "offset"])
@pytest.mark.parametrize("shape,B", [((16, 16), 2), ((37, 53), 9), ((1, 1), 5)])
def test_consistency_layouts(layout, shape, B):
    check_consistency(B, *shape, layout)


def test_consistency_view_and_batch_without_a_selected_pixel():
    loss, ga, gb = check_consistency(5, 16, 16, "planar", empty_views=(1, 4))
    assert torch.isfinite(loss) and not ga[1].any() and not gb[4].any() and ga[0].any()
    loss, ga, gb = check_consistency(9, 37, 53, "permuted", empty_views=(8,))
    assert torch.isfinite(loss) and not ga[8].any()
    loss, ga, gb = check_consistency(2, 16, 16, "planar", empty_views=(0, 1))
    assert torch.isnan(loss) and not ga.any() and not gb.any()                 # NaN value, zero gradients: the reference's empty mean


@pytest.mark.parametrize("shape,B,layout", [((16, 16), 2, "planar"), ((37, 53), 5, "permuted"), ((16, 16), 9, "offset")])
def test_consistency_with_a_weight_that_is_no_power_of_two(shape, B, layout):
    """weight = 0.3: the product with the weight rounds, so a kernel that fused differently from the cosine kernel would show"""
    loss, ga, gb = check_consistency(B, *shape, layout, weight=0.3)
    assert torch.isfinite(loss) and ga.any() and gb.any()


def nudge(x, steps):
    """x moved by `steps` (an integer tensor, either sign) float32 ulps"""
    out = x.clone()
    for k in range(1, int(steps.abs().max()) + 1):
        up, down = steps >= k, steps <= -k
        out = torch.where(up, torch.nextafter(out, torch.full_like(out, 2.0)), out)
        out = torch.where(down, torch.nextafter(out, torch.full_like(out, -1.0)), out)
    return out


@pytest.mark.parametrize("B", [2, 8])
def test_consistency_on_the_selection_boundary(B):
    """both images hold the same non-axis unit normals up to 0..3 ulps: every cosine lies within a few ulps of cos(thrsh), where the
    selection sits on the last rounding of the sum (16x16: the four-pixel walk)"""
    g = torch.Generator().manual_seed(40 + B)
    n = torch.nn.functional.normalize(torch.randn(B, 3, 16, 16, generator=g), dim=1)
    a0 = ((n + 1) / 2)
    b0 = nudge(a0, torch.randint(-3, 4, a0.shape, generator=g))
    a, b = place(a0.to(DEV), "planar"), place(b0.to(DEV), "planar")
    thr = 0.0                                          # cos < 1
    loss = S.consistency_loss(a, b, thr)
    ga, gb = torch.autograd.grad(loss, (a, b))
    want = L.cos_loss(a, b.detach(), None, thr)
    wa, = torch.autograd.grad(want, a)
    wb, = torch.autograd.grad(L.cos_loss(b, a.detach(), None, thr), b)
    picked = (wa != 0).any(1)
    print(f"\nB={B}: {int(picked.sum())} of {picked.numel()} pixels selected")
    assert 0 < int(picked.sum()) < picked.numel()
    assert same(loss.detach(), want.detach()) and same(ga, wa) and same(gb, wb)
    assert torch.equal((ga != 0).any(1), picked) and torch.equal((gb != 0).any(1), picked)


def test_consistency_views_of_mixed_alignment_walk_single_pixels():
    """16x16 views 773 floats apart: view 0 is 16-byte aligned, view 1 is not.  `losses.cos_loss` refuses such a batch; here all views
    then walk single pixels -- like a contiguous copy of the batch at an odd base, which has an oracle (test_consistency_layouts)"""
    a0, b0 = normal_pair(2, 16, 16, 91)
    n = 3 * 16 * 16

    def odd_stride(data):
        big = torch.zeros(2, n + 5, device=DEV)
        big[:, :n] = data.reshape(2, n)
        t = big[:, :n].view(2, 3, 16, 16)
        assert t[0].data_ptr() % 16 == 0 and t[1].data_ptr() % 16 != 0
        return t.detach().requires_grad_(True)

    a, b = odd_stride(a0), odd_stride(b0)
    loss = S.consistency_loss(a, b, THR)
    ga, gb = torch.autograd.grad(loss * 0.37, (a, b))
    c, d = place(a0, "offset"), place(b0, "offset")
    want = S.consistency_loss(c, d, THR)
    wa, wb = torch.autograd.grad(want * 0.37, (c, d))
    oracle = L.cos_loss(c, d.detach(), None, THR)
    assert same(loss.detach(), want.detach()) and same(want.detach(), oracle.detach()) and same(ga, wa) and same(gb, wb)


def test_consistency_second_trip_of_the_walk():
    """520x512 pixels from an odd base: 1040 workgroups' worth of single pixels against the 1024 a walk has"""
    check_consistency(1, 520, 512, "offset")


# ---- the two normal views ------------------------------------------------------------------------------------------------------
def normal_view_case(Rr, layout, seed, with_B=True):
    g = torch.Generator().manual_seed(seed)
    cn = place(torch.rand(2, 3, Rr, Rr, generator=g).to(DEV), layout)
    cm = place(torch.rand(2, 1, Rr, Rr, generator=g).to(DEV), layout)
    if layout in ("strided", "offset"):               # the plugin hands [V,R,R,C] views: permute these too
        cn, cm = cn.detach().permute(0, 2, 3, 1).requires_grad_(True), cm.detach().permute(0, 2, 3, 1).requires_grad_(True)
    gF = torch.rand(1, Rr, Rr, 3, generator=g).to(DEV)                  # interleaved, as the data module hands them
    gB = torch.rand(1, Rr, Rr, 3, generator=g).to(DEV) if with_B else None
    # a fractional float mask: 0, values below and above the 1e-5 selection, 0.3, 1
    levels = torch.tensor([0.0, 5e-6, 2e-5, 0.3, 1.0, 1.0])
    gm = levels[torch.randint(0, 6, (1, Rr, Rr), generator=g)].to(DEV)
    if Rr == 1:
        gm[:] = 0.3
    # where the mask image equals the target mask the L1 gradient is sign(0) = 0
    with torch.no_grad():
        eq = (torch.rand(Rr, Rr, generator=g) < 0.2).to(DEV)
        cm_cf = cm if layout == "planar" else cm.permute(0, 3, 1, 2)
        cm_cf[0, 0][eq] = gm[0][eq]
    return cn, cm, gF, gB, gm


def normal_view_oracle(cn, cm, gF, gB, gm, layout):
    cn_cf = cn if layout == "planar" else cn.permute(0, 3, 1, 2)
    cm_cf = cm if layout == "planar" else cm.permute(0, 3, 1, 2)
    sel = gm > 1e-5
    out = {"cos_F": 0.2 * L.cos_loss(cn_cf[0], gF.permute(0, 3, 1, 2)[0], sel, thrsh=0, weight=1),
           "cos_B": None if gB is None else 0.2 * L.cos_loss(cn_cf[1], gB.permute(0, 3, 1, 2)[0], sel, thrsh=0, weight=1),
           "mask_l1": L.masked_l1(cm_cf[0], gm)}
    cn_last = cn_cf.permute(0, 2, 3, 1)
    mf, mb = gm[..., None], sel.float()[..., None]
    f = lambda x, m: ((x * m).permute(0, 3, 1, 2) - 0.5) * 2
    rows = [f(cn_last[[0]], mf)] + ([f(cn_last[[1]], mb)] if gB is not None else []) + [f(gF, mf)] + ([f(gB, mb)] if gB is not None else [])
    out["lpips_in"] = torch.cat(rows, 0)
    return out


@pytest.mark.parametrize("layout", ["planar", "permuted", "strided", "offset"])
@pytest.mark.parametrize("Rr", [1, 16, 37])
@pytest.mark.parametrize("with_B", [True, False])
def test_normal_view_terms(Rr, layout, with_B):
    cn, cm, gF, gB, gm = normal_view_case(Rr, layout, 100 + Rr, with_B)
    views = 2 if with_B else 1
    out = S.normal_view_terms(cn, cm, gF, gB, gm)
    want = normal_view_oracle(cn, cm, gF, gB, gm, layout)
    keys = ["cos_F", "cos_B", "mask_l1"] if with_B else ["cos_F", "mask_l1"]
    for k in keys:
        print(f"\nR={Rr} {layout} {k}: {out[k].item():.9g} against {want[k].item():.9g}")
        assert same(out[k].detach(), want[k].detach()), k
    assert (out["cos_B"] is None) == (not with_B)
    assert out["lpips_in"].shape == (2 * views, 3, Rr, Rr) and out["lpips_in"].is_contiguous()
    assert same(out["lpips_in"].detach(), want["lpips_in"].detach())
    # the asymmetry is visible: a fractional mask scales the front view, the back view only sees 0 / 1
    if Rr > 1 and with_B:
        frac = ((gm > 1e-5) & (gm < 1))[0]
        assert frac.any()
        x = cn.detach() if layout == "planar" else cn.detach().permute(0, 3, 1, 2)
        assert same(out["lpips_in"][1, :, frac], ((x[1][:, frac] * 1.0) - 0.5) * 2)
        assert not same(out["lpips_in"][0, :, frac], ((x[0][:, frac] * 1.0) - 0.5) * 2)

    w = torch.tensor([0.7, 1.3, 0.45], device=DEV)
    U = torch.randn(out["lpips_in"].shape, generator=torch.Generator().manual_seed(5)).to(DEV)

    def total(o, cos=True, lp=True):
        t = 0.0
        if cos:
            t = o["cos_F"] * w[0] + o["mask_l1"] * w[2] + (o["cos_B"] * w[1] if o["cos_B"] is not None else 0.0)
        if lp:
            t = t + (o["lpips_in"] * U).sum()
        return t

    # one term at a time: bit for bit
    g_cos, g_m = torch.autograd.grad(total(out, lp=False), (cn, cm), retain_graph=True)
    w_cos, w_m = torch.autograd.grad(total(want, lp=False), (cn, cm), retain_graph=True)
    assert g_cos.shape == cn.shape and g_m.shape == cm.shape
    assert same(g_cos, w_cos) and same(g_m, w_m)
    if Rr > 1:
        assert (g_m[0] == 0).any() and (g_m[0] != 0).any() and not g_m[1].any()
        if not with_B:
            assert not g_cos[1].any()
    g_lp, = torch.autograd.grad(total(out, cos=False), cn, retain_graph=True)
    w_lp, = torch.autograd.grad(total(want, cos=False), cn, retain_graph=True)
    assert same(g_lp, w_lp)
    # both: one float32 addition, at most 1 ulp of the larger addend
    g_all, g_m2 = torch.autograd.grad(total(out), (cn, cm), retain_graph=True)
    err = (g_all - (w_cos + w_lp)).abs()
    bound = ulp(torch.maximum(w_cos.abs(), w_lp.abs()))
    print(f"cos + lpips gradient: largest error {float((err / bound.clamp_min(1e-45)).max()):.2f} ulp of the larger addend")
    assert (err <= bound).all() and same(g_m2, w_m)
    # again: the same bits
    out2 = S.normal_view_terms(cn, cm, gF, gB, gm)
    g_all2, g_m3 = torch.autograd.grad(total(out2), (cn, cm))
    assert all(same(out2[k].detach(), out[k].detach()) for k in keys + ["lpips_in"]) and same(g_all2, g_all) and same(g_m3, g_m2)


@pytest.mark.parametrize("Rr", [16, 32])
def test_normal_views_on_the_selection_boundary(Rr):
    """The rendered normals equal non-axis unit targets up to 0..3 ulps -- what training converges to, and exactly the `thrsh=0`
    boundary cos < 1.  Aligned planes, R R a multiple of 4: the four-pixel walk.  The selected counts and the zero pattern of the
    gradient are those of `losses.cos_loss`: forward, backward and the cosine kernel select the same pixels."""
    g = torch.Generator().manual_seed(60 + Rr)
    unit = lambda: (torch.nn.functional.normalize(torch.randn(1, Rr, Rr, 3, generator=g), dim=-1) + 1) / 2
    gF, gB = unit().to(DEV), unit().to(DEV)
    cn0 = torch.cat([nudge(gF.cpu(), torch.randint(-3, 4, gF.shape, generator=g)), nudge(gB.cpu(), torch.randint(-3, 4, gB.shape, generator=g))])
    cn = place(cn0.permute(0, 3, 1, 2).contiguous().to(DEV), "permuted")
    cm = place(torch.rand(2, 1, Rr, Rr, generator=g).to(DEV), "permuted")
    gm = (torch.rand(1, Rr, Rr, generator=g) < 0.9).float().to(DEV)
    out = S.normal_view_terms(cn, cm, gF, gB, gm)
    want = normal_view_oracle(cn, cm, gF, gB, gm, "permuted")
    w = torch.tensor([0.7, 1.3, 0.45], device=DEV)
    tot = lambda o: o["cos_F"] * w[0] + o["cos_B"] * w[1] + o["mask_l1"] * w[2]
    g_n, = torch.autograd.grad(tot(out), cn)
    w_n, = torch.autograd.grad(tot(want), cn)
    picked = (w_n != 0).any(-1)                                     # [2,R,R]: a selected pixel has a non-zero gradient (unit targets)
    counts = picked.reshape(2, -1).sum(1)
    print(f"\nR={Rr}: {counts.tolist()} of {Rr * Rr} pixels selected; stats {out['stats'].tolist()}")
    assert all(0 < int(c) < int(gm.sum()) for c in counts)
    assert float(out["stats"][1]) == float(counts[0]) and float(out["stats"][3]) == float(counts[1])
    assert torch.equal((g_n != 0).any(-1), picked) and same(g_n, w_n)
    for k in ("cos_F", "cos_B", "mask_l1", "lpips_in"):
        assert same(out[k].detach(), want[k].detach()), k


# ---- loss_occ, the blended target, mean|x| -------------------------------------------------------------------------------------
def frame_case(H, W, seed, empty=False, colour=True):
    g = torch.Generator().manual_seed(seed)
    occ = torch.rand(1, 3, H, W, generator=g).to(DEV).permute(0, 2, 3, 1).requires_grad_(True)      # the plugin's layout
    rgb = torch.rand(1, H, W, 3, generator=g).to(DEV)
    levels = torch.tensor([0.0, 0.0, 1e-7, 0.4, 1.0])
    m = levels[torch.randint(0, 5, (1, H, W), generator=g)].to(DEV)
    if empty:
        m.zero_()
    elif H * W == 1:
        m[:] = 0.4
    c = torch.rand(3, generator=g).to(DEV)
    bg = c if colour else torch.ones_like(rgb) * c
    return occ, rgb, m, bg


@pytest.mark.parametrize("shape", SHAPES + [(520, 512)])
@pytest.mark.parametrize("colour", [True, False])
def test_frame_extra_terms(shape, colour):
    occ, rgb, m, bg = frame_case(*shape, 31 + shape[0], colour=colour)
    out = S.frame_extra_terms(occ, rgb, m, bg)
    assert out["gt_rgb_blended"].shape == rgb.shape
    assert same(out["gt_rgb_blended"], rgb * m[..., None] + bg * (1 - m[..., None]))
    ref = R.loss_occ(occ.detach().cpu(), m.cpu(), torch.float64)
    err = abs(out["loss_occ"].item() - ref.item()) / ulp(ref).item()
    print(f"\n{shape}: loss_occ {out['loss_occ'].item():.9g}, float64 {ref.item():.12g}, {err:.2f} ulp")
    assert err <= 2.0
    up = torch.tensor(0.37, device=DEV)
    g, = torch.autograd.grad(out["loss_occ"] * up, occ)
    sel = (m > 0)[..., None].expand_as(occ)
    count = sel.sum().to(torch.float32)
    assert float(out["stats"][1]) == float(count)
    assert g.shape == occ.shape and same(g, torch.where(sel, -quotient(up, count), torch.zeros((), device=DEV)))
    out2 = S.frame_extra_terms(occ, rgb, m, bg)
    g2, = torch.autograd.grad(out2["loss_occ"] * up, occ)
    assert same(out2["loss_occ"].detach(), out["loss_occ"].detach()) and same(g2, g) and same(out2["gt_rgb_blended"], out["gt_rgb_blended"])


def test_frame_extra_terms_empty_mask():
    occ, rgb, m, bg = frame_case(37, 53, 3, empty=True)
    out = S.frame_extra_terms(occ, rgb, m, bg)
    assert torch.isnan(out["loss_occ"]) and torch.isnan(R.loss_occ(occ.detach().cpu(), m.cpu()))
    g, = torch.autograd.grad(out["loss_occ"], occ)
    assert not g.any() and not torch.isnan(g).any()
    assert same(out["gt_rgb_blended"], (torch.ones_like(rgb) * bg).contiguous())


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 16, 16), (4, 37, 53), (1, 520, 512)])
@pytest.mark.parametrize("layout", ["permuted", "offset"])
def test_abs_mean(shape, layout):
    B, H, W = shape
    g = torch.Generator().manual_seed(B + H)
    data = torch.randn(B, 1, H, W, generator=g)
    data[torch.rand(B, 1, H, W, generator=g) < 0.3] = 0.0                  # exact zeros: sign = 0
    if H * W == 1:
        data[:] = -0.75
    x = place(data.to(DEV), layout)
    v = S.abs_mean(x)
    ref = R.abs_mean(x.detach().cpu())
    err = abs(v.item() - ref.item()) / ulp(ref).item()
    print(f"\n{shape} {layout}: mean|x| {v.item():.9g}, float64 {ref.item():.12g}, {err:.2f} ulp")
    assert err <= 2.0
    up = torch.tensor(0.37, device=DEV)
    gx, = torch.autograd.grad(v * up, x)
    assert gx.shape == x.shape and same(gx, torch.sign(x.detach()) * quotient(up, x.numel()))
    if H * W > 1:
        assert (gx == 0).any()
    v2 = S.abs_mean(x)
    gx2, = torch.autograd.grad(v2 * up, x)
    assert same(v2.detach(), v.detach()) and same(gx2, gx)


def test_cpu_tensors_are_refused():
    z = torch.zeros(1, 4, 4, 3)
    for call in (lambda: S.consistency_loss(z, z), lambda: S.abs_mean(z), lambda: S.frame_extra_terms(z, z, z[..., 0], z[0, 0, 0]),
                 lambda: S.normal_view_terms(z, z[..., :1], z, None, z[..., 0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
