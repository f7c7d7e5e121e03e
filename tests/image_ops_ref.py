"""Float64 references and the case tables of the image-space loss and post-op kernels (soar_amd/csrc/ssim.hip, image_losses.hip,
postops.hip).  TEST INFRASTRUCTURE: only tests/ import this module (tests/test_image_ops_cpu.py checks the references themselves and
the room the bars leave, tests/test_image_ops_gpu.py holds the kernels to them).

Plain torch on the CPU, float64 throughout, differentiated by autograd.

* SSIM, masked L1, cosine loss: oracle/loss_oracle.py is dtype-generic; called with float64 tensors it IS the reference.
* depth2normal / normal2curv / view_finish: restated here.  oracle/postops_oracle.py builds its pixel coordinates in float32 whatever
  the input, and its F.normalize has a noisy gradient even in float64: where the summed cross products N vanish -- fewer than two
  independent differences survive the mask or the replicate padding, each of the others is (x - x) or (...) * 0 -- N / max(|N|, 1e-12)
  is the linear map 1e12 N, and the +-1e12-scaled pairs of its gradient cancel only to rounding.  Here N is divided by
  where(|N| > 1e-12, |N|, 1): the gradient of such a pixel is exactly zero, which is the rule postops.hip documents."""
from __future__ import annotations

import math
import types

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss_oracle as lo

F64 = torch.float64

# ---- the bars of the GPU tests, all against float64 (the project's existing ones: tests/test_plugin_gpu.py) ----
SSIM_VALUE_BAR, SSIM_GRAD_BAR = 2e-6, 1e-4              # absolute; max-norm relative
D2N_VALUE_BAR, D2N_GRAD_BAR, D2N_GRAD_L2_BAR = 2e-5, 2e-4, 1e-4
N2C_VALUE_BAR, N2C_GRAD_BAR = 5e-6, 1e-5
LOSS_VALUE_BAR, LOSS_GRAD_BAR = 1e-5, 1e-4              # value: 1e-5 * max(1, |v|)
FLAT_SSIM_FACTOR = 4.0                                  # flat SSIM cases: the kernel may be this many times the float32 oracle's distance


def rel_max(a, b) -> float:
    """largest element of |a - b| relative to the largest of |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rel_l2(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# =====================================================================================================================================
# SSIM
# =====================================================================================================================================
# (name, (C, H, W), kind): kind "plain" | "misaligned" (a contiguous view one float into its allocation) | "flat"
SSIM_CASES = [
    ("one_pixel", (1, 1, 1), "plain"),                  # scalar path
    ("one_column", (3, 4, 1), "plain"),                 # scalar path
    ("narrowest_vector", (3, 1, 4), "plain"),           # the clamped 16-byte unit address is W - 4 = 0
    ("below_radius", (1, 5, 8), "plain"),               # height at most the window radius
    ("window_height", (3, 11, 12), "plain"),            # height equal to the window
    ("one_tile", (2, 32, 32), "plain"),
    ("into_next_tiles", (3, 33, 36), "plain"),          # one row and four columns into the next tiles, 16-byte path
    ("around_a_tile_scalar", (1, 31, 33), "plain"),     # one short of / one past a tile, scalar path
    ("seams_vector", (3, 64, 68), "plain"),             # 2 x 3 tiles
    ("seams_scalar", (3, 65, 67), "plain"),             # 3 x 3 tiles
    ("second_tile_row", (3, 43, 100), "plain"),         # 2 x 4 tiles, rows 32 .. 42 in the second row of tiles
    ("misaligned", (3, 33, 36), "misaligned"),          # W % 4 == 0 but no 16-byte alignment: the scalar kernels
    ("flat_vector", (3, 64, 68), "flat"),               # a frame of one person: constant colour around a 25 x 26 patch
    ("flat_scalar", (3, 65, 67), "flat"),
]
SSIM_IDS = [c[0] for c in SSIM_CASES]
FLAT_COLOUR = (0.2, 0.5, 0.7)
FLAT_PATCH = (21, 19, 25, 26)                           # y0, x0, height, width: across the seams of the first tiles


def ssim_case(name):
    return next(c for c in SSIM_CASES if c[0] == name)


def ssim_images(shape, seed):
    """a = rand, b = clamp(a + 0.2 randn, 0, 1): float32 [C,H,W]"""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(*shape, generator=g)
    b = (a + 0.2 * torch.randn(*shape, generator=g)).clamp(0, 1)
    return a, b


def ssim_inputs(case):
    """float32 images (img1, img2) of a case; content depends on the case alone"""
    name, shape, kind = case
    seed = 100 + SSIM_IDS.index(name)
    a, b = ssim_images(shape, seed)
    if kind == "flat":
        y0, x0, ph, pw = FLAT_PATCH
        col = torch.tensor(FLAT_COLOUR, dtype=torch.float32)[:, None, None]
        fa, fb = col.expand(shape).clone(), col.expand(shape).clone()
        fa[:, y0:y0 + ph, x0:x0 + pw] = a[:, y0:y0 + ph, x0:x0 + pw]
        fb[:, y0:y0 + ph, x0:x0 + pw] = b[:, y0:y0 + ph, x0:x0 + pw]
        a, b = fa, fb
    return a, b


def ssim_ref(a, b, dtype=F64):
    """mean SSIM and its gradient w.r.t. the first image by oracle/loss_oracle.py in `dtype`: (float, tensor [C,H,W])"""
    x = a.detach().to(dtype).clone().requires_grad_(True)
    v = lo.ssim(x, b.detach().to(dtype))
    v.backward()
    return float(v.detach()), x.grad


SSIM_TILE = 32


def ssim_rendered_cases(shape):
    """(name, rendered [H,W] float32) of soar_ssim_rendered's opacity images: one pixel above 1e-5 in the middle tile, in a corner
    tile, in the last (partial) tile; nothing rendered; everything rendered"""
    _, H, W = shape
    ty, tx = (H + SSIM_TILE - 1) // SSIM_TILE, (W + SSIM_TILE - 1) // SSIM_TILE

    def one(y, x):
        r = torch.zeros(H, W)
        r[y, x] = 0.9
        return r
    mid = ((ty - 1) // 2 * SSIM_TILE + 9, (tx - 1) // 2 * SSIM_TILE + 8)
    return [("centre", one(*mid)), ("corner", one(3, 5)), ("last", one(H - 1, W - 1)), ("none", torch.zeros(H, W)), ("all", torch.ones(H, W))]


def ssim_tile_mask(rendered):
    """[H,W] bool: the pixels of the 32 x 32 tiles that hold a pixel with rendered > 1e-5"""
    H, W = rendered.shape
    out = torch.zeros(H, W, dtype=torch.bool)
    for y0 in range(0, H, SSIM_TILE):
        for x0 in range(0, W, SSIM_TILE):
            if bool((rendered[y0:y0 + SSIM_TILE, x0:x0 + SSIM_TILE] > 1e-5).any()):
                out[y0:y0 + SSIM_TILE, x0:x0 + SSIM_TILE] = True
    return out


# =====================================================================================================================================
# post-ops
# =====================================================================================================================================
POSTOP_CASES = [(1, 1), (1, 9), (9, 1), (2, 2), (8, 32), (9, 33), (3, 65), (17, 31)]        # (H, W); the block is 32 x 8
POSTOP_IDS = [f"{h}x{w}" for h, w in POSTOP_CASES]
DEGENERATE_POSTOP_CASES = [(1, 1), (1, 9), (9, 1)]      # no pixel has two independent differences: the depth normal is zero everywhere
PRCP = (0.47, 0.55)
FOVX, FOVY = 1.1, 0.8
# amplitude of the surface's random term.  At 3 x 65 the focal of a 3-pixel height puts x / K00 near 9, the differences cancel most of
# the points' digits, and with the older test's 0.02 the float32 oracle sits 1e-5 from float64 -- half the value bar; 0.05 and 0.15 are
# no better (up to 2e-5 over four seeds), 1.0 keeps every case below 6.1e-6
DEPTH_ROUGHNESS = 1.0
OPAC_LIMIT = np.float32(1e-5)
SIGNS = (1.0, -1.0, -1.0)


def fov2focal(fov, pixels):
    return pixels / (2 * math.tan(fov / 2))


def focals(H, W):
    """(k00, k11) as the C ABI receives them: float32 values of focal(FoVy, H) -- applied to x -- and focal(FoVx, W) -- to y"""
    return float(np.float32(fov2focal(FOVY, H))), float(np.float32(fov2focal(FOVX, W)))


def camera(H, W):
    """the camera of a case as oracle/postops_oracle.py and soar_amd.renderer.postops take it"""
    return types.SimpleNamespace(prcppoint=torch.tensor(PRCP, dtype=torch.float32), image_width=W, image_height=H, FoVx=FOVX, FoVy=FOVY)


def postop_inputs(hw, seed_offset=0):
    """float32 inputs of a post-op case: depth [1,H,W] (a smooth surface with roughness), mask [1,H,W] bool (about 30 % outside), normal
    [3,H,W] (unit), upstream gradients of the depth normal [3,H,W] and of the curvature [1,H,W]"""
    H, W = hw
    g = torch.Generator().manual_seed(1000 * H + W + 7919 * seed_offset)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    depth = (2.0 + 0.3 * torch.sin(xx / 7.0) * torch.cos(yy / 5.0) + DEPTH_ROUGHNESS * torch.rand(H, W, generator=g))[None]
    mask = torch.rand(1, H, W, generator=g) > 0.3
    if hw == (2, 2):                                    # one pixel outside: a normal from two differences, two pixels left with one, a masked centre
        mask = torch.tensor([[[True, True], [True, False]]])
    normal = F.normalize(torch.randn(3, H, W, generator=g), dim=0)
    up_n, up_c = torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g)
    return types.SimpleNamespace(depth=depth, mask=mask, normal=normal, up_n=up_n, up_c=up_c)


def _stencil(img_hwc, mask_hw1):
    """centre value and the four masked neighbour differences on a replicate-padded grid, in the image's dtype"""
    p = F.pad(img_hwc.permute(2, 0, 1)[None], [1, 1, 1, 1], mode="replicate")[0].permute(1, 2, 0)
    m = F.pad(mask_hw1.permute(2, 0, 1)[None].to(torch.float32), [1, 1, 1, 1], mode="replicate")[0].permute(1, 2, 0).to(img_hwc.dtype)
    c = p[1:-1, 1:-1] * m[1:-1, 1:-1]
    u = (p[:-2, 1:-1] - c) * m[:-2, 1:-1]
    l = (p[1:-1, :-2] - c) * m[1:-1, :-2]
    b = (p[2:, 1:-1] - c) * m[2:, 1:-1]
    r = (p[1:-1, 2:] - c) * m[1:-1, 2:]
    return u, l, b, r, m[1:-1, 1:-1]


def depth2normal_N(depth, mask, prcp=PRCP, k=None):
    """the summed cross products N [H,W,3] of depth [1,H,W] in the depth's dtype.  cx W and cy H are the float32 products the kernel
    forms, taken to that dtype; everything after that is in that dtype."""
    H, W = depth.shape[-2:]
    dt = depth.dtype
    k00, k11 = focals(H, W) if k is None else k
    cxW = float(np.float32(prcp[0]) * np.float32(W))
    cyH = float(np.float32(prcp[1]) * np.float32(H))
    hh, ww = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    d = depth[0]
    pts = torch.stack([(ww - cxW) * d / k00, (hh - cyH) * d / k11, d], -1)
    u, l, b, r, m = _stencil(pts, mask.permute(1, 2, 0))
    N = torch.linalg.cross(u, l, dim=-1) + torch.linalg.cross(r, u, dim=-1) + torch.linalg.cross(b, r, dim=-1) + torch.linalg.cross(l, b, dim=-1)
    return N, m


def depth2normal(depth, mask, prcp=PRCP, k=None, form="where"):
    """depth [1,H,W] (float64 for the reference), mask [1,H,W] bool -> normals [3,H,W]:  N / where(|N| > 1e-12, |N|, 1) m.
    form="normalize": F.normalize's N / max(|N|, 1e-12) instead (the same values; for the comparison of the two gradients)."""
    N, m = depth2normal_N(depth, mask, prcp, k)
    if form == "normalize":
        n = F.normalize(N, dim=-1)
    else:
        sq = (N * N).sum(-1, keepdim=True)
        ok = sq > 1e-24
        n = N / torch.where(ok, torch.where(ok, sq, torch.ones_like(sq)).sqrt(), torch.ones_like(sq))
    return (n * m).permute(2, 0, 1)


def depth2normal_vanishing(depth, mask, prcp=PRCP, k=None):
    """[H,W] bool: where N vanishes (|N| <= 1e-12)"""
    N, _ = depth2normal_N(depth.detach(), mask, prcp, k)
    return ~((N * N).sum(-1) > 1e-24)


def normal2curv(normal, mask):
    """normal [3,H,W], mask [1,H,W] bool -> curvature proxy [1,H,W]: the L1 norm of the masked 4-neighbour Laplacian"""
    u, l, b, r, m = _stencil(normal.permute(1, 2, 0), mask.permute(1, 2, 0))
    return ((u + l + b + r) * m).abs().sum(-1)[None]


def d2n_ref(depth, mask, up, dtype=F64, form="where"):
    """values [3,H,W] and the gradient [1,H,W] of sum(out * up) w.r.t. the depth, in `dtype`"""
    d = depth.detach().to(dtype).clone().requires_grad_(True)
    out = depth2normal(d, mask, form=form)
    (out * up.to(dtype)).sum().backward()
    return out.detach(), d.grad


def n2c_ref(normal, mask, up, dtype=F64):
    n = normal.detach().to(dtype).clone().requires_grad_(True)
    out = normal2curv(n, mask)
    (out * up.to(dtype)).sum().backward()
    return out.detach(), n.grad


# ---- view_finish: everything the plugin does to a view behind the rasterizer, as include/soar_hip.h states it ----
VIEW_COMBOS = [("all", (1, 1, 1, 1)), ("normal_out+depth_direct", (1, 0, 0, 1)), ("curv", (0, 1, 0, 0)), ("pred", (0, 0, 1, 0)),
               ("depth_direct", (0, 0, 0, 1))]          # which of dL/dnormal_out, dL/dcurv, dL/dpred_normal, dL/ddepth_direct are given
VIEW_COMBO_IDS = [c[0] for c in VIEW_COMBOS]


def view_inputs(hw, seed_offset=0):
    """float32 inputs of a view_finish case.  The opacity image is random with about 30 % at or below the limit and holds, where they
    fit: the limit 1e-5f itself (outside), the next float above it (inside), 0 and 1, and a 3 x 3 region entirely outside -- the
    kernel's shortcut branch at its centre -- with the unit normals every pixel has under it."""
    H, W = hw
    base = postop_inputs(hw, seed_offset)
    g = torch.Generator().manual_seed(31 * H + W + 104729 * seed_offset)
    opac = torch.rand(1, H, W, generator=g)
    opac = torch.where(opac > 0.3, opac, 1e-5 * torch.rand(1, H, W, generator=g)).reshape(-1)
    above = float(np.nextafter(OPAC_LIMIT, np.float32(1)))
    special = [float(OPAC_LIMIT), above, 0.0, 1.0]
    n = H * W
    at = {}
    for i, v in enumerate(special):
        if n >= 4:
            j = (i * (n - 1)) // 3
            opac[j] = v
            at[j] = v
    opac = opac.reshape(1, H, W).clone()
    hole = None
    if H >= 3 and W >= 3:
        y0, x0 = (H - 3) // 2, max((W - 3) // 2 - 1, 0)
        opac[0, y0:y0 + 3, x0:x0 + 3] = 0.0
        for j, v in at.items():                         # (a special pixel wins where it falls into the region; checked below)
            opac[0, j // W, j % W] = v
        if not bool((opac[0, y0:y0 + 3, x0:x0 + 3] > 1e-5).any()):
            hole = (y0 + 1, x0 + 1)
    up_no, up_pred = torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g)
    up_dd = torch.randn(1, H, W, generator=g)
    return types.SimpleNamespace(depth=base.depth, normal=base.normal, opac=opac, up_no=up_no, up_curv=base.up_c, up_pred=up_pred,
                                 up_dd=up_dd, special=at, hole=hole, above=above)


def view_mask(opac):
    """mask = opac > 1e-5, compared in float32"""
    return opac.to(torch.float32) > torch.tensor(OPAC_LIMIT)


def view_finish(normal, depth, opac):
    """(normal_out [3,H,W], curv [1,H,W], pred_normal [3,H,W]) in the dtype of normal / depth"""
    mask = view_mask(opac)
    s = torch.tensor(SIGNS, dtype=normal.dtype)[:, None, None]
    no = (normal * s + 1) / 2
    normal_out = torch.where(mask, no, no.detach())                 # gradient only inside the mask
    curv = normal2curv(normal * s, mask)
    pred = (depth2normal(depth, mask) * s + 1) / 2
    return normal_out, curv, pred


def view_finish_ref(v, combo=None, dtype=F64):
    """values and, for a combination of incoming gradients, the result block [4,H,W] = dL/dnormal [3] then dL/ddepth [1]"""
    n = v.normal.detach().to(dtype).clone().requires_grad_(True)
    d = v.depth.detach().to(dtype).clone().requires_grad_(True)
    normal_out, curv, pred = view_finish(n, d, v.opac)
    if combo is None:
        return normal_out.detach(), curv.detach(), pred.detach()
    use_no, use_c, use_p, use_dd = combo
    L = (n * 0).sum() + (d * 0).sum()
    if use_no:
        L = L + (normal_out * v.up_no.to(dtype)).sum()
    if use_c:
        L = L + (curv * v.up_curv.to(dtype)).sum()
    if use_p:
        L = L + (pred * v.up_pred.to(dtype)).sum()
    if use_dd:
        L = L + (d * v.up_dd.to(dtype)).sum()
    L.backward()
    return torch.cat([n.grad, d.grad], 0)


# =====================================================================================================================================
# masked L1 and cosine loss
# =====================================================================================================================================
# (name, (H, W), mask kind): "random" | "offset1" (the mask is a view at byte offset 1 of its allocation) | "empty" (all false)
LOSS_CASES = [
    ("1x1", (1, 1), "random"),                          # scalar
    ("1x3", (1, 3), "random"),                          # scalar
    ("2x2", (2, 2), "random"),                          # n = 4: one vector
    ("16x17", (16, 17), "random"),                      # an odd width, but n = 272 is a multiple of 4: the vector walk
    ("15x17", (15, 17), "random"),                      # scalar, n = 255: one thread short of a block
    ("37x52_mask_offset", (37, 52), "offset1"),         # vector images, a mask that must drop the walk to the scalar path
    ("16x17_empty_mask", (16, 17), "empty"),
    ("2x2_empty_mask", (2, 2), "empty"),
    ("513x513_second_trip", (513, 513), "random"),      # scalar, n = 263 169 > 1024 * 256
    ("1026x1024_second_trip", (1026, 1024), "random"),  # vector, n / 4 = 262 656 > 1024 * 256
]
LOSS_IDS = [c[0] for c in LOSS_CASES]
COS_SETTINGS = [(0.0, 1.0), (0.6, 0.5)]                 # (thrsh, weight)
COS_MARGIN = 1e-5                                       # no pixel's float64 cosine lies this close to cos(thrsh)
LOSS_UPSTREAM = 1.7
LOSS_BLOCKS = 1024                                      # workgroups of a loss walk at the most (soar_amd/csrc/loss_pixel.h)


def loss_case(name):
    return next(c for c in LOSS_CASES if c[0] == name)


def loss_walk(case, masked=True):
    """(16-byte path?, trips of the grid-stride loop) of a case with aligned images: image_losses.hip takes four pixels per thread when
    n % 4 == 0 and every plane -- the mask to 4 bytes -- is aligned, and caps its grid at LOSS_BLOCKS workgroups of 256 threads"""
    _, (H, W), kind = case
    n = H * W
    vec = n % 4 == 0 and not (masked and kind == "offset1")
    units = n // 4 if vec else n
    return vec, -(-units // (LOSS_BLOCKS * 256))


def loss_images(hw, seed):
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    o = torch.rand(H, W, 3, generator=g)
    t = F.normalize(torch.randn(H, W, 3, generator=g), dim=-1) * 0.5 + 0.5
    o = (0.5 * o + 0.5 * t).clamp(0, 1)
    m = torch.rand(H, W, generator=g) > 0.4
    if H * W == 1:
        m[:] = True
    return o, t, m


def loss_mask(case):
    name, hw, kind = case
    m = loss_images(hw, 500 + LOSS_IDS.index(name))[2]
    return torch.zeros_like(m) if kind == "empty" else m


def l1_inputs(case):
    """(img, gt, mask) as [H,W,3] float32 and [H,W] bool; a handful of elements with img == gt exactly"""
    name, hw, kind = case
    o, t, _ = loss_images(hw, 500 + LOSS_IDS.index(name))
    n = hw[0] * hw[1]
    eq = torch.zeros(n, 3, dtype=torch.bool)
    eq[0, 1] = True
    eq[n - 1, 2] = True
    if n > 4:
        eq[n // 2, :] = True
        eq[n // 3, 0] = True
    o = torch.where(eq.reshape(hw[0], hw[1], 3), t, o)
    return o, t, loss_mask(case), eq.reshape(hw[0], hw[1], 3)


def cos_of(o, t, weight):
    """float64 cosine per pixel: weight * sum_c (2 o - 1)(2 t - 1)"""
    return ((o.double() * 2 - 1) * (t.double() * 2 - 1) * weight).sum(-1)


def cos_inputs(case, thrsh, weight):
    """(output, gt, mask): the few pixels whose float64 cosine lies within COS_MARGIN of cos(thrsh) are pulled towards grey (their
    cosine shrinks by a tenth), so the selection cos < cos(thrsh) is the same in float32 and float64"""
    name, hw, kind = case
    o, t, _ = loss_images(hw, 500 + LOSS_IDS.index(name))
    limit = math.cos(thrsh)
    for _ in range(4):
        close = (cos_of(o, t, weight) - limit).abs() < 4 * COS_MARGIN
        if not bool(close.any()):
            break
        o = torch.where(close[..., None], 0.5 + 0.9 * (o - 0.5), o)
    assert float((cos_of(o, t, weight) - limit).abs().min()) >= COS_MARGIN, "a cosine sits on the threshold"
    return o, t, loss_mask(case)


def masked_l1_ref(o, t, mask, upstream=LOSS_UPSTREAM, dtype=F64):
    """(value, selected pixels, gradient [H,W,3]) of upstream * l1_loss_w(o[mask], t[mask]) by oracle/loss_oracle.py"""
    x = o.detach().to(dtype).clone().requires_grad_(True)
    y = t.detach().to(dtype)
    v = lo.l1_loss_w(x[mask], y[mask]) if mask is not None else lo.l1_loss_w(x, y)
    (upstream * v + (x * 0).sum()).backward()
    count = int(mask.sum()) if mask is not None else o.shape[0] * o.shape[1]
    return float(v.detach()), count, torch.nan_to_num(x.grad) if count == 0 else x.grad


def cos_loss_ref(o, t, mask, thrsh, weight, upstream=LOSS_UPSTREAM, dtype=F64):
    """(value, selected pixels, gradient [H,W,3]) of upstream * cos_loss(o, t, mask, thrsh, weight) by oracle/loss_oracle.py"""
    x = o.detach().to(dtype).clone().requires_grad_(True)
    y = t.detach().to(dtype)
    v = lo.cos_loss(x, y, mask, thrsh=thrsh, weight=weight)
    (upstream * v + (x * 0).sum()).backward()
    sel = ((x.detach() * 2 - 1) * (y * 2 - 1) * weight).sum(-1) < np.cos(thrsh)       # (the selection as `dtype` sees it)
    if mask is not None:
        sel = sel & mask
    count = int(sel.sum())
    return float(v.detach()), count, torch.nan_to_num(x.grad) if count == 0 else x.grad
