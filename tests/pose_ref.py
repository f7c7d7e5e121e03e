"""Plain torch / NumPy restatement of soar_amd/pose.py, written from the definition in include/soar_hip.h:

* ``RefNet``: the BODY_25 network as torch modules' functional calls, at whatever dtype its state dict has (float64 is the yardstick,
  float32 the measure of what float32 costs); it reads the layer list, the concatenation orders and nothing else from ``soar_amd.pose``.
* ``peaks_ref`` / ``assemble_ref``: the post-processing in NumPy float32, operation by operation in the order the header states, so
  that the kernels' results can be compared bit for bit.
* ``make_state_dict``: seeded random weights of any configuration; ``scene``: constructed heat maps and part-affinity fields.
"""
import numpy as np
import torch
import torch.nn.functional as F

from soar_amd import pose

TINY = dict(c1=8, c2=16, c3=16, c4=32, cpm=24, feat=16, w0=8, w1=16, m0=24, m1=32, n_paf=2, n_heat=2)
TINY_1 = dict(c1=8, c2=16, c3=16, c4=32, cpm=24, feat=16, w0=8, w1=8, m0=24, m1=24, n_paf=1, n_heat=1)
SHIPPED = dict(c1=64, c2=128, c3=256, c4=512, cpm=256, feat=128, w0=96, w1=128, m0=256, m1=512, n_paf=4, n_heat=2)
f32 = np.float32


def make_state_dict(cfg, seed=0, dtype=torch.float32):
    """He-scaled weights, small biases, PReLU slopes in [-0.2, 0.6): activations stay of order one through every stage"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for conv, prelu, shape in pose.layer_keys(cfg):
        fan_in = shape[1] * shape[2] * shape[3]
        sd[f"{conv}.weight"] = (torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).to(dtype)
        sd[f"{conv}.bias"] = (torch.randn(shape[0], generator=g, dtype=torch.float64) * 0.1).to(dtype)
        if prelu:
            sd[f"{prelu}.weight"] = (torch.rand(shape[0], generator=g, dtype=torch.float64) * 0.8 - 0.2).to(dtype)
    return sd


class RefNet(torch.nn.Module):
    """forward(x [B,3,H,W]) -> (features, [stage outputs: every L2 stage, then every L1 stage]) in NCHW"""

    def __init__(self, state_dict):
        super().__init__()
        self.cfg = pose.read_config(state_dict)
        self.keys = pose.layer_keys(self.cfg)
        self.p = torch.nn.ParameterDict({k.replace(".", "/"): torch.nn.Parameter(v.detach().clone(), requires_grad=False)
                                         for k, v in state_dict.items()})

    def _conv(self, x, conv, prelu, relu=False):
        w = self.p[f"{conv}/weight"]
        y = F.conv2d(x, w, self.p[f"{conv}/bias"], padding=w.shape[-1] // 2)
        if prelu:
            return F.prelu(y, self.p[f"{prelu}/weight"])
        return F.relu(y) if relu else y

    @torch.no_grad()
    def forward(self, x):
        c = self.cfg
        for name in pose.VGG:
            x = self._conv(x, name, pose.VGG_PRELU.get(name), relu=True)
            if name in pose.POOL_AFTER:
                x = F.max_pool2d(x, 2, 2)
        have = {"features": x}
        stages = []
        for branch, n, kind in (("L2", c["n_paf"], "paf"), ("L1", c["n_heat"], "heat")):
            for s in range(n):
                y = torch.cat([have[k] for k in pose.STAGE_INPUTS[branch, s == 0]], dim=1)
                for b in range(1, 6):
                    outs = []
                    for j in range(3):
                        y = self._conv(y, f"Mconv{b}_stage{s}_{branch}_{j}", f"Mprelu{b}_stage{s}_{branch}_{j}")
                        outs.append(y)
                    y = torch.cat(outs, dim=1)
                y = self._conv(y, f"Mconv6_stage{s}_{branch}", f"Mprelu6_stage{s}_{branch}")
                y = self._conv(y, f"Mconv7_stage{s}_{branch}", None)
                have[kind] = y
                stages.append(y)
        return have["features"], stages


# ---- peaks ----
def _cubic_table():
    a = f32(-0.75)
    tab = np.zeros((8, 4), f32)
    for ph in range(8):
        t = f32(2 * ph + 1) / f32(16)
        t1, u = t + f32(1), f32(1) - t
        w0 = ((a * t1 - f32(5) * a) * t1 + f32(8) * a) * t1 - f32(4) * a
        w1 = ((a + f32(2)) * t - (a + f32(3))) * t * t + f32(1)
        w2 = ((a + f32(2)) * u - (a + f32(3))) * u * u + f32(1)
        tab[ph] = (w0, w1, w2, f32(1) - w0 - w1 - w2)
    return tab


def upsample8(m):
    """m [h,w] float32 -> [8h,8w]: bicubic, a = -0.75, source (X + 0.5) / 8 - 0.5, clamped; the row's four products left to right,
    then the four rows"""
    m = np.asarray(m, f32)
    h, w = m.shape
    tab = _cubic_table()

    def axis(n, size):
        q = 2 * np.arange(n) - 7
        return q >> 4, tab[(q & 15) >> 1], size

    iy, wy, _ = axis(8 * h, h)
    ix, wx, _ = axis(8 * w, w)
    cols = [m[:, np.clip(ix - 1 + i, 0, w - 1)] for i in range(4)]                        # [h, 8w] each
    rowsum = ((wx[:, 0] * cols[0] + wx[:, 1] * cols[1]) + wx[:, 2] * cols[2]) + wx[:, 3] * cols[3]
    r = [rowsum[np.clip(iy - 1 + j, 0, h - 1)] for j in range(4)]                          # [8h, 8w] each
    out = ((wy[:, 0:1] * r[0] + wy[:, 1:2] * r[1]) + wy[:, 2:3] * r[2]) + wy[:, 3:4] * r[3]
    assert out.dtype == np.float32
    return out


def peak_pixels(U, threshold=0.05):
    """the (Y, X) of the strict 3 x 3 maxima above the threshold off the outermost ring, in raster order"""
    HH, WW = U.shape
    c = U[1:-1, 1:-1]
    is_peak = c > f32(threshold)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                is_peak &= c > U[1 + dy:HH - 1 + dy, 1 + dx:WW - 1 + dx]
    return np.argwhere(is_peak) + 1


def peaks_ref(heat, threshold=0.05, max_peaks=32, fill=0.0):
    """heat [h,w,P] -> (peaks [P,max_peaks,3] with `fill` where nothing is written, counts [P])"""
    heat = np.asarray(heat, f32)
    h, w, P = heat.shape
    peaks = np.full((P, max_peaks, 3), fill, f32)
    counts = np.zeros((P,), np.int32)
    for p in range(P - 1):
        U = upsample8(heat[:, :, p])
        HH, WW = U.shape
        found = peak_pixels(U, threshold)
        counts[p] = len(found)
        for i, (Y, X) in enumerate(found[:max_peaks]):
            sx = sy = sw = f32(0)
            for yy in range(max(Y - 3, 0), min(Y + 3, HH - 1) + 1):
                for xx in range(max(X - 3, 0), min(X + 3, WW - 1) + 1):
                    s = U[yy, xx]
                    if s > 0:
                        sx = sx + f32(xx) * s
                        sy = sy + f32(yy) * s
                        sw = sw + s
            peaks[p, i] = (sx / sw + f32(0.5), sy / sw + f32(0.5), U[Y, X])
    return peaks, counts


def peaks_ref_batch(heat, threshold=0.05, max_peaks=32, fill=0.0):
    out = [peaks_ref(m, threshold, max_peaks, fill) for m in heat]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- assembly ----
def _score(a, b, paf, cx, cy, inter_threshold, min_above):
    """the connection a -> b: its score, or None"""
    h, w, _ = paf.shape
    dx, dy = b[0] - a[0], b[1] - a[1]
    n = np.sqrt(dx * dx + dy * dy)
    if not n >= f32(1e-6):
        return None
    m = min(max(5, int(np.floor(np.sqrt(f32(5) * n) + f32(0.5)))), 25)
    ux, uy, den = dx / n, dy / n, f32(max(m - 1, 1))
    total, k = f32(0), 0
    for i in range(m):
        t = f32(i) / den
        sx, sy = a[0] + dx * t, a[1] + dy * t
        ix = int(min(max(np.floor(sx * f32(0.125)), f32(0)), f32(w - 1)))
        iy = int(min(max(np.floor(sy * f32(0.125)), f32(0)), f32(h - 1)))
        s = paf[iy, ix, cx] * ux + paf[iy, ix, cy] * uy
        if s > inter_threshold:
            total = total + s
            k += 1
    if k > 0 and f32(k) / f32(m) > min_above:
        return total / f32(k)
    return None


def assemble_ref(peaks, counts, paf, inter_threshold=0.05, min_above=0.95, min_parts=3, min_score=0.4, max_people=8):
    """one frame: peaks [26,max_peaks,3], counts [26], paf [h,w,52] -> (people [max_people,25,3], n_people)"""
    peaks, paf = np.asarray(peaks, f32), np.asarray(paf, f32)
    max_peaks = peaks.shape[1]
    inter_threshold, min_above, min_score = f32(inter_threshold), f32(min_above), f32(min_score)
    n_of = [min(max(int(c), 0), max_peaks) for c in counts]
    persons = []                                                   # dict(part={part: peak}, score, alive)
    for (pa, pb), (cx, cy) in zip(pose.PAIRS, pose.PAF_CHANNELS):
        cand = []
        for ia in range(n_of[pa]):
            for ib in range(n_of[pb]):
                s = _score(peaks[pa, ia], peaks[pb, ib], paf, cx, cy, inter_threshold, min_above)
                if s is not None:
                    cand.append((s, ia, ib))
        cand.sort(key=lambda c: (-float(c[0]), c[1], c[2]))        # (float32 -> float is exact: the order is the float32 order)
        used_a, used_b, conns = set(), set(), []
        for s, ia, ib in cand:
            if ia not in used_a and ib not in used_b:
                used_a.add(ia); used_b.add(ib); conns.append((s, ia, ib))
        for cs, ia, ib in conns:
            sa, sb = peaks[pa, ia, 2], peaks[pb, ib, 2]
            alive = [q for q in persons if q["alive"]]
            i = next((q for q in alive if q["part"].get(pa) == ia), None)
            j = next((q for q in alive if q["part"].get(pb) == ib), None)
            if i is not None and j is not None:
                if i is j or set(i["part"]) & set(j["part"]):
                    continue
                i["part"].update(j["part"])
                i["score"] = (i["score"] + j["score"]) + cs
                j["alive"] = False
            elif i is not None:
                if pb not in i["part"]:
                    i["part"][pb] = ib
                    i["score"] = i["score"] + (sb + cs)
            elif j is not None:
                if pa not in j["part"]:
                    j["part"][pa] = ia
                    j["score"] = j["score"] + (sa + cs)
            else:
                persons.append(dict(part={pa: ia, pb: ib}, score=(sa + sb) + cs, alive=True))
    people = np.zeros((max_people, pose.N_PARTS, 3), f32)
    n = 0
    for q in persons:
        npart = len(q["part"])
        if not q["alive"] or npart < min_parts or q["score"] / f32(npart) < min_score:
            continue
        if n < max_people:
            for part, i in q["part"].items():
                people[n, part] = peaks[part, i]
        n += 1
    return people, n


def assemble_ref_batch(peaks, counts, paf, **kw):
    out = [assemble_ref(p, c, f, **kw) for p, c, f in zip(peaks, counts, paf)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.int32)


def scale_ref(people, image_hw, net_hw):
    out = np.array(people, f32, copy=True)
    out[..., 0] = out[..., 0] * f32(image_hw[1]) / f32(net_hw[1])
    out[..., 1] = out[..., 1] * f32(image_hw[0]) / f32(net_hw[0])
    return out


# ---- constructed scenes ----
# a standing person, net-input pixels relative to its centre
TEMPLATE = {0: (0, -60), 1: (0, -40), 2: (-20, -40), 3: (-28, -12), 4: (-30, 14), 5: (20, -40), 6: (28, -12), 7: (30, 14), 8: (0, 10),
            9: (-12, 10), 10: (-14, 42), 11: (-14, 74), 12: (12, 10), 13: (14, 42), 14: (14, 74), 15: (-5, -65), 16: (5, -65), 17: (-10, -62),
            18: (10, -62), 19: (20, 82), 20: (24, 80), 21: (12, 80), 22: (-20, 82), 23: (-24, 80), 24: (-12, 80)}


def person(cx, cy, parts=TEMPLATE):
    return {p: (cx + dx, cy + dy) for p, (dx, dy) in parts.items()}


def scene(h, w, persons, sigma=1.1, radius=0.9, margin=12.0):
    """heat [h,w,26] and paf [h,w,52] of persons (dicts part -> (x, y) in net-input pixels): a Gaussian blob (sigma in cells) per
    part that lies at least `margin` pixels inside the image, a unit vector along every limb in the cells whose centre lies within
    `radius` cells of it.  -> (heat, paf, the persons cut to their visible parts).  A net pixel x is the cell coordinate x / 8 - 0.5."""
    heat = np.zeros((h, w, pose.N_HEAT), np.float64)
    paf = np.zeros((h, w, pose.N_PAF), np.float64)
    gy, gx = np.mgrid[0:h, 0:w].astype(np.float64)
    seen = []
    for who in persons:
        vis = {p: xy for p, xy in who.items() if margin <= xy[0] <= 8 * w - margin and margin <= xy[1] <= 8 * h - margin}
        seen.append(vis)
        for p, (x, y) in vis.items():
            heat[:, :, p] = np.maximum(heat[:, :, p], np.exp(-((gx - (x / 8 - 0.5)) ** 2 + (gy - (y / 8 - 0.5)) ** 2) / (2 * sigma ** 2)))
        for (pa, pb), (cx, cy) in zip(pose.PAIRS, pose.PAF_CHANNELS):
            if pa not in vis or pb not in vis:
                continue
            a = np.array(vis[pa]) / 8 - 0.5
            d = np.array(vis[pb]) / 8 - 0.5 - a
            n = np.linalg.norm(d)
            t = np.clip(((gx - a[0]) * d[0] + (gy - a[1]) * d[1]) / (n * n), 0, 1)
            near = np.hypot(gx - (a[0] + t * d[0]), gy - (a[1] + t * d[1])) <= radius
            paf[:, :, cx][near] = d[0] / n
            paf[:, :, cy][near] = d[1] / n
    heat[:, :, -1] = 1 - heat[:, :, :-1].max(axis=2)
    return heat.astype(f32), paf.astype(f32), seen
