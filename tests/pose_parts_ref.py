"""Plain torch / NumPy restatement of soar_amd/pose_parts.py, written from the definition in include/soar_hip.h:

* ``RefCpmNet``: the convolutional pose machine as torch's functional calls, at whatever dtype its state dict has (float64 is the
  yardstick, float32 the measure of what float32 costs).  A 7 x 7 layer sums kernel row by kernel row, top to bottom, as the seven
  launches of the device do; ``rowwise=False`` runs the same layers through one ``F.conv2d`` each.  It reads the layer names, the pool
  places and the concatenation order from ``soar_amd.pose_parts`` and nothing else.
* ``boxes_ref`` / ``crop_ref`` / ``keypoints_ref``: NumPy float32, operation by operation in the order the header states, so that the
  kernels' results can be compared bit for bit.
* ``make_state_dict``: seeded random weights of any configuration.
"""
import numpy as np
import torch
import torch.nn.functional as F

import pose_ref
from soar_amd import pose_parts as PP

f32 = np.float32
N_FRONT = len(PP.FRONT)


def make_cfg(n_maps, n_stages, front=(8, 8, 8, 16, 16), feat=8, w6=8, stage=8, stage_side=7):
    """the released design at small widths: front widths (conv1, conv2, conv3, conv4, conv5_1/5_2), 3 x 3 up to conv5_3_CPM, 1 x 1 in
    stage 1, five stage_side x stage_side and two 1 x 1 convolutions in every later stage"""
    c1, c2, c3, c4, c5 = front
    width = [c1, c1, c2, c2, c3, c3, c3, c3, c4, c4, c4, c4, c5, c5, feat, w6, n_maps]
    side = [3] * N_FRONT + [1, 1]
    for _ in range(n_stages - 1):
        width += [stage] * 6 + [n_maps]
        side += [stage_side] * 5 + [1, 1]
    return dict(n_stages=n_stages, n_maps=n_maps, width=width, side=side)


HAND = make_cfg(22, 3)
FACE = make_cfg(71, 2)
# the released shapes: VGG-19's front, 6 stages
SHIPPED_HAND = make_cfg(22, 6, front=(64, 128, 256, 512, 512), feat=128, w6=512, stage=128)
SHIPPED_FACE = make_cfg(71, 6, front=(64, 128, 256, 512, 512), feat=128, w6=512, stage=128)


def make_state_dict(cfg, seed=0, dtype=torch.float32):
    """He-scaled weights and small biases: activations stay of order one through every stage"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in PP.layer_keys(cfg):
        fan_in = shape[1] * shape[2] * shape[3]
        sd[f"{name}.weight"] = (torch.randn(shape, generator=g, dtype=torch.float64) * (2.0 / fan_in) ** 0.5).to(dtype)
        sd[f"{name}.bias"] = (torch.randn(shape[0], generator=g, dtype=torch.float64) * 0.1).to(dtype)
    return sd


class RefCpmNet(torch.nn.Module):
    """forward(x [M,3,S,S]) -> (features, [every stage's maps]) in NCHW"""

    def __init__(self, state_dict, rowwise=True):
        super().__init__()
        self.cfg = PP.read_config(state_dict)
        self.rowwise = rowwise
        self.p = torch.nn.ParameterDict({k.replace(".", "/"): torch.nn.Parameter(v.detach().clone(), requires_grad=False)
                                         for k, v in state_dict.items()})

    def _conv(self, x, name, relu):
        w, b = self.p[f"{name}/weight"], self.p[f"{name}/bias"]
        k = w.shape[-1]
        if k <= 3 or not self.rowwise:
            y = F.conv2d(x, w, b, padding=k // 2)
        else:
            # kernel row r reads the input dy = r - k // 2 rows down: the first carries the bias, the later ones add to it
            xp = F.pad(x, (0, 0, k // 2, k // 2))
            H = x.shape[2]
            y = F.conv2d(xp[:, :, 0:H], w[:, :, 0:1], b, padding=(0, k // 2))
            for r in range(1, k):
                y = F.conv2d(xp[:, :, r:r + H], w[:, :, r:r + 1], None, padding=(0, k // 2)) + y
        return F.relu(y) if relu else y

    @torch.no_grad()
    def forward(self, x):
        n = self.cfg["n_stages"]
        for name in PP.FRONT:
            x = self._conv(x, name, True)
            if name in PP.POOL_AFTER:
                x = F.max_pool2d(x, 2, 2)
        have = {"features": x}
        y = self._conv(self._conv(x, PP.STAGE_1[0], True), PP.STAGE_1[1], False)
        stages = [y]
        for s in range(2, n + 1):
            have["maps"] = y
            y = torch.cat([have[k] for k in PP.STAGE_INPUT], dim=1)
            for j in range(1, PP.N_MCONV + 1):
                y = self._conv(y, f"Mconv{j}_stage{s}", j < PP.N_MCONV)
            stages.append(y)
        return have["features"], stages


# ---- the rectangles ----
def _dist(a, b):
    dx, dy = a[0] - b[0], a[1] - b[1]
    return np.sqrt(dx * dx + dy * dy)


def hand_box(J, left, hand_min_conf=0.03, min_hand_area=10.0):
    """J [25,3] float32 -> (x0, y0, side, valid)"""
    sh, el, wr = (J[i] for i in PP.HAND_JOINTS["left" if left else "right"])
    t = f32(hand_min_conf)
    cx = wr[0] + f32(0.33) * (wr[0] - el[0])
    cy = wr[1] + f32(0.33) * (wr[1] - el[1])
    side = f32(1.5) * max(_dist(wr, el), f32(0.9) * _dist(el, sh))
    x0, y0 = cx - side / f32(2), cy - side / f32(2)
    valid = sh[2] > t and el[2] > t and wr[2] > t and side > f32(1) and side * side > f32(min_hand_area)
    return (x0, y0, side, f32(1)) if valid else (f32(0),) * 4


def face_box(J, face_min_conf=0.25, min_face_area=40.0):
    neck, nose, r_eye, l_eye, r_ear, l_ear = (J[PP.FACE_JOINTS[k]] for k in ("neck", "nose", "r_eye", "l_eye", "r_ear", "l_ear"))
    t = f32(face_min_conf)
    has = lambda p: bool(p[2] > t)
    cx = cy = size = f32(0)
    count = 0
    if has(neck) and has(nose):
        nn = _dist(neck, nose)
        if has(l_eye) == has(l_ear) and has(r_eye) == has(r_ear) and has(l_eye) != has(r_eye):
            eye, ear = (l_eye, l_ear) if has(l_eye) else (r_eye, r_ear)
            cx = cx + ((eye[0] + ear[0]) + nose[0]) / f32(3)
            cy = cy + ((eye[1] + ear[1]) + nose[1]) / f32(3)
            size = size + f32(0.85) * ((_dist(nose, eye) + _dist(nose, ear)) + nn)
        else:
            cx = cx + (neck[0] + nose[0]) / f32(2)
            cy = cy + (neck[1] + nose[1]) / f32(2)
            size = size + f32(2) * nn
        count += 1
    if has(l_eye) and has(r_eye):
        cx = cx + (l_eye[0] + r_eye[0]) / f32(2)
        cy = cy + (l_eye[1] + r_eye[1]) / f32(2)
        size = size + f32(3) * _dist(l_eye, r_eye)
        count += 1
    if has(l_ear) and has(r_ear):
        cx = cx + (l_ear[0] + r_ear[0]) / f32(2)
        cy = cy + (l_ear[1] + r_ear[1]) / f32(2)
        size = size + f32(2) * _dist(l_ear, r_ear)
        count += 1
    if count == 0:
        return (f32(0),) * 4
    cx, cy, size = cx / f32(count), cy / f32(count), size / f32(count)
    x0, y0 = cx - size / f32(2), cy - size / f32(2)
    return (x0, y0, size, f32(1)) if size * size > f32(min_face_area) else (f32(0),) * 4


def boxes_ref(people, n_people, part_people=1, hand_min_conf=0.03, min_hand_area=10.0, face_min_conf=0.25, min_face_area=40.0):
    """people [B,max_people,25,3], n_people [B] -> boxes [B,part_people,3,4]"""
    people = np.asarray(people, f32)
    B, max_people = people.shape[:2]
    out = np.zeros((B, part_people, 3, 4), f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            for q in range(min(part_people, max_people, max(int(n_people[b]), 0))):
                J = people[b, q]
                out[b, q, 0] = hand_box(J, True, hand_min_conf, min_hand_area)
                out[b, q, 1] = hand_box(J, False, hand_min_conf, min_hand_area)
                out[b, q, 2] = face_box(J, face_min_conf, min_face_area)
    return out


# ---- the crops ----
def crop_one(img, box, S, mirrored):
    """img [H,W,3] uint8 RGB, box (x0, y0, side, valid) -> [3,S,S] float32 BGR"""
    H, W, _ = img.shape
    out = np.zeros((3, S, S), f32)
    if box[3] != 0:
        s = f32(box[2]) / f32(S)
        u = np.arange(S)
        x = (f32(box[0]) + (S - 1 - u if mirrored else u).astype(f32) * s)[None, :]
        y = (f32(box[1]) + u.astype(f32) * s)[:, None]
        x, y = np.broadcast_to(x, (S, S)), np.broadcast_to(y, (S, S))
        assert x.dtype == np.float32 and y.dtype == np.float32
        with np.errstate(invalid="ignore"):
            inside = (x > f32(-1)) & (x < f32(W)) & (y > f32(-1)) & (y < f32(H))
        xs, ys = np.where(inside, x, f32(0)), np.where(inside, y, f32(0))
        fx, fy = np.floor(xs), np.floor(ys)
        ax, ay = xs - fx, ys - fy
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        bgr = img[:, :, ::-1].astype(f32)

        def px(yy, xx):
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            return np.where(ok[..., None], bgr[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], f32(0))

        p00, p01, p10, p11 = px(iy, ix), px(iy, ix + 1), px(iy + 1, ix), px(iy + 1, ix + 1)
        ax, ay = ax[..., None], ay[..., None]
        val = (p00 * (f32(1) - ax) + p01 * ax) * (f32(1) - ay) + (p10 * (f32(1) - ax) + p11 * ax) * ay
        val = np.where(inside[..., None], val, f32(0))
        assert val.dtype == np.float32
        out = np.ascontiguousarray(val.transpose(2, 0, 1))
    return out / f32(256) - f32(0.5)


def crop_ref(images, boxes, S):
    """images [B,H,W,3] uint8, boxes [B,P,3,4] -> (hands [B P 2,3,S,S], faces [B P,3,S,S])"""
    B, P = boxes.shape[:2]
    hands = np.stack([crop_one(images[b], boxes[b, q, k], S, k == 0) for b in range(B) for q in range(P) for k in range(2)]) \
        if B * P else np.zeros((0, 3, S, S), f32)
    faces = np.stack([crop_one(images[b], boxes[b, q, 2], S, False) for b in range(B) for q in range(P)]) if B * P else np.zeros((0, 3, S, S), f32)
    return hands, faces


# ---- the maxima ----
def keypoints_ref(heat, boxes, which):
    """heat [M,h,w,n_maps], boxes [B,P,3,4], which "hands" or "face" -> [M,n_maps-1,3]"""
    heat = np.asarray(heat, f32)
    M, h, w, n_maps = heat.shape
    flat = np.asarray(boxes, f32).reshape(-1, 3, 4)
    out = np.zeros((M, n_maps - 1, 3), f32)
    for m in range(M):
        hand = m % 2 if which == "hands" else 2
        box = flat[m // 2 if which == "hands" else m, hand]
        for p in range(n_maps - 1):
            U = pose_ref.upsample8(heat[m, :, :, p])
            with np.errstate(invalid="ignore"):
                U = np.where(np.isnan(U), -np.inf, U).astype(f32)
            at = int(np.argmax(U))                                         # (the first of equal maxima)
            Y, X = divmod(at, 8 * w)
            best = U[Y, X]
            if best > 0 and box[3] != 0:
                s = box[2] / f32(8 * w)
                out[m, p] = (box[0] + f32(8 * w - 1 - X if hand == 0 else X) * s, box[1] + f32(Y) * s, best)
    return out
