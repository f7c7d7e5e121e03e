"""Procedural inputs of the normal-prior tests: a torus, a capsule, hand-written triangles, and the awkward faces every visibility
case carries.  No model file, no golden file."""
import numpy as np


def torus(nu, nv, R=0.5, r=0.2):
    """nu x nv vertices, 2 nu nv faces, outward orientation."""
    u, v = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    verts = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return verts.astype(np.float32), np.array(faces, np.int64)


def capsule(n_around=14, n_cap=4, n_body=5, radius=0.25, half=0.45):
    """A closed capsule along y: two poles, 2 n_cap + n_body - 1 rings of n_around vertices."""
    rings = []
    for k in range(1, n_cap + 1):                                        # upper cap, from the pole down
        t = 0.5 * np.pi * k / n_cap
        rings.append((half + radius * np.cos(t), radius * np.sin(t)))
    for k in range(1, n_body):
        rings.append((half - 2 * half * k / n_body, radius))
    for k in range(n_cap, 0, -1):
        t = 0.5 * np.pi * k / n_cap
        rings.append((-half - radius * np.cos(t), radius * np.sin(t)))
    ang = np.arange(n_around) * 2 * np.pi / n_around
    verts = [(0.0, half + radius, 0.0)] + [(rr * np.cos(a), y, rr * np.sin(a)) for y, rr in rings for a in ang] + [(0.0, -half - radius, 0.0)]
    at = lambda ring, j: 1 + ring * n_around + j % n_around
    last = len(verts) - 1
    faces = [(0, at(0, j + 1), at(0, j)) for j in range(n_around)]
    for ring in range(len(rings) - 1):
        for j in range(n_around):
            a, b, c, d = at(ring, j), at(ring, j + 1), at(ring + 1, j + 1), at(ring + 1, j)
            faces += [(a, b, c), (a, c, d)]
    faces += [(last, at(len(rings) - 1, j), at(len(rings) - 1, j + 1)) for j in range(n_around)]
    return np.array(verts, np.float32), np.array(faces, np.int64)


def camera(W, H, fill=0.8, dist=3.0, extent=0.75, tilt=(0.9, 0.4, 0.2), seed=0):
    """(K [3,3], w2c [4,4]) float32: a body of half-extent ``extent`` at ``dist`` fills ``fill`` of the smaller image side; the
    principal point sits off the centre by a fraction of a pixel."""
    f = fill * min(W, H) / 2 * dist / extent
    K = np.array([[f, 0, W / 2 + 0.3], [0, f * 1.07, H / 2 - 0.2], [0, 0, 1]], np.float32)
    ax, ay, az = tilt
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    w2c = np.eye(4)
    w2c[:3, :3] = rz @ ry @ rx
    w2c[:3, 3] = (0.03, -0.02, dist)
    return K, w2c.astype(np.float32)


def with_extras(verts, faces, K, w2c, W, H, quad=True, dist=3.0):
    """The body plus, as further vertices and faces: (quad) two triangles larger than the image behind the body; faces wholly and
    partly outside the image on all four sides (negative snapped coordinates among them); one face past the guard band of 2^20
    pixels; one with a vertex behind the camera; one degenerate (collinear) and one with a repeated vertex; and exact copies of
    every 7th body face and of one quad triangle (the copies come last: the lower index is the original).  The extra vertices are
    given in pixel coordinates and depth and taken back through the camera, so they land where they are meant to."""
    K64, M = K.astype(np.float64), w2c.astype(np.float64)
    Rt, t = M[:3, :3].T, M[:3, 3]

    def world(px, py, z):
        cam = np.array([(px - K64[0, 2]) / K64[0, 0] * z, (py - K64[1, 2]) / K64[1, 1] * z, z])
        return Rt @ (cam - t)

    V0, F0 = verts.shape[0], faces.shape[0]
    new_v, new_f = [], []

    def tri(points):
        base = V0 + len(new_v)
        new_v.extend(world(*p) for p in points)
        new_f.append((base, base + 1, base + 2))

    zf, zn = dist + 2.0, dist - 1.2
    if quad:
        base = V0 + len(new_v)
        new_v.extend(world(*p) for p in ((-0.6 * W, -0.7 * H, zf), (1.7 * W, -0.6 * H, zf * 1.1), (1.6 * W, 1.8 * H, zf), (-0.5 * W, 1.7 * H, zf * 1.2)))
        new_f += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    tri([(-40.0, 3.0, zn), (-25.5, 9.0, zn), (-30.0, 20.0, zn)])                         # wholly left of the image
    tri([(W + 12.0, 4.0, zn), (W + 30.0, 6.0, zn), (W + 20.0, 25.0, zn)])                # wholly right
    tri([(5.0, -33.0, zn), (16.0, -20.25, zn), (9.0, -7.0, zn)])                         # wholly above
    tri([(8.0, H + 6.0, zn), (20.0, H + 9.0, zn), (12.0, H + 31.0, zn)])                 # wholly below
    tri([(-9.25, 0.3 * H, zn), (4.6, 0.3 * H - 3, zn), (3.1, 0.3 * H + 6, zn)])          # across the left border
    tri([(W - 4.4, 0.6 * H, zn), (W + 7.5, 0.6 * H + 2, zn), (W - 2.0, 0.6 * H + 7, zn)])  # across the right border
    tri([(0.4 * W, -6.5, zn), (0.4 * W + 8, 3.7, zn), (0.4 * W - 3, 4.2, zn)])           # across the top
    tri([(0.7 * W, H - 3.3, zn), (0.7 * W + 6, H + 8.0, zn), (0.7 * W - 5, H + 2.0, zn)])  # across the bottom
    tri([(-5.5, -4.5, zn), (6.0, -2.0, zn), (-1.0, 7.0, zn)])                            # across the corner (0, 0)
    tri([(float(1 << 22), 5.0, zn), (10.0, 5.0, zn), (10.0, 12.0, zn)])                  # a vertex past the guard band
    tri([(0.5 * W, 0.5 * H, -0.5), (0.5 * W + 9, 0.5 * H, zn), (0.5 * W, 0.5 * H + 9, zn)])   # a vertex behind the camera
    tri([(10.0, 10.0, zn), (14.0, 14.0, zn), (18.0, 18.0, zn)])                          # collinear: zero area
    base = V0 + len(new_v)
    new_v.append(world(0.5 * W, 0.4 * H, zn))
    new_v.append(world(0.5 * W + 6, 0.4 * H + 5, zn))
    new_f.append((base, base + 1, base + 1))                                             # a repeated vertex
    copies = [tuple(int(x) for x in faces[f]) for f in range(0, F0, 7)]
    if quad:
        copies.append(new_f[1])
    all_v = np.concatenate([verts.astype(np.float64), np.array(new_v)], 0).astype(np.float32)
    all_f = np.concatenate([faces, np.array(new_f, np.int64), np.array(copies, np.int64)], 0)
    return all_v, all_f, dict(first_copy=F0 + len(new_f), copies_of=list(range(0, F0, 7)) + ([F0 + 1] if quad else []))


# name -> (mesh, (W, H)): the visibility cases.  33 x 47: one partial tile; 96 x 80: 2 x 2 tiles of 32 ... 3 x 3; 48 x 40 with 2304
# mostly sub-pixel faces in one or two tiles: more hits than a slab or the queue holds; the capsule at 130 x 70
CASES = {
    "torus16x10_33x47": (lambda: torus(16, 10), (33, 47)),
    "torus24x12_96x80": (lambda: torus(24, 12), (96, 80)),
    "torus48x24_48x40": (lambda: torus(48, 24), (48, 40)),
    "capsule_130x70": (lambda: capsule(), (130, 70)),
}


def make_case(name, quad=True):
    mesh, (W, H) = CASES[name]
    v, f = mesh()
    K, w2c = camera(W, H)
    v, f, info = with_extras(v, f, K, w2c, W, H, quad=quad)
    return dict(verts=v, faces=f, K=K, w2c=w2c, W=W, H=H, **info)
