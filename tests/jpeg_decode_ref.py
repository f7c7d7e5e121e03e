"""NumPy restatement of the baseline JPEG decoder of csrc/jpeg_decode.hip and csrc/jpeg_entropy.h, and of the bicubic
resize of csrc/image_resize.hip: libjpeg's and Pillow's integer rules, one after the other.

``decode(data, H=None, W=None, C=None)`` -> ``Result``: the status (``SOAR_JPEG_*``), the pixels uint8 ``[H,W,C]`` (zeros for a failed
file), the number of restart intervals the file was decoded in, and a checksum of the coefficients (what tests/tools/jpeg_entropy_host.cpp
prints).  ``resize_bicubic(image, h, w)`` is ``Image.resize((w, h), Image.BICUBIC)`` for 8-bit images.  The entropy decoder is a plain
Python loop; everything behind it is vectorised integer arithmetic.
"""
import math
from dataclasses import dataclass

import numpy as np

from jpeg_ref import AC_CHR, AC_LUM, DC_CHR, DC_LUM, ZIGZAG

OK, BAD_STRUCTURE, UNSUPPORTED, MISSING_TABLE, CORRUPT, TRUNCATED = range(6)


@dataclass
class Result:
    status: int
    image: np.ndarray = None
    intervals: int = 0
    checksum: int = 0
    coef: np.ndarray = None
    header: object = None


class Header:
    pass


# ---- the Huffman tables ---------------------------------------------------------------------------------------------------------------
class Huff:
    """Annex C's canonical code as (first code, first index, count) per length; ``ok`` is False for counts that are no prefix code"""

    def __init__(self, bits, vals):
        self.bits, self.vals = list(bits), list(vals)
        self.first, self.index = [0] * 17, [0] * 17
        code = k = 0
        self.ok = True
        for length in range(1, 17):
            self.first[length], self.index[length] = code, k
            code += bits[length - 1]
            k += bits[length - 1]
            if code > (1 << length):
                self.ok = False
            code <<= 1

    def decode(self, br):
        """-> the symbol, or -1 where the next 16 bits begin no code"""
        v = br.peek16()
        for length in range(1, 17):
            d = (v >> (16 - length)) - self.first[length]
            if 0 <= d < self.bits[length - 1]:
                br.drop(length)
                return self.vals[self.index[length] + d]
        return -1


# ---- the marker walk ------------------------------------------------------------------------------------------------------------------
def parse(f, want=None):
    """-> (status, Header): SOI to the end of SOS.  ``want``: the (H, W, C) the file must have, or None."""
    f = bytes(f)
    L = len(f)
    h = Header()
    h.qt, h.dc, h.ac = [None] * 4, [None] * 4, [None] * 4
    h.ri, h.nc, any_dht = 0, 0, False
    if L < 2 or f[0] != 0xFF or f[1] != 0xD8:
        return BAD_STRUCTURE, h
    if L > 0x7FFFFFFF:
        return UNSUPPORTED, h
    pos = 2
    while True:
        if pos >= L or f[pos] != 0xFF:
            return BAD_STRUCTURE, h
        while pos + 1 < L and f[pos + 1] == 0xFF:                 # fill bytes
            pos += 1
        if pos + 1 >= L:
            return BAD_STRUCTURE, h
        m = f[pos + 1]
        pos += 2
        if m == 0x00 or m == 0x01 or 0xD0 <= m <= 0xD9:            # no segment may stand here without a length
            return BAD_STRUCTURE, h
        if pos + 2 > L:
            return BAD_STRUCTURE, h
        n = f[pos] << 8 | f[pos + 1]
        if n < 2 or pos + n > L:
            return BAD_STRUCTURE, h
        p, e = pos + 2, pos + n
        if m == 0xC0:
            if h.nc or n < 8:
                return BAD_STRUCTURE, h
            prec, hh, ww, nc = f[p], f[p + 1] << 8 | f[p + 2], f[p + 3] << 8 | f[p + 4], f[p + 5]
            if n != 8 + 3 * nc:
                return BAD_STRUCTURE, h
            if prec != 8:
                return UNSUPPORTED, h
            if hh == 0 or ww == 0:
                return BAD_STRUCTURE, h
            if nc not in (1, 3):
                return UNSUPPORTED, h
            h.ids, h.hs, h.vs, h.tq = [], [], [], []
            for c in range(nc):
                h.ids.append(f[p + 6 + 3 * c])
                h.hs.append(f[p + 7 + 3 * c] >> 4)
                h.vs.append(f[p + 7 + 3 * c] & 15)
                h.tq.append(f[p + 8 + 3 * c])
            if any(t > 3 for t in h.tq):
                return BAD_STRUCTURE, h
            if nc == 1:
                if (h.hs[0], h.vs[0]) != (1, 1):
                    return UNSUPPORTED, h
            elif (h.hs[1], h.vs[1], h.hs[2], h.vs[2]) != (1, 1, 1, 1) or (h.hs[0], h.vs[0]) not in ((1, 1), (2, 1), (2, 2)):
                return UNSUPPORTED, h
            if want is not None and (hh, ww, nc) != tuple(want):
                return UNSUPPORTED, h
            h.H, h.W, h.nc = hh, ww, nc
        elif 0xC1 <= m <= 0xCF and m != 0xC4:
            return UNSUPPORTED, h
        elif m in (0xDC, 0xDE, 0xDF):                              # DNL, DHP, EXP
            return UNSUPPORTED, h
        elif m == 0xDB:
            while p < e:
                pq, tq = f[p] >> 4, f[p] & 15
                if pq > 1 or tq > 3:
                    return BAD_STRUCTURE, h
                if pq == 1:
                    return UNSUPPORTED, h
                if p + 65 > e:
                    return BAD_STRUCTURE, h
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = np.frombuffer(f[p + 1:p + 65], np.uint8)
                h.qt[tq] = q
                p += 65
        elif m == 0xC4:
            while p < e:
                tc, th = f[p] >> 4, f[p] & 15
                if tc > 1 or th > 3 or p + 17 > e:
                    return BAD_STRUCTURE, h
                bits = list(f[p + 1:p + 17])
                cnt = sum(bits)
                if cnt > 256 or p + 17 + cnt > e:
                    return BAD_STRUCTURE, h
                t = Huff(bits, f[p + 17:p + 17 + cnt])
                if not t.ok:
                    return BAD_STRUCTURE, h
                (h.ac if tc else h.dc)[th] = t
                any_dht = True
                p += 17 + cnt
        elif m == 0xDD:
            if n != 4:
                return BAD_STRUCTURE, h
            h.ri = f[p] << 8 | f[p + 1]
        elif m == 0xDA:
            if not h.nc or n < 3:
                return BAD_STRUCTURE, h
            ns = f[p]
            if n != 6 + 2 * ns:
                return BAD_STRUCTURE, h
            if ns != h.nc:
                return UNSUPPORTED, h
            h.td, h.ta = [], []
            for c in range(ns):
                if f[p + 1 + 2 * c] != h.ids[c]:
                    return UNSUPPORTED, h
                h.td.append(f[p + 2 + 2 * c] >> 4)
                h.ta.append(f[p + 2 + 2 * c] & 15)
            if any(t > 3 for t in h.td + h.ta):
                return BAD_STRUCTURE, h
            if (f[p + 1 + 2 * ns], f[p + 2 + 2 * ns], f[p + 3 + 2 * ns]) != (0, 63, 0):
                return UNSUPPORTED, h
            if not any_dht:                                        # an MJPG chunk: Annex K's tables
                h.dc[0], h.dc[1], h.ac[0], h.ac[1] = Huff(*DC_LUM), Huff(*DC_CHR), Huff(*AC_LUM), Huff(*AC_CHR)
            for c in range(ns):
                if h.qt[h.tq[c]] is None or h.dc[h.td[c]] is None or h.ac[h.ta[c]] is None:
                    return MISSING_TABLE, h
            h.scan = e
            break
        pos = e
    geometry(h)
    return OK, h


def geometry(h):
    hmax, vmax = h.hs[0], h.vs[0]
    h.hmax, h.vmax = hmax, vmax
    h.mcu_cols, h.mcu_rows = -(-h.W // (8 * hmax)), -(-h.H // (8 * vmax))
    h.mcus = h.mcu_cols * h.mcu_rows
    h.bw = [h.mcu_cols * s for s in h.hs]
    h.bh = [h.mcu_rows * s for s in h.vs]
    h.off, at = [], 0
    for c in range(h.nc):
        h.off.append(at)
        at += h.bw[c] * h.bh[c]
    h.blocks = at


def find_markers(f, a):
    """positions p >= a with f[p] = FF and f[p+1] neither 00 nor FF"""
    d = np.frombuffer(f, np.uint8)[a:]
    if d.size < 2:
        return np.zeros(0, np.int64)
    return a + np.nonzero((d[:-1] == 0xFF) & (d[1:] != 0) & (d[1:] != 0xFF))[0]


# ---- the entropy-coded segment ----------------------------------------------------------------------------------------------------------
class Bits:
    """f[pos, end) from the most significant bit, FF 00 unstuffed.  Behind the end, or an FF that no 00 follows, the bits are zeros;
    ``past_end`` says that one of those was taken."""

    def __init__(self, f, pos, end):
        self.f, self.pos, self.end = f, pos, end
        self.acc = self.cnt = self.fake = 0

    def fill(self):
        while self.cnt <= 24:
            b = 0
            if self.pos < self.end:
                b = self.f[self.pos]
                self.pos += 1
                if b == 0xFF:
                    if self.pos < self.end and self.f[self.pos] == 0:
                        self.pos += 1
                    else:
                        self.pos, b = self.end, 0
                        self.fake += 8
            else:
                self.fake += 8
            self.acc = (self.acc << 8 | b) & 0xFFFFFFFF
            self.cnt += 8

    def peek16(self):
        self.fill()
        return (self.acc >> (self.cnt - 16)) & 0xFFFF

    def drop(self, n):
        self.cnt -= n

    def take(self, n):
        if n == 0:
            return 0
        v = self.peek16() >> (16 - n)
        self.cnt -= n
        return v

    @property
    def past_end(self):
        return self.fake > self.cnt


def decode_block(br, dc, ac, pred, out):
    """one block into out[64] (natural order, int64 holding int16 values) -> (status, the new DC predictor as a uint32)"""
    s = dc.decode(br)
    if s < 0 or s > 15:
        return CORRUPT, pred
    diff = 0
    if s:
        v = br.take(s)
        diff = v if v >= (1 << (s - 1)) else v - ((1 << s) - 1)
    pred = (pred + diff) & 0xFFFFFFFF
    out[0] = ((pred & 0xFFFF) ^ 0x8000) - 0x8000
    k = 1
    while k < 64:
        rs = ac.decode(br)
        if rs < 0:
            return CORRUPT, pred
        r, s = rs >> 4, rs & 15
        if s:
            k += r
            if k > 63:
                return CORRUPT, pred
            v = br.take(s)
            out[ZIGZAG[k]] = v if v >= (1 << (s - 1)) else v - ((1 << s) - 1)
            k += 1
        elif r == 15:
            k += 16
            if k > 64:
                return CORRUPT, pred
        else:
            break
    return OK, pred


def decode_interval(f, h, coef, start, end, mcu0, n_mcus, last_open):
    """the MCUs [mcu0, mcu0 + n_mcus) from f[start, end) -> status"""
    br = Bits(f, start, end)
    pred = [0] * h.nc
    for m in range(mcu0, mcu0 + n_mcus):
        my, mx = divmod(m, h.mcu_cols)
        for c in range(h.nc):
            for v in range(h.vs[c]):
                for u in range(h.hs[c]):
                    blk = h.off[c] + (my * h.vs[c] + v) * h.bw[c] + mx * h.hs[c] + u
                    st, pred[c] = decode_block(br, h.dc[h.td[c]], h.ac[h.ta[c]], pred[c], coef[blk])
                    if br.past_end:
                        return TRUNCATED if last_open else CORRUPT
                    if st != OK:
                        return st
    return OK


def checksum_of(coef):
    c = coef.reshape(-1).astype(np.int64) & 0xFFFF
    i = np.arange(c.size, dtype=np.int64)
    return int(((c * ((i * 31 + 7) & 0xFFFF)) & 0xFFFFFFFF).sum() & 0xFFFFFFFF)


# ---- reconstruction -----------------------------------------------------------------------------------------------------------------------
def _idct_1d(d, shift):
    """jidctint's pass over the last axis of d [...,8] (int64); the result descaled by ``shift``"""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * 4433
    t2 = z1 + z3 * -15137
    t3 = z1 + z2 * 6270
    t0 = (d[..., 0] + d[..., 4]) << 13
    t1 = (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return (np.stack(out, axis=-1) + (1 << (shift - 1))) >> shift


def planes_of(h, coef):
    """-> per component the uint8 sample plane [8 bh, 8 bw]"""
    out = []
    for c in range(h.nc):
        n = h.bw[c] * h.bh[c]
        d = coef[h.off[c]:h.off[c] + n].astype(np.int64) * h.qt[h.tq[c]][None, :]
        d = d.reshape(n, 8, 8)
        d = _idct_1d(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)     # columns
        d = _idct_1d(d, 18)                                        # rows
        d = np.clip(d + 128, 0, 255)
        out.append(d.reshape(h.bh[c], h.bw[c], 8, 8).transpose(0, 2, 1, 3).reshape(8 * h.bh[c], 8 * h.bw[c]))
    return out


def upsample(plane, H, W, hs, vs):
    """a chroma plane's true part [ceil(H / vs), ceil(W / hs)] -> [H, W]: libjpeg's triangle filters, or plain replication where the
    downsampled width is 2 or less (jdsample.c chooses so)"""
    ch, cw = -(-H // vs), -(-W // hs)
    p = plane[:ch, :cw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)[:H, :W]
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    if vs == 1:
        out = np.empty((ch, 2 * cw), np.int64)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        return out[:H, :W]
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    down = np.concatenate([p[1:], p[-1:]], axis=0)
    rows = np.empty((2 * ch, cw), np.int64)
    rows[0::2] = 3 * p + up
    rows[1::2] = 3 * p + down
    left = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * rows + left + 8) >> 4
    out[:, 1::2] = (3 * rows + right + 7) >> 4
    return out[:H, :W]


def rgb_of(y, cb, cr):
    cb, cr = cb - 128, cr - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels_of(h, coef):
    planes = planes_of(h, coef)
    y = planes[0][:h.H, :h.W].astype(np.int64)
    if h.nc == 1:
        return y.astype(np.uint8)[..., None]
    return rgb_of(y, upsample(planes[1], h.H, h.W, h.hmax, h.vmax), upsample(planes[2], h.H, h.W, h.hmax, h.vmax))


# ---- a file ---------------------------------------------------------------------------------------------------------------------------
def decode(data, H=None, W=None, C=None):
    f = bytes(data)
    want = None if H is None else (H, W, C)
    st, h = parse(f, want)

    def failed(status, intervals=0):
        shape = want if want is not None else ((h.H, h.W, h.nc) if getattr(h, "nc", 0) and hasattr(h, "H") else (0, 0, 0))
        return Result(status, np.zeros(shape, np.uint8), intervals, 0, None, h)

    if st != OK:
        return failed(st)
    marks = find_markers(f, h.scan)
    codes = np.array([f[p + 1] for p in marks], np.int64)
    other = np.nonzero((codes < 0xD0) | (codes > 0xD7))[0]
    has_end = other.size > 0
    seg_end = int(marks[other[0]]) if has_end else len(f)
    k = int(other[0]) if has_end else len(marks)
    n_int = -(-h.mcus // h.ri) if h.ri else 1
    if k != n_int - 1:
        return failed(TRUNCATED if (k < n_int - 1 and not has_end) else CORRUPT)
    if any(int(codes[j]) != 0xD0 + (j & 7) for j in range(k)):
        return failed(CORRUPT)
    coef = np.zeros((h.blocks, 64), np.int64)
    status = OK
    for j in range(n_int):
        start = h.scan if j == 0 else int(marks[j - 1]) + 2
        end = int(marks[j]) if j < k else seg_end
        per = h.ri if h.ri else h.mcus
        st = decode_interval(f, h, coef, start, end, j * per, min(per, h.mcus - j * per), j == n_int - 1 and not has_end)
        if st != OK and (status == OK or st < status):
            status = st
    if status != OK:
        return failed(status, n_int)
    return Result(OK, pixels_of(h, coef), n_int, checksum_of(coef), coef, h)


# ---- Pillow's bicubic resize for 8-bit images ---------------------------------------------------------------------------------------------
PRECISION_BITS = 32 - 8 - 2


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_coeffs(in_size, out_size):
    """Resample.c's precompute_coeffs and normalize_coeffs_8bpc over the whole axis -> (bounds int32 [out,2]: first sample and count,
    coefficients int32 [out,ksize], ksize)"""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        k = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _pass(img, out_size, axis):
    bounds, kk, _ = resize_coeffs(img.shape[axis], out_size)
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((out_size,) + src.shape[1:], np.int64)
    for xx in range(out_size):
        x0, n = bounds[xx]
        k = kk[xx, :n].astype(np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        out[xx] = (1 << (PRECISION_BITS - 1)) + (src[x0:x0 + n] * k).sum(axis=0)
    return np.moveaxis(np.clip(out >> PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def resize_bicubic(image, h, w):
    """uint8 [H,W] or [H,W,C] -> [h,w(,C)]: the horizontal pass into 8 bits, then the vertical one"""
    return _pass(_pass(np.asarray(image), w, 1), h, 0)
