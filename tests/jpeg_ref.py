"""NumPy restatement of the baseline JPEG encoder of csrc/video.hip: libjpeg's integer rules, one after the other.

``encode(image, qtables, subsampling, restart_interval)`` -> ``(header, scan, stats)``: the header from SOI to the end of SOS, the
entropy-coded bytes with their restart markers (what lies between SOS and EOI), and counts of the corners the coder went through.
``jpeg_file`` is ``header + scan + EOI``.  Everything is integer arithmetic; the entropy coder is a plain Python loop.
"""
import numpy as np

# ---- literal data: Annex K's zigzag order and Huffman tables (bits[1..16], values) ---------------------------------------------------
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
DC_LUM = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHR = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUM = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHR = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def _codes(spec):
    """symbol -> (code, length): Annex C's canonical assignment"""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


# ---- the transform ------------------------------------------------------------------------------------------------------------------
def ycbcr(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    """replicate the last row and the last column up to [rows, cols]"""
    h, w = plane.shape
    return np.pad(plane, ((0, rows - h), (0, cols - w)), mode="edge")


def downsample_420(plane, mcus_y, mcus_x):
    """[H,W] -> [8 mcus_y, 8 mcus_x]: columns replicated to 16 mcus_x, rows to an even height, (a + b + c + d + bias) >> 2 with bias 1 in
    even and 2 in odd output columns, then the last downsampled row replicated down to the MCU grid"""
    h, _ = plane.shape
    p = _pad(plane, h + (h & 1), 16 * mcus_x)
    bias = np.tile(np.array([1, 2]), 4 * mcus_x)
    d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad(d, 8 * mcus_y, 8 * mcus_x)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_1d(d, first):
    """jfdctint's pass over the last axis of d [...,8] (int64); first: the row pass (outputs up by PASS1_BITS = 2)"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, n)
    out[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1)


def blocks_of(plane, qtable):
    """[8 by, 8 bx] samples -> [by, bx, 64] quantised coefficients in zigzag order"""
    by, bx = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(by, 8, bx, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    c = _dct_1d(b, True)                                          # rows
    c = _dct_1d(c.swapaxes(-1, -2), False).swapaxes(-1, -2)       # columns
    q = 8 * np.asarray(qtable, np.int64).reshape(8, 8)
    mag = (np.abs(c) + (q >> 1)) // q
    return (np.sign(c) * mag).reshape(by, bx, 64)[..., ZIGZAG]


def mcu_blocks(image, qtables, subsampling):
    """-> (coefficients [mcus, blocks per MCU, 64] in coding order, component of each block of an MCU, dummy flags [mcus, blocks per MCU])"""
    H, W = image.shape[:2]
    y, cb, cr = ycbcr(image)
    if subsampling == "444":
        my, mx = -(-H // 8), -(-W // 8)
        planes = [blocks_of(_pad(p, 8 * my, 8 * mx), qtables[min(i, 1)]) for i, p in enumerate((y, cb, cr))]
        coef = np.stack(planes, axis=2).reshape(my * mx, 3, 64)
        return coef, (0, 1, 2), np.zeros((my * mx, 3), bool)
    if subsampling != "420":
        raise ValueError(subsampling)
    my, mx = -(-H // 16), -(-W // 16)
    nby, nbx = -(-H // 8), -(-W // 8)                              # the real luma blocks
    lum = blocks_of(_pad(y, 16 * my, 16 * mx), qtables[0])          # (what lies in a dummy block is not used)
    cbq = blocks_of(downsample_420(cb, my, mx), qtables[1])
    crq = blocks_of(downsample_420(cr, my, mx), qtables[1])
    coef = np.zeros((my, mx, 6, 64), np.int64)
    dummy = np.zeros((my, mx, 6), bool)
    for k in range(4):
        coef[:, :, k] = lum[k >> 1::2, k & 1::2]
        dummy[:, :, k] = (2 * np.arange(my)[:, None] + (k >> 1) >= nby) | (2 * np.arange(mx)[None, :] + (k & 1) >= nbx)
    coef[:, :, 4], coef[:, :, 5] = cbq, crq
    for k in range(1, 4):                                           # a dummy block: no AC, the DC of the block coded before it
        prev = coef[:, :, k - 1, 0].copy()
        coef[:, :, k][dummy[:, :, k]] = 0
        coef[:, :, k, 0] = np.where(dummy[:, :, k], prev, coef[:, :, k, 0])
    return coef.reshape(my * mx, 6, 64), (0, 0, 0, 0, 1, 2), dummy.reshape(my * mx, 6)


# ---- the entropy coder --------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.stuffed = bytearray(), 0, 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _category(v):
    return int(abs(int(v))).bit_length()


def entropy_code(coef, comps, restart_interval):
    """-> (scan bytes, stats)"""
    dc_tab = [_codes(DC_LUM), _codes(DC_CHR)]
    ac_tab = [_codes(AC_LUM), _codes(AC_CHR)]
    bits = _Bits()
    stats = {"zrl": 0, "dc_category": 0, "ac_category": 0, "restarts": 0}
    pred = [0, 0, 0]
    for m in range(coef.shape[0]):
        if m and m % restart_interval == 0:
            bits.pad()
            bits.out += bytes([0xFF, 0xD0 + ((m // restart_interval - 1) & 7)])
            stats["restarts"] += 1
            pred = [0, 0, 0]
        for k, comp in enumerate(comps):
            blk, t = coef[m, k], min(comp, 1)
            diff = int(blk[0]) - pred[comp]
            pred[comp] = int(blk[0])
            n = _category(diff)
            stats["dc_category"] = max(stats["dc_category"], n)
            bits.put(*dc_tab[t][n])
            if n:
                bits.put((diff if diff > 0 else diff + (1 << n) - 1), n)
            run = 0
            for z in range(1, 64):
                v = int(blk[z])
                if v == 0:
                    run += 1
                    continue
                while run > 15:
                    bits.put(*ac_tab[t][0xF0])
                    stats["zrl"] += 1
                    run -= 16
                n = _category(v)
                stats["ac_category"] = max(stats["ac_category"], n)
                bits.put(*ac_tab[t][(run << 4) | n])
                bits.put((v if v > 0 else v + (1 << n) - 1), n)
                run = 0
            if run:
                bits.put(*ac_tab[t][0x00])
    bits.pad()
    stats["stuffed"] = bits.stuffed
    return bytes(bits.out), stats


# ---- the header ---------------------------------------------------------------------------------------------------------------------
def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def header(H, W, qtables, subsampling, restart_interval):
    out = bytes([0xFF, 0xD8]) + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in np.asarray(qtables[i]).reshape(64)[ZIGZAG]))
    s = 0x22 if subsampling == "420" else 0x11
    out += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, s, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc, (bits, vals) in ((0x00, DC_LUM), (0x10, AC_LUM), (0x01, DC_CHR), (0x11, AC_CHR)):
        out += _segment(0xC4, bytes([tc]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(image, qtables, subsampling="444", restart_interval=1):
    """image uint8 [H,W,3] or [H,W,4] (the fourth channel is ignored), qtables [2,64] in natural order -> (header, scan, stats)"""
    image = np.asarray(image)[..., :3]
    H, W = image.shape[:2]
    coef, comps, dummy = mcu_blocks(image, qtables, subsampling)
    scan, stats = entropy_code(coef, comps, int(restart_interval))
    stats["dummy_blocks"] = int(dummy.sum())
    stats["mcus"] = coef.shape[0]
    return header(H, W, qtables, subsampling, int(restart_interval)), scan, stats


def jpeg_file(image, qtables, subsampling="444", restart_interval=1):
    head, scan, _ = encode(image, qtables, subsampling, restart_interval)
    return head + scan + b"\xff\xd9"
