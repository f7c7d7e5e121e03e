"""NumPy and pure-Python restatement of the PNG encoder of csrc/png.hip: every rule, one after the other, giving the
exact bytes the kernels must give.

``png_file(image, filters, piece_bytes)`` -> the file; ``encode(...)`` -> ``(file, stats)`` with the filtered stream, the rows' filter
types and, per piece, whether it was stored, its code lengths (None where a piece is too short for any code to win) and its payload.
Everything is integer arithmetic.

The rules:
* filter per row: None, Sub, Up, Average, Paeth of the PNG specification on the raw row above; the one with the smallest sum of
  |residual as int8|, ties to the lowest type; or one type forced for every row.
* the filtered stream (H rows of 1 + W C bytes) is cut into pieces of ``piece_bytes``; nothing in a piece refers to another.
* tokens: maximal runs of equal bytes inside a piece, from the left.  The run's first byte is a literal; of the ``rest`` bytes behind
  it, while ``rest >= 3`` a match of ``min(rest, 258)`` at distance 1; what is left (1 or 2) are literals.
* code lengths over the 286 literal/length symbols (the end-of-block symbol counted once): with T the number of tokens + 1,
  ``f = 1 + T // 32000``, every used count raised to at least f, T' their sum, a symbol's length is the smallest l with
  ``count << l >= T'`` (a Shannon length; never above 15, never below 1); then sweeps over the lengths L = 2 .. 15 shorten, at every L,
  the first ``min(symbols of length L, D >> (15 - L))`` symbols in symbol order by one bit, D being what the Kraft sum lacks to
  2^15; sweeps repeat until D is 0.  Canonical codes as RFC 1951 assigns them.
* a dynamic block: BFINAL 0, BTYPE 2, HLIT 29, HDIST 0, HCLEN 15; the code-length alphabet has 4 bits for 0 .. 15 and none for
  16 .. 18, so every one of the 286 + 1 lengths is sent as its own 4 bits (no run-length coding of the header); one distance code of
  one bit.  Behind the end-of-block symbol an empty stored block (000, padding, 00 00 FF FF) aligns the piece.
* a piece whose dynamic block with that marker is not smaller than ``5 + n`` bytes is one stored block instead.
* framing: signature, IHDR, one IDAT per piece (the first begins with 78 01), an IDAT with the final empty fixed block 03 00 and the
  Adler-32 of the filtered stream combined from the pieces' values, IEND.
"""
import struct
import zlib

import numpy as np

DEFAULT_PIECE_BYTES = 65535
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + 287 * 4
SMALLEST_DYNAMIC = (HEADER_BITS + 2 + 3 + 7) // 8 + 4             # a header, two codes of a bit, the aligning block: 158 bytes
REV4 = tuple(int(format(v, "04b")[::-1], 2) for v in range(16))
CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# RFC 1951, 3.2.5: length symbol 257 + i: (extra bits, first length)
LENGTH_TABLE = ((0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 9), (0, 10), (1, 11), (1, 13), (1, 15), (1, 17), (2, 19), (2, 23),
                (2, 27), (2, 31), (3, 35), (3, 43), (3, 51), (3, 59), (4, 67), (4, 83), (4, 99), (4, 115), (5, 131), (5, 163), (5, 195),
                (5, 227), (0, 258))


def length_symbol(n):
    """a match length 3 .. 258 -> (symbol, extra bits, their value)"""
    if n == 258:
        return 285, 0, 0
    for i in range(27, -1, -1):
        eb, first = LENGTH_TABLE[i]
        if n >= first:
            return 257 + i, eb, n - first
    raise ValueError(n)


def png_bound(H, W, C, piece_bytes=DEFAULT_PIECE_BYTES):
    """every piece stored"""
    S = H * (1 + W * C)
    pieces = (S + piece_bytes - 1) // piece_bytes
    return 8 + 25 + 2 + pieces * (12 + 5) + S + 18 + 12


def filter_rows(img, filters="adaptive"):
    """uint8 [H,W,C] -> (the filtered stream, the rows' types)"""
    h, w, c = img.shape
    raw = img.reshape(h, w * c).astype(np.int32)
    out, types = bytearray(), []
    prev = np.zeros(w * c, np.int32)
    zero = np.zeros(c, np.int32)
    for y in range(h):
        r = raw[y]
        a = np.concatenate([zero, r[:-c]])
        b = prev
        cc = np.concatenate([zero, prev[:-c]])
        p = a + b - cc
        pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - cc)
        paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, cc))
        cands = [((x) & 255).astype(np.uint8) for x in (r, r - a, r - b, r - ((a + b) >> 1), r - paeth)]
        if filters == "adaptive":
            cost = [int(np.abs(x.view(np.int8).astype(np.int32)).sum()) for x in cands]
            k = cost.index(min(cost))                             # the first of the smallest: ties to the lowest type
        else:
            k = int(filters)
        types.append(k)
        out += bytes([k]) + cands[k].tobytes()
        prev = r
    return bytes(out), types


def tokens(piece):
    """bytes -> [(symbol, extra bits, their value)]: literals (symbol < 256) and matches at distance 1 (symbol >= 257)"""
    d = np.frombuffer(piece, np.uint8)
    n = len(d)
    starts = np.flatnonzero(np.concatenate([[True], d[1:] != d[:-1]]))
    ends = np.concatenate([starts[1:], [n]])
    out = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        v, N = int(d[s]), e - s
        lit = (v, 0, 0)
        if N < 4:
            out += [lit] * N
            continue
        out.append(lit)
        rest = N - 1
        while rest >= 3:
            m = min(rest, 258)
            out.append(length_symbol(m))
            rest -= m
        out += [lit] * rest
    return out


def code_lengths(counts):
    """[286] counts (the end-of-block symbol's among them) -> [286] lengths of a complete prefix code, 0 for an unused symbol"""
    counts = [int(x) for x in counts]
    used = [s for s in range(286) if counts[s] > 0]
    assert len(used) >= 2
    T = sum(counts)
    f = 1 + T // 32000
    raised = {s: max(counts[s], f) for s in used}
    T2 = sum(raised.values())
    L = [0] * 286
    for s in used:
        l = 1
        while (raised[s] << l) < T2:
            l += 1
        L[s] = l
    assert max(L) <= 15
    D = 32768 - sum(1 << (15 - L[s]) for s in used)
    assert D >= 0
    while D > 0:
        for length in range(2, 16):
            u = 1 << (15 - length)
            at = [s for s in used if L[s] == length]
            k = min(len(at), D // u)
            for s in at[:k]:
                L[s] = length - 1
            D -= k * u
    return L


def canonical_codes(L):
    """RFC 1951, 3.2.2"""
    bl = [0] * 17
    for l in L:
        bl[l] += 1
    bl[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 16):
        code = (code + bl[bits - 1]) << 1
        nxt[bits] = code
    codes = [0] * len(L)
    for s, l in enumerate(L):
        if l:
            codes[s] = nxt[l]
            nxt[l] += 1
    return codes


class BitWriter:
    """deflate's order: bits fill a byte from its least significant end"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, n):
        """an integer field: least significant bit first"""
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: most significant bit first"""
        self.bits(int(format(code, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def deflate_piece(piece):
    """-> (payload, stored, lengths): the piece's deflate blocks, byte-aligned at both ends and not final"""
    n = len(piece)
    assert 1 <= n <= 65535
    if SMALLEST_DYNAMIC >= 5 + n:                                 # no code can win: stored, whatever the lengths would be
        return b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + piece, True, None
    toks = tokens(piece)
    counts = [0] * 286
    for s, _, _ in toks:
        counts[s] += 1
    counts[256] = 1
    L = code_lengths(counts)
    codes = canonical_codes(L)
    w = BitWriter()
    w.bits(0, 1)
    w.bits(2, 2)
    w.bits(29, 5)
    w.bits(0, 5)
    w.bits(15, 4)
    for s in CLEN_ORDER:
        w.bits(0 if s >= 16 else 4, 3)
    for l in L + [1]:                                             # the 286 lengths and the one distance code's
        w.bits(REV4[l], 4)                                        # (sixteen codes of 4 bits: the code of l is l, its first bit first)
    assert len(w.out) * 8 + w.n == HEADER_BITS
    for s, eb, ev in toks:
        w.code(codes[s], L[s])
        if s >= 257:
            w.bits(ev, eb)
            w.bits(0, 1)                                          # distance 1: the only distance code, one bit
    w.code(codes[256], L[256])
    assert len(w.out) * 8 + w.n >= HEADER_BITS + 2
    w.bits(0, 3)                                                  # an empty stored block, not final
    w.align()
    w.out += b"\x00\x00\xff\xff"
    stored = len(w.out) >= 5 + n
    if stored:
        return b"\x00" + struct.pack("<HH", n, n ^ 0xFFFF) + piece, True, L
    return bytes(w.out), False, L


def adler_combine(a1, a2, len2):
    M = 65521
    A1, B1, A2, B2 = a1 & 0xFFFF, a1 >> 16, a2 & 0xFFFF, a2 >> 16
    return (((B1 + B2 + (len2 % M) * (A1 + M - 1)) % M) << 16) | ((A1 + A2 + M - 1) % M)


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def encode(img, filters="adaptive", piece_bytes=DEFAULT_PIECE_BYTES):
    img = np.ascontiguousarray(img)
    if img.ndim == 2:
        img = img[..., None]
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] in COLOUR_TYPE and 32 <= piece_bytes <= 65535
    h, w, c = img.shape
    stream, types = filter_rows(img, filters)
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, COLOUR_TYPE[c], 0, 0, 0))
    adler, pieces = 1, []
    for o in range(0, len(stream), piece_bytes):
        p = stream[o:o + piece_bytes]
        payload, stored, L = deflate_piece(p)
        adler = adler_combine(adler, zlib.adler32(p), len(p))
        out += chunk(b"IDAT", (b"\x78\x01" if o == 0 else b"") + payload)
        pieces.append({"stored": stored, "lengths": L, "payload": payload, "bytes": len(p)})
    out += chunk(b"IDAT", b"\x03\x00" + struct.pack(">I", adler)) + chunk(b"IEND", b"")
    return out, {"stream": stream, "types": types, "pieces": pieces, "adler": adler}


def png_file(img, filters="adaptive", piece_bytes=DEFAULT_PIECE_BYTES):
    return encode(img, filters, piece_bytes)[0]
