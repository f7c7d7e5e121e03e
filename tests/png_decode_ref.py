"""Plain-Python restatement of the PNG decoder of csrc/png_decode.hip: the chunk walk, inflate (RFC 1951), the segment
rule, Adler-32 and the row filters, with the decoder's statuses and in its order of checks; and a small PNG writer on zlib.

``decode(data, want=None)`` -> ``Result``: status, image (uint8 [H,W,C]; zeros on failure), segments and a report of what the file
exercises -- block types, the longest code, the code-length symbols, the largest length and distance, whether a copy overlapped its
source, the rows' filters, the IDATs, and whether an IDAT boundary fell inside a Huffman code or a stored block's header.

The order of checks, which decides the status of a file with several faults:
* the walk, chunk by chunk: signature; a chunk that does not fit the file (1); IHDR first, 13 bytes (1), its CRC (3), zero sizes (1),
  depth / colour type / methods / interlace (2), another shape than the call's (2); a second IHDR (1); an IDAT's CRC (3); an unknown
  critical chunk other than PLTE (2); IEND ends the walk; no IDAT (1).  CRCs of other chunks are not looked at.
* the zlib header (2 for another method, window or FDICT; 4 for its check bits), then the blocks.  Bits beyond the end read as zeros
  and "the input ended" (4) is noticed at the next check.  In a block: a literal that does not fit the output is 5; a match is
  checked for reaching before the output's start (4) first and for fitting (5) second.  Behind the final block fewer than four
  bytes are 4, more are 5; then fewer than H (1 + W C) bytes of output are 5.
* Adler-32 (6); a filter byte above 4 (7).
Segments: see ``segment_starts`` and ``decode``; ``segments`` counts the segments that gave at least one byte, so the encoder's last
IDAT (an empty final block and the Adler bytes) is a segment that is not counted.
"""
import bisect
import struct
import zlib

import numpy as np

import png_ref as P

OK, BAD_STRUCTURE, UNSUPPORTED, BAD_CRC, CORRUPT, WRONG_LENGTH, BAD_ADLER, BAD_FILTER = range(8)
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 6: 4}
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class Stop(Exception):
    def __init__(self, status):
        self.status = status


class Report:
    def __init__(self):
        self.block_types, self.stored_blocks, self.longest_code = set(), 0, 0
        self.clen_symbols, self.max_length, self.max_distance, self.overlap = set(), 0, 0, False
        self.filters, self.idats, self.idat_sizes, self.boundary_in_code, self.boundary_in_stored_header = set(), 0, [], False, False
        self.chunks = []


class Result:
    def __init__(self):
        self.status, self.image, self.segments, self.shape, self.report, self.stream = OK, None, 1, None, Report(), b""


def png_info(data):
    if len(data) < 26 or data[:8] != SIGNATURE or data[12:16] != b"IHDR":
        raise ValueError("not a PNG header")
    w, h, depth, colour = struct.unpack(">IIBB", data[16:26])
    if depth != 8 or colour not in CHANNELS:
        raise ValueError("unsupported")
    return h, w, CHANNELS[colour]


def walk(data, want, rep):
    """-> (status, (H, W, C), z, the IDAT payloads' starts in z)"""
    L = len(data)
    if L < 8 or data[:8] != SIGNATURE:
        return BAD_STRUCTURE, None, b"", []
    pos, first, shape, z, starts = 8, True, None, bytearray(), []
    while True:
        if pos + 12 > L:
            return BAD_STRUCTURE, shape, b"", []
        n, kind = struct.unpack(">I", data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        if n > 0x7FFFFFFF or pos + 12 + n > L:
            return BAD_STRUCTURE, shape, b"", []
        body = data[pos + 8:pos + 8 + n]
        crc_ok = zlib.crc32(kind + body) == struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]
        rep.chunks.append(kind)
        if first:
            if kind != b"IHDR" or n != 13:
                return BAD_STRUCTURE, shape, b"", []
            if not crc_ok:
                return BAD_CRC, shape, b"", []
            w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", body)
            if w == 0 or h == 0 or w > 0x7FFFFFFF or h > 0x7FFFFFFF:
                return BAD_STRUCTURE, shape, b"", []
            if depth != 8 or colour not in CHANNELS or comp or filt or lace:
                return UNSUPPORTED, shape, b"", []
            shape = (h, w, CHANNELS[colour])
            if want is not None and tuple(want) != shape:
                return UNSUPPORTED, shape, b"", []
            first = False
        elif kind == b"IHDR":
            return BAD_STRUCTURE, shape, b"", []
        elif kind == b"IDAT":
            if not crc_ok:
                return BAD_CRC, shape, b"", []
            starts.append(len(z))
            rep.idats += 1
            rep.idat_sizes.append(n)
            z += body
        elif kind == b"IEND":
            break
        elif not (kind[0] & 0x20) and kind != b"PLTE":
            return UNSUPPORTED, shape, b"", []
        pos += 12 + n
    if not starts:
        return BAD_STRUCTURE, shape, b"", []
    return OK, shape, bytes(z), starts


def whole_stored_block(z, a, b):
    """z[a, b), an IDAT's payload (behind the zlib header if it begins the stream), is exactly one stored block that is not final"""
    a = 2 if a == 0 else a
    return b - a >= 5 and z[a] == 0 and (z[a + 1] ^ z[a + 3]) == 0xFF and (z[a + 2] ^ z[a + 4]) == 0xFF and b - a == 5 + z[a + 1] + 256 * z[a + 2]


def segment_starts(z, idat_starts):
    """Byte 2, and every later start p of an IDAT payload that has a byte of its own and in front of which the stream provably may
    be at a block boundary: the four bytes before p are 00 00 FF FF (an empty stored block: what a flush, and png.hip behind a coded
    piece, write), or the IDAT before it is exactly one stored block (png.hip's stored pieces)."""
    out, ends = [2], idat_starts[1:] + [len(z)]
    for k in range(1, len(idat_starts)):
        p = idat_starts[k]
        if 6 <= p < len(z) and p > out[-1] and (z[p - 4:p] == b"\x00\x00\xff\xff" or whole_stored_block(z, idat_starts[k - 1], ends[k - 1])):
            out.append(p)
    return out


class Code:
    """a canonical code: None if over-subscribed; ``left`` what it lacks to be complete"""

    def __init__(self, lens):
        self.count = [0] * 16
        for l in lens:
            self.count[l] += 1
        left = 1
        for l in range(1, 16):
            left = (left << 1) - self.count[l]
            if left < 0:
                break
        self.left = left
        self.maxlen = max([l for l in range(1, 16) if self.count[l]], default=0)
        if left < 0:
            return
        nxt, code = [0] * 16, 0
        for l in range(1, 16):
            code = (code + (self.count[l - 1] if l > 1 else 0)) << 1
            nxt[l] = code
        self.table = [None] * (1 << 15)                          # 15 bits of the stream -> (symbol, length)
        for s, l in enumerate(lens):
            if l:
                r = int(format(nxt[l], f"0{l}b")[::-1], 2)
                nxt[l] += 1
                self.table[r::1 << l] = [(s, l)] * (1 << (15 - l))


class Inflater:
    """z[.., n) from byte ``at`` into ``out`` (None: count only), at most ``cap`` bytes"""

    def __init__(self, z, n, at, cap, out, rep, bounds):
        self.z, self.n, self.bit, self.cap, self.out, self.pos, self.rep = z, n, 8 * at, cap, out, 0, rep
        self.pad = bytes(z[:n]) + bytes(64)
        self.bounds = bounds                                     # sorted bit positions of the IDAT boundaries

    def peek(self, k):
        p = min(self.bit, 8 * self.n + 256)
        return (int.from_bytes(self.pad[p >> 3:(p >> 3) + 5], "little") >> (p & 7)) & ((1 << k) - 1)

    def take(self, k):
        v = self.peek(k)
        self.bit += k
        return v

    def past(self):
        return self.bit > 8 * self.n

    def crosses(self, a, b):
        i = bisect.bisect_right(self.bounds, a) if self.bounds else 0
        return bool(self.bounds) and i < len(self.bounds) and self.bounds[i] < b

    def sym(self, code):
        e = code.table[self.peek(15)] if code.left >= 0 and code.maxlen else None
        if e is None:
            return -1
        if self.rep is not None:
            if e[1] > self.rep.longest_code:
                self.rep.longest_code = e[1]
            if self.bounds and self.crosses(self.bit, self.bit + e[1]):
                self.rep.boundary_in_code = True
        self.bit += e[1]
        return e[0]

    def put(self, data):
        if self.out is not None:
            self.out[self.pos:self.pos + len(data)] = data
        self.pos += len(data)

    def dynamic(self):
        nlen, ndist, ncode = self.take(5) + 257, self.take(5) + 1, self.take(4) + 4
        if nlen > 286 or ndist > 30:
            raise Stop(CORRUPT)
        cl = [0] * 19
        for i in range(ncode):
            cl[P.CLEN_ORDER[i]] = self.take(3)
        clc = Code(cl)
        if clc.left != 0:
            raise Stop(CORRUPT)
        lens, prev = [], 0
        while len(lens) < nlen + ndist:
            s = self.sym(clc)
            if s < 0 or self.past():
                raise Stop(CORRUPT)
            if s < 16:
                prev = s
                lens.append(s)
                continue
            if self.rep is not None:
                self.rep.clen_symbols.add(s)
            if s == 16:
                if not lens:
                    raise Stop(CORRUPT)
                v, rep = prev, 3 + self.take(2)
            elif s == 17:
                v, rep = 0, 3 + self.take(3)
            else:
                v, rep = 0, 11 + self.take(7)
            if len(lens) + rep > nlen + ndist:
                raise Stop(CORRUPT)
            lens += [v] * rep
            prev = v
        if self.past() or lens[256] == 0:
            raise Stop(CORRUPT)
        lit, dist = Code(lens[:nlen] + [0] * (288 - nlen)), Code(lens[nlen:] + [0] * (32 - ndist))
        if lit.left != 0:
            raise Stop(CORRUPT)
        if dist.left != 0 and dist.left != 1 << 15 and not (dist.left == 1 << 14 and dist.count[1] == 1):
            raise Stop(CORRUPT)
        return lit, dist

    def run(self, last):
        try:
            return self._run(last)
        except Stop as s:
            return s.status

    def _run(self, last):
        rep = self.rep
        while True:
            final, kind = self.take(1), self.take(2)
            if self.past() or kind == 3:
                return CORRUPT
            if rep is not None:
                rep.block_types.add(kind)
            if kind == 0:
                head = self.bit
                self.bit = (self.bit + 7) & ~7
                n, nn = self.take(16), self.take(16)
                if self.past() or (n ^ nn) != 0xFFFF:
                    return CORRUPT
                if rep is not None:
                    rep.stored_blocks += 1
                    if self.crosses(head - 3, self.bit):
                        rep.boundary_in_stored_header = True
                start = self.bit >> 3
                if start + n > self.n:
                    return CORRUPT
                if self.pos + n > self.cap:
                    return WRONG_LENGTH
                self.put(self.z[start:start + n])
                self.bit = 8 * (start + n)
            else:
                lit, dist = (Code(FIXED_LIT), Code(FIXED_DIST)) if kind == 1 else self.dynamic()
                while True:
                    s = self.sym(lit)
                    if s < 0 or self.past():
                        return CORRUPT
                    if s < 256:
                        if self.pos >= self.cap:
                            return WRONG_LENGTH
                        self.put(bytes([s]))
                        continue
                    if s == 256:
                        break
                    if s > 285:
                        return CORRUPT
                    n = LEN_BASE[s - 257] + self.take(LEN_EXTRA[s - 257])
                    d = self.sym(dist)
                    if d < 0 or d > 29:
                        return CORRUPT
                    d = DIST_BASE[d] + self.take(DIST_EXTRA[d])
                    if self.past():
                        return CORRUPT
                    if d > self.pos:
                        return CORRUPT
                    if self.pos + n > self.cap:
                        return WRONG_LENGTH
                    if rep is not None:
                        rep.max_length, rep.max_distance = max(rep.max_length, n), max(rep.max_distance, d)
                        rep.overlap |= d < n
                    if self.out is not None:
                        for i in range(n):
                            self.out[self.pos + i] = self.out[self.pos + i - d]
                    self.pos += n
            if final:
                if not last:
                    return CORRUPT
                left = self.n - ((self.bit + 7) >> 3)
                return CORRUPT if left < 4 else (WRONG_LENGTH if left > 4 else OK)
            if not last and self.bit == 8 * self.n:
                return OK


def zlib_header(cmf, flg):
    if (cmf & 15) != 8 or (cmf >> 4) > 7:
        return UNSUPPORTED
    if (cmf * 256 + flg) % 31:
        return CORRUPT
    if flg & 32:
        return UNSUPPORTED
    return OK


def unfilter(stream, h, w, c, rep=None):
    """-> (status, uint8 [h,w,c]): the PNG specification's reconstruction, bytes beyond the image being 0"""
    stride = w * c
    out = np.zeros((h, stride), np.uint8)
    prev = bytearray(stride)
    for y in range(h):
        t, row = stream[y * (stride + 1)], bytearray(stream[y * (stride + 1) + 1:(y + 1) * (stride + 1)])
        if t > 4:
            return BAD_FILTER, np.zeros((h, w, c), np.uint8)
        if rep is not None:
            rep.filters.add(t)
        if t == 1:
            for x in range(c, stride):
                row[x] = (row[x] + row[x - c]) & 255
        elif t == 2:
            row = bytearray(((np.frombuffer(bytes(row), np.uint8).astype(np.int32) + np.frombuffer(bytes(prev), np.uint8)) & 255).astype(np.uint8).tobytes())
        elif t == 3:
            for x in range(stride):
                row[x] = (row[x] + (((row[x - c] if x >= c else 0) + prev[x]) >> 1)) & 255
        elif t == 4:
            for x in range(stride):
                a, b, cc = (row[x - c] if x >= c else 0), prev[x], (prev[x - c] if x >= c else 0)
                p = a + b - cc
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                row[x] = (row[x] + (a if pa <= pb and pa <= pc else (b if pb <= pc else cc))) & 255
        out[y] = np.frombuffer(bytes(row), np.uint8)
        prev = row
    return OK, out.reshape(h, w, c)


def decode(data, want=None, report=True):
    """``want``: the call's (H, W, C); None: the file's own"""
    r = Result()
    rep = r.report
    st, shape, z, idat_starts = walk(data, want, rep)
    r.shape = shape
    zero = np.zeros(want if want is not None else (shape or (0, 0, 0)), np.uint8)
    r.status, r.image = st, zero
    if st:
        return r
    h, w, c = shape
    S, n = h * (1 + w * c), len(z)
    if S > 0x7FFFFFFF:
        r.status = UNSUPPORTED
        return r
    if n < 2:
        r.status = CORRUPT
        return r
    r.status = zlib_header(z[0], z[1])
    if r.status:
        return r
    bounds = sorted(8 * p for p in idat_starts if 0 < p < n)
    starts = segment_starts(z, idat_starts)
    ends = starts[1:] + [n]
    parallel, lens = len(starts) > 1, []
    if parallel:
        for k, (a, b) in enumerate(zip(starts, ends)):           # the first pass: nothing is written
            inf = Inflater(z, b, a, S, None, None, None)
            if inf.run(k + 1 == len(starts)) != OK:
                parallel = False
            lens.append(inf.pos)
        parallel = parallel and sum(lens) == S
    out = bytearray(S)
    if parallel:
        r.segments, at = sum(1 for x in lens if x > 0), 0
        for k, (a, b) in enumerate(zip(starts, ends)):
            part = bytearray(lens[k])
            inf = Inflater(z, b, a, lens[k], part, rep if report else None, bounds)
            st = inf.run(k + 1 == len(starts))
            assert st == OK and inf.pos == lens[k]               # the first pass proved it
            out[at:at + lens[k]] = part
            at += lens[k]
    else:
        inf = Inflater(z, n, 2, S, out, rep if report else None, bounds)
        r.status = inf.run(True)
        if r.status == OK and inf.pos != S:
            r.status = WRONG_LENGTH
        if r.status:
            return r
    r.stream = bytes(out)
    if zlib.adler32(r.stream) != struct.unpack(">I", z[n - 4:])[0]:
        r.status = BAD_ADLER
        return r
    r.status, r.image = unfilter(r.stream, h, w, c, rep)
    return r


# ---- a writer on zlib -----------------------------------------------------------------------------------------------------------------
def chunk(kind, data, crc=None):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) if crc is None else crc)


def split(z, sizes):
    """z cut into pieces of ``sizes`` (an int: every piece that long; a list: those lengths in turn, 0 allowed, the rest in one)"""
    if isinstance(sizes, int):
        return [z[i:i + sizes] for i in range(0, len(z), sizes)] or [b""]
    out, at = [], 0
    for s in sizes:
        out.append(z[at:at + s])
        at += s
    if at < len(z):
        out.append(z[at:])
    return out


def make_png(image, filters="adaptive", level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, mem_level=8, idat_sizes=None, flush_at=(),
             flush_mode=zlib.Z_FULL_FLUSH, split_at_flushes=False, extra_chunks=(), stream=None):
    """A PNG file of ``image`` (uint8 [H,W,C] or [H,W]).  ``filters``: as png_ref.filter_rows, or a list with a type per row;
    ``level`` .. ``mem_level``: zlib.compressobj's; ``flush_at``: offsets of the filtered stream at which the compressor is flushed
    with ``flush_mode``; ``split_at_flushes``: an IDAT ends at every flush point (otherwise ``idat_sizes``, see ``split``);
    ``extra_chunks``: (kind, data, where) with where "before" the IDATs or an index: in front of that IDAT; ``stream``: these bytes
    in place of the filtered image."""
    img = np.ascontiguousarray(image)
    if img.ndim == 2:
        img = img[..., None]
    h, w, c = img.shape
    if stream is None:
        if isinstance(filters, (list, tuple)):
            stream = b"".join(P.filter_rows(img[:y + 1], t)[0][y * (1 + w * c):] for y, t in enumerate(filters))
        else:
            stream = P.filter_rows(img, filters)[0]
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    parts, at, cur = [], 0, b""
    for f in list(flush_at) + [len(stream)]:
        cur += co.compress(stream[at:f])
        at = f
        if f < len(stream):
            cur += co.flush(flush_mode)
            if split_at_flushes:
                parts.append(cur)
                cur = b""
    cur += co.flush()
    parts.append(cur)
    pieces = parts if split_at_flushes else split(b"".join(parts), idat_sizes if idat_sizes is not None else 1 << 30)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, P.COLOUR_TYPE[c], 0, 0, 0))
    for kind, data, where in extra_chunks:
        if where == "before":
            out += chunk(kind, data)
    for i, p in enumerate(pieces):
        for kind, data, where in extra_chunks:
            if where == i:
                out += chunk(kind, data)
        out += chunk(b"IDAT", p)
    return out + chunk(b"IEND", b"")


def chunks_of(png):
    """[(offset, kind, data)] of a well-formed file"""
    out, pos = [], 8
    while pos < len(png):
        n = struct.unpack(">I", png[pos:pos + 4])[0]
        out.append((pos, png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]))
        pos += 12 + n
    return out


def rebuild(png, edit):
    """the file with every chunk passed through ``edit(index, kind, data) -> [(kind, data)]``, CRCs made anew"""
    out = SIGNATURE
    for i, (_, kind, data) in enumerate(chunks_of(png)):
        for k, d in edit(i, kind, data):
            out += chunk(k, d)
    return out


def with_zlib_stream(png, z):
    """the file with its IDATs replaced by one that holds ``z``"""
    done = []

    def edit(i, kind, data):
        if kind != b"IDAT":
            return [(kind, data)]
        if done:
            return []
        done.append(1)
        return [(kind, z)]
    return rebuild(png, edit)


def zlib_stream_of(png):
    return b"".join(d for _, k, d in chunks_of(png) if k == b"IDAT")
