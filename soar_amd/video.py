"""MJPEG video output: baseline JPEG frames encoded on the device (csrc/video.hip), wrapped in a plain AVI file on the host.

SOAR ends with a video (the reference writes ``video.mp4`` with imageio from render_rot.py, ``save_img_sequence`` and
``SMPLify.visualize_params``).  The finished uint8 frames are on the device already; here they are compressed there, so only
compressed bytes cross to the host, and the result is one file every player opens -- no video library is involved.

* ``jpeg_tables(quality)``: libjpeg's quality scaling of the Annex K tables, on the host.
* ``encode_jpeg(frames, ...)`` -> ``(data, offsets)`` on the device: complete JPEG files, one after the other.
* ``save_jpeg(path, image, ...)``: a still image.
* ``MjpegWriter``: a context manager; ``write(frames)`` encodes a chunk and appends it to the AVI file.
* ``read_mjpeg_avi(path)``: the frames' JPEG bytes back, from the file's index, on the host.
* ``MjpegReader(path)``: ``height``, ``width``, ``fps``, ``frames`` from the headers; ``read(start, stop, step, device)`` yields decoded
  chunks on the device (``soar_amd.jpeg.decode_jpeg``); ``read_video(path, device)`` is the whole file.

The plumbing around the kernels that PNG needs as well (guards, measure and emit, statuses, bytes to the host) is in ``codec_io.py``.

The encoder's rules are libjpeg's, exact in integers (include/soar_hip.h and DESIGN.md 9r state them): with the same tables,
subsampling and restart interval the entropy-coded bytes are those libjpeg-turbo (Pillow) writes.  HIP only: CPU tensors are refused,
there is no CPU fallback.  Out of scope: H.264 / MP4, progressive or optimised-Huffman JPEG, 4:2:2, audio, OpenDML AVI (files of
4 GB and more).
"""
from __future__ import annotations

import ctypes
import struct
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import codec_io, hip_lib

# Annex K's example tables, natural (row-major) order
_BASE_LUM = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_BASE_CHR = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

SUBSAMPLINGS = {"444": 444, "420": 420}
# The encoder gives every restart interval a wavefront of its own, and its transform works on tiles of 64 pixels across: 8 MCUs at
# 4:4:4, 4 at 4:2:0, 24 blocks either way.  That tile is the default interval (about 2.5 bytes of marker and padding per 24 blocks).
DEFAULT_RESTART_INTERVAL = {"444": 8, "420": 4}
AVI_MAX_BYTES = 2 ** 32 - 1
_AVI_HEADER_BYTES = 224               # RIFF .. the 'movi' list's type; the first frame chunk starts here
_MOVI_FOURCC_AT = 220


def jpeg_tables(quality: int) -> np.ndarray:
    """The luminance and the chrominance quantisation table for ``quality`` (1 .. 100): uint8 ``[2,64]`` in natural order.  libjpeg's
    ``jpeg_quality_scaling``: scale = 5000 / quality below 50 and 200 - 2 quality from 50 up (integer division), every entry
    ``(base * scale + 50) / 100`` clamped to 1 .. 255."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"jpeg_tables: quality must be 1 .. 100 (got {quality})")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_BASE_LUM, _BASE_CHR], np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint8)


def _encode(frames, quality, subsampling, restart_interval, out):
    codec_io.need_hip_tensor("frames", frames, "video")
    if frames.dim() != 4 or frames.dtype != torch.uint8 or frames.shape[3] not in (3, 4):
        raise ValueError(f"encode_jpeg: frames must be uint8 [B,H,W,3] or [B,H,W,4] (got {frames.dtype} {tuple(frames.shape)})")
    if subsampling not in SUBSAMPLINGS:
        raise ValueError(f"encode_jpeg: subsampling must be '444' or '420' (got {subsampling!r})")
    ri = DEFAULT_RESTART_INTERVAL[subsampling] if restart_interval is None else int(restart_interval)
    if not 1 <= ri <= 65535:
        raise ValueError(f"encode_jpeg: restart_interval must be 1 .. 65535 MCUs (got {restart_interval})")
    a = hip_lib.SoarJpegArgs()
    a.B, a.H, a.W, a.channels, a.subsampling, a.restart_interval = *frames.shape, SUBSAMPLINGS[subsampling], ri
    frames, a.frames, a.frame_stride = codec_io.batch_view("encode_jpeg", frames)
    ctypes.memmove(a.qtables, jpeg_tables(quality).tobytes(), 128)
    return codec_io.measure_and_emit("encode_jpeg", a, ("soar_jpeg_workspace_bytes", "soar_jpeg_measure", "soar_jpeg_emit"), a.B, frames.device, out)


def encode_jpeg(frames: torch.Tensor, quality: int = 90, subsampling: str = "444", restart_interval: Optional[int] = None,
                out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``frames``: uint8 ``[B,H,W,3]`` or ``[B,H,W,4]`` on the device (a fourth channel is ignored; every frame contiguous, any step
    from frame to frame) -> ``(data, offsets)``, both on the device: ``data`` uint8, the B complete JPEG files (SOI .. EOI) one after
    the other, and ``offsets`` int64 ``[B+1]``: frame b is ``data[offsets[b]:offsets[b+1]]``.  ``subsampling``: ``"444"`` or ``"420"``;
    ``restart_interval``: MCUs between restart markers, 1 .. 65535 (default: ``DEFAULT_RESTART_INTERVAL``, one transform tile; every
    interval is one wavefront's serial work, so a large value is correct and slow).

    With ``out=None`` the sizes are measured on the device, the ``B + 1`` offsets are read back -- the call's one synchronisation --
    and ``data`` is allocated exactly.  With a caller's ``out`` (1-D uint8 on the device) nothing synchronises; ``data`` is ``out``.
    If it is too small NOTHING is written into it and ``offsets[-1] > out.numel()`` says so: overflow is reported, never written."""
    data, offsets, _ = _encode(frames, quality, subsampling, restart_interval, out)
    return data, offsets


def save_jpeg(path: str, image: torch.Tensor, quality: int = 90, subsampling: str = "444", restart_interval: Optional[int] = None) -> None:
    """``image``: uint8 ``[H,W,3]`` or ``[H,W,4]`` on the device -> a baseline JPEG file at ``path``."""
    if isinstance(image, torch.Tensor) and image.dim() != 3:
        raise ValueError(f"save_jpeg: image must be uint8 [H,W,3] or [H,W,4] (got {tuple(image.shape)})")
    data, _, offsets = _encode(image[None] if isinstance(image, torch.Tensor) else image, quality, subsampling, restart_interval, None)
    with open(path, "wb") as f:
        f.write(codec_io.host_items(data, offsets)[0][0])


# ---- the container ------------------------------------------------------------------------------------------------------------------
def _avi_header(width: int, height: int, rate: int, scale: int, frames: int, movi_bytes: int, idx_bytes: int, largest: int) -> bytes:
    """the first 224 bytes: RIFF, hdrl (avih, one strl with strh and strf), the 'movi' list's head.  movi_bytes: 'movi' and the chunks"""
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIHHHH", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, frames, largest, 0xFFFFFFFF, 0, 0, 0, width, height)
    avih = struct.pack("<IIIIIIIIII16x", (1000000 * scale + rate // 2) // rate, 0, 0, 0x10, frames, 0, 1, largest, width, height)
    strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
    riff = 4 + 8 + len(hdrl) + 8 + movi_bytes + idx_bytes
    head = b"RIFF" + struct.pack("<I", riff) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"
    assert len(head) == _AVI_HEADER_BYTES
    return head


class MjpegWriter:
    """A Motion-JPEG AVI file: ``RIFF``/``AVI `` with ``hdrl`` (``avih``, one ``strl``: ``strh`` ``vids``/``MJPG`` and ``strf``, a
    ``BITMAPINFOHEADER`` with ``biCompression`` ``MJPG``, 24 bit), ``movi`` with one ``00dc`` chunk per frame padded to even length, and
    ``idx1``.  ``write(frames)`` encodes uint8 ``[n,height,width,3 or 4]`` on the device (``encode_jpeg``), copies the compressed
    bytes -- and nothing else -- to the host and appends them; ``close()`` writes the index and the sizes.  A frame that would take the
    file past 2^32 - 1 bytes is refused (ValueError) before anything of it is written; the file stays valid and can be closed.

    ``fps``: an integer, or a float kept to 1/1000.  ``bytes_to_host``: what ``write`` has copied from the device so far."""

    def __init__(self, path: str, height: int, width: int, fps: float = 25, quality: int = 90, subsampling: str = "420",
                 restart_interval: Optional[int] = None):
        if not (1 <= int(height) <= 65535 and 1 <= int(width) <= 65535):
            raise ValueError(f"MjpegWriter: height and width must be 1 .. 65535 (got {height}, {width})")
        if not fps > 0:
            raise ValueError(f"MjpegWriter: fps must be positive (got {fps})")
        if subsampling not in SUBSAMPLINGS:
            raise ValueError(f"MjpegWriter: subsampling must be '444' or '420' (got {subsampling!r})")
        jpeg_tables(quality)
        self.path, self.height, self.width = path, int(height), int(width)
        self.rate, self.scale = (int(fps), 1) if float(fps) == int(fps) else (int(round(float(fps) * 1000)), 1000)
        self.quality, self.subsampling, self.restart_interval = int(quality), subsampling, restart_interval
        self.bytes_to_host = 0
        self._index: List[Tuple[int, int]] = []                  # (offset from the 'movi' fourcc, length) per frame
        self._pos = _AVI_HEADER_BYTES                            # bytes of the file so far
        self._largest = 0
        self._file = open(path, "wb")
        self._file.write(_avi_header(self.width, self.height, self.rate, self.scale, 0, 4, 0, 0))

    frames = property(lambda s: len(s._index))

    def __enter__(self) -> "MjpegWriter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def append_jpeg(self, jpeg: bytes) -> None:
        """one frame that is a JPEG file already (host bytes)"""
        if self._file is None:
            raise ValueError("MjpegWriter: the file is closed")
        n = len(jpeg)
        end = self._pos + 8 + n + (n & 1) + 8 + 16 * (len(self._index) + 1)      # with this frame and the index behind it
        if end > AVI_MAX_BYTES:
            raise ValueError(f"MjpegWriter: frame {len(self._index)} would take '{self.path}' to {end} bytes, past the {AVI_MAX_BYTES} "
                             "a plain AVI file can hold (OpenDML is not written)")
        self._file.write(b"00dc" + struct.pack("<I", n) + jpeg + (b"\x00" if n & 1 else b""))
        self._index.append((self._pos - _MOVI_FOURCC_AT, n))
        self._pos += 8 + n + (n & 1)
        self._largest = max(self._largest, n)

    def write(self, frames: torch.Tensor) -> None:
        """uint8 ``[n,height,width,3 or 4]`` (or one frame ``[height,width,3 or 4]``) on the device"""
        if isinstance(frames, torch.Tensor) and frames.dim() == 3:
            frames = frames[None]
        if isinstance(frames, torch.Tensor) and frames.dim() == 4 and tuple(frames.shape[1:3]) != (self.height, self.width):
            raise ValueError(f"MjpegWriter: frames of {self.height} x {self.width} expected (got {tuple(frames.shape)})")
        data, _, offsets = _encode(frames, self.quality, self.subsampling, self.restart_interval, None)
        jpegs, n = codec_io.host_items(data, offsets)
        self.bytes_to_host += n
        for blob in jpegs:
            self.append_jpeg(blob)

    def close(self) -> None:
        if self._file is None:
            return
        f, self._file = self._file, None
        idx = b"".join(b"00dc" + struct.pack("<III", 0x10, o, n) for o, n in self._index)
        f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        f.seek(0)
        f.write(_avi_header(self.width, self.height, self.rate, self.scale, len(self._index), self._pos - _MOVI_FOURCC_AT, 8 + len(idx),
                            self._largest))
        f.close()


def read_mjpeg_avi(path: str) -> List[bytes]:
    """The frames' JPEG bytes of an AVI file as ``MjpegWriter`` writes it, through its ``idx1`` index, on the host (for tests, and to
    get the frames back through any JPEG decoder)."""
    with open(path, "rb") as f:
        d = f.read()
    if len(d) < 12 or d[:4] != b"RIFF" or d[8:12] != b"AVI ":
        raise ValueError(f"read_mjpeg_avi: '{path}' is not a RIFF AVI file")
    movi = idx = None
    p = 12
    while p + 8 <= len(d):
        cc, n = d[p:p + 4], struct.unpack_from("<I", d, p + 4)[0]
        if cc == b"LIST" and d[p + 8:p + 12] == b"movi":
            movi = p + 8
        if cc == b"idx1":
            idx = (p + 8, n)
        p += 8 + n + (n & 1)
    if movi is None or idx is None:
        raise ValueError(f"read_mjpeg_avi: '{path}' has no 'movi' list or no 'idx1' index")
    out = []
    for e in range(idx[0], idx[0] + idx[1], 16):
        cc, _, off, n = struct.unpack_from("<4sIII", d, e)
        at = movi + off
        if cc != b"00dc" or d[at:at + 4] != b"00dc" or struct.unpack_from("<I", d, at + 4)[0] != n:
            raise ValueError(f"read_mjpeg_avi: index entry {len(out)} of '{path}' does not point at a '00dc' chunk of its length")
        out.append(d[at + 8:at + 8 + n])
    return out


class MjpegReader:
    """An MJPEG AVI file read back.  ``height``, ``width`` and ``fps`` come from the ``avih`` and ``strh`` headers,
    ``frames`` from the ``idx1`` index ``read_mjpeg_avi`` walks.  Index entries other than ``00dc`` (audio, a second stream) and
    zero-length entries (dropped frames) are skipped, so frame numbers count the pictures that are there.  The frames' bytes are
    uploaded as they are and decoded on the device (``soar_amd.jpeg``): baseline JPEG, grey or 4:4:4 / 4:2:2 / 4:2:0, with or without
    Huffman tables of their own.  OpenDML files (more than one RIFF chunk) are not read."""

    def __init__(self, path: str):
        from . import jpeg
        self.path = path
        with open(path, "rb") as f:
            d = f.read()
        if len(d) < 12 or d[:4] != b"RIFF" or d[8:12] != b"AVI ":
            raise ValueError(f"MjpegReader: '{path}' is not a RIFF AVI file")
        self._data = d
        movi = idx = avih = strh = None

        def walk(p, end):
            nonlocal movi, idx, avih, strh
            while p + 8 <= end:
                cc, n = d[p:p + 4], struct.unpack_from("<I", d, p + 4)[0]
                if cc == b"LIST" and d[p + 8:p + 12] == b"movi":
                    movi = p + 8
                elif cc == b"LIST" and d[p + 8:p + 12] in (b"hdrl", b"strl"):
                    walk(p + 12, min(end, p + 8 + n))
                elif cc == b"avih" and avih is None:
                    avih = p + 8
                elif cc == b"strh" and strh is None and d[p + 8:p + 12] == b"vids":
                    strh = p + 8
                elif cc == b"idx1":
                    idx = (p + 8, min(n, len(d) - p - 8))
                p += 8 + n + (n & 1)

        walk(12, len(d))
        if movi is None or idx is None or avih is None or avih + 40 > len(d):
            raise ValueError(f"MjpegReader: '{path}' has no 'avih' header, no 'movi' list or no 'idx1' index")
        usec, self.width, self.height = struct.unpack_from("<I", d, avih)[0], *struct.unpack_from("<II", d, avih + 32)
        self.fps = 1e6 / usec if usec else 25.0
        if strh is not None and strh + 28 <= len(d):
            scale, rate = struct.unpack_from("<II", d, strh + 20)
            if scale and rate:
                self.fps = rate / scale
        self._index: List[Tuple[int, int]] = []                  # (first byte, length) of every picture
        for e in range(idx[0], idx[0] + idx[1] - 15, 16):
            cc, _, off, n = struct.unpack_from("<4sIII", d, e)
            at = movi + off
            if cc[2:] not in (b"dc", b"db") or cc[:2] != b"00" or n == 0:
                continue
            if at + 8 + n > len(d) or struct.unpack_from("<I", d, at + 4)[0] != n:
                raise ValueError(f"MjpegReader: an index entry of '{path}' does not point at a chunk of its length")
            self._index.append((at + 8, n))
        self.frames = len(self._index)
        self.channels = jpeg.jpeg_info(self.frame_bytes(0))[2] if self.frames else 3

    def frame_bytes(self, i: int) -> bytes:
        """frame i as the JPEG file it is, on the host"""
        at, n = self._index[i]
        return self._data[at:at + n]

    def read(self, start: int = 0, stop: Optional[int] = None, step: int = 1, device="cuda", chunk: int = 8):
        """yields uint8 ``[n,height,width,C]`` on the device, n <= ``chunk``: the frames ``range(start, stop, step)``"""
        from . import jpeg
        dev = codec_io.hip_device(device, "video")
        if int(step) < 1 or int(start) < 0:
            raise ValueError(f"MjpegReader.read: need start >= 0 and step >= 1 (got {start}, {step})")
        which = list(range(int(start), self.frames if stop is None else min(int(stop), self.frames), int(step)))
        for i in range(0, len(which), max(1, int(chunk))):
            part = which[i:i + max(1, int(chunk))]
            images, status = jpeg.decode_blobs([self.frame_bytes(k) for k in part], self.height, self.width, self.channels, dev)
            codec_io.raise_on_status(status, jpeg.JPEG_STATUS, lambda k: f"{self.path}: frame {part[k]}")
            yield images


def read_video(path: str, device="cuda", chunk: int = 8) -> torch.Tensor:
    """An MJPEG AVI file -> uint8 ``[F,H,W,C]`` on the device"""
    r = MjpegReader(path)
    if not r.frames:
        raise ValueError(f"read_video: '{path}' has no frames")
    return torch.cat(list(r.read(device=device, chunk=chunk)), dim=0)


def write_video(path: str, frames: torch.Tensor, chunk: int = 8, **options) -> MjpegWriter:
    """``frames`` uint8 ``[F,H,W,3 or 4]`` on the device -> an MJPEG AVI at ``path``, ``chunk`` frames per encoder call; ``options``:
    ``MjpegWriter``'s keywords.  -> the closed writer (``frames``, ``bytes_to_host``)."""
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
        raise ValueError("write_video: frames must be uint8 [F,H,W,3] or [F,H,W,4]")
    with MjpegWriter(path, frames.shape[1], frames.shape[2], **options) as w:
        for f0 in range(0, frames.shape[0], max(1, int(chunk))):
            w.write(frames[f0:f0 + max(1, int(chunk))])
    return w


def video_options(video) -> dict:
    """``video=True`` or a dict of ``MjpegWriter`` keywords (``fps``, ``quality``, ``subsampling``, ``restart_interval``) -> the dict"""
    if video is True:
        return {}
    if isinstance(video, dict):
        return dict(video)
    raise ValueError(f"video must be None, True or a dict of MjpegWriter's keywords (got {video!r})")
