"""JPEG input on the device (csrc/jpeg_decode.hip, csrc/jpeg_entropy.h) and the resize that frame extraction needs
(csrc/image_resize.hip), so that only compressed bytes cross the bus.

The host reads the files' bytes and uploads them; the marker walk, the restart scan, the Huffman decode, the inverse DCT, the chroma
upsampling and the colour conversion run on the device and every file gets a status.

* ``jpeg_info(data)`` -> ``(H, W, C, subsampling)`` from a file's headers, on the host: what sizes the output.
* ``decode_jpeg(data, offsets, H, W, C, ...)`` -> uint8 ``[B,H,W,C]`` on the device.
* ``read_jpeg_files(paths, device, chunk=32)`` -> uint8 ``[N,H,W,C]`` on the device.
* ``resize_images(images, height, width=None)`` -> uint8 ``[B,h,w,C]`` on the device.

Baseline sequential files only (SOF0, 8 bit, Huffman): grey, or YCbCr at 4:4:4, 4:2:2 or 4:2:0, one interleaved scan, any tables,
any restart interval.  The pixels are libjpeg's, bit for bit what Pillow (libjpeg-turbo) decodes: include/soar_hip.h states the
rules, tests/jpeg_decode_ref.py restates them.  The resize is Pillow's ``Image.resize(BICUBIC)``, bit for bit -- not ffmpeg's scaler.
A file's restart intervals are decoded in parallel, one lane each; a file without restart markers is one lane's serial work, correct
and slow.  HIP only: CPU tensors are refused, there is no CPU fallback.  Out of scope: progressive, extended, lossless and arithmetic
files, 12 bit, four components, other sampling factors, several scans, EXIF orientation.

The plumbing around the kernels that PNG needs as well (guards, upload, the decoder's call, statuses, file lists) is in ``codec_io.py``.
"""
from __future__ import annotations

import ctypes
import functools
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import codec_io, hip_lib
from .hip_lib import check

# a file's status (SOAR_JPEG_* of include/soar_hip.h)
JPEG_OK, JPEG_BAD_STRUCTURE, JPEG_UNSUPPORTED, JPEG_MISSING_TABLE, JPEG_CORRUPT, JPEG_TRUNCATED = range(6)
JPEG_STATUS = {
    JPEG_OK: "ok",
    JPEG_BAD_STRUCTURE: "bad structure (no SOI, a segment running past the end, SOS before SOF, a width or height of 0, or bad offsets)",
    JPEG_UNSUPPORTED: "unsupported (progressive, extended, lossless or arithmetic; 12 bit; 16-bit quantisers; other component counts or "
                      "sampling factors; several scans; or another height, width or component count than the call's)",
    JPEG_MISSING_TABLE: "the frame or the scan names a table that was never defined",
    JPEG_CORRUPT: "corrupt (an invalid Huffman code, a run past coefficient 63, or a wrong or misplaced restart marker)",
    JPEG_TRUNCATED: "truncated: the data ends before the last MCU",
}
_SUBSAMPLING = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}


def jpeg_info(data: bytes) -> Tuple[int, int, int, str]:
    """``(H, W, C, subsampling)`` of a baseline JPEG file from its segments up to the frame header, on the host; subsampling is
    ``"grey"``, ``"444"``, ``"422"`` or ``"420"``.  ``ValueError`` for anything the decoder would call unsupported from the header
    alone.  (The device checks the same fields again, and the rest of the file.)"""
    d = bytes(data)
    if len(d) < 4 or d[:2] != b"\xff\xd8":
        raise ValueError("jpeg_info: not the beginning of a JPEG file")
    p = 2
    while True:
        if p + 4 > len(d) or d[p] != 0xFF:
            raise ValueError("jpeg_info: no frame header before the data ends")
        if d[p + 1] == 0xFF:                                      # a fill byte
            p += 1
            continue
        m, n = d[p + 1], d[p + 2] << 8 | d[p + 3]
        if m in (0x00, 0x01) or 0xD0 <= m <= 0xDA or n < 2:
            raise ValueError(f"jpeg_info: marker FF{m:02X} before the frame header")
        if 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            break
        p += 2 + n
    if m != 0xC0:
        raise ValueError(f"jpeg_info: frame type FF{m:02X}: only baseline sequential files (FFC0) are read")
    if p + 2 + n > len(d) or n < 8 or n != 8 + 3 * d[p + 9]:
        raise ValueError("jpeg_info: the frame header runs past the data or has the wrong length")
    prec, h, w, nc = d[p + 4], d[p + 5] << 8 | d[p + 6], d[p + 7] << 8 | d[p + 8], d[p + 9]
    sampling = [(d[p + 11 + 3 * c] >> 4, d[p + 11 + 3 * c] & 15) for c in range(nc)]
    if prec != 8 or h < 1 or w < 1 or nc not in (1, 3):
        raise ValueError(f"jpeg_info: {w} x {h}, {prec} bit, {nc} components: only 8-bit files of 1 or 3 components are read")
    if nc == 1:
        if sampling[0] != (1, 1):
            raise ValueError(f"jpeg_info: sampling factors {sampling}")
        return h, w, 1, "grey"
    if sampling[0] not in _SUBSAMPLING or sampling[1:] != [(1, 1), (1, 1)]:
        raise ValueError(f"jpeg_info: sampling factors {sampling}: only 4:4:4, 4:2:2 and 4:2:0 are read")
    return h, w, 3, _SUBSAMPLING[sampling[0]]


def decode_jpeg(data: torch.Tensor, offsets: torch.Tensor, H: int, W: int, C: int, strict: bool = True, out: Optional[torch.Tensor] = None,
                return_info: bool = False):
    """``data``: uint8 1-D on the device, B JPEG files one after the other; ``offsets``: int64 ``[B+1]`` on the device, file b being
    ``data[offsets[b]:offsets[b+1]]``; every file ``H`` x ``W`` with ``C`` = 1 (grey) or 3 (YCbCr, returned as RGB) components
    -> uint8 ``[B,H,W,C]`` on the device (``out`` if given).

    Every file gets a status (``JPEG_STATUS``); the image of a failed file is zeros.  With ``strict`` the statuses are read back -- the
    call's one synchronisation -- and a ``ValueError`` names the first failed index and its reason.  With ``strict=False`` nothing is
    read back and ``(images, status)`` is returned, status int32 ``[B]`` on the device.  ``return_info`` adds ``intervals`` (int32
    ``[B]``: the restart intervals the file was decoded in, in parallel; 1 for a file without restart markers)."""
    return codec_io.decode("decode_jpeg", "jpeg", hip_lib.SoarJpegDecodeArgs(), ("soar_jpeg_decode_workspace_bytes", "soar_jpeg_decode"), JPEG_STATUS,
                           data, offsets, H, W, C, strict, out, return_info, channels=(1, 3), sizes_capped=True, empty_ok=False, files_capped=True)


def decode_blobs(blobs: Sequence[bytes], H: int, W: int, C: int, device, out: Optional[torch.Tensor] = None):
    """JPEG files as host bytes -> ``(images, status)`` on the device, nothing read back (``decode_jpeg`` with ``strict=False``)"""
    return decode_jpeg(*codec_io.upload(blobs, torch.device(device)), H, W, C, strict=False, out=out)


def read_jpeg_files(paths: Sequence[str], device="cuda", chunk: int = 32) -> torch.Tensor:
    """The JPEG files ``paths`` (all of one size and component count; the subsampling may differ) -> uint8 ``[N,H,W,C]`` on the device.
    The host reads the files and uploads their bytes, ``chunk`` files per decoder call; nothing is decoded on the host.  Raises with
    the file's name on any status."""
    return codec_io.read_files("read_jpeg_files", "jpeg", paths, device, chunk, lambda blob: jpeg_info(blob)[:3], "components", decode_jpeg,
                               JPEG_STATUS)


# ---- resize -------------------------------------------------------------------------------------------------------------------------
_PRECISION_BITS = 32 - 8 - 2


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _triangle(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


# filter name -> (function, support): Pillow's BICUBIC and BILINEAR (Resample.c: bicubic_filter, bilinear_filter)
_FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_triangle, 1.0)}


def bicubic_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray, int]:
    """``resize_tables(in_size, out_size, "bicubic")``."""
    return resize_tables(in_size, out_size, "bicubic")


@functools.lru_cache(maxsize=32)
def resize_tables(in_size: int, out_size: int, filter: str = "bicubic") -> Tuple[np.ndarray, np.ndarray, int]:
    """Pillow's ``precompute_coeffs`` and ``normalize_coeffs_8bpc`` (Resample.c) for one axis, in the same double arithmetic:
    -> ``(bounds int32 [out,2]`` (first input sample, count), ``coefficients int32 [out,ksize]`` (22-bit fixed point), ``ksize)``.
    The support of the filter (2 for bicubic, 1 for bilinear: the triangle) is widened by the scale factor when shrinking; the
    coefficients of an output are normalised to sum 1.
    (Kept for the sizes last asked for: the arrays are shared and must not be written.)"""
    _kernel, _support = _FILTERS[filter]
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = _support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [_kernel((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        for x in range(xmax):
            v = k[x] / ww if ww != 0.0 else k[x]
            kk[xx, x] = int(-0.5 + v * (1 << _PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << _PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def resize_images(images: torch.Tensor, height: int, width: Optional[int] = None, filter: str = "bicubic") -> torch.Tensor:
    """``images``: uint8 ``[B,H,W,C]`` on the device, C = 1 .. 4 -> uint8 ``[B,height,width,C]``: Pillow's
    ``Image.resize((width, height), Image.BICUBIC)`` (or ``Image.BILINEAR`` with ``filter="bilinear"``), bit for bit (a horizontal pass
    into 8 bits, then a vertical one).  ``width``: ``round(W * height / H)``
    when not given, at least 1.  No synchronisation."""
    if filter not in _FILTERS:
        raise ValueError(f"resize_images: filter must be one of {sorted(_FILTERS)} (got {filter!r})")
    codec_io.need_hip_tensor("images", images, "jpeg")
    if images.dim() != 4 or images.dtype != torch.uint8 or not 1 <= images.shape[3] <= 4 or images.shape[1] < 1 or images.shape[2] < 1:
        raise ValueError(f"resize_images: images must be uint8 [B,H,W,C] with C = 1 .. 4 (got {images.dtype} {tuple(images.shape)})")
    B, H, W, ch = images.shape
    h = int(height)
    w = max(1, int(round(W * h / H))) if width is None else int(width)
    if not (1 <= h <= 65535 and 1 <= w <= 65535 and H <= 65535 and W <= 65535):
        raise ValueError(f"resize_images: sizes must be 1 .. 65535 (got {H} x {W} -> {height} x {width})")
    images = images.detach().contiguous()
    dev = images.device
    out = torch.empty((B, h, w, ch), dtype=torch.uint8, device=dev)
    if B == 0:
        return out
    bh, kh, nh = resize_tables(W, w, filter)
    bv, kv, nv = resize_tables(H, h, filter)
    tables = [torch.from_numpy(t).to(dev, non_blocking=True) for t in (bh, kh, bv, kv)]
    temp = torch.empty((B, H, w, ch), dtype=torch.uint8, device=dev)
    a = hip_lib.SoarResizeArgs()
    a.B, a.H, a.W, a.channels, a.out_h, a.out_w, a.ksize_h, a.ksize_v = B, H, W, ch, h, w, nh, nv
    a.images, a.temp = images.data_ptr(), temp.data_ptr()
    a.bounds_h, a.coef_h, a.bounds_v, a.coef_v = (t.data_ptr() for t in tables)
    with torch.cuda.device(dev):
        check(hip_lib.lib().soar_resize_u8(ctypes.byref(a), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "soar_resize_u8")
    return out
