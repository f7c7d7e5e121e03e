"""PNG output and input on the device (csrc/png.hip, csrc/png_decode.hip), so that only compressed bytes cross the bus.

Every stage that ends in a folder of PNGs -- playback, fit inspection, normal maps, masks, evaluation, texture export -- has its uint8
images on the device already.  PNG is what the reference writes (``save_image``) and what ``FrameStore.read_dataroot`` reads back, so
it is not optional; here the row filters, the deflate stream and the checksums are computed on the device and the host only writes
the files.

* ``encode_png(images, ...)`` -> ``(data, offsets)`` on the device: complete PNG files, one after the other.
* ``png_bound(H, W, C, piece_bytes)``: the largest file an image of that shape can become (every piece stored).
* ``save_png(path, image)``: one image.
* ``write_png_files(paths, images, chunk=8)``: a list of files, ``chunk`` images per encoder call; -> the bytes copied to the host.

The deflate stream is cut into independent pieces of ``piece_bytes``, each with a Huffman code of its own over literals and
run-length matches (distance 1 only); include/soar_hip.h and DESIGN.md 9s state every rule, tests/png_ref.py restates them byte for
byte.  Any decoder gives the pixels back exactly.  HIP only: CPU tensors are refused, there is no CPU fallback.  Out of scope:
matches at other distances, 16-bit and palette images, interlacing, ancillary chunks.

Reading: the host reads the files' bytes and uploads them; the chunk walk, the CRCs, inflate, the Adler-32 and the row
filters run on the device and every file gets a status.

* ``png_info(data)`` -> ``(H, W, C)`` from a file's first bytes, on the host: what sizes the output.
* ``decode_png(data, offsets, H, W, C, ...)`` -> uint8 ``[B,H,W,C]`` on the device.
* ``read_png_files(paths, device, chunk=32)`` -> uint8 ``[N,H,W,C]`` on the device.

The plumbing around the kernels that JPEG needs as well (guards, measure and emit, statuses, file lists) is in ``codec_io.py``.
"""
from __future__ import annotations

import struct
from typing import Optional, Sequence, Tuple, Union

import torch

from . import codec_io, hip_lib

FILTERS = {"adaptive": -1, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4}
# A piece is one wavefront's serial work and pays 153 bytes of block header.  Measured on 8 RGBA frames of 1080 x 1920 of the playback
# workload (profiles/png_time.json): pieces of 16 KiB, 32 KiB and 65535 bytes encode in 0.65, 0.98 and 1.69 ms and give 1 369, 1 038 and
# 875 KB -- such frames are mostly background, a piece shrinks to a few hundred bytes and the header is a large part of it.  The
# files are what is kept, and a millisecond per 8 frames is little next to writing them: the largest piece.
DEFAULT_PIECE_BYTES = 65535
_COLOUR_CHANNELS = (1, 3, 4)


def png_bound(H: int, W: int, C: int, piece_bytes: Optional[int] = None) -> int:
    """The largest PNG file ``encode_png`` writes for one ``[H,W,C]`` image: every piece a stored block.  8 bytes of signature, IHDR
    (25), the zlib header (2), per piece an IDAT's framing (12) and a stored block's (5), the filtered stream ``H (1 + W C)``, the
    final IDAT (18) and IEND (12)."""
    P = DEFAULT_PIECE_BYTES if piece_bytes is None else int(piece_bytes)
    if not 32 <= P <= 65535:
        raise ValueError(f"png_bound: piece_bytes must be 32 .. 65535 (got {piece_bytes})")
    S = int(H) * (1 + int(W) * int(C))
    return 8 + 25 + 2 + ((S + P - 1) // P) * 17 + S + 18 + 12


def _encode(images, filters, piece_bytes, out):
    codec_io.need_hip_tensor("images", images, "png")
    if images.dim() != 4 or images.dtype != torch.uint8 or images.shape[3] not in _COLOUR_CHANNELS:
        raise ValueError(f"encode_png: images must be uint8 [B,H,W,1], [B,H,W,3] or [B,H,W,4] (got {images.dtype} {tuple(images.shape)})")
    if isinstance(filters, bool) or filters not in FILTERS:
        raise ValueError(f"encode_png: filters must be 'adaptive' or a filter type 0 .. 4 (got {filters!r})")
    P = DEFAULT_PIECE_BYTES if piece_bytes is None else int(piece_bytes)
    if not 32 <= P <= 65535:
        raise ValueError(f"encode_png: piece_bytes must be 32 .. 65535 (got {piece_bytes})")
    a = hip_lib.SoarPngArgs()
    a.B, a.H, a.W, a.channels, a.filter, a.piece_bytes = *images.shape, FILTERS[filters], P
    images, a.images, a.image_stride = codec_io.batch_view("encode_png", images)
    return codec_io.measure_and_emit("encode_png", a, ("soar_png_workspace_bytes", "soar_png_measure", "soar_png_emit"), a.B, images.device, out)


def encode_png(images: torch.Tensor, filters: Union[str, int] = "adaptive", piece_bytes: Optional[int] = None,
               out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``images``: uint8 ``[B,H,W,C]`` on the device, C = 1 (grey), 3 (RGB) or 4 (RGBA); every image contiguous, any step from image
    to image -> ``(data, offsets)``, both on the device: ``data`` uint8, the B complete PNG files one after the other, and ``offsets``
    int64 ``[B+1]``: image b is ``data[offsets[b]:offsets[b+1]]``.  ``filters``: ``"adaptive"`` (per row the filter with the smallest
    sum of absolute residuals) or one PNG filter type 0 .. 4 for every row; ``piece_bytes``: 32 .. 65535 bytes of the filtered
    stream per independent deflate block and wavefront (default ``DEFAULT_PIECE_BYTES``).

    With ``out=None`` the sizes are measured on the device, the ``B + 1`` offsets are read back -- the call's one synchronisation --
    and ``data`` is allocated exactly.  With a caller's ``out`` (1-D uint8 on the device; ``B * png_bound(...)`` always suffices)
    nothing synchronises; ``data`` is ``out``.  If it is too small NOTHING is written into it and ``offsets[-1] > out.numel()`` says
    so: overflow is reported, never written."""
    data, offsets, _ = _encode(images, filters, piece_bytes, out)
    return data, offsets


def save_png(path: str, image: torch.Tensor) -> None:
    """``image``: uint8 ``[H,W]``, ``[H,W,1]``, ``[H,W,3]`` or ``[H,W,4]`` on the device -> a PNG file at ``path``."""
    if isinstance(image, torch.Tensor) and image.dim() not in (2, 3):
        raise ValueError(f"save_png: image must be uint8 [H,W] or [H,W,C] with C = 1, 3 or 4 (got {tuple(image.shape)})")
    write_png_files([path], image[None] if isinstance(image, torch.Tensor) else image)


def write_png_files(paths: Sequence[str], images: torch.Tensor, chunk: int = 8) -> int:
    """``images``: uint8 ``[N,H,W,C]`` (or ``[N,H,W]``: grey) on the device; ``paths``: N file names.  ``chunk`` images are encoded
    per call, only the compressed bytes are copied to the host, and the files are written.  -> the bytes copied."""
    if isinstance(images, torch.Tensor) and images.dim() == 3:
        images = images[..., None]
    if isinstance(images, torch.Tensor) and (images.dim() != 4 or images.shape[0] != len(paths)):
        raise ValueError(f"write_png_files: images must be uint8 [N,H,W,C] or [N,H,W] with one of the {len(paths)} paths each (got {tuple(images.shape)})")
    step, copied = max(1, int(chunk)), 0
    for i in range(0, len(paths), step):
        data, _, offsets = _encode(images[i:i + step] if isinstance(images, torch.Tensor) else images, "adaptive", None, None)
        files, n = codec_io.host_items(data, offsets)
        copied += n
        for path, file in zip(paths[i:], files):
            with open(path, "wb") as f:
                f.write(file)
    return copied


# ---- reading --------------------------------------------------------------------------------------------------------------------------
# a file's status (SOAR_PNG_* of include/soar_hip.h)
PNG_OK, PNG_BAD_STRUCTURE, PNG_UNSUPPORTED, PNG_BAD_CRC, PNG_CORRUPT, PNG_WRONG_LENGTH, PNG_BAD_ADLER, PNG_BAD_FILTER = range(8)
PNG_STATUS = {
    PNG_OK: "ok",
    PNG_BAD_STRUCTURE: "bad signature or chunk structure (truncated, no IDAT, IHDR not first, a width or height of 0, or bad offsets)",
    PNG_UNSUPPORTED: "unsupported (interlace, a depth other than 8, colour type 3 or 4, FDICT, or another height, width or colour type "
                     "than the call's)",
    PNG_BAD_CRC: "chunk CRC mismatch",
    PNG_CORRUPT: "corrupt deflate stream",
    PNG_WRONG_LENGTH: "the stream does not inflate to H (1 + W C) bytes, or bytes follow its final block other than the Adler-32",
    PNG_BAD_ADLER: "Adler-32 mismatch",
    PNG_BAD_FILTER: "filter byte above 4",
}
_SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS_OF_TYPE = {0: 1, 2: 3, 6: 4}


def png_info(data: bytes) -> Tuple[int, int, int]:
    """``(H, W, C)`` of a PNG file from its first 26 bytes, on the host; ``ValueError`` for anything that is not the header of an 8-bit
    grey, RGB or RGBA file.  (The device checks the same fields again, and the rest of the file.)"""
    data = bytes(data[:26])
    if len(data) < 26 or data[:8] != _SIGNATURE or data[12:16] != b"IHDR":
        raise ValueError("png_info: not the beginning of a PNG file")
    w, h, depth, colour = struct.unpack(">IIBB", data[16:26])
    if depth != 8 or colour not in _CHANNELS_OF_TYPE or w < 1 or h < 1:
        raise ValueError(f"png_info: {w} x {h}, bit depth {depth}, colour type {colour}: only 8-bit colour types 0, 2 and 6 are read")
    return h, w, _CHANNELS_OF_TYPE[colour]


def decode_png(data: torch.Tensor, offsets: torch.Tensor, H: int, W: int, C: int, strict: bool = True, out: Optional[torch.Tensor] = None,
               return_info: bool = False):
    """``data``: uint8 1-D on the device, B PNG files one after the other; ``offsets``: int64 ``[B+1]`` on the device, file b being
    ``data[offsets[b]:offsets[b+1]]``; every file ``H`` x ``W`` with ``C`` = 1 (grey), 3 (RGB) or 4 (RGBA) channels of 8 bits
    -> uint8 ``[B,H,W,C]`` on the device (``out`` if given).

    Every file gets a status (``PNG_STATUS``); the image of a failed file is zeros.  With ``strict`` the statuses are read back -- the
    call's one synchronisation -- and a ``ValueError`` names the first failed index and its reason.  With ``strict=False`` nothing is
    read back and ``(images, status)`` is returned, status int32 ``[B]`` on the device.  ``return_info`` adds ``segments`` (int32
    ``[B]``: the pieces the file's deflate stream was proven to consist of and was decoded in, 1 for a serial stream)."""
    return codec_io.decode("decode_png", "png", hip_lib.SoarPngDecodeArgs(), ("soar_png_decode_workspace_bytes", "soar_png_decode"), PNG_STATUS,
                           data, offsets, H, W, C, strict, out, return_info, channels=_COLOUR_CHANNELS, sizes_capped=False, empty_ok=True,
                           files_capped=False)


def read_png_files(paths: Sequence[str], device="cuda", chunk: int = 32) -> torch.Tensor:
    """The PNG files ``paths`` (all of one size and colour type) -> uint8 ``[N,H,W,C]`` on the device.  The host reads the files and
    uploads their bytes, ``chunk`` files per decoder call; nothing is decoded on the host.  Raises with the file's name on any status."""
    return codec_io.read_files("read_png_files", "png", paths, device, chunk, png_info, "channels", decode_png, PNG_STATUS)
