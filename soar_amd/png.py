"""PNG output: complete PNG files made on the device (csrc/png.hip), so that only compressed bytes cross to the host.

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
matches at other distances, 16-bit and palette images, interlacing, ancillary chunks, decoding.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple, Union

import torch

from . import hip_lib
from .hip_lib import check

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


def _args_of(images: torch.Tensor, filters, piece_bytes: Optional[int]):
    if not isinstance(images, torch.Tensor) or not images.is_cuda:
        where = images.device if isinstance(images, torch.Tensor) else type(images).__name__
        raise RuntimeError(f"images is on '{where}': soar_amd.png runs on HIP devices only; there is no CPU fallback")
    if images.dim() != 4 or images.dtype != torch.uint8 or images.shape[3] not in _COLOUR_CHANNELS:
        raise ValueError(f"encode_png: images must be uint8 [B,H,W,1], [B,H,W,3] or [B,H,W,4] (got {images.dtype} {tuple(images.shape)})")
    if isinstance(filters, bool) or filters not in FILTERS:
        raise ValueError(f"encode_png: filters must be 'adaptive' or a filter type 0 .. 4 (got {filters!r})")
    P = DEFAULT_PIECE_BYTES if piece_bytes is None else int(piece_bytes)
    if not 32 <= P <= 65535:
        raise ValueError(f"encode_png: piece_bytes must be 32 .. 65535 (got {piece_bytes})")
    B, H, W, ch = images.shape
    if not (1 <= H <= 65535 and 1 <= W <= 65535 and B <= 65535):
        raise ValueError(f"encode_png: need 1 <= H, W <= 65535 and B <= 65535 (got {tuple(images.shape)})")
    images = images.detach()
    # every image contiguous; the step from image to image is free
    if B and not (images[0].is_contiguous() and (B < 2 or images.stride(0) >= H * W * ch)):
        images = images.contiguous()
    a = hip_lib.SoarPngArgs()
    a.B, a.H, a.W, a.channels, a.filter, a.piece_bytes = B, H, W, ch, FILTERS[filters], P
    a.images = images.data_ptr() if B else None
    a.image_stride = images.stride(0) if B > 1 else H * W * ch
    return a, images


def _encode(images, filters, piece_bytes, out):
    a, images = _args_of(images, filters, piece_bytes)
    dev = images.device
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8 or out.dim() != 1 or
                            not out.is_contiguous()):
        raise ValueError(f"encode_png: out must be a contiguous 1-D uint8 tensor on {dev}")
    lib = hip_lib.lib()
    ws = torch.empty(hip_lib._bytes(lib.soar_png_workspace_bytes, "soar_png_workspace_bytes", C.byref(a)), dtype=torch.uint8, device=dev)
    offsets = torch.empty(a.B + 1, dtype=torch.int64, device=dev)
    host = None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib.soar_png_measure(C.byref(a), ws.data_ptr(), ws.numel(), offsets.data_ptr(), stream), "soar_png_measure")
        if out is None:
            host = offsets.cpu()                                  # the one read-back: B + 1 offsets
            out = torch.empty(int(host[-1]), dtype=torch.uint8, device=dev)
        check(lib.soar_png_emit(C.byref(a), ws.data_ptr(), ws.numel(), hip_lib.ptr(out), out.numel(), stream), "soar_png_emit")
    return out, offsets, host


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
        host = data.cpu().numpy().tobytes()
        copied += len(host)
        off = offsets.tolist()                                    # (the host copy of the offsets that sized data)
        for b in range(len(off) - 1):
            with open(paths[i + b], "wb") as f:
                f.write(host[off[b]:off[b + 1]])
    return copied
