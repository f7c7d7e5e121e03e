"""What the image codecs share around their kernels (png.py, video.py, jpeg.py; the host side's counterpart is csrc/codec_common.h):
the HIP-only guard, the rule for a batch of images, the encoders' measure / read back the offsets / emit, the upload of a list of
files, the decoders' call, the reading of the statuses and of a list of files, and the compressed bytes' way to the host.  Private:
the formats' modules are the interface, and every message names the function the caller called (``who``) or its module."""
from __future__ import annotations

import ctypes
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check


def need_hip_tensor(name: str, t, module: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        where = t.device if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name} is on '{where}': soar_amd.{module} runs on HIP devices only; there is no CPU fallback")


def hip_device(device, module: str) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device is '{dev}': soar_amd.{module} runs on HIP devices only; there is no CPU fallback")
    return dev


def batch_view(who: str, images: torch.Tensor) -> Tuple[torch.Tensor, Optional[int], int]:
    """uint8 ``[B,H,W,C]`` -> ``(tensor, its pointer or None, bytes from image to image)`` as the encoders' args take them: every
    image contiguous, the step from image to image free, so a batch cut out of a larger buffer is not copied."""
    B, H, W, ch = images.shape
    if not (1 <= H <= 65535 and 1 <= W <= 65535 and B <= 65535):
        raise ValueError(f"{who}: need 1 <= H, W <= 65535 and B <= 65535 (got {tuple(images.shape)})")
    images = images.detach()
    if B and not (images[0].is_contiguous() and (B < 2 or images.stride(0) >= H * W * ch)):
        images = images.contiguous()
    return images, images.data_ptr() if B else None, images.stride(0) if B > 1 else H * W * ch


def measure_and_emit(who: str, a, entry_points: Tuple[str, str, str], B: int, dev, out: Optional[torch.Tensor]):
    """``a``: an encoder's args; ``entry_points``: its sizing, measure and emit calls -> ``(data, offsets, host)``: ``host`` is the
    host copy of the offsets that sized ``data``, None with a caller's ``out``."""
    if out is not None and (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8 or out.dim() != 1 or
                            not out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous 1-D uint8 tensor on {dev}")
    sizing, measure, emit = entry_points
    lib = hip_lib.lib()
    ws = _workspace(_bytes(getattr(lib, sizing), sizing, ctypes.byref(a)), dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    host = None
    with torch.cuda.device(dev):
        stream = _stream(dev)
        check(getattr(lib, measure)(ctypes.byref(a), ws.data_ptr(), ws.numel(), offsets.data_ptr(), stream), measure)
        if out is None:
            host = offsets.cpu()                                  # the one read-back: B + 1 offsets
            out = torch.empty(int(host[-1]), dtype=torch.uint8, device=dev)
        check(getattr(lib, emit)(ctypes.byref(a), ws.data_ptr(), ws.numel(), hip_lib.ptr(out), out.numel(), stream), emit)
    return out, offsets, host


def host_items(data: torch.Tensor, host_offsets: torch.Tensor) -> Tuple[List[bytes], int]:
    """The compressed bytes to the host in one copy, cut by the host copy of the offsets -> ``(the items, the bytes copied)``"""
    host = data.cpu().numpy().tobytes()
    off = host_offsets.tolist()
    return [host[off[b]:off[b + 1]] for b in range(len(off) - 1)], len(host)


def upload(blobs: Sequence[bytes], dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """files as host bytes -> ``(data, offsets)`` on the device (a list of nothing but empty files has a buffer to start from, too)"""
    off = [0]
    for b in blobs:
        off.append(off[-1] + len(b))
    data = torch.frombuffer(bytearray(b"".join(blobs) or b"\x00"), dtype=torch.uint8)[:off[-1]].to(dev, non_blocking=True)
    return data, torch.tensor(off, dtype=torch.int64).to(dev, non_blocking=True)


def raise_on_status(status: torch.Tensor, table: Dict[int, str], name_of: Callable[[int], str], list_failed: bool = False) -> None:
    """``status``: int32 per item, read back here (a synchronisation).  A ``ValueError`` for the first item that is not ok: what
    ``name_of(i)`` calls it, the table's text, and with ``list_failed`` every failed index."""
    host = status.cpu()
    bad = torch.nonzero(host).reshape(-1).tolist()
    if bad:
        code = int(host[bad[0]])
        raise ValueError(f"{name_of(bad[0])}: {table.get(code, code)} (status {code})" + (f"; failed files: {bad}" if list_failed else ""))


def decode(who: str, module: str, a, entry_points: Tuple[str, str], table: Dict[int, str], data, offsets, H, W, C, strict: bool,
           out: Optional[torch.Tensor], return_info: bool, channels: Tuple[int, ...], sizes_capped: bool, empty_ok: bool,
           files_capped: bool):
    """The body of ``decode_png`` and ``decode_jpeg``.  ``a``: the decoder's args, empty; ``entry_points``: its sizing call and the
    decoder; the rest of the keywords are the format's limits: C, whether H and W end at 65535, whether no file at all is a call,
    whether a call ends at 65535 files."""
    for name, t, dt in (("data", data, torch.uint8), ("offsets", offsets, torch.int64)):
        need_hip_tensor(name, t, module)
        if t.dtype != dt or t.dim() != 1 or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous 1-D {dt} tensor (got {t.dtype} {tuple(t.shape)})")
    dev = data.device
    if offsets.device != dev or offsets.numel() < (1 if empty_ok else 2):
        raise ValueError(f"{who}: offsets must be B + 1 values on {dev}" + ("" if empty_ok else ", B >= 1"))
    H, W, ch = int(H), int(W), int(C)
    if H < 1 or W < 1 or (sizes_capped and (H > 65535 or W > 65535)) or ch not in channels:
        raise ValueError(f"{who}: need {'1 <= H, W <= 65535' if sizes_capped else 'H, W >= 1'} and "
                         f"C = {', '.join(map(str, channels[:-1]))} or {channels[-1]} (got {H}, {W}, {C})")
    B = offsets.numel() - 1
    if files_capped and B > 65535:
        raise ValueError(f"{who}: at most 65535 files per call (got {B})")
    if out is None:
        out = torch.empty((B, H, W, ch), dtype=torch.uint8, device=dev)
    elif (not isinstance(out, torch.Tensor) or out.device != dev or out.dtype != torch.uint8 or tuple(out.shape) != (B, H, W, ch) or
          not out.is_contiguous()):
        raise ValueError(f"{who}: out must be a contiguous uint8 [{B},{H},{W},{ch}] tensor on {dev}")
    status = torch.empty(B, dtype=torch.int32, device=dev)
    info = torch.empty(B, dtype=torch.int32, device=dev)
    if B:
        sizing, decoder = entry_points
        a.B, a.H, a.W, a.channels, a.total_bytes = B, H, W, ch, data.numel()
        a.data, a.offsets = hip_lib.ptr(data), offsets.data_ptr()
        lib = hip_lib.lib()
        ws = _workspace(_bytes(getattr(lib, sizing), sizing, ctypes.byref(a)), dev)
        with torch.cuda.device(dev):
            if data.numel() == 0:
                a.data = ws.data_ptr()                            # (no byte of it is read: every file is empty)
            check(getattr(lib, decoder)(ctypes.byref(a), ws.data_ptr(), ws.numel(), out.data_ptr(), status.data_ptr(), info.data_ptr(),
                                        _stream(dev)), decoder)
    if strict:
        raise_on_status(status, table, lambda i: f"{who}: file {i} of {B}", list_failed=True)
        return (out, info) if return_info else out
    return (out, status, info) if return_info else (out, status)


def read_files(who: str, module: str, paths: Sequence[str], device, chunk: int, info_of: Callable[[bytes], Tuple[int, int, int]], noun: str,
               decoder: Callable, table: Dict[int, str]) -> torch.Tensor:
    """The body of ``read_png_files`` and ``read_jpeg_files``.  ``info_of``: a file's bytes -> ``(H, W, C)`` on the host; ``noun``:
    what the format calls C; ``decoder``: ``decode_png`` or ``decode_jpeg``."""
    dev = hip_device(device, module)
    paths = list(paths)
    if not paths:
        raise ValueError(f"{who}: no files")
    blobs, info = [], None
    for p in paths:
        with open(p, "rb") as f:
            blobs.append(f.read())
        try:
            here = tuple(info_of(blobs[-1]))
        except ValueError as e:
            raise ValueError(f"{p}: {e}") from None
        if info is None:
            info = here
        elif here != info:
            raise ValueError(f"{p}: {here[0]} x {here[1]} with {here[2]} {noun}, but {paths[0]} has {info[0]} x {info[1]} with {info[2]}")
    H, W, ch = info
    out = torch.empty((len(paths), H, W, ch), dtype=torch.uint8, device=dev)
    step, pending = max(1, int(chunk)), []
    for i in range(0, len(paths), step):
        part = blobs[i:i + step]
        _, status = decoder(*upload(part, dev), H, W, ch, strict=False, out=out[i:i + len(part)])
        pending.append((i, status))
    for i, status in pending:                                     # the statuses of all calls, read once they all are queued
        raise_on_status(status, table, lambda k: paths[i + k])
    return out
