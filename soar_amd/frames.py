"""Frame extraction on the device: the reference's first preprocessing stage (``preproc/extract_frames.py``), from a video to
``<data_root>/<seq>/images/%05d.png``.

The reference calls ffmpeg: every ``skip_time``-th frame between two times, scaled to a height, written as PNGs numbered from 0.
Here the video is an MJPEG ``.avi`` (what ``MjpegWriter`` writes, and what phones and cameras record) or a directory of ``.jpg`` /
``.jpeg`` files; its frames are uploaded as the compressed bytes they are, decoded (``soar_amd.jpeg``), resized
(``resize_images``) and encoded as PNG (``soar_amd.png``) on the device, chunk by chunk: only compressed bytes cross the bus, in
either direction.  The pixels are libjpeg's through Pillow's bicubic resize -- not ffmpeg's scaler and not its YUV -> RGB path, which
are other rules.  ``FrameStore.from_dataroot(..., device_png=True)`` and every later stage take it from there.  Out of scope:
H.264 / MP4 and every other codec and container, audio, OpenDML AVIs, EXIF orientation.
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch

from . import jpeg
from .png import write_png_files
from .video import MjpegReader


def _seconds(t) -> float:
    """``"HH:MM:SS[.fff]"``, ``"MM:SS"``, or a number of seconds, as ffmpeg's ``-ss`` / ``-to`` take them"""
    if isinstance(t, (int, float)):
        return float(t)
    total = 0.0
    for part in str(t).split(":"):
        total = total * 60.0 + float(part)
    return total


def frame_indices(frames: int, fps: float, skip_time: int = 1, start_time="00:00:00", end_time=None) -> List[int]:
    """The frames ffmpeg's ``select='not(mod(n,skip_time))'`` with ``-ss start_time -to end_time`` keeps: every ``skip_time``-th frame n
    (counted from the file's first) whose time ``n / fps`` lies in ``[start_time, end_time)``."""
    if int(skip_time) < 1:
        raise ValueError(f"extract_frames: skip_time must be at least 1 (got {skip_time})")
    first = max(0, math.ceil(_seconds(start_time) * fps - 1e-9))
    last = frames if end_time is None else min(frames, math.ceil(_seconds(end_time) * fps - 1e-9))
    return [n for n in range(0, frames, int(skip_time)) if first <= n < last]


def extract_frames(video_path: str, data_root: str, height: int = -1, skip_time: int = 1, start_time: str = "00:00:00",
                   end_time: Optional[str] = None, chunk: int = 8, device="cuda") -> int:
    """The reference's stage with its argument names and folder layout.  ``video_path``: an MJPEG ``.avi``, or a directory of
    ``.jpg`` / ``.jpeg`` files taken in sorted order (a directory has no times: anything but the default ``skip_time``,
    ``start_time`` and ``end_time`` is refused).  ``height`` > 0: frames are resized to that height, the width following
    (``scale=-1:height``); otherwise they keep their size.  -> the number of frames written; 0 if
    ``<data_root>/<stem>/images`` already holds files, which are left alone, as the reference leaves them.  A link
    ``<data_root>/<stem>/video<ext>`` to the source is made as the reference's ``video.mp4`` is."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"device is '{dev}': soar_amd.frames runs on HIP devices only; there is no CPU fallback")
    source = os.path.normpath(video_path)
    stem, ext = os.path.splitext(os.path.basename(source))
    is_dir = os.path.isdir(source)
    if is_dir:
        stem, ext = os.path.basename(source), ""
    img_dir = os.path.join(data_root, stem, "images")
    if os.path.exists(img_dir) and len(os.listdir(img_dir)) > 0:
        return 0
    step = max(1, int(chunk))
    if is_dir:
        if int(skip_time) != 1 or _seconds(start_time) != 0.0 or end_time is not None:
            raise ValueError("extract_frames: a directory of pictures has no times: skip_time, start_time and end_time must keep their defaults")
        files = sorted(os.path.join(source, f) for f in os.listdir(source) if f.lower().endswith((".jpg", ".jpeg")))
        if not files:
            raise ValueError(f"extract_frames: no .jpg or .jpeg files in '{video_path}'")
        chunks = (jpeg.read_jpeg_files(files[i:i + step], dev, chunk=step) for i in range(0, len(files), step))
    else:
        reader = MjpegReader(source)
        which = frame_indices(reader.frames, reader.fps, skip_time, start_time, end_time)
        if not which:
            raise ValueError(f"extract_frames: no frame of '{video_path}' ({reader.frames} frames at {reader.fps:g} per second) is selected")
        # every skip_time-th frame from the first selected one: a range, which is what the reader takes
        chunks = reader.read(which[0], which[-1] + 1, int(skip_time), dev, chunk=step)
    os.makedirs(img_dir, exist_ok=True)
    written = 0
    for images in chunks:
        if int(height) > 0:
            images = jpeg.resize_images(images, int(height))
        write_png_files([os.path.join(img_dir, f"{written + k:05d}.png") for k in range(images.shape[0])], images, chunk=step)
        written += images.shape[0]
    link = os.path.join(data_root, stem, "video" + ext)
    if not os.path.lexists(link):
        os.symlink(os.path.abspath(source), link)
    return written
