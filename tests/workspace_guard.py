"""Guard bands round every caller-owned workspace (helper of test_workspace_contract_{cpu,gpu}.py).

``guarded(fill)`` swaps ``hip_lib._workspace`` -- under every name by which a ``soar_amd`` module holds it -- and
``soar_amd.rasterizer._scratch`` for an allocator that puts each workspace between two bands of ``GUARD_BYTE`` and fills the
workspace itself with zeros, 0xFF bytes or seeded noise.  The slice handed out has exactly the size that was asked for, so an entry
point is told what its sizing call answered and not a byte more; the caching allocator's rounding no longer hides an overrun, and
its zeroed or stale pages no longer hide a read of something nobody wrote.
"""
from __future__ import annotations

import contextlib
import importlib
import pkgutil
import sys

import numpy as np
import torch

GUARD = 64 * 1024
GUARD_BYTE = 0xA5
ALIGN = 256
FILLS = ("zeros", "ones", "noise")
NOISE_SEED = 0x5EED


def modules_with_workspace():
    """Every module of the ``soar_amd`` package that has a ``_workspace`` attribute, found by walking the package."""
    import soar_amd
    out = []
    for info in pkgutil.walk_packages(soar_amd.__path__, soar_amd.__name__ + "."):
        mod = importlib.import_module(info.name)
        if hasattr(mod, "_workspace"):
            out.append(mod)
    return out


def _asker() -> str:
    """The ``soar_amd`` module whose code asked for the workspace (the nearest such frame above the allocator)."""
    f = sys._getframe(2)
    while f is not None:
        name = f.f_globals.get("__name__", "")
        if name.startswith("soar_amd"):
            return name
        f = f.f_back
    return "?"


class Guard:
    """The allocator of one ``guarded`` context and the buffers it has handed out."""

    def __init__(self, fill: str, shorten: int = 0):
        if fill not in FILLS:
            raise ValueError(f"fill must be one of {FILLS}, got {fill!r}")
        self.fill, self.buffers = fill, []
        self._shorten = int(shorten)     # by-hand demonstration only (see the GPU test's docstring): the slice ends early

    def alloc(self, nbytes: int, device) -> torch.Tensor:
        nbytes, device = int(nbytes), torch.device(device)
        index = len(self.buffers)
        raw = torch.full((nbytes + 2 * GUARD + ALIGN,), GUARD_BYTE, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % ALIGN          # 0 on the device (its allocations are 256-byte aligned); anything on the host
        buf = raw[off:off + nbytes + 2 * GUARD]
        ws = buf[GUARD:GUARD + nbytes]
        assert ws.data_ptr() % ALIGN == 0 and ws.numel() == nbytes
        if self.fill == "zeros":
            ws.zero_()
        elif self.fill == "ones":
            ws.fill_(0xFF)
        else:
            noise = np.random.default_rng([NOISE_SEED, index]).integers(0, 256, nbytes, dtype=np.uint8)
            ws.copy_(torch.from_numpy(noise))
        self.buffers.append((index, nbytes, _asker(), buf))
        if self._shorten:
            # the entry point is still told `nbytes` (every caller passes the sizing call's answer, not ws.numel()): the last
            # `shorten` bytes of what it may use are guard band
            buf[GUARD + nbytes - self._shorten:GUARD + nbytes] = GUARD_BYTE
        return ws

    def check(self) -> None:
        """Both bands of every buffer still hold GUARD_BYTE everywhere."""
        if any(b[3].is_cuda for b in self.buffers):
            torch.cuda.synchronize()
        for index, nbytes, asker, buf in self.buffers:
            end = GUARD + nbytes - self._shorten
            for after, band in ((True, buf[end:]), (False, buf[:GUARD])):
                dead = (band != GUARD_BYTE).nonzero().flatten()
                if dead.numel() == 0:
                    continue
                at = int(dead[0] if after else dead[-1])         # the dead byte nearest to the workspace
                where = f"{at} bytes past the workspace's end" if after else f"{GUARD - at} bytes before the workspace's start"
                raise AssertionError(f"workspace #{index} ({nbytes} bytes, asked for by {asker}, fill {self.fill!r}): {dead.numel()} guard "
                                     f"byte(s) {'after' if after else 'before'} it overwritten, the nearest {where} (it holds {int(band[at])})")


@contextlib.contextmanager
def guarded(fill: str, shorten: int = 0):
    """Within the context every workspace of the package comes from a ``Guard``; yields it (``check()``, ``buffers``)."""
    import soar_amd.rasterizer as rasterizer
    g = Guard(fill, shorten)
    saved = [(m, "_workspace", m._workspace) for m in modules_with_workspace()] + [(rasterizer, "_scratch", rasterizer._scratch)]
    try:
        for m, name, _ in saved:
            setattr(m, name, g.alloc)
        yield g
    finally:
        for m, name, orig in saved:
            setattr(m, name, orig)
        g.buffers.clear()
