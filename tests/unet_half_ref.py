"""The restatement of tests/unet_ref.py with 16-bit matrix products (soar_amd/unet.py ``precision="bf16"`` / ``"f16"``):
every product operand -- both sides of each ``linear`` and ``conv2d`` -- is rounded to the type (through float32, to nearest even, as
the kernels round a float32 activation and the packer a float32 weight), everything else is float64.  It runs unet_ref's own
functions: for the duration of a call ``unet_ref.linear`` and the ``F`` that unet_ref sees are substituted, and put back in a
``finally``."""
import torch
import torch.nn.functional as F

import unet_ref as R

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def rounded(t, dt):
    """t (float64) rounded to dt, as float64"""
    return t.to(torch.float32).to(dt).to(torch.float64)


class _RoundedF:
    """torch.nn.functional with conv2d's two operands rounded"""

    def __init__(self, dt):
        self.dt = dt

    def conv2d(self, x, w, b=None, **kw):
        return F.conv2d(rounded(x, self.dt), rounded(w, self.dt), b, **kw)

    def __getattr__(self, name):
        return getattr(F, name)


def forward(sd, cfg, x, t, context, camera=None, ip_tokens=None, precision="bf16"):
    """-> (eps, stages) of unet_ref.forward in float64 with the products' operands rounded to ``precision``"""
    dt = DTYPES[precision]

    def linear(x_, sd_, p):
        y = rounded(x_, dt) @ rounded(sd_[p + ".weight"], dt).t()
        return y + sd_[p + ".bias"] if p + ".bias" in sd_ else y

    old = R.linear, R.F
    R.linear, R.F = linear, _RoundedF(dt)
    try:
        return R.forward(sd, cfg, x, t, context, camera, ip_tokens, dtype=torch.float64)
    finally:
        R.linear, R.F = old
