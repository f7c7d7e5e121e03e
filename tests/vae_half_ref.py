"""The float64 restatement (tests/vae_ref.py) with 16-bit operands where the encoder's 16-bit precisions have them:
every convolution of the chain except ``conv_in``, ``conv_out`` and ``quant_conv`` -- the residual blocks' conv1 / conv2 /
nin_shortcut, the downsamples, q, k, v, proj_out -- becomes

    forward   conv2d(rounded(x), rounded(w)) + b
    backward  conv2d_input(rounded(g), rounded(w))

with ``rounded(t) = t.to(type).to(float64)`` (nearest even) and everything else, the sums included, in float64.  The attention's
products of two activations, softmax, GroupNorm, the resize and the sample are vae_ref's own.  At f16 the backward of each such
product runs on ``g * 2^10`` and divides by ``2^10`` afterwards; the chain between the products is linear and a power of two is exact,
so this is the chain run on ``2^10 g`` as a whole and divided at the end.

``vae_ref`` is not edited: ``half(dtype)`` swaps its ``_conv`` for the duration of a ``with`` block.  The rounding has no derivative,
so this restatement cannot be gradchecked; it is the yardstick for how far 16-bit operands may move a result, not an oracle of its
own correctness.

Per product the backward records (``Stats``): the share of the non-zero gradient operands (after the 2^10, before rounding) that lie
below 2^-14, f16's smallest normal number, and the largest such operand.
"""
import contextlib

import torch
import torch.nn.functional as F

import vae_ref as R

FLOAT32_KEYS = ("encoder.conv_in", "encoder.conv_out", "quant_conv")
F16_PRESCALE = 2.0 ** 10
TINY = 2.0 ** -14


class Stats:
    """what the products' backward passes saw: key -> (share of non-zero gradient operands below 2^-14, largest operand)"""

    def __init__(self):
        self.per_product = {}

    def add(self, key, g):
        a = g.detach().abs()
        nz = a > 0
        n = int(nz.sum())
        share = float(((a < TINY) & nz).sum()) / n if n else 0.0
        self.per_product[key] = (share, float(a.max()) if a.numel() else 0.0)

    def worst_share(self):
        return max((s for s, _ in self.per_product.values()), default=0.0)

    def largest(self):
        return max((m for _, m in self.per_product.values()), default=0.0)


def _rounded(t, dtype):
    return t.to(dtype).to(torch.float64)


class _Conv16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, dtype, stride, padding, key, stats):
        wr = _rounded(w, dtype)
        ctx.save_for_backward(wr)
        ctx.meta = (tuple(x.shape), dtype, stride, padding, key, stats)
        return F.conv2d(_rounded(x, dtype), wr, b, stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, g):
        (wr,) = ctx.saved_tensors
        shape, dtype, stride, padding, key, stats = ctx.meta
        pre = F16_PRESCALE if dtype == torch.float16 else 1.0
        gs = g * pre
        if stats is not None:
            stats.add(key, gs)
        gx = torch.nn.grad.conv2d_input(shape, wr, _rounded(gs, dtype), stride=stride, padding=padding) / pre
        return gx, None, None, None, None, None, None, None


@contextlib.contextmanager
def half(dtype, stats=None):
    """inside: vae_ref's chain with 16-bit operands of ``dtype`` (torch.bfloat16 / torch.float16); ``stats``: a Stats to fill"""
    plain = R._conv

    def conv(x, w, p, stride=1, padding=0):
        if p in FLOAT32_KEYS:
            return plain(x, w, p, stride=stride, padding=padding)
        return _Conv16.apply(x, w[p + ".weight"], w[p + ".bias"], dtype, stride, padding, p, stats)

    R._conv = conv
    try:
        yield
    finally:
        R._conv = plain


def latents_and_grad(x, w, image_size, eps, gw, dtype=None, stats=None):
    """x, eps, gw float64, w float64 weights -> (latents, d sum(latents gw) / d x, mean, logvar): plain float64 (dtype None) or
    with 16-bit operands"""
    ctx = half(dtype, stats) if dtype is not None else contextlib.nullcontext()
    with ctx:
        xv = x.detach().clone().requires_grad_(True)
        lat = R.latents(xv, w, image_size, eps)
        (lat * gw).sum().backward()
        with torch.no_grad():
            mean, logvar = R.moments(x, w, image_size)
    return lat.detach(), xv.grad, mean, logvar
