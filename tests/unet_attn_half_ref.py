"""The restatement of the 16-bit attention (csrc/attention.hip kv_attn16_kernel) in float64, and tests/unet_ref.py's
network with it (soar_amd/unet.py ``attention_precision="bf16"`` / ``"f16"``, alone or with the rounded products of
tests/unet_half_ref.py).

``attention16`` rounds what the kernel rounds and nothing else: ``q scale``, ``k`` and ``v`` to the type (through float32, to nearest
even), and ``p = exp(s - max)`` -- taken against the row's final maximum -- as the operand of ``p v`` only; the softmax's sum runs over
the unrounded ``p``, and every sum is float64."""
import torch

import unet_half_ref as H
import unet_ref as R

DTYPES = H.DTYPES
rounded = H.rounded


def attention16(q, k, v, heads, scale=None, causal=False, precision="bf16"):
    """q [B,Lq,C], k, v [B,Lk,C] (float64) -> [B,Lq,C] with the kernel's four roundings"""
    dt = DTYPES[precision]
    B, Lq, C = q.shape
    Lk, hd = k.shape[1], C // heads
    scale = hd ** -0.5 if scale is None else scale
    qh, kh, vh = (t.reshape(B, -1, heads, hd).permute(0, 2, 1, 3) for t in (rounded(q.double() * scale, dt), rounded(k.double(), dt), rounded(v.double(), dt)))
    s = torch.einsum("bhqd,bhkd->bhqk", qh, kh)
    if causal:
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = torch.einsum("bhqk,bhkd->bhqd", rounded(p, dt), vh) / p.sum(dim=-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B, Lq, C)


def forward(sd, cfg, x, t, context, camera=None, ip_tokens=None, precision="f32", attention_precision="bf16"):
    """-> (eps, stages) of unet_ref.forward in float64 with both attentions as ``attention16`` and, with a 16-bit ``precision``, the
    products' operands rounded as in unet_half_ref.  unet_ref.attention is substituted for the call and put back in a ``finally``."""
    old = R.attention
    R.attention = lambda q, k, v, heads, scale=None: attention16(q, k, v, heads, scale, precision=attention_precision)
    try:
        if precision == "f32":
            return R.forward(sd, cfg, x, t, context, camera, ip_tokens, dtype=torch.float64)
        return H.forward(sd, cfg, x, t, context, camera, ip_tokens, precision=precision)
    finally:
        R.attention = old
