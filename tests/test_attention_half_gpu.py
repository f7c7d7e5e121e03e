"""The 16-bit matrix-core attention by itself (include/soar_hip.h soar_attention16, csrc/attention.hip kv_attn16_kernel).

1. Exact, no tolerance: inputs on which every operand, score, weight and sum is exact in bf16 and in f16, so the 16-bit kernel must give
   the float32 kernel's bits -- a wrong operand map, mask or tail cannot hide in a tolerance.
2. The rounding rule: with one key the result is v rounded to the type, bit for bit.
3. Determinism, independence of the batch, B = 0.
4. Real data against float64: ``e16`` is the distance of the restatement with the kernel's roundings (tests/unet_attn_half_ref.py) from
   plain float64, worst element over the float64 tensor's RMS, and the kernel must lie within ``4 e16`` of float64 -- the bar of every
   16-bit and float32 stage of the project (tests/test_unet_half_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import unet_attn_half_ref as A
import unet_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FACTOR = 4.0
TYPES = {"bf16": 1, "f16": 2}
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
B, HEADS = 2, 2
HDS = [20, 64, 80]


def rel(a, b):
    """worst element of a - b over b's RMS (b: float64)"""
    return float((a.double().cpu() - b.cpu()).abs().max() / b.cpu().pow(2).mean().sqrt())


def attention16(prec, q, k, v, k2=None, v2=None, w2=0.5, causal=False, scale=None):
    """soar_attention16 straight through the C interface, the output between two guard rows of NaN that must stay NaN"""
    from soar_amd import hip_lib
    from soar_amd.hip_lib import _stream, check
    Bq, Lq, Cw = q.shape
    buf = torch.full((Bq * Lq + 2, Cw), float("nan"), device=q.device)
    out = buf[1:-1].view(Bq, Lq, Cw)
    a = hip_lib.SoarUnetAttnArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(1), k.stride(1), v.stride(1), Cw
    a.B, a.Lq, a.Lk, a.heads, a.hd = Bq, Lq, k.shape[1], HEADS, Cw // HEADS
    a.scale, a.w2 = float(Cw // HEADS) ** -0.5 if scale is None else scale, w2
    if k2 is not None:
        a.k2, a.v2, a.ldk2, a.ldv2, a.Lk2 = k2.data_ptr(), v2.data_ptr(), k2.stride(1), v2.stride(1), k2.shape[1]
    check(hip_lib.lib().soar_attention16(C.byref(a), TYPES[prec], int(causal), _stream(q.device)), "soar_attention16")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), "a guard row was written"
    assert not bool(torch.isnan(out).any())
    return out


def attention32(q, k, v, causal=False, scale=None):
    """the float32 kernel: soar_unet_attention up to hd 64 without a mask, soar_clip_attention otherwise"""
    from soar_amd import clip, unet
    if not causal and q.shape[2] // HEADS <= 64:
        return unet.attention(q, k, v, HEADS, scale=scale)
    return clip.attention(q, k, v, HEADS, scale=scale, causal=causal)


# ---- 1. exact ---------------------------------------------------------------------------------------------------------------------------
def exact_inputs(Lq, Lk, hd, seed):
    """q = 8 onehot(c), k in {0, 16}, v integers in [-8, 8]: with scale 1 a score is 0 or 128, p exactly 1 or 0.  Channel 0 is zero in
    every key and query 0 of every head asks for it, so all its scores tie at 0."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, hd, (B, Lq, HEADS), generator=g)
    c[:, 0] = 0
    q = torch.zeros(B, Lq, HEADS, hd).scatter_(3, c[..., None], 8.0)
    k = 16.0 * (torch.rand(B, Lk, HEADS, hd, generator=g) < 0.25).float()
    k[..., 0] = 0
    v = torch.randint(-8, 9, (B, Lk, HEADS, hd), generator=g).float()
    return q.reshape(B, Lq, -1), k.reshape(B, Lk, -1), v.reshape(B, Lk, -1)


def selected_mean(q, k, v, causal):
    """float64: the mean of the v rows whose score is the row's largest (among the visible keys)"""
    Lq, Lk, hd = q.shape[1], k.shape[1], q.shape[2] // HEADS
    qh, kh, vh = (t.double().reshape(B, -1, HEADS, hd).permute(0, 2, 1, 3) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2)
    assert set(s.unique().tolist()) <= {0.0, 128.0}
    if causal:
        s = s.masked_fill(torch.ones(Lq, Lk, dtype=torch.bool).triu(1), float("-inf"))
    sel = (s == s.amax(dim=-1, keepdim=True)).double()
    return ((sel @ vh) / sel.sum(dim=-1, keepdim=True)).permute(0, 2, 1, 3).reshape(B, Lq, -1)


def sources(q, k, v, packed):
    """on the device: three tensors of their own, or (Lq = Lk) slices of one row of pitch 3 C"""
    if not packed:
        return q.to(DEV), k.to(DEV), v.to(DEV)
    Cw = q.shape[2]
    rows = torch.cat([q, k, v], dim=2).to(DEV)
    return rows[..., :Cw], rows[..., Cw:2 * Cw], rows[..., 2 * Cw:]


def check_exact(got, want32, mean64, scale64):
    assert torch.equal(got, want32), f"{int((got != want32).sum())} of {got.numel()} elements differ from the float32 kernel"
    # the oracle itself: sum (1 / l) rounds twice, a second set adds its own two and the sum's: within 2^-22 of the terms' magnitudes
    assert bool(((got.double().cpu() - mean64).abs() <= 2.0 ** -22 * scale64).all())


SHAPES = [(1, 1), (33, 31), (129, 33), (135, 135), (128, 93)]


@pytest.mark.parametrize("prec", list(TYPES))
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("Lq,Lk", SHAPES)
def test_exact_one_key_set(Lq, Lk, hd, prec):
    q, k, v = exact_inputs(Lq, Lk, hd, 100 * Lq + Lk + hd)
    mean = selected_mean(q, k, v, False)
    for packed in ([False, True] if Lq == Lk else [False]):
        qd, kd, vd = sources(q, k, v, packed)
        check_exact(attention16(prec, qd, kd, vd, scale=1.0), attention32(qd, kd, vd, scale=1.0), mean, mean.abs())


@pytest.mark.parametrize("prec", list(TYPES))
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("Lk2", [16, 35])
def test_exact_second_key_set(Lk2, hd, prec):
    from soar_amd import unet
    Lq, Lk = 129, 33
    q, k, v = exact_inputs(Lq, Lk, hd, 7 + Lk2 + hd)
    _, k2, v2 = exact_inputs(Lq, Lk2, hd, 11 + Lk2 + hd)
    m1, m2 = selected_mean(q, k, v, False), selected_mean(q, k2, v2, False)
    qd, kd, vd = sources(q, k, v, False)
    k2d, v2d = k2.to(DEV), v2.to(DEV)
    got = attention16(prec, qd, kd, vd, k2d, v2d, w2=0.5, scale=1.0)
    # 1 x + 0.5 y is exact up to the sum's rounding, fused or not: the float32 kernel's two results combined give the launch's bits
    want = attention32(qd, kd, vd, scale=1.0) + 0.5 * attention32(qd, k2d, v2d, scale=1.0)
    check_exact(got, want, m1 + 0.5 * m2, m1.abs() + 0.5 * m2.abs())
    if hd <= 64:
        assert torch.equal(got, unet.attention(qd, kd, vd, HEADS, scale=1.0, k2=k2d, v2=v2d, w2=0.5))


@pytest.mark.parametrize("prec", list(TYPES))
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("L", [77, 135])
def test_exact_causal(L, hd, prec):
    """135: two query tiles, the first of which stops after key tile 3 and the second after tile 4"""
    q, k, v = exact_inputs(L, L, hd, 3 * L + hd)
    mean = selected_mean(q, k, v, True)
    for packed in (False, True):
        qd, kd, vd = sources(q, k, v, packed)
        check_exact(attention16(prec, qd, kd, vd, causal=True, scale=1.0), attention32(qd, kd, vd, causal=True, scale=1.0), mean, mean.abs())


# ---- 2. the rounding rule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(TYPES))
@pytest.mark.parametrize("hd", HDS)
def test_one_key_gives_v_rounded_to_the_type(hd, prec):
    """ties (the bits below the type's last one are 100..0) over even and odd last bits, their two neighbours, both signs"""
    drop = 16 if prec == "bf16" else 13                         # float32 mantissa bits the type does not keep
    Cw, Lq = HEADS * hd, 33
    n = B * Cw
    i = np.arange(n, dtype=np.uint32)
    keep = np.uint32(0x3F800000) + (((i * 37) % 1024) << 13 if prec == "f16" else ((i * 5) % 128) << 16)      # 1.0 .. 2.0, every kept last bit
    half = np.uint32(1 << (drop - 1))
    tail = np.stack([half, half + 1, half - 1])[i % 3]
    bits = (keep | tail | ((i // 3 % 2) << 31)).astype(np.uint32)
    v = torch.from_numpy(bits.view(np.float32).copy()).reshape(B, 1, Cw)
    want = v.to(DTYPES[prec]).float()
    assert int((want != v).sum()) == v.numel() and int((want.abs() > v.abs()).sum()) > n // 4 and int((want.abs() < v.abs()).sum()) > n // 4
    g = torch.Generator().manual_seed(hd)
    q, k = torch.randn(B, Lq, Cw, generator=g), torch.randn(B, 1, Cw, generator=g)
    got = attention16(prec, q.to(DEV), k.to(DEV), v.to(DEV))
    assert torch.equal(got.cpu(), want.expand(B, Lq, Cw))


# ---- 3. determinism and independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(TYPES))
@pytest.mark.parametrize("hd", HDS)
def test_runs_and_batch_elements_are_bit_equal(hd, prec):
    from soar_amd import hip_lib, unet
    Cw, Lq, Lk, Lk2 = HEADS * hd, 135, 93, 16
    g = torch.Generator().manual_seed(5 + hd)
    q, k, v = (torch.randn(B, L, Cw, generator=g).to(DEV) for L in (Lq, Lk, Lk))
    k2, v2 = (torch.randn(B, Lk2, Cw, generator=g).to(DEV) for _ in range(2))
    both = attention16(prec, q, k, v, k2, v2)
    assert torch.equal(both, attention16(prec, q, k, v, k2, v2))
    for b in range(B):
        one = attention16(prec, q[b:b + 1], k[b:b + 1], v[b:b + 1], k2[b:b + 1], v2[b:b + 1])
        assert torch.equal(one[0], both[b]), b
    if hd <= 64:
        assert torch.equal(both, unet.attention(q, k, v, HEADS, k2=k2, v2=v2, w2=0.5, precision=prec))
    # B = 0: nothing is launched, nothing written
    canary = torch.full((4, Cw), 3.0, device=DEV)
    a = hip_lib.SoarUnetAttnArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), canary.data_ptr()
    a.ldq = a.ldk = a.ldv = a.ldo = Cw
    a.B, a.Lq, a.Lk, a.heads, a.hd, a.scale = 0, 2, Lk, HEADS, hd, 1.0
    assert hip_lib.lib().soar_attention16(C.byref(a), TYPES[prec], 0, None) == 0
    torch.cuda.synchronize()
    assert bool((canary == 3.0).all())
    assert unet.attention(q[:0], k[:0], v[:0], HEADS, precision=prec).shape == (0, Lq, Cw)


# ---- 4. real data -------------------------------------------------------------------------------------------------------------------------
REAL = [(129, 33, 0, False), (135, 135, 0, False), (135, 135, 0, True), (128, 93, 35, False)]
_ratios = {}


@pytest.mark.parametrize("prec", list(TYPES))
@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("peak", [1.0, 4.0])
@pytest.mark.parametrize("Lq,Lk,Lk2,causal", REAL)
def test_real_data_within_4_e16_of_float64(Lq, Lk, Lk2, causal, peak, hd, prec):
    from soar_amd import clip
    Cw = HEADS * hd
    g = torch.Generator().manual_seed(1000 * Lq + Lk + hd)
    q = torch.randn(B, Lq, Cw, generator=g) * peak
    k, v = torch.randn(B, Lk, Cw, generator=g), torch.randn(B, Lk, Cw, generator=g)
    mask = torch.ones(Lq, Lk, dtype=torch.bool).triu(1) if causal else None

    def plain(dt, kk, vv):
        """float64 / float32 without any rounding (tests/unet_ref.py's attention, with the mask)"""
        qh, kh, vh = (t.to(dt).reshape(B, -1, HEADS, hd).permute(0, 2, 1, 3) for t in (q, kk, vv))
        s = qh @ kh.transpose(-1, -2) * hd ** -0.5
        if mask is not None:
            s = s.masked_fill(mask, float("-inf"))
        return (torch.softmax(s, dim=-1) @ vh).permute(0, 2, 1, 3).reshape(B, Lq, Cw)

    r64, r32, r16 = plain(torch.float64, k, v), plain(torch.float32, k, v), A.attention16(q, k, v, HEADS, causal=causal, precision=prec)
    if not causal:
        assert rel(R.attention(q.double(), k.double(), v.double(), HEADS), r64) < 1e-12
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    extra = ()
    if Lk2:
        k2, v2 = torch.randn(B, Lk2, Cw, generator=g), torch.randn(B, Lk2, Cw, generator=g)
        r64, r32 = r64 + 0.5 * plain(torch.float64, k2, v2), r32 + 0.5 * plain(torch.float32, k2, v2)
        r16 = r16 + 0.5 * A.attention16(q, k2, v2, HEADS, precision=prec)
        extra = (k2.to(DEV), v2.to(DEV))
    got = attention16(prec, qd, kd, vd, *extra, causal=causal)
    e16, err = rel(r16, r64), rel(got, r64)
    name = f"attention16 {prec} hd={hd} Lq={Lq} Lk={Lk} Lk2={Lk2} causal={causal} peak={peak}"
    _ratios[name] = err / e16
    print(f"{name}: err {err:.3g}  e16 {e16:.3g}  ratio {err / e16:.2f}  (largest so far {max(_ratios.values()):.2f})")
    assert e16 > 0 and err <= FACTOR * e16, f"{name}: {err:.3g} from float64, rounded restatement {e16:.3g}: ratio {err / e16:.2f} > {FACTOR}"
    # the harness: the float32 kernel on the same inputs still meets its own bar (tests/test_unet_gpu.py, tests/test_clip_gpu.py)
    f32 = attention32(qd, kd, vd, causal=causal)
    if Lk2:
        f32 = f32 + 0.5 * clip.attention(qd, *extra, HEADS)
    e32, err32 = rel(r32, r64), rel(f32, r64)
    print(f"    float32 kernel: err {err32:.3g}  e32 {e32:.3g}  ratio {err32 / e32:.2f}")
    assert err32 <= FACTOR * e32
    assert err32 < err                                           # ... and the 16-bit path is another
