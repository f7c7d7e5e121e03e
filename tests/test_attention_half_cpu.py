"""CPU tests of the 16-bit attention's interface (include/soar_hip.h soar_attention16, SoarUnetConfig / SoarClipConfig /
SoarResamplerConfig ``precision`` and ``attn_precision``): every refusal comes before any launch, so it is asked for
with a NULL stream and made-up (aligned, never read) pointers; the packed sizes are worked out here from the key lists.  No kernel is
launched."""
import ctypes as C

import pytest
import torch

import clip_ref as CR
import unet_ref as UR

PTR = 0x10000                                                    # 16-byte aligned, never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def L():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def err():
    from soar_amd import hip_lib
    return hip_lib.last_error()


def attn_args(B=2, Lq=8, Lk=8, heads=2, hd=16, **kw):
    from soar_amd import hip_lib
    a = hip_lib.SoarUnetAttnArgs()
    Cw = heads * hd
    a.q, a.k, a.v, a.out = PTR, PTR, PTR, PTR
    a.ldq = a.ldk = a.ldv = a.ldo = Cw
    a.B, a.Lq, a.Lk, a.heads, a.hd, a.scale, a.w2 = B, Lq, Lk, heads, hd, 1.0, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_entry_point_is_declared_and_bound(L):
    import os
    from soar_amd import hip_lib
    header = open(os.path.join(os.path.dirname(hip_lib.__file__), "..", "include", "soar_hip.h")).read()
    assert "int soar_attention16(const SoarUnetAttnArgs *args, int32_t type, int32_t causal, void *stream);" in header
    assert "int32_t attn_precision;" in header and "int32_t precision, attn_precision;" in header
    assert L.soar_attention16.argtypes is not None


@pytest.mark.parametrize("type_", [0, 3, -1])
def test_a_type_outside_1_2_is_refused(L, type_):
    assert L.soar_attention16(C.byref(attn_args()), type_, 0, None) == 1
    assert "1 (bf16) or 2 (f16)" in err() and f"got {type_}" in err()


@pytest.mark.parametrize("type_", [1, 2])
def test_refusals_before_any_launch(L, type_):
    call = lambda a, causal=0: L.soar_attention16(C.byref(a), type_, causal, None)
    assert L.soar_attention16(None, type_, 0, None) == 1 and "NULL args" in err()
    assert call(attn_args(hd=100)) == 1 and "hd=100" in err() and "up to 96" in err()
    assert call(attn_args(hd=6)) == 1 and "hd=6" in err()
    assert call(attn_args(ldk=2 * 16 - 4)) == 1 and "row pitch of 28" in err()                  # below heads hd
    assert call(attn_args(ldv=2 * 16 + 2)) == 1 and "row pitch of 34" in err()                  # no multiple of 4
    assert call(attn_args(ldo=2 * 16 - 4)) == 1 and "row pitch" in err()
    assert call(attn_args(k=PTR + 4)) == 1 and "16-byte aligned" in err()
    assert call(attn_args(out=PTR + 8)) == 1 and "16-byte aligned" in err()
    assert call(attn_args(k2=PTR, Lk2=4, ldk2=32, ldv2=32)) == 1 and "second key set without its values" in err()
    assert call(attn_args(k2=PTR, v2=PTR, Lk2=0, ldk2=32, ldv2=32)) == 1 and "Lk2 = 0" in err()
    assert call(attn_args(k2=PTR, v2=PTR, Lk2=4, ldk2=32, ldv2=32), causal=1) == 1 and "causal mask needs one key set" in err()
    assert call(attn_args(Lq=8, Lk=9), causal=1) == 1 and "Lq = Lk" in err()
    assert call(attn_args(q=None)) == 1 and "NULL q" in err()
    assert call(attn_args(Lk=0)) == 1 and "bad sizes" in err()
    # nothing to do: no pointer is looked at
    assert call(attn_args(B=0, q=None, k=None, v=None, out=None)) == 0
    assert call(attn_args(B=0, hd=96, Lq=5, Lk=5), causal=1) == 0


def test_python_arguments_name_the_three_choices():
    from soar_amd import clip, unet
    z = torch.zeros(1, 4, 8)
    for fn in (unet.attention, clip.attention):
        with pytest.raises(ValueError, match="'f32', 'bf16', 'f16'"):
            fn(z, z, z, 1, precision="fp16")
        with pytest.raises(ValueError, match="'f32', 'bf16', 'f16'"):
            fn(z, z, z, 1, precision=None)
    cfg = UR.CONFIG_A
    kw = dict(num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"], ip_weight=cfg["ip_weight"], n_view=cfg["n_view"])
    sd = UR.tiny_state_dict(cfg, 0)
    with pytest.raises(ValueError, match="attention_precision must be one of 'f32', 'bf16', 'f16'"):
        unet.MultiviewUNet(sd, attention_precision="half", **kw)
    with pytest.raises(ValueError, match="precision must be one of 'f32', 'bf16', 'f16'"):
        unet.MultiviewUNet(sd, precision="half", **kw)
    net = unet.MultiviewUNet(sd, attention_precision="f16", **kw)
    assert net.attention_precision == "f16" and net.precision == "f32" and net._c.attn_precision == 2 and net._c.precision == 0
    text = CR.tiny_state_dict(CR.text_shapes(CR.TEXT_A), 0)
    vis = CR.tiny_state_dict(CR.vision_shapes(CR.VISION_A), 0)
    res = CR.tiny_state_dict(CR.resampler_shapes(CR.RESAMPLER_A), 0)
    for make in (lambda **k: clip.ClipTextEncoder(text, heads=2, **k), lambda **k: clip.ClipImageEncoder(vis, heads=2, **k),
                 lambda **k: clip.Resampler(res, dim_head=32, **k)):
        with pytest.raises(ValueError, match="attention_precision must be one of 'f32', 'bf16', 'f16'"):
            make(attention_precision="bfloat16")
        with pytest.raises(ValueError, match=" precision must be one of 'f32', 'bf16', 'f16'"):
            make(precision=16)
        m = make(precision="bf16", attention_precision="f16")
        assert (m.precision, m.attention_precision, m._c.precision, m._c.attn_precision) == ("bf16", "f16", 1, 2)
        assert m.weights.dtype == torch.float32


def sized(L, fn, c):
    nb, cnt, nf = C.c_size_t(0), C.c_int32(0), C.c_size_t(0)
    assert getattr(L, fn)(C.byref(c), C.byref(nb), C.byref(cnt), C.byref(nf)) == 0, err()
    return nb.value, cnt.value, nf.value


def test_unet_weights_do_not_depend_on_attn_precision_and_3_is_refused(L):
    from soar_amd import unet
    cfg = UR.CONFIG_A
    kw = dict(num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"], ip_weight=cfg["ip_weight"], n_view=cfg["n_view"])
    sd = UR.tiny_state_dict(cfg, 0)
    for prec in ("f32", "bf16"):
        sizes = set()
        for ap in (0, 1, 2):
            c = unet.MultiviewUNet(sd, precision=prec, **kw)._c
            c.attn_precision = ap
            sizes.add(sized(L, "soar_unet_weights_bytes", c))
        assert len(sizes) == 1
    c = unet.MultiviewUNet(sd, **kw)._c
    nb = C.c_size_t(0)
    c.attn_precision = 3
    assert L.soar_unet_weights_bytes(C.byref(c), C.byref(nb), None, None) == 1 and "attn_precision=3" in err()
    assert L.soar_unet_workspace_bytes(C.byref(c), 4, 8, 8, 7, 0, C.byref(nb)) == 1 and "attn_precision=3" in err()
    c.attn_precision, c.precision = 0, 3
    assert L.soar_unet_weights_bytes(C.byref(c), C.byref(nb), None, None) == 1 and "precision=3" in err()


# the tensors that are a product's B operand, by the packed order's names (soar_amd/clip.py tensor_names)
TOWER_MATS = ("conv1.weight", "attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")
RESAMPLER_MATS = ("proj_in.weight", "proj_out.weight", "to_q.weight", "to_kv.weight", "to_out.weight", "1.1.weight", "1.3.weight")


def expected_bytes(module, mats, half, padded=None):
    """the plan's rule: a tensor takes its floats (the patch rows padded), a B operand half of them at 16 bits, each start a multiple
    of 4 floats; the buffer a multiple of 256 bytes"""
    total = 0
    for name, n in zip(module.tensor_names, module._sizes):
        if padded and name == padded[0]:
            n = padded[1]
        if half and name.endswith(mats):
            n = (n + 1) // 2
        total += (n + 3) // 4 * 4
    return (total * 4 + 255) // 256 * 256


@pytest.mark.parametrize("which", ["text", "vision", "resampler"])
def test_clip_and_resampler_packed_sizes(L, which):
    from soar_amd import clip
    if which == "text":
        sd = CR.tiny_state_dict(CR.text_shapes(CR.TEXT_A), 0)
        make, fn, mats, padded = (lambda **k: clip.ClipTextEncoder(sd, heads=2, **k)), "soar_clip_weights_bytes", TOWER_MATS, None
    elif which == "vision":
        sd = CR.tiny_state_dict(CR.vision_shapes(CR.VISION_A), 0)
        make, fn, mats = (lambda **k: clip.ClipImageEncoder(sd, heads=2, **k)), "soar_clip_weights_bytes", TOWER_MATS
        v = CR.VISION_A
        padded = ("conv1.weight", v["width"] * ((3 * v["patch"] ** 2 + 7) // 8 * 8))            # 588 -> 592 a row
    else:
        sd = CR.tiny_state_dict(CR.resampler_shapes(CR.RESAMPLER_A), 0)
        make, fn, mats, padded = (lambda **k: clip.Resampler(sd, dim_head=32, **k)), "soar_resampler_weights_bytes", RESAMPLER_MATS, None
    m32 = make()
    assert sum(name.endswith(mats) for name in m32.tensor_names) >= 4
    b32, cnt, floats = sized(L, fn, m32._c)
    assert b32 == m32._packed_bytes == expected_bytes(m32, mats, False, padded)
    assert cnt == len(m32.tensor_names) and floats == sum(m32._sizes)
    for prec in ("bf16", "f16"):
        m = make(precision=prec)
        b16, cnt16, floats16 = sized(L, fn, m._c)
        assert b16 == m._packed_bytes == expected_bytes(m, mats, True, padded) < b32
        assert (cnt16, floats16) == (cnt, floats)
        for ap in (1, 2):                                        # the attention's type changes no size
            m._c.attn_precision = ap
            assert sized(L, fn, m._c) == (b16, cnt, floats)
    nb = C.c_size_t(0)
    c = make()._c
    c.precision = 3
    assert getattr(L, fn)(C.byref(c), C.byref(nb), None, None) == 1 and "precision = 3" in err() and "attn" not in err()
    c.precision, c.attn_precision = 0, 3
    assert getattr(L, fn)(C.byref(c), C.byref(nb), None, None) == 1 and "attn_precision = 3" in err()
    c.attn_precision = -1
    ws = "soar_clip_workspace_bytes" if which != "resampler" else "soar_resampler_workspace_bytes"
    assert getattr(L, ws)(C.byref(c), 1, 5 if which != "vision" else m32.cfg["tokens"], C.byref(nb)) == 1 and "attn_precision = -1" in err()
