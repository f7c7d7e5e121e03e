"""The 16-bit form of the shared implicit-GEMM convolution without a GPU (csrc/conv_gemm.hip, csrc/unet.hip): through
soar_selftest_conv_gemm16 with a NULL stream the launcher refuses, before it launches anything, what the 16-bit kernel cannot run --
and still what the float32 kernel cannot; the UNet's packed layout shrinks with a 16-bit precision; the Python argument is checked."""
import ctypes as C
import math
from dataclasses import replace

import pytest

import conv_gemm_ref as ref
import unet_ref as R


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


X, W_, B, R_, Y = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # addresses nothing reads: every call below stops at a check


def _desc(d, **kw):
    """d over unguarded layouts at the fake addresses"""
    d = replace(d, ph=[replace(t) for t in d.ph], **kw)
    d.ldx, d.xim, d.ldy, d.yim = d.Cin, d.Hin * d.Win, d.Cout, d.Hout * d.Wout
    off = 0
    for t in d.ph:
        t.ldw, t.w_off = t.ntaps * d.Cin, off
        off += d.Cout * t.ldw
    return d


def _call(lib, a, wtype):
    from soar_amd import hip_lib
    tile = C.c_int32(-1)
    rc = lib.soar_selftest_conv_gemm16(C.byref(a), wtype, C.byref(tile), None)
    return rc, hip_lib.last_error(), tile.value


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _tab(p, **kw):
    def f(a):
        for k, v in kw.items():
            setattr(a.ph[p], k, v)
    return f


NEW = {
    "w off 16 bytes by 8": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, w=W_ + 8), "tap table 0: w must be 16-byte aligned"),
    "w off 16 bytes by 2": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(2, w=W_ + 2), "tap table 2: w must be 16-byte aligned"),
    "ldw=76": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, ldw=76), "ldw must be a multiple of 8: the loads are 8 elements (ldw=76"),
    "ldw=76 of a later table": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(3, ldw=76), "tap table 3: with 16-bit weights ldw"),
    "wbat=580": (ref.matmul(2, 4, 8, 8), _set(wbat=580), "wbat must be a multiple of 8: the loads are 8 elements (wbat=580"),
}
# a choice of tests/test_conv_gemm_cpu.py's: what the launcher refused before it knew of wtype
OLD = {
    "Cin=12": (ref.conv3x3(2, 4, 4, 8, 8), _set(Cin=12), "Cin a multiple of 8"),
    "nph=5": (ref.conv3x3(2, 4, 4, 8, 8), _set(nph=5), "1 .. 4 tap tables"),
    "wbat without per_image": (ref.conv3x3(2, 4, 4, 8, 8), _set(wbat=1024), "B per image only with tiles per image"),
    "rows": (ref.conv1x1(2, 1 << 15, 1 << 15, 8, 8), _set(), "at most 2^30 rows"),
    "dil=3": (ref.conv3x3(2, 4, 4, 8, 8), _set(dil=3), "dil must be 1, or 2"),
    "dil=2 reflect": (ref.conv3x3_reflect(2, 4, 4, 8, 8), _set(dil=2), "dil must be 1, or 2 with zero padding"),
    "stride=0": (ref.conv3x3(2, 4, 4, 8, 8), _set(stride=0), "stride=0"),
    "ntaps=10": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, ntaps=10), "tap table 0: ntaps must be 1 .. 9 (got 10)"),
    "px=2, os=2": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(1, px=2), "tap table 1: py and px"),
    "reflect, one row": (ref.conv3x3_reflect(2, 1, 4, 8, 8), _set(), "mirrors once: rows -1 .. 1 of a 1-row input"),
    "x NULL": (ref.conv3x3(2, 4, 4, 8, 8), _set(x=None), "NULL x"),
    "w NULL": (ref.conv_transpose_phases(2, 4, 4, 8, 8), _tab(1, w=None), "tap table 1: NULL w"),
    "x off 16 bytes": (ref.conv3x3(2, 4, 4, 8, 8), _set(x=X + 4), "x must be 16-byte aligned"),
    "ldx=10": (ref.conv3x3(2, 4, 4, 8, 8), _set(ldx=10), "ldx=10"),
    "wbat=6": (ref.matmul(2, 4, 8, 8), _set(wbat=6), "wbat=6"),
    "ldw=74": (ref.conv3x3(2, 4, 4, 8, 8), _tab(0, ldw=74), "ldw=74"),
}


@pytest.mark.parametrize("wtype", [1, 2])
@pytest.mark.parametrize("name", list(NEW) + list(OLD))
def test_launcher_refuses(lib, name, wtype):
    d, mutate, telling = (NEW[name] if name in NEW else OLD[name])
    a = ref.c_args(_desc(d), X, W_, B, R_, Y)
    mutate(a)
    rc, err, _ = _call(lib, a, wtype)
    assert rc != 0 and err.startswith("conv_gemm:") and telling in err, err
    # ... and the same descriptor without rows is nothing to do, whatever else it says
    a.N = 0
    assert _call(lib, a, wtype)[0] == 0


@pytest.mark.parametrize("wtype", [0, 3, -1, 256])
def test_wtype_outside_1_to_2_is_refused(lib, wtype):
    a = ref.c_args(_desc(ref.conv3x3(2, 4, 4, 8, 8)), X, W_, B, R_, Y)
    rc, err, _ = _call(lib, a, wtype)
    assert rc != 0 and "wtype must be" in err and f"got {wtype}" in err, err


def test_the_new_refusals_are_the_16_bit_paths_alone(lib):
    """ldw = 76 and wbat = 580 are multiples of 4: the float32 entry point does not refuse them (it would launch: no rows here)"""
    from soar_amd import hip_lib
    for name in ("ldw=76", "wbat=580"):
        d, mutate, _ = NEW[name]
        a = ref.c_args(_desc(d), X, W_, B, R_, Y)
        mutate(a)
        a.N = 0
        tile = C.c_int32(0)
        assert lib.soar_selftest_conv_gemm(C.byref(a), C.byref(tile), None) == 0
    tile = C.c_int32(0)
    assert lib.soar_selftest_conv_gemm16(None, 1, C.byref(tile), None) != 0 and "NULL args" in hip_lib.last_error()
    a = ref.c_args(_desc(ref.conv3x3(2, 4, 4, 8, 8)), X, W_, None, None, Y)
    assert lib.soar_selftest_conv_gemm16(C.byref(a), 1, None, None) != 0 and "NULL tile_out" in hip_lib.last_error()
    assert lib.soar_selftest_conv_gemm_act(C.byref(a), 1, 3, C.byref(tile), None) != 0 and "act must be" in hip_lib.last_error()
    # the packer's entry: arguments only
    assert lib.soar_selftest_conv_pack16(None, Y, 4, 8, 8, 9, 1, None) != 0 and "soar_selftest_conv_pack16" in hip_lib.last_error()
    assert lib.soar_selftest_conv_pack16(X, None, 4, 8, 8, 9, 1, None) != 0
    assert lib.soar_selftest_conv_pack16(X, Y, 4, 8, 4, 9, 1, None) != 0 and "Cinp=4" in hip_lib.last_error()
    assert lib.soar_selftest_conv_pack16(X, Y, 4, 8, 8, 9, 0, None) != 0 and "wtype must be" in hip_lib.last_error()
    assert lib.soar_selftest_conv_pack16(X, Y, 4, 8, 8, 9, 3, None) != 0 and "wtype must be" in hip_lib.last_error()


def _config(lib, cfg, precision):
    from soar_amd import hip_lib
    c = hip_lib.SoarUnetConfig()
    c.in_channels, c.out_channels, c.model_channels = cfg["in_channels"], cfg["out_channels"], cfg["model_channels"]
    c.levels, c.num_res_blocks = len(cfg["channel_mult"]), cfg["num_res_blocks"]
    for l, (m, a) in enumerate(zip(cfg["channel_mult"], cfg["attention"])):
        c.channel_mult[l], c.attention[l] = m, int(a)
    c.context_dim, c.camera_dim, c.with_ip = cfg["context_dim"], cfg["camera_dim"], int(cfg["with_ip"])
    c.head_channels, c.n_view, c.precision = cfg["num_head_channels"], cfg["n_view"], precision
    return c


@pytest.mark.parametrize("cfg", [R.CONFIG_A, R.CONFIG_B], ids=["A", "B"])
def test_unet_weights_bytes_shrink_with_a_16_bit_precision(lib, cfg):
    from soar_amd import hip_lib
    assert hip_lib.SoarUnetConfig().precision == 0
    got = {}
    for precision in (0, 1, 2):
        c = _config(lib, cfg, precision)
        nb, cnt, nf = C.c_size_t(0), C.c_int32(0), C.c_size_t(0)
        assert lib.soar_unet_weights_bytes(C.byref(c), C.byref(nb), C.byref(cnt), C.byref(nf)) == 0, hip_lib.last_error()
        got[precision] = (nb.value, cnt.value, nf.value)
    shapes = R.state_dict_shapes(cfg)
    floats = sum(math.prod(s) for s in shapes.values())
    assert got[0][1:] == got[1][1:] == got[2][1:] == (len(shapes), floats)
    assert got[1][0] == got[2][0] < got[0][0]
    # the matrices are all but a few per cent of the weights: a 16-bit layout is little more than half the float32 one
    assert got[1][0] < 0.6 * got[0][0]
    c = _config(lib, cfg, 3)
    nb = C.c_size_t(0)
    assert lib.soar_unet_weights_bytes(C.byref(c), C.byref(nb), None, None) != 0 and "precision=3" in hip_lib.last_error()


def test_the_module_checks_its_precision(lib):
    from soar_amd import unet
    sd = R.tiny_state_dict(R.CONFIG_B, 0)
    kw = dict(num_head_channels=R.CONFIG_B["num_head_channels"], n_view=1)
    with pytest.raises(ValueError, match="'f32', 'bf16', 'f16'"):
        unet.MultiviewUNet(sd, precision="fp8", **kw)
    sizes = {}
    for p in ("f32", "bf16", "f16"):
        net = unet.MultiviewUNet(sd, precision=p, **kw)
        assert net.precision == p and net._c.precision == unet.PRECISIONS[p] and net.weights.dtype.is_floating_point
        sizes[p] = net._packed_bytes
    assert unet.MultiviewUNet(sd, **kw)._c.precision == 0
    assert sizes["bf16"] == sizes["f16"] < sizes["f32"]
