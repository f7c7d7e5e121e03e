"""CPU tests of the VAE encoder's 16-bit precisions (csrc/vae.hip: soar_vae_*16; soar_amd/sds.py: LatentEncoder(precision=...);
DESIGN.md 9zd): the new entry points' refusals through the C ABI (with a NULL stream: nothing is launched), the packed
sizes per precision, the Python argument, and the conditions under which the 16-bit restatement (tests/vae_half_ref.py) is a fair
yardstick at f16 -- at the GPU suite's inputs hardly any gradient operand lies below f16's normal range once the backward runs on
2^10 g, and none comes near its largest number."""
import ctypes as C

import pytest
import torch

import vae_half_ref as HR
import vae_ref as R
from soar_amd import sds

RAW_FLOATS = 34163664
# the restatement's own conditions at f16, per product (the issue's caps; measured: tests' docstrings and DESIGN.md 9zd)
SHARE_CAP = 1e-3
LARGEST_CAP = 2.0 ** 12


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def _b_operand_elements():
    """elements of the tensors that are B operands of a 16-bit product: every convolution weight but conv_in, conv_out, quant_conv"""
    return sum(int(torch.tensor(s).prod()) for k, s in R.keys(128)
               if len(s) == 4 and not any(k.startswith(p + ".") for p in HR.FLOAT32_KEYS))


def test_packed_sizes_per_precision(lib):
    from soar_amd import hip_lib
    n32, n = C.c_size_t(0), C.c_size_t(0)
    assert lib.soar_vae_weights_bytes(C.byref(n32)) == 0
    assert lib.soar_vae_weights_bytes16(0, C.byref(n)) == 0 and n.value == n32.value
    sizes = {}
    for p in (1, 2):
        assert lib.soar_vae_weights_bytes16(p, C.byref(n)) == 0 and n.value % 256 == 0
        sizes[p] = n.value
    assert sizes[1] == sizes[2]
    # each B operand is packed twice (forward and data-gradient form); every one has a multiple of 128 elements, so neither form
    # is padded at either width: the 16-bit tensors take exactly half, everything else (the raw copy, the biases) is unchanged
    nb = _b_operand_elements()
    assert nb == RAW_FLOATS - 128 * 27 - 8 * 512 * 9 - 64 - sum(int(torch.tensor(s).prod()) for _, s in R.keys(128) if len(s) == 1)
    assert n32.value - sizes[1] == 2 * nb * 2
    assert n32.value - 2 * nb * 4 == sizes[1] - 2 * nb * 2
    for p in (-1, 3, 16):
        assert lib.soar_vae_weights_bytes16(p, C.byref(n)) != 0 and "precision must be 0 (f32), 1 (bf16) or 2 (f16)" in hip_lib.last_error()
    assert lib.soar_vae_weights_bytes16(1, None) != 0 and "NULL" in hip_lib.last_error()


def test_new_entries_refuse_bad_arguments_without_touching_the_gpu(lib):
    from soar_amd import hip_lib
    a = hip_lib.SoarVaeArgs()
    a.N, a.H, a.W, a.image_size = 2, 50, 90, 72
    a.weights = 0x100000
    a.x = a.eps = a.latents = a.g_latents = a.g_x = 0x100000
    n = C.c_size_t(0)
    assert lib.soar_vae_workspace_bytes(2, 50, 90, 72, C.byref(n)) == 0
    # a precision outside 0 .. 2: refused by name before anything else is looked at, a complete call included
    for entry, name in ((lib.soar_vae_forward16, "soar_vae_forward16"), (lib.soar_vae_backward16, "soar_vae_backward16")):
        for p in (-1, 3, 7):
            assert entry(C.byref(a), p, 0x100000, n.value, None) != 0
            assert f"{name}: precision must be 0 (f32), 1 (bf16) or 2 (f16) (got {p})" in hip_lib.last_error()
        assert entry(None, 1, None, 0, None) != 0 and "NULL args" in hip_lib.last_error()
        # the workspace contract is the float32 entries': one byte short is refused at every precision
        for p in (0, 1, 2):
            assert entry(C.byref(a), p, 0x100000, n.value - 1, None) != 0
            assert f"workspace of {n.value - 1} bytes, need {n.value} (soar_vae_workspace_bytes)" in hip_lib.last_error()
    a.x = None
    assert lib.soar_vae_forward16(C.byref(a), 1, 0x100000, n.value, None) != 0 and "soar_vae_forward16: NULL x" in hip_lib.last_error()
    a.g_x = None
    assert lib.soar_vae_backward16(C.byref(a), 2, 0x100000, n.value, None) != 0 and "g_latents" in hip_lib.last_error()
    a.N = 0
    assert lib.soar_vae_forward16(C.byref(a), 1, None, 0, None) == 0 and lib.soar_vae_backward16(C.byref(a), 2, None, 0, None) == 0
    # the packer: the precision, the raw size, then a packed buffer of exactly the precision's size
    size = {}
    for p in (0, 1, 2):
        assert lib.soar_vae_weights_bytes16(p, C.byref(n)) == 0
        size[p] = n.value
    assert lib.soar_vae_pack_weights16(0x100000, RAW_FLOATS, 0x100000, size[1], 3, None) != 0 and "precision must be" in hip_lib.last_error()
    assert lib.soar_vae_pack_weights16(0x100000, 5, 0x100000, size[1], 1, None) != 0 and "floats" in hip_lib.last_error()
    assert lib.soar_vae_pack_weights16(None, RAW_FLOATS, 0x100000, size[1], 1, None) != 0 and "NULL" in hip_lib.last_error()
    for p, wrong in ((1, size[0]), (2, size[0]), (0, size[1]), (1, size[1] - 1), (2, size[2] + 256), (1, 0)):
        assert lib.soar_vae_pack_weights16(0x100000, RAW_FLOATS, 0x100000, wrong, p, None) != 0
        assert f"packed must be {size[p]} bytes at precision {p}" in hip_lib.last_error(), (p, wrong)
    assert lib.soar_vae_pack_weights16(0x100000, RAW_FLOATS, 0x100010, size[1], 1, None) != 0 and "256-byte aligned" in hip_lib.last_error()


def test_the_data_gradient_packer_refuses_bad_arguments(lib):
    from soar_amd import hip_lib
    f = lib.soar_selftest_conv_pack16_bwd
    assert f(None, 0x100000, 16, 16, 9, 16, 1, None) != 0 and "soar_selftest_conv_pack16_bwd" in hip_lib.last_error()
    assert f(0x100000, None, 16, 16, 9, 16, 1, None) != 0
    assert f(0x100000, 0x100000, 24, 16, 9, 16, 1, None) != 0 and "ldb >= Cout" in hip_lib.last_error()      # ldb < Cout
    assert f(0x100000, 0x100000, 16, 16, 9, 20, 1, None) != 0 and "multiple of 8" in hip_lib.last_error()
    assert f(0x100000, 0x100000, 16, 0, 9, 16, 1, None) != 0
    for wt in (0, 3):
        assert f(0x100000, 0x100000, 16, 16, 9, 16, wt, None) != 0 and "wtype must be 1 (bf16) or 2 (f16)" in hip_lib.last_error()


def test_the_precision_argument():
    sd = R.random_weights(2)
    m = sds.LatentEncoder(sd)
    assert m.precision == "f32"
    for p in ("f32", "bf16", "f16"):
        mp = sds.LatentEncoder(sd, precision=p)
        assert mp.precision == p
        assert mp.weights.dtype == torch.float32 and torch.equal(mp.weights, m.weights)
        assert mp.scale_factor == m.scale_factor
    assert sds.LatentEncoder(sd, 0.5, "bf16").scale_factor == 0.5
    for bad in ("fp16", "half", "F16", "", None, 1, torch.bfloat16):
        with pytest.raises(ValueError, match="'f32', 'bf16', 'f16'"):
            sds.LatentEncoder(sd, precision=bad)
    # still HIP only, at every precision
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sds.LatentEncoder(sd, precision="f16")(torch.zeros(1, 3, 64, 64), 64)


def _inputs(N, H, W, S, seed):
    """tests/test_sds_half_gpu.py's inputs, in float64 on the CPU"""
    x = R.images(N, H, W, seed)
    g = torch.Generator().manual_seed(seed + 1)
    eps = torch.randn(N, 4, S // 8, S // 8, generator=g)
    gw = torch.randn(N, 4, S // 8, S // 8, generator=g)
    return x.double(), eps.double(), gw.double()


@pytest.fixture(scope="module")
def weights64():
    return R.cast(R.random_weights(0), torch.float64)


def test_the_swap_is_undone_and_leaves_the_float32_convolutions_alone(weights64):
    plain = R._conv
    x, eps, gw = _inputs(1, 8, 8, 8, seed=8)
    with HR.half(torch.bfloat16):
        assert R._conv is not plain
        # conv_in is not rounded: its output is the plain one's bits
        a = R._conv(x, weights64, "encoder.conv_in", padding=1)
    assert R._conv is plain
    assert torch.equal(a, R._conv(x, weights64, "encoder.conv_in", padding=1))
    with pytest.raises(ZeroDivisionError):
        with HR.half(torch.float16):
            1 / 0
    assert R._conv is plain


# the GPU suite's table (test_sds_half_gpu.py: CASES) but 50 x 90 -> 72, which takes six seconds here: that suite computes the
# restatement on the device anyway and holds it to the same caps there, at every case
@pytest.mark.parametrize("N,H,W,S", [(2, 8, 8, 8), (3, 30, 22, 24), (1, 8, 200, 40)])
def test_f16_restatement_conditions_at_the_gpu_suites_inputs(weights64, N, H, W, S):
    """Measured here, per product, worst over the products: share of non-zero gradient operands below 2^-14 and the largest operand
    with the 2^10 -- 8 x 8 -> 8: 6.1e-4, 57; 30 x 22 -> 24: 1.1e-4, 74; 8 x 200 -> 40: 9.8e-5, 81; 50 x 90 -> 72 (run once by hand):
    1.2e-4, 107.  e16 there: latents 3.3e-4 ... 6.1e-4, gradient 1.7e-3 ... 2.0e-3."""
    x, eps, gw = _inputs(N, H, W, S, seed=H)
    st = HR.Stats()
    l16, g16, _, _ = HR.latents_and_grad(x, weights64, S, eps, gw, torch.float16, st)
    l64, g64, _, _ = HR.latents_and_grad(x, weights64, S, eps, gw)
    # 32 convolutions, 29 of them 16-bit products
    assert len(st.per_product) == 29 and not any(k in st.per_product for k in HR.FLOAT32_KEYS)
    e_lat = float((l16 - l64).norm() / l64.norm())
    e_g = float((g16 - g64).norm() / g64.norm())
    print(f"\n{N}x{H}x{W}->{S} f16: worst share below 2^-14 {st.worst_share():.2e}, largest operand {st.largest():.1f}, "
          f"e16 latents {e_lat:.2e} gradient {e_g:.2e}")
    assert st.worst_share() <= SHARE_CAP, st.per_product
    assert st.largest() <= LARGEST_CAP, st.per_product
    # rounding moved the result, and by about the type's precision: the restatement is neither the plain chain nor broken
    assert 1e-5 < e_lat < 5e-3 and 1e-4 < e_g < 2e-2, (e_lat, e_g)
