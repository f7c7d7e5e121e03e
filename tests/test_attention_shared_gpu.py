"""The two tiled attention kernels of csrc/attention.hip run on one tile step: on a whole grid without
relative-position tables, SAM's grid attention and the key/value attention are the same function of the same numbers, so on one packed
``qkv [B][gh][gw][3 C]`` they must give equal values -- no tolerance.  (A value comparison: the sign of a zero does not count.)

5 x 7 is 35 keys: two key tiles, the second with 3 keys, and a partly filled query tile in both kernels.  9 x 15 is 135 keys: SAM's
kernel runs three query tiles of 64, the other two of 128, both with tails.  Head dimensions 20 (padded to 32 in LDS), 64 (exact) and
80 (padded to 96).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


@pytest.mark.parametrize("hd", [20, 64, 80])
@pytest.mark.parametrize("gh,gw", [(5, 7), (9, 15)])
def test_grid_attention_equals_key_value_attention(gh, gw, hd):
    from soar_amd import clip, hip_lib
    B, heads = 2, 2
    Cw = heads * hd
    qkv = torch.randn(B, gh, gw, 3 * Cw, generator=torch.Generator().manual_seed(gh * 1000 + gw * 10 + hd)).to(DEV)
    grid = torch.full((B, gh, gw, Cw), float("nan"), device=DEV)
    hip_lib.check(hip_lib.lib().soar_sam_attention(qkv.data_ptr(), None, None, None, grid.data_ptr(), B, gh, gw, heads, hd, 0, hd ** -0.5,
                                                   torch.cuda.current_stream().cuda_stream), "soar_sam_attention")
    rows = qkv.view(B, gh * gw, 3 * Cw)                                # q, k, v at offsets 0, C and 2 C of one row, pitch 3 C
    kv = clip.attention(rows[..., :Cw], rows[..., Cw:2 * Cw], rows[..., 2 * Cw:], heads, causal=False)
    torch.cuda.synchronize()
    assert torch.isfinite(grid).all()
    diff = float((grid.view(B, gh * gw, Cw) - kv).abs().max())
    print(f"\ngrid {gh}x{gw} hd {hd}: max |grid attention - key/value attention| = {diff:.3g}")
    assert torch.equal(grid.view(B, gh * gw, Cw), kv)
