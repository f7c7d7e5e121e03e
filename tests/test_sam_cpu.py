"""SAM without a GPU: the plain-torch restatement (tests/sam_ref.py) against an independent implementation, its resize against
Pillow, and the size inference of ``soar_amd.sam``."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import sam_ref

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
    return np.load(os.path.join(HERE, "golden", "sam_tiny.npz"))


def _rel(a, b):
    """worst element of a - b over b's RMS"""
    return float((a - b).abs().max() / b.pow(2).mean().sqrt())


def test_restatement_reproduces_the_fixture_in_float64():
    """tests/golden/sam_tiny.npz is transformers' SamModel in float64 at configuration A (tests/tools/make_sam_golden.py)."""
    z = _fixture()
    sd = {k[2:]: torch.from_numpy(z[k]).double() for k in z.files if k.startswith("w:")}
    assert set(sd) == set(sam_ref.state_dict_shapes(sam_ref.CONFIG_A))
    for i, n_points in ((0, 5), (1, 1)):
        frame, pts = z[f"frame{i}"], z[f"points{i}"]
        assert frame.dtype == np.uint8 and pts.shape == (n_points, 2)
        r = sam_ref.predict_logits(sd, sam_ref.CONFIG_A, frame, pts, np.ones(n_points), torch.float64)
        for name, key in (("emb", "emb"), ("low", "low"), ("iou", "iou")):
            want = torch.from_numpy(z[f"{key}{i}"])
            assert want.dtype == torch.float64 and want.shape == r[name].shape
            err = _rel(r[name], want)
            print(f"frame {i} {name}: {err:.3g}")
            assert err <= 1e-9


def test_restatement_matches_transformers_at_configuration_b():
    pytest.importorskip("transformers")
    spec = importlib.util.spec_from_file_location("make_sam_golden", os.path.join(HERE, "tools", "make_sam_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    cfg = sam_ref.CONFIG_B
    sd = sam_ref.tiny_state_dict(cfg, 1)
    model = mg.hf_model(cfg, sd)
    frames, pts = mg.frames_and_points()
    sd64 = {k: v.double() for k, v in sd.items()}
    emb, low, iou = mg.hf_run(model, cfg, frames[0], pts[0], np.ones(len(pts[0]), np.int64))
    r = sam_ref.predict_logits(sd64, cfg, frames[0], pts[0], np.ones(len(pts[0])), torch.float64)
    for name, want in (("emb", emb), ("low", low), ("iou", iou)):
        assert _rel(r[name], want) <= 1e-9, name


RESIZE_CASES, resize_case_image = sam_ref.RESIZE_CASES, sam_ref.resize_case_image


@pytest.mark.parametrize("hw,out", RESIZE_CASES)
def test_restated_resize_is_pillows_bilinear(hw, out):
    from PIL import Image
    assert sam_ref.resized_hw(hw[0], hw[1], 112) == out
    img = resize_case_image(hw)
    want = np.asarray(Image.fromarray(img).resize((out[1], out[0]), Image.BILINEAR))
    assert np.array_equal(sam_ref.resize_bilinear_u8(img, out[0], out[1]), want)


def test_resize_tables_of_the_library_agree_with_the_restatement():
    """soar_amd.jpeg builds the tables the device kernel reads: the triangle filter's equal the restatement's, and the default is
    still the bicubic one."""
    from soar_amd import jpeg
    for n_in, n_out in ((160, 112), (37, 83), (301, 112), (112, 112)):
        b, k, ks = jpeg.resize_tables(n_in, n_out, "bilinear")
        rb, rk = sam_ref.bilinear_tables(n_in, n_out)
        assert np.array_equal(b, rb) and np.array_equal(k, rk) and ks == rk.shape[1]
    for got, want in zip(jpeg.resize_tables(160, 112), jpeg.bicubic_tables(160, 112)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("cfg", [sam_ref.CONFIG_A, sam_ref.CONFIG_B], ids=["A", "B"])
def test_sizes_come_from_the_state_dict(cfg):
    from soar_amd import sam
    sd = sam_ref.tiny_state_dict(cfg, 0)
    got = sam.infer_config(sd)
    got["dec_heads"] = cfg["dec_heads"]               # no shape shows it: a constructor argument
    assert got == cfg
    assert [(k, tuple(s)) for k, s in sam.tensor_keys(cfg)] == [(k, tuple(sd[k].shape)) for k, _ in sam.tensor_keys(cfg)]
    assert {k for k, _ in sam.tensor_keys(cfg)} == set(sd) - {"prompt_encoder.point_embeddings.2.weight", "prompt_encoder.point_embeddings.3.weight"}


@pytest.mark.parametrize("key", ["image_encoder.blocks.2.attn.rel_pos_w", "mask_decoder.transformer.layers.1.norm3.bias",
                                 "prompt_encoder.not_a_point_embed.weight", "image_encoder.neck.2.weight"])
def test_a_missing_or_misshapen_key_is_named(key):
    from soar_amd import sam
    sd = sam_ref.tiny_state_dict(sam_ref.CONFIG_A, 0)
    less = {k: v for k, v in sd.items() if k != key}
    with pytest.raises(KeyError, match=key.replace(".", r"\.")):
        sam.SamSegmenter(less, decoder_heads=2)
    bad = dict(sd)
    bad[key] = torch.zeros(tuple(s + 1 for s in sd[key].shape))
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        sam.SamSegmenter(bad, decoder_heads=2)


def test_a_rel_pos_table_that_does_not_match_the_grid_is_refused():
    from soar_amd import sam
    sd = sam_ref.tiny_state_dict(sam_ref.CONFIG_A, 0)
    sd["image_encoder.blocks.1.attn.rel_pos_h"] = torch.zeros(11, 16)          # a 6-token axis: neither the grid's 7 nor the window's 3
    with pytest.raises(ValueError, match=r"blocks\.1\.attn\.rel_pos_h"):
        sam.SamSegmenter(sd, decoder_heads=2)


def test_sizing_calls_refuse_what_the_kernels_cannot_run():
    """soar_sam_weights_bytes / _workspace_bytes: host-side only, nothing is launched."""
    import ctypes as C
    from soar_amd import hip_lib, sam
    seg = sam.SamSegmenter(sam_ref.tiny_state_dict(sam_ref.CONFIG_A, 0), decoder_heads=2)
    assert seg.weights.numel() == sum(int(np.prod(s)) for _, s in sam.tensor_keys(sam_ref.CONFIG_A))
    L, nb, cnt = hip_lib.lib(), C.c_size_t(0), C.c_int32(0)
    assert L.soar_sam_weights_bytes(C.byref(seg._c), C.byref(nb), C.byref(cnt)) == 0
    assert cnt.value == len(sam.tensor_keys(sam_ref.CONFIG_A)) and nb.value >= 4 * seg.weights.numel() and nb.value % 256 == 0
    assert L.soar_sam_workspace_bytes(C.byref(seg._c), 2, 25, C.byref(nb)) == 0 and nb.value % 256 == 0
    assert L.soar_sam_workspace_bytes(C.byref(seg._c), 2, 59, C.byref(nb)) != 0 and "at most 58 points" in hip_lib.last_error()
    bad = hip_lib.SoarSamConfig.from_buffer_copy(seg._c)
    bad.head_dim, bad.heads = 100, 1                       # a head the attention kernel has no padding for
    assert L.soar_sam_weights_bytes(C.byref(bad), C.byref(nb), None) != 0 and "head_dim 100" in hip_lib.last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.embed(torch.zeros((1, 8, 8, 3), dtype=torch.uint8))
