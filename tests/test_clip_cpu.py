"""CPU tests of soar_amd/clip.py: the restatement of tests/clip_ref.py against transformers' CLIP in float64 (the
committed fixture, and live where transformers is installed), the two key layouts, what the constructors read from shapes and refuse,
the sizing calls' refusals, and the preprocessing against Pillow.  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import clip_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_tiny.npz")
TOL = 1e-9


def rel(a, b):
    """worst element of a - b over b's RMS"""
    return float((a.double() - b.double()).abs().max() / b.double().pow(2).mean().sqrt())


@pytest.fixture(scope="module")
def clip():
    from soar_amd import build, clip
    build.build()
    return clip


@pytest.fixture(scope="module")
def golden():
    return R.load_golden(GOLDEN)


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 500_000


@pytest.mark.parametrize("L", [13, 5])
def test_text_restatement_reproduces_transformers_fixture(golden, L):
    sd, _, z = golden
    out, st = R.text_forward(sd, R.TEXT_A, z[f"text.ids.{L}"], torch.float64)
    hidden = z[f"text.hidden.{L}"]
    assert rel(st[("embed", "")], hidden[0]) <= TOL
    for i in range(R.TEXT_A["layers"]):
        assert rel(st[(i, "block")], hidden[i + 1]) <= TOL, i
    assert rel(out, z[f"text.out.{L}"]) <= TOL


def test_vision_restatement_reproduces_transformers_fixture(golden):
    _, sd, z = golden
    pixels = R.normalized(z["vision.u8"], torch.float64)
    out, st = R.vision_forward(sd, R.VISION_A, pixels, torch.float64)
    hidden = z["vision.hidden"]
    assert rel(st[("pre", "")], hidden[0]) <= TOL
    for i in range(R.VISION_A["layers"]):
        assert rel(st[(i, "block")], hidden[i + 1]) <= TOL, i
    assert rel(out, hidden[-1]) <= TOL
    assert rel(R.vision_forward(sd, R.VISION_A, pixels, torch.float64, post_norm=True)[0], z["vision.post"]) <= TOL


@pytest.mark.parametrize("skip_last", [0, 1])
def test_text_restatement_matches_live_transformers(skip_last):
    tf = pytest.importorskip("transformers")
    t = R.TEXT_B
    sd = {k: v.double() for k, v in R.tiny_state_dict(R.text_shapes(t), 5).items()}
    m = tf.CLIPTextModel(tf.CLIPTextConfig(vocab_size=t["vocab"], hidden_size=t["width"], intermediate_size=t["mlp"], num_hidden_layers=t["layers"],
                                           num_attention_heads=t["heads"], max_position_embeddings=t["context"], hidden_act="gelu",
                                           bos_token_id=0, pad_token_id=1, eos_token_id=t["vocab"] - 1)).double().eval()
    assert not m.load_state_dict(sd, strict=False).unexpected_keys
    inner = m.text_model if hasattr(m, "text_model") else m
    for L in (77, 150):
        ids = torch.randint(0, t["vocab"], (2, L), generator=torch.Generator().manual_seed(L))
        with torch.no_grad():
            o = m(input_ids=ids, output_hidden_states=True)
            want = inner.final_layer_norm(o.hidden_states[-1 - skip_last])
        if not skip_last:
            assert torch.equal(want, o.last_hidden_state)
        assert rel(R.text_forward(sd, t, ids, torch.float64, skip_last=skip_last)[0], want) <= TOL


@pytest.mark.parametrize("skip_last", [0, 1])
@pytest.mark.parametrize("post_norm", [False, True])
def test_vision_restatement_matches_live_transformers(skip_last, post_norm):
    tf = pytest.importorskip("transformers")
    v = R.VISION_B
    sd = {k: t.double() for k, t in R.tiny_state_dict(R.vision_shapes(v), 6).items()}
    m = tf.CLIPVisionModel(tf.CLIPVisionConfig(hidden_size=v["width"], intermediate_size=v["mlp"], num_hidden_layers=v["layers"],
                                               num_attention_heads=v["heads"], image_size=v["image"], patch_size=v["patch"],
                                               hidden_act="gelu")).double().eval()
    assert not m.load_state_dict(sd, strict=False).unexpected_keys
    inner = m.vision_model if hasattr(m, "vision_model") else m
    pixels = torch.randn(2, 3, v["image"], v["image"], dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        want = m(pixel_values=pixels, output_hidden_states=True).hidden_states[-1 - skip_last]
        if post_norm:
            want = inner.post_layernorm(want)
    assert rel(R.vision_forward(sd, v, pixels, torch.float64, skip_last=skip_last, post_norm=post_norm)[0], want) <= TOL


def test_open_clip_layout_gives_the_same_tensors(clip):
    t, v = R.TEXT_A, R.VISION_A
    sd = R.tiny_state_dict(R.text_shapes(t), 1)
    oc = R.to_open_clip_text(sd, t, "cond_stage_model.model.")
    oc["cond_stage_model.model.text_projection"] = torch.zeros(4, 4)       # ignored
    oc["cond_stage_model.model.logit_scale"] = torch.zeros(())
    ids = torch.randint(0, t["vocab"], (2, 13), generator=torch.Generator().manual_seed(0))
    a = R.text_forward(sd, t, ids, torch.float64)[0]
    b = R.text_forward(oc, t, ids, torch.float64, pre="cond_stage_model.model.")[0]
    assert torch.equal(a, b)
    hf = clip.ClipTextEncoder({"text_model." + k: w for k, w in sd.items()}, heads=t["heads"])
    op = clip.ClipTextEncoder(oc, heads=t["heads"])
    bare = clip.ClipTextEncoder(R.to_open_clip_text(sd, t), heads=t["heads"])
    assert hf.layout == "transformers" and op.layout == bare.layout == "open_clip"
    assert (hf.skip_last, op.skip_last) == (0, 1)
    assert torch.equal(hf.weights, op.weights) and torch.equal(hf.weights, bare.weights) and hf.tensor_names == op.tensor_names
    assert torch.equal(clip.ClipTextEncoder(sd, heads=t["heads"]).weights, hf.weights)        # without the prefix

    sv = R.tiny_state_dict(R.vision_shapes(v), 2)
    ov = R.to_open_clip_vision(sv, v, "model.")
    pixels = torch.randn(1, 3, v["image"], v["image"], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.vision_forward(sv, v, pixels, torch.float64)[0], R.vision_forward(ov, v, pixels, torch.float64, pre="model.visual.")[0])
    hv = clip.ClipImageEncoder({"vision_model." + k: w for k, w in sv.items()}, heads=v["heads"])
    assert torch.equal(hv.weights, clip.ClipImageEncoder(ov, heads=v["heads"]).weights)
    assert torch.equal(hv.weights, clip.ClipImageEncoder(sv, heads=v["heads"]).weights)


def test_sizes_are_read_from_the_shapes(clip):
    t = clip.ClipTextEncoder(R.tiny_state_dict(R.text_shapes(R.TEXT_B), 0))
    assert t.cfg == dict(width=128, heads=2, head_dim=64, layers=3, mlp=256, tokens=150, vocab=50, context=150)
    v = clip.ClipImageEncoder(R.tiny_state_dict(R.vision_shapes(R.VISION_A), 0), heads=2, skip_last=1, post_norm=True)
    assert v.cfg == dict(width=160, heads=2, head_dim=80, layers=2, mlp=320, tokens=26, patch=14, grid=5, image_size=70, patch_k=592)
    assert (v.skip_last, v.post_norm) == (1, True)
    assert clip.ClipImageEncoder(R.tiny_state_dict(R.vision_shapes(R.VISION_B), 0)).cfg["heads"] == 1          # width / 64
    wide = dict(R.VISION_A, width=1280, layers=0, mlp=8)
    assert clip.ClipImageEncoder(R.tiny_state_dict(R.vision_shapes(wide), 0)).cfg["head_dim"] == 80           # ViT-H's 16 heads
    sd = {"image_embed." + k: w for k, w in R.tiny_state_dict(R.resampler_shapes(R.RESAMPLER_A), 0).items()}
    r = clip.Resampler(sd, dim_head=32)
    assert r.cfg == dict(dim=64, depth=2, heads=2, dim_head=32, queries=5, emb=160, out=48, ff=256)
    assert clip.Resampler(R.tiny_state_dict(R.resampler_shapes(R.RESAMPLER_B), 0)).cfg["heads"] == 2           # dim_head = 64


def test_a_missing_or_misshapen_key_is_named(clip):
    sd = R.tiny_state_dict(R.text_shapes(R.TEXT_A), 0)
    bad = dict(sd)
    del bad["encoder.layers.1.self_attn.k_proj.bias"]
    with pytest.raises(KeyError, match=r"encoder\.layers\.1\.self_attn\.k_proj\.bias"):
        clip.ClipTextEncoder(bad, heads=2)
    bad = dict(sd, **{"encoder.layers.0.mlp.fc2.weight": torch.zeros(64, 120)})
    with pytest.raises(ValueError, match=r"encoder\.layers\.0\.mlp\.fc2\.weight' has shape \[64, 120\], expected \[64, 128\]"):
        clip.ClipTextEncoder(bad, heads=2)
    oc = R.to_open_clip_text(sd, R.TEXT_A)
    del oc["ln_final.weight"]
    with pytest.raises(KeyError, match="ln_final.weight"):
        clip.ClipTextEncoder(oc, heads=2)
    with pytest.raises(KeyError, match="token_embedding.weight"):
        clip.ClipTextEncoder({"x": torch.zeros(1)})
    sv = R.tiny_state_dict(R.vision_shapes(R.VISION_A), 0)
    bad = dict(sv)
    del bad["pre_layrnorm.bias"]
    with pytest.raises(KeyError, match="pre_layrnorm.bias"):
        clip.ClipImageEncoder(bad, heads=2)
    bad = dict(sv, **{"embeddings.position_embedding.weight": torch.zeros(27, 160)})
    with pytest.raises(ValueError, match="square number of positions"):
        clip.ClipImageEncoder(bad, heads=2)
    sr = R.tiny_state_dict(R.resampler_shapes(R.RESAMPLER_A), 0)
    bad = dict(sr)
    del bad["layers.1.0.to_kv.weight"]
    with pytest.raises(KeyError, match=r"layers\.1\.0\.to_kv\.weight"):
        clip.Resampler(bad, dim_head=32)
    bad = dict(sr, **{"layers.0.1.3.weight": torch.zeros(64, 250)})
    with pytest.raises(ValueError, match=r"layers\.0\.1\.3\.weight' has shape \[64, 250\]"):
        clip.Resampler(bad, dim_head=32)


def test_refusals_before_any_launch(clip):
    sd = R.tiny_state_dict(R.text_shapes(R.TEXT_A), 0)
    with pytest.raises(ValueError, match="quick_gelu"):
        clip.ClipTextEncoder(sd, heads=2, hidden_act="quick_gelu")
    with pytest.raises(ValueError, match="quick_gelu"):
        clip.ClipImageEncoder(R.tiny_state_dict(R.vision_shapes(R.VISION_A), 0), heads=2, hidden_act="quick_gelu")
    with pytest.raises(ValueError, match="skip_last = 3"):
        clip.ClipTextEncoder(sd, heads=2, skip_last=3)
    enc = clip.ClipTextEncoder(sd, heads=2)
    with pytest.raises(ValueError, match="L = 14 tokens: the position embedding has 13"):
        enc(torch.zeros(1, 14, dtype=torch.long))
    with pytest.raises(ValueError, match="token id 50 outside the vocabulary of 50"):
        enc(torch.tensor([[1, 50, 3]]))
    with pytest.raises(ValueError, match="token id -1 outside"):
        enc(torch.tensor([[1, -1, 3]]))
    with pytest.raises(ValueError, match="integer tensor"):
        enc(torch.zeros(1, 5))
    with pytest.raises(ValueError, match="pad them to one length"):
        clip.encode_prompts(enc, torch.zeros(5, dtype=torch.long), torch.zeros(6, dtype=torch.long))


def test_cpu_tensors_are_refused(clip):
    enc = clip.ClipTextEncoder(R.tiny_state_dict(R.text_shapes(R.TEXT_A), 0), heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(1, 5, dtype=torch.long))
    vis = clip.ClipImageEncoder(R.tiny_state_dict(R.vision_shapes(R.VISION_A), 0), heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vis(torch.zeros(37, 83, 3))
    res = clip.Resampler(R.tiny_state_dict(R.resampler_shapes(R.RESAMPLER_A), 0), dim_head=32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        res(torch.zeros(1, 26, 160))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clip.ImageTokens(vis, res)(torch.zeros(37, 83, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clip.attention(torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), torch.zeros(1, 4, 8), 1)
    with pytest.raises(ValueError, match="the Resampler takes 160 channels, the encoder gives 64"):
        clip.ImageTokens(clip.ClipImageEncoder(R.tiny_state_dict(R.vision_shapes(R.VISION_B), 0)), res)


def test_sizing_calls_refuse_what_the_kernels_cannot_run(clip):
    from soar_amd import hip_lib
    L = hip_lib.lib()
    nb = C.c_size_t(0)
    c = hip_lib.SoarClipConfig()
    c.kind, c.width, c.heads, c.layers, c.mlp, c.tokens, c.vocab = hip_lib.CLIP_TEXT, 200, 2, 1, 400, 77, 50
    assert L.soar_clip_workspace_bytes(C.byref(c), 1, 77, C.byref(nb)) == 1 and "head_dim = 100" in hip_lib.last_error()
    assert L.soar_clip_weights_bytes(C.byref(c), C.byref(nb), None, None) == 1 and "head_dim = 100" in hip_lib.last_error()
    c.width, c.mlp = 100, 400
    assert L.soar_clip_workspace_bytes(C.byref(c), 1, 77, C.byref(nb)) == 1 and "width = 100" in hip_lib.last_error()
    c.width, c.heads = 192, 2
    assert L.soar_clip_workspace_bytes(C.byref(c), 2, 77, C.byref(nb)) == 0 and nb.value >= 4 * 2 * 77 * (6 * 192 + 400) and nb.value % 256 == 0
    assert L.soar_clip_workspace_bytes(C.byref(c), 2, 78, C.byref(nb)) == 1 and "L=78" in hip_lib.last_error()
    c.kind, c.patch, c.grid, c.tokens = hip_lib.CLIP_VISION, 14, 5, 27
    assert L.soar_clip_workspace_bytes(C.byref(c), 1, 27, C.byref(nb)) == 1 and "tokens=27" in hip_lib.last_error()
    r = hip_lib.SoarResamplerConfig()
    r.dim, r.depth, r.heads, r.dim_head, r.queries, r.emb, r.out, r.ff = 64, 1, 2, 100, 16, 64, 64, 256
    assert L.soar_resampler_workspace_bytes(C.byref(r), 1, 26, C.byref(nb)) == 1 and "dim_head = 100" in hip_lib.last_error()
    r.dim_head, r.emb = 64, 100
    assert L.soar_resampler_workspace_bytes(C.byref(r), 1, 26, C.byref(nb)) == 1 and "emb = 100" in hip_lib.last_error()
    # the modules refuse the same from their constructors: nothing could be packed
    with pytest.raises(hip_lib.SoarHipError, match="head_dim = 100"):
        clip.ClipTextEncoder(R.tiny_state_dict(R.text_shapes(dict(R.TEXT_A, width=200, mlp=400)), 0), heads=2)
    a = hip_lib.SoarClipAttnArgs()
    a.B, a.Lq, a.Lk, a.heads, a.hd, a.scale = 1, 4, 4, 1, 100, 1.0
    assert L.soar_clip_attention(C.byref(a), None) == 1 and "hd=100: a multiple of 4 up to 96" in hip_lib.last_error()


@pytest.mark.parametrize("hw", [(37, 83), (301, 160)])
def test_preprocess_restatement_equals_pillow_and_torchvision_arithmetic(hw):
    """the bytes after the resize are Pillow's; the floats are to_tensor's and Normalize's float32 operations, here in NumPy"""
    from PIL import Image
    S, p = 70, 14
    for img in (R.sample_image(*hw, seed=1), R.sample_image(*hw, seed=2, as_float=True)):
        u8 = R.to_bytes(img)[0].numpy()
        if img.dtype != torch.uint8:
            assert np.array_equal(u8, (img.numpy() * np.float32(255)).astype(np.uint8))          # to_pil_image: mul(255).byte()
        want = np.asarray(Image.fromarray(u8).resize((S, S), Image.BICUBIC))
        got = R.resized(img, S)
        assert np.array_equal(got[0].numpy(), want)
        x = want.astype(np.float32).transpose(2, 0, 1) / np.float32(255)
        x = (x - np.array(R.MEAN, np.float32).reshape(3, 1, 1)) / np.array(R.STD, np.float32).reshape(3, 1, 1)
        px = R.normalized(got)[0].numpy()
        assert px.dtype == np.float32
        assert np.all(np.abs(px - x) <= np.spacing(np.abs(x)))
        rows = R.patch_rows(R.normalized(got), p)[0]
        assert rows.shape == (25, 592) and float(rows[:, 588:].abs().max()) == 0
        assert rows[7, 2 * 196 + 3 * 14 + 5] == px[2, 1 * 14 + 3, 2 * 14 + 5]                    # token (1, 2), channel 2, pixel (3, 5)
