"""Writes tests/golden/clip_tiny.npz: transformers' CLIPTextModel and CLIPVisionModel in float64 at the text and vision configurations A
of tests/clip_ref.py -- the weights, the inputs, every hidden state and the final-normed output.  tests/test_clip_cpu.py holds the
restatement of tests/clip_ref.py against it, so that the restatement the kernels are measured against has an oracle that shares no
code with it.

The weights are small integers times a power of two (exact in every float format), stored as int8 with their scale, so that the file
stays small: python tests/tools/make_clip_golden.py
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_ref as R  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "golden", "clip_tiny.npz")
LEVELS = 7                             # vectors and embeddings are integers in -7 .. 7 times a power of two,
MATRIX_LEVELS = 2                      # the matrices, which are most of the file, in -2 .. 2


def grid_weights(shapes, seed):
    """-> {key: (int8 array, scale)}: matrices of standard deviation about 1 / sqrt(fan_in), gains near 1, small biases"""
    rng = np.random.default_rng(seed)
    out = {}
    for k, s in shapes.items():
        levels, std = LEVELS, 4.3                                # the standard deviation of integers uniform in -7 .. 7
        if k.endswith("bias"):
            target = 0.1
        elif "norm" in k:
            target = 0.1                                         # around 1: clip_ref.golden_values adds it
        elif len(s) <= 2 and "embedding" in k:
            target = 0.7
        else:
            target, levels, std = 1 / math.sqrt(float(np.prod(s[1:]))), MATRIX_LEVELS, 1.4
        q = rng.integers(-levels, levels + 1, size=s).astype(np.int8)
        out[k] = (q, 2.0 ** round(math.log2(target / std)))
    return out


def main():
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPVisionConfig, CLIPVisionModel
    t, v = R.TEXT_A, R.VISION_A
    data = {}
    tg, vg = grid_weights(R.text_shapes(t), 1), grid_weights(R.vision_shapes(v), 2)
    for name, grid in (("text", tg), ("vision", vg)):
        for k, (q, s) in grid.items():
            data[f"{name}.q.{k}"], data[f"{name}.s.{k}"] = q, np.float64(s)

    tm = CLIPTextModel(CLIPTextConfig(vocab_size=t["vocab"], hidden_size=t["width"], intermediate_size=t["mlp"], num_hidden_layers=t["layers"],
                                      num_attention_heads=t["heads"], max_position_embeddings=t["context"], hidden_act="gelu",
                                      bos_token_id=0, pad_token_id=1, eos_token_id=t["vocab"] - 1)).double().eval()
    missing = tm.load_state_dict(R.golden_values(tg), strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
    g = torch.Generator().manual_seed(3)
    for L in (t["context"], 5):
        ids = torch.randint(0, t["vocab"], (2, L), generator=g)
        with torch.no_grad():
            o = tm(input_ids=ids, output_hidden_states=True)
        assert len(o.hidden_states) == t["layers"] + 1
        data[f"text.ids.{L}"] = ids.numpy()
        data[f"text.hidden.{L}"] = torch.stack(o.hidden_states).numpy()
        data[f"text.out.{L}"] = o.last_hidden_state.numpy()

    vm = CLIPVisionModel(CLIPVisionConfig(hidden_size=v["width"], intermediate_size=v["mlp"], num_hidden_layers=v["layers"],
                                          num_attention_heads=v["heads"], image_size=v["image"], patch_size=v["patch"],
                                          hidden_act="gelu")).double().eval()
    missing = vm.load_state_dict(R.golden_values(vg), strict=False)
    assert not missing.unexpected_keys and all("position_ids" in k for k in missing.missing_keys), missing
    u8 = R.resized(R.sample_image(37, 83, 4), v["image"])
    pixels = R.normalized(u8, torch.float64)
    with torch.no_grad():
        o = vm(pixel_values=pixels, output_hidden_states=True)
        inner = vm.vision_model if hasattr(vm, "vision_model") else vm
        post = inner.post_layernorm(o.last_hidden_state)
    assert len(o.hidden_states) == v["layers"] + 1
    data["vision.u8"] = u8.numpy()
    data["vision.hidden"] = torch.stack(o.hidden_states).numpy()  # [0]: after pre_layrnorm; [-1]: the output
    assert torch.equal(o.hidden_states[-1], o.last_hidden_state)  # (no post_layernorm in it: only the pooled class token gets one)
    data["vision.post"] = post.numpy()                            # post_layernorm on every token
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
