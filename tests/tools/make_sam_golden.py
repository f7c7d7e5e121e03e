"""Writes tests/golden/sam_tiny.npz: configuration A of tests/sam_ref.py through ``transformers.SamModel`` in float64, an
implementation of SAM that shares no code with this repository.  Run on the CPU: ``python tests/tools/make_sam_golden.py``.

The fixture holds the weights (float32, ``segment_anything``'s key names), two uint8 frames (90 x 160 and 160 x 90), their points
(5 and 1) and, per frame, the image embedding, the low-resolution logits and the IoU predictions as float64.

``hf_model(cfg, sd)`` (the model under HF's key names) and ``hf_run`` are also what tests/test_sam_cpu.py compares the restatement
with at configuration B.
"""
import os
import re
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sam_ref  # noqa: E402


def hf_key(key, cfg):
    """segment_anything's key -> the list of HF ``SamModel`` keys that hold the same tensor."""
    if key == "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix":
        return ["prompt_encoder.shared_embedding.positional_embedding", "shared_image_embedding.positional_embedding"]
    k = key
    k = k.replace("image_encoder.patch_embed.proj.", "image_encoder.patch_embed.projection.")
    k = re.sub(r"image_encoder\.blocks\.(\d+)\.norm([12])\.", r"image_encoder.layers.\1.layer_norm\2.", k)
    k = k.replace("image_encoder.blocks.", "image_encoder.layers.")
    for a, b in (("neck.0.", "neck.conv1."), ("neck.1.", "neck.layer_norm1."), ("neck.2.", "neck.conv2."), ("neck.3.", "neck.layer_norm2.")):
        k = k.replace("image_encoder." + a, "image_encoder." + b)
    k = k.replace("image_encoder.", "vision_encoder.")
    k = k.replace("prompt_encoder.point_embeddings.", "prompt_encoder.point_embed.")
    k = re.sub(r"(mask_decoder\.transformer\.layers\.\d+)\.norm(\d)\.", r"\1.layer_norm\2.", k)
    k = k.replace("transformer.norm_final_attn.", "transformer.layer_norm_final_attn.")
    k = k.replace("output_upscaling.0.", "upscale_conv1.").replace("output_upscaling.1.", "upscale_layer_norm.").replace("output_upscaling.3.", "upscale_conv2.")
    m = re.match(r"(mask_decoder\.(?:output_hypernetworks_mlps\.\d+|iou_prediction_head))\.layers\.(\d+)\.(weight|bias)", k)
    if m:
        depth = cfg["iou_depth"] if "iou_prediction_head" in k else cfg["hyper_depth"]
        l = int(m.group(2))
        name = "proj_in" if l == 0 else ("proj_out" if l == depth - 1 else f"layers.{l - 1}")
        k = f"{m.group(1)}.{name}.{m.group(3)}"
    return [k]


def hf_model(cfg, sd):
    from transformers import SamConfig, SamModel
    from transformers.models.sam.configuration_sam import SamMaskDecoderConfig, SamPromptEncoderConfig, SamVisionConfig
    P = cfg["out_chans"]
    v = SamVisionConfig(hidden_size=cfg["embed"], output_channels=P, num_hidden_layers=cfg["depth"], num_attention_heads=cfg["heads"],
                        image_size=cfg["image_size"], patch_size=cfg["patch"], window_size=cfg["window"],
                        global_attn_indexes=list(cfg["global_blocks"]), mlp_dim=cfg["mlp"], num_pos_feats=P // 2)
    # segment_anything's decoder norms are nn.LayerNorm defaults (1e-5); HF's configuration default is 1e-6
    d = SamMaskDecoderConfig(hidden_size=P, mlp_dim=cfg["dec_mlp"], num_hidden_layers=cfg["dec_layers"], num_attention_heads=cfg["dec_heads"],
                             attention_downsample_rate=cfg["dec_down"], num_multimask_outputs=cfg["mask_tokens"] - 1,
                             iou_head_depth=cfg["iou_depth"], iou_head_hidden_dim=cfg["iou_hidden"], layer_norm_eps=1e-5)
    p = SamPromptEncoderConfig(hidden_size=P, image_size=cfg["image_size"], patch_size=cfg["patch"])
    model = SamModel(SamConfig(vision_config=v, mask_decoder_config=d, prompt_encoder_config=p)).double().eval()
    own = model.state_dict()
    seen = set()
    for key, t in sd.items():
        for k in hf_key(key, cfg):
            if k not in own or tuple(own[k].shape) != tuple(t.shape):
                raise KeyError(f"{key} -> {k}: no such tensor of shape {tuple(t.shape)} in SamModel")
            own[k] = t.to(torch.float64)
            seen.add(k)
    left = [k for k in own if k not in seen and ".mask_embed." not in k and "point_embed.2" not in k and "point_embed.3" not in k]
    if left:
        raise KeyError(f"SamModel tensors the state dict does not set: {left}")
    model.load_state_dict(own)
    return model


@torch.no_grad()
def hf_run(model, cfg, image_u8, points, labels):
    """One frame through HF's model on the restatement's pre-processed image -> (embedding [P,g,g], low-res logits [3,4g,4g], iou [3])."""
    x, new_hw = sam_ref.preprocess(np.asarray(image_u8)[None], cfg, torch.float64)
    pts = sam_ref.scale_points(torch.as_tensor(np.asarray(points, np.float32).reshape(-1, 2)).double(), image_u8.shape[:2], new_hw)
    emb = model.get_image_embeddings(x)
    lab = torch.as_tensor(np.asarray(labels).reshape(1, 1, -1)).long()
    out = model(image_embeddings=emb, input_points=pts[None, None], input_labels=lab, multimask_output=True)
    return emb[0], out.pred_masks[0, 0], out.iou_scores[0, 0]


def frames_and_points(seed=0):
    """Two frames of smooth colour with a bright body in the middle, and points on it."""
    rng = np.random.default_rng(seed)
    frames = []
    for H, W in ((90, 160), (160, 90)):
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([40 + 60 * np.sin(xx / 17.0 + c) + 50 * np.cos(yy / 11.0 - c) for c in range(3)], -1)
        body = ((yy - H / 2) / (H * 0.35)) ** 2 + ((xx - W / 2) / (W * 0.2)) ** 2 < 1
        img[body] += 90
        frames.append(np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8))
    pts = [np.array([[80, 45], [70, 30], [90, 60], [75, 50], [85.5, 40.25]], np.float32), np.array([[45, 80]], np.float32)]
    return frames, pts


def main():
    cfg = sam_ref.CONFIG_A
    sd = sam_ref.tiny_state_dict(cfg, 0)
    model = hf_model(cfg, sd)
    frames, pts = frames_and_points()
    out = {"w:" + k: v.numpy() for k, v in sd.items()}
    for i, (f, p) in enumerate(zip(frames, pts)):
        emb, low, iou = hf_run(model, cfg, f, p, np.ones(len(p), np.int64))
        out.update({f"frame{i}": f, f"points{i}": p, f"emb{i}": emb.numpy(), f"low{i}": low.numpy(), f"iou{i}": iou.numpy()})
    path = os.path.join(os.path.dirname(HERE), "golden", "sam_tiny.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
