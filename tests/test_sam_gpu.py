"""SAM on the device (soar_amd/sam.py, csrc/sam.hip) against the plain-torch restatement of tests/sam_ref.py in float64.

Tolerance, measured not fixed: for every compared tensor ``e32`` is the distance of the restatement run in float32 from the
restatement run in float64 (worst element over the float64 tensor's RMS), and the kernels must lie within ``4 e32`` of float64: the
factor covers another order of accumulation over the same float32 operands.  Both configurations are tiny (tests/sam_ref.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sam_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FACTOR = 4.0
CFGS = {"A": sam_ref.CONFIG_A, "B": sam_ref.CONFIG_B}
# per configuration: (H, W, points, labels): landscape, portrait, square
FRAMES = {
    "A": [(90, 160, [[80, 45], [70, 30], [90, 60], [75, 50], [85.5, 40.25]], [1, 1, 1, 1, 1]), (160, 90, [[45, 80]], [1]),
          (130, 130, [[60, 70], [20, 15], [66.5, 40]], [1, 0, 1])],
    "B": [(100, 170, [[85, 50], [70, 30], [100, 70]], [1, 1, 1]), (170, 100, [[50, 85]], [1]), (120, 120, [[60, 60], [10, 12]], [1, 0])],
}
_cache = {}


def rel(a, b):
    """worst element of a - b over b's RMS (b: float64)"""
    return float((a.double().cpu() - b).abs().max() / b.pow(2).mean().sqrt())


def within(name, got, ref64, ref32, floor=0.0):
    e32 = max(rel(ref32, ref64), floor)
    err = rel(got, ref64)
    print(f"{name}: err {err:.3g}  e32 {e32:.3g}  ratio {err / e32 if e32 else float('inf'):.2f}")
    assert err <= FACTOR * e32, f"{name}: {err:.3g} from float64, float32 restatement {e32:.3g}: ratio {err / e32:.2f} > {FACTOR}"


def setup(name):
    """The segmenter, the weights in both precisions and, per frame, the restatement's stages in float64 and float32 (computed once)."""
    if name not in _cache:
        from soar_amd import sam
        cfg = CFGS[name]
        sd = sam_ref.tiny_state_dict(cfg, 0)
        sd64 = {k: v.double() for k, v in sd.items()}
        seg = sam.SamSegmenter(sd, decoder_heads=cfg["dec_heads"]).to(DEV)
        frames = []
        for i, (H, W, pts, lab) in enumerate(FRAMES[name]):
            img = sam_ref.synthetic_frame(H, W, i)
            frames.append(dict(img=img, pts=np.asarray(pts, np.float32), lab=np.asarray(lab), r64=sam_ref.predict_logits(sd64, cfg, img, pts, lab, torch.float64),
                               r32=sam_ref.predict_logits(sd, cfg, img, pts, lab, torch.float32)))
        _cache[name] = (cfg, sd, sd64, seg, frames)
    return _cache[name]


def dev_frame(f):
    return (torch.from_numpy(f["img"]).to(DEV)[None], torch.from_numpy(f["pts"]).to(DEV)[None], torch.from_numpy(f["lab"]).to(DEV, torch.int32)[None])


@pytest.mark.parametrize("name", ["A", "B"])
def test_preprocessing_is_exact(name):
    cfg, sd, sd64, seg, frames = setup(name)
    from soar_amd.jpeg import resize_images
    for f in frames:
        img, _, _ = dev_frame(f)
        nh, nw = sam_ref.resized_hw(*f["img"].shape[:2], cfg["image_size"])
        assert np.array_equal(resize_images(img, nh, nw, filter="bilinear")[0].cpu().numpy(), sam_ref.resize_bilinear_u8(f["img"], nh, nw))
        assert torch.equal(seg.preprocessed(img)[0].cpu(), f["r32"]["pre"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_encoder_stage_by_stage(name):
    """patch embedding + pos_embed, one windowed block alone, one global block alone, the encoder's output"""
    cfg, sd, sd64, seg, frames = setup(name)
    assert 0 not in cfg["global_blocks"] and 1 in cfg["global_blocks"]
    for i, f in enumerate(frames):
        img, _, _ = dev_frame(f)
        patches, _ = seg.patches(img)
        t64 = sam_ref.patch_embed(sd64, f["r64"]["pre"][None])
        within(f"{name}{i} patch_embed", seg.encode(patches=patches, blocks=(0, 0), neck=False), t64, sam_ref.patch_embed(sd, f["r32"]["pre"][None]))
        for blk in (0, 1):
            x32 = t64.float()                                      # the block's input, the same float32 numbers for everyone
            o64 = sam_ref.encoder_block(sd64, cfg, x32.double(), blk)
            within(f"{name}{i} block {blk} ({'global' if blk in cfg['global_blocks'] else 'windowed'})",
                   seg.encode(tokens=x32.to(DEV), blocks=(blk, blk + 1), neck=False), o64, sam_ref.encoder_block(sd, cfg, x32, blk))
            t64 = o64
        within(f"{name}{i} embeddings", seg.embed(img)[0], f["r64"]["emb"], f["r32"]["emb"])


@pytest.mark.parametrize("name", ["A", "B"])
def test_decoder_stage_by_stage(name):
    """prompt tokens, tokens after the two-way transformer, low-resolution logits, IoU, full-resolution logits; the decoder is fed
    the float64 restatement's embedding, rounded, so that each side's error is the decoder's own"""
    cfg, sd, sd64, seg, frames = setup(name)
    for i, f in enumerate(frames):
        img, pts, lab = dev_frame(f)
        hw = f["img"].shape[:2]
        new_hw = sam_ref.resized_hw(*hw, cfg["image_size"])
        emb32 = f["r64"]["emb"].float()
        r = {}
        for dt, w in ((torch.float64, sd64), (torch.float32, sd)):
            sparse = sam_ref.prompt_tokens(w, cfg, torch.from_numpy(f["pts"]).to(dt), list(f["lab"]), hw, new_hw)
            low, iou, tok0, tok1 = sam_ref.decode(w, cfg, emb32.to(dt), sparse)
            r[dt] = dict(low=low, iou=iou, tok0=tok0, tok1=tok1, logits=sam_ref.postprocess(low, cfg, new_hw, hw))
        low, iou, tok0, tok1 = seg.decode(emb32.to(DEV)[None], pts, None, hw, lab, return_tokens=True)
        n = 2 + cfg["mask_tokens"] + len(f["pts"])
        assert tok0.shape[1] == n
        r64, r32 = r[torch.float64], r[torch.float32]
        within(f"{name}{i} prompt tokens", tok0[0], r64["tok0"], r32["tok0"])
        within(f"{name}{i} decoder tokens", tok1[0], r64["tok1"], r32["tok1"])
        within(f"{name}{i} low-res logits", low[0], r64["low"], r32["low"])
        # The IoU head turns token 0 into three numbers.  The worst of three float32 errors is a lottery as a yardstick (one frame's
        # came out six times below the same float32 run's error on the tokens the head reads), so for this tensor alone e32 is not
        # allowed to fall below the e32 of the head's input, the decoder tokens; the factor stays 4.
        within(f"{name}{i} iou", iou[0], r64["iou"], r32["iou"], floor=rel(r32["tok1"], r64["tok1"]))
        within(f"{name}{i} full-res logits", seg.postprocess(low, hw)[0], r64["logits"], r32["logits"])
        # and the interpolations alone, on the restatement's low-resolution logits
        low32 = r64["low"].float()
        within(f"{name}{i} postprocess alone", seg.postprocess(low32.to(DEV)[None], hw)[0], sam_ref.postprocess(low32.double(), cfg, new_hw, hw),
               sam_ref.postprocess(low32, cfg, new_hw, hw))


@pytest.mark.parametrize("name", ["A", "B"])
def test_end_to_end_logits_and_masks(name):
    """The whole chain against float64, and the thresholded masks: equal to the float64 restatement's everywhere except where its
    logit is within 4 e32 rms of zero, and those pixels are at most 1 % of a frame."""
    cfg, sd, sd64, seg, frames = setup(name)
    for i, f in enumerate(frames):
        img, pts, lab = dev_frame(f)
        l64, l32 = f["r64"]["logits"], f["r32"]["logits"]
        got = seg.logits(img, pts, None, lab)[0]
        within(f"{name}{i} logits end to end", got, l64, l32)
        within(f"{name}{i} low-res end to end", seg.decode(seg.embed(img), pts, None, f["img"].shape[:2], lab)[0][0], f["r64"]["low"], f["r32"]["low"])
        rms = l64.pow(2).mean().sqrt()
        band = FACTOR * rel(l32, l64) * rms
        unsure = l64.abs() <= band
        share = float(unsure.double().mean())
        print(f"{name}{i} pixels within {float(band):.3g} of zero: {100 * share:.3f} %")
        assert share <= 0.01
        m = seg.masks(img, pts, None, lab)[0].cpu()
        assert m.dtype == torch.bool and m.shape == l64.shape
        assert torch.equal(m[~unsure], (l64 > 0)[~unsure])
        assert torch.equal(m, got.cpu() > 0)


ATTN_CASES = [(7, 7, 0), (8, 8, 0), (5, 13, 0), (17, 17, 0), (7, 7, 3), (17, 17, 5)]       # 49, 64, 65, 289 keys; padded windows of 3 and 5


@pytest.mark.parametrize("rel_pos", [True, False], ids=["rel", "norel"])
@pytest.mark.parametrize("hd", [16, 80])
@pytest.mark.parametrize("gh,gw,win", ATTN_CASES)
def test_attention_kernel_alone(gh, gw, win, hd, rel_pos):
    from soar_amd import hip_lib
    B, heads = 2, 2
    Cw = heads * hd
    gen = torch.Generator().manual_seed(gh * 1000 + gw * 10 + win + hd)
    qkv = torch.randn(B, gh, gw, 3 * Cw, generator=gen)
    bias = 0.5 * torch.randn(3 * Cw, generator=gen)
    Sh, Sw = (win, win) if win else (gh, gw)
    rh = 0.3 * torch.randn(2 * Sh - 1, hd, generator=gen) if rel_pos else None
    rw = 0.3 * torch.randn(2 * Sw - 1, hd, generator=gen) if rel_pos else None
    dbl = lambda t: None if t is None else t.double()
    want = sam_ref.attention_from_qkv(qkv.double(), bias.double(), dbl(rh), dbl(rw), heads, win)
    want32 = sam_ref.attention_from_qkv(qkv, bias, rh, rw, heads, win)
    d = lambda t: None if t is None else t.to(DEV).contiguous()
    q_d, b_d, rh_d, rw_d = d(qkv), d(bias), d(rh), d(rw)
    out = torch.full((B, gh, gw, Cw), float("nan"), device=DEV)
    hip_lib.check(hip_lib.lib().soar_sam_attention(q_d.data_ptr(), b_d.data_ptr(), rh_d.data_ptr() if rel_pos else None, rw_d.data_ptr() if rel_pos else None,
                                                   out.data_ptr(), B, gh, gw, heads, hd, win, hd ** -0.5, torch.cuda.current_stream().cuda_stream),
                  "soar_sam_attention")
    assert torch.isfinite(out).all()                                   # every query of the grid was written, none twice as NaN
    within(f"attention {gh}x{gw} win {win} hd {hd} rel {rel_pos}", out, want, want32)


def test_batching_is_bit_exact():
    """Frames with 0, 1, 5 and 25 points in one batch equal the same frames alone and in another order, bit for bit; two runs agree."""
    cfg, sd, sd64, seg, frames = setup("A")
    H, W = 90, 160
    counts = [0, 1, 5, 25]
    rng = np.random.default_rng(3)
    imgs = torch.from_numpy(np.stack([sam_ref.synthetic_frame(H, W, 10 + i) for i in range(4)])).to(DEV)
    pts = torch.from_numpy(rng.uniform([0, 0], [W, H], (4, 25, 2)).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(rng.integers(0, 2, (4, 25)).astype(np.int32)).to(DEV)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    full = seg.logits(imgs, pts, cnt, lab)
    assert torch.isfinite(full).all()
    assert torch.equal(full, seg.logits(imgs, pts, cnt, lab))
    order = [2, 0, 3, 1]
    assert torch.equal(seg.logits(imgs[order], pts[order], cnt[order], lab[order]), full[order])
    for b, n in enumerate(counts):
        alone = seg.logits(imgs[b:b + 1], pts[b:b + 1, :max(n, 1)], cnt[b:b + 1], lab[b:b + 1, :max(n, 1)])
        assert torch.equal(alone[0], full[b]), f"frame {b} with {n} points"
    # slots past a frame's count take part in nothing: other numbers there change nothing
    pts2 = pts.clone()
    pts2[1, 1:] = 1e6
    assert torch.equal(seg.logits(imgs, pts2, cnt, lab), full)
    # a frame without points is defined (only the padding point) and is what the restatement gives
    r64 = sam_ref.predict_logits(sd64, cfg, imgs[0].cpu().numpy(), np.zeros((0, 2), np.float32), np.zeros(0), torch.float64)
    r32 = sam_ref.predict_logits(sd, cfg, imgs[0].cpu().numpy(), np.zeros((0, 2), np.float32), np.zeros(0), torch.float32)
    within("no points", full[0], r64["logits"], r32["logits"])


def test_resize_filter_argument():
    """filter="bilinear" is Pillow's BILINEAR byte for byte on the CPU test's cases; the default call is still the bicubic one."""
    from PIL import Image
    from soar_amd.jpeg import resize_images
    RESIZE_CASES, resize_case_image = sam_ref.RESIZE_CASES, sam_ref.resize_case_image
    for hw, out in RESIZE_CASES:
        img = resize_case_image(hw)
        got = resize_images(torch.from_numpy(img).to(DEV)[None], out[0], out[1], filter="bilinear")[0].cpu().numpy()
        assert np.array_equal(got, np.asarray(Image.fromarray(img).resize((out[1], out[0]), Image.BILINEAR))), (hw, out)
        cub = resize_images(torch.from_numpy(img).to(DEV)[None], out[0], out[1])[0].cpu().numpy()
        assert np.array_equal(cub, np.asarray(Image.fromarray(img).resize((out[1], out[0]), Image.BICUBIC)))
        assert np.array_equal(cub, resize_images(torch.from_numpy(img).to(DEV)[None], out[0], out[1], filter="bicubic")[0].cpu().numpy())
    with pytest.raises(ValueError, match="filter"):
        resize_images(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=DEV), 2, 2, filter="lanczos")


def _sequence(n=4, H=72, W=96):
    imgs = [sam_ref.synthetic_frame(H, W, 20 + i) for i in range(n)]
    kp = np.zeros((n, 25, 3), np.float32)
    rng = np.random.default_rng(5)
    for i in range(n):
        m = 3 + 2 * i                                                  # 3, 5, 7, 9 confident keypoints
        kp[i, :m, 0] = rng.uniform(W * 0.35, W * 0.65, m)
        kp[i, :m, 1] = rng.uniform(H * 0.2, H * 0.8, m)
        kp[i, :m, 2] = 0.9
    return imgs, kp


def test_segment_sequence_with_the_segmenter():
    from soar_amd import masks
    cfg, sd, sd64, seg, frames = setup("A")
    imgs, kp = _sequence()
    prompts = masks.keypoint_prompts(kp)
    flipped = [np.ascontiguousarray(img[..., ::-1]) for img in imgs]
    l64 = [sam_ref.predict_logits(sd64, cfg, f, c, l, torch.float64)["logits"] for f, (c, l) in zip(flipped, prompts)]
    l32 = [sam_ref.predict_logits(sd, cfg, f, c, l, torch.float32)["logits"] for f, (c, l) in zip(flipped, prompts)]
    # With seeded random weights the union of the three candidates at threshold 0 is nearly the whole frame and its clean-up all of
    # it.  The threshold is therefore put where the float64 restatement's union is half the pixels, so that the cleaned masks have
    # shapes worth comparing; the 1 % rule is applied around that threshold.
    thr = float(torch.stack(l64).amax(1).median())
    calls = []

    def restated(image, coords, labels):
        calls.append(len(coords))
        return sam_ref.predict_logits(sd64, cfg, np.ascontiguousarray(image), coords, labels, torch.float64)["logits"].float()
    want_m, want_s = masks.segment_sequence(restated, imgs, kp, chunk=3, device=DEV, threshold=thr)
    assert calls == [3, 5, 7, 9]
    got_m, got_s = masks.segment_sequence(seg, imgs, kp, chunk=3, threshold=thr)
    assert got_m.shape == want_m.shape == (4, 72, 96) and got_m.dtype == torch.uint8 and got_s.shape == (4, 4)
    # The candidates under the 1 % rule: one frame at a time through the segmenter (the path the batching test ties to the batched
    # one, bit for bit) against float64 ...
    dev_cands, ref_cands, flips = [], [], 0
    for i, (f, (c, l)) in enumerate(zip(flipped, prompts)):
        unsure = (l64[i] - thr).abs() <= FACTOR * rel(l32[i], l64[i]) * l64[i].pow(2).mean().sqrt()
        assert float(unsure.double().mean()) <= 0.01
        logit = seg(f, c, l)
        cand = logit.cpu() > thr
        assert torch.equal(cand[~unsure], (l64[i].float() > thr)[~unsure])
        flips += int((cand != (l64[i].float() > thr)).sum())
        dev_cands.append(logit)
        # the restatement's candidates with the device's value on the (at most 1 % of) pixels inside the band
        ref_cands.append(torch.where(unsure, logit.cpu(), l64[i].float()).to(DEV))
    print("candidate pixels on the other side of the threshold:", flips)
    # ... and what segment_sequence made of the chunk -- its runs, prompt slices, padded labels and counts, channel order -- is the
    # clean-up of exactly these candidates, and of the restatement's outside the band: no condition on either
    one_m, one_s = masks.clean_masks(torch.stack(dev_cands), threshold=thr, return_stats=True)
    assert torch.equal(got_m, one_m) and torch.equal(got_s, one_s)
    ref_m, ref_s = masks.clean_masks(torch.stack(ref_cands), threshold=thr, return_stats=True)
    assert torch.equal(got_m, ref_m) and torch.equal(got_s, ref_s)
    if flips == 0:
        assert torch.equal(got_m, want_m) and torch.equal(got_s, want_s)       # (then the lambda path saw the same candidates)
    print("stats:", got_s.tolist())
    for union, _, _, kept in got_s.tolist():                                    # unions neither empty nor full, something kept: shapes to compare
        assert 0.05 * 72 * 96 < union < 0.95 * 72 * 96 and kept > 0
    # no host round trip per frame: the same bits on another stream, and in chunks of another size
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m2, s2 = masks.segment_sequence(seg, imgs, kp, chunk=4, threshold=thr)
    s.synchronize()
    assert torch.equal(m2, got_m) and torch.equal(s2, got_s)
    # reverse_channels keeps its meaning
    m3, _ = masks.segment_sequence(seg, flipped, kp, chunk=2, reverse_channels=False, threshold=thr)
    assert torch.equal(m3, got_m)
    # and at the default threshold the two paths agree as well
    d_m, d_s = masks.segment_sequence(seg, imgs, kp, chunk=3)
    z_m, z_s = masks.clean_masks(torch.stack(dev_cands), return_stats=True)
    assert torch.equal(d_m, z_m) and torch.equal(d_s, z_s)


def test_a_plain_callable_still_takes_the_loop():
    from soar_amd import masks
    imgs, kp = _sequence()
    seen = []

    def stub(image, coords, labels):
        seen.append((image.shape, image[0, 0].tolist(), len(coords), labels.tolist()))
        H, W = image.shape[:2]
        yy, xx = np.mgrid[0:H, 0:W]
        return np.stack([((yy - c[1]) ** 2 + (xx - c[0]) ** 2 < 150).astype(np.float32) - 0.5 for c in coords[:3]])
    got_m, got_s = masks.segment_sequence(stub, imgs, kp, chunk=3, device=DEV)
    # what the loop did before this module knew a segmenter of its own: one call per frame, channels reversed, stacked, cleaned
    cands = []
    for img, (c, l) in zip(imgs, masks.keypoint_prompts(kp)):
        cands.append(torch.from_numpy(stub(img[..., ::-1], c, l)).to(DEV))
    want_m, want_s = masks.clean_masks(torch.stack(cands), return_stats=True)
    assert torch.equal(got_m, want_m) and torch.equal(got_s, want_s)
    assert len(seen) == 8 and seen[0][1] == imgs[0][0, 0, ::-1].tolist() and seen[0] == seen[4]


def test_refusals_come_before_any_launch():
    from soar_amd import hip_lib, sam
    cfg, sd, sd64, seg, frames = setup("A")
    img, pts, lab = dev_frame(frames[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.logits(img.cpu(), pts, None, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        seg.decode(seg.embed(img), pts.cpu(), None, (90, 160))
    with pytest.raises(TypeError, match="float images"):
        seg.logits(img.float(), pts, None, lab)
    with pytest.raises(NotImplementedError):
        seg.decode(seg.embed(img), pts, None, (90, 160), boxes=torch.zeros(1, 4, device=DEV))
    with pytest.raises(NotImplementedError):
        seg(frames[0]["img"], frames[0]["pts"], frames[0]["lab"], mask_input=np.zeros((1, 28, 28), np.float32))
    with pytest.raises(ValueError, match="at most"):
        seg.decode(seg.embed(img), torch.zeros(1, 59, 2, device=DEV), None, (90, 160))
    bad = dict(sd)
    bad["image_encoder.blocks.3.attn.rel_pos_w"] = torch.zeros(9, 16)
    with pytest.raises(ValueError, match=r"blocks\.3\.attn\.rel_pos_w"):
        sam.SamSegmenter(bad, decoder_heads=2)
    patches, _ = seg.patches(img)
    small = torch.empty(256, dtype=torch.uint8, device=DEV)
    with pytest.raises(hip_lib.SoarHipError, match=r"workspace of 256 bytes, need [1-9]\d{3,} \(soar_sam_workspace_bytes\)"):
        seg.encode(patches=patches, workspace=small)
    with pytest.raises(hip_lib.SoarHipError, match=r"workspace of 256 bytes, need [1-9]\d{3,} \(soar_sam_workspace_bytes\)"):
        seg.decode(seg.embed(img), pts, None, (90, 160), lab, workspace=small)
    # the library's own checks: a head dimension or a sequence the attention kernel cannot run
    p = C.c_void_p(patches.data_ptr())
    assert hip_lib.lib().soar_sam_attention(p, p, None, None, p, 1, 7, 7, 2, 100, 0, 1.0, None) != 0 and "hd=100" in hip_lib.last_error()
    assert hip_lib.lib().soar_sam_attention(p, p, None, None, p, 1, 65, 7, 2, 16, 0, 1.0, None) != 0 and "at most 64" in hip_lib.last_error()
