"""GPU tests of the mask clean-up (csrc/masks.hip, soar_amd/masks.py): every comparison is exact equality of masks and
statistics with the NumPy restatement of tests/masks_ref.py (itself checked against scipy.ndimage in tests/test_masks_cpu.py).  No
tolerance is involved anywhere: the kernels are integer arithmetic."""
import numpy as np
import pytest
import torch

import masks_ref as R
from soar_amd import masks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _np(t):
    return t.cpu().numpy()


def _check_pipeline(cand, dev, name, threshold=0.0):
    """cand [N,K,H,W] (NumPy): clean_masks and open_close against the oracle."""
    want, want_stats = R.clean_batch(cand, threshold)
    got, stats = masks.clean_masks(torch.from_numpy(cand).to(dev), threshold=threshold, return_stats=True)
    assert got.dtype == torch.uint8 and stats.dtype == torch.int32
    assert np.array_equal(_np(stats), want_stats), (name, _np(stats).tolist(), want_stats.tolist())
    assert np.array_equal(_np(got), want), (name, int((_np(got) != want).sum()))
    oc, oc_stats = masks.open_close(torch.from_numpy(cand).to(dev), threshold=threshold, return_stats=True)
    want_oc = np.stack([R.open_close(R.union(c, threshold)) for c in cand]).astype(np.uint8)
    assert np.array_equal(_np(oc), want_oc), (name, int((_np(oc) != want_oc).sum()))
    assert np.array_equal(_np(oc_stats)[:, :2], want_stats[:, :2]) and not _np(oc_stats)[:, 2:].any(), name
    return got, stats


def _check_labelling(mask, dev, name):
    want, n, kept = R.largest_component(mask)
    got, stats = masks.largest_component(torch.from_numpy(mask.astype(np.uint8))[None].to(dev), return_stats=True)
    area = int(mask.sum())
    assert _np(stats)[0].tolist() == [area, area, n, kept], (name, _np(stats)[0].tolist(), (area, n, kept))
    assert np.array_equal(_np(got)[0], want), (name, int((_np(got)[0] != want).sum()))


@pytest.mark.parametrize("W", R.SMALL_W)
def test_sizes_below_and_around_the_machinery(dev, W):
    """Zero padding at the borders, padding bits of the last word, windows larger than the image."""
    for H in R.SMALL_H:
        _check_pipeline(np.ones((1, 1, H, W), np.uint8), dev, f"ones_{H}x{W}")
        _check_pipeline(R.bernoulli(H, W, 0.7, 100 * H + W)[None, None].astype(np.uint8), dev, f"bernoulli_{H}x{W}")


def test_open_close_hand_made(dev):
    m = R.handmade_morph()
    c = R.open_close(m)
    assert not c[11:15, 3:7].any() and c[11:16, 11:16].all() and c[11:16, 22:68].all() and not c[8].any()      # the scene does what it says
    _check_pipeline(m[None, None].astype(np.uint8), dev, "handmade_morph")
    _check_pipeline(R.stripes(m)[None], dev, "handmade_morph_stripes")


@pytest.mark.parametrize("shape", R.BLOB_SHAPES)
def test_blob_scenes(dev, shape):
    H, W, sigma = shape
    for seed in range(4):
        m = R.blobs(H, W, sigma, seed)
        _check_pipeline(R.split_candidates(m, 3, seed)[None], dev, f"blobs_{H}x{W}_{seed}")


def test_labelling_on_noise(dev):
    counts = {}
    for name, m in R.noise_scenes():
        _check_labelling(m, dev, name)
        counts[name] = len(R.label(m)[1])
    assert (counts["noise_0.3_7"], counts["noise_0.41_7"], counts["noise_0.55_7"]) == (296, 88, 14)   # 790 / 599 / 272 with 4-connectivity


def test_labelling_hand_made(dev):
    scenes = R.handmade_labels()
    for name, m in scenes.items():
        _check_labelling(m, dev, name)
    got = masks.largest_component(torch.from_numpy(scenes["equal_squares_a"].astype(np.uint8))[None].to(dev))
    assert _np(got)[0, 10:20, 200:210].all() and not _np(got)[0, 60:70, 30:40].any()            # the smaller raster index wins
    got = masks.largest_component(torch.from_numpy(scenes["equal_squares_b"])[None].to(dev))     # bool input
    assert _np(got)[0, 10:20, 30:40].all() and int(_np(got).sum()) == 100


def test_batch(dev):
    cand = R.batch_scene()
    assert not np.array_equal(cand[0, 0], cand[0, 1]) and not R.union(cand[1]).any() and R.union(cand[2]).all()
    # frame 0: no candidate alone holds the kept component's connections (column stripes)
    alone = max(R.largest_component(R.open_close(c))[2] for c in cand[0])
    want, want_stats = R.clean_batch(cand)
    assert alone < want_stats[0, 3]
    got, stats = _check_pipeline(cand, dev, "batch")
    for i in range(len(cand)):
        one, one_stats = masks.clean_masks(torch.from_numpy(cand[i:i + 1]).to(dev), return_stats=True)
        assert torch.equal(one[0], got[i]) and torch.equal(one_stats[0], stats[i]), i
    assert not _np(got)[1].any() and _np(stats)[1].tolist() == [0, 0, 0, 0]
    assert _np(stats)[2].tolist() == [64 * 96, 64 * 96, 1, 64 * 96] and _np(got)[2].all()


def test_dtypes(dev):
    H, W = 64, 96
    m = np.stack([R.blobs(H, W, 3.0, 20 + k) for k in range(3)])
    rng = np.random.default_rng(3)
    want, want_stats = R.clean_batch(m[None].astype(np.uint8))
    # bool
    got, stats = masks.clean_masks(torch.from_numpy(m)[None].to(dev), return_stats=True)
    assert np.array_equal(_np(got), want) and np.array_equal(_np(stats), want_stats)
    # uint8 with values {0, 1, 2, 255}
    u8 = np.where(m, rng.choice(np.array([1, 2, 255], np.uint8), m.shape), np.uint8(0)).astype(np.uint8)
    got, stats = masks.clean_masks(torch.from_numpy(u8)[None].to(dev), return_stats=True)
    assert np.array_equal(_np(got), want) and np.array_equal(_np(stats), want_stats)
    # float32 logits: 0.0, -0.0, NaN, -inf and -1e-30 are unset; +inf and +1e-30 are set
    on = rng.choice(np.array([1.5, np.inf, 1e-30], np.float32), m.shape)
    off = rng.choice(np.array([0.0, -0.0, np.nan, -np.inf, -1e-30, -2.0], np.float32), m.shape)
    logits = np.where(m, on, off).astype(np.float32)
    assert np.array_equal(R.union(logits), R.union(m)) and np.isnan(logits).any() and np.signbit(logits[logits == 0]).any()
    got, stats = masks.clean_masks(torch.from_numpy(logits)[None].to(dev), return_stats=True)
    assert np.array_equal(_np(got), want) and np.array_equal(_np(stats), want_stats)
    # another threshold
    lg = rng.standard_normal((1, 3, H, W)).astype(np.float32)
    w2, s2 = R.clean_batch(lg, 0.75)
    got, stats = masks.clean_masks(torch.from_numpy(lg).to(dev), threshold=0.75, return_stats=True)
    assert np.array_equal(_np(got), w2) and np.array_equal(_np(stats), s2)
    # a non-contiguous view
    wide = torch.zeros((1, 3, H, 2 * W + 1), dtype=torch.float32, device=dev)
    wide[..., 1::2] = torch.from_numpy(logits).to(dev)
    view = wide[..., 1::2]
    assert not view.is_contiguous()
    got, stats = masks.clean_masks(view, return_stats=True)
    assert np.array_equal(_np(got), want) and np.array_equal(_np(stats), want_stats)
    t = torch.from_numpy(u8).to(dev).permute(1, 2, 0).contiguous()[None]  # channels-last storage
    tv = t.permute(0, 3, 1, 2)
    assert not tv.is_contiguous()
    got = masks.clean_masks(tv)
    assert np.array_equal(_np(got), want)


def test_one_full_hd_frame(dev):
    big = R.big_scene(0)
    cand = R.split_candidates(big, 3, 1)[None]
    want, want_stats = R.clean_batch(cand)
    assert want_stats[0, 2] > 1 and 0 < want_stats[0, 3] < want_stats[0, 1] < want_stats[0, 0]
    t = torch.from_numpy(cand).to(dev)
    got, stats = masks.clean_masks(t, return_stats=True)
    assert np.array_equal(_np(stats), want_stats), (_np(stats).tolist(), want_stats.tolist())
    assert np.array_equal(_np(got), want)
    # N = 2 in one chunk, in two chunks, and once more: the same bits
    two = torch.cat([t, torch.from_numpy(R.stripes(np.roll(big, 100, axis=1), 3, 64))[None].to(dev)])
    a, sa = masks.clean_masks(two, return_stats=True)
    cap = masks.workspace_bytes(1, 1080, 1920) + 1024
    assert masks.workspace_bytes(2, 1080, 1920) > cap
    b, sb = masks.clean_masks(two, return_stats=True, max_workspace_bytes=cap)
    c, sc = masks.clean_masks(two, return_stats=True)
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.equal(a, c) and torch.equal(sa, sc)
    assert torch.equal(a[0], got[0]) and torch.equal(sa[0], stats[0]) and int(sa[1, 3]) > 0


def test_segment_sequence_with_a_fake_predictor(dev, tmp_path):
    from PIL import Image
    H, W, N = 96, 128, 3
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(N)]
    logits = [np.where(R.split_candidates(R.blobs(H, W, 4.0, 30 + i), 3, i) != 0, 2.0, -3.0).astype(np.float32) for i in range(N)]
    kp = np.zeros((N, 137, 3), np.float32)
    kp[..., :2] = rng.uniform(0, 90, (N, 137, 2))
    kp[..., 2] = rng.uniform(0, 1, (N, 137))
    kp[1, 4, 2] = 0.5
    seen = []

    def predict(image, coords, labels):
        i = len(seen)
        seen.append((np.array(image), coords.copy(), labels.copy()))
        return torch.from_numpy(logits[i]) if i % 2 else logits[i]           # a tensor or an array

    got, stats = masks.segment_sequence(predict, images, kp, chunk=2)
    prompts = masks.keypoint_prompts(kp)
    assert len(seen) == N
    for i in range(N):
        assert np.array_equal(seen[i][0], images[i][..., ::-1])               # the channel-reversed image, as in the reference
        assert np.array_equal(seen[i][1], prompts[i][0]) and np.array_equal(seen[i][2], prompts[i][1])
    want, want_stats = masks.clean_masks(torch.from_numpy(np.stack(logits)).to(dev), return_stats=True)
    assert torch.equal(got, want) and torch.equal(stats, want_stats)
    ref, ref_stats = R.clean_batch(np.stack(logits))
    assert np.array_equal(_np(got), ref) and np.array_equal(_np(stats), ref_stats)
    paths = masks.save_masks(got, str(tmp_path))
    back = np.stack([np.asarray(Image.open(p)) > 0 for p in paths])
    assert np.array_equal(back, _np(got) != 0)
