"""CPU tests of the normal-map preprocessing (soar_amd/normals.py): the checkpoint's key layout, the argument checks of
the C calls (no launch), the restatement's phase table and crop, and the PNG round trip."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import normalnet_ref as ref
from soar_amd import normals


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_key_layout_small():
    lay = normals.state_dict_layout(8, 2, 1)
    want = {"model.1": (8, 6, 7, 7), "model.4": (16, 8, 3, 3), "model.7": (32, 16, 3, 3), "model.10.conv_block.1": (32, 32, 3, 3),
            "model.10.conv_block.5": (32, 32, 3, 3), "model.11": (32, 16, 3, 3), "model.14": (16, 8, 3, 3), "model.18": (3, 8, 7, 7)}
    bias = {"model.1": 8, "model.4": 16, "model.7": 32, "model.10.conv_block.1": 32, "model.10.conv_block.5": 32, "model.11": 16,
            "model.14": 8, "model.18": 3}
    expect = {}
    for net in ("netF", "netB"):
        for k, s in want.items():
            expect[f"{net}.{k}.weight"] = s
            expect[f"{net}.{k}.bias"] = (bias[k],)
    assert lay == expect


def test_key_layout_shipped_on_meta():
    """ngf 64, four levels, nine blocks: keys and shapes only, nothing allocated."""
    lay = normals.state_dict_layout(64, 4, 9)
    assert lay["netF.model.1.weight"] == (64, 6, 7, 7)
    assert [lay[f"netB.model.{i}.weight"] for i in (4, 7, 10, 13)] == [(128, 64, 3, 3), (256, 128, 3, 3), (512, 256, 3, 3), (1024, 512, 3, 3)]
    for i in range(16, 25):
        assert lay[f"netF.model.{i}.conv_block.1.weight"] == lay[f"netF.model.{i}.conv_block.5.weight"] == (1024, 1024, 3, 3)
    assert [lay[f"netF.model.{i}.weight"] for i in (25, 28, 31, 34)] == [(1024, 512, 3, 3), (512, 256, 3, 3), (256, 128, 3, 3), (128, 64, 3, 3)]
    assert lay["netF.model.25.bias"] == (512,) and lay["netF.model.38.weight"] == (3, 64, 7, 7) and lay["netF.model.38.bias"] == (3,)
    assert len(lay) == 2 * 2 * (1 + 4 + 18 + 4 + 1)
    sd = {k: torch.empty(s, device="meta") for k, s in lay.items()}
    net = normals.NormalNet(sd)
    assert net.netF_w5.shape == (1024, 1024, 3, 3) and net.netF_w5.device.type == "meta" and net.netB_bias.shape == (3,)


def test_lightning_prefix_and_named_errors():
    sd = ref.random_state_dict(8, 2, 1, seed=1)
    a = normals.NormalNet(sd, 8, 2, 1)
    b = normals.NormalNet({"netG." + k: v for k, v in sd.items()}, 8, 2, 1)
    assert all(torch.equal(x, y) for x, y in zip(a.buffers(), b.buffers()))
    # the biases in front of an InstanceNorm cancel in it: a checkpoint without them is complete
    normals.NormalNet({k: v for k, v in sd.items() if not (k.endswith(".bias") and ".model.18." not in k)}, 8, 2, 1)
    missing = dict(sd)
    del missing["netB.model.10.conv_block.5.weight"]
    with pytest.raises(KeyError, match=r"netB\.model\.10\.conv_block\.5\.weight"):
        normals.NormalNet(missing, 8, 2, 1)
    bad = dict(sd)
    bad["netF.model.11.weight"] = torch.zeros(16, 32, 3, 3)           # a transposed convolution is [Cin][Cout]
    with pytest.raises(ValueError, match=r"netF\.model\.11\.weight.*\[16, 32, 3, 3\].*\[32, 16, 3, 3\]"):
        normals.NormalNet(bad, 8, 2, 1)
    with pytest.raises(ValueError, match="ngf"):
        normals.NormalNet(sd, 12, 2, 1)


def test_c_calls_refuse_bad_arguments_without_a_launch(lib):
    from soar_amd import hip_lib
    n = C.c_size_t(0)
    assert lib.soar_normalnet_weights_bytes(64, 4, 9, C.byref(n)) == 0
    trunk = 18 * 1024 * 1024 * 9 * 4
    assert trunk <= n.value <= trunk * 1.2 and n.value % 256 == 0
    assert lib.soar_normalnet_weights_bytes(12, 4, 9, C.byref(n)) != 0 and "ngf" in hip_lib.last_error()
    assert lib.soar_normalnet_weights_bytes(64, 5, 9, C.byref(n)) != 0 and "n_down" in hip_lib.last_error()
    assert lib.soar_normalnet_workspace_bytes(4, 512, 512, 64, 4, 9, C.byref(n)) == 0
    assert n.value >= 3 * 4 * 512 * 512 * 64 * 4 and n.value % 256 == 0
    assert lib.soar_normalnet_workspace_bytes(1, 520, 512, 64, 4, 9, C.byref(n)) != 0 and "multiples of 2^n_down" in hip_lib.last_error()
    assert lib.soar_normalnet_workspace_bytes(1, 16, 32, 8, 4, 1, C.byref(n)) != 0          # one pixel at the bottom level
    assert lib.soar_normalnet_workspace_bytes(-1, 32, 32, 8, 4, 1, C.byref(n)) != 0 and "N must" in hip_lib.last_error()
    assert lib.soar_normalnet_workspace_bytes(65536, 4, 4, 8, 1, 0, C.byref(n)) != 0 and "N must" in hip_lib.last_error()
    assert lib.soar_normalnet_workspace_bytes(0, 32, 32, 8, 4, 1, C.byref(n)) == 0
    assert lib.soar_normalnet_weights_bytes(8, 1, 100, C.byref(n)) == 0 and n.value >= 200 * 16 * 16 * 9 * 4     # any number of blocks
    a = hip_lib.SoarNormalNetArgs()
    a.N, a.H, a.W, a.ngf, a.n_down, a.n_blocks = 1, 32, 32, 8, 4, 1
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p).value                 # any non-NULL address: nothing reads it before the checks fail
    assert lib.soar_normalnet_forward(C.byref(a), None, 0, None) != 0 and "NULL" in hip_lib.last_error()
    a.image = a.prior_F = a.prior_B = a.normal_F = a.normal_B = p
    a.weights_F = a.weights_B = 0x1000
    assert lib.soar_normalnet_forward(C.byref(a), None, 0, None) != 0 and "workspace" in hip_lib.last_error()
    a.ngf = 20
    assert lib.soar_normalnet_forward(C.byref(a), 0x1000, 1 << 30, None) != 0 and "ngf" in hip_lib.last_error()
    a.ngf, a.H = 8, 40
    assert lib.soar_normalnet_forward(C.byref(a), 0x1000, 1 << 30, None) != 0 and "multiples" in hip_lib.last_error()
    a.H, a.N = 32, 0
    assert lib.soar_normalnet_forward(C.byref(a), None, 0, None) == 0                       # nothing to do
    arr = (C.c_void_p * 3)(p, p, p)
    assert lib.soar_normalnet_pack_weights(8, 4, 1, arr, 3, 0x1000, 1 << 30, None) != 0 and "13 tensors" in hip_lib.last_error()
    st = (C.c_int64 * 3)(1, 1, 1)
    assert lib.soar_normal_crop_boxes(1, 0, 8, 512, p, st, p, p, p, p, None) != 0 and "H and W" in hip_lib.last_error()
    assert lib.soar_normal_crop_boxes(1, 8, 8, 512, None, st, p, p, p, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert lib.soar_normal_crop_bytes(1, 8, 8, None, p, p, p, p, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert lib.soar_normal_crop_bytes(0, 8, 8, None, None, None, None, None, None, None) == 0


def test_cpu_tensors_are_refused():
    sd = ref.random_state_dict(8, 2, 1, seed=1)
    net = normals.NormalNet(sd, 8, 2, 1)
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        normals.crop_frames(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.ones(1, 8, 8, dtype=torch.uint8), torch.eye(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        normals.estimate_normals(net, torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.ones(1, 8, 8, dtype=torch.uint8), torch.eye(3),
                                 torch.zeros(1, 3, 512, 512), torch.zeros(1, 3, 512, 512))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        normals.normal_bytes(x, x, x[:, :1])


def test_transposed_convolution_equals_its_four_phases():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 4, 3, 5), generator=g, dtype=torch.float64)
    w = torch.randn((4, 6, 3, 3), generator=g, dtype=torch.float64)
    want = F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1)
    got = ref.conv_transpose_phases(x, w)
    assert got.shape == want.shape == (2, 6, 6, 10)
    assert torch.allclose(got, want, rtol=0, atol=1e-13)
    assert sum(len(ref.PHASE_TAPS[py]) * len(ref.PHASE_TAPS[px]) for py in (0, 1) for px in (0, 1)) == 9


def _bilinear(plane, x, y):
    """the sample at pixel position (x, y) of a list of rows, zeros outside: written out by hand"""
    x0, y0 = math.floor(x), math.floor(y)
    wx, wy = x - x0, y - y0
    v = 0.0
    for yy, wyy in ((y0, 1 - wy), (y0 + 1, wy)):
        for xx, wxx in ((x0, 1 - wx), (x0 + 1, wx)):
            if 0 <= yy < len(plane) and 0 <= xx < len(plane[0]):
                v += wyy * wxx * plane[yy][xx]
    return v


def test_crop_restatement_on_a_hand_worked_example():
    """8 x 8 frames, a 4 x 4 crop.  Frame 0: mask rows 2..5, columns 3..6 -> box (3, 2, 6, 5), centre (4.5, 3.5), side 3.3: the crop box
    is (2.85, 1.85, 6.15, 5.15).  Frame 1: rows 0..7, columns 5..7 -> centre (6, 3.5), side 7.7: (2.15, -0.35, 9.85, 7.35), which
    leaves the frame at the top, the bottom and the right."""
    S = 4
    images = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    images[..., 0] = (torch.arange(8) * 30)[None, None, :].to(torch.uint8)       # red rises along x
    images[..., 1] = (torch.arange(8) * 20)[None, :, None].to(torch.uint8)       # green rises along y
    images[..., 2] = 255
    masks = torch.zeros((2, 8, 8), dtype=torch.uint8)
    masks[0, 2:6, 3:7] = 255
    masks[1, :, 5:8] = 102                                                       # a soft mask: 0.4
    K = torch.tensor([[10.0, 0.0, 4.0], [0.0, 12.0, 3.0], [0.0, 0.0, 1.0]]).repeat(2, 1, 1)
    img, msk, nK, boxes = ref.crop(images, masks, K, S=S, dtype=torch.float64)
    assert torch.allclose(boxes, torch.tensor([[2.85, 1.85, 6.15, 5.15], [2.15, -0.35, 9.85, 7.35]], dtype=torch.float64), atol=1e-12)
    want_K0 = [[S / 3.3 * 10.0, 0.0, S / 3.3 * (4.0 - 2.85)], [0.0, S / 3.3 * 12.0, S / 3.3 * (3.0 - 1.85)], [0.0, 0.0, 1.0]]
    want_K1 = [[S / 7.7 * 10.0, 0.0, S / 7.7 * (4.0 - 2.15)], [0.0, S / 7.7 * 12.0, S / 7.7 * (3.0 + 0.35)], [0.0, 0.0, 1.0]]
    assert torch.allclose(nK, torch.tensor([want_K0, want_K1], dtype=torch.float64), atol=1e-12)
    for n in range(2):
        m = (masks[n].double() / 255).tolist()
        planes = [((images[n, :, :, c].double() / 255 * 2 - 1) * (masks[n].double() / 255)).tolist() for c in range(3)]
        b = boxes[n].tolist()
        for jy in range(S):
            for jx in range(S):
                x = b[0] + (b[2] - b[0]) * jx / (S - 1) - 0.5
                y = b[1] + (b[3] - b[1]) * jy / (S - 1) - 0.5
                assert abs(msk[n, 0, jy, jx].item() - _bilinear(m, x, y)) < 1e-12
                for c in range(3):
                    assert abs(img[n, c, jy, jx].item() - _bilinear(planes[c], x, y)) < 1e-12
    # three samples by hand.  Frame 0, sample (0, 0) sits at (2.35, 1.35): only pixel (3, 2) of its four neighbours is masked,
    # weight 0.35 * 0.35; blue there is 1.  Frame 1, row 0 is 0.85 above the first row: weight 0.15 of it.
    assert abs(msk[0, 0, 0, 0].item() - 0.35 * 0.35) < 1e-12 and abs(img[0, 2, 0, 0].item() - 0.35 * 0.35) < 1e-12
    assert abs(msk[1, 0, 0, 1].item() - 0.15 * 0.4 * (2.15 + 7.7 / 3 - 0.5 - 4)) < 1e-12
    assert msk[1, 0, 1, 3].item() == 0.0                                          # x = 9.35: right of the frame
    with pytest.raises(ValueError, match="empty mask"):
        ref.crop(images, torch.zeros_like(masks), K, S=S)


def test_test_inputs_stay_clear_of_the_norm_floor():
    """The GPU tests leave pixels whose float64 vector is shorter than 1e-3 before the normalisation out of the worst-element bar: with
    the tests' seeds that is at most 0.1 % of the masked pixels."""
    for name in ref.CASES:
        c = ref.make_case(name)
        nF, nB, rF, rB = ref.normalnet(c["image"], c["prior_F"], c["prior_B"], c["sd"], *c["cfg"], dtype=torch.float64)
        inside = c["image"].abs().sum(dim=1, keepdim=True) != 0
        assert 0.1 < inside.float().mean().item() < 0.9
        assert bool((inside[:, :, 0, :].any()) and (inside[:, :, :, 0].any()))             # the mask touches two borders
        for r, n in ((rF, nF), (rB, nB)):
            short = ((r < ref.NORM_FLOOR) & inside).sum().item()
            assert short <= 1e-3 * inside.sum().item(), (name, short)
            assert torch.all(n[~inside.expand_as(n)] == 0)
            assert (torch.norm(n, dim=1, keepdim=True)[inside & (r >= ref.NORM_FLOOR)] - 1).abs().max().item() < 1e-12


def test_save_normals_round_trips_through_the_png_reader(tmp_path):
    """save_normals next to a sequence's images/ and smplx/params.pth, then the reader of data.py: the bytes and normal_Ks come back."""
    from PIL import Image
    from soar_amd.data import FrameStore
    g = torch.Generator().manual_seed(2)
    N = 2
    res = dict(normal_F=torch.randint(0, 256, (N, 512, 512, 3), generator=g, dtype=torch.uint8),
               normal_B=torch.randint(0, 256, (N, 512, 512, 3), generator=g, dtype=torch.uint8),
               normal_mask=torch.randint(0, 256, (N, 512, 512), generator=g, dtype=torch.uint8),
               normal_Ks=torch.rand((N, 3, 3), generator=g))
    images = torch.randint(0, 256, (N, 12, 16, 4), generator=g, dtype=torch.uint8)           # RGBA: the alpha is the mask
    (tmp_path / "images").mkdir()
    (tmp_path / "smplx").mkdir()
    for i in range(N):
        Image.fromarray(images[i].numpy(), "RGBA").save(tmp_path / "images" / f"{i:05d}.png")
    body = dict(w2c=torch.eye(4), Ks=torch.eye(3).repeat(N, 1, 1), betas=torch.zeros(10), body_pose=torch.zeros(N, 63),
                global_orient=torch.zeros(N, 3), transl=torch.zeros(N, 3))
    torch.save(body, tmp_path / "smplx" / "params.pth")
    normals.save_normals(res, str(tmp_path))
    got = FrameStore.read_dataroot(str(tmp_path), "smplx")
    for k in ("normal_F", "normal_B", "normal_mask"):
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], res[k].numpy()), k
    assert torch.equal(torch.as_tensor(got["normal_Ks"]), res["normal_Ks"])
    assert np.array_equal(got["images"], images[..., :3].numpy()) and torch.equal(torch.as_tensor(got["Ks"]), body["Ks"])
    # the reader insists on one normal map per image: a result of another length does not pass for this sequence
    normals.save_normals({k: v[:1] for k, v in res.items()}, str(tmp_path / "short"))
    (tmp_path / "normal_F" / "00001.png").unlink()
    with pytest.raises(ValueError, match="must agree"):
        FrameStore.read_dataroot(str(tmp_path), "smplx")
    # without a smplx/params.pth there is nothing to put normal_Ks into: the PNGs are written, the caller keeps normal_Ks
    assert sorted(p.name for p in (tmp_path / "short" / "normal_B").iterdir()) == ["00000.png"] and not (tmp_path / "short" / "smplx").exists()
