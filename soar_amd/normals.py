"""Normal-map preprocessing: what makes ``normal_F`` / ``normal_B`` / ``normal_mask`` / ``normal_Ks`` of a sequence (the inputs
``FrameStore.from_arrays`` demands) from its frames, masks and intrinsics, on HIP kernels (csrc/normalnet.hip, csrc/normal_io.hip).

* ``NormalNet(state_dict, ngf=64, n_down=4, n_blocks=9)``: the two generators ``netF`` / ``netB`` of the reference's normal
  checkpoint (keys ``netF.model.<i>.weight|bias`` and ``netF.model.<i>.conv_block.{1,5}.weight|bias``, with or without the Lightning
  ``netG.`` prefix).  ``forward(image, prior_F, prior_B) -> (normal_F, normal_B)``, float32 ``[N,3,H,W]``.
* ``crop_frames(images, masks, Ks)``: per frame the square box of 1.1 x the mask's longer side and its 512 x 512 bilinear crop.
* ``estimate_normals(net, images, masks, Ks, prior_F, prior_B, batch=4)``: crop, networks, bytes, in chunks of ``batch`` frames.
* ``save_normals(result, data_dir)``: ``normal_F/%05d.png`` / ``normal_B/%05d.png`` as RGBA, as ``FrameStore.read_dataroot`` reads them.

The priors are the caller's: ``prior_F`` / ``prior_B`` ``[N,3,512,512]`` are the SMPL-X body's normal map rendered into the crop's
camera (``normal_Ks``) from the front and from behind, in [-1, 1] and zero off the body; zeros are a legal input.  The frames are RGB
(``FrameStore`` holds RGB; the reference flips cv2's BGR, there is nothing to flip here).  HIP only: CPU tensors are refused, there
is no CPU fallback.  (DESIGN.md 9l states the computation in full.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Mapping, Tuple

import torch
from torch import nn

from . import hip_lib
from .hip_lib import _bytes, _stream, _workspace, check

CROP = hip_lib.DATA_CROP
CIN = 6


def layer_keys(ngf: int = 64, n_down: int = 4, n_blocks: int = 9) -> List[Tuple[str, Tuple[int, ...]]]:
    """(key under ``model.``, weight shape) of every convolution of one generator, in the order of the layers.
    Indices: 0 pad, 1 conv, 2 norm, 3 ReLU; three per stride-2 level; one per residual block (conv_block: 0 pad, 1 conv, 2 norm,
    3 ReLU, 4 pad, 5 conv, 6 norm); three per transposed level; pad, conv, tanh."""
    out: List[Tuple[str, Tuple[int, ...]]] = [("1", (ngf, CIN, 7, 7))]
    i = 4
    for d in range(n_down):
        c = ngf << d
        out.append((str(i), (2 * c, c, 3, 3)))
        i += 3
    ct = ngf << n_down
    for _ in range(n_blocks):
        out.append((f"{i}.conv_block.1", (ct, ct, 3, 3)))
        out.append((f"{i}.conv_block.5", (ct, ct, 3, 3)))
        i += 1
    for d in range(n_down):
        c = ngf << (n_down - d)
        out.append((str(i), (c, c // 2, 3, 3)))             # ConvTranspose2d: [Cin][Cout][3][3]
        i += 3
    out.append((str(i + 1), (3, ngf, 7, 7)))
    return out


def state_dict_layout(ngf: int = 64, n_down: int = 4, n_blocks: int = 9) -> Dict[str, Tuple[int, ...]]:
    """key -> shape of every tensor of the checkpoint that belongs to the two generators (weights and biases).  The biases in front
    of an InstanceNorm cancel in it: ``NormalNet`` checks their shapes when they are present and does not need them."""
    layers = layer_keys(ngf, n_down, n_blocks)
    lay: Dict[str, Tuple[int, ...]] = {}
    for net in ("netF", "netB"):
        for idx, (key, shape) in enumerate(layers):
            lay[f"{net}.model.{key}.weight"] = shape
            transposed = 1 + n_down + 2 * n_blocks <= idx < 1 + 2 * n_down + 2 * n_blocks
            lay[f"{net}.model.{key}.bias"] = (shape[1] if transposed else shape[0],)
    return lay


def _check_cfg(ngf: int, n_down: int, n_blocks: int) -> None:
    if not (isinstance(ngf, int) and 8 <= ngf <= 512 and ngf % 8 == 0):
        raise ValueError(f"NormalNet: ngf must be a multiple of 8 in 8 .. 512 (got {ngf})")
    if not (isinstance(n_down, int) and 1 <= n_down <= 4):
        raise ValueError(f"NormalNet: n_down must be 1 .. 4 (got {n_down})")
    if not (isinstance(n_blocks, int) and n_blocks >= 0):
        raise ValueError(f"NormalNet: n_blocks must be >= 0 (got {n_blocks})")


class NormalNet(nn.Module):
    """The reference's ``NormalNet`` in eval mode from its state dict.  The weights are frozen buffers (``netF_w{i}`` / ``netB_w{i}``
    in the order of ``layer_keys`` and ``net*_bias``, the last layer's); move the module with ``.to(device)``.  They are packed for
    the kernels once per device, on first use.  Memory: the module then holds the float32 buffers and their packed copy on the device,
    2 x 1.4 GB for both generators at the shipped configuration, and every ``forward`` takes its workspace (three activation buffers
    of N x H x W x ngf floats: 0.8 GB at N = 4, 512 x 512, ngf 64) from torch's caching allocator, which hands the same block back
    call after call."""

    def __init__(self, state_dict: Mapping[str, torch.Tensor], ngf: int = 64, n_down: int = 4, n_blocks: int = 9):
        super().__init__()
        _check_cfg(ngf, n_down, n_blocks)
        self.ngf, self.n_down, self.n_blocks = ngf, n_down, n_blocks
        sd = dict(state_dict)
        if not any(k.startswith("netF.") for k in sd) and any(k.startswith("netG.netF.") for k in sd):
            sd = {k[len("netG."):]: v for k, v in sd.items() if k.startswith("netG.")}
        lay = state_dict_layout(ngf, n_down, n_blocks)
        layers = layer_keys(ngf, n_down, n_blocks)
        problems = []
        for key, shape in lay.items():
            needed = key.endswith(".weight") or key.endswith(f".model.{layers[-1][0]}.bias")
            if key not in sd:
                if needed:
                    problems.append(f"missing key '{key}' (expected shape {list(shape)})")
                continue
            t = sd[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
                problems.append(f"key '{key}' has shape {list(getattr(t, 'shape', ()))}, expected {list(shape)}")
        if problems:
            missing = all(p.startswith("missing") for p in problems)
            raise (KeyError if missing else ValueError)("NormalNet: " + "; ".join(problems))
        take = lambda k: sd[k].detach().to(torch.float32).contiguous().clone()
        for net in ("netF", "netB"):
            for i, (key, _) in enumerate(layers):
                self.register_buffer(f"{net}_w{i}", take(f"{net}.model.{key}.weight"))
            self.register_buffer(f"{net}_bias", take(f"{net}.model.{layers[-1][0]}.bias"))
        self._n_layers = len(layers)
        self._pack = hip_lib.PackedWeights()
        self.eval()

    def _tensors(self, net: str) -> List[torch.Tensor]:
        return [getattr(self, f"{net}_w{i}") for i in range(self._n_layers)] + [getattr(self, f"{net}_bias")]

    def _packed(self, dev) -> Tuple[torch.Tensor, torch.Tensor]:
        def pack():
            L = hip_lib.lib()
            nb = _bytes(L.soar_normalnet_weights_bytes, "soar_normalnet_weights_bytes", self.ngf, self.n_down, self.n_blocks)
            packed = []
            for net in ("netF", "netB"):
                ts = self._tensors(net)
                arr = (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
                p = _workspace(nb, dev)
                with torch.cuda.device(dev):
                    check(L.soar_normalnet_pack_weights(self.ngf, self.n_down, self.n_blocks, arr, len(ts), p.data_ptr(), nb, _stream(dev)),
                          "soar_normalnet_pack_weights")
                packed.append(p)
            return packed[0], packed[1]

        return self._pack.get(self._tensors("netF") + self._tensors("netB"), dev,
                              f"NormalNet: weights are not on {dev}: move the module with .to('{dev}')", pack)

    def _check(self, image, prior_F, prior_B):
        for name, t in (("image", image), ("prior_F", prior_F), ("prior_B", prior_B)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 3:
                raise ValueError(f"NormalNet: {name} must be an [N, 3, H, W] tensor (got {tuple(getattr(t, 'shape', ()))})")
            if t.shape != image.shape:
                raise ValueError(f"NormalNet: {name} has shape {tuple(t.shape)}, the image {tuple(image.shape)}")
        for name, t in (("image", image), ("prior_F", prior_F), ("prior_B", prior_B)):
            if not t.is_cuda:
                raise RuntimeError(f"NormalNet: {name} is on '{t.device}': soar_amd.normals runs on HIP devices only; there is no CPU fallback")
            if t.dtype != torch.float32:
                raise TypeError(f"NormalNet: {name} must be float32 (got {t.dtype})")
            if t.device != image.device:
                raise ValueError(f"NormalNet: {name} is on {t.device}, the image on {image.device}")
        H, W = image.shape[2:]
        m = 1 << self.n_down
        if H < 4 or W < 4 or H % m or W % m or H // m < 2 or W // m < 2:
            raise ValueError(f"NormalNet: H and W must be multiples of {m}, at least 4, with at least 2 pixels at the bottom level (got {H} x {W})")

    @torch.no_grad()
    def forward(self, image: torch.Tensor, prior_F: torch.Tensor, prior_B: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """image, prior_F, prior_B: float32 ``[N,3,H,W]`` with any strides -> (normal_F, normal_B), unit vectors where the image is
        not zero and exactly 0 elsewhere."""
        self._check(image, prior_F, prior_B)
        dev = image.device
        N, _, H, W = image.shape
        nF = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
        nB = torch.empty_like(nF)
        if N == 0:
            return nF, nB
        wF, wB = self._packed(dev)
        L = hip_lib.lib()
        ws = _workspace(_bytes(L.soar_normalnet_workspace_bytes, "soar_normalnet_workspace_bytes", N, H, W, self.ngf, self.n_down, self.n_blocks), dev)
        a = hip_lib.SoarNormalNetArgs()
        a.N, a.H, a.W, a.ngf, a.n_down, a.n_blocks = N, H, W, self.ngf, self.n_down, self.n_blocks
        a.image, a.prior_F, a.prior_B = image.data_ptr(), prior_F.data_ptr(), prior_B.data_ptr()
        for i in range(4):
            a.image_stride[i], a.prior_F_stride[i], a.prior_B_stride[i] = image.stride(i), prior_F.stride(i), prior_B.stride(i)
        a.weights_F, a.weights_B = wF.data_ptr(), wB.data_ptr()
        a.normal_F, a.normal_B = nF.data_ptr(), nB.data_ptr()
        with torch.cuda.device(dev):
            check(L.soar_normalnet_forward(C.byref(a), ws.data_ptr(), ws.numel(), _stream(dev)), "soar_normalnet_forward")
        return nF, nB


def _frames(images, masks, what: str):
    """-> (rgb view [N,H,W,3], mask view [N,H,W]) of uint8 device tensors; RGBA frames carry their own mask."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[-1] not in (3, 4):
        raise ValueError(f"{what}: images must be a uint8 [N,H,W,3] (or RGBA [N,H,W,4]) tensor (got {tuple(getattr(images, 'shape', ()))})")
    if not images.is_cuda:
        raise RuntimeError(f"{what}: images are on '{images.device}': soar_amd.normals runs on HIP devices only; there is no CPU fallback")
    if images.shape[-1] == 4 and masks is None:
        masks = images[..., 3]
    if masks is None:
        raise ValueError(f"{what}: RGB frames need masks [N,H,W]")
    images = images[..., :3]
    if not isinstance(masks, torch.Tensor) or masks.shape != images.shape[:3]:
        raise ValueError(f"{what}: masks must be [N,H,W] = {tuple(images.shape[:3])} (got {tuple(getattr(masks, 'shape', ()))})")
    if not masks.is_cuda or masks.device != images.device:
        raise RuntimeError(f"{what}: masks are on '{masks.device}', the images on '{images.device}'; there is no CPU fallback")
    if images.dtype != torch.uint8 or masks.dtype != torch.uint8:
        raise TypeError(f"{what}: images and masks must be uint8 (got {images.dtype}, {masks.dtype})")
    return images, masks


def _strides(t: torch.Tensor):
    return (C.c_int64 * t.dim())(*t.stride())


def _crop_launch(images, masks, Ks):
    dev = images.device
    N, H, W = masks.shape
    Ks = torch.as_tensor(Ks, dtype=torch.float32).to(dev)
    Ks = (Ks.expand(N, 3, 3) if Ks.dim() == 2 else Ks).contiguous()
    if Ks.shape != (N, 3, 3):
        raise ValueError(f"crop_frames: Ks must be [N,3,3] or [3,3] (got {tuple(Ks.shape)})")
    image = torch.empty((N, 3, CROP, CROP), dtype=torch.float32, device=dev)
    mask = torch.empty((N, 1, CROP, CROP), dtype=torch.float32, device=dev)
    boxes = torch.empty((N, 4), dtype=torch.float64, device=dev)
    nKs = torch.empty((N, 3, 3), dtype=torch.float32, device=dev)
    status = torch.zeros((N,), dtype=torch.int32, device=dev)
    if N:
        L = hip_lib.lib()
        with torch.cuda.device(dev):
            s = _stream(dev)
            check(L.soar_normal_crop_boxes(N, H, W, CROP, masks.data_ptr(), _strides(masks), Ks.data_ptr(), boxes.data_ptr(), nKs.data_ptr(),
                                           status.data_ptr(), s), "soar_normal_crop_boxes")
            check(L.soar_normal_crop_sample(N, H, W, CROP, images.data_ptr(), _strides(images), masks.data_ptr(), _strides(masks),
                                            boxes.data_ptr(), image.data_ptr(), mask.data_ptr(), s), "soar_normal_crop_sample")
    return image, mask, nKs, boxes.to(torch.float32), status


def _raise_on_status(status: torch.Tensor, first: int = 0) -> None:
    st = status.cpu()
    bad = torch.nonzero(st).reshape(-1).tolist()
    if bad:
        empty = [first + i for i in bad if int(st[i]) == 1]
        if empty:
            raise ValueError(f"frame {empty[0]} has an empty mask (frames without a mask: {empty}): no crop box")
        single = [first + i for i in bad]
        raise ValueError(f"frame {single[0]}: the mask is a single pixel (frames: {single}): no crop box")


def crop_frames(images: torch.Tensor, masks, Ks) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """images uint8 ``[N,H,W,3]`` RGB (or RGBA, masks None), masks uint8 ``[N,H,W]`` (a soft mask counts as / 255), Ks ``[N,3,3]`` ->
    (image ``[N,3,512,512]`` = the crop of (rgb * 2 - 1) * mask, mask ``[N,1,512,512]``, normal_Ks ``[N,3,3]``, boxes ``[N,4]``
    (x1, y1, x2, y2)).  Two launches for all frames; the frames' status words are looked at once, at the end: an empty mask raises."""
    images, masks = _frames(images, masks, "crop_frames")
    image, mask, nKs, boxes, status = _crop_launch(images, masks, Ks)
    _raise_on_status(status)
    return image, mask, nKs, boxes


def normal_bytes(normal_F: torch.Tensor, normal_B: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """float32 ``[N,3,H,W]`` x 2 and the cropped mask ``[N,1,H,W]`` -> uint8 ``[N,H,W,3]`` x 2 and ``[N,H,W]``:
    ``trunc(((n + 1) / 2 * mask) * 255)`` and ``trunc(mask * 255)``, one launch."""
    for t in (normal_F, normal_B, mask):
        if not t.is_cuda:
            raise RuntimeError(f"normal_bytes: a tensor is on '{t.device}': soar_amd.normals runs on HIP devices only; there is no CPU fallback")
    N, _, H, W = normal_F.shape
    if normal_B.shape != normal_F.shape or normal_F.shape[1] != 3 or mask.numel() != N * H * W:
        raise ValueError("normal_bytes: need normal_F, normal_B [N,3,H,W] and mask [N,1,H,W]")
    normal_F, normal_B, mask = (t.to(torch.float32).contiguous() for t in (normal_F, normal_B, mask))
    dev = normal_F.device
    oF = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    oB = torch.empty_like(oF)
    oM = torch.empty((N, H, W), dtype=torch.uint8, device=dev)
    if N:
        with torch.cuda.device(dev):
            check(hip_lib.lib().soar_normal_crop_bytes(N, H, W, normal_F.data_ptr(), normal_B.data_ptr(), mask.data_ptr(), oF.data_ptr(),
                                                       oB.data_ptr(), oM.data_ptr(), _stream(dev)),
                  "soar_normal_crop_bytes")
    return oF, oB, oM


def estimate_normals(net: NormalNet, images, masks, Ks, prior_F: torch.Tensor, prior_B: torch.Tensor, batch: int = 4) -> Dict[str, torch.Tensor]:
    """The preprocessing stage for a whole sequence -> dict(normal_F, normal_B uint8 ``[N,512,512,3]``, normal_mask uint8
    ``[N,512,512]``, normal_Ks float32 ``[N,3,3]``), device tensors of the shapes ``FrameStore.from_arrays`` takes.  ``batch`` frames
    go through the networks per call; nothing is read back between the chunks: the masks' status words are looked at once, at the end."""
    images, masks = _frames(images, masks, "estimate_normals")
    N = images.shape[0]
    if batch < 1:
        raise ValueError(f"estimate_normals: batch must be >= 1 (got {batch})")
    for name, t in (("prior_F", prior_F), ("prior_B", prior_B)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (N, 3, CROP, CROP):
            raise ValueError(f"estimate_normals: {name} must be [{N},3,{CROP},{CROP}] (got {tuple(getattr(t, 'shape', ()))})")
    dev = images.device
    Ks = torch.as_tensor(Ks, dtype=torch.float32).to(dev)
    Ks = (Ks.expand(N, 3, 3) if Ks.dim() == 2 else Ks).contiguous()
    out = dict(normal_F=torch.empty((N, CROP, CROP, 3), dtype=torch.uint8, device=dev),
               normal_B=torch.empty((N, CROP, CROP, 3), dtype=torch.uint8, device=dev),
               normal_mask=torch.empty((N, CROP, CROP), dtype=torch.uint8, device=dev),
               normal_Ks=torch.empty((N, 3, 3), dtype=torch.float32, device=dev))
    status = torch.zeros((N,), dtype=torch.int32, device=dev)
    for i in range(0, N, batch):
        j = min(i + batch, N)
        image, mask, nKs, _, st = _crop_launch(images[i:j], masks[i:j], Ks[i:j])
        nF, nB = net(image, prior_F[i:j], prior_B[i:j])
        bF, bB, bM = normal_bytes(nF, nB, mask)
        out["normal_F"][i:j], out["normal_B"][i:j], out["normal_mask"][i:j], out["normal_Ks"][i:j] = bF, bB, bM, nKs
        status[i:j] = st
    _raise_on_status(status)
    return out


def _save_normals_on_device(result: Mapping[str, torch.Tensor], data_dir: str) -> None:
    from .png import write_png_files
    mask = result["normal_mask"].detach()
    for name in ("normal_F", "normal_B"):
        rgb = result[name].detach()
        if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[-1] != 3 or mask.shape != rgb.shape[:3] or mask.dtype != torch.uint8:
            raise ValueError(f"save_normals: {name} must be uint8 [N,H,W,3] and normal_mask uint8 [N,H,W]")
        os.makedirs(os.path.join(data_dir, name), exist_ok=True)
        write_png_files([os.path.join(data_dir, name, f"{i:05d}.png") for i in range(rgb.shape[0])], torch.cat([rgb, mask[..., None]], dim=-1))


def _save_normals_on_host(result: Mapping[str, torch.Tensor], data_dir: str) -> None:
    from PIL import Image
    import numpy as np
    nM = result["normal_mask"].detach().cpu().numpy()
    for name in ("normal_F", "normal_B"):
        os.makedirs(os.path.join(data_dir, name), exist_ok=True)
        rgb = result[name].detach().cpu().numpy()
        if rgb.dtype != np.uint8 or rgb.ndim != 4 or rgb.shape[-1] != 3 or nM.shape != rgb.shape[:3]:
            raise ValueError(f"save_normals: {name} must be uint8 [N,H,W,3] and normal_mask [N,H,W]")
        for i in range(rgb.shape[0]):
            Image.fromarray(np.concatenate([rgb[i], nM[i][..., None]], axis=-1), "RGBA").save(os.path.join(data_dir, name, f"{i:05d}.png"))


def save_normals(result: Mapping[str, torch.Tensor], data_dir: str, device_png: bool = False) -> None:
    """Writes ``normal_F/%05d.png`` and ``normal_B/%05d.png`` (RGBA: the normal's bytes and the normal mask) under ``data_dir``, the
    layout ``FrameStore.read_dataroot`` reads, and, as the reference does, puts ``normal_Ks`` into ``data_dir/smplx/params.pth`` next
    to ``Ks`` when that file exists (it holds the body's parameters and is not made here; without it ``normal_Ks`` stays with the
    caller).  ``device_png=True`` joins the channels and makes the PNG files on the device (``png.write_png_files``; the maps must then
    be on a HIP device): the same names and pixels, and only compressed bytes are copied to the host."""
    (_save_normals_on_device if device_png else _save_normals_on_host)(result, data_dir)
    params = os.path.join(data_dir, "smplx", "params.pth")
    if "normal_Ks" in result and os.path.exists(params):
        body = torch.load(params, map_location="cpu")
        body["normal_Ks"] = result["normal_Ks"].detach().to("cpu", torch.float32)
        torch.save(body, params)
