"""torch-CPU restatement of the reference's training data module, to be read side by side with it:
TS/data/uncond_multiview.py:137-154 (split), :246-313 (crops and per-frame rays), :340-681 (collate), :68-90
(get_projection_matrix_cxcy), and the four threestudio helpers it imports (get_ray_directions, get_rays, get_projection_matrix,
get_mvp_matrix: threestudio/utils/ops.py, whose submodule directory is empty in the reference tree).  The yardstick of
soar_amd/data.py and csrc/data.hip: float32 on the CPU, torch's own grid_sample / nonzero / normalize / inverse / linspace."""
import bisect
import math
import random
from types import SimpleNamespace

import torch
import torch.nn.functional as F

CROP = 512


# ---- threestudio/utils/ops.py -------------------------------------------------------------------------------------------------
def get_ray_directions(H, W, focal, principal=None):
    if isinstance(focal, float):
        fx, fy, cx, cy = focal, focal, W / 2, H / 2
    else:
        (fx, fy), (cx, cy) = focal, principal
    i, j = torch.meshgrid(torch.arange(W, dtype=torch.float32) + 0.5, torch.arange(H, dtype=torch.float32) + 0.5, indexing="xy")
    return torch.stack([(i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)], -1)


def get_rays(directions, c2w, normalize=True):
    """the [B,H,W,3] / [B,4,4] case with keepdim=True"""
    rays_d = (directions[:, :, :, None, :] * c2w[:, None, None, :3, :3]).sum(-1)
    rays_o = c2w[:, None, None, :3, 3].expand(rays_d.shape)
    if normalize:
        rays_d = F.normalize(rays_d, dim=-1)
    return rays_o, rays_d


def get_projection_matrix(fovy, aspect_wh, near, far, cxcy=None, img_wh=None):
    """get_projection_matrix, and with cxcy / img_wh the reference's get_projection_matrix_cxcy (:68-90)"""
    proj = torch.zeros(fovy.shape[0], 4, 4, dtype=torch.float32)
    proj[:, 0, 0] = 1.0 / (torch.tan(fovy / 2.0) * aspect_wh)
    proj[:, 1, 1] = -1.0 / torch.tan(fovy / 2.0)
    proj[:, 2, 2] = -(far + near) / (far - near)
    proj[:, 2, 3] = -2.0 * far * near / (far - near)
    proj[:, 3, 2] = -1.0
    if cxcy is not None and img_wh is not None:
        (cx, cy), (W, H) = cxcy, img_wh
        proj[:, 0, 2] = -(2.0 * cx - W) / W
        proj[:, 1, 2] = -(2.0 * cy - H) / H
    return proj


def get_mvp_matrix(c2w, proj):
    w2c = torch.zeros(c2w.shape[0], 4, 4).to(c2w)
    w2c[:, :3, :3] = c2w[:, :3, :3].permute(0, 2, 1)
    w2c[:, :3, 3:] = -c2w[:, :3, :3].permute(0, 2, 1) @ c2w[:, :3, 3:]
    w2c[:, 3, 3] = 1.0
    return proj @ w2c


# ---- :137-154 -----------------------------------------------------------------------------------------------------------------
def split_indices(scene_length, split):
    num_val = scene_length // 5
    length = int(1 / (num_val) * scene_length)
    offset = length // 2
    val_list = list(range(scene_length))[offset::length]
    train_list = list(set(range(scene_length)) - set(val_list))
    test_list = val_list[:len(val_list) // 2]
    val_list = val_list[len(val_list) // 2:]
    return {"train": train_list, "val": val_list, "test": test_list}[split]


# ---- :190-203: the float video the reference keeps on the host ----------------------------------------------------------------
def float_frames(images_u8, masks_u8):
    """images [N,H,W,3] uint8, masks [N,H,W] uint8 (0 / 1) -> frames_img (already multiplied by the mask), frames_mask"""
    mask = masks_u8.float()
    return images_u8.float() / 255.0 * mask[..., None], mask


def mask_bbox(mask):
    idx = torch.nonzero(mask)
    return torch.cat([idx.min(0)[0].flip(0), idx.max(0)[0].flip(0)])


# ---- :246-313 -----------------------------------------------------------------------------------------------------------------
def crop_grid(bbox_xyxy, H, W):
    """-> the sampling grid [1,CROP,CROP,2] of one frame and the float box"""
    bbox = bbox_xyxy
    bbox_c = bbox[:2] + (bbox[2:] - bbox[:2]) / 2.0
    bbox_s = max((bbox[2] - bbox[0]).item(), (bbox[3] - bbox[1]).item()) * 1.1
    bbox = torch.cat([bbox_c - bbox_s / 2.0, bbox_c + bbox_s / 2.0])
    grid = torch.stack(torch.meshgrid(torch.linspace(bbox[0].item(), bbox[2].item(), CROP) / W,
                                      torch.linspace(bbox[1].item(), bbox[3].item(), CROP) / H, indexing="xy"), dim=-1)[None] * 2.0 - 1.0
    return grid, bbox


def crop_frame(img, mask):
    """img [H,W,3] float (masked), mask [H,W] float -> cropped_img [CROP,CROP,3], cropped_mask [CROP,CROP], grid"""
    grid, _ = crop_grid(mask_bbox(mask), img.shape[0], img.shape[1])
    ci = F.grid_sample(img[None].permute(0, 3, 1, 2), grid, mode="bilinear", align_corners=False)
    cm = F.grid_sample(mask[None, ..., None].permute(0, 3, 1, 2), grid, mode="bilinear", align_corners=False)
    return ci[0].permute(1, 2, 0), cm[0, 0], grid


def crop_fractions(grid, H, W):
    """the fractional parts of the pixel coordinates grid_sample derives from `grid` (to tell where a tap may flip)"""
    x = (grid[0, ..., 0] + 1) * (W / 2) - 0.5
    y = (grid[0, ..., 1] + 1) * (H / 2) - 0.5
    return x - x.floor(), y - y.floor()


def frame_rays_d(normal_K, extrinsic):
    d = get_ray_directions(H=CROP, W=CROP, focal=(normal_K[0, 0], normal_K[1, 1]), principal=(normal_K[0, 2], normal_K[1, 2]))[None]
    return get_rays(d, torch.inverse(extrinsic).unsqueeze(0), normalize=True)[1]


# ---- the dataset's state and :340-681 -----------------------------------------------------------------------------------------
CFG_DEFAULTS = dict(height=64, width=64, batch_size=1, resolution_milestones=(), elevation_range=(-10, 90), azimuth_range=(-180, 180),
                    camera_distance_range=(1, 1.5), fovy_range=(40, 70), camera_perturb=0.1, center_perturb=0.2, up_perturb=0.02,
                    light_position_perturb=1.0, light_distance_range=(0.8, 1.5), light_sample_strategy="dreamfusion",
                    relative_radius=True, n_view=1, zoom_range=(1.0, 1.0), smpl_type="smplx", index_range=(0, 1), rays_d_normalize=True)


def make_state(cfg, images, masks, normal_F, normal_B, normal_mask, Ks, normal_Ks, w2c, smpl_parms, split="train", with_crops=True):
    """what RandomMultiviewCameraIterableDataset.__init__ leaves in `self` (w2c: the extrinsic AFTER `extrinsic[1:3] *= -1`)"""
    s = SimpleNamespace(cfg=SimpleNamespace(**dict(CFG_DEFAULTS, **cfg)))
    c = s.cfg
    s.heights = [c.height] if isinstance(c.height, int) else list(c.height)
    s.widths = [c.width] if isinstance(c.width, int) else list(c.width)
    s.batch_sizes = [c.batch_size] if isinstance(c.batch_size, int) else list(c.batch_size)
    s.resolution_milestones = [-1] + list(c.resolution_milestones)
    s.directions_unit_focals = [get_ray_directions(H=h, W=w, focal=1.0) for h, w in zip(s.heights, s.widths)]
    s.elevation_range, s.azimuth_range = c.elevation_range, c.azimuth_range
    s.camera_distance_range, s.fovy_range, s.zoom_range = c.camera_distance_range, c.fovy_range, c.zoom_range
    update_step(s, 0)
    s.frames_img, s.frames_mask = float_frames(images, masks)
    s.frames_normal_F, s.frames_normal_B = normal_F.float() / 255.0, normal_B.float() / 255.0
    s.frames_normal_mask = normal_mask.float() / 255.0
    s.n_frames = len(s.frames_img)
    s.gt_height, s.gt_width = images.shape[1], images.shape[2]
    s.index_list = split_indices(s.n_frames, split)
    s.extrinsic, s.intrinsics, s.normal_intrinsics, s.smpl_parms = w2c, Ks, normal_Ks, smpl_parms
    if with_crops:
        crops = [crop_frame(i, m) for i, m in zip(s.frames_img, s.frames_mask)]
        s.frames_img_crop = torch.stack([c_[0] for c_ in crops])
        s.frames_mask_crop = torch.stack([c_[1] for c_ in crops])
        s.frames_rays_d = torch.cat([frame_rays_d(normal_Ks[i], w2c) for i in range(s.n_frames)])
    return s


def update_step(s, global_step):
    size_ind = bisect.bisect_right(s.resolution_milestones, global_step) - 1
    s.height, s.width, s.batch_size = s.heights[size_ind], s.widths[size_ind], s.batch_sizes[size_ind]
    s.directions_unit_focal = s.directions_unit_focals[size_ind]


def collate(s, gt_index=None):
    """:340-681 (gt_index given: ValDataset.__getitem__, which makes the same draws without the frame's)"""
    cfg = s.cfg
    assert s.batch_size % cfg.n_view == 0
    real_batch_size = s.batch_size // cfg.n_view
    if gt_index is None:
        gt_index = s.index_list[torch.randint(0, len(s.index_list), (1,)).item()]
    gt_c2w = torch.inverse(s.extrinsic).unsqueeze(0)
    gt_fx, gt_fy = s.intrinsics[gt_index, 0, 0], s.intrinsics[gt_index, 1, 1]
    gt_cx, gt_cy = s.intrinsics[gt_index, 0, 2], s.intrinsics[gt_index, 1, 2]
    gt_fovy = (2 * torch.atan(s.gt_height / (2 * gt_fy))).unsqueeze(0)
    gt_fovx = (2 * torch.atan(s.gt_width / (2 * gt_fx))).unsqueeze(0)
    gt_cx, gt_cy = gt_cx.unsqueeze(0), gt_cy.unsqueeze(0)
    gt_near = 0.1
    if cfg.smpl_type == "smplx":
        gt_near = s.smpl_parms["transl"][gt_index][-1].item() - 5.0
    extra = {} if cfg.smpl_type == "smpl" else {"cxcy": (gt_cx.item(), gt_cy.item()), "img_wh": (s.gt_width, s.gt_height)}
    gt_proj_mtx = get_projection_matrix(gt_fovy, s.gt_width / s.gt_height, gt_near, 1000.0, **extra)
    gt_normal_res = CROP
    nK = s.normal_intrinsics[gt_index]
    gt_normal_fovy = (2 * torch.atan(gt_normal_res / (2 * nK[1, 1]))).unsqueeze(0)
    gt_normal_fovx = (2 * torch.atan(gt_normal_res / (2 * nK[0, 0]))).unsqueeze(0)
    gt_mvp_mtx = get_mvp_matrix(gt_c2w, gt_proj_mtx)
    gt_directions = get_ray_directions(H=gt_normal_res, W=gt_normal_res, focal=(nK[0, 0], nK[1, 1]), principal=(nK[0, 2], nK[1, 2]))[None]
    gt_rays_o, gt_rays_d = get_rays(gt_directions, gt_c2w, normalize=True)

    if random.random() < 0.5:
        elevation_deg = (torch.rand(real_batch_size) * (s.elevation_range[1] - s.elevation_range[0])
                         + s.elevation_range[0]).repeat_interleave(cfg.n_view, dim=0)
        elevation = elevation_deg * math.pi / 180
    else:
        pct = [(s.elevation_range[0] + 90.0) / 180.0, (s.elevation_range[1] + 90.0) / 180.0]
        elevation = torch.asin(2 * (torch.rand(real_batch_size) * (pct[1] - pct[0]) + pct[0]) - 1.0).repeat_interleave(cfg.n_view, dim=0)
        elevation_deg = elevation / math.pi * 180.0
    azimuth_deg = (torch.rand(real_batch_size).reshape(-1, 1) + torch.arange(cfg.n_view).reshape(1, -1)).reshape(-1) / cfg.n_view * (
        s.azimuth_range[1] - s.azimuth_range[0]) + s.azimuth_range[0]
    azimuth = azimuth_deg * math.pi / 180
    fovy_deg = (torch.rand(real_batch_size) * (s.fovy_range[1] - s.fovy_range[0]) + s.fovy_range[0]).repeat_interleave(cfg.n_view, dim=0)
    fovy = fovy_deg * math.pi / 180
    camera_distances = (torch.rand(real_batch_size) * (s.camera_distance_range[1] - s.camera_distance_range[0])
                        + s.camera_distance_range[0]).repeat_interleave(cfg.n_view, dim=0)
    if cfg.relative_radius:
        camera_distances = 1 / torch.tan(0.5 * fovy) * camera_distances
    zoom = (torch.rand(real_batch_size) * (s.zoom_range[1] - s.zoom_range[0]) + s.zoom_range[0]).repeat_interleave(cfg.n_view, dim=0)
    fovy = fovy * zoom
    fovy_deg = fovy_deg * zoom
    camera_positions = torch.stack([camera_distances * torch.cos(elevation) * torch.cos(azimuth),
                                    camera_distances * torch.cos(elevation) * torch.sin(azimuth),
                                    camera_distances * torch.sin(elevation)], dim=-1)
    center = torch.zeros_like(camera_positions)
    up = torch.as_tensor([0, 0, 1], dtype=torch.float32)[None, :].repeat(s.batch_size, 1)
    camera_perturb = (torch.rand(real_batch_size, 3) * 2 * cfg.camera_perturb - cfg.camera_perturb).repeat_interleave(cfg.n_view, dim=0)
    camera_positions = camera_positions + camera_perturb
    center = center + (torch.randn(real_batch_size, 3) * cfg.center_perturb).repeat_interleave(cfg.n_view, dim=0)
    up = up + (torch.randn(real_batch_size, 3) * cfg.up_perturb).repeat_interleave(cfg.n_view, dim=0)
    light_distances = (torch.rand(real_batch_size) * (cfg.light_distance_range[1] - cfg.light_distance_range[0])
                       + cfg.light_distance_range[0]).repeat_interleave(cfg.n_view, dim=0)
    if cfg.light_sample_strategy == "dreamfusion":
        light_direction = F.normalize(camera_positions + torch.randn(real_batch_size, 3).repeat_interleave(cfg.n_view, dim=0)
                                      * cfg.light_position_perturb, dim=-1)
        light_positions = light_direction * light_distances[:, None]
    elif cfg.light_sample_strategy == "magic3d":
        local_z = F.normalize(camera_positions, dim=-1)
        local_x = F.normalize(torch.stack([local_z[:, 1], -local_z[:, 0], torch.zeros_like(local_z[:, 0])], dim=-1), dim=-1)
        local_y = F.normalize(torch.cross(local_z, local_x, dim=-1), dim=-1)
        rot = torch.stack([local_x, local_y, local_z], dim=-1)
        light_azimuth = (torch.rand(real_batch_size) * math.pi - 2 * math.pi).repeat_interleave(cfg.n_view, dim=0)
        light_elevation = (torch.rand(real_batch_size) * math.pi / 3 + math.pi / 6).repeat_interleave(cfg.n_view, dim=0)
        light_positions_local = torch.stack([light_distances * torch.cos(light_elevation) * torch.cos(light_azimuth),
                                             light_distances * torch.cos(light_elevation) * torch.sin(light_azimuth),
                                             light_distances * torch.sin(light_elevation)], dim=-1)
        light_positions = (rot @ light_positions_local[:, :, None])[:, :, 0]
    else:
        raise ValueError(f"Unknown light sample strategy: {cfg.light_sample_strategy}")
    lookat = F.normalize(center - camera_positions, dim=-1)
    right = F.normalize(torch.cross(lookat, up, dim=-1), dim=-1)
    up = F.normalize(torch.cross(right, lookat, dim=-1), dim=-1)
    c2w3x4 = torch.cat([torch.stack([right, up, -lookat], dim=-1), camera_positions[:, :, None]], dim=-1)
    c2w = torch.cat([c2w3x4, torch.zeros_like(c2w3x4[:, :1])], dim=1)
    c2w[:, 3, 3] = 1.0
    focal_length = 0.5 * s.height / torch.tan(0.5 * fovy)
    directions = s.directions_unit_focal[None, :, :, :].repeat(s.batch_size, 1, 1, 1)
    directions[:, :, :, :2] = directions[:, :, :, :2] / focal_length[:, None, None, None]
    rays_o, rays_d = get_rays(directions, c2w, normalize=cfg.rays_d_normalize)
    proj_mtx = get_projection_matrix(fovy, s.width / s.height, 0.1, 1000.0)
    mvp_mtx = get_mvp_matrix(c2w, proj_mtx)
    smpl_collate = {"betas": s.smpl_parms["betas"][None], "body_pose": s.smpl_parms["body_pose"][gt_index][None],
                    "global_orient": s.smpl_parms["global_orient"][gt_index][None], "transl": s.smpl_parms["transl"][gt_index][None]}
    out = {"rays_o": rays_o, "rays_d": rays_d, "frames_rays_d": getattr(s, "frames_rays_d", None), "cam_d": directions, "mvp_mtx": mvp_mtx,
           "camera_positions": camera_positions, "c2w": c2w, "light_positions": light_positions, "elevation": elevation_deg,
           "azimuth": azimuth_deg, "camera_distances": camera_distances, "height": s.height, "width": s.width, "fovy": fovy,
           "gt_index": gt_index, "gt_rays_o": gt_rays_o, "gt_rays_d": gt_rays_d, "gt_cam_d": gt_directions, "gt_mvp_mtx": gt_mvp_mtx,
           "gt_c2w": gt_c2w, "gt_fovx": gt_fovx, "gt_fovy": gt_fovy, "gt_cx": gt_cx, "gt_cy": gt_cy, "gt_normal_fovx": gt_normal_fovx,
           "gt_normal_fovy": gt_normal_fovy, "gt_normal_cx": nK[0, 2].unsqueeze(0), "gt_normal_cy": nK[1, 2].unsqueeze(0),
           "gt_normal_res": gt_normal_res, "gt_near": torch.tensor(gt_near).unsqueeze(0), "gt_height": s.gt_height,
           "gt_width": s.gt_width, "gt_smpl": smpl_collate, "gt_rgb": s.frames_img[gt_index:gt_index + 1],
           "gt_mask": s.frames_mask[gt_index:gt_index + 1]}
    if hasattr(s, "frames_img_crop"):
        out["gt_rgb_crop"] = s.frames_img_crop[gt_index:gt_index + 1]
        out["gt_mask_crop"] = s.frames_mask_crop[gt_index:gt_index + 1]
    out["gt_normal_F"] = s.frames_normal_F[gt_index:gt_index + 1]
    out["gt_normal_B"] = s.frames_normal_B[gt_index:gt_index + 1]
    out["gt_normal_mask"] = s.frames_normal_mask[gt_index:gt_index + 1]
    return out


# the keys of :635-680, in the reference's order
KEYS = ("rays_o", "rays_d", "frames_rays_d", "cam_d", "mvp_mtx", "camera_positions", "c2w", "light_positions", "elevation", "azimuth",
        "camera_distances", "height", "width", "fovy", "gt_index", "gt_rays_o", "gt_rays_d", "gt_cam_d", "gt_mvp_mtx", "gt_c2w",
        "gt_fovx", "gt_fovy", "gt_cx", "gt_cy", "gt_normal_fovx", "gt_normal_fovy", "gt_normal_cx", "gt_normal_cy", "gt_normal_res",
        "gt_near", "gt_height", "gt_width", "gt_smpl", "gt_rgb", "gt_mask", "gt_rgb_crop", "gt_mask_crop", "gt_normal_F", "gt_normal_B",
        "gt_normal_mask")


# ---- synthetic sequences (seeded; the tests' inputs) --------------------------------------------------------------------------
def synthetic_sequence(N, H, W, seed=0, empty=()):
    """N frames of noise with blob masks: frame 0's blob touches the image border (the crop box leaves the image), frame 1's mask is
    ONE pixel, the others are ellipses; frames listed in `empty` have no mask at all."""
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    masks = torch.zeros(N, H, W, dtype=torch.uint8)
    for n in range(N):
        if n in empty:
            continue
        if n == 0:
            cx, cy, rx, ry = 0.12 * W, 0.5 * H, 0.2 * W, 0.45 * H              # cut by the left border
        elif n == 1:
            masks[n, H // 3, (2 * W) // 3] = 1
            continue
        else:
            u = torch.rand(4, generator=g)
            cx, cy = (0.3 + 0.4 * u[0]) * W, (0.35 + 0.3 * u[1]) * H
            rx, ry = (0.05 + 0.15 * u[2]) * W, (0.1 + 0.3 * u[3]) * H
        masks[n] = ((((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2) <= 1.0).to(torch.uint8)
    normal_F = torch.randint(0, 256, (N, CROP, CROP, 3), generator=g, dtype=torch.uint8)
    normal_B = torch.randint(0, 256, (N, CROP, CROP, 3), generator=g, dtype=torch.uint8)
    normal_mask = torch.randint(0, 256, (N, CROP, CROP), generator=g, dtype=torch.uint8)
    f = 1.2 * H
    Ks = torch.tensor([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]]).repeat(N, 1, 1)
    Ks[:, 0, 2] += torch.rand(N, generator=g) * 8 - 4
    Ks[:, 1, 2] += torch.rand(N, generator=g) * 8 - 4
    normal_Ks = torch.tensor([[1400.0, 0.0, 256.0], [0.0, 1400.0, 256.0], [0.0, 0.0, 1.0]]).repeat(N, 1, 1)
    normal_Ks[:, 0, 0] += torch.rand(N, generator=g) * 200
    normal_Ks[:, 1, 1] += torch.rand(N, generator=g) * 200
    normal_Ks[:, :2, 2] += torch.rand(N, 2, generator=g) * 20 - 10
    ang = 0.3
    w2c = torch.tensor([[math.cos(ang), 0.0, math.sin(ang), 0.05], [0.0, 1.0, 0.0, -0.1], [-math.sin(ang), 0.0, math.cos(ang), 3.0],
                        [0.0, 0.0, 0.0, 1.0]])
    w2c[1:3] *= -1
    smpl = {"betas": torch.randn(10, generator=g), "body_pose": torch.randn(N, 63, generator=g) * 0.1,
            "global_orient": torch.randn(N, 3, generator=g) * 0.1, "transl": torch.cat([torch.randn(N, 2, generator=g) * 0.1,
                                                                                      8.0 + torch.rand(N, 1, generator=g)], dim=1)}
    return dict(images=images, masks=masks, normal_F=normal_F, normal_B=normal_B, normal_mask=normal_mask, Ks=Ks, normal_Ks=normal_Ks,
                w2c=w2c, smpl_parms=smpl)
