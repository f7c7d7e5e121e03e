"""The small synthetic scene of the training-system tests, the guidance stand-in and the reference's step composed by hand -- shared by
tests/test_system_gpu.py and scripts/system_time.py (which builds the same scene at the shipped configs' sizes)."""
import collections
import math
import random
import types

import torch

import data_ref
import lpips_ref
import vae_ref
from soar_amd import synthetic as syn

DEV = torch.device("cuda:0")
# surfels, video frames (5: the fewest the data module splits into train / val / test), frame size, normal-view and SDS-view size
Sizes = collections.namedtuple("Sizes", "P FRAMES H W RES VIEW")
SMALL = Sizes(2000, 5, 48, 64, 32, 32)
CONFIG = Sizes(100000, 5, 1080, 1920, 512, 512)               # TS/configs/gaussiansurfel_imagedream_s{0,1}.yaml


def smpl_parms(poses):
    """the synthetic pose sequence under the reference's smpl_parms key names"""
    fp = poses["full_pose"]
    return {"betas": poses["betas"], "expression": poses["expression"], "global_orient": fp[:, :3], "body_pose": fp[:, 3:66],
            "jaw_pose": fp[:, 66:69], "leye_pose": fp[:, 69:72], "reye_pose": fp[:, 72:75], "left_hand_pose": fp[:, 75:120],
            "right_hand_pose": fp[:, 120:165], "transl": poses["transl"]}


def eps_fn(x, t):
    """a deterministic linear stand-in for the UNet: the (text, uncond) halves as two affine maps of the noisy latents"""
    B = x.shape[0] // 2
    s = 1e-3 * t.to(x.dtype).view(-1, 1, 1, 1)
    return torch.cat([0.7 * x[:B] + 0.1 + s[:B], 0.4 * x[B:] - 0.05 * x[B:].flip(1) - s[B:]])


LOSS = {"lambda_sds": 0.0001, "lambda_recon": 1.0, "lambda_mask": 1.0, "lambda_normal_F": 1.0, "lambda_normal_B": 1.0, "lambda_normal_mask": 1.0,
        "lambda_normal_consistency": 0.01, "lambda_vgg": 0.5, "lambda_sparsity": 0.0, "lambda_position": 0.0, "lambda_opacity": 0.0,
        "lambda_scales": 0.1, "lambda_tv_loss": 0.0, "lambda_depth_tv_loss": 0.0, "lambda_delta": 1.0, "lambda_occ": 0.1, "lambda_curv": 0.5,
        "lambda_offsets": 0.1}
GUIDANCE = {"min_step_percent": 0.02, "max_step_percent": [0, 0.75, 0.25, 2000]}


def system_cfg(stage):
    return {"training_stage": stage, "loss": dict(LOSS), "guidance": dict(GUIDANCE), "renderer": {"use_explicit": False},
            "optimizer": {"params": {"background": {"lr": 0.001}}}, "guidance_type": "imagedream-multiview-diffusion-guidance"}


class SmallNormalViews:
    """The data module's batches with the normal-view tensors (its crop size is fixed at 512) subsampled to RES x RES."""

    def __init__(self, ds, res):
        self.ds, self.res, self.steps = ds, res, []

    def update_step(self, epoch, global_step):
        self.steps.append((epoch, global_step))
        self.ds.update_step(epoch, global_step)

    def collate(self, batch=None, gt_index=None):
        b = self.ds.collate(batch, gt_index=gt_index)
        k = b["gt_normal_res"] // self.res
        for name in ("gt_rays_d", "gt_cam_d", "gt_rays_o", "gt_normal_F", "gt_normal_B", "gt_rgb_crop", "gt_normal_mask", "gt_mask_crop"):
            b[name] = b[name][:, ::k, ::k].contiguous()
        b["gt_normal_res"] = self.res
        b["gt_normal_cx"], b["gt_normal_cy"] = b["gt_normal_cx"] / k, b["gt_normal_cy"] / k
        return b


class Guidance:
    """INTEGRATION.md 5f around ``MultiviewSDS``, with a fixed linear stand-in for the UNet and fixed ``t`` and noises"""

    def __init__(self, sds_module):
        g = torch.Generator().manual_seed(21)
        self.sds, self.ranges, self.calls = sds_module, [], []
        self.t = torch.tensor([400], device=DEV)
        self.noise = torch.randn(4, 4, 8, 8, generator=g).to(DEV)
        self.post = torch.randn(4, 4, 8, 8, generator=g).to(DEV)

    def set_step_range(self, lo, hi):
        self.ranges.append((lo, hi))
        self.sds.set_step_range(lo, hi)

    def __call__(self, rgb, grad_scale=None, normal_flag=False, ref_rgb=None, ref_mask=None, comp_bg=None, **batch):
        self.calls.append({"normal_flag": normal_flag, "ref_rgb": tuple(ref_rgb.shape), "ref_mask": tuple(ref_mask.shape),
                           "comp_bg": tuple(comp_bg.shape), "grad_scale": None if grad_scale is None else tuple(grad_scale.shape),
                           "has_batch": "gt_index" in batch})
        return self.sds(rgb, eps_fn, t=self.t, noise=self.noise, posterior_noise=self.post, grad_scale=grad_scale)


def make_world(sz=SMALL):
    """the scene at the given sizes"""
    P, FRAMES, H, W, RES, VIEW = sz
    from soar_amd import data as D
    from soar_amd import sds
    from soar_amd.lpips import LPIPSVGG
    from soar_amd.renderer import registry
    from soar_amd.smpl_guidance import SMPLGuidance
    import soar_amd.renderer  # noqa: F401
    guide = SMPLGuidance(syn.make_body_model(0, V=2048), smpl_parms(syn.make_pose_sequence(FRAMES, 0)), device=DEV)
    store = D.FrameStore.from_arrays(**data_ref.synthetic_sequence(FRAMES, H, W, seed=3), device=DEV)
    ds = registry.find("mvdream-random-multiview-camera-datamodule")(
        dict(height=VIEW, width=VIEW, batch_size=4, n_view=4, smpl_type="smplx", rays_d_normalize=False, elevation_range=(0, 30),
             camera_distance_range=(0.8, 1.0), fovy_range=(15, 60), camera_perturb=0.0, center_perturb=0.0, up_perturb=0.0), store, "train")
    lpips = LPIPSVGG(lpips_ref.lpips_state_dict(lpips_ref.random_weights(0))).to(DEV)
    enc = sds.LatentEncoder(vae_ref.random_weights(0)).to(DEV)
    torch.manual_seed(5)
    random.seed(5)
    dataset = SmallNormalViews(ds, RES)
    batch = dataset.collate(None, gt_index=2)                  # one batch for the comparisons (the ring keeps it for four further collates)
    return types.SimpleNamespace(guide=guide, store=store, dataset=dataset, lpips=lpips, enc=enc, batch=batch, surf=syn.make_surfels(P, 0))


def build(w, stage, with_guidance=True, geometry_cfg=None, random_aug=True, **kw):
    """a system over a fresh model, renderer and background: the same state every time"""
    from soar_amd import sds
    from soar_amd.background import NeuralEnvironmentMapBackground as Env
    from soar_amd.field import HashMLPField
    from soar_amd.geometry import GaussianSurfelModel
    from soar_amd.renderer import registry
    torch.manual_seed(11)
    random.seed(11)
    geo = GaussianSurfelModel(dict(geometry_cfg or {}))
    geo.create_from_pcd(w.surf.xyz, w.surf.colors.clamp(0.02, 0.98), 10, smpl_guidance=w.guide)
    with torch.no_grad():
        geo._rotation.copy_(w.surf.rot.to(DEV))
        geo._scaling.copy_(torch.log(w.surf.scales[:, :1].to(DEV)))
    field = HashMLPField(geo.aabb.cpu(), log2_hashmap_size=10)                   # a small hash field
    with torch.no_grad():
        field.encoding.hash_table.mul_(300.0)                                    # (an untrained table gives one grey)
    geo.attribute_field = field.to(DEV)
    geo.invalidate()
    geo.training_setup()
    renderer = registry.find("gaussiansurfel-rasterizer")({"use_explicit": False}, geometry=geo)
    env = Env({"random_aug": random_aug, "share_aug_bg": True, "random_aug_prob": 0.5}).to(DEV)
    renderer.background = env
    guidance = None
    if with_guidance:
        guidance = Guidance(sds.MultiviewSDS(w.enc, guidance_scale=5.0, n_view=4, recon_loss=True, recon_std_rescale=0.2, image_size=64).to(DEV))
    system = registry.find("gaussiansurfel-mvdream-system")(system_cfg(stage), geometry=geo, renderer=renderer, background=env, lpips=w.lpips,
                                                             guidance=guidance, **kw)
    return system


def leaves_of(system):
    return [(g["name"], p) for g in system.geometry.optimizer.param_groups for p in g["params"]]


def seeded():
    torch.manual_seed(77)
    random.seed(77)


def grads_of(system):
    return {f"{name}/{i}": (None if p.grad is None else p.grad.detach().clone()) for i, (name, p) in enumerate(leaves_of(system))}


def system_step(system, batch, it):
    """one training_step at global_step = it -> (logged, the leaves' gradients in front of opt.step())"""
    got = {}
    system.global_step = it
    system.before_step = lambda: got.update(grads_of(system))
    seeded()
    system.training_step(dict(batch))
    return dict(system.logged), got


def compose_reference_step(system, batch, it):
    """The reference's step composed by hand from the parent's public functions and plain torch ops, in the reference's order
    (TS/system/gaussian_surfel_mvdream.py:87-463); no optimizer step.  -> (logged, the leaves' gradients)"""
    from soar_amd.geometry import LAMBDAS
    from soar_amd.losses import _AvatarStageLoss as S, avatar_stage_loss, cos_loss, masked_l1
    from soar_amd.system import C
    geo, renderer, lpips, guidance, stage = system.geometry, system.renderer, system.lpips, system.guidance, system.training_stage
    loss_cfg, sds_start = LOSS, (0 if stage == 1 else 500)
    lam = lambda k: C(loss_cfg[k], 0, it)
    log = {}
    batch = dict(batch)
    seeded()
    geo.optimizer.zero_grad(set_to_none=True)
    geo.invalidate()                               # (no optimizer step lies between two composed steps: a fresh activation node)
    head_flag = random.random() < 0.4
    geo.update_learning_rate(it)
    out, gt_out = renderer.batch_forward(batch, mode="gen", head_flag=head_flag, stage=stage)
    log["gauss_num"] = int(geo.get_xyz.shape[0])
    loss_sds, loss = 0.0, 0.0
    if guidance is not None:
        kw = {"comp_bg": gt_out["comp_bg"][0].permute(2, 0, 1)}
        if stage == 1:
            kw.update(ref_rgb=batch["gt_rgb_crop"][0].permute(2, 0, 1), ref_mask=batch["gt_mask_crop"])
        else:
            up = lambda x: torch.nn.functional.interpolate(x[None], (512, 512), mode="bilinear", align_corners=False)[0]
            kw.update(ref_rgb=up(batch["gt_normal_F"][0].permute(2, 0, 1)), ref_mask=up(batch["gt_normal_mask"].float()), normal_flag=True)
        image = out["comp_rgb"] if stage == 1 else out["comp_normal"].clone()
        g_out = guidance(image, grad_scale=torch.exp(-3 * out["comp_occ"].detach()[..., 0]), **kw, **batch)
        for name, value in g_out.items():
            log[f"train/{name}"] = value.detach()
            if name.startswith("loss_"):
                loss_sds = loss_sds + value * lam(name.replace("loss_", "lambda_"))
    active = {k: lam(k) for k in LAMBDAS if loss_cfg[k] > 0.0}
    reg, terms = geo.regularizers(active, scales=geo.attribute_field(geo.get_xyz)["scales"])
    loss = loss + reg
    for i, (k, name) in enumerate((("lambda_position", "train/loss_position"), ("lambda_delta", "train/loss_delta"),
                                   ("lambda_opacity", "train/loss_opacity"), ("lambda_sparsity", "train/loss_sparsity"),
                                   ("lambda_scales", "train/scales"))):
        if k in active:
            log[name] = terms[i].detach()
    G = {k: v.permute(0, 3, 1, 2) for k, v in gt_out.items() if torch.is_tensor(v) and v.dim() == 4}
    SV = {k: v.permute(0, 3, 1, 2) for k, v in out.items() if torch.is_tensor(v) and v.dim() == 4}
    m = batch["gt_mask"]
    blended = batch["gt_rgb"] * m[..., None] + gt_out["rand_bg"] * (1 - m[..., None])
    half = torch.full(tuple(G["comp_rgb"].shape[1:]), 0.5, device=DEV)
    frame = {"render": G["comp_rgb"][0], "mask": G["comp_mask"][0], "normal": half}
    frame_loss, t = avatar_stage_loss(frame, batch["gt_rgb"][0].permute(2, 0, 1).contiguous(), m, half, m[0] > 1e-5,
                                      gt_rgb_blended=blended.permute(0, 3, 1, 2)[0].contiguous(), lambda_recon=lam("lambda_recon"),
                                      lambda_mask=lam("lambda_mask"), lambda_normal=0.0, return_terms=True)
    loss = loss + frame_loss
    log["train/loss_recon"] = (0.8 * t[S.L1] + 0.2 * (1 - t[S.SSIM])) * lam("lambda_recon")
    log["train/loss_mask"] = t[S.L1M] * lam("lambda_mask")
    gm = batch["gt_normal_mask"]
    sel = gm > 1e-5
    chw = lambda x: x.permute(0, 3, 1, 2)
    lp_in = lambda x, mask: (chw(x * mask[..., None]) - 0.5) * 2
    loss_normal = (0.2 * cos_loss(G["comp_normal"][0], chw(batch["gt_normal_F"])[0], sel, thrsh=0, weight=1)
                   + 1 * lpips(lp_in(gt_out["comp_normal"][[0]], gm), lp_in(batch["gt_normal_F"], gm)).mean()) * lam("lambda_normal_F")
    log["train/loss_normal_F"] = loss_normal.detach()
    loss = loss + loss_normal
    selF = sel.float()
    loss_normal = (0.2 * cos_loss(G["comp_normal"][1], chw(batch["gt_normal_B"])[0], sel, thrsh=0, weight=1)
                   + lpips(lp_in(gt_out["comp_normal"][[1]], selF), lp_in(batch["gt_normal_B"], selF)).mean()) * lam("lambda_normal_B")
    log["train/loss_normal_B"] = loss_normal.detach()
    loss = loss + loss_normal
    loss = loss + masked_l1(G["comp_normal_mask"][0], gm) * lam("lambda_normal_mask")
    vgg = lam("lambda_vgg") * lpips((G["comp_rgb"] - 0.5) * 2, (chw(blended) - 0.5) * 2).mean()
    log["train/vgg_loss"] = vgg.detach()
    loss = loss + vgg
    m3 = (m > 0)[..., None].expand_as(gt_out["comp_occ"])
    loss = loss + (1 - gt_out["comp_occ"][m3]).double().mean().float() * lam("lambda_occ")
    thr = math.pi / 10000

    def both_sides(a, b):                       # value counted once, each image's gradient from its own call
        second = cos_loss(b, a.detach(), None, thr)
        return cos_loss(a, b.detach(), None, thr) + (second - second.detach())

    pn = both_sides(G["comp_pred_normal"], G["comp_normal"])
    if it > sds_start:
        pn = (pn + both_sides(SV["comp_pred_normal"], SV["comp_normal"])) * 0.5
    log["train/loss_pred_normal_consistency"] = pn.detach()
    loss = loss + (lam("lambda_normal_consistency") + 0.1 * min(2 * it / 2000, 1)) * pn
    loss_curv = out["comp_curv"].double().abs().mean().float() * lam("lambda_curv")          # (the mean itself, rounded once)
    log["train/loss_curv"] = loss_curv.detach()
    loss = loss + loss_curv
    if torch.is_tensor(loss_sds) and it > sds_start:
        loss_sds.backward(retain_graph=True)
    loss.backward()
    grads = grads_of(system)
    geo.optimizer.zero_grad(set_to_none=True)
    return log, grads
