"""``SurfelMVDreamSystem``: SOAR's two-stage training step over the modules of this package.

The counterpart of the reference's ``SurfelMVDreamSystem`` (TS/system/gaussian_surfel_mvdream.py:34-474) without Lightning or
threestudio: ``training_step`` is :87-474 in the reference's order, ``fit`` the loop around it, ``validation_step`` / ``test_step``
the images and metrics, ``save_checkpoint`` / ``load_checkpoint`` the reference's checkpoint keys.  It takes the ``system:`` section
of the reference's configs as a dict and the objects it cannot build itself::

    system = registry.find("gaussiansurfel-mvdream-system")(cfg["system"], geometry=model, renderer=renderer, background=env,
                                                             lpips=LPIPSVGG(sd), guidance=guidance)
    system.fit(dataset, max_steps=cfg["trainer"]["max_steps"])
    system.save_checkpoint("last.ckpt")

``guidance`` is any callable ``guidance(rgb, grad_scale=..., normal_flag=..., ref_rgb=..., ref_mask=..., comp_bg=..., **batch) ->
{"loss_sds": ..., ...}`` (INTEGRATION.md 5f around ``MultiviewSDS`` is one) or None; ``lpips`` an ``LPIPSVGG`` or None when
``lambda_normal_F``, ``lambda_normal_B`` and ``lambda_vgg`` are 0.

Quirks of the reference that are kept:
  * ``head_flag = random.random() < 0.4`` is drawn from Python's ``random`` in front of the renders;
  * the front normal view's LPIPS input multiplies by the float mask, the back view's by its binarisation;
  * ``lambda_normal_mask`` and ``lambda_vgg`` only act inside the ``lambda_normal_B`` block (:363-410);
  * the consistency term differentiates both images, covers the SDS views only beyond ``sds_start`` (0 in stage 1, 500 in stage 0)
    and is then halved; its weight is ``C(lambda_normal_consistency) + 0.1 min(2 it / 2000, 1)``;
  * two ``backward()`` calls, the guidance's first with ``retain_graph=True`` and only when ``iteration > sds_start``;
  * the background has an optimizer that is never stepped (:59-66) -- ``train_background=True`` steps it;
  * no densification: the surfel system never calls ``update_states`` -- ``densify=True`` does, once per step.

Deviations:
  * the reference tests ``loss_sds > 0`` and ``loss > 0`` on the host in front of each ``backward()``: two read-backs.  Here the
    guidance's backward is decided from ``iteration`` alone and the main backward always runs;
  * ``grad_scale = exp(-3 comp_occ)`` is handed to the guidance instead of a gradient hook on the image;
  * the ``save_image`` block that fires every 250 steps (:99-167) and ``depth2rgb`` (matplotlib's colour table) are left out;
  * ``tv_loss`` lives in threestudio, not in the reference tree, and every shipped config sets ``lambda_tv_loss`` and
    ``lambda_depth_tv_loss`` to 0: a non-zero value raises ``NotImplementedError``.
"""
from __future__ import annotations

import gc
import random
from typing import Any, Callable, Dict, Mapping, Optional

import torch

from .renderer import registry

LAMBDA_TERMS = (("lambda_position", "train/loss_position"), ("lambda_delta", "train/loss_delta"), ("lambda_opacity", "train/loss_opacity"),
                ("lambda_sparsity", "train/loss_sparsity"), ("lambda_scales", "train/scales"))
UNBUILT = ("lambda_tv_loss", "lambda_depth_tv_loss")
IMAGEDREAM = "imagedream-multiview-diffusion-guidance"


def C(value: Any, epoch: int, global_step: int) -> float:
    """threestudio's schedule rule: a number stays; ``[start_value, end_value, end_step]`` gets a leading 0;
    ``[start_step, start_value, end_value, end_step]`` is linear between the two steps and clamped at both ends.  An integer
    ``end_step`` runs on ``global_step``, a float one on ``epoch``.  Anything else raises ``TypeError``."""
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        return value
    if isinstance(value, (str, bytes, Mapping)) or not hasattr(value, "__len__"):
        raise TypeError(f"Scalar specification only supports list, got {type(value)}")
    value = list(value)
    if len(value) == 3:
        value = [0] + value
    if len(value) != 4 or not all(isinstance(v, (int, float)) and not isinstance(v, bool) for v in value):
        raise TypeError(f"Scalar specification must be a number or a list of 3 or 4 numbers, got {value}")
    start_step, start_value, end_value, end_step = value
    current = global_step if isinstance(end_step, int) else epoch
    return start_value + (end_value - start_value) * max(min(1.0, (current - start_step) / (end_step - start_step)), 0.0)


def sds_start_of(training_stage: int) -> int:
    """:53"""
    return 0 if training_stage == 1 else 500


def consistency_weight(lam: float, iteration: int) -> float:
    """:450-453"""
    return lam + 0.1 * min(2 * iteration / 2000, 1)


def parse_loss(loss: Mapping[str, Any]) -> Dict[str, Any]:
    """The ``loss:`` block of a config as a plain dict; refuses the terms that are not built."""
    loss = dict(loss)
    for k in UNBUILT:
        v = loss.get(k, 0.0)
        if (isinstance(v, (int, float)) and v != 0) or not isinstance(v, (int, float)):
            raise NotImplementedError(f"{k} = {v}: tv_loss is threestudio's, not the reference tree's, and every shipped config sets {k} to 0; "
                                      "it is not built")
    for k, v in loss.items():
        C(v, 0, 0)                                  # a malformed schedule fails here, not in step 1000
    return loss


@registry.register("gaussiansurfel-mvdream-system")
class SurfelMVDreamSystem:
    def __init__(self, cfg: Optional[Mapping[str, Any]] = None, geometry=None, renderer=None, background=None, lpips=None,
                 guidance: Optional[Callable] = None, train_background: bool = False, densify: bool = False):
        cfg = dict(cfg or {})
        self.cfg = cfg
        self.training_stage = int(cfg.get("training_stage", 0))
        if self.training_stage not in (0, 1):
            raise ValueError(f"training_stage must be 0 or 1, got {self.training_stage}")
        self.loss_cfg = parse_loss(cfg.get("loss", {}))
        self.guidance_cfg = dict(cfg.get("guidance", {}) or {})
        self.guidance_type = cfg.get("guidance_type", IMAGEDREAM)
        self.use_explicit = bool((cfg.get("renderer", {}) or {}).get("use_explicit", getattr(getattr(renderer, "cfg", None), "use_explicit", False)))
        self.sds_start = sds_start_of(self.training_stage)
        self.geometry, self.renderer, self.background, self.lpips, self.guidance = geometry, renderer, background, lpips, guidance
        if renderer is not None and background is not None and getattr(renderer, "background", None) is None:
            renderer.background = background
        if lpips is None and any(self._lam(k) > 0 for k in ("lambda_normal_F", "lambda_normal_B", "lambda_vgg")):
            raise ValueError("lambda_normal_F / lambda_normal_B / lambda_vgg need `lpips` (an LPIPSVGG)")
        self.train_background, self.densify = bool(train_background), bool(densify)
        self.bg_optimizer = None
        if background is not None and list(background.parameters()):
            bg_lr = (((cfg.get("optimizer", {}) or {}).get("params", {}) or {}).get("background", {}) or {}).get("lr", 0.001)
            # (the reference builds it and returns only the geometry's: :59-66)
            self.bg_optimizer = torch.optim.Adam(background.parameters(), lr=bg_lr)
        self.global_step, self.epoch = 0, 0
        self.logged: Dict[str, torch.Tensor] = {}
        self.logged_params: Dict[str, float] = {}
        self.evaluator = None
        self._half = {}

    # ---- schedules ---------------------------------------------------------------------------------------------------------------
    def C(self, value: Any) -> float:
        return C(value, self.epoch, self.global_step)

    def _lam(self, key: str) -> float:
        """what the reference's ``self.cfg.loss[key] > 0.0`` tests look at: the number, or 1.0 for a schedule (a list is "on")"""
        v = self.loss_cfg.get(key, 0.0)
        return v if isinstance(v, (int, float)) else 1.0

    def _weight(self, key: str) -> float:
        return self.C(self.loss_cfg.get(key, 0.0))

    def step_range(self):
        """(min_step_percent, max_step_percent) of this step, from the ``guidance:`` section"""
        return self.C(self.guidance_cfg.get("min_step_percent", 0.02)), self.C(self.guidance_cfg.get("max_step_percent", 0.98))

    # ---- the step ------------------------------------------------------------------------------------------------------------------
    def forward(self, batch: Dict[str, Any], head_flag: bool = False):
        """:79-85"""
        self.geometry.update_learning_rate(self.global_step)
        return self.renderer.batch_forward(batch, mode="gen", head_flag=head_flag, stage=self.training_stage)

    __call__ = forward

    def _log(self, name: str, value) -> None:
        self.logged[name] = value.detach() if torch.is_tensor(value) else value

    def _guidance_kwargs(self, batch, gt_out) -> Dict[str, Any]:
        """:182-210"""
        kw: Dict[str, Any] = {}
        if self.guidance_type != IMAGEDREAM:
            return kw
        if self.training_stage == 1:
            kw["ref_rgb"] = batch["gt_rgb_crop"][0].permute(2, 0, 1)
            kw["ref_mask"] = batch["gt_mask_crop"]
        else:
            kw["ref_rgb"] = batch["gt_normal_F"][0].permute(2, 0, 1)
            kw["ref_mask"] = batch["gt_normal_mask"]
            if kw["ref_rgb"].shape[1] != 512:
                up = lambda x: torch.nn.functional.interpolate(x[None], (512, 512), mode="bilinear", align_corners=False)[0]
                kw["ref_rgb"], kw["ref_mask"] = up(kw["ref_rgb"]), up(kw["ref_mask"].float())
        kw["comp_bg"] = gt_out["comp_bg"][0].permute(2, 0, 1)
        return kw

    def _half_image(self, H: int, W: int, dev) -> torch.Tensor:
        key = (H, W, str(dev))
        if key not in self._half:
            self._half[key] = torch.full((3, H, W), 0.5, dtype=torch.float32, device=dev)
        return self._half[key]

    def compute_losses(self, batch: Dict[str, Any], out: Dict[str, Any], gt_out: Dict[str, Any]):
        """-> (loss_sds or None, loss): everything between the renders and the two ``backward()`` calls (:170-463)"""
        from . import step_losses as SL
        from .geometry import LAMBDAS
        from .losses import _AvatarStageLoss, avatar_stage_loss
        it, lam, wt = self.global_step, self._lam, self._weight
        geo = self.geometry
        self._log("gauss_num", int(geo.get_xyz.shape[0]))

        # ---- guidance (:212-254)
        loss_sds = None
        if self.guidance is not None:
            image = out["comp_rgb"] if self.training_stage == 1 else out["comp_normal"].clone()
            grad_scale = torch.exp(-3 * out["comp_occ"].detach()[..., 0]) if lam("lambda_occ") > 0.0 else None
            extra = {"normal_flag": True} if self.training_stage == 0 else {}
            g_out = self.guidance(image, grad_scale=grad_scale, **extra, **self._guidance_kwargs(batch, gt_out), **batch)
            loss_sds = 0.0
            for name, value in g_out.items():
                self._log(f"train/{name}", value)
                if name.startswith("loss_"):
                    loss_sds = loss_sds + value * wt(name.replace("loss_", "lambda_"))

        # ---- per-surfel regularizers (:259-296)
        loss = 0.0
        active = {k: wt(k) for k in LAMBDAS if lam(k) > 0.0}
        if active:
            scales = None
            if "lambda_scales" in active and not self.use_explicit:
                scales = geo.attribute_field(geo.get_xyz)["scales"]
            reg, terms = geo.regularizers(active, scales=scales)
            loss = loss + reg
            for i, (k, name) in enumerate(LAMBDA_TERMS):
                if k in active:
                    self._log(name, terms[i])

        # ---- the video frame (:305-330, :412-417)
        G = {k: v.permute(0, 3, 1, 2) for k, v in gt_out.items() if torch.is_tensor(v) and v.dim() == 4}
        gt_mask = batch["gt_mask"]
        extra_terms = SL.frame_extra_terms(gt_out["comp_occ"], batch["gt_rgb"], gt_mask, gt_out["rand_bg"])
        blended = extra_terms["gt_rgb_blended"]
        l_recon, l_mask = (wt("lambda_recon") if lam("lambda_recon") > 0.0 else 0.0), (wt("lambda_mask") if lam("lambda_mask") > 0.0 else 0.0)
        if l_recon or l_mask:
            _, H, W = G["comp_rgb"][0].shape
            half = self._half_image(H, W, gt_mask.device)
            frame = {"render": G["comp_rgb"][0], "mask": G["comp_mask"][0], "normal": half}
            gt_rgb = batch["gt_rgb"][0].permute(2, 0, 1).contiguous()
            frame_loss, t = avatar_stage_loss(frame, gt_rgb, gt_mask, half, gt_mask[0] > 1e-5, gt_rgb_blended=blended.permute(0, 3, 1, 2)[0],
                                              lambda_recon=l_recon, lambda_mask=l_mask, lambda_normal=0.0, return_terms=True)
            loss = loss + frame_loss
            S = _AvatarStageLoss
            if l_recon:
                self._log("train/loss_recon", (0.8 * t[S.L1] + 0.2 * (1 - t[S.SSIM])) * l_recon)
            if l_mask:
                self._log("train/loss_mask", t[S.L1M] * l_mask)

        # ---- the normal views (:332-410)
        use_F = lam("lambda_normal_F") > 0.0 and "gt_normal_F" in batch
        use_B = lam("lambda_normal_B") > 0.0 and "gt_normal_B" in batch
        if use_F or use_B:
            # (the node reads the front view always: with only the back block on, its terms get no upstream; a batch without
            # gt_normal_F lends it the back target to read)
            front = batch["gt_normal_F"] if "gt_normal_F" in batch else batch["gt_normal_B"]
            nv = SL.normal_view_terms(gt_out["comp_normal"], gt_out["comp_normal_mask"], front, batch["gt_normal_B"] if use_B else None,
                                      batch["gt_normal_mask"])
            views = 2 if use_B else 1
            lp = self.lpips(nv["lpips_in"][:views], nv["lpips_in"][views:].detach()).reshape(-1)      # (the targets' rows are constants)
            if use_F:
                loss_normal = (nv["cos_F"] + 1 * lp[0]) * wt("lambda_normal_F")
                self._log("train/loss_normal_F", loss_normal)
                loss = loss + loss_normal
            if use_B:
                loss_normal = (nv["cos_B"] + lp[1]) * wt("lambda_normal_B")
                self._log("train/loss_normal_B", loss_normal)
                loss = loss + loss_normal
                if lam("lambda_normal_mask") > 0.0:
                    loss = loss + nv["mask_l1"] * wt("lambda_normal_mask")
                if lam("lambda_vgg") > 0.0:
                    vgg = wt("lambda_vgg") * self.lpips((G["comp_rgb"] - 0.5) * 2, (blended.permute(0, 3, 1, 2) - 0.5) * 2).mean()
                    self._log("train/vgg_loss", vgg)
                    loss = loss + vgg

        if lam("lambda_occ") > 0.0:
            loss = loss + extra_terms["loss_occ"] * wt("lambda_occ")

        # ---- predicted-normal consistency (:429-453), curvature (:455-460)
        if lam("lambda_normal_consistency") > 0.0 and "comp_pred_normal" in out:
            pn = SL.consistency_loss(gt_out["comp_pred_normal"], gt_out["comp_normal"])
            if it > self.sds_start:
                pn = (pn + SL.consistency_loss(out["comp_pred_normal"], out["comp_normal"])) * 0.5
            self._log("train/loss_pred_normal_consistency", pn)
            loss = loss + consistency_weight(wt("lambda_normal_consistency"), it) * pn
        if lam("lambda_curv") > 0.0 and "comp_curv" in out:
            loss_curv = SL.abs_mean(out["comp_curv"]) * wt("lambda_curv")
            self._log("train/loss_curv", loss_curv)
            loss = loss + loss_curv
        self.logged_params = {f"train_params/{k}": self.C(v) for k, v in self.loss_cfg.items()}
        return loss_sds, loss

    def training_step(self, batch: Dict[str, Any], batch_idx: int = 0) -> Dict[str, Any]:
        """:87-474"""
        opt = self.geometry.optimizer
        if opt is None:
            raise RuntimeError("training_step: call geometry.training_setup() first")
        it = self.global_step
        self.logged = {}
        head_flag = random.random() < 0.4
        out, gt_out = self.forward(batch, head_flag=head_flag)
        loss_sds, loss = self.compute_losses(batch, out, gt_out)
        if torch.is_tensor(loss_sds) and it > self.sds_start:
            loss_sds.backward(retain_graph=True)
        if torch.is_tensor(loss):                        # (a config with every weight at 0 has nothing to differentiate)
            loss.backward()
        self.before_step()
        opt.step()
        if self.train_background and self.bg_optimizer is not None:
            self.bg_optimizer.step()
        if self.densify:
            both = lambda k: list(out[k]) + list(gt_out[k])
            self.geometry.update_states(it, both("visibility_filter"), both("radii"), both("viewspace_points"))
        opt = self.geometry.optimizer                    # (densification keeps the optimizer; a restored model has a new one)
        opt.zero_grad(set_to_none=True)
        if self.train_background and self.bg_optimizer is not None:
            self.bg_optimizer.zero_grad(set_to_none=True)
        self.global_step += 1
        total = loss if not torch.is_tensor(loss_sds) else loss_sds + loss
        return {"loss": total.detach() if torch.is_tensor(total) else total}

    def before_step(self) -> None:
        """between the two ``backward()`` calls and ``opt.step()``: the leaves hold this step's gradients (a hook for callers)"""

    def fit(self, dataset, max_steps: int) -> "SurfelMVDreamSystem":
        """``max_steps`` training steps over ``dataset`` (a ``RandomMultiviewCameraDataset`` of the train split)."""
        if self.geometry.optimizer is None:
            self.geometry.training_setup()
        gc.collect()
        gc.freeze()                                      # (README "For integrators": the model's objects leave the collector's lists)
        g = self.guidance
        for _ in range(int(max_steps)):
            dataset.update_step(self.epoch, self.global_step)
            if g is not None and (hasattr(g, "set_step_range") or hasattr(g, "update_step")):
                lo, hi = self.step_range()
                if hasattr(g, "set_step_range"):
                    g.set_step_range(lo, hi)
                else:
                    g.update_step(self.epoch, self.global_step)
            self.training_step(dataset.collate())
        return self

    # ---- validation and testing --------------------------------------------------------------------------------------------------
    def _checkpoint_surfels(self):
        from .playback import CheckpointSurfels
        geo = self.geometry
        return CheckpointSurfels(geo._xyz, geo._rotation, geo._occ, geo._colors, geo._scaling, geo.attribute_field, geo.smpl_guidance)

    @torch.no_grad()
    def validation_step(self, batch: Dict[str, Any], batch_idx: int = 0) -> Dict[str, Optional[torch.Tensor]]:
        """The four images of :476-522 -- ``comp_rgb``, ``comp_normal``, ``comp_pred_normal``, ``comp_occ`` of the first view -- as
        byte images [H,W,4] (the image, the mask as fourth channel) and the byte mask, through ``playback_finish``.  A batch that
        holds ``"camera"`` (a ``renderer.cameras.Camera``) and ``"pose"`` (a pose dict of one frame, ``AvatarPlayer.frame_pose``) is a
        playback frame: it is rendered the way ``AvatarPlayer`` renders the checkpoint this system would save, so the two agree
        bit for bit (``pred_normal`` is None there: the player has none)."""
        from .playback import AvatarPlayer, playback_finish
        if "camera" in batch:
            guide = self.geometry.smpl_guidance
            player = AvatarPlayer(self._checkpoint_surfels(), guide, use_explicit=self.use_explicit)
            res = player.render(batch["pose"], batch["camera"], bg=batch.get("bg_color"), chunk=1)
            return {"rgb": res["rgb"][0], "normal": res["normal"][0], "pred_normal": None, "occ": res["occ"][0], "mask": res["mask"][0]}
        out = self.forward(batch)
        out = out[0] if isinstance(out, tuple) else out
        first = lambda k: out[k].detach().permute(0, 3, 1, 2)[:1].contiguous()
        a = playback_finish(first("comp_rgb"), first("comp_normal"), first("comp_mask"), first("comp_occ") if "comp_occ" in out else None)
        res = {"rgb": a["rgb"][0], "normal": a["normal"][0], "pred_normal": None, "occ": None if a["occ"] is None else a["occ"][0],
               "mask": a["mask"][0]}
        if "comp_pred_normal" in out:
            res["pred_normal"] = playback_finish(first("comp_pred_normal"), first("comp_pred_normal"), first("comp_mask"))["rgb"][0]
        return res

    def on_test_epoch_start(self, capacity: int, keep_images: bool = False) -> None:
        from .evaluate import TestEvaluator
        self.evaluator = TestEvaluator(self.lpips, capacity=capacity, keep_images=keep_images)

    @torch.no_grad()
    def test_step(self, batch: Dict[str, Any], batch_idx: int = 0) -> None:
        """:527-567 through ``TestEvaluator``: nothing leaves the device"""
        if self.evaluator is None:
            raise RuntimeError("test_step: call on_test_epoch_start(capacity) first")
        out, gt_out = self.forward(batch)
        self.evaluator.add(gt_out["comp_rgb"], batch)

    def on_test_epoch_end(self, save_dir: Optional[str] = None) -> Dict[str, Any]:
        """:569-589: the one read-back; the four text files and the images when ``save_dir`` is given"""
        res = self.evaluator.finish(save_dir=save_dir, step=self.global_step)
        registry.info(f"Average PSNR: {res['psnr']}; SSIM: {res['ssim']}; LPIPS: {res['lpips_mean']}")
        return res

    # ---- checkpoints -------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference's keys: ``geometry._xyz`` ... ``geometry._occ``, ``geometry.latent_pose``, ``geometry.attribute_field.*``,
        ``background.*``; and ``geometry.original_pos``, which ``lambda_delta`` measures from."""
        from .geometry import LEAVES
        geo = self.geometry
        sd = {f"geometry.{attr}": getattr(geo, attr).detach() for _, attr in LEAVES}
        sd["geometry.original_pos"] = geo.original_pos.detach()
        if hasattr(geo, "latent_pose"):
            sd["geometry.latent_pose"] = geo.latent_pose.detach()
        if geo.attribute_field is not None:
            sd.update({f"geometry.attribute_field.{k}": v.detach() for k, v in geo.attribute_field.state_dict().items()})
        if self.background is not None:
            sd.update({f"background.{k}": v.detach() for k, v in self.background.state_dict().items()})
        return sd

    def save_checkpoint(self, path) -> None:
        torch.save({"state_dict": {k: v.cpu().clone() for k, v in self.state_dict().items()}, "global_step": self.global_step,
                    "epoch": self.epoch}, path)

    def load_checkpoint(self, path) -> None:
        """``on_load_checkpoint`` (:68-77): a model of the checkpoint's size from a zero point cloud, ``training_setup()``; then the
        state dict, as Lightning loads it behind the hook, and ``training_setup()`` for the new leaves.  (Only open files you trust.)"""
        from .geometry import LEAVES
        ckpt = path if isinstance(path, Mapping) else torch.load(path, map_location="cpu", weights_only=False)
        sd = ckpt["state_dict"]
        geo = self.geometry
        num_pts = sd["geometry._xyz"].shape[0]
        geo.create_from_pcd(torch.zeros(num_pts, 3), torch.full((num_pts, 3), 0.5), 10)
        geo.training_setup()
        dev = geo._xyz.device
        leaves = {name: sd[f"geometry.{attr}"].to(dev) for name, attr in LEAVES if f"geometry.{attr}" in sd}
        if "geometry.original_pos" in sd:
            leaves["original_pos"] = sd["geometry.original_pos"].to(dev)
        geo.set_leaves(**leaves)
        if "geometry.latent_pose" in sd:
            geo.latent_pose = torch.nn.Parameter(sd["geometry.latent_pose"].to(dev).clone().requires_grad_(True))
        prefix = "geometry.attribute_field."
        field_sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        if field_sd:
            from .field import HashMLPField
            rows = field_sd["encoding.hash_table"].shape[0] // int(field_sd["num_levels"])
            field = HashMLPField(field_sd["aabb"].detach().float().cpu(), log2_hashmap_size=rows.bit_length() - 1,
                                 max_res=int(field_sd["max_res"]), num_levels=int(field_sd["num_levels"]))
            field.load_state_dict({k: v.detach().cpu() for k, v in field_sd.items()})
            geo.attribute_field = field.to(dev)
            geo.aabb = field_sd["aabb"].to(dev)
        bg_sd = {k[len("background."):]: v for k, v in sd.items() if k.startswith("background.")}
        if bg_sd and self.background is not None:
            self.background.load_state_dict(bg_sd)
        geo.training_setup()
        self.global_step, self.epoch = int(ckpt.get("global_step", 0)), int(ckpt.get("epoch", 0))
