"""ctypes binding of libsoar_hip.so (include/soar_hip.h).

There is no CPU fallback: if the library is missing the import of a symbol fails loudly with a build hint.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SOAR_HIP_LIB: another build of the same library (development A/B runs: scripts/variant.py); still no fallback of any kind
LIB_PATH = os.environ.get("SOAR_HIP_LIB") or os.path.join(_HERE, "_lib", "libsoar_hip.so")
if os.environ.get("SOAR_HIP_LIB"):
    import sys as _sys
    print(f"[soar_amd] SOAR_HIP_LIB is set: loading {LIB_PATH} instead of the in-tree build (development A/B runs only)", file=_sys.stderr)

FRAME_LOSS_SCRATCH_FLOATS = 4 * 2048   # SOAR_FRAME_LOSS_SCRATCH_FLOATS: the scratch argument of soar_frame_loss[_pooled]
ABI_VERSION = 8          # SOAR_HIP_ABI_VERSION of include/soar_hip.h this binding was written for
c_f32p = C.c_void_p
_vp = C.c_void_p


class SoarRastParams(C.Structure):
    """Mirror of ``struct SoarRastParams`` (include/soar_hip.h)."""
    _fields_ = [
        ("P", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("sh_degree", C.c_int32), ("M", C.c_int32),
        ("prefiltered", C.c_int32), ("render_front", C.c_int32), ("sort_descending", C.c_int32), ("debug", C.c_int32),
        ("cfg_surface", C.c_int32), ("cfg_normalize_depth", C.c_int32), ("cfg_perpix_depth", C.c_int32),
        ("cfg_lrn_cam", C.c_int32),
        ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
        ("bg_dev", _vp), ("viewmatrix_dev", _vp), ("projmatrix_dev", _vp), ("prcppoint_dev", _vp),
        ("patchbbox_dev", _vp), ("campos_dev", _vp),
    ]


class SoarDensifyRow(C.Structure):
    """Mirror of ``struct SoarDensifyRow`` (include/soar_hip.h)."""
    _fields_ = [("src", _vp), ("dst", _vp), ("width", C.c_int32), ("mode", C.c_int32)]


class SoarAdamRow(C.Structure):
    """Mirror of ``struct SoarAdamRow`` (include/soar_hip.h)."""
    _fields_ = [("param", _vp), ("grad", _vp), ("exp_avg", _vp), ("exp_avg_sq", _vp), ("count", C.c_int64), ("lr", C.c_float),
                ("pad_", C.c_int32)]


class SoarPoseArgs(C.Structure):
    """Mirror of ``struct SoarPoseArgs`` (include/soar_hip.h)."""
    _fields_ = [("P", C.c_int32), ("J", C.c_int32), ("scale_width", C.c_int32), ("warp", C.c_int32),
                ("xyz", _vp), ("rot", _vp), ("weights", _vp), ("joint_mats", _vp), ("offsets", _vp), ("axis_perm", _vp),
                ("colors", _vp), ("scale_src", _vp), ("occ", _vp), ("occ3", _vp), ("posed", _vp),
                ("grad_scratch", _vp), ("dL_dxyz", _vp), ("dL_drot", _vp), ("dL_dcolors", _vp), ("dL_dscale", _vp), ("dL_docc", _vp)]


class SoarCameraSpec(C.Structure):
    """Mirror of ``struct SoarCameraSpec`` (include/soar_hip.h)."""
    _fields_ = [("fovx", C.c_double), ("fovy", C.c_double), ("znear", C.c_double), ("zfar", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("img_w", C.c_double), ("img_h", C.c_double), ("has_cxcy", C.c_int32), ("pad_", C.c_int32)]


class SoarFrameHead(C.Structure):
    """Mirror of ``struct SoarFrameHead`` (include/soar_hip.h): one frame of soar_frames_warp_preprocess."""
    _fields_ = [("prm", _vp), ("geom_buffer", _vp), ("radii", _vp)]


class SoarFrameTail(C.Structure):
    """Mirror of ``struct SoarFrameTail`` (include/soar_hip.h): one frame of soar_frames_geometry_warp_backward."""
    _fields_ = [("prm", _vp), ("means3D", _vp), ("rotations", _vp), ("radii", _vp), ("geom_buffer", _vp), ("workspace", _vp),
                ("dL_dmeans2D", _vp)]


class SoarLossFinish(C.Structure):
    """Mirror of ``struct SoarLossFinish`` (include/soar_hip.h): what soar_frame_loss_partials leaves for the tail of the step."""
    _fields_ = [("sums4", _vp), ("loss_out", _vp), ("blocks", C.c_int32), ("n", C.c_int32), ("w_color", C.c_float), ("w_mask", C.c_float),
                ("w_normal", C.c_float), ("w_depth", C.c_float)]


BACKWARD_LOSS_SCRATCH_FLOATS = 4 * FRAME_LOSS_SCRATCH_FLOATS   # SOAR_BACKWARD_LOSS_SCRATCH_FLOATS: SoarBackwardLoss.wave_sums


class SoarBackwardLoss(C.Structure):
    """Mirror of ``struct SoarBackwardLoss`` (include/soar_hip.h): the loss record of soar_rast_backward_plan_loss."""
    _fields_ = [("color", _vp), ("normal", _vp), ("depth", _vp), ("opac", _vp), ("target_color", _vp), ("target_mask", _vp),
                ("target_normal", _vp), ("set_index_dev", _vp), ("n_sets", C.c_int32), ("w_color", C.c_float), ("w_mask", C.c_float),
                ("w_normal", C.c_float), ("w_depth", C.c_float), ("loss_out", _vp), ("wave_sums", _vp)]


class SoarViewArgs(C.Structure):
    """Mirror of ``struct SoarViewArgs`` (include/soar_hip.h)."""
    _fields_ = [("rast", SoarRastParams), ("focal_k00", C.c_float), ("focal_k11", C.c_float), ("back", C.c_int32), ("pad_", C.c_int32),
                ("capacity", C.c_int64),
                ("buffer", _vp), ("buffer_bytes", C.c_size_t), ("out", _vp), ("radii", _vp), ("status_pinned", _vp),
                ("g_render", _vp), ("g_normal", _vp), ("g_depth", _vp), ("g_pred_normal", _vp), ("g_mask", _vp), ("g_occ", _vp),
                ("g_curv", _vp), ("dL_dmeans2D", _vp)]


class SoarAvatarLossArgs(C.Structure):
    """Mirror of ``struct SoarAvatarLossArgs`` (include/soar_hip.h)."""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("cos_limit", C.c_float), ("cos_weight", C.c_float),
                ("render", _vp), ("gt_rgb", _vp), ("mask_img", _vp), ("gt_mask", _vp), ("normal", _vp), ("gt_normal", _vp), ("occ", _vp),
                ("sel", _vp), ("sel_normal", _vp), ("sel_occ", _vp), ("stats", _vp), ("stats_occ", _vp), ("scratch", _vp), ("counts", _vp),
                ("up_l1", _vp), ("up_l1m", _vp), ("up_cos", _vp), ("up_occ", _vp), ("up_ssim", _vp), ("g_ssim", _vp),
                ("g_render", _vp), ("g_mask", _vp), ("g_normal", _vp), ("g_occ", _vp),
                ("normal_raw", C.c_int32), ("occ_grad_summed", C.c_int32), ("cos_scale_out", _vp), ("background", _vp)]


class SoarFieldHead(C.Structure):
    """Mirror of ``struct SoarFieldHead`` (include/soar_hip.h)."""
    _fields_ = [("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp)]


FIELD_LEVELS = 16        # SOAR_FIELD_LEVELS


class SoarFieldArgs(C.Structure):
    """Mirror of ``struct SoarFieldArgs`` (include/soar_hip.h)."""
    _fields_ = [("N", C.c_int32), ("log2_T", C.c_int32), ("normalized", C.c_int32), ("pad_", C.c_int32),
                ("res", C.c_float * FIELD_LEVELS), ("xyz", _vp), ("aabb", _vp), ("table", _vp), ("qtable", _vp), ("z", _vp),
                ("head", SoarFieldHead * 5), ("enc", _vp), ("qenc", _vp), ("out", _vp * 5), ("g_out", _vp * 5),
                ("d_table", _vp), ("d_qtable", _vp), ("d_head", _vp * 5), ("d_xyz", _vp), ("d_z", _vp)]


class SoarEnvmapArgs(C.Structure):
    """Mirror of ``struct SoarEnvmapArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_comp", C.c_int32), ("color_rows", C.c_int32),
                ("pad_", C.c_int32), ("render_stride", C.c_int64), ("mask_stride", C.c_int64), ("g_comp_stride", C.c_int64 * 4),
                ("dirs", _vp), ("w1", _vp), ("w2", _vp), ("w3", _vp), ("color", _vp), ("render", _vp), ("mask", _vp),
                ("bg", _vp), ("comp", _vp), ("g_comp", _vp), ("g_bg", _vp), ("g_mask", _vp), ("d_w1", _vp), ("d_w2", _vp), ("d_w3", _vp)]


LPIPS_LAYERS, LPIPS_TAPS = 13, 5     # SOAR_LPIPS_LAYERS, SOAR_LPIPS_TAPS


class SoarLpipsWeights(C.Structure):
    """Mirror of ``struct SoarLpipsWeights`` (include/soar_hip.h)."""
    _fields_ = [("conv_w", _vp * LPIPS_LAYERS), ("conv_b", _vp * LPIPS_LAYERS), ("lin", _vp * LPIPS_TAPS), ("shift", _vp), ("scale", _vp)]


class SoarLpipsArgs(C.Structure):
    """Mirror of ``struct SoarLpipsArgs`` (include/soar_hip.h)."""
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("grads", C.c_int32), ("in0", _vp), ("in1", _vp),
                ("in0_stride", C.c_int64 * 4), ("in1_stride", C.c_int64 * 4), ("weights", _vp), ("out", _vp), ("g_out", _vp),
                ("g_in0", _vp), ("g_in1", _vp), ("g_in0_stride", C.c_int64 * 4), ("g_in1_stride", C.c_int64 * 4)]


class SoarVaeArgs(C.Structure):
    """Mirror of ``struct SoarVaeArgs`` (include/soar_hip.h)."""
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("image_size", C.c_int32), ("x", _vp), ("x_stride", C.c_int64 * 4),
                ("weights", _vp), ("scale_factor", C.c_float), ("eps", _vp), ("mean", _vp), ("logvar", _vp), ("latents", _vp),
                ("g_latents", _vp), ("g_scale", _vp), ("grad_scale", _vp), ("grad_scale_stride", C.c_int64 * 3), ("g_x", _vp),
                ("g_x_stride", C.c_int64 * 4)]


SDS_PLAIN, SDS_RECON = 0, 1          # SOAR_SDS_PLAIN, SOAR_SDS_RECON


class SoarSdsArgs(C.Structure):
    """Mirror of ``struct SoarSdsArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("n_view", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("mode", C.c_int32), ("n_timesteps", C.c_int32),
                ("guidance_scale", C.c_float), ("recon_std_rescale", C.c_float), ("grad_clip", C.c_float), ("t", _vp), ("tables", _vp),
                ("latents", _vp), ("noise", _vp), ("eps_pred", _vp), ("x_in", _vp), ("loss", _vp), ("grad_norm", _vp), ("g_lat", _vp)]


DATA_CROP, DATA_MAX_VIEWS, DATA_SMALL_FLOATS = 512, 8, 256     # SOAR_DATA_CROP, SOAR_DATA_MAX_VIEWS, SOAR_DATA_SMALL_FLOATS


class SoarDataStepArgs(C.Structure):
    """Mirror of ``struct SoarDataStepArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("n_frames", C.c_int32), ("Hv", C.c_int32), ("Wv", C.c_int32),
                ("frame", C.c_int32), ("rays_d_normalize", C.c_int32), ("gt_has_cxcy", C.c_int32), ("n_small", C.c_int32),
                ("near_plane", C.c_double), ("far_plane", C.c_double), ("gt_near", C.c_double),
                ("c2w", (C.c_float * 16) * DATA_MAX_VIEWS), ("focal", C.c_float * DATA_MAX_VIEWS), ("tan_half", C.c_float * DATA_MAX_VIEWS),
                ("gt_c2w", C.c_float * 16), ("gt_tan_half", C.c_float), ("gt_cx", C.c_float), ("gt_cy", C.c_float),
                ("small", C.c_float * DATA_SMALL_FLOATS),
                ("images", _vp), ("masks", _vp), ("normal_F", _vp), ("normal_B", _vp), ("normal_mask", _vp),
                ("rgb_crop", _vp), ("mask_crop", _vp), ("normal_Ks", _vp),
                ("rays_d", _vp), ("cam_d", _vp), ("gt_rays_d", _vp), ("gt_cam_d", _vp),
                ("gt_rgb", _vp), ("gt_mask", _vp), ("gt_normal_F", _vp), ("gt_normal_B", _vp), ("gt_normal_mask", _vp),
                ("gt_rgb_crop", _vp), ("gt_mask_crop", _vp),
                ("mvp_mtx", _vp), ("proj", _vp), ("gt_mvp_mtx", _vp), ("small_out", _vp)]


class SoarEvalArgs(C.Structure):
    """Mirror of ``struct SoarEvalArgs`` (include/soar_hip.h)."""
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pad_", C.c_int32), ("pred", _vp), ("gt_rgb", _vp), ("gt_mask", _vp),
                ("pred_stride", C.c_int64 * 4), ("gt_stride", C.c_int64 * 4), ("mask_stride", C.c_int64 * 3),
                ("gt_white", _vp), ("pred2", _vp), ("gt2", _vp), ("grid", _vp), ("metrics", _vp)]


class SoarPlaybackArgs(C.Structure):
    """Mirror of ``struct SoarPlaybackArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("normal_as_rgb", C.c_int32), ("render", _vp), ("normal", _vp),
                ("mask", _vp), ("occ", _vp), ("render_stride", C.c_int64), ("normal_stride", C.c_int64), ("mask_stride", C.c_int64),
                ("occ_stride", C.c_int64), ("rgb", _vp), ("normal_out", _vp), ("occ_out", _vp), ("mask_out", _vp)]


class SoarFitvizStripArgs(C.Structure):
    """Mirror of ``struct SoarFitvizStripArgs`` (include/soar_hip.h)."""
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("K", C.c_int32), ("L", C.c_int32), ("radius", C.c_int32),
                ("thickness", C.c_int32), ("half", C.c_int32), ("target_px", _vp), ("fit_px", _vp), ("kp_mask", _vp), ("limbs", _vp),
                ("limb_rgb", _vp), ("imgs", _vp), ("imgs_stride", C.c_int64 * 4), ("prior", _vp), ("mask", _vp),
                ("target_rgb", C.c_uint8 * 4), ("fit_rgb", C.c_uint8 * 4), ("out", _vp)]


class SoarNormalNetArgs(C.Structure):
    """Mirror of ``struct SoarNormalNetArgs`` (include/soar_hip.h)."""
    _fields_ = [("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ngf", C.c_int32), ("n_down", C.c_int32), ("n_blocks", C.c_int32),
                ("image", _vp), ("prior_F", _vp), ("prior_B", _vp), ("image_stride", C.c_int64 * 4), ("prior_F_stride", C.c_int64 * 4),
                ("prior_B_stride", C.c_int64 * 4), ("weights_F", _vp), ("weights_B", _vp), ("normal_F", _vp), ("normal_B", _vp)]


class SoarConvGemmTaps(C.Structure):
    """Mirror of ``struct SoarConvGemmTaps`` (include/soar_hip.h)."""
    _fields_ = [("w", _vp), ("ldw", C.c_int64), ("ntaps", C.c_int32), ("py", C.c_int32), ("px", C.c_int32), ("dy", C.c_int8 * 9),
                ("dx", C.c_int8 * 9)]


class SoarConvGemmArgs(C.Structure):
    """Mirror of ``struct SoarConvGemmArgs`` (include/soar_hip.h)."""
    _fields_ = [("x", _vp), ("ldx", C.c_int64), ("xim", C.c_int64), ("wbat", C.c_int64), ("bias", _vp), ("res", _vp), ("y", _vp),
                ("ldy", C.c_int64), ("yim", C.c_int64), ("alpha", C.c_float), ("N", C.c_int32), ("Hg", C.c_int32), ("Wg", C.c_int32),
                ("Hin", C.c_int32), ("Win", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("stride", C.c_int32), ("dil", C.c_int32),
                ("reflect", C.c_int32), ("Wout", C.c_int32), ("os", C.c_int32), ("per_image", C.c_int32), ("nph", C.c_int32),
                ("ph", SoarConvGemmTaps * 4)]


class SoarSmplifyRig(C.Structure):
    """Mirror of ``struct SoarSmplifyRig`` (include/soar_hip.h)."""
    _fields_ = [("J", C.c_int32), ("NBS", C.c_int32), ("NE", C.c_int32), ("VS", C.c_int32), ("P", C.c_int32), ("pad_", C.c_int32),
                ("J_template", _vp), ("J_dirs", _vp), ("parents", _vp), ("v_template", _vp), ("shapedirs", _vp), ("posedirs", _vp),
                ("lbs_weights", _vp), ("pt_kind", _vp), ("pt_idx", _vp), ("pt_w", _vp), ("pt_dst", _vp), ("kp_mask", _vp)]


_SMPLIFY_PARAMS = ("global_orient", "body_pose", "left_hand_pose", "right_hand_pose", "betas", "transl", "jaw_pose", "leye_pose", "reye_pose",
                   "expression")


class SoarSmplifyArgs(C.Structure):
    """Mirror of ``struct SoarSmplifyArgs`` (include/soar_hip.h)."""
    _fields_ = ([("N", C.c_int32), ("ignore_hands", C.c_int32), ("grads", C.c_int32), ("pad_", C.c_int32)]
                + [(k, _vp) for k in _SMPLIFY_PARAMS] + [(k + "0", _vp) for k in _SMPLIFY_PARAMS]
                + [("Ks", _vp), ("w2c", _vp), ("target_kps", _vp), ("target_scales", _vp),
                   ("img_w", C.c_float), ("img_h", C.c_float), ("sigma", C.c_float), ("kp_scale", C.c_float), ("pose_scale", C.c_float * 4),
                   ("row_scale", C.c_float), ("w_preserve", C.c_float), ("smooth_scale", C.c_float * 4)]
                + [("g_" + k, _vp) for k in _SMPLIFY_PARAMS[:6]] + [("loss", _vp), ("kps", _vp), ("frame_betas", _vp), ("frame_loss", _vp)])


class SoarPoseSearch(C.Structure):
    """Mirror of ``struct SoarPoseSearch`` (include/soar_hip.h)."""
    _fields_ = ([(k, C.c_int32) for k in ("N", "B", "H", "PA", "P", "min_points")]
                + [(k, _vp) for k in ("points0", "pivot", "rotations", "src_inds", "dst_inds", "kp_mask", "target_kps", "Ks", "w2c", "scales")]
                + [(k, C.c_float) for k in ("img_w", "img_h", "sigma", "conf_min", "z_min", "pad_")]
                + [("cost", _vp), ("transl", _vp), ("valid", _vp)])


class SoarSmplifyBody(C.Structure):
    """Mirror of ``struct SoarSmplifyBody`` (include/soar_hip.h)."""
    _fields_ = [("L_dyn", C.c_int32), ("n_rows", C.c_int32), ("neck", C.c_int32), ("VU", C.c_int32), ("dyn_vrow", _vp), ("dyn_bary", _vp),
                ("dyn_point", _vp), ("pose_mean", _vp), ("mean_mask", C.c_uint64), ("rows_out", _vp)]


class SoarNormalViewArgs(C.Structure):
    """Mirror of ``struct SoarNormalViewArgs`` (include/soar_hip.h)."""
    _fields_ = [("R", C.c_int32), ("views", C.c_int32), ("normal", _vp), ("normal_stride", C.c_int64), ("mask0", _vp), ("gt_F", _vp),
                ("gt_B", _vp), ("gt_mask", _vp), ("values", _vp), ("stats", _vp), ("lpips_in", _vp), ("scratch", _vp), ("up", _vp),
                ("g_lpips", _vp), ("g_normal", _vp), ("g_mask0", _vp)]


class SoarFrameExtraArgs(C.Structure):
    """Mirror of ``struct SoarFrameExtraArgs`` (include/soar_hip.h)."""
    _fields_ = [("H", C.c_int32), ("W", C.c_int32), ("occ", _vp), ("gt_rgb", _vp), ("gt_mask", _vp), ("rand_bg", _vp),
                ("rgb_stride", C.c_int64 * 2), ("bg_stride", C.c_int64 * 2), ("stats", _vp), ("blended", _vp), ("scratch", _vp), ("up", _vp),
                ("g_occ", _vp)]


class SoarJpegArgs(C.Structure):
    """Mirror of ``struct SoarJpegArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("subsampling", C.c_int32),
                ("restart_interval", C.c_int32), ("frames", _vp), ("frame_stride", C.c_int64), ("qtables", (C.c_uint8 * 64) * 2)]


class SoarPngArgs(C.Structure):
    """Mirror of ``struct SoarPngArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("filter", C.c_int32),
                ("piece_bytes", C.c_int32), ("images", _vp), ("image_stride", C.c_int64)]


class SoarPngDecodeArgs(C.Structure):
    """Mirror of ``struct SoarPngDecodeArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("data", _vp), ("offsets", _vp),
                ("total_bytes", C.c_int64)]


class SoarJpegDecodeArgs(C.Structure):
    """Mirror of ``struct SoarJpegDecodeArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("data", _vp), ("offsets", _vp),
                ("total_bytes", C.c_int64)]


class SoarResizeArgs(C.Structure):
    """Mirror of ``struct SoarResizeArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("channels", C.c_int32), ("out_h", C.c_int32), ("out_w", C.c_int32),
                ("ksize_h", C.c_int32), ("ksize_v", C.c_int32), ("images", _vp), ("temp", _vp), ("bounds_h", _vp), ("coef_h", _vp),
                ("bounds_v", _vp), ("coef_v", _vp)]


SAM_MAX_DEPTH = 32


class SoarSamConfig(C.Structure):
    """Mirror of ``struct SoarSamConfig`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("image_size", "patch", "grid", "embed", "depth", "heads", "head_dim", "mlp", "out_chans")] + \
               [("window", C.c_int32 * SAM_MAX_DEPTH)] + \
               [(n, C.c_int32) for n in ("dec_layers", "dec_heads", "dec_down", "dec_mlp", "mask_tokens", "hyper_depth", "iou_depth", "iou_hidden")]


class SoarSamEncodeArgs(C.Structure):
    """Mirror of ``struct SoarSamEncodeArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("block_begin", C.c_int32), ("block_end", C.c_int32), ("patches", _vp), ("tokens_in", _vp),
                ("tokens_out", _vp), ("embeddings", _vp)]


class SoarSamDecodeArgs(C.Structure):
    """Mirror of ``struct SoarSamDecodeArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("max_points", C.c_int32), ("scale_x", C.c_float), ("scale_y", C.c_float), ("embeddings", _vp),
                ("points", _vp), ("labels", _vp), ("counts", _vp), ("low_res", _vp), ("iou", _vp), ("prompt_tokens", _vp), ("tokens_out", _vp)]


UNET_MAX_LEVELS = 8
UNET_MAX_PROBES = 16
UNET_PROBE_EMB = 1000000


class SoarUnetConfig(C.Structure):
    """Mirror of ``struct SoarUnetConfig`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "out_channels", "model_channels", "levels", "num_res_blocks")] + \
               [("channel_mult", C.c_int32 * UNET_MAX_LEVELS), ("attention", C.c_int32 * UNET_MAX_LEVELS)] + \
               [(n, C.c_int32) for n in ("context_dim", "camera_dim", "with_ip", "head_channels", "n_view", "precision",
                                            "attn_precision")]


class SoarUnetArgs(C.Structure):
    """Mirror of ``struct SoarUnetArgs`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("N", "H", "W", "T", "n_ip")] + [("ip_weight", C.c_float), ("x", _vp), ("x_stride", C.c_int64 * 4),
                ("t", _vp), ("context", _vp), ("camera", _vp), ("ip_tokens", _vp), ("eps", _vp), ("n_probes", C.c_int32),
                ("probe_code", C.c_int32 * UNET_MAX_PROBES), ("probe_dst", _vp * UNET_MAX_PROBES)]


class SoarUnetAttnArgs(C.Structure):
    """Mirror of ``struct SoarUnetAttnArgs`` (include/soar_hip.h)."""
    _fields_ = [(n, _vp) for n in ("q", "k", "v", "k2", "v2", "out")] + [(n, C.c_int64) for n in ("ldq", "ldk", "ldv", "ldk2", "ldv2", "ldo")] + \
               [(n, C.c_int32) for n in ("B", "Lq", "Lk", "Lk2", "heads", "hd")] + [("scale", C.c_float), ("w2", C.c_float)]


CLIP_TEXT, CLIP_VISION = 0, 1        # SOAR_CLIP_TEXT, SOAR_CLIP_VISION
CLIP_MAX_LAYERS = 64
CLIP_MAX_PROBES = 16
CLIP_PROBE_EMBED, CLIP_PROBE_PRE = 1000000, 1000001


class SoarClipConfig(C.Structure):
    """Mirror of ``struct SoarClipConfig`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("kind", "width", "heads", "layers", "mlp", "tokens", "vocab", "patch", "grid", "precision",
                                           "attn_precision")]


class SoarClipArgs(C.Structure):
    """Mirror of ``struct SoarClipArgs`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "L", "run_layers", "final_norm")] + [("ids", _vp), ("patches", _vp), ("out", _vp),
                ("n_probes", C.c_int32), ("probe_code", C.c_int32 * CLIP_MAX_PROBES), ("probe_dst", _vp * CLIP_MAX_PROBES)]


class SoarClipAttnArgs(C.Structure):
    """Mirror of ``struct SoarClipAttnArgs`` (include/soar_hip.h)."""
    _fields_ = [(n, _vp) for n in ("q", "k", "v", "out")] + [(n, C.c_int64) for n in ("ldq", "ldk", "ldv", "ldo")] + \
               [(n, C.c_int32) for n in ("B", "Lq", "Lk", "heads", "hd", "causal")] + [("scale", C.c_float)]


class SoarResamplerConfig(C.Structure):
    """Mirror of ``struct SoarResamplerConfig`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("dim", "depth", "heads", "dim_head", "queries", "emb", "out", "ff", "precision", "attn_precision")]


class SoarResamplerArgs(C.Structure):
    """Mirror of ``struct SoarResamplerArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("n", C.c_int32), ("x", _vp), ("out", _vp), ("n_probes", C.c_int32),
                ("probe_code", C.c_int32 * CLIP_MAX_PROBES), ("probe_dst", _vp * CLIP_MAX_PROBES)]


POSE_PAF, POSE_HEAT, POSE_PARTS, POSE_PAIRS = 52, 26, 25, 26      # SOAR_POSE_PAF, SOAR_POSE_HEAT, SOAR_POSE_PARTS, SOAR_POSE_PAIRS
POSE_MAX_STAGES, POSE_MAX_PEAKS, POSE_MAX_PEOPLE = 8, 32, 32     # SOAR_POSE_MAX_STAGES, SOAR_POSE_MAX_PEAKS, SOAR_POSE_MAX_PEOPLE


class SoarPoseConfig(C.Structure):
    """Mirror of ``struct SoarPoseConfig`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("c1", "c2", "c3", "c4", "cpm", "feat", "w0", "w1", "m0", "m1", "n_paf", "n_heat")]


class SoarPoseNetArgs(C.Structure):
    """Mirror of ``struct SoarPoseNetArgs`` (include/soar_hip.h)."""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("pad_", C.c_int32), ("x", _vp), ("x_stride", C.c_int64 * 4),
                ("features", _vp), ("stage_out", _vp * (2 * POSE_MAX_STAGES))]


class SoarPoseAssembleArgs(C.Structure):
    """Mirror of ``struct SoarPoseAssembleArgs`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "h", "w", "max_peaks", "max_people", "min_parts")] + \
               [(n, C.c_float) for n in ("inter_threshold", "min_above", "min_score")] + \
               [(n, C.c_int8 * POSE_PAIRS) for n in ("pair_a", "pair_b", "paf_x", "paf_y")] + \
               [(n, _vp) for n in ("peaks", "counts", "paf", "people", "n_people")]


CPM_FRONT, CPM_MAX_STAGES = 15, 8                                # SOAR_CPM_FRONT, SOAR_CPM_MAX_STAGES
CPM_MAX_LAYERS = 17 + 7 * (CPM_MAX_STAGES - 1)                   # SOAR_CPM_MAX_LAYERS


class SoarCpmConfig(C.Structure):
    """Mirror of ``struct SoarCpmConfig`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_stages", "n_maps", "n_layers", "pool_mask", "maps_first", "pad_")] + \
               [("width", C.c_int32 * CPM_MAX_LAYERS), ("side", C.c_int32 * CPM_MAX_LAYERS)]


class SoarCpmArgs(C.Structure):
    """Mirror of ``struct SoarCpmArgs`` (include/soar_hip.h)."""
    _fields_ = [("M", C.c_int32), ("S", C.c_int32), ("x", _vp), ("x_stride", C.c_int64 * 4), ("features", _vp),
                ("stage_out", _vp * CPM_MAX_STAGES)]


class SoarPartBoxArgs(C.Structure):
    """Mirror of ``struct SoarPartBoxArgs`` (include/soar_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("B", "max_people", "part_people", "pad_")] + \
               [(n, C.c_float) for n in ("hand_min_conf", "min_hand_area", "face_min_conf", "min_face_area")] + \
               [(n, _vp) for n in ("people", "n_people", "boxes")]


# name -> (restype, argtypes); every symbol include/soar_hip.h declares
SIGNATURES = {
    "soar_last_error": (C.c_char_p, []),
    "soar_abi_version": (C.c_int, []),
    "soar_rast_geometry_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_rast_image_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_rast_binning_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "soar_rast_backward_workspace_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_rast_forward_geometry": (C.c_int, [C.POINTER(SoarRastParams)] + [_vp] * 7 + [_vp, _vp, C.POINTER(C.c_int64), _vp]),
    "soar_rast_num_rendered": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(C.c_int64), _vp]),
    "soar_rast_binning_status": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _vp]),
    "soar_rast_binning_status_sticky": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, _vp]),
    "soar_rast_binning_status_async": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, _vp]),
    "soar_rast_prefilter_violations": (C.c_int, [_vp, C.c_int32, C.c_int32, C.POINTER(C.c_int64), _vp]),
    "soar_rast_forward_render": (C.c_int, [C.POINTER(SoarRastParams), _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "soar_rast_forward_render_occ": (C.c_int, [C.POINTER(SoarRastParams), _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp,
                                               _vp, _vp, _vp]),
    "soar_rast_backward": (C.c_int, [C.POINTER(SoarRastParams)] + [_vp] * 7 + [_vp, _vp, _vp, C.c_int64] + [_vp] * 4
                           + [_vp] * 11 + [_vp, C.c_size_t, _vp]),
    "soar_rast_backward_scaled": (C.c_int, [C.POINTER(SoarRastParams)] + [_vp] * 7 + [_vp, _vp, _vp, C.c_int64] + [_vp] * 5
                                  + [_vp] * 11 + [_vp, C.c_size_t, _vp]),
    "soar_rast_backward_occ": (C.c_int, [C.POINTER(SoarRastParams)] + [_vp] * 7 + [_vp, _vp, _vp, C.c_int64] + [_vp] * 6 + [C.c_int32]
                               + [_vp] * 12 + [_vp, C.c_size_t, _vp]),
    "soar_rast_backward_plan": (C.c_int, [C.POINTER(SoarRastParams), C.c_int32] + [_vp] * 7 + [_vp, _vp, _vp, C.c_int64] + [_vp] * 4
                                + [_vp] * 11 + [_vp, C.c_size_t, _vp]),
    "soar_rast_backward_plan_loss": (C.c_int, [C.POINTER(SoarRastParams), C.c_int32] + [_vp] * 7 + [_vp, _vp, _vp, C.c_int64] + [_vp]
                                     + [_vp] * 11 + [_vp, C.c_size_t, _vp, _vp]),
    "soar_rast_backward_occ_plan": (C.c_int, [C.POINTER(SoarRastParams), C.c_int32] + [_vp] * 7 + [_vp, _vp, _vp, C.c_int64] + [_vp] * 6
                                    + [C.c_int32] + [_vp] * 12 + [_vp, C.c_size_t, _vp]),
    "soar_rast_backward_region_counts": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "soar_batch_begin": (C.c_int, [C.c_int32]),
    "soar_batch_frame": (C.c_int, [C.c_int32]),
    "soar_batch_end": (C.c_int, []),
    "soar_rast_occ_backward": (C.c_int, [C.POINTER(SoarRastParams), _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp]),
    "soar_rast_mark_visible": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "soar_rast_export_state": (C.c_int, [C.POINTER(SoarRastParams), _vp, _vp, _vp, C.c_int64] + [_vp] * 17 + [_vp]),
    "soar_lbs_knn_weights_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_lbs_knn_weights": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "soar_lbs_knn_grid_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_lbs_knn_query_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_lbs_knn_build_grid": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _vp, _vp]),
    "soar_lbs_knn_query": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "soar_lbs_knn_query_ordered": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp,
                                             _vp, C.c_size_t, _vp]),
    "soar_lbs_knn_state_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_lbs_knn_query_state": (C.c_int, [_vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "soar_lbs_knn_refresh": (C.c_int, [_vp, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "soar_lbs_warp_forward": (C.c_int, [_vp] * 6 + [C.c_int32, C.c_int32] + [_vp] * 4),
    "soar_lbs_warp_backward": (C.c_int, [_vp] * 5 + [C.c_int32, C.c_int32] + [_vp] * 5),
    "soar_lbs_warp_forward_batch": (C.c_int, [_vp] * 4 + [C.c_int32] * 3 + [_vp] * 3),
    "soar_lbs_warp_backward_sum": (C.c_int, [_vp] * 4 + [C.c_int32] * 3 + [_vp] * 4 + [C.c_int32, _vp, _vp, _vp, _vp]),
    "soar_frames_warp_preprocess": (C.c_int, [C.c_int32, _vp] + [_vp] * 4 + [C.c_int32, C.c_int32] + [_vp] * 6),
    "soar_rast_backward_rows": (C.c_int, [_vp] * 22),
    "soar_frames_geometry_warp_backward": (C.c_int, [C.c_int32, _vp] + [_vp] * 4 + [C.c_int32, C.c_int32] + [_vp] * 7),
    "soar_frames_geometry_warp_backward_losses": (C.c_int, [C.c_int32, _vp] + [_vp] * 4 + [C.c_int32, C.c_int32] + [_vp] * 8),
    "soar_frames_geometry_warp_backward_wave_losses": (C.c_int, [C.c_int32, _vp] + [_vp] * 4 + [C.c_int32, C.c_int32] + [_vp] * 8),
    "soar_dist2_knn3": (C.c_int, [_vp, C.c_int32, _vp, _vp]),
    "soar_depth2normal": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp]),
    "soar_depth2normal_backward": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp,
                                             _vp]),
    "soar_normal2curv": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp]),
    "soar_normal2curv_backward": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "soar_view_finish": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "soar_view_finish_backward": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _vp,
                                            _vp, _vp]),
    "soar_ssim_scratch_floats": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_ssim": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "soar_ssim_rendered": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "soar_densify_stats": (C.c_int, [C.c_int32, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "soar_densify_plan_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_densify_plan": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float,
                                    C.c_float, _vp, C.POINTER(C.c_int64), _vp]),
    "soar_densify_flags": (C.c_int, [C.c_int32, _vp, _vp, _vp]),
    "soar_densify_apply": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_int32, C.POINTER(SoarDensifyRow), _vp, _vp, _vp, C.c_int32, _vp]),
    "soar_smplx_joint_mats": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "soar_image_loss_scratch_floats": (C.c_int, [C.POINTER(C.c_size_t)]),
    "soar_masked_l1": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "soar_masked_l1_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "soar_cos_loss": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp]),
    "soar_cos_loss_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "soar_frame_loss": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, C.c_float, C.c_float,
                                  C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp]),
    "soar_frame_loss_pooled": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_float, C.c_float, C.c_float,
                                         C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp]),
    "soar_frame_loss_partials": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_float, C.c_float, C.c_float,
                                           C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "soar_frame_loss_pooled_partials": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_float, C.c_float,
                                                  C.c_float, C.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp]),
    "soar_selftest_exp": (C.c_int, [_vp, C.c_int32, _vp, _vp, _vp]),
    "soar_selftest_affine_scan": (C.c_int, [_vp, _vp, _vp, _vp]),
    "soar_selftest_conv_gemm": (C.c_int, [C.POINTER(SoarConvGemmArgs), C.POINTER(C.c_int32), _vp]),
    "soar_selftest_conv_pack": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, _vp]),
    "soar_selftest_conv_gemm16": (C.c_int, [C.POINTER(SoarConvGemmArgs), C.c_int32, C.POINTER(C.c_int32), _vp]),
    "soar_selftest_conv_pack16": (C.c_int, [_vp, _vp] + [C.c_int32] * 5 + [_vp]),
    "soar_selftest_conv_pack16_bwd": (C.c_int, [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, _vp]),
    "soar_selftest_conv_gemm_act": (C.c_int, [C.POINTER(SoarConvGemmArgs), C.c_int32, C.c_int32, C.POINTER(C.c_int32), _vp]),
    "soar_selftest_conv_gemm_slope": (C.c_int, [C.POINTER(SoarConvGemmArgs), C.c_int32, C.c_int32, _vp, C.POINTER(C.c_int32), _vp]),
    "soar_prof_enable": (C.c_int, [C.c_int]),
    "soar_prof_reset": (C.c_int, []),
    "soar_prof_stage_count": (C.c_int, []),
    "soar_prof_stage_name": (C.c_char_p, [C.c_int]),
    "soar_prof_read": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "soar_sum_frames": (C.c_int, [C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "soar_gather_step_inputs": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "soar_gather_step_inputs_ids": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp]),
    "soar_prof_timestamp": (C.c_int, [_vp, C.c_int64, C.c_int64, _vp]),
    "soar_view_buffer_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_views_grad_scratch_floats": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_views_forward": (C.c_int, [C.POINTER(SoarPoseArgs), C.c_int32, C.POINTER(SoarViewArgs), _vp]),
    "soar_views_backward": (C.c_int, [C.POINTER(SoarPoseArgs), C.c_int32, C.POINTER(SoarViewArgs), _vp]),
    "soar_step_views_forward": (C.c_int, [C.c_int32, C.POINTER(SoarPoseArgs), C.POINTER(C.c_int32), C.POINTER(SoarViewArgs), _vp]),
    "soar_step_views_backward": (C.c_int, [C.c_int32, C.POINTER(SoarPoseArgs), C.POINTER(C.c_int32), C.POINTER(SoarViewArgs), _vp]),
    "soar_cameras_from_c2w": (C.c_int, [C.c_int32, _vp, C.POINTER(C.c_float), C.POINTER(SoarCameraSpec), _vp, _vp]),
    "soar_rast_forward_render_status": (C.c_int, [C.POINTER(SoarRastParams), _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp]),
    "soar_lbs_warp_backward_views": (C.c_int, [_vp] * 5 + [C.c_int32] * 3 + [_vp] * 4 + [C.c_int32, _vp, _vp, _vp, _vp]),
    "soar_avatar_loss_scratch_floats": (C.c_int, [C.POINTER(C.c_size_t)]),
    "soar_avatar_pixel_losses": (C.c_int, [C.POINTER(SoarAvatarLossArgs), C.c_int32, _vp]),
    "soar_adam_step": (C.c_int, [C.c_int32, C.POINTER(SoarAdamRow), C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "soar_adam_step_at": (C.c_int, [C.c_int32, C.POINTER(SoarAdamRow), C.c_double, C.c_double, C.c_double, C.c_int64, _vp]),
    "soar_adam_step_at_gather": (C.c_int, [C.c_int32, C.POINTER(SoarAdamRow), C.c_double, C.c_double, C.c_double, C.c_int64] + [C.c_int32] * 4
                                 + [C.POINTER(C.c_int32), _vp, _vp, _vp, _vp]),
    "soar_adam_step_rows": (C.c_int, [C.c_int32, C.POINTER(SoarAdamRow), C.c_double, C.c_double, C.c_double, _vp, C.c_int32, _vp]),
    "soar_adam_step_rows_wide": (C.c_int, [C.c_int32, C.POINTER(SoarAdamRow), C.c_double, C.c_double, C.c_double, _vp, C.c_int32, _vp]),
    "soar_tsdf_integrate": (C.c_int, [C.c_int32] * 3 + [_vp] * 5 + [C.c_float] * 4 + [C.c_int32] * 3 + [C.c_float] * 3 + [_vp] * 3),
    "soar_mc_workspace_bytes": (C.c_int, [C.c_int32] * 3 + [C.POINTER(C.c_size_t)]),
    "soar_mc_count": (C.c_int, [C.c_int32] * 3 + [_vp, _vp, C.c_float, _vp, C.c_size_t, C.POINTER(C.c_int64), _vp]),
    "soar_mc_emit": (C.c_int, [C.c_int32] * 3 + [_vp, _vp, C.c_float, _vp, C.c_size_t, _vp, _vp, _vp]),
    "soar_mesh_filter_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_filter_components": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_int32, C.c_float, _vp, C.c_size_t, _vp, _vp,
                                              C.POINTER(C.c_int64), _vp]),
    "soar_mesh_simplify_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_simplify_count": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_float, _vp, C.c_size_t, C.POINTER(C.c_int64), _vp]),
    "soar_mesh_simplify": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_float, _vp, C.c_size_t, _vp, _vp, C.POINTER(C.c_int64), _vp]),
    "soar_mesh_attr_transfer_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_attr_transfer": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "soar_mesh_adjacency_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_adjacency": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "soar_mesh_smooth_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_smooth": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_int32, _vp, C.c_size_t, _vp, _vp]),
    "soar_mesh_prune_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_prune": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, _vp, C.c_size_t, _vp, _vp, _vp,
                                  C.POINTER(C.c_int64), _vp]),
    "soar_mesh_close_holes_bytes": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_close_holes": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, C.c_size_t, _vp, _vp, _vp,
                                        C.POINTER(C.c_int64), _vp]),
    "soar_mesh_repair_workspace_size": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_repair_count": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_int64), _vp]),
    "soar_mesh_repair": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp, C.POINTER(C.c_int64), _vp]),
    "soar_mesh_atlas_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_atlas_levels": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32, _vp, C.c_size_t, C.POINTER(C.c_int64), _vp]),
    "soar_mesh_atlas_place": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "soar_mesh_texels_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_texel_offsets": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_int64), _vp]),
    "soar_mesh_texels": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int64, C.c_int32, _vp, _vp,
                                   _vp, _vp, _vp, _vp]),
    "soar_mesh_texture_write": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "soar_field_workspace_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_field_forward": (C.c_int, [C.POINTER(SoarFieldArgs), _vp]),
    "soar_field_backward": (C.c_int, [C.POINTER(SoarFieldArgs), _vp, C.c_size_t, _vp]),
    "soar_envmap_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_envmap_forward": (C.c_int, [C.POINTER(SoarEnvmapArgs), _vp]),
    "soar_envmap_backward": (C.c_int, [C.POINTER(SoarEnvmapArgs), _vp, C.c_size_t, _vp]),
    "soar_lpips_weights_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
    "soar_lpips_pack_weights": (C.c_int, [C.POINTER(SoarLpipsWeights), _vp, C.c_size_t, _vp]),
    "soar_lpips_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_lpips_forward": (C.c_int, [C.POINTER(SoarLpipsArgs), _vp, C.c_size_t, _vp]),
    "soar_lpips_backward": (C.c_int, [C.POINTER(SoarLpipsArgs), _vp, C.c_size_t, _vp]),
    "soar_vae_weights_floats": (C.c_int, [C.POINTER(C.c_size_t)]),
    "soar_vae_weights_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
    "soar_vae_pack_weights": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, _vp]),
    "soar_vae_workspace_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_vae_forward": (C.c_int, [C.POINTER(SoarVaeArgs), _vp, C.c_size_t, _vp]),
    "soar_vae_backward": (C.c_int, [C.POINTER(SoarVaeArgs), _vp, C.c_size_t, _vp]),
    "soar_vae_weights_bytes16": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_vae_pack_weights16": (C.c_int, [_vp, C.c_size_t, _vp, C.c_size_t, C.c_int32, _vp]),
    "soar_vae_forward16": (C.c_int, [C.POINTER(SoarVaeArgs), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_vae_backward16": (C.c_int, [C.POINTER(SoarVaeArgs), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_sds_q_sample": (C.c_int, [C.POINTER(SoarSdsArgs), _vp]),
    "soar_sds_loss": (C.c_int, [C.POINTER(SoarSdsArgs), _vp]),
    "soar_surfel_activations_forward": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 10 + [_vp]),
    "soar_surfel_activations_backward": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 16 + [_vp]),
    "soar_surfel_regularizers_workspace_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_surfel_regularizers": (C.c_int, [C.c_int32] * 3 + [_vp] * 11 + [_vp, C.c_size_t, _vp]),
    "soar_smplx_vertices": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int32] + [_vp] * 8 + [_vp]),
    "soar_mesh_workspace_bytes": (C.c_int, [C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_mesh_subdivide_edges": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_size_t, C.POINTER(C.c_int64), _vp]),
    "soar_mesh_subdivide": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp, C.c_size_t, _vp, _vp, _vp]),
    "soar_mesh_vertex_normals": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp, C.c_size_t, _vp, _vp]),
    "soar_mesh_vertex_frames": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp]),
    "soar_data_mask_bbox": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "soar_data_crops": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "soar_data_step_batch": (C.c_int, [C.POINTER(SoarDataStepArgs), _vp]),
    "soar_eval_scratch_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_eval_image_metrics": (C.c_int, [C.POINTER(SoarEvalArgs), _vp, C.c_size_t, _vp]),
    "soar_motion_resample": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [_vp] * 8 + [_vp]),
    "soar_playback_finish": (C.c_int, [C.POINTER(SoarPlaybackArgs), _vp]),
    "soar_normalnet_weights_bytes": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_normalnet_pack_weights": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_normalnet_workspace_bytes": (C.c_int, [C.c_int32] * 6 + [C.POINTER(C.c_size_t)]),
    "soar_normalnet_forward": (C.c_int, [C.POINTER(SoarNormalNetArgs), _vp, C.c_size_t, _vp]),
    "soar_normal_crop_boxes": (C.c_int, [C.c_int32] * 4 + [_vp, C.POINTER(C.c_int64), _vp, _vp, _vp, _vp, _vp]),
    "soar_normal_crop_sample": (C.c_int, [C.c_int32] * 4 + [_vp, C.POINTER(C.c_int64), _vp, C.POINTER(C.c_int64), _vp, _vp, _vp, _vp]),
    "soar_normal_crop_bytes": (C.c_int, [C.c_int32] * 3 + [_vp] * 6 + [_vp]),
    "soar_smplify_objective": (C.c_int, [C.POINTER(SoarSmplifyRig), C.POINTER(SoarSmplifyArgs), _vp]),
    "soar_smplify_objective_body": (C.c_int, [C.POINTER(SoarSmplifyRig), C.POINTER(SoarSmplifyBody), C.POINTER(SoarSmplifyArgs), _vp]),
    "soar_smplify_target_scales": (C.c_int, [C.c_int32, _vp, C.c_float, C.c_float, _vp, _vp]),
    "soar_smplify_model_points": (C.c_int, [C.POINTER(SoarSmplifyRig), C.POINTER(SoarSmplifyBody), C.POINTER(SoarSmplifyArgs), C.c_int32,
                                            _vp, _vp, _vp, _vp]),
    "soar_pose_init_search": (C.c_int, [C.POINTER(SoarPoseSearch), _vp]),
    "soar_pose_init_viterbi": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 8 + [_vp]),
    "soar_prior_vertex_setup": (C.c_int, [C.c_int32] * 3 + [_vp, C.POINTER(C.c_int64), _vp, C.c_int32] + [_vp] * 7 + [_vp]),
    "soar_prior_face_boxes": (C.c_int, [C.c_int32] * 3 + [_vp] * 3 + [_vp]),
    "soar_prior_raster": (C.c_int, [C.c_int32] * 6 + [_vp] * 8 + [_vp]),
    "soar_masks_workspace_bytes": (C.c_int, [C.c_int32] * 3 + [C.POINTER(C.c_size_t)]),
    "soar_masks_open_close": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int32, C.c_float, _vp, _vp, _vp, C.c_size_t, _vp]),
    "soar_masks_largest_component": (C.c_int, [C.c_int32] * 3 + [_vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "soar_masks_clean": (C.c_int, [C.c_int32] * 4 + [_vp, C.c_int32, C.c_float, _vp, _vp, _vp, C.c_size_t, _vp]),
    "soar_step_terms_scratch_bytes": (C.c_int, [C.POINTER(C.c_size_t)]),
    "soar_consistency_loss": (C.c_int, [C.c_int32] * 3 + [_vp, C.c_int64, _vp, C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp]),
    "soar_consistency_loss_backward": (C.c_int, [C.c_int32] * 3 + [_vp, C.c_int64, _vp, C.c_int64, C.c_float, C.c_float, _vp, _vp, _vp, _vp,
                                                 _vp]),
    "soar_normal_view_terms": (C.c_int, [C.POINTER(SoarNormalViewArgs), C.c_int32, _vp]),
    "soar_frame_extra_terms": (C.c_int, [C.POINTER(SoarFrameExtraArgs), _vp]),
    "soar_frame_extra_terms_backward": (C.c_int, [C.POINTER(SoarFrameExtraArgs), _vp]),
    "soar_abs_mean": (C.c_int, [C.c_int64, _vp, _vp, _vp, _vp]),
    "soar_abs_mean_backward": (C.c_int, [C.c_int64, _vp, _vp, _vp, _vp]),
    "soar_fitviz_yaw_views": (C.c_int, [C.c_int32] * 3 + [_vp, C.POINTER(C.c_int64), _vp, _vp, _vp, _vp]),
    "soar_fitviz_strip": (C.c_int, [C.POINTER(SoarFitvizStripArgs), _vp]),
    "soar_fitviz_residuals": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, C.c_float, _vp, _vp]),
    "soar_jpeg_workspace_bytes": (C.c_int, [C.POINTER(SoarJpegArgs), C.POINTER(C.c_size_t)]),
    "soar_jpeg_measure": (C.c_int, [C.POINTER(SoarJpegArgs), _vp, C.c_size_t, _vp, _vp]),
    "soar_jpeg_emit": (C.c_int, [C.POINTER(SoarJpegArgs), _vp, C.c_size_t, _vp, C.c_int64, _vp]),
    "soar_png_workspace_bytes": (C.c_int, [C.POINTER(SoarPngArgs), C.POINTER(C.c_size_t)]),
    "soar_png_measure": (C.c_int, [C.POINTER(SoarPngArgs), _vp, C.c_size_t, _vp, _vp]),
    "soar_png_emit": (C.c_int, [C.POINTER(SoarPngArgs), _vp, C.c_size_t, _vp, C.c_int64, _vp]),
    "soar_png_decode_workspace_bytes": (C.c_int, [C.POINTER(SoarPngDecodeArgs), C.POINTER(C.c_size_t)]),
    "soar_png_decode": (C.c_int, [C.POINTER(SoarPngDecodeArgs), _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "soar_jpeg_decode_workspace_bytes": (C.c_int, [C.POINTER(SoarJpegDecodeArgs), C.POINTER(C.c_size_t)]),
    "soar_jpeg_decode": (C.c_int, [C.POINTER(SoarJpegDecodeArgs), _vp, C.c_size_t, _vp, _vp, _vp, _vp]),
    "soar_resize_u8": (C.c_int, [C.POINTER(SoarResizeArgs), _vp, _vp]),
    "soar_sam_weights_bytes": (C.c_int, [C.POINTER(SoarSamConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "soar_sam_pack_weights": (C.c_int, [C.POINTER(SoarSamConfig), C.POINTER(_vp), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_sam_workspace_bytes": (C.c_int, [C.POINTER(SoarSamConfig), C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_sam_preprocess": (C.c_int, [C.POINTER(SoarSamConfig), C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp]),
    "soar_sam_encode": (C.c_int, [C.POINTER(SoarSamConfig), _vp, C.POINTER(SoarSamEncodeArgs), _vp, C.c_size_t, _vp]),
    "soar_sam_decode": (C.c_int, [C.POINTER(SoarSamConfig), _vp, C.POINTER(SoarSamDecodeArgs), _vp, C.c_size_t, _vp]),
    "soar_sam_postprocess": (C.c_int, [C.c_int32] * 8 + [_vp, _vp, _vp, _vp]),
    "soar_sam_attention": (C.c_int, [_vp] * 5 + [C.c_int32] * 6 + [C.c_float, _vp]),
    "soar_unet_weights_bytes": (C.c_int, [C.POINTER(SoarUnetConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "soar_unet_pack_weights": (C.c_int, [C.POINTER(SoarUnetConfig), C.POINTER(_vp), C.POINTER(C.c_int64), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_unet_workspace_bytes": (C.c_int, [C.POINTER(SoarUnetConfig)] + [C.c_int32] * 5 + [C.POINTER(C.c_size_t)]),
    "soar_unet_forward": (C.c_int, [C.POINTER(SoarUnetConfig), _vp, C.POINTER(SoarUnetArgs), _vp, C.c_size_t, _vp]),
    "soar_unet_attention": (C.c_int, [C.POINTER(SoarUnetAttnArgs), _vp]),
    "soar_attention16": (C.c_int, [C.POINTER(SoarUnetAttnArgs), C.c_int32, C.c_int32, _vp]),
    "soar_clip_weights_bytes": (C.c_int, [C.POINTER(SoarClipConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "soar_clip_pack_weights": (C.c_int, [C.POINTER(SoarClipConfig), C.POINTER(_vp), C.POINTER(C.c_int64), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_clip_workspace_bytes": (C.c_int, [C.POINTER(SoarClipConfig), C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_clip_preprocess": (C.c_int, [C.POINTER(SoarClipConfig), C.c_int32, _vp, _vp, _vp]),
    "soar_clip_forward": (C.c_int, [C.POINTER(SoarClipConfig), _vp, C.POINTER(SoarClipArgs), _vp, C.c_size_t, _vp]),
    "soar_clip_attention": (C.c_int, [C.POINTER(SoarClipAttnArgs), _vp]),
    "soar_resampler_weights_bytes": (C.c_int, [C.POINTER(SoarResamplerConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    "soar_resampler_pack_weights": (C.c_int, [C.POINTER(SoarResamplerConfig), C.POINTER(_vp), C.POINTER(C.c_int64), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_resampler_workspace_bytes": (C.c_int, [C.POINTER(SoarResamplerConfig), C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_resampler_forward": (C.c_int, [C.POINTER(SoarResamplerConfig), _vp, C.POINTER(SoarResamplerArgs), _vp, C.c_size_t, _vp]),
    "soar_pose_weights_size": (C.c_int, [C.POINTER(SoarPoseConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "soar_pose_workspace_size": (C.c_int, [C.POINTER(SoarPoseConfig), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_pose_pack_weights": (C.c_int, [C.POINTER(SoarPoseConfig), C.POINTER(_vp), C.POINTER(C.c_int64), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_pose_preprocess": (C.c_int, [C.c_int32] * 3 + [_vp, _vp, _vp]),
    "soar_pose_forward": (C.c_int, [C.POINTER(SoarPoseConfig), _vp, C.POINTER(SoarPoseNetArgs), _vp, C.c_size_t, _vp]),
    "soar_pose_peaks": (C.c_int, [C.c_int32] * 3 + [_vp, C.c_float, C.c_int32, _vp, _vp, _vp]),
    "soar_pose_assemble": (C.c_int, [C.POINTER(SoarPoseAssembleArgs), _vp]),
    "soar_pose_scale": (C.c_int, [C.c_int64, _vp, C.c_float, C.c_float, C.c_float, C.c_float, _vp]),
    "soar_cpm_weights_size": (C.c_int, [C.POINTER(SoarCpmConfig), C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]),
    "soar_cpm_workspace_size": (C.c_int, [C.POINTER(SoarCpmConfig), C.c_int32, C.c_int32, C.POINTER(C.c_size_t)]),
    "soar_cpm_pack_weights": (C.c_int, [C.POINTER(SoarCpmConfig), C.POINTER(_vp), C.POINTER(C.c_int64), C.c_int32, _vp, C.c_size_t, _vp]),
    "soar_cpm_forward": (C.c_int, [C.POINTER(SoarCpmConfig), _vp, C.POINTER(SoarCpmArgs), _vp, C.c_size_t, _vp]),
    "soar_part_boxes": (C.c_int, [C.POINTER(SoarPartBoxArgs), _vp]),
    "soar_part_crop": (C.c_int, [C.c_int32] * 5 + [_vp] * 5),
    "soar_part_keypoints": (C.c_int, [C.c_int32] * 4 + [_vp, _vp, C.c_int32, _vp, _vp]),
}

_lib: Optional[C.CDLL] = None


class SoarHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libsoar_hip.so (once).  Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        # PyTorch-ROCm ships its own HIP runtime: it must be the one this process uses, so torch is loaded first (this module imports
        # it; loading libsoar_hip.so first would pull a second libamdhip64 from /opt/rocm into the process)
        if not os.path.exists(LIB_PATH):
            raise SoarHipError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m soar_amd.build` "
                "(hipcc --offload-arch=gfx950). soar_amd has no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError if a declared symbol is missing
            fn.restype = res
            fn.argtypes = args
        if handle.soar_abi_version() != ABI_VERSION:
            raise SoarHipError("libsoar_hip.so ABI version mismatch; rebuild with `python -m soar_amd.build --force`")
        _lib = handle
    return _lib


def last_error() -> str:
    msg = lib().soar_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise SoarHipError(f"{what} failed: {last_error()}")


def _bytes(fn, name: str, *sizes) -> int:
    """What the sizing call ``fn`` (named ``name`` in the error) answers for ``sizes``."""
    nb = C.c_size_t(0)
    check(fn(*sizes, C.byref(nb)), name)
    return nb.value


def _workspace(nbytes: int, device):
    """A caller-owned workspace of ``nbytes`` on ``device``, as every entry point that takes one wants it."""
    buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    if buf.data_ptr() % 256:
        raise RuntimeError("device allocation is not 256-byte aligned")
    return buf


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


class PackedWeights:
    """The packed form of a net's weights, kept until a weight moves or is written in place."""

    def __init__(self):
        self._key = self.packed = None

    def get(self, tensors, device, wrong_device: str, pack):
        """``tensors``: the module's weights; ``wrong_device``: the module's error text for weights that are not on ``device``;
        ``pack()`` packs them into fresh buffers and returns those.  -> what ``pack()`` returned, now or for the same weights."""
        if any(w.device != device for w in tensors):
            raise RuntimeError(wrong_device)
        key = (device, tuple(w.data_ptr() for w in tensors), tuple(w._version for w in tensors))
        if key != self._key:
            self.packed = pack()
            self._key = key
        return self.packed


def ptr(t) -> Optional[int]:
    """Device/host pointer of a torch tensor (None for an empty / missing tensor, like the reference's nullptr)."""
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()
