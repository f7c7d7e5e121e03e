/*
 * include/soar_hip.h -- C ABI of libsoar_hip.so, the MI355X (gfx950) implementation of SOAR's
 * per-frame avatar path: Gaussian-surfel rasterizer forward/backward, SMPL-X LBS warp, 3-NN distance.
 *
 * Every entry point replaces one interface of the reference (hangg7/soar); citations are file:line
 * relative to the reference root, DGR/ = submodules/diff-gaussian-rasterization/,
 * TS/ = soar/threestudio-soar/.
 *
 * Conventions
 *  - plain pointers and sizes only; no torch / STL types cross the boundary;
 *  - pointers named *_dev (and all array arguments unless stated otherwise) are DEVICE pointers;
 *    they may be NULL exactly where the reference accepts an empty tensor;
 *  - `stream` is a hipStream_t passed as void* (PyTorch-ROCm: torch.cuda.current_stream().cuda_stream);
 *  - every function returns 0 on success and non-zero on failure; soar_last_error() then holds a
 *    message (thread-local).  Nothing throws across the ABI;
 *  - outputs and gradient arrays are fully written (or zero-filled) by the callee, so the caller
 *    may pass uninitialised memory (the reference zero-fills in DGR/rasterize_points.cu:61-66,133-147);
 *  - the three scratch buffers (geometry / binning / image) are opaque, caller-owned byte arrays, as in
 *    the reference (DGR/rasterize_points.cu:68-75): sizes come from soar_rast_*_bytes(), the same
 *    buffers must be handed to soar_rast_backward().  Base pointers must be 256-byte aligned.
 */
#ifndef SOAR_HIP_H
#define SOAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  1: round 1.  2: the KNN query's sort scratch is caller-owned (soar_lbs_knn_query_bytes).  3 (round 2): soar_frame_loss
 * takes SOAR_FRAME_LOSS_SCRATCH_FLOATS floats of scratch, the background colour and the normalize_depth switch; new entry points
 * soar_lbs_warp_forward_batch / soar_lbs_warp_backward_sum, soar_view_finish[_backward], soar_rast_occ_backward;
 * soar_sum_frames_when_last (introduced and withdrawn within round 2) is gone.  4 (round 3): soar_lbs_knn_state_bytes / _query_state /
 * _refresh, soar_adam_step, soar_rast_prefilter_violations, soar_selftest_affine_scan.  5 (round 3): soar_rast_binning_status_async;
 * the geometry buffer grew (ask soar_rast_geometry_bytes); inside the binning buffer the tiles' lists are no longer in tile order
 * (`ranges` says where each list is; soar_rast_export_state re-packs them into the reference's layout).  6 (round 4): the betas and eps
 * of soar_adam_step / _at / _rows are doubles; soar_views_forward / _backward (+ soar_view_buffer_bytes, soar_views_grad_scratch_floats),
 * soar_rast_forward_render_status, soar_lbs_warp_backward_views, soar_rast_binning_status_sticky, soar_avatar_pixel_losses, soar_rast_backward_occ (the image
 * buffer grew by two planes: ask soar_rast_image_bytes), soar_gather_step_inputs_ids;
 * soar_selftest_wave_reduce is gone with the backward form it tested.  7 (round 5): soar_step_views_forward / _backward (several poses
 * behind one call each way), soar_cameras_from_c2w, soar_ssim_rendered, SoarAvatarLossArgs::background.  8 (round 6):
 * soar_frames_warp_preprocess (+ SoarFrameHead; SoarRastParams.debug bit 4) and soar_frames_geometry_warp_backward (+ SoarFrameTail;
 * debug bit 3): the head of the forward pass and the tail of the backward pass of all frames of a step as one kernel each;
 * soar_rast_backward_rows; the geometry buffer grew (one statistics row per 64 Gaussians: ask soar_rast_geometry_bytes) and so did
 * soar_views_grad_scratch_floats (a block per back view).  Still 8, additive: soar_tsdf_integrate, soar_mc_workspace_bytes / _count / _emit,
 * soar_mesh_filter_bytes / _components, soar_mesh_simplify_bytes / _count / soar_mesh_simplify, soar_mesh_attr_transfer[_bytes],
 * soar_mesh_adjacency[_bytes], soar_mesh_smooth[_bytes], soar_mesh_prune[_bytes], soar_mesh_close_holes[_bytes], soar_mesh_repair_workspace_size / _count / soar_mesh_repair, soar_mesh_atlas_bytes / _levels / _place,
 * soar_mesh_texels_bytes / soar_mesh_texel_offsets / soar_mesh_texels / soar_mesh_texture_write (mesh export).  soar_field_workspace_bytes / _forward / _backward (+ SoarFieldHead,
 * SoarFieldArgs: the attribute field).  soar_envmap_workspace_bytes / _forward / _backward (+ SoarEnvmapArgs: the environment-map
 * background).  soar_lpips_weights_bytes / _pack_weights / _workspace_bytes / _forward / _backward (+ SoarLpipsWeights, SoarLpipsArgs:
 * the LPIPS-VGG loss).  soar_vae_weights_floats / _weights_bytes / _pack_weights / _workspace_bytes / _forward / _backward,
 * soar_sds_q_sample / _loss (+ SoarVaeArgs, SoarSdsArgs: the SDS guidance's VAE encoder and loss tail); soar_vae_weights_bytes16 /
 * _pack_weights16 / _forward16 / _backward16: the encoder with bf16 / f16 weight products, both directions.  soar_data_mask_bbox / _crops /
 * _step_batch (+ SoarDataStepArgs: the training data module).  soar_frame_loss_partials / _pooled_partials,
 * soar_frames_geometry_warp_backward_losses (+ SoarLossFinish), soar_adam_step_at_gather: two small launches of the step plan folded
 * into their neighbours.  soar_eval_scratch_bytes / _image_metrics (+ SoarEvalArgs: test-split evaluation).
 * soar_normalnet_weights_bytes / _pack_weights / _workspace_bytes / _forward (+ SoarNormalNetArgs), soar_normal_crop_boxes / _sample /
 * _bytes: normal-map preprocessing.  soar_selftest_conv_gemm / _conv_pack (+ SoarConvGemmArgs, SoarConvGemmTaps): the shared
 * implicit-GEMM convolution and its weight packer by themselves, for the tests; soar_selftest_conv_gemm16 / _conv_pack16 /
 * _conv_pack16_bwd / _conv_gemm_act: the same with bf16 / f16 operands (SoarUnetConfig.precision uses them).  soar_prior_vertex_setup / _face_boxes / soar_prior_raster: the SMPL-X
 * normal priors (a triangle-mesh rasterizer).  soar_rast_backward_plan_loss (+ SoarBackwardLoss),
 * soar_frames_geometry_warp_backward_wave_losses: the frame loss inside the backward blend's launch.  soar_sam_weights_bytes /
 * _pack_weights / _workspace_bytes / _preprocess / _encode / _decode / _postprocess / _attention (+ SoarSamConfig, SoarSamEncodeArgs,
 * SoarSamDecodeArgs): SAM point-prompt segmentation.  soar_unet_weights_bytes / _pack_weights / _workspace_bytes / _forward / _attention
 * (+ SoarUnetConfig, SoarUnetArgs, SoarUnetAttnArgs): the SDS guidance's multi-view diffusion UNet.  soar_clip_weights_bytes /
 * _pack_weights / _workspace_bytes / _preprocess / _forward / _attention and soar_resampler_weights_bytes / _pack_weights /
 * _workspace_bytes / _forward (+ SoarClipConfig, SoarClipArgs, SoarClipAttnArgs, SoarResamplerConfig, SoarResamplerArgs): the
 * guidance's conditioning, CLIP's two encoders and the image-token Resampler.  soar_attention16: soar_unet_attention's /
 * soar_clip_attention's attention on the 16-bit matrix core (SoarUnetConfig.attn_precision, SoarClipConfig.attn_precision and
 * SoarResamplerConfig.attn_precision use it). */
#define SOAR_HIP_ABI_VERSION 8

/* Mirrors GaussianRasterizationSettings (DGR/diff_gaussian_rasterization/__init__.py:267-284) and the
 * scalar arguments of RasterizeGaussiansCUDA (DGR/rasterize_points.h:17-31). */
typedef struct SoarRastParams {
    int32_t P;                 /* number of Gaussians (means3D.size(0)) */
    int32_t W, H;              /* image_width, image_height */
    int32_t sh_degree;         /* active SH degree D */
    int32_t M;                 /* SH coefficients per Gaussian (sh.size(1)), 0 with colors_precomp */
    int32_t prefiltered;
    int32_t render_front;
    int32_t sort_descending;
    int32_t debug;             /* bit 0: synchronise + check after every stage (CHECK_CUDA, DGR/cuda_rasterizer/auxiliary.h:419-426);
                                  bit 1 (backward only): order-insensitive accumulation -- the per-Gaussian gradient sums of the backward
                                  blend go through float64 atomics instead of float32 ones (the reference's atomicAdd order,
                                  backward.cu:845-855, is undefined; in float64 the order no longer reaches the float32 result).
                                  Test / debugging mode: ~2x the atomic traffic;
                                  bit 2 (forward blend only): the caller states that image_buffer AND every output plane are the ones of
                                  the previous forward call with this image_buffer, untouched since: tiles without Gaussians in both calls
                                  are not written again (their pixels already hold the background values; a background colour or
                                  normalize-depth switch that differs from the previous call's is noticed on the device and every tile is
                                  written).  Never set it on the first call with an image_buffer;
                                  bit 3 (backward only): the call stops behind the backward blend -- the accumulation rows stay in the
                                  workspace and NO gradient output is written; the caller finishes all frames of the step with ONE
                                  soar_frames_geometry_warp_backward (the per-Gaussian stage and the warp's backward in one kernel);
                                  bit 4 (soar_rast_forward_geometry only): the preprocess stage of this frame has been run by
                                  soar_frames_warp_preprocess (the warp and the per-Gaussian forward stage in one kernel): the call goes
                                  straight to what follows it. */
    /* `config` tensor of the reference (TS/geometry/surfel_base.py:166,675-679), as host flags (config[i] > 0) */
    int32_t cfg_surface;       /* config[0] */
    int32_t cfg_normalize_depth; /* config[1] */
    int32_t cfg_perpix_depth;  /* config[2] */
    int32_t cfg_lrn_cam;       /* config[3] */
    float tanfovx, tanfovy;
    float scale_modifier;
    const float *bg_dev;         /* [3]  */
    const float *viewmatrix_dev; /* [16] row-vector (transposed) world->view, element 12..14 = translation */
    const float *projmatrix_dev; /* [16] full projection, same convention */
    const float *prcppoint_dev;  /* [2]  principal point (cx/W, cy/H) */
    const float *patchbbox_dev;  /* [4]  (h0, w0, h1, w1) */
    const float *campos_dev;     /* [3]  */
} SoarRastParams;

/* ---- the same stage of several frames in ONE launch (no reference counterpart) ----
 * Every kernel of the rasterizer's frame chain (geometry, binning, blends, frame loss, backward) takes its frame's argument block
 * by blockIdx.y.  Between soar_batch_begin(n) and soar_batch_end() the caller walks ONE entry point at a time over the n frames
 * of a step -- soar_batch_frame(f) in front of each call, f = 0 .. n-1 in order -- and the library launches every stage once,
 * with gridDim.y = n, when the last frame's call arrives:
 *     soar_batch_begin(4);
 *     for (f = 0; f < 4; f++) { soar_batch_frame(f); soar_rast_forward_geometry(prm[f], ..., stream); }
 *     for (f = 0; f < 4; f++) { soar_batch_frame(f); soar_rast_forward_render_occ(prm[f], ..., capacity, ..., stream); }
 *     ...
 *     soar_batch_end();
 * Requirements: the frames agree in everything that shapes a launch (P, M, W, H, sort order, capacity, buffer alignment, which
 * optional pointers are NULL); sync-free forms only (no num_rendered read-back inside a batch); one stream; per thread (the
 * state is thread-local).  n <= 8.  The calls of the frames 0 .. n-2 only record their argument blocks and return 0. */
int soar_batch_begin(int32_t n_frames);
int soar_batch_frame(int32_t frame);
int soar_batch_end(void);

/* ---- scratch sizing: replaces required<GeometryState/ImageState/BinningState>()
 *      (DGR/cuda_rasterizer/rasterizer_impl.h:77-84, rasterizer_impl.cu:134-184) ---- */
int soar_rast_geometry_bytes(int32_t P, int32_t M, size_t *bytes);
int soar_rast_image_bytes(int32_t W, int32_t H, size_t *bytes);
int soar_rast_binning_bytes(int64_t num_rendered, size_t *bytes);

/* ---- forward, replaces CudaRasterizer::Rasterizer::forward (DGR/cuda_rasterizer/rasterizer_impl.cu:188-312)
 *      split at its one host synchronisation point (the D2H copy of num_rendered, :250-257), because the
 *      binning buffer is sized by the caller from that number (resizeFunctional, DGR/rasterize_points.cu:27-33).
 *
 * stage 1: preprocess (forward.cu:205-385) + inclusive scan (:242-245) + blocking read-back of num_rendered.
 *   means3D [P,3]; opacities [P]; exactly one of shs [P,M,3] / colors_precomp [P,3];
 *   (scales [P,3], rotations [P,4]) or cov3D_precomp [P,6] (the Python layer enforces exactly one; like the reference's _C
 *   module this level also takes rotations WITH cov3D_precomp: covariance from cov3D_precomp, surfel normal from rotations).
 *   radii_out [P] int32 (API output).  *num_rendered_host receives R (NULL: asynchronous form, see below). */
int soar_rast_forward_geometry(const SoarRastParams *prm,
                               const float *means3D, const float *shs, const float *colors_precomp,
                               const float *opacities, const float *scales, const float *rotations,
                               const float *cov3D_precomp,
                               void *geom_buffer, int32_t *radii_out, int64_t *num_rendered_host,
                               void *stream);

/* Asynchronous form of stage 1: pass num_rendered_host == NULL to soar_rast_forward_geometry (no host synchronisation),
 * enqueue the geometry stage of several views / frames, then read each R with this call (it synchronises `stream`
 * once; later calls return immediately).  One sync per batch of views instead of one per view. */
int soar_rast_num_rendered(const void *geom_buffer, int32_t P, int32_t M, int64_t *num_rendered_host, void *stream);

/* Sync-free form of the forward pass: `num_rendered` passed to stage 2 (and to backward) may be any CAPACITY >= the
 * actual number of (tile, Gaussian) instances -- it only sizes / carves the caller's binning buffer (ascending sort;
 * the tile binning of rast_tilebin.hip does not use it otherwise).  The actual number is found on the device; if it
 * exceeds the capacity nothing is binned or rendered (images = background) and this call reports it, so a caller can
 * enqueue whole steps without the reference's blocking read-back (rasterizer_impl.cu:250) and check once afterwards.
 * Synchronises `stream`.  *instances_host = instances found, *overflow_host = 0 or the number that did not fit. */
int soar_rast_binning_status(const void *geom_buffer, int32_t P, int32_t M, int64_t *instances_host, int64_t *overflow_host,
                             void *stream);

/* The largest instance count and the largest overflow over ALL frames binned through this geometry buffer since the two words were
 * last cleared (the tile binning keeps running maxima in the buffer's header; reset != 0 clears them behind the read).  For a
 * caller that keeps its geometry buffers between frames (soar_amd/step_plan.py): one look covers a whole timed region, where
 * soar_rast_binning_status only sees the last frame.  A freshly allocated buffer must be cleared (one call with reset) before its
 * first frame.  Synchronises `stream`. */
int soar_rast_binning_status_sticky(void *geom_buffer, int32_t P, int32_t M, int64_t *max_instances_host, int64_t *max_overflow_host,
                                    int32_t reset, void *stream);

/* The same two words without blocking: copied into `status_pinned` (two uint32 of page-locked host memory: instances found, 0 or the
 * number that did not fit) behind whatever `stream` already holds.  Both words are set to 0xFFFFFFFF by this call and overwritten when
 * the copy lands: the caller polls them (or waits for an event it records behind this call).  What a caller that sizes its binning buffers from earlier frames polls between frames. */
int soar_rast_binning_status_async(const void *geom_buffer, int32_t P, int32_t M, uint32_t *status_pinned, void *stream);

/* `prefiltered` (GaussianRasterizationSettings.prefiltered): the caller promises that no Gaussian is culled.  The reference prints
 * "Point is filtered although prefiltered is set. This shouldn't happen!" from the kernel and traps (auxiliary.h:163-167, 195-199),
 * which takes the context down; here the culled Gaussians are counted on the device.  In debug mode (SoarRastParams.debug bit 0)
 * soar_rast_forward_geometry reads the count and fails with that message; otherwise this call reads it (one stream sync). */
int soar_rast_prefilter_violations(const void *geom_buffer, int32_t P, int32_t M, int64_t *violations_host, void *stream);

/* stage 2: duplicateWithKeys (:66-99) + radix sort on bits [0,32+bit) (:266-285) + identifyTileRanges
 *   (:104-124,287-295) + per-tile blend (forward.cu:390-692).
 *   out_color [3,H,W], out_normal [3,H,W], out_depth [1,H,W], out_opac [1,H,W]. */
int soar_rast_forward_render(const SoarRastParams *prm, const int32_t *radii,
                             void *geom_buffer, void *binning_buffer, void *image_buffer,
                             int64_t num_rendered,
                             float *out_color, float *out_normal, float *out_depth, float *out_opac,
                             void *stream);

/* stage 2 with the occlusion pass fused in.  threestudio-soar rasterizes every frame twice with the same camera and
 * geometry: the main pass and an occlusion pass with render_front = 1 and colours = per-Gaussian occlusion values
 * (TS/renderer/diff_gaussian_rasterizer.py:254-263 and :281-291).  The second pass differs from the first only by the
 * back-face cull in preprocess (forward.cu:262-266), so its per-pixel blend sequence is a subsequence of the first one:
 * this entry point walks the tile lists once and returns, next to the four main images, out_occ [3,H,W] =
 * out_color of that second pass (occ_values [P] broadcast to the three channels, same bg).
 * Requires prm->render_front == 0 and prm->sort_descending == 0.  occ_values == out_occ == NULL: plain stage 2. */
int soar_rast_forward_render_occ(const SoarRastParams *prm, const int32_t *radii,
                                 void *geom_buffer, void *binning_buffer, void *image_buffer,
                                 int64_t num_rendered,
                                 float *out_color, float *out_normal, float *out_depth, float *out_opac,
                                 const float *occ_values, float *out_occ,
                                 void *stream);

/* ---- backward, replaces CudaRasterizer::Rasterizer::backward (DGR/cuda_rasterizer/rasterizer_impl.cu:316-379)
 *      and the gradient allocation of RasterizeGaussiansBackwardCUDA (DGR/rasterize_points.cu:107-187).
 *   dL_dout_* are the four image gradients.  Outputs (all fully written):
 *   dL_dmeans2D [P,3], dL_dcolors [P,3], dL_dopacity [P], dL_dmeans3D [P,3], dL_dcov3D [P,6],
 *   dL_dsh [P,M,3] (may be NULL when M == 0), dL_dscales [P,3], dL_drotations [P,4],
 *   dL_dviewmat [16], dL_dprojmat [16], dL_dcampos [3]. */
int soar_rast_backward(const SoarRastParams *prm,
                       const float *means3D, const int32_t *radii, const float *shs,
                       const float *colors_precomp, const float *scales, const float *rotations,
                       const float *cov3D_precomp,
                       const void *geom_buffer, const void *binning_buffer, const void *image_buffer,
                       int64_t num_rendered,
                       const float *dL_dout_color, const float *dL_dout_normal,
                       const float *dL_dout_depth, const float *dL_dout_opac,
                       float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity, float *dL_dmeans3D,
                       float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drotations,
                       float *dL_dviewmat, float *dL_dprojmat, float *dL_dcampos,
                       void *workspace, size_t workspace_bytes,
                       void *stream);
/* soar_rast_occ_backward: gradient of the occlusion image of soar_rast_forward_render_occ w.r.t. the per-Gaussian occlusion
 * values: dL_docc[i] = sum over pixels of (g_0 + g_1 + g_2) alpha_i T_occ,i -- what the reference gets as dL_dcolors (summed over
 * the three equal channels) of its separate occlusion pass, whose colours are occ.repeat(1, 3) and whose geometry is detached
 * (TS/renderer/diff_gaussian_rasterizer.py:281-291; loss_occ, TS/system/gaussian_surfel_mvdream.py:412-417).  One walk of the
 * MAIN pass's lists (its geom / binning / image buffers: render_front = 0, sort_descending = 0) over the camera-facing entries,
 * same arithmetic as the forward's occlusion chain.  dL_dout_occ [3,H,W]; dL_docc [P], overwritten. */
int soar_rast_occ_backward(const SoarRastParams *prm, const void *geom_buffer, const void *binning_buffer,
                           const void *image_buffer, int64_t num_rendered, const float *dL_dout_occ, float *dL_docc,
                           void *stream);
/* soar_rast_backward and soar_rast_occ_backward in ONE walk of the lists (round 4): the backward blend also takes the fused
 * occlusion chain of soar_rast_forward_render_occ back to front -- from the chain's final transmittance and last contributor, which
 * that forward left in the image buffer -- with T in front of an entry recovered by division like the reference's own backward pass of
 * its separate occlusion rasterization (backward.cu:683).  dL_dout_occ [3,H,W]; dL_docc [P], overwritten.  For a main pass
 * (render_front = 0, sort_descending = 0) whose forward was soar_rast_forward_render_occ. */
int soar_rast_backward_occ(const SoarRastParams *prm,
                           const float *means3D, const int32_t *radii, const float *shs,
                           const float *colors_precomp, const float *scales, const float *rotations,
                           const float *cov3D_precomp,
                           const void *geom_buffer, const void *binning_buffer, const void *image_buffer,
                           int64_t num_rendered,
                           const float *dL_dout_color, const float *dL_dout_normal,
                           const float *dL_dout_depth, const float *dL_dout_opac, const float *dL_dout_occ,
                           const float *normal_scale_dev,   /* optional device scalar dL_dout_normal is multiplied by on load */
                           int32_t occ_planes,              /* 3: dL_dout_occ is [3,H,W]; 1: [1,H,W], the three channels' gradients already summed */
                           float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity, float *dL_dmeans3D,
                           float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drotations,
                           float *dL_dviewmat, float *dL_dprojmat, float *dL_dcampos, float *dL_docc,
                           void *workspace, size_t workspace_bytes,
                           void *stream);
/* Same, with the four image gradients multiplied by the device scalar *grad_scale_dev while they are loaded (the
 * upstream gradient of a scalar image loss whose gradient planes soar_frame_loss wrote): no scaling pass. */
int soar_rast_backward_scaled(const SoarRastParams *prm,
                              const float *means3D, const int32_t *radii, const float *shs,
                              const float *colors_precomp, const float *scales, const float *rotations,
                              const float *cov3D_precomp,
                              const void *geom_buffer, const void *binning_buffer, const void *image_buffer,
                              int64_t num_rendered,
                              const float *dL_dout_color, const float *dL_dout_normal,
                              const float *dL_dout_depth, const float *dL_dout_opac, const float *grad_scale_dev,
                              float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity, float *dL_dmeans3D,
                              float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drotations,
                              float *dL_dviewmat, float *dL_dprojmat, float *dL_dcampos,
                              void *workspace, size_t workspace_bytes,
                              void *stream);
/* soar_rast_backward / soar_rast_backward_occ for the training step plan: the same calls with the form of the backward blend named by
 * the caller.  region = 1: a wavefront per 4 x 4 pixel block -- exactly what the entries above launch; region = 2: a wavefront per
 * pair of blocks side by side (40 % fewer accumulation rows; faster from about a megapixel up, slower on small images, and inside
 * the strict gradient bar for loss-derived image gradients only: rast_render_bwd.hip). */
int soar_rast_backward_plan(const SoarRastParams *prm, int32_t region,
                            const float *means3D, const int32_t *radii, const float *shs,
                            const float *colors_precomp, const float *scales, const float *rotations,
                            const float *cov3D_precomp,
                            const void *geom_buffer, const void *binning_buffer, const void *image_buffer,
                            int64_t num_rendered,
                            const float *dL_dout_color, const float *dL_dout_normal,
                            const float *dL_dout_depth, const float *dL_dout_opac,
                            float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity, float *dL_dmeans3D,
                            float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drotations,
                            float *dL_dviewmat, float *dL_dprojmat, float *dL_dcampos,
                            void *workspace, size_t workspace_bytes,
                            void *stream);
int soar_rast_backward_occ_plan(const SoarRastParams *prm, int32_t region,
                                const float *means3D, const int32_t *radii, const float *shs,
                                const float *colors_precomp, const float *scales, const float *rotations,
                                const float *cov3D_precomp,
                                const void *geom_buffer, const void *binning_buffer, const void *image_buffer,
                                int64_t num_rendered,
                                const float *dL_dout_color, const float *dL_dout_normal,
                                const float *dL_dout_depth, const float *dL_dout_opac, const float *dL_dout_occ,
                                const float *normal_scale_dev, int32_t occ_planes,
                                float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity, float *dL_dmeans3D,
                                float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drotations,
                                float *dL_dviewmat, float *dL_dprojmat, float *dL_dcampos, float *dL_docc,
                                void *workspace, size_t workspace_bytes,
                                void *stream);
/* how many frames' backward blends this process has issued in each form since the library was loaded (host-side counters) */
int soar_rast_backward_region_counts(int64_t *single_blocks, int64_t *pairs);
/* bytes of `workspace` needed by soar_rast_backward (per-Gaussian accumulation rows) */
int soar_rast_backward_workspace_bytes(int32_t P, size_t *bytes);

/* ---- markVisible (DGR/rasterize_points.cu:189-205): the reference kernel body is commented out
 *      (DGR/cuda_rasterizer/rasterizer_impl.cu:52-62), so `present` [P] (bool/uint8) is all false. */
int soar_rast_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                           uint8_t *present, void *stream);

/* ---- debugging / parity: copy intermediates out of the opaque buffers into caller arrays (any may be NULL).
 *   means2D [P,2], depths [P], conic_opacity [P,4], normal [P,3], depth_plane [P,2] (the two per-pixel-depth
 *   coefficients folded from Jinv), rgb [P,3], cov3D [P,6], tiles_touched [P], point_offsets [P],
 *   keys_unsorted/keys_sorted [R] uint64, vals_unsorted/point_list [R] uint32, ranges [T,2] uint32,
 *   final_T [H*W], final_D [H*W], n_contrib [H*W] uint32. */
int soar_rast_export_state(const SoarRastParams *prm, const void *geom_buffer, const void *binning_buffer,
                           const void *image_buffer, int64_t num_rendered,
                           float *means2D, float *depths, float *conic_opacity, float *normal,
                           float *depth_plane, float *rgb, float *cov3D,
                           uint32_t *tiles_touched, uint32_t *point_offsets,
                           uint64_t *keys_unsorted, uint32_t *vals_unsorted,
                           uint64_t *keys_sorted, uint32_t *point_list, uint32_t *ranges,
                           float *final_T, float *final_D, uint32_t *n_contrib, void *stream);

/* ---- SMPL-X linear-blend skinning of canonical Gaussians ----
 * soar_lbs_knn_weights: SMPL_Guidance.query_weights_smpl (TS/utils/smpl.py:618-637).
 *   xyz [P,3] canonical points, verts [V,3] canonical SMPL-X vertices, vert_weights [V,J] skinning weights;
 *   K nearest vertices (the reference hard-codes 30), d = clamp(sqrt(d2), 1e-4, 1), ws = (1/d)/sum(1/d),
 *   weights_out [P,J] = sum_k ws_k * vert_weights[idx_k].  knn_idx_out [P,K] int32 optional (may be NULL).
 *   workspace: soar_lbs_knn_weights_bytes(P, V) bytes of 256-byte aligned device memory owned by the CALLER (vertex grid +
 *   query sort scratch), like every other scratch buffer of this ABI: the library keeps no device state of its own, so
 *   concurrent callers on different streams / threads and captured HIP graphs never share or outlive a hidden buffer. */
int soar_lbs_knn_weights_bytes(int32_t P, int32_t V, size_t *bytes);
int soar_lbs_knn_weights(const float *xyz, int32_t P, const float *verts, int32_t V,
                         const float *vert_weights, int32_t J, int32_t K,
                         float *weights_out, int32_t *knn_idx_out,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The same in two steps for a STATIC vertex set (SOAR's canonical SMPL-X vertices and lbs_weights never change during
 * training, TS/utils/smpl.py:508-511): build the vertex grid once, query it every optimizer step.
 *   grid_buffer: soar_lbs_knn_grid_bytes(V) bytes of 256-byte aligned device memory, owned by the caller.
 *   query_workspace: soar_lbs_knn_query_bytes(P) bytes, owned by the caller (one per concurrent query / per step plan;
 *   a plan that captures the query in a HIP graph keeps it alive as long as the graph).  Besides the sort scratch it holds the
 *   heaviest-first order of the query kernel's work items, rebuilt with every sort: a call that reuses a stored query order
 *   (soar_lbs_knn_query_ordered, resort = 0) should pass the workspace of the call that sorted (any other one is accepted: the
 *   items are then taken in place). */
int soar_lbs_knn_grid_bytes(int32_t V, size_t *bytes);
int soar_lbs_knn_query_bytes(int32_t P, size_t *bytes);
int soar_lbs_knn_build_grid(const float *verts, int32_t V, const float *vert_weights, int32_t J, void *grid_buffer,
                            void *stream);
int soar_lbs_knn_query(const void *grid_buffer, int32_t V, const float *vert_weights, int32_t J,
                       const float *xyz, int32_t P, int32_t K, float *weights_out, int32_t *knn_idx_out,
                       void *query_workspace, size_t query_workspace_bytes, void *stream);
/* Same with a caller-owned query order [P] (uint32): resort != 0 sorts the queries by grid cell and stores the order;
 * resort == 0 reuses the stored order (only the cell keys are recomputed from the current positions).  Canonical positions
 * move little between optimizer steps, so a training loop re-sorts every few steps; results never depend on the order. */
int soar_lbs_knn_query_ordered(const void *grid_buffer, int32_t V, const float *vert_weights, int32_t J,
                               const float *xyz, int32_t P, int32_t K, uint32_t *order, int32_t resort,
                               float *weights_out, int32_t *knn_idx_out,
                               void *query_workspace, size_t query_workspace_bytes, void *stream);

/* ---- neighbour sets that follow the queries (round 3).  The canonical vertices are constants (TS/utils/smpl.py:508-511) and a
 * query moves by an optimizer step between two calls of query_weights_smpl (:618-637): its K = 30 nearest vertices are almost always
 * the same.  soar_lbs_knn_query_state = soar_lbs_knn_query_ordered that also stores, per query, its neighbour set (state_buffer:
 * soar_lbs_knn_state_bytes(P), caller-owned, 256-byte aligned).  soar_lbs_knn_refresh then recomputes the blend weights of moved
 * queries: a query whose displacement since its set was found stays below half the gap between its K-th and (K+1)-th neighbour
 * distance keeps its set (certified: the full search would return the same one) and only recomputes the K distances, the weights
 * and the blend of the skinning rows; the state holds the 32 nearest vertices and a second gap behind the 32nd, so that a query
 * whose first gap is smaller than a step re-ranks its 32 instead of searching; a query that fails both certificates is searched
 * exactly, seeded by its old set, and gets a new set and new gaps.
 * Either way the weights are those of soar_lbs_knn_query_ordered at the same positions, bit for bit.  `order`: the
 * query order soar_lbs_knn_query_state stored -- the state is kept in that order.  searched_counter_dev (nullable): device uint32 that the number of queries that
 * needed the search is added to.  The state is tied to (grid, P): after densification start again with soar_lbs_knn_query_state.
 * Round 4: a refresh is two launches -- the certificates, then the blends of the certified queries with the seeded searches running
 * under them -- and the state also holds the refresh's 32 distances per query and the searches' work lists (about 306 bytes per
 * query; ask soar_lbs_knn_state_bytes).  The lists are left empty by every refresh: one refresh of a state at a time (one stream). */
int soar_lbs_knn_state_bytes(int32_t P, size_t *bytes);
int soar_lbs_knn_query_state(const void *grid_buffer, int32_t V, const float *vert_weights, int32_t J, const float *xyz, int32_t P,
                             uint32_t *order, int32_t resort, float *weights_out, void *state_buffer, void *query_workspace,
                             size_t query_workspace_bytes, void *stream);
int soar_lbs_knn_refresh(const void *grid_buffer, int32_t V, int32_t J, const float *xyz, int32_t P, const uint32_t *order,
                         void *state_buffer, float *weights_out, uint32_t *searched_counter_dev, void *stream);

/* soar_lbs_warp_forward: blend + apply, i.e. SMPL_Guidance.__call__ line TS/utils/smpl.py:613
 *   (pt_mats = einsum("bnj,bjxy->bnxy", w, cano2live)) fused with DiffGaussian.forward's warp
 *   (TS/renderer/diff_gaussian_rasterizer.py:103-114 / :138-149):
 *     p' = M3 p + t ; R' = M3 R(q) ; optionally p' <- p' T, R' <- T^T R' (axis_perm, row-major 3x3, may be NULL);
 *     q' = normalize(matrix_to_quaternion(R')).
 *   weights [P,J]; joint_mats [J,16] row-major 4x4 (cano2live = A_live @ inv(A_cano));
 *   alternatively weights == NULL and joint_mats = one ready-made row-major 4x4 per Gaussian [P,16] (the pt_mats
 *   tensor SMPL_Guidance.__call__ returns, TS/utils/smpl.py:613-615; J is ignored);
 *   offsets [P,3] optional additive offsets applied after the warp (cfg.offset, :107-108), may be NULL.
 *   xyz_out [P,3], rot_out [P,4]; pt_mats_out [P,16] optional (may be NULL). */
int soar_lbs_warp_forward(const float *xyz, const float *rot, const float *weights, const float *joint_mats,
                          const float *offsets, const float *axis_perm, int32_t P, int32_t J,
                          float *xyz_out, float *rot_out, float *pt_mats_out, void *stream);

/* soar_lbs_warp_backward: gradient of the above w.r.t. xyz and rot (weights and joint matrices are
 *   constants in the reference: TS/utils/smpl.py:611 detaches, :543-545 plain tensors). */
int soar_lbs_warp_backward(const float *xyz, const float *rot, const float *weights, const float *joint_mats,
                           const float *axis_perm, int32_t P, int32_t J,
                           const float *dL_dxyz_out, const float *dL_drot_out,
                           float *dL_dxyz, float *dL_drot, void *stream);

/* The head of the forward pass of the n frames of one optimizer step in ONE kernel (round 6; no reference counterpart: the reference
 * warps with torch ops, TS/renderer/diff_gaussian_rasterizer.py:103-114 / :138-149, and runs FORWARD::preprocess per frame,
 * forward.cu:205-385): per frame and Gaussian the warp through that frame's joint transforms, then the per-Gaussian forward stage of the
 * rasterizer on the posed values, in registers.  Writes what soar_lbs_warp_forward_batch writes (xyz_out [n][P][3], rot_out [n][P][4])
 * and, into every frame's geom_buffer / radii, what the preprocess stage of soar_rast_forward_geometry writes -- bit for bit.  Every
 * frame's soar_rast_forward_geometry then runs with SoarRastParams.debug bit 4 (its preprocess stage has been done: the depth buckets
 * follow).  Explicit colours [P,3] (M == 0), opacities [P], scales [P,3] shared by the frames; not prefiltered. */
typedef struct SoarFrameHead {
    const SoarRastParams *prm;
    void *geom_buffer;
    int32_t *radii;              /* [P] */
} SoarFrameHead;
int soar_frames_warp_preprocess(int32_t n, const SoarFrameHead *frames, const float *xyz, const float *rot, const float *weights,
                                const float *joint_mats, int32_t P, int32_t J, const float *colors, const float *opacities, const float *scales,
                                float *xyz_out, float *rot_out, void *stream);

/* The per-Gaussian stage of the backward ALONE (BACKWARD::preprocess, backward.cu:437-526 with :163-322 and :326-432), over the
 * accumulation rows that a soar_rast_backward* call with SoarRastParams.debug bit 3 left at the start of its workspace: together the two
 * calls are soar_rast_backward.  Outputs as soar_rast_backward's (all fully written; dL_dsh / dL_docc may be NULL). */
int soar_rast_backward_rows(const SoarRastParams *prm, const float *means3D, const int32_t *radii, const float *shs, const float *scales,
                            const float *rotations, const float *cov3D_precomp, const void *geom_buffer, const void *workspace,
                            float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity, float *dL_dmeans3D, float *dL_dcov3D, float *dL_dsh,
                            float *dL_dscales, float *dL_drotations, float *dL_dviewmat, float *dL_dprojmat, float *dL_dcampos, float *dL_docc,
                            void *stream);

/* The tail of the backward pass of the n frames of one optimizer step in ONE kernel (round 6; no reference counterpart: the reference
 * runs BACKWARD::preprocess per frame, backward.cu:437-526 + :163-322 + :326-432, and autograd carries dL_dmeans3D / dL_drotations
 * through the torch ops of the warp, TS/renderer/diff_gaussian_rasterizer.py:103-114).  Every frame's soar_rast_backward /
 * soar_rast_backward_occ ran with SoarRastParams.debug bit 3: its accumulation rows wait in `workspace`.  Per frame and Gaussian the
 * per-Gaussian backward of the rasterizer, then the warp's backward through that frame's joint transforms, in registers; the frames'
 * gradients are added in frame order.  Explicit colours (M == 0), scales + quaternions (no precomputed covariance), cfg_lrn_cam == 0.
 * Writes dL_dmeans2D of every frame ([P,3]: what the densifier's statistics read) and the sums over the frames dL_dxyz [P,3],
 * dL_drot [P,4] (canonical), dL_dscales [P,3], dL_dcolors [P,3] and -- when the frames ran soar_rast_backward_occ -- dL_docc [P].
 * Bit for bit what soar_rast_backward* (without bit 3) + soar_lbs_warp_backward_sum (+ soar_sum_frames) leave in those outputs. */
typedef struct SoarFrameTail {
    const SoarRastParams *prm;
    const float *means3D;        /* [P,3] posed (what the forward was given) */
    const float *rotations;      /* [P,4] posed */
    const int32_t *radii;
    const void *geom_buffer;
    const void *workspace;       /* the backward call's workspace: accumulation rows [P][16] at its start */
    float *dL_dmeans2D;          /* [P,3] */
} SoarFrameTail;
int soar_frames_geometry_warp_backward(int32_t n, const SoarFrameTail *frames, const float *xyz, const float *rot, const float *weights,
                                       const float *joint_mats, int32_t P, int32_t J, const float *scales, float *dL_dxyz, float *dL_drot,
                                       float *dL_dscales, float *dL_dcolors, float *dL_docc, void *stream);
/* ... which also finishes the frames' image losses: soar_frame_loss_partials / soar_frame_loss_pooled_partials left the per-workgroup
 * partial sums of frame f in its scratch and what to do with them in finish[f] (HOST array, n entries); one more workgroup per frame
 * adds them up -- in soar_frame_loss's order: the same bits in loss_out -- off the chain between the loss and the backward blend,
 * which reads the gradient planes, never the value.  finish == NULL: soar_frames_geometry_warp_backward. */
typedef struct SoarLossFinish {
    const float *sums4;          /* the loss call's scratch */
    float *loss_out;             /* [1] */
    int32_t blocks, n;           /* partial sums (4 floats each), pixels */
    float w_color, w_mask, w_normal, w_depth;
} SoarLossFinish;
int soar_frames_geometry_warp_backward_losses(int32_t n, const SoarFrameTail *frames, const float *xyz, const float *rot,
                                              const float *weights, const float *joint_mats, int32_t P, int32_t J, const float *scales,
                                              float *dL_dxyz, float *dL_drot, float *dL_dscales, float *dL_dcolors, float *dL_docc,
                                              const SoarLossFinish *finish, void *stream);

/* The warps of the n frames of one optimizer step, one launch each way (no reference counterpart: the reference warps frame by
 * frame).  The canonical model (xyz, rot) and the blend weights are shared; joint_mats [n][J][16]; xyz_out / dL_dxyz_out
 * [n][P][3], rot_out / dL_drot_out [n][P][4] (frame-major).  The backward form returns the SUM over the frames, added in frame
 * order: dL_dxyz [P][3], dL_drot [P][4]; on the way it can sum up to two more per-frame gradient blocks of the same points
 * (extra_src[e] = [n][P][extra_width[e]] -> extra_dst[e] = [P][extra_width[e]]; host arrays of device pointers). */
int soar_lbs_warp_forward_batch(const float *xyz, const float *rot, const float *weights, const float *joint_mats, int32_t n,
                                int32_t P, int32_t J, float *xyz_out, float *rot_out, void *stream);
int soar_lbs_warp_backward_sum(const float *xyz, const float *rot, const float *weights, const float *joint_mats, int32_t n,
                               int32_t P, int32_t J, const float *dL_dxyz_out, const float *dL_drot_out, float *dL_dxyz,
                               float *dL_drot, int32_t n_extra, const float *const *extra_src, float *const *extra_dst,
                               const int32_t *extra_width, void *stream);

/* ---- simple-knn distCUDA2 (call sites TS/geometry/surfel_base.py:499-503, gaussian_base.py:585-588):
 *   out[i] = mean of the 3 smallest squared distances from point i to the other points. */
int soar_dist2_knn3(const float *points, int32_t N, float *out, void *stream);

/* ---- per-frame image loss, value + pixel gradients in one pass (the dense
 *      four-output loss of section 8(d):  L = wc mean|color - tc| + wm mean|opac - tm| + wn mean(normal . tn) + wd mean(depth);
 *      same per-pixel structure as the reference's frame losses, TS/system/gaussian_surfel_mvdream.py:311-330,622-630).
 *   color/normal/target_color/target_normal [3,H,W], depth/opac/target_mask [1,H,W] (16-byte accesses when W*H is a multiple of 4 and the planes are aligned).
 *   loss_out [1], scratch [SOAR_FRAME_LOSS_SCRATCH_FLOATS] (per-workgroup partial sums of the four terms, added up in a fixed
 *   order: the loss value does not depend on the order in which workgroups finish), dL_d* = gradient of L w.r.t. the four images.
 *   image_buffer (optional, may be NULL): the rasterizer image buffer that belongs to these outputs.  When given, the gradient
 *   planes are only written at pixels with n_contrib > 0 -- the backward blend starts its walk at n_contrib
 *   (backward.cu:604,653), so the gradients of pixels nothing was blended into (85 % of a 1080p frame of one person) are
 *   never read; the loss value always covers every pixel.
 *   background (optional device [3], only with image_buffer) + normalize_depth (SoarRastParams.cfg_normalize_depth of that forward):
 *   the background colour the images were blended over.  When given, the four images are not READ at pixels with n_contrib == 0
 *   either: what the blend wrote there are its background constants (forward.cu:618-633), recomputed here bit for bit. */
#define SOAR_FRAME_LOSS_SCRATCH_FLOATS (4 * 2048)
int soar_frame_loss(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                    const float *opac, const float *target_color, const float *target_mask,
                    const float *target_normal, float w_color, float w_mask, float w_normal, float w_depth,
                    float *loss_out, float *scratch, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                    float *dL_dopac, const void *image_buffer, const float *background, int32_t normalize_depth, void *stream);

/* Same loss with the frame data resident in HBM: target_pool [n_sets][7][H*W] (colour 3, mask 1, normal 3 planes per
 * frame), the set is chosen on the DEVICE as *set_index_dev mod n_sets -- the launch stays valid when it is replayed from a
 * HIP graph for another frame (the host only rewrites the 4-byte index). */
int soar_frame_loss_pooled(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                           const float *opac, const float *target_pool, int32_t n_sets, const int32_t *set_index_dev,
                           float w_color, float w_mask, float w_normal, float w_depth, float *loss_out, float *scratch,
                           float *dL_dcolor, float *dL_dnormal, float *dL_ddepth, float *dL_dopac, const void *image_buffer,
                           const float *background, int32_t normalize_depth, void *stream);
/* The two calls above without their second launch: the gradient planes and the partial sums in `scratch` are written, loss_out is
 * NOT; *finish_out (host memory) receives what soar_frames_geometry_warp_backward_losses needs to write it later in the step. */
int soar_frame_loss_partials(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                             const float *opac, const float *target_color, const float *target_mask,
                             const float *target_normal, float w_color, float w_mask, float w_normal, float w_depth,
                             float *loss_out, float *scratch, float *dL_dcolor, float *dL_dnormal, float *dL_ddepth,
                             float *dL_dopac, const void *image_buffer, const float *background, int32_t normalize_depth,
                             SoarLossFinish *finish_out, void *stream);
int soar_frame_loss_pooled_partials(int32_t W, int32_t H, const float *color, const float *normal, const float *depth,
                                    const float *opac, const float *target_pool, int32_t n_sets, const int32_t *set_index_dev,
                                    float w_color, float w_mask, float w_normal, float w_depth, float *loss_out, float *scratch,
                                    float *dL_dcolor, float *dL_dnormal, float *dL_ddepth, float *dL_dopac, const void *image_buffer,
                                    const float *background, int32_t normalize_depth, SoarLossFinish *finish_out, void *stream);

/* ---- the frame loss inside the backward blend's launch (the batched eager step plan).  soar_rast_backward_plan with a loss record in
 * place of the four gradient planes: soar_frame_loss[_pooled]_partials + soar_rast_backward_plan as ONE launch, without the
 * gradient planes' round trip through memory.
 *   - the blend computes dL/dcolor, dL/dnormal, dL/ddepth, dL/dopac of a pixel in its prologue, from the forward's color / opac
 *     planes and the frame's targets, with soar_frame_loss's expressions (the same bits; only pixels with contributors matter);
 *   - the loss's value pass runs as extra workgroups ("riders") of the same launch: bandwidth work next to issue-bound work.  They
 *     leave one partial sum per WAVEFRONT of soar_frame_loss's grid in wave_sums; *finish_out (host memory) describes them for
 *     soar_frames_geometry_warp_backward_wave_losses, which adds the four wavefronts of a workgroup first and then goes on in
 *     soar_frame_loss's order: loss_out receives soar_frame_loss's bits there.  loss_out is NOT written by this call.
 * The image buffer, background and normalize_depth of the loss are those of the call (image_buffer, prm->bg_dev,
 * prm->cfg_normalize_depth).  target_*: explicit planes (set_index_dev = NULL), or all three = a resident pool [n_sets][7][H*W] and
 * set_index_dev a device integer, as in soar_frame_loss_pooled.  Batch-safe.  Needs P > 0 and num_rendered > 0 (the binning
 * capacity): with nothing to launch the riders would have no launch to ride in.  Everything else is soar_rast_backward_plan. */
#define SOAR_BACKWARD_LOSS_SCRATCH_FLOATS (4 * SOAR_FRAME_LOSS_SCRATCH_FLOATS)
typedef struct SoarBackwardLoss {
    const float *color, *normal, *depth, *opac;                     /* the forward's outputs */
    const float *target_color, *target_mask, *target_normal;
    const int32_t *set_index_dev;
    int32_t n_sets;
    float w_color, w_mask, w_normal, w_depth;
    float *loss_out;                                                /* [1]: handed on in *finish_out */
    float *wave_sums;                                               /* [SOAR_BACKWARD_LOSS_SCRATCH_FLOATS] */
} SoarBackwardLoss;
int soar_rast_backward_plan_loss(const SoarRastParams *prm, int32_t region,
                                 const float *means3D, const int32_t *radii, const float *shs,
                                 const float *colors_precomp, const float *scales, const float *rotations,
                                 const float *cov3D_precomp,
                                 const void *geom_buffer, const void *binning_buffer, const void *image_buffer,
                                 int64_t num_rendered, const SoarBackwardLoss *loss,
                                 float *dL_dmeans2D, float *dL_dcolors, float *dL_dopacity, float *dL_dmeans3D,
                                 float *dL_dcov3D, float *dL_dsh, float *dL_dscales, float *dL_drotations,
                                 float *dL_dviewmat, float *dL_dprojmat, float *dL_dcampos,
                                 void *workspace, size_t workspace_bytes, SoarLossFinish *finish_out,
                                 void *stream);
/* soar_frames_geometry_warp_backward_losses for finish[] records of soar_rast_backward_plan_loss (per-wavefront partials) */
int soar_frames_geometry_warp_backward_wave_losses(int32_t n, const SoarFrameTail *frames, const float *xyz, const float *rot,
                                                   const float *weights, const float *joint_mats, int32_t P, int32_t J, const float *scales,
                                                   float *dL_dxyz, float *dL_drot, float *dL_dscales, float *dL_dcolors, float *dL_docc,
                                                   const SoarLossFinish *finish, void *stream);

/* ---- the same terms in ONE pass over the images (round 4, ABI 6): masked L1 of the colours over `sel`, L1 of the mask image over
 * every pixel, cosine loss of the normals over `sel_normal`, and -- when `occ` is given -- masked L1 of the occlusion image against 1
 * over `sel_occ` (loss_occ, TS/system/gaussian_surfel_mvdream.py:412-417).  mode bit 0: the values, stats [6] = {loss, count} of L1,
 * mask L1, cosine (and stats_occ [2]); mode bit 1: the gradient planes, scaled by the device scalars up_* (NULL: 1) and by the
 * selected counts, which come from `stats` (the two-pass form: a values call first) or from `counts` [4] given by the caller (the
 * masks are constants of the target: mode 3 = value and gradient in one pass).  g_render optionally takes the SSIM term's gradient
 * on the way (+ up_ssim * g_ssim).  Same per-pixel expressions and the same order of additions as soar_masked_l1 / soar_cos_loss:
 * the same values bit for bit.  H * W a multiple of 4, planes 16-byte aligned (every image of the path).
 * scratch: soar_avatar_loss_scratch_floats() floats. */
typedef struct SoarAvatarLossArgs {
    int32_t H, W;
    float cos_limit, cos_weight;                 /* cos(thrsh), weight of cos_loss */
    const float *render, *gt_rgb;                /* [3,H,W] */
    const float *mask_img, *gt_mask;             /* [1,H,W] */
    const float *normal, *gt_normal;             /* [3,H,W] */
    const float *occ;                            /* [3,H,W] or NULL */
    const uint8_t *sel, *sel_normal, *sel_occ;   /* [H,W] one byte per pixel; sel_occ NULL iff occ is */
    float *stats, *stats_occ;                    /* device: [6], [2] */
    float *scratch;
    const float *counts;                         /* device [4] or NULL */
    const float *up_l1, *up_l1m, *up_cos, *up_occ, *up_ssim;
    const float *g_ssim;                         /* [3,H,W] or NULL */
    float *g_render, *g_mask, *g_normal, *g_occ; /* [3,H,W], [1,H,W], [3,H,W], [3,H,W] */
    /* normal_raw != 0: `normal` still is the plugin's normal' = (n (1,-1,-1) + 1) / 2, but g_normal leaves as the gradient of the
     * rasterizer's n (x 0.5, signs, zero where mask_img -- the opacity image -- is <= 1e-5: what soar_view_finish_backward makes of
     * dL/dnormal' alone).  cos_scale_out (mode 3 with counts only): the cosine term's gradient leaves without its factor
     * upstream / count, which is written here when the pass ends -- for a consumer that multiplies on load
     * (soar_rast_backward_occ's normal_scale_dev): value and gradient of every term in ONE pass over the images. */
    int32_t normal_raw;
    int32_t occ_grad_summed;                     /* != 0: g_occ is ONE plane [1,H,W], the sum (g_0 + g_1) + g_2 of the three channels' gradients
                                                  * -- all the occlusion chain's backward reads of them (soar_rast_backward_occ, occ_planes = 1) */
    float *cos_scale_out;
    /* (ABI 7) background != NULL -- [3] floats in device memory -- is a promise of the caller's: the images are the rasterizer's blend
     * over this background colour followed by the plugin's post-ops, and the gradients of pixels nothing contributed to (mask_img <=
     * 1e-5) are never read (the backward blend's walk of a pixel starts at its contributor count).  Groups of four such pixels -- 85 %
     * of a frame of one person -- are answered from the blend's constants (render = occ = (1 - 1e-6) background, normal' = 0.5): their
     * images and g_ssim are not read, their gradient planes not written.  The values are the same bit for bit. */
    const float *background;
} SoarAvatarLossArgs;
int soar_avatar_loss_scratch_floats(size_t *count);
int soar_avatar_pixel_losses(const SoarAvatarLossArgs *args, int32_t mode, void *stream);

/* ---- SSIM (TS/utils/loss_utils.py:36-76: 11x11 Gaussian window, sigma 1.5, zero padding):
 *      mean SSIM of img1, img2 [C,H,W] and, when dssim_dimg1 != NULL, its gradient w.r.t. img1 -- one kernel per
 *      direction instead of five grouped convolutions and ~15 element-wise kernels each way.
 *   scratch: soar_ssim_scratch_floats(C, H, W) floats. */
int soar_ssim_scratch_floats(int32_t C, int32_t H, int32_t W, size_t *count);
int soar_ssim(int32_t C, int32_t H, int32_t W, const float *img1, const float *img2, float *ssim_out, float *scratch,
              float *dssim_dimg1, void *stream);
/* (ABI 7) the same with `rendered` [H,W]: the opacity image of the rasterization that produced img1.  The gradient is only WRITTEN for
 * the 32x32 tiles that hold a pixel with rendered > 1e-5 -- the gradient of a pixel nothing contributed to is never read by the
 * backward blend -- and the forward only leaves its derivative maps where such a tile can want them; the mean is everybody's. */
int soar_ssim_rendered(int32_t C, int32_t H, int32_t W, const float *img1, const float *img2, float *ssim_out, float *scratch,
                       float *dssim_dimg1, const float *rendered, void *stream);

/* ---- densification / pruning state machine (TS/geometry/surfel_base.py:850-1136,1198-1230).
 * soar_densify_stats: update_states' per-view body + add_densification_stats (:1102-1128,1208-1216) in one pass.
 *   radii [P] int32 (filter = radii > 0), grad2d [P,grad_stride] (viewspace gradient, first two columns read),
 *   scaling_grad [P,3], rotation [P,4], opacity [P] (raw), accum [5,P] = {xyz, scale, rot, opac gradient accumulators, denom},
 *   max_radii2D [P]; all updated in place.
 * soar_densify_plan: adaptive_prune (:1067-1087, when do_prune) + the clone / split masks of adaptive_densify
 *   (:982-1000,1032-1046,1089-1100, when do_densify) over the points that survive the prune, and the destination row of
 *   every point.  Thresholds are passed as the reference compares them: prune_scale_max = 0.5 extent, prune_area_min =
 *   1e-8 extent^2, dense_scale = percent_dense * extent.  plan: soar_densify_plan_bytes(P) bytes, 256-byte aligned, opaque.
 *   counts_host [3] = {kept, clones, split parents} (blocking read-back) or NULL.  New size = kept + clones + N * split.
 * soar_densify_flags: copies the per-point flag byte (1 pruned, 2 clone, 4 split) to flags_out [P].
 * soar_densify_apply: moves every listed tensor (rows of `width` floats) into its new buffer in one launch, layout
 *   [kept and not split | clones | split children rep 0 | rep 1 ...] exactly as the reference's cat / prune sequence leaves it.
 *   mode 0: copy rows; 1: Adam moments (new rows zero); 2: xyz (children = R(q) (noise * exp(scaling)) + xyz, :1001-1004);
 *   3: scaling (children = log(exp(s) / (0.8 N)), last column -1e10 when surface, :1005-1009).
 *   scaling / rotation: the OLD [P,3] / [P,4] tensors; noise [N * split, 3] standard normals (row = child index; may be NULL
 *   only when the plan holds no split parents). */
typedef struct SoarDensifyRow {
    const float *src;
    float *dst;
    int32_t width;
    int32_t mode;
} SoarDensifyRow;
int soar_densify_stats(int32_t P, const int32_t *radii, const float *grad2d, int32_t grad_stride, const float *scaling_grad,
                       const float *rotation, const float *opacity, float *accum, float *max_radii2D, void *stream);
int soar_densify_plan_bytes(int32_t P, size_t *bytes);
int soar_densify_plan(int32_t P, const float *accum, const float *scaling, const float *opacity, int32_t do_prune,
                      int32_t do_densify, float min_opacity, float prune_scale_max, float prune_area_min, float max_grad,
                      float dense_scale, void *plan, int64_t *counts_host, void *stream);
int soar_densify_flags(int32_t P, const void *plan, uint8_t *flags_out, void *stream);
int soar_densify_apply(int32_t P, int32_t N, const void *plan, int32_t n_rows, const SoarDensifyRow *rows, const float *scaling,
                       const float *rotation, const float *noise, int32_t surface, void *stream);

/* ---- SMPL-X joint transforms of B frames in one launch.
 * Replaces, for the per-frame path, SMPLX.forward -> lbs() -> batch_rodrigues / batch_rigid_transform
 * (TS/utils/smplx/lbs.py:147-246,293-396, body_models.py:1383) and the A_live @ inv(A_cano) product of SMPL_Guidance
 * (TS/utils/smpl.py:601-609).  J <= 64 joints; betas [betas_batch,NB] with betas_batch 1 or B (shape and expression
 * coefficients concatenated); J_template [J,3] = J_regressor v_template; J_dirs [J,3,NB] = J_regressor shapedirs;
 * parents [J] (root < 0); full_pose [B,J*3] axis-angle; transl [B,3] or NULL; right_mats [J,4,4] or NULL
 * (out_j = A_j right_mats_j, e.g. inv(A_cano)); out [B,J,4,4].  The parameters are not optimised in the reference: no backward. */
int soar_smplx_joint_mats(int32_t B, int32_t J, int32_t NB, const float *betas, int32_t betas_batch, const float *J_template,
                          const float *J_dirs, const int32_t *parents, const float *full_pose, const float *transl,
                          const float *right_mats, float *out, void *stream);

/* ---- masked image losses of the avatar stage, value in one pass, gradient in one pass:
 *   masked L1  = l1_loss_w(img[mask], gt[mask])  (TS/system/gaussian_surfel_mvdream.py:311-314, TS/utils/loss_utils.py:9-10)
 *   cosine loss = cos_loss(output, gt, mask, thrsh, weight)  (TS/system/gaussian_surfel_mvdream.py:622-630; cos_thrsh = cos(thrsh))
 *   img / gt / output [C,H,W]; mask [H,W] one byte per pixel or NULL; stats2 [2] = {loss, selected count} (device);
 *   scratch: soar_image_loss_scratch_floats() floats; upstream_dev: device scalar dL/dloss or NULL (= 1). */
int soar_image_loss_scratch_floats(size_t *count);
int soar_masked_l1(int32_t C, int32_t H, int32_t W, const float *img, const float *gt, const uint8_t *mask, float *stats2,
                   float *scratch, void *stream);
int soar_masked_l1_backward(int32_t C, int32_t H, int32_t W, const float *img, const float *gt, const uint8_t *mask,
                            const float *stats2, const float *upstream_dev, float *dL_dimg, void *stream);
int soar_cos_loss(int32_t C, int32_t H, int32_t W, const float *output, const float *gt, const uint8_t *mask, float cos_thrsh,
                  float weight, float *stats2, float *scratch, void *stream);
int soar_cos_loss_backward(int32_t C, int32_t H, int32_t W, const float *output, const float *gt, const uint8_t *mask,
                           float cos_thrsh, float weight, const float *stats2, const float *upstream_dev, float *dL_doutput,
                           void *stream);

/* ---- renderer post-ops: depth2normal and normal2curv
 *      (TS/renderer/diff_gaussian_rasterizer.py:359-448) as fused 5-point-stencil kernels with analytic backward.
 *   depth [1,H,W], normal [3,H,W], curv [1,H,W]; mask [1,H,W] one byte per pixel (torch.bool);
 *   prcp_* = principal point (cx/W, cy/H); focal_k00 = focal(FoVy, H) is applied to x and focal_k11 = focal(FoVx, W) to y,
 *   as the reference's K does (:386-389).  The backward calls zero-fill and fully define their outputs. */
int soar_depth2normal(int32_t W, int32_t H, const float *depth, const uint8_t *mask, float prcp_x, float prcp_y,
                      float focal_k00, float focal_k11, float *normal_out, void *stream);
int soar_depth2normal_backward(int32_t W, int32_t H, const float *depth, const uint8_t *mask, float prcp_x, float prcp_y,
                               float focal_k00, float focal_k11, const float *dL_dnormal, float *dL_ddepth, void *stream);
int soar_normal2curv(int32_t W, int32_t H, const float *normal, const uint8_t *mask, float *curv_out, void *stream);
int soar_normal2curv_backward(int32_t W, int32_t H, const float *normal, const uint8_t *mask, const float *dL_dcurv,
                              float *dL_dnormal, void *stream);

/* soar_view_finish[_backward]: everything DiffGaussian.forward does to a view behind the rasterizer
 *   (TS/renderer/diff_gaussian_rasterizer.py:292-303) in one launch each way -- mask = opac > 1e-5;
 *   normal_out = (normal * (1,-1,-1) + 1) / 2 with gradient inside the mask only (the torch.where of :294);
 *   curv = normal2curv(normal * (1,-1,-1), mask); pred_normal = (depth2normal(depth, mask) * (1,-1,-1) + 1) / 2 -- the same
 *   values as the separate entry points above give.  prcppoint_dev: the camera's principal point, 2 floats in DEVICE memory
 *   (no host read of a device tensor per frame).  Backward: each incoming gradient may be NULL; dL_ddepth_direct is the
 *   gradient that reaches the depth image itself; the result is ONE block [4][H][W] = dL/dnormal [3] then dL/ddepth [1]. */
int soar_view_finish(int32_t W, int32_t H, const float *normal, const float *depth, const float *opac,
                     const float *prcppoint_dev, float focal_k00, float focal_k11, float *normal_out, float *curv_out,
                     float *pred_normal_out, void *stream);
int soar_view_finish_backward(int32_t W, int32_t H, const float *normal, const float *depth, const float *opac,
                              const float *prcppoint_dev, float focal_k00, float focal_k11, const float *dL_dnormal_out,
                              const float *dL_dcurv, const float *dL_dpred_normal, const float *dL_ddepth_direct,
                              float *dL_dnormal_and_depth, void *stream);

/* ---- the views of one pose behind ONE call each way (round 4, ABI 6) ----
 * DiffGaussian.forward (TS/renderer/diff_gaussian_rasterizer.py:52-318) per view: LBS warp (:77-149), scales.repeat(1, 3) with the
 * third column overwritten and opacities = 1 (:232-234), main rasterization (:173-191, :236-279), occlusion rasterization
 * (:193-211, :280-291), image post-ops (:292-303); gt_forward / batch_forward (TS/renderer/gaussian_batch_renderer.py:243-398,
 * :10-241) call it for several views of one pose.  soar_views_forward issues the launches of all of that for up to 8 views of ONE
 * pose (warp once; views of one size and capacity share their launches, one per stage); soar_views_backward takes the gradients of
 * the views' images back to the canonical model (the views' contributions summed in view order).  Same kernels as the per-stage
 * entry points above, same results bit for bit.  Front views (main pass front to back, occlusion image fused into its blend) and back
 * views (`back`: main pass back to front, occlusion image a pass of its own) alike.
 * Nothing is read back: the binning part of a view's buffer holds `capacity` instances, and the two status words {instances found,
 * 0 or the number needed} are copied to status_pinned right behind the binning chain (0xFFFFFFFF until they land); a view that did
 * not fit renders as background, and the caller -- who polls the words before it runs the backward -- renders it again. */
typedef struct SoarPoseArgs {
    int32_t P, J;
    int32_t scale_width;         /* columns of scale_src: 1 */
    int32_t warp;                /* forward: != 0 warp into `posed` (0: `posed` already holds this pose) */
    const float *xyz, *rot;      /* canonical surfels [P,3], [P,4] */
    const float *weights;        /* blend weights [P,J] */
    const float *joint_mats;     /* cano2live [J,16] */
    const float *offsets;        /* [P,3] or NULL (cfg.offset) */
    const float *axis_perm;      /* row-major 3x3 or NULL */
    const float *colors;         /* colors_precomp [P,3] */
    const float *scale_src;      /* get_scaling [P,scale_width] */
    const float *occ;            /* get_occ [P] or NULL: no occlusion image */
    float *occ3;                 /* caller-owned [P,3] (written when warp != 0) or NULL: occ.repeat(1, 3), needed by back views */
    float *posed;                /* caller-owned [11][P] floats: xyz' [P,3] | rot' [P,4] | scales3 [P,3] | ones [P]; kept for the backward */
    /* backward only */
    float *grad_scratch;         /* soar_views_grad_scratch_floats(P, n_views) floats */
    float *dL_dxyz, *dL_drot, *dL_dcolors, *dL_dscale;    /* [P,3] [P,4] [P,3] [P,scale_width]: written */
    float *dL_docc;              /* [P] or NULL: the occlusion values are not trained */
} SoarPoseArgs;
typedef struct SoarViewArgs {
    SoarRastParams rast;         /* P of the pose, M = 0, render_front = 0; sort_descending = back */
    float focal_k00, focal_k11;  /* fov2focal(FoVy, H), fov2focal(FoVx, W): depth2normal's intrinsics */
    int32_t back;                /* != 0: the plugin's render_front = False -- main pass sorted back to front (:173-191), the occlusion image a
                                  * front-to-back rasterization of its own (:193-211) */
    int32_t pad_;
    int64_t capacity;            /* (tile, Gaussian) instances the binning part of `buffer` holds */
    void *buffer;                /* soar_view_buffer_bytes(P, W, H, capacity) bytes, 256-byte aligned; kept for the backward */
    size_t buffer_bytes;
    float *out;                  /* [18][H][W]: render 0-2 | normal 3-5 | depth 6 | pred_normal 7-9 | mask 10 | occ 11-13 | curv 14 |
                                  * the rasterizer's own normal image 15-17 (read by the backward) */
    int32_t *radii;              /* [P] */
    uint32_t *status_pinned;     /* 4 words of page-locked host memory, or NULL: {instances found, 0 or the number needed} of the main pass,
                                  * then of a back view's occlusion pass */
    /* backward only: gradients of the images (each [c][H][W], NULL: not used by the loss) and this view's dL_dmeans2D [P,3] */
    const float *g_render, *g_normal, *g_depth, *g_pred_normal, *g_mask, *g_occ, *g_curv;
    float *dL_dmeans2D;
} SoarViewArgs;
int soar_view_buffer_bytes(int32_t P, int32_t W, int32_t H, int64_t capacity, int32_t back, size_t *bytes);
int soar_views_grad_scratch_floats(int32_t P, int32_t n_views, size_t *floats);
int soar_views_forward(const SoarPoseArgs *pose, int32_t n_views, const SoarViewArgs *views, void *stream);
int soar_views_backward(const SoarPoseArgs *pose, int32_t n_views, const SoarViewArgs *views, void *stream);
/* ---- the views of a whole optimizer step behind ONE call each way (round 5, ABI 7) ----
 * One step of the reference's training loop renders the 4 SDS views of the canonical (zeroed-root) pose and the 3 views of the video
 * frame's pose (TS/system/gaussian_surfel_mvdream.py:79-92 -> TS/renderer/gaussian_batch_renderer.py:243-398 and :10-241): 2 poses, 7
 * views.  soar_step_views_forward / _backward take n_poses poses with views_per_pose[p] views each (`views`: pose after pose, at most
 * 8 in all): every pose is warped once each way; front views of one size and capacity -- of ANY pose -- share their launches, one per
 * stage; the groups (another size, a back view) are issued on streams of the library's own beside each other, forked from `stream`
 * behind the warps and joined into it before the call returns.  Every pose carries its own
 * gradient outputs: the caller adds the poses' contributions to a shared model.  soar_views_forward / _backward are the n_poses = 1 forms. */
int soar_step_views_forward(int32_t n_poses, const SoarPoseArgs *poses, const int32_t *views_per_pose, const SoarViewArgs *views, void *stream);
int soar_step_views_backward(int32_t n_poses, const SoarPoseArgs *poses, const int32_t *views_per_pose, const SoarViewArgs *views, void *stream);
/* The cameras of a step in one launch: get_cam_info_gaussian_cxcy (TS/renderer/gaussian_batch_renderer.py:401-471) for n <= 8
 * camera-to-world matrices [n][16] (row-major; in device memory, or on the host: then they travel in the kernel's arguments -- no
 * copy, no synchronisation either way).  out_dev [n][48]: world_view_transform 16 | full_proj_transform 16 | camera_center 3 | 13 unused (every block 16-byte aligned), the
 * transposed (row-vector) convention of the reference's Camera. */
typedef struct SoarCameraSpec {
    double fovx, fovy, znear, zfar;
    double cx, cy, img_w, img_h;  /* principal point and image size: used when has_cxcy != 0 (:425-432) */
    int32_t has_cxcy, pad_;
} SoarCameraSpec;
int soar_cameras_from_c2w(int32_t n, const float *c2w_dev, const float *c2w_host, const SoarCameraSpec *specs, float *out_dev, void *stream);
/* soar_rast_forward_render_occ with the status words of soar_rast_binning_status_async copied out right behind the binning chain,
 * in front of the blend (status_pinned may be NULL). */
int soar_rast_forward_render_status(const SoarRastParams *prm, const int32_t *radii, void *geom_buffer, void *binning_buffer,
                                    void *image_buffer, int64_t num_rendered, float *out_color, float *out_normal, float *out_depth,
                                    float *out_opac, const float *occ_values, float *out_occ, uint32_t *status_pinned, void *stream);
/* soar_lbs_warp_backward_sum for n VIEWS of one pose: one set of joint transforms [J,16], optional axis permutation. */
int soar_lbs_warp_backward_views(const float *xyz, const float *rot, const float *weights, const float *joint_mats, const float *axis_perm,
                                 int32_t n, int32_t P, int32_t J, const float *dL_dxyz_out, const float *dL_drot_out, float *dL_dxyz,
                                 float *dL_drot, int32_t n_extra, const float *const *extra_src, float *const *extra_dst,
                                 const int32_t *extra_width, void *stream);

/* ---- per-stage timing (no reference counterpart; used by bench.py for the roofline figure) ----
 * When enabled, every kernel stage is bracketed by two hipEvents recorded on the launch stream.
 * soar_prof_read synchronises the pending events and returns the accumulated device time and launch count of
 * one stage (ids/names via soar_prof_stage_count / soar_prof_stage_name). */
int soar_prof_enable(int on);
int soar_prof_reset(void);
int soar_prof_stage_count(void);
const char *soar_prof_stage_name(int stage);
int soar_prof_read(int stage, double *total_ms, int64_t *launches);
/* ---- step-level helpers of the frame data-parallel step (new capability, no counterpart in the reference: SURVEY.md 8e) ----
 * soar_sum_frames: out[j] = sum_f in[f * count + j], f < n_frames (the per-frame gradient blocks of one per-Gaussian leaf summed
 *   into that leaf's slice of the flat gradient buffer that is all-reduced over the ranks).
 * soar_gather_step_inputs: for the n_frames frames of an optimizer step, copy row (frame_ids[f] mod num_frames_seq) of a
 *   per-frame table [num_frames_seq, floats_per_frame] (the joint transforms cano2live [55*16]) into mats_out [n_frames, ...]
 *   and write the frame's target-set index ((id mod n_sets), optional) -- frame_ids is a DEVICE array: a captured HIP graph
 *   stays valid for any frames, the host refreshes n_frames integers per step. */
int soar_sum_frames(int32_t n_frames, int64_t count, const float *in_dev, float *out_dev, void *stream);
int soar_gather_step_inputs(int32_t n_frames, int32_t num_frames_seq, int32_t floats_per_frame, int32_t n_sets,
                            const int32_t *frame_ids_dev, const float *table_dev, float *mats_out_dev,
                            int32_t *set_index_out_dev, void *stream);
/* ... with the (at most 8) frame ids read from HOST memory at the call and passed in the kernel's arguments: no device copy of
 * them in front of a step (launches issued directly; a captured graph needs the device form above). */
int soar_gather_step_inputs_ids(int32_t n_frames, int32_t num_frames_seq, int32_t floats_per_frame, int32_t n_sets,
                                const int32_t *frame_ids_host, const float *table_dev, float *mats_out_dev,
                                int32_t *set_index_out_dev, void *stream);

/* ---- the optimizer step (round 3).  torch.optim.Adam(eps=1e-15) over the parameter groups of the Gaussian model
 * (TS/geometry/surfel_base.py:596-681 training_setup, TS/system/gaussian_surfel_mvdream.py:471-472 optimizer.step()) as ONE launch
 * over a table of up to 8 rows, a row = one leaf {parameter, gradient, first moment, second moment, number of floats, learning
 * rate}.  No weight decay, no amsgrad.  state_dev: 16 bytes of zero-initialised device memory owned by the caller = {int32 step,
 * float 1 - beta1^step, float sqrt(1 - beta2^step), pad}; every call advances the step on the device (graph-capturable).
 * beta1 / beta2 / eps are doubles (ABI 6), as torch keeps them: 1 - beta is formed in double and rounded once (float(1 - 0.9) = 0.1,
 * whereas 1.f - 0.9f = 0.100000024).  Rows of a step that was never started (soar_adam_step_rows with advance = 0 on a zeroed state)
 * are left untouched. */
typedef struct SoarAdamRow {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t count;
    float lr;
    int32_t pad_;
} SoarAdamRow;
int soar_adam_step(int32_t n_rows, const SoarAdamRow *rows_host, double beta1, double beta2, double eps, void *state_dev, void *stream);
/* The same update with the step number (1, 2, ...) kept by the caller, as torch.optim.Adam keeps it: the bias corrections are worked
 * out on the host in double precision, there is no device counter and no launch to advance it.  Several calls with the same `step`
 * update further rows of that step.  Not inside a captured graph (a replay would repeat the step number).
 * 1 <= step <= INT32_MAX; a larger step is refused with an error (it is not truncated), here and in soar_adam_step_at_gather. */
int soar_adam_step_at(int32_t n_rows, const SoarAdamRow *rows, double beta1, double beta2, double eps, int64_t step, void *stream);
/* soar_adam_step_at and soar_gather_step_inputs_ids (same arguments, same results) in ONE launch: the gather depends on nothing the
 * update writes, its n_frames workgroups ride behind the update's.  The first launch of a training step's prologue. */
int soar_adam_step_at_gather(int32_t n_rows, const SoarAdamRow *rows, double beta1, double beta2, double eps, int64_t step,
                             int32_t n_frames, int32_t num_frames_seq, int32_t floats_per_frame, int32_t n_sets,
                             const int32_t *frame_ids_host, const float *table_dev, float *mats_out_dev, int32_t *set_index_out_dev,
                             void *stream);
/* The same step in parts: `advance` != 0 moves the step counter (and the bias corrections) on before the rows are updated, 0 updates
 * further rows of the SAME step -- a caller whose gradients arrive in buckets updates the leaves of a bucket as soon as it is there
 * (soar_amd/step_plan.py: the positions behind the first bucket, in front of the KNN refresh; the rest behind the second). */
int soar_adam_step_rows(int32_t n_rows, const SoarAdamRow *rows, double beta1, double beta2, double eps, void *state_dev, int32_t advance,
                        void *stream);
/* soar_adam_step_rows over a table of up to 40 rows (a whole geometry model -- the leaves, the attribute field's two hash tables and
 * the weights of its heads -- in one launch: soar_amd/geometry.py); same state, same arithmetic per element. */
int soar_adam_step_rows_wide(int32_t n_rows, const SoarAdamRow *rows, double beta1, double beta2, double eps, void *state_dev,
                             int32_t advance, void *stream);

/* soar_prof_timestamp: one-thread kernel that appends {tag, device wall clock (100 MHz ticks)} to a ring in device memory when
 * `stream` gets there: ring[0] counts the stamps, stamp n lies at ring[1 + 2 (n mod capacity)].  Timelines of launch chains
 * without host synchronisation; capturable in a HIP graph (every replay appends). */
int soar_prof_timestamp(unsigned long long *ring_dev, int64_t capacity, int64_t tag, void *stream);

/* ---- device self-test of the 64-lane scan of affine maps of the backward blend's entry-lane form (rast_render_bwd.hip):
 * m64_dev / b64_dev [64] = the map P -> m P + b of every lane; out192_dev [192]: [0..63] m and [64..127] b of the composition of
 * the maps of the lanes 0..i (lane 0's applied first), [128..191] b of lane i - 1 (lane 0: -7). */
int soar_selftest_affine_scan(const float *m64_dev, const float *b64_dev, float *out192_dev, void *stream);

/* ---- device self-test of the blend kernels' exp: out_dev[i] = the kernels' exp(x[i]), expf_dev[i] = the device math
 * library's expf(x[i]) (what the reference's `exp(power)` becomes when built for this GPU); equal bit for bit on [-87, 0]. */
int soar_selftest_exp(const float *x_dev, int32_t n, float *out_dev, float *expf_dev, void *stream);

/* ---- the shared implicit-GEMM convolution and the weight packer by themselves (csrc/conv_gemm.h): what the VAE
 * encoder, the normal networks and LPIPS reach only through whole networks, for tests/test_conv_gemm_*.py.
 * SoarConvGemmTaps / SoarConvGemmArgs mirror ConvTaps / ConvGemm of csrc/conv_gemm.h field by field (the launcher's tiles_* left out).
 * One tap table: output (gy os + py, gx os + px) of grid row (n, gy, gx) sums, tap by tap, input (gy stride + dy, gx stride + dx)
 * times w[co][tap][ci]: row co of B at w + image wbat + co ldw, k = tap Cin + ci.  y = alpha (A B^T) + bias + res:
 *   x      image n's pixel (iy, ix) at x + (n xim + iy Win + ix) ldx, Cin floats (Cin a multiple of 8)
 *   wbat   B's offset per image (per_image only)
 *   bias   [Cout] or NULL; res: indexed as y, or NULL
 *   y      image n's output pixel (oy, ox) at y + (n yim + oy Wout + ox) ldy, Cout floats
 *   N, Hg, Wg   the grid a row walks: N Hg Wg rows, at most 2^30
 *   dil    1, or 2: the input is x zero-dilated by two (odd coordinates load zeros, even ones x at half; zero padding only)
 *   reflect     outside the input: mirrored once (-i, 2 (n - 1) - i), or zero
 *   per_image   1: 64 x 64 tiles that never cross an image; 0: tiles over the batch's flat rows, 128 x 128 where those still fill
 *               the chip and Cout >= 128
 *   nph    tap tables in use, 1 .. 4 (the phases of a transposed convolution)
 * soar_selftest_conv_gemm hands the descriptor to the networks' own launcher and writes the side of the tile that launcher picks (64
 * or 128) to *tile_out.  The launcher refuses, with nothing launched: more than 2^30 rows; Cin no multiple of 8; nph outside
 * 1 .. 4; wbat without per_image; dil not 1 or 2, or 2 with reflect; stride, os, Cout, Hin or Win below 1; NULL x, y or a table's w;
 * x or w off 16 bytes, ldx, ldw or wbat no multiple of 4; ntaps outside 1 .. 9; py or px outside [0, os); with reflect, a coordinate
 * gy stride + dy outside [-(Hin - 1), 2 (Hin - 1)], likewise along x.  N Hg Wg == 0 is a no-op.
 * soar_selftest_conv_pack: torch [Cout][Cin][kk] -> fwd [Cout][kk][Cin] and, unless bwd is NULL, the data gradient's form, spatially
 * flipped and transposed: bwd[(ci kk + kk - 1 - t) ldb + co] (ldb >= Cout; the columns behind Cout are left alone). */
typedef struct SoarConvGemmTaps {
    const float *w;
    int64_t ldw;
    int32_t ntaps, py, px;
    int8_t dy[9], dx[9];
} SoarConvGemmTaps;
typedef struct SoarConvGemmArgs {
    const float *x;
    int64_t ldx, xim;
    int64_t wbat;
    const float *bias;
    const float *res;
    float *y;
    int64_t ldy, yim;
    float alpha;
    int32_t N, Hg, Wg;
    int32_t Hin, Win, Cin, Cout;
    int32_t stride, dil;
    int32_t reflect;
    int32_t Wout, os;
    int32_t per_image;
    int32_t nph;
    SoarConvGemmTaps ph[4];
} SoarConvGemmArgs;
int soar_selftest_conv_gemm(const SoarConvGemmArgs *args, int32_t *tile_out, void *stream);
int soar_selftest_conv_pack(const float *w, float *fwd, float *bwd, int32_t Cout, int32_t Cin, int32_t kk, int64_t ldb, void *stream);
/* The same with 16-bit operands: wtype 1 bf16, 2 f16.  soar_selftest_conv_gemm16 reads the taps' w as 16-bit values
 * (ldw and wbat still count elements), rounds A to the type (nearest even) as it is loaded and accumulates in float32; x, bias, res
 * and y stay float32.  It refuses, besides the above: a wtype outside 1 .. 2; an ldw or wbat that is no multiple of 8.
 * soar_selftest_conv_pack16: torch [Cout][Cin][kk] float32 -> fwd [Cout][kk][Cinp] of the type, rounded to nearest even, channels
 * Cin .. Cinp - 1 zeros (Cinp >= Cin); kk = 1 converts a linear layer's matrix.
 * soar_selftest_conv_pack16_bwd: the same tensor -> the data gradient's form in the type, soar_selftest_conv_pack's bwd:
 * bwd[(ci kk + kk - 1 - t) ldb + co], rounded to nearest even; ldb >= Cout and a multiple of 8, columns Cout .. ldb - 1 zeros. */
int soar_selftest_conv_gemm16(const SoarConvGemmArgs *args, int32_t wtype, int32_t *tile_out, void *stream);
int soar_selftest_conv_pack16(const float *w, void *fwd, int32_t Cout, int32_t Cin, int32_t Cinp, int32_t kk, int32_t wtype, void *stream);
int soar_selftest_conv_pack16_bwd(const float *w, void *bwd, int32_t Cout, int32_t Cin, int32_t kk, int64_t ldb, int32_t wtype, void *stream);
/* SoarConvGemmArgs carries no activation: the descriptor at either operand type (wtype 0 .. 2) with the epilogue's act (0 none, 1 exact
 * GELU, 2 ReLU): y = act(alpha (A B^T) + bias) + res */
int soar_selftest_conv_gemm_act(const SoarConvGemmArgs *args, int32_t wtype, int32_t act, int32_t *tile_out, void *stream);
/* ... and with the epilogue's PReLU: slope [Cout], one per output channel, or NULL (off).  Legal with act == 0 only (the
 * launcher refuses the pair); then y = (v > 0 ? v : slope[co] v) + res with v = alpha (A B^T) + bias, at every wtype. */
int soar_selftest_conv_gemm_slope(const SoarConvGemmArgs *args, int32_t wtype, int32_t act, const float *slope, int32_t *tile_out,
                                  void *stream);

/* ---- mesh export (mesh.hip, soar_amd/mesh.py; DESIGN.md "Mesh export").  Not part of the training step.
 * soar_tsdf_integrate: fuses n_views (1..64) rendered depth / opacity planes [n_views][H][W] into the TSDF of a dense grid
 *   [X][Y][Z] (X * Y * Z < 2^31) whose voxel (x, y, z) sits at origin + voxel * (x, y, z).  viewmatrix / projmatrix
 *   [n_views][16]: world_view_transform / full_proj_transform (row-vector convention); prcppoint [n_views][2].  Per voxel and
 *   view: skip when the view-space z <= znear or the nearest pixel floor(pix + 0.5) is outside the image; opac < min_opacity
 *   records s = +1, else skip when depth - z < -trunc, else s = min(1, (depth - z) / trunc); sum += s, weight += 1.
 *   Non-finite pixels: a view whose pixel has a NaN opacity, or an opacity >= min_opacity with a NaN depth, is no observation
 *   of that voxel (sum and weight stay as they were); +-inf follow the arithmetic above (+inf depth: s = 1; -inf depth:
 *   hidden, skipped; +inf opacity: opaque; -inf opacity: free space).  One thread per voxel, no atomics: deterministic.
 *   sum / weight are read and written in place (zero them before the first call); calls accumulate.
 * soar_mc_workspace_bytes / soar_mc_count / soar_mc_emit: marching cubes of values [X][Y][Z] at `level` (inside: value <
 *   level), valid [X][Y][Z] bytes or NULL.  An edge carries a vertex when both ends are valid and exactly one is inside; a
 *   cell emits triangles only when its 8 corners are valid.  soar_mc_count reads back counts_host[2] = {vertices, triangles}
 *   (a stream synchronisation: this is the export path); soar_mc_emit then writes verts [V][3] (index coordinates) and faces
 *   [F][3] (int32, facing the values above level) from the same workspace, values, valid and level.  Vertex ids follow
 *   (voxel, axis), triangles (cell, table order): the output is bit-identical from run to run.
 * soar_mesh_filter_bytes / soar_mesh_filter_components: removes the connected components (over the faces' edges) with fewer
 *   than min_faces faces or a bounding-box diagonal below min_diag_frac times the whole mesh's, and vertices used by no face;
 *   writes the kept vertices and the re-indexed faces in their input order to verts_out [<= V][3] / faces_out [<= F][3] and
 *   reads back counts_host[2] = {kept vertices, kept faces} (a stream synchronisation).  Deterministic.
 * All pointers but counts_host are device pointers; workspaces are 256-byte aligned and caller-owned. */
int soar_tsdf_integrate(int32_t n_views, int32_t H, int32_t W, const float *depth, const float *opac, const float *viewmatrix,
                        const float *projmatrix, const float *prcppoint, float origin_x, float origin_y, float origin_z, float voxel,
                        int32_t X, int32_t Y, int32_t Z, float trunc, float znear, float min_opacity, float *sum, float *weight,
                        void *stream);
int soar_mc_workspace_bytes(int32_t X, int32_t Y, int32_t Z, size_t *bytes);
int soar_mc_count(int32_t X, int32_t Y, int32_t Z, const float *values, const uint8_t *valid, float level, void *workspace,
                  size_t workspace_bytes, int64_t *counts_host, void *stream);
int soar_mc_emit(int32_t X, int32_t Y, int32_t Z, const float *values, const uint8_t *valid, float level, const void *workspace,
                 size_t workspace_bytes, float *verts, int32_t *faces, void *stream);
int soar_mesh_filter_bytes(int32_t V, int32_t F, size_t *bytes);
int soar_mesh_filter_components(int32_t V, int32_t F, const float *verts, const int32_t *faces, int32_t min_faces, float min_diag_frac,
                                void *workspace, size_t workspace_bytes, float *verts_out, int32_t *faces_out, int64_t *counts_host,
                                void *stream);
/* Decimation by quadric vertex clustering (mesh_simplify.hip; DESIGN.md 9b states the computation; not pymeshlab's edge collapse).
 * One output vertex per occupied cell of the uniform grid of size `cell` over the vertices' bounding box (n_k = floor((hi_k -
 * lo_k) / cell) + 1 cells along axis k, at most 2^21), placed at the minimum of the summed float64 face quadrics (eigenvalues
 * below 1e-3 of the largest count as zero; the cluster's mean vertex where that leaves the cell's neighbourhood); faces with two
 * corners in one cell and all but the first of the faces with the same three cells are dropped, cells no face uses too.
 * Surviving faces keep their input order and winding, output vertices follow the cell key (ix * ny + iy) * nz + iz.
 * soar_mesh_simplify_bytes: the workspace of a mesh of 1 <= V <= 2^30 vertices and 0 <= F <= 2^30 faces.
 * soar_mesh_simplify_count: counts_host[2] = {output vertices, output faces} for `cell`; no quadric work, no output mesh.
 * soar_mesh_simplify: the same counts, verts_out [<= V][3] and faces_out [<= F][3].
 * Refused before any launch: V < 1, F < 0, V or F above 2^30, a cell size that is not positive and finite, NULL pointers, a short or misaligned
 * workspace.  Refused after the bounding-box launch, before any other: a non-finite coordinate, more than 2^21 cells along an
 * axis.  Both read back the bounding box and the totals (two stream synchronisations).  Deterministic bit for bit. */
int soar_mesh_simplify_bytes(int32_t V, int32_t F, size_t *bytes);
int soar_mesh_simplify_count(int32_t V, int32_t F, const float *verts, const int32_t *faces, float cell, void *workspace,
                             size_t workspace_bytes, int64_t *counts_host, void *stream);
int soar_mesh_simplify(int32_t V, int32_t F, const float *verts, const int32_t *faces, float cell, void *workspace,
                       size_t workspace_bytes, float *verts_out, int32_t *faces_out, int64_t *counts_host, void *stream);
/* Colour, smoothing and pruning of the exported mesh (mesh_attr.hip; DESIGN.md 9b, "Colour, smoothing, skinning" states the
 * computation).  Every workspace is the caller's, 256-byte aligned, sized by the call's _bytes query.  A size, pointer or
 * workspace that is refused is refused before anything is launched; the CONTENTS of idx and faces can only be judged on the
 * device, so transfer, adjacency and prune refuse those after their launches, with their outputs written (see each call).
 * soar_mesh_attr_transfer: verts [V][3] mesh vertices, points [N][3] surfel centres, colors [N][3], idx [V][K] the K nearest centres
 *   of every vertex, 1 <= K <= 8, AS soar_lbs_knn_query WRITES THEM to knn_idx_out (ascending float32 squared distance, equal
 *   distances among the K by ascending index; that order is kept.  Which of several points at exactly the K-th distance the
 *   search keeps is its grid walk's matter, not the lower index: it admits only a strictly nearer point).  color_out [V][3] = clamp(float32 mean of the K colours added in rank order, 0, 1);
 *   quality_out [V] = the squared distance to rank 0, (dx dx + dy dy) + dz dz in float32; d2_out [V][K] all K of them, or NULL.
 *   Reads back how many vertices had an index outside [0, N) (one stream synchronisation) and refuses then.
 * soar_mesh_adjacency: faces [F][3] -> CSR rows.  row_start [V + 1], nbr [6 F], border [V].  Row i holds, for every face at i, its
 *   two other corners; the row is ascending, so a neighbour across an edge of m faces stands m times.  border[i] = 1 when some
 *   neighbour stands exactly once (an edge of exactly one face).  Built by a sort of the 6 F entries: deterministic.  faces and nbr
 *   may be NULL when F = 0.  A face naming a vertex outside [0, V) or one vertex twice is counted on the device and the call
 *   refused at its end (its one stream synchronisation); the rows written then leave that face out and are not to be used.
 * soar_mesh_smooth: `steps` Jacobi steps of the uniform umbrella operator over those rows: S = the sum of the positions of the row in
 *   row order -- for a border vertex only of the neighbours that stand once --, P' = (P + S) / (n + 1), n the number of terms; n = 0
 *   keeps P.  float32, no atomics: bit-reproducible.  verts_out [V][3] must not be verts; steps = 0 copies.  nnz = 6 F; row bounds
 *   and entries outside their ranges are skipped.
 * soar_mesh_prune: drops the vertices with quality > thresh (a NaN quality stays) and the faces that touch one; the kept keep their
 *   order, faces are re-indexed, keep_out [<= V] = the old index of every new vertex, counts_host[2] = {vertices, faces} kept.
 *   verts_out [<= V][3], faces_out [<= F][3].  One stream synchronisation, for the totals.
 * All: 1 <= V <= 2^30, 0 <= F <= 2^28. */
int soar_mesh_attr_transfer_bytes(int32_t V, int32_t K, size_t *bytes);
int soar_mesh_attr_transfer(int32_t V, int32_t N, int32_t K, const float *verts, const float *points, const float *colors,
                            const int32_t *idx, void *workspace, size_t workspace_bytes, float *color_out, float *quality_out,
                            float *d2_out, void *stream);
int soar_mesh_adjacency_bytes(int32_t V, int32_t F, size_t *bytes);
int soar_mesh_adjacency(int32_t V, int32_t F, const int32_t *faces, void *workspace, size_t workspace_bytes, int32_t *row_start,
                        int32_t *nbr, uint8_t *border, void *stream);
int soar_mesh_smooth_bytes(int32_t V, size_t *bytes);
int soar_mesh_smooth(int32_t V, int32_t nnz, const float *verts, const int32_t *row_start, const int32_t *nbr, const uint8_t *border,
                     int32_t steps, void *workspace, size_t workspace_bytes, float *verts_out, void *stream);
int soar_mesh_prune_bytes(int32_t V, int32_t F, size_t *bytes);
int soar_mesh_prune(int32_t V, int32_t F, const float *verts, const int32_t *faces, const float *quality, float thresh, void *workspace,
                    size_t workspace_bytes, float *verts_out, int32_t *faces_out, int32_t *keep_out, int64_t *counts_host, void *stream);
/* Hole closing of the exported mesh (mesh_holes.hip; DESIGN.md 9b, "Closing holes" states the definition: a deterministic loop
 * search with a centroid fan, NOT MeshLab's minimum-weight ear cutting).  Half-edge h = 3 f + c runs faces[f][c] ->
 * faces[f][(c + 1) % 3]; it is a border when its undirected edge occurs once among the 3 F half-edges (soar_mesh_adjacency's rule).
 * A vertex is simple when one border half-edge leaves it and one arrives.  A loop of 3 <= n <= max_hole_edges border half-edges
 * whose vertices are all simple and which do not all come from one face is closed: n = 3 by one face, n >= 4 by one new vertex (the
 * mean of the ring's vertices, added in float64 in ring order from the loop's least half-edge id, rounded once) and n faces, every
 * new face with its border edge reversed.  Anything else is left as it is.
 * soar_mesh_close_holes: verts_out [V + (3 F) / 4][3] and faces_out [4 F][3] hold the V vertices and F faces unchanged, then the new
 *   ones loop by loop in ascending order of the loops' least half-edge ids; loop_edges_out [F] the n of every closed loop in that
 *   order; counts_host[4] = {vertices, faces, loops closed, border half-edges still open}.  The outputs must not be the inputs.
 *   1 <= V <= 2^30, 0 <= F <= 2^28, 3 <= max_hole_edges <= 65535; the workspace is the caller's, 256-byte aligned, sized by
 *   soar_mesh_close_holes_bytes; sizes, pointers and workspaces that are refused are refused before any launch.  F = 0 copies the
 *   vertices (faces, faces_out and loop_edges_out may then be NULL).  A face naming a vertex outside [0, V) or one vertex twice is
 *   counted on the device and the call refused at its end (the one stream synchronisation, which also reads the totals); the outputs
 *   written then are not to be used.  Integer atomics only: bit-reproducible. */
int soar_mesh_close_holes_bytes(int32_t V, int32_t F, size_t *bytes);
int soar_mesh_close_holes(int32_t V, int32_t F, const float *verts, const int32_t *faces, int32_t max_hole_edges, void *workspace,
                          size_t workspace_bytes, float *verts_out, int32_t *faces_out, int32_t *loop_edges_out, int64_t *counts_host,
                          void *stream);
/* Repair of non-manifold edges and vertices of the exported mesh (mesh_repair.hip; DESIGN.md 9b, "Repairing non-manifold edges and
 * vertices" states the definition; MeshLab's two repair filters made order-free, NOT its edge-splitting method).  In order: a face
 * with two equal corners goes; on every undirected edge with k > 2 remaining faces the k - 2 that come first in ascending (bits of
 * the float32 squared doubled area as uint32, face index) go, in one pass; over the corners of the surviving faces, the two faces of
 * every edge that has exactly two are joined at both ends of the edge, a fan is a connected set of corners and its id its least
 * corner index 3 f + c; per vertex the fan of least id keeps the vertex and every other fan gets a copy of it.  Output: the input
 * vertices some surviving face names, in input order, then the copies in ascending fan id; the surviving faces in input order and
 * winding.
 * soar_mesh_repair_count: the analysis alone.  counts_host[9] = {output vertices, output faces, edges that had more than two faces,
 *   faces removed on such edges, faces with two equal corners dropped, copies added, input vertices no surviving face names, edges
 *   of the result whose two faces run in the same direction (counted, not changed), border edges of the result}.
 * soar_mesh_repair: runs the same analysis again (it does not depend on what the workspace holds) and writes verts_out
 *   [counts_host[0]][3], faces_out [counts_host[1]][3] and source_out [counts_host[0]] = the input vertex every output vertex came
 *   from; the sizes are those soar_mesh_repair_count reports for the same mesh (never more than 3 F vertices and F faces).  The
 *   outputs must not be the inputs.
 * 1 <= V <= 2^30, 0 <= F <= 2^28; the workspace is the caller's, 256-byte aligned, sized by soar_mesh_repair_workspace_size; sizes, pointers
 * and workspaces that are refused are refused before any launch.  F = 0 launches nothing (no vertex is named: the result is empty).
 * A face naming a vertex outside [0, V) is counted on the device and the call refused at its one stream synchronisation, which also
 * reads the counts: soar_mesh_repair_count writes nothing but its workspace; what soar_mesh_repair wrote by then is not to be used.
 * Integer atomics only (atomicMin hooking, same-value flag stores, counters): bit-reproducible. */
int soar_mesh_repair_workspace_size(int32_t V, int32_t F, size_t *bytes);
int soar_mesh_repair_count(int32_t V, int32_t F, const float *verts, const int32_t *faces, void *workspace, size_t workspace_bytes,
                           int64_t *counts_host, void *stream);
int soar_mesh_repair(int32_t V, int32_t F, const float *verts, const int32_t *faces, void *workspace, size_t workspace_bytes,
                     float *verts_out, int32_t *faces_out, int32_t *source_out, int64_t *counts_host, void *stream);
/* The texture atlas of the exported mesh (mesh_texture.hip, soar_amd/texture.py; DESIGN.md 9b, "Texture atlas" states the layout).
 * Every face gets half of a square cell of side s texels, s a power of two in [4, texture_size / 2]; the cells stand one behind the
 * other, largest first, on the Morton curve of the image's 4 x 4 texel units.  texture_size is a power of two in [16, 16384];
 * 1 <= V <= 2^30, 1 <= F <= 2^28; every workspace is the caller's, 256-byte aligned, sized by its _bytes query; a size, pointer or
 * workspace that is refused is refused before any launch.  Integer atomics only: bit-reproducible.
 * soar_mesh_atlas_levels: the float32 area of every face (0.5 sqrt of the squared cross product of its two edges from corner 0,
 *   every operation rounded as written, the square root correctly rounded), its level = the number of the n_ladder <= 1024 ascending
 *   thresholds ladder[] (device) that are <= area, kept in the workspace (its first F int32 words; -1: no area), and hist_host[n_ladder + 2] = the faces of every level 0 .. n_ladder, then the faces whose
 *   area is not a positive finite number.  One stream synchronisation; a face naming a vertex outside [0, V) is refused there.
 * soar_mesh_atlas_place: with the workspace soar_mesh_atlas_levels filled for the same faces and ladder.  Side of a face:
 *   q = floor((level + scale_step) / 8), s = 4 for q < 2 (and for the faces without an area), texture_size / 2 for
 *   q >= log2(texture_size / 2), else 2^q.  Order: decreasing s, then face index; the r-th face of a size takes half r % 2 (0: lower)
 *   of that size's cell r / 2.  Writes cell_out [F][4] = {x0, y0, s, half} (image texels, row 0 at the top), uv_out [3 F][2] (OBJ
 *   convention, v = 0 at the bottom; the corners sit on texel centres) and uv_faces_out [F][3] = {3 f, 3 f + 1, 3 f + 2}.  A
 *   scale_step whose cells do not fit the image is refused (one stream synchronisation) before anything is written.
 * soar_mesh_texel_offsets: checks every cell (a power-of-two square in [4, texture_size / 2], aligned to its side, inside the image)
 *   and every face, and enumerates the texels the faces own, face after face: a lower half owns the local texels with
 *   a + b <= s - 1, an upper half those with a + b >= s.  total_host = their number; the ranges stay in the workspace.  One stream
 *   synchronisation; bad cells or faces are refused there, and nothing else of this group runs on them.  Cells are checked ONE BY
 *   ONE: that two cells of a hand-made atlas overlap is noticed only when the texels owned exceed T^2.  Overlapping cells that
 *   pass are written twice, in the enumeration's order: in bounds and repeatable, but not an atlas.  soar_mesh_atlas_place's are disjoint.
 * soar_mesh_texels: for the texels first .. first + count - 1 of that enumeration, pos_out [count][3] = b0 v0 + b1 v1 + b2 v2 with
 *   the barycentrics of the texel centre in UV space (from the integers a, b and m = s - 3; negative weights clamped to 0 and the
 *   three divided by their sum) and addr_out [count] = y * texture_size + x.  A position that is not finite is written as the origin
 *   and its address as ~addr.  owner_img [T^2], bary_img [T^2][3], position_img [T^2][3]: optional images of the face, the weights
 *   and the unmodified position of every texel visited.
 * soar_mesh_texture_write: texture_out [T^2][3] bytes = floor(255 c + 0.5) of color [count][3] clamped to [0, 1] at the addresses
 *   soar_mesh_texels wrote (1 <= count <= T^2), zero at a flagged (~addr) one; color_img [T^2][3] optionally receives the floats behind the bytes. */
int soar_mesh_atlas_bytes(int32_t F, size_t *bytes);
int soar_mesh_atlas_levels(int32_t V, int32_t F, const float *verts, const int32_t *faces, const float *ladder, int32_t n_ladder,
                           void *workspace, size_t workspace_bytes, int64_t *hist_host, void *stream);
int soar_mesh_atlas_place(int32_t F, int32_t texture_size, int32_t n_ladder, int32_t scale_step, void *workspace, size_t workspace_bytes,
                          float *uv_out, int32_t *uv_faces_out, int32_t *cell_out, void *stream);
int soar_mesh_texels_bytes(int32_t F, size_t *bytes);
int soar_mesh_texel_offsets(int32_t V, int32_t F, int32_t texture_size, const int32_t *faces, const int32_t *cell, void *workspace,
                            size_t workspace_bytes, int64_t *total_host, void *stream);
int soar_mesh_texels(int32_t V, int32_t F, int32_t texture_size, const float *verts, const int32_t *faces, const int32_t *cell,
                     const void *workspace, size_t workspace_bytes, int64_t first, int32_t count, float *pos_out, int32_t *addr_out,
                     int32_t *owner_img, float *bary_img, float *position_img, void *stream);
int soar_mesh_texture_write(int32_t count, int32_t texture_size, const int32_t *addr, const float *color, uint8_t *texture_out,
                            float *color_img, void *stream);

/* ---- the surfels' attribute field (field.hip, soar_amd/field.py; DESIGN.md "Attribute field"): the reference's HashMLPSDFField
 * (TS/geometry/sdf_fields.py:41-219) with nerfstudio's torch HashEncoding / MLP semantics.  Two multiresolution hash encodings of
 * SOAR_FIELD_LEVELS levels x 2 features (`table` for shs, scales, offsets, opacities; `qtable` for quats), five heads
 * Linear(in, 64) -> ReLU -> Linear(64, out) with in = 32 (offsets: 34, the encoding and z) and out = 3, 1, 4, 3, 1.
 *   p = (xyz - aabb[0]) / (aabb[1] - aabb[0]) and p = 0 unless 0 < p < 1 on every axis (normalized = 0), else p = xyz;
 *   per level l: q = p * res[l], c = ceil(q), f = floor(q) (int32), o = q - f; corner slots
 *   ((u32)x ^ (u32)y * 2654435761 ^ (u32)z * 805459861) & (2^log2_T - 1), rows l * 2^log2_T + slot of [16 * 2^log2_T][2] tables;
 *   trilinear weights in o.  Outputs: shs = sigmoid, scales = sigmoid * 2e-2, quats = x / max(|x|, 1e-12), offsets (input
 *   [encoding, z], z = 0 when NULL), opacities = sigmoid.
 * Head index k: 0 shs, 1 scales, 2 quats, 3 offsets, 4 opacities.  Weights as nn.Linear keeps them: w1 [64][in], b1 [64],
 *   w2 [out][64], b2 [out].  A head's gradient buffer d_head[k] holds SOAR_FIELD_HEAD_FLOATS(in, out) floats:
 *   dw1 [64][in], db1 [64], dw2 [out][64], db2 [out], in that order.
 * soar_field_forward writes out[k] ([N][out]) and the two encodings enc / qenc ([N][32]), which soar_field_backward reads.
 * soar_field_backward: g_out[k] [N][out] upstream gradients, NULL = zero (the head then launches nothing).  Writes what is not
 *   NULL of d_table / d_qtable ([16 * 2^log2_T][2], zero-filled by the call), d_head[k], d_xyz [N][3], d_z [2].  The head
 *   gradients and d_xyz / d_z are sums in a fixed order: bitwise reproducible.  The table gradients are float atomics
 *   (global_atomic_add_f32 per corner and feature; neighbouring lanes of a wave that hold the same row add once): their last bits
 *   depend on arrival order.  The workspace holds
 *   soar_field_workspace_bytes(N) bytes, 256-byte aligned.  No host synchronisation, no allocation: both calls can be captured.
 * 0 <= N <= 2^26; N = 0 launches no kernel (the backward still zero-fills its outputs). */
#define SOAR_FIELD_LEVELS 16
#define SOAR_FIELD_HIDDEN 64
#define SOAR_FIELD_HEAD_FLOATS(in, out) (SOAR_FIELD_HIDDEN * (in) + SOAR_FIELD_HIDDEN + (out) * SOAR_FIELD_HIDDEN + (out))
typedef struct SoarFieldHead {
    const float *w1, *b1, *w2, *b2;
} SoarFieldHead;

typedef struct SoarFieldArgs {
    int32_t N;
    int32_t log2_T;                  /* rows per level = 2^log2_T, 1 <= log2_T <= 24 */
    int32_t normalized;              /* is_normalized: no aabb, no selector */
    int32_t pad_;
    float res[SOAR_FIELD_LEVELS];    /* level resolutions (float32, nerfstudio's `scalings`) */
    const float *xyz;                /* [N][3] */
    const float *aabb;               /* [2][3]; unused when normalized */
    const float *table, *qtable;     /* [16 * 2^log2_T][2] each */
    const float *z;                  /* [2] or NULL */
    SoarFieldHead head[5];
    float *enc, *qenc;               /* [N][32] each */
    float *out[5];                   /* forward outputs [N][out_k] */
    const float *g_out[5];           /* backward: upstream gradients or NULL */
    float *d_table, *d_qtable;       /* backward outputs or NULL */
    float *d_head[5];
    float *d_xyz, *d_z;
} SoarFieldArgs;

int soar_field_workspace_bytes(int32_t N, size_t *bytes);
int soar_field_forward(const SoarFieldArgs *args, void *stream);
int soar_field_backward(const SoarFieldArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the environment-map background (envmap.hip, soar_amd/background.py): the reference's
 * NeuralEnvironmentMapBackground ("gaussiandreamer-background") with tiny-cuda-nn's SphericalHarmonics (degree 3) and threestudio's
 * VanillaMLP (16 neurons, 2 hidden layers, no bias, ReLU), then sigmoid.  Per pixel of dirs [B][H][W][3]:
 *   x = ((d + 1) / 2) * 2 - 1 per component (float32; |d| = 1 is not assumed), e = the 9 SH values of x (bands 0..2, with the
 *   0.94617469575755997 z^2 - 0.31539156525251999 form), bg = sigmoid(w3 relu(w2 relu(w1 e))) with w1 [16][9], w2 [16][16], w3 [3][16]
 *   as nn.Linear keeps them.  color != NULL: bg = color[row] ([1][3] for every row or [B][3] per row) and the MLP is skipped.
 * soar_envmap_forward writes bg [B][H][W][3] and, for the first n_comp rows, comp [n_comp][3][H][W] = render + (1 - mask) * bg,
 *   each of the three operations rounded on its own.  render [n_comp][3][H][W] and mask [n_comp][1][H][W] are contiguous per image,
 *   render_stride / mask_stride elements apart.
 * soar_envmap_backward: g_comp the gradient of comp at strides g_comp_stride (elements, NCHW order; NULL = zero), g_bg [B][H][W][3]
 *   contiguous (NULL = zero).  Writes what is not NULL of g_mask [n_comp][H][W] = -sum_c g_comp_c * bg_c, and d_w1 / d_w2 / d_w3
 *   (all three or none): (1 - mask) g_comp + g_bg back through the sigmoid and the layers, summed over the pixels in double in a
 *   fixed order (bitwise reproducible; exact zeros with color != NULL).  The gradient of render is g_comp itself (no kernel).  The
 *   workspace holds soar_envmap_workspace_bytes(B, H, W) bytes, 256-byte aligned.  No host synchronisation, no allocation: both
 *   calls can be captured.  B * H * W <= 2^30; B * H * W = 0 launches no kernel (the backward still zero-fills d_w*). */
#define SOAR_ENVMAP_ENC 9
#define SOAR_ENVMAP_HIDDEN 16
#define SOAR_ENVMAP_WEIGHTS (SOAR_ENVMAP_HIDDEN * SOAR_ENVMAP_ENC + SOAR_ENVMAP_HIDDEN * SOAR_ENVMAP_HIDDEN + 3 * SOAR_ENVMAP_HIDDEN)
typedef struct SoarEnvmapArgs {
    int32_t B, H, W;
    int32_t n_comp;                  /* rows composited, 0 <= n_comp <= B */
    int32_t color_rows;              /* rows of color: 1 or B (read only when color != NULL) */
    int32_t pad_;
    int64_t render_stride, mask_stride;  /* elements from one image of render / mask to the next */
    int64_t g_comp_stride[4];        /* strides of g_comp in elements, NCHW order */
    const float *dirs;               /* [B][H][W][3]; unused when color != NULL */
    const float *w1, *w2, *w3;       /* [16][9], [16][16], [3][16]; unused when color != NULL */
    const float *color;              /* device [color_rows][3] or NULL (the MLP) */
    const float *render, *mask;
    float *bg;                       /* forward output [B][H][W][3] */
    float *comp;                     /* forward output [n_comp][3][H][W] */
    const float *g_comp;             /* backward inputs or NULL */
    const float *g_bg;
    float *g_mask;                   /* backward outputs or NULL */
    float *d_w1, *d_w2, *d_w3;
} SoarEnvmapArgs;

int soar_envmap_workspace_bytes(int32_t B, int32_t H, int32_t W, size_t *bytes);
int soar_envmap_forward(const SoarEnvmapArgs *args, void *stream);
int soar_envmap_backward(const SoarEnvmapArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* ---- LPIPS-VGG (lpips.hip, soar_amd/lpips.py): lpips 0.1, net='vgg', eval mode, spatial=False.  Per image n of
 * in0 / in1 [N][3][H][W] (float32, any element strides, NCHW order):
 *   x' = (x - shift) / scale, VGG16 features[0:30] (13 conv3x3 pad 1 + bias + ReLU, 2x2 max pools in floor mode after relu1_2,
 *   relu2_2, relu3_3, relu4_3), taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3; per tap k and pixel: u = f / (sqrt(sum_c f_c^2)
 *   + 1e-10), s = sum_c lin_k[c] (u0_c - u1_c)^2; out[n] = sum_k mean over the tap's pixels of s.
 * soar_lpips_pack_weights builds the private packed form (soar_lpips_weights_bytes bytes, 256-byte aligned) from the torch layouts:
 *   conv_w[i] [Cout][Cin][3][3], conv_b[i] [Cout], lin[k] [C_k], shift [3], scale [3], all contiguous device arrays.
 * soar_lpips_forward writes out [N] and, for every branch whose bit is set in `grads` (1: in0, 2: in1), keeps that branch's activations
 *   and its tap gradients in the workspace (soar_lpips_workspace_bytes(N, H, W, grads) bytes, 256-byte aligned); a branch without
 *   its bit keeps nothing.  soar_lpips_backward, with the same workspace and `grads` as the forward before it, writes g_in0 / g_in1
 *   (NULL = not wanted; the bit must have been set) at their own strides: the input gradient of out scaled by g_out [N].
 *   Every sum has a fixed order (bitwise reproducible); no host synchronisation, no allocation: both calls can be captured.
 *   H, W >= 16, N >= 0 (N = 0 launches nothing), N * H * W <= 2^30. */
#define SOAR_LPIPS_LAYERS 13
#define SOAR_LPIPS_TAPS 5
typedef struct SoarLpipsWeights {
    const float *conv_w[SOAR_LPIPS_LAYERS];
    const float *conv_b[SOAR_LPIPS_LAYERS];
    const float *lin[SOAR_LPIPS_TAPS];
    const float *shift, *scale;
} SoarLpipsWeights;
typedef struct SoarLpipsArgs {
    int32_t N, H, W;
    int32_t grads;                   /* bit 0: in0's branch is kept for a backward, bit 1: in1's */
    const float *in0, *in1;          /* [N][3][H][W] at in*_stride (elements, NCHW order) */
    int64_t in0_stride[4], in1_stride[4];
    const void *weights;             /* soar_lpips_pack_weights' output */
    float *out;                      /* forward output [N] */
    const float *g_out;              /* backward input [N] */
    float *g_in0, *g_in1;            /* backward outputs or NULL, at g_in*_stride */
    int64_t g_in0_stride[4], g_in1_stride[4];
} SoarLpipsArgs;

int soar_lpips_weights_bytes(size_t *bytes);
int soar_lpips_pack_weights(const SoarLpipsWeights *w, void *packed, size_t packed_bytes, void *stream);
int soar_lpips_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t grads, size_t *bytes);
int soar_lpips_forward(const SoarLpipsArgs *args, void *workspace, size_t workspace_bytes, void *stream);
int soar_lpips_backward(const SoarLpipsArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the SDS guidance's VAE encoder and loss tail (vae.hip, soar_amd/sds.py) ----
 * The Stable-Diffusion-2.1 AutoencoderKL encoder (ldm Encoder: ch 128, ch_mult (1,2,4,4), 2 ResnetBlocks per level without temb,
 * GroupNorm 32 groups eps 1e-6 + SiLU, Downsample = zero pad right / bottom by 1 + 3x3 stride-2 conv, mid ResnetBlock / single-head
 * AttnBlock / ResnetBlock, norm_out + SiLU + conv_out 512 -> 8) and quant_conv 8 -> 8; mean, logvar = chunk(2); logvar clamped to
 * [-30, 20]; latents = scale_factor (mean + exp(0.5 logvar) eps).  The input x [N][3][H][W] (any element strides, NCHW order) is
 * resized to image_size^2 (bilinear, align_corners=False, no antialias) and mapped x * 2 - 1 on load.
 * Raw weights: one contiguous device float array of soar_vae_weights_floats floats, ldm's tensors in their torch layouts, in this
 * order (soar_amd/sds.py: WEIGHT_ORDER): conv_in.w, .b; for level i = 0..3, block j = 0..1: norm1.w, .b, conv1.w, .b, norm2.w, .b,
 * conv2.w, .b, (nin_shortcut.w, .b when Cin != Cout); downsample.conv.w, .b (i < 3); mid.block_1 (as a block); mid.attn_1: norm.w,
 * .b, q.w, .b, k.w, .b, v.w, .b, proj_out.w, .b; mid.block_2; norm_out.w, .b; conv_out.w, .b; quant_conv.w, .b.
 * soar_vae_pack_weights builds the private packed form (soar_vae_weights_bytes bytes, 256-byte aligned).
 * soar_vae_forward writes mean / logvar [N][4][h][w] (h = w = image_size / 8; NULL = not wanted) and, when latents is not NULL,
 *   latents from eps [N][4][h][w]; it keeps what the backward needs in the workspace (soar_vae_workspace_bytes bytes).
 * soar_vae_backward, with the workspace of the forward before it (latents written), writes g_x at its strides: the data gradient of
 *   latents scaled by g_latents (times *g_scale when not NULL), times grad_scale[n][y][x] (NULL = 1) per input pixel.  The weights
 *   get no gradient.
 * Every sum has a fixed order, independent of N (bitwise reproducible; N = 4 equals four N = 1 calls); no host synchronisation, no
 * allocation: both calls can be captured.  N >= 0 (N = 0 launches nothing), H, W >= 1, image_size a positive multiple of 8,
 * N * image_size^2 and N * H * W <= 2^28. */
typedef struct SoarVaeArgs {
    int32_t N, H, W, image_size;
    const float *x;                  /* [N][3][H][W] at x_stride (elements, NCHW order) */
    int64_t x_stride[4];
    const void *weights;             /* soar_vae_pack_weights' output */
    float scale_factor;
    const float *eps;                /* [N][4][h][w] posterior noise (needed when latents is not NULL) */
    float *mean, *logvar, *latents;  /* forward outputs [N][4][h][w] or NULL */
    const float *g_latents;          /* backward input [N][4][h][w] */
    const float *g_scale;            /* backward: a device scalar multiplied into g_latents, or NULL */
    const float *grad_scale;         /* backward: per input pixel [N][H][W] at grad_scale_stride, or NULL */
    int64_t grad_scale_stride[3];
    float *g_x;                      /* backward output at g_x_stride */
    int64_t g_x_stride[4];
} SoarVaeArgs;

int soar_vae_weights_floats(size_t *floats);
int soar_vae_weights_bytes(size_t *bytes);
int soar_vae_pack_weights(const float *raw, size_t raw_floats, void *packed, size_t packed_bytes, void *stream);
int soar_vae_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t image_size, size_t *bytes);
int soar_vae_forward(const SoarVaeArgs *args, void *workspace, size_t workspace_bytes, void *stream);
int soar_vae_backward(const SoarVaeArgs *args, void *workspace, size_t workspace_bytes, void *stream);
/* The same encoder with 16-bit matrix-core products.  precision: 0 f32 (the entries above, bit for bit), 1 bf16,
 * 2 f16; anything else is refused and nothing is launched.  At 1 / 2 exactly the products whose B operand is a weight tensor
 * (the residual blocks' conv1 / conv2 / nin_shortcut, the stride-2 downsamples, q | k | v, proj_out, and the data gradient of each)
 * read 16-bit packed weights and round their A operand to the type (nearest even) as it is loaded; sums, activations in memory,
 * conv_in, conv_out, quant_conv, the attention's activation products, softmax, GroupNorm, the resize and the sample stay float32.
 * SoarVaeArgs, the workspace and its size are those above.  soar_vae_weights_bytes16: the packed size at the precision (the 16-bit
 * tensors take half).  soar_vae_pack_weights16 refuses a packed_bytes other than exactly that.  weights must come from
 * soar_vae_pack_weights16 at the same precision.
 * soar_vae_backward16 at 1 / 2 applies *g_scale behind the last 16-bit product (at conv_in's data gradient), not to g_latents, so a
 * small loss weight never enters a 16-bit operand; at f16 it also runs on g_latents 2^10 and multiplies by 2^-10 in that same step.
 * Both are exact in float32.  The 2^10 is this library's choice, checked on random weights only: train with bf16. */
int soar_vae_weights_bytes16(int32_t precision, size_t *bytes);
int soar_vae_pack_weights16(const float *raw, size_t raw_floats, void *packed, size_t packed_bytes, int32_t precision, void *stream);
int soar_vae_forward16(const SoarVaeArgs *args, int32_t precision, void *workspace, size_t workspace_bytes, void *stream);
int soar_vae_backward16(const SoarVaeArgs *args, int32_t precision, void *workspace, size_t workspace_bytes, void *stream);

/* The loss tail around the caller's UNet (ImageDream's MultiviewDiffusionGuidance.forward), t read from device memory (clamped to
 * [0, n_timesteps)).  tables [5][n_timesteps]: sqrt(ac), sqrt(1 - ac), sqrt(1 / ac), sqrt(1 / ac - 1), ac (alphas_cumprod).
 * soar_sds_q_sample: x_in [2B][4][h][w], both halves = sqrt(ac[t]) latents + sqrt(1 - ac[t]) noise.
 * soar_sds_loss, eps_pred [2B][4][h][w] = (text, uncond): e = uncond + guidance_scale (text - uncond);
 *   SOAR_SDS_RECON: recon = sqrt(1/ac) x_t - sqrt(1/ac - 1) e; with recon_std_rescale r > 0, per group of n_view images
 *     recon = r recon f + (1 - r) recon, f = (std(recon_text) + 1e-8) / (std(recon) + 1e-8) (unbiased std over the group);
 *     loss = 0.5 sum (latents - recon)^2 / B, g_lat = (latents - recon) / B, grad_norm = |g_lat|;
 *   SOAR_SDS_PLAIN: g = (1 - ac[t]) (e - noise), clamped to +-grad_clip when grad_clip > 0, nan_to_num; loss = 0.5 sum g^2 / B,
 *     g_lat = g / B, grad_norm = |g|.
 *   loss, grad_norm: device scalars.  One workgroup, sums in double in a fixed order. */
#define SOAR_SDS_PLAIN 0
#define SOAR_SDS_RECON 1
typedef struct SoarSdsArgs {
    int32_t B, n_view, h, w;
    int32_t mode, n_timesteps;
    float guidance_scale, recon_std_rescale, grad_clip;
    const int64_t *t;                /* device scalar */
    const float *tables;             /* [5][n_timesteps] */
    const float *latents, *noise;    /* [B][4][h][w] */
    const float *eps_pred;           /* [2B][4][h][w] */
    float *x_in;                     /* q_sample output [2B][4][h][w] */
    float *loss, *grad_norm;         /* device scalars */
    float *g_lat;                    /* [B][4][h][w] */
} SoarSdsArgs;

int soar_sds_q_sample(const SoarSdsArgs *args, void *stream);
int soar_sds_loss(const SoarSdsArgs *args, void *stream);

/* ---- the geometry model's per-surfel passes (soar_amd/geometry.py, csrc/geometry.hip).  One thread per surfel, one launch each.
 * Activations (TS/geometry/surfel_base.py:441-476): rotation_out = rotation / max(|rotation|_2, 1e-12) (F.normalize) [P][4],
 * scaling_out = exp(scaling) [P][S] (S in 1..3), opacity_out / occ_out [P] and colors_out [P][3] = sigmoid.  An input that is NULL
 * is skipped together with its output.  Backward: the five leaf gradients d_* from the five output gradients g_* (NULL = zero; a
 * d_* that is NULL is not written), from the SAVED outputs (and, for the normalisation, the leaf: its norm is needed once more).
 * P = 0 succeeds without a launch. */
int soar_surfel_activations_forward(int32_t P, int32_t S, const float *rotation, const float *scaling, const float *opacity,
                                    const float *occ, const float *colors, float *rotation_out, float *scaling_out,
                                    float *opacity_out, float *occ_out, float *colors_out, void *stream);
int soar_surfel_activations_backward(int32_t P, int32_t S, const float *rotation, const float *rotation_out, const float *scaling_out,
                                     const float *opacity_out, const float *occ_out, const float *colors_out,
                                     const float *g_rotation, const float *g_scaling, const float *g_opacity, const float *g_occ,
                                     const float *g_colors, float *d_rotation, float *d_scaling, float *d_opacity, float *d_occ,
                                     float *d_colors, void *stream);
/* The per-surfel regularizers of the training step (TS/system/gaussian_surfel_mvdream.py:257-296), values and gradients in one pass:
 *   terms[0] = mean(|xyz|_2), [1] = mean(|xyz - original_pos|_2), [2] = sum(|scaling|_2 opacity) (no gradient to scaling),
 *   [3] = -mean((opacity - 0.5)^2), [4] = mean(scales), [5] = sum_t coef[t] terms[t].
 * xyz, original_pos [P][3]; scaling [P][S] and opacity [P] activated; scales [P][K] (S, K in 1..3).  coef_dev: five floats in
 * device memory; a term whose coefficient is 0 is reported as 0 and contributes no gradient.  upstream_dev: a device scalar every
 * gradient is multiplied by, or NULL (1).  g_xyz [P][3], g_opacity [P], g_scales [P][K] (each may be NULL) receive
 * upstream * sum_t coef[t] d terms[t]; the norm's gradient at a zero vector is zero (torch).  Sums: per-workgroup partial sums in
 * double in `workspace` (soar_surfel_regularizers_workspace_bytes), added in a fixed order by a second one-workgroup launch: the
 * values are bitwise reproducible.  terms_dev: six floats.  P = 0 succeeds without a launch and writes nothing. */
int soar_surfel_regularizers_workspace_bytes(int32_t P, size_t *bytes);
int soar_surfel_regularizers(int32_t P, int32_t S, int32_t K, const float *xyz, const float *original_pos, const float *scaling,
                             const float *opacity, const float *scales, const float *coef_dev, const float *upstream_dev,
                             float *terms_dev, float *g_xyz, float *g_opacity, float *g_scales, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ---- avatar initialisation (soar_amd/body.py, csrc/body.hip): body-model vertices, subdivision, vertex normals, surfel frames.
 * soar_smplx_vertices: lbs() of the SMPL-X body model plus transl for B frames in one launch,
 *   v_shaped = v_template + shapedirs betas[b];  v_posed = v_shaped + (R[b, 1:] - I) posedirs;
 *   out[b, v] = (sum_j lbs_weights[v, j] joint_mats[b, j]) [v_posed, 1] + transl[b].
 * betas [betas_batch][NB] (betas_batch 1 or B), v_template [V][3], shapedirs [V][3][NB], posedirs [(J - 1) 9][V 3],
 * lbs_weights [V][J], full_pose [B][J 3] axis-angle, joint_mats [B][J][4][4] = soar_smplx_joint_mats of the same betas and
 * full_pose WITHOUT transl, transl [B][3] or NULL, out [B][V][3].  2 <= J <= 64.  Every sum has a fixed order that depends on
 * neither B nor the frame's place in the batch.  B = 0 or V = 0 with valid pointers succeeds without a launch. */
int soar_smplx_vertices(int32_t B, int32_t V, int32_t J, int32_t NB, const float *betas, int32_t betas_batch, const float *v_template,
                        const float *shapedirs, const float *posedirs, const float *lbs_weights, const float *full_pose,
                        const float *joint_mats, const float *transl, float *out, void *stream);
/* Midpoint subdivision of an index triangle mesh (open, non-manifold, unused vertices: all fine), one level per call pair.
 * soar_mesh_workspace_bytes: the workspace of a mesh of F faces (256-byte aligned), for the three mesh entry points below.
 * soar_mesh_subdivide_edges: sorts the 3 F edge keys (min << 32) | max, leaves the unique ones in the workspace and returns their
 *   number E (synchronises the stream).  A face naming a vertex outside [0, V) is refused.
 * soar_mesh_subdivide: with the workspace soar_mesh_subdivide_edges filled for the same faces, writes verts_out [V + E][3] (the
 *   old vertices, then one midpoint (a + b) * 0.5f per unique edge IN ASCENDING KEY ORDER) and faces_out [4 F][3]: the children of
 *   face f = (a, b, c) at rows 4 f .. 4 f + 3 are (a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca). */
int soar_mesh_workspace_bytes(int32_t F, size_t *bytes);
int soar_mesh_subdivide_edges(int32_t V, int32_t F, const int32_t *faces, void *workspace, size_t workspace_bytes, int64_t *edges_host,
                              void *stream);
int soar_mesh_subdivide(int32_t V, int32_t F, int64_t E, const float *verts, const int32_t *faces, const void *workspace,
                        size_t workspace_bytes, float *verts_out, int32_t *faces_out, void *stream);
/* Vertex normals [V][3]: normalize(sum over the vertex's face corners, in ascending (face, corner) order, of weight * unit face
 * normal), weight = the corner's interior angle, the face's area, or 1; normalize is x / max(|x|, 1e-12), so a vertex no face
 * uses gets (0, 0, 0).  No atomics: bit-reproducible.  Synchronises the stream once (the face indices are checked first). */
#define SOAR_NORMALS_ANGLE 0
#define SOAR_NORMALS_AREA 1
#define SOAR_NORMALS_UNIFORM 2
int soar_mesh_vertex_normals(int32_t V, int32_t F, const float *verts, const int32_t *faces, int32_t weighting, void *workspace,
                             size_t workspace_bytes, float *normals, void *stream);
/* Surfel frames: uz = normals[p], ux = normalize(uz x rand_dir[p]), uy = normalize(uz x ux), quats[p] = the quaternion (real part
 * first, non-negative, unit length) of the matrix with columns (ux, uy, uz)  (TS/utils/smpl.py:115-120). */
int soar_mesh_vertex_frames(int32_t P, const float *normals, const float *rand_dir, float *quats, void *stream);

/* ---- the training data module (soar_amd/data.py, csrc/data.hip): the video stays on the device as bytes; boxes and crops once,
 * a step's whole batch in one launch.  Restates TS/data/uncond_multiview.py:246-313 and :340-681 and threestudio's get_ray_directions,
 * get_rays, get_projection_matrix and get_mvp_matrix.  Every call checks its arguments before any launch.
 * soar_data_mask_bbox: boxes [N][4] = the inclusive (xmin, ymin, xmax, ymax) of the non-zero bytes of masks [N][H][W]; a frame without
 *   one gets (W, H, -1, -1).  One workgroup per frame, integer min / max only: deterministic.  N = 0 succeeds without a launch.
 * soar_data_crops: the 512 x 512 ImageDream crops of N frames from images [N][H][W][3], masks [N][H][W] (0 / 1) and the boxes ON THE
 *   DEVICE.  c = min + (max - min) / 2 in float32; s = max(xmax - xmin, ymax - ymin) * 1.1 in double, as the reference's Python
 *   number; box = c -+ (float)(s / 2).  Crop pixel (u, v) samples x = ((lin[u] / W * 2 - 1) + 1) * (W / 2) - 0.5 (the last
 *   multiply-subtract fused), y likewise, lin = torch.linspace(box.x0, box.x1, 512) in torch's own arithmetic (a fused start + step i
 *   below the middle, end - step (511 - i) from it on): the positions of F.grid_sample(align_corners=False) bit for bit.  Bilinear,
 *   zero padding; the RGB taps are byte / 255 * mask, the mask taps the mask.  rgb_crop [N][512][512][3], mask_crop [N][512][512].
 *   The sources are read as bytes: no scratch, whatever N.  A sentinel box gives a crop of zeros. */
#define SOAR_DATA_CROP 512
#define SOAR_DATA_MAX_VIEWS 8
#define SOAR_DATA_SMALL_FLOATS 256
int soar_data_mask_bbox(int32_t N, int32_t H, int32_t W, const uint8_t *masks, int32_t *boxes, void *stream);
int soar_data_crops(int32_t N, int32_t H, int32_t W, const uint8_t *images, const uint8_t *masks, const int32_t *boxes, float *rgb_crop,
                    float *mask_crop, void *stream);
/* soar_data_step_batch: ONE launch per training step.  The small inputs travel in the struct, by value, as soar_cameras_from_c2w takes
 * its host matrices: no copy, no synchronisation.  An output that is NULL is not written (and its inputs not read).
 *   random views (B <= 8, H x W):  cam_d [B][H][W][3] = ((i + .5 - W / 2) / focal[b], -(j + .5 - H / 2) / focal[b], -1);
 *     rays_d[r] = sum_k cam_d[k] c2w[b][r][k] in the order k = 0, 1, 2, then x / max(|x|, 1e-12) when rays_d_normalize.
 *     (rays_o is the translation column: the caller expands it from `small`.)
 *     proj [B][4][4]: [0][0] = 1 / (tan_half[b] aspect), [1][1] = -1 / tan_half[b], [2][2] = -(far + near) / (far - near),
 *     [2][3] = -2 far near / (far - near), [3][2] = -1;  mvp_mtx [B][4][4] = proj [R^T | -R^T t].
 *   the frame's own camera:  gt_cam_d [512][512][3] = ((i + .5 - cx) / fx, -(j + .5 - cy) / fy, -1) with fx, fy, cx, cy from
 *     normal_Ks [n_frames][3][3] on the device at row `frame`, gt_rays_d = the rotation by gt_c2w, always normalised;
 *     gt_mvp_mtx [4][4] with gt_near and, when gt_has_cxcy, [0][2] = -(2 cx - W) / W and [1][2] = -(2 cy - H) / H of the video image.
 *   the frame, gathered and converted:  gt_rgb [Hv][Wv][3] = byte / 255 * mask, gt_mask [Hv][Wv] = mask,
 *     gt_normal_F / _B [512][512][3] = byte / 255, gt_normal_mask [512][512] = byte / 255, gt_rgb_crop / gt_mask_crop = the rows of
 *     rgb_crop / mask_crop.  Streaming: 16-byte loads and stores (through LDS, so that neighbouring lanes store neighbouring 16 bytes)
 *     when Hv Wv is a multiple of 16, byte loads otherwise; the float outputs must be 16-byte aligned.
 *   small_out [n_small] = small[0 .. n_small): the step's per-camera vectors, as they are, for the caller to slice. */
typedef struct SoarDataStepArgs {
    int32_t B, H, W;               /* the random views */
    int32_t n_frames, Hv, Wv;      /* the stored video */
    int32_t frame;                 /* gt_index */
    int32_t rays_d_normalize, gt_has_cxcy, n_small;
    double near_plane, far_plane;  /* of the random views (0.1, 1000 in the reference: Python numbers, hence doubles) */
    double gt_near;                /* the frame's own near plane; its far plane is 1000 */
    float c2w[SOAR_DATA_MAX_VIEWS][16], focal[SOAR_DATA_MAX_VIEWS], tan_half[SOAR_DATA_MAX_VIEWS];
    float gt_c2w[16], gt_tan_half, gt_cx, gt_cy;
    float small[SOAR_DATA_SMALL_FLOATS];
    const uint8_t *images, *masks, *normal_F, *normal_B, *normal_mask;
    const float *rgb_crop, *mask_crop, *normal_Ks;
    float *rays_d, *cam_d, *gt_rays_d, *gt_cam_d;
    float *gt_rgb, *gt_mask, *gt_normal_F, *gt_normal_B, *gt_normal_mask, *gt_rgb_crop, *gt_mask_crop;
    float *mvp_mtx, *proj, *gt_mvp_mtx, *small_out;
} SoarDataStepArgs;
int soar_data_step_batch(const SoarDataStepArgs *args, void *stream);

/* ---- test-split evaluation (eval.hip, soar_amd/evaluate.py): the numbers of the reference's test_step
 * (TS/system/gaussian_surfel_mvdream.py:527-589), which takes them from skimage on the host.  Per image n, in one pass:
 *   gt_white = gt_mask > 0.5 ? gt_rgb : 1.0f;
 *   mse = sum over the 3 H W values of (double)(d * d), d = gt_white - pred and d * d in float32, / (3 H W);
 *   psnr = 10 log10(1 / mse) (data range 1; +inf when mse == 0);
 *   ssim = structural_similarity(pred, gt_white, channel_axis=-1, data_range=1): per channel, over the (H - 6)(W - 6) 7x7 windows
 *     wholly inside the image, in float64: u* = window sums of x, y, xx, yy, xy / 49, v = 49 / 48 (uxx - ux ux) (vy, vxy likewise),
 *     S = (2 ux uy + C1)(2 vxy + C2) / ((ux ux + uy uy + C1)(vx + vy + C2)), C1 = 1e-4, C2 = 9e-4; the mean of S over the windows,
 *     then over the channels;
 *   metrics[n] = {psnr, ssim, mse};  pred2 = pred * 2 - 1, gt2 = gt_white * 2 - 1 (the LPIPS inputs);
 *   grid (NULL = skip) [N][H][2 W][3] = pred | gt_white as bytes: clamp(v, 0, 1) * 255, truncated.
 * pred, gt_rgb [N][H][W][3] and gt_mask [N][H][W] are read at their element strides; gt_white, pred2, gt2 are contiguous [N][H][W][3].
 * No float atomics: every workgroup writes four float64 partial sums into `scratch` (soar_eval_scratch_bytes bytes, 256-byte aligned),
 * a second kernel of the same call adds them in a fixed order: two calls give the same bits.  No host synchronisation, no allocation.
 * Refused before any launch: H < 7 or W < 7 (no window fits; skimage raises too), N < 1, N > 65535, N H W > 2^30, a NULL pointer other
 * than grid, a short scratch. */
typedef struct SoarEvalArgs {
    int32_t N, H, W, pad_;
    const float *pred, *gt_rgb, *gt_mask;
    int64_t pred_stride[4], gt_stride[4];   /* elements, in the order N, H, W, channel */
    int64_t mask_stride[3];                 /* elements, N, H, W */
    float *gt_white, *pred2, *gt2;
    uint8_t *grid;                          /* or NULL */
    double *metrics;                        /* [N][3] */
} SoarEvalArgs;
int soar_eval_scratch_bytes(int32_t N, int32_t H, int32_t W, size_t *bytes);
int soar_eval_image_metrics(const SoarEvalArgs *args, void *scratch, size_t scratch_bytes, void *stream);

/* ---- avatar playback (playback.hip, soar_amd/playback.py): what the reference's inference harness
 * (TS/test/render_rot.py) does on the host per frame, either side of the renderer.  Both calls: the caller's stream, no allocation,
 * no host synchronisation; compiled without FMA contraction and restated operation by operation in tests/playback_ref.py.
 *
 * soar_motion_resample: K key poses sampled at F times, one thread per (frame, joint), one launch.
 *   key_pose [K][55][3] axis-angle (full_pose order), key_transl [K][3], key_expr [K][E]; t [F] in key units, clamped to [0, K - 1];
 *   yaw [F] radians or NULL;  pose [F][55][3], transl [F][3], expr [F][E].
 *   tc = clamp(t), i0 = floor(tc), i1 = min(i0 + 1, K - 1), u = tc - i0.  Per joint:
 *     q(a) = (cos(|a| / 2), s a), s = sin(|a| / 2) / |a|, or 1/2 - |a|^2 / 48 when |a| < 1e-3;
 *     dot = q0 . q1; dot < 0: q1 = -q1, dot = -dot;  dot > 0.999999: weights (1 - u, u) (normalised lerp), else with
 *     th = acos(dot): (sin((1 - u) th), sin(u th)) / sin(th);  q = the weighted sum, divided by its length;
 *     joint 0 with yaw: q = q (x) (cos(yaw / 2), 0, sin(yaw / 2), 0), i.e. R <- R Ry(yaw) (euler2mat(yaw, 0, 0, "syxz"));
 *     w < 0: q = -q;  n = |(x, y, z)|;  out = k (x, y, z), k = 2 atan2(n, w) / n, or 2 + n^2 / 3 when n < 1e-3: angle in [0, pi].
 *   u == 0 and no turn: the key's three floats are copied as they are (so is a value of transl / expr at u == 0);
 *   transl, expr otherwise = (1 - u) v[i0] + u v[i1]. */
int soar_motion_resample(int32_t K, int32_t F, int32_t E, const float *key_pose, const float *key_transl, const float *key_expr,
                         const float *t, const float *yaw, float *pose, float *transl, float *expr, void *stream);

/* soar_playback_finish: B rendered frames -> the byte images render_rot.py saves, one launch, every pixel's 10 floats read once.
 *   render, normal, occ: per frame [3][H][W], mask [H][W], float32, frame b at base + b * stride (floats; the planes of a frame are
 *   contiguous); occ may be NULL (occ_out is not written then).
 *   rgb, normal_out, occ_out [B][H][W][4] = (the three channels, the mask), mask_out [B][H][W], uint8, contiguous.
 *   byte(x) = (uint8) clamp(x * 255 + 0.5, 0, 255): multiply, add (no FMA), clamp, truncate -- torchvision's save_image; NaN -> 0.
 *   normal_as_rgb != 0: the normal is n * 0.5 + 0.5 first.
 *   Any H, W >= 1: 16-byte accesses when H W and the strides are multiples of 4 and the bases 16-byte aligned, 4-byte ones otherwise
 *   (the float inputs and RGBA outputs must be 4-byte aligned); nothing is read or written behind a frame's last pixel.
 *   B <= 65535, B H W <= 2^30; B == 0 is a no-op. */
typedef struct SoarPlaybackArgs {
    int32_t B, H, W, normal_as_rgb;
    const float *render, *normal, *mask, *occ;
    int64_t render_stride, normal_stride, mask_stride, occ_stride;
    uint8_t *rgb, *normal_out, *occ_out, *mask_out;
} SoarPlaybackArgs;
int soar_playback_finish(const SoarPlaybackArgs *args, void *stream);

/* ---- normal-map preprocessing (normalnet.hip, normal_io.hip, soar_amd/normals.py) ----
 * Two generators of one architecture, netF on cat(image, prior_F) and netB on cat(image, prior_B) (6 input channels), inference only:
 *   reflection pad 3, conv 7x7 6 -> ngf, IN, ReLU;  n_down x (conv 3x3 stride 2 zero pad 1, c -> 2c, IN, ReLU);
 *   n_blocks x (x + IN(conv3x3(rpad1(ReLU(IN(conv3x3(rpad1(x))))))))  at ngf 2^n_down channels (rpad1: reflection pad 1);
 *   n_down x (transposed conv 3x3 stride 2 pad 1 output_padding 1, c -> c / 2, IN, ReLU);  reflection pad 3, conv 7x7 ngf -> 3 + bias, tanh.
 *   IN: InstanceNorm without affine parameters, eps 1e-5, biased variance over H x W per image and channel (sums in double, one
 *   fixed order).  The biases of the convolutions in front of an IN cancel in it and are not part of the packed weights.
 *   Head: n / |n|_2 over the three channels where sum_c |image_c| != 0, exactly 0 elsewhere.
 * soar_normalnet_pack_weights packs ONE generator (soar_normalnet_weights_bytes bytes, 256-byte aligned) from `count` contiguous device
 *   arrays in torch's layouts, in this order: first [ngf][6][7][7]; n_down x down [2c][c][3][3]; 2 n_blocks x trunk [C][C][3][3] (a
 *   block's first, then its second); n_down x up [c][c/2][3][3] (ConvTranspose2d: [Cin][Cout]); last [3][ngf][7][7]; last bias [3].
 *   count = 2 n_down + 2 n_blocks + 3.
 * soar_normalnet_forward evaluates both generators; image / prior_F / prior_B [N][3][H][W] float32 at their element strides (NCHW
 *   order), normal_F / normal_B [N][3][H][W] contiguous.  Workspace: soar_normalnet_workspace_bytes, 256-byte aligned, the caller's.
 *   ngf: a multiple of 8, at most 512 (8192 trunk channels: the kernels' channel and K indices are int); n_down 1 .. 4; n_blocks >= 0;
 *   H, W multiples of 2^n_down, >= 4, >= 2 at the bottom level; 0 <= N <= 65535 (0 launches nothing; the image is a grid dimension);
 *   N H W <= 2^30.  Anything else is refused before any launch.  No atomics, no host synchronisation,
 *   no allocation; a batch of N gives the bits of N single calls. */
typedef struct SoarNormalNetArgs {
    int32_t N, H, W;
    int32_t ngf, n_down, n_blocks;
    const float *image, *prior_F, *prior_B;
    int64_t image_stride[4], prior_F_stride[4], prior_B_stride[4];
    const void *weights_F, *weights_B;       /* soar_normalnet_pack_weights' outputs */
    float *normal_F, *normal_B;
} SoarNormalNetArgs;
int soar_normalnet_weights_bytes(int32_t ngf, int32_t n_down, int32_t n_blocks, size_t *bytes);
int soar_normalnet_pack_weights(int32_t ngf, int32_t n_down, int32_t n_blocks, const float *const *tensors, int32_t count, void *packed,
                                size_t packed_bytes, void *stream);
int soar_normalnet_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t ngf, int32_t n_down, int32_t n_blocks, size_t *bytes);
int soar_normalnet_forward(const SoarNormalNetArgs *args, void *workspace, size_t workspace_bytes, void *stream);

/* The crop in front of the networks and the byte images behind them.  images [N][H][W][3] and mask [N][H][W] are uint8 at their byte
 * strides ((n, y, x, c) and (n, y, x): an RGBA array serves as both); a mask byte counts as m / 255.
 * soar_normal_crop_boxes, one launch for all frames: (x0, y0, x1, y1) = the inclusive bounding box of the non-zero mask bytes;
 *   c = (x0 + (x1 - x0) / 2, y0 + (y1 - y0) / 2), half = 1.1 max(x1 - x0, y1 - y0) / 2, boxes[n] = (c - half, c + half) in double;
 *   normal_Ks[n] = [[S fx / (bx2 - bx1), 0, S (cx - bx1) / (bx2 - bx1)], [0, S fy / (by2 - by1), S (cy - by1) / (by2 - by1)], [0, 0, 1]]
 *   from Ks[n] [3][3]; status[n] = 0, 1 (empty mask: the whole frame stands in as the box) or 2 (the mask is a single pixel).  Nothing
 *   is read back: the caller looks at status where it next synchronises.
 * soar_normal_crop_sample, one launch for all frames: sample (jy, jx) of the S x S crop sits at pixel coordinate
 *   x = bx1 + (bx2 - bx1) jx / (S - 1), likewise y, and is the bilinear sample at (x - 1/2, y - 1/2) (grid-sample arithmetic with
 *   align_corners = False), zeros outside the frame, of (rgb / 255 * 2 - 1) * m -> out_image [N][3][S][S] and of m -> out_mask
 *   [N][S][S]; evaluated in double, rounded once.
 * soar_normal_crop_bytes, one launch: out_F / out_B [N][H][W][3] = trunc(((n + 1) / 2 * mask) * 255), out_mask [N][H][W] =
 *   trunc(mask * 255), float32 operations in that order without contraction; normal_F / normal_B [N][3][H][W], mask [N][H][W]. */
int soar_normal_crop_boxes(int32_t N, int32_t H, int32_t W, int32_t S, const uint8_t *mask, const int64_t *mask_stride, const float *Ks,
                           double *boxes, float *normal_Ks, int32_t *status, void *stream);
int soar_normal_crop_sample(int32_t N, int32_t H, int32_t W, int32_t S, const uint8_t *images, const int64_t *image_stride,
                            const uint8_t *mask, const int64_t *mask_stride, const double *boxes, float *out_image, float *out_mask,
                            void *stream);
int soar_normal_crop_bytes(int32_t N, int32_t H, int32_t W, const float *normal_F, const float *normal_B, const float *mask,
                           uint8_t *out_F, uint8_t *out_B, uint8_t *out_mask, void *stream);

/* ---- SMPL-X keypoint fitting (smplify.hip, soar_amd/smplify.py) ----
 * The SMPLify objective of the reference's preprocessing (preproc/utils.py:626-685) and the gradient of its sum, for N frames.
 * SoarSmplifyRig: the part of the body model the objective reads.  J = 55 joints in SMPL-X order (global, 21 body, jaw, two eyes,
 *   15 + 15 hand joints; parents[j] < j, parents[0] < 0); NB = NBS + NE shape and expression directions (<= 64); VS gathered
 *   vertices (<= 256); P model points (<= 160), each either a joint (pt_kind 0, pt_idx[p][0] = joint) or a weighted sum of up to
 *   three gathered vertices (pt_kind 1: a selected vertex with weights (1, 0, 0), a landmark with its barycentric coordinates),
 *   written to keypoint pt_dst[p] of 137.  Every pointer is device memory; the indices are the caller's to check
 *   (soar_amd.smplify.KeypointRig does, on the host): the kernels trust them.
 * SoarSmplifyArgs: rotations of the optimised joints as 6-D vectors (two rows, Gram-Schmidt), jaw and eyes as rotation vectors;
 *   *0 are the initial values of the preserve term.  kp_scale = w_kp / (NF 137 2), pose_scale[k] = w_preserve / (NF J_k),
 *   row_scale = w_preserve / NF, smooth_scale[k] = w_smooth / ((N - 1) J_k) (0 for N = 1), NF: the frame count the means divide by.
 *   Outputs: g_* the gradient of the sum of the three losses ([N][1|21|15|15][6], [NBS], [N][3]), loss[3] = (kp, preserve,
 *   smooth), weighted; kps [N][137][2] the projected keypoints or NULL.  Scratch: frame_betas [N][NBS], frame_loss [N][2].
 * soar_smplify_objective: two launches -- one workgroup per frame for the forward and the adjoint of the per-frame part, then one
 *   workgroup for the smooth term (a thread per (frame, joint) reads both neighbours) and the sums over frames in a fixed order.
 *   No atomics, no host synchronisation, no allocation; two calls give the same bits, and a frame's keypoint and preserve
 *   gradients depend neither on N nor on its place (for a given NF).  grads = 0: only loss[0] and kps are computed (one launch).
 * soar_smplify_target_scales: per frame the larger side of the bounding box of the keypoints (x img_w, y img_h, confidence)
 *   [N][137][3] with confidence above 0.3; -1 for a frame that has none. */
typedef struct SoarSmplifyRig {
    int32_t J, NBS, NE, VS, P, pad_;
    const float *J_template;      /* [J][3]      J_regressor v_template */
    const float *J_dirs;          /* [J][3][NB]  J_regressor shapedirs */
    const int32_t *parents;       /* [J] */
    const float *v_template;      /* [VS][3] */
    const float *shapedirs;       /* [VS][3][NB] */
    const float *posedirs;        /* [(J - 1) 9][VS 3] */
    const float *lbs_weights;     /* [VS][J] */
    const int32_t *pt_kind;       /* [P] */
    const int32_t *pt_idx;        /* [P][3] */
    const float *pt_w;            /* [P][3] */
    const int32_t *pt_dst;        /* [P], distinct, in [0, 137) */
    const float *kp_mask;         /* [137] */
} SoarSmplifyRig;
typedef struct SoarSmplifyArgs {
    int32_t N, ignore_hands, grads, pad_;
    const float *global_orient, *body_pose, *left_hand_pose, *right_hand_pose, *betas, *transl, *jaw_pose, *leye_pose, *reye_pose,
        *expression;
    const float *global_orient0, *body_pose0, *left_hand_pose0, *right_hand_pose0, *betas0, *transl0, *jaw_pose0, *leye_pose0,
        *reye_pose0, *expression0;
    const float *Ks;              /* [N][3][3] */
    const float *w2c;             /* [4][4], rows 0 .. 2 are read */
    const float *target_kps;      /* [N][137][3]: x / img_w, y / img_h, confidence */
    const float *target_scales;   /* [N] */
    float img_w, img_h, sigma, kp_scale, pose_scale[4], row_scale, w_preserve, smooth_scale[4];
    float *g_global_orient, *g_body_pose, *g_left_hand_pose, *g_right_hand_pose, *g_betas, *g_transl, *loss, *kps;
    float *frame_betas, *frame_loss;
} SoarSmplifyArgs;
int soar_smplify_objective(const SoarSmplifyRig *rig, const SoarSmplifyArgs *args, void *stream);
/* SoarSmplifyBody, soar_smplify_objective_body: the same objective for the body model the reference creates (use_face_contour=True,
 *   flat_hand_mean=False).  The rig's gathered arrays (v_template, shapedirs, posedirs, lbs_weights) then hold VU rows: the rig's
 *   VS static rows first, then the vertices of all 79 rows of the contour table (any count: only a frame's active set, VS +
 *   3 L_dyn <= 256 slots, is held on chip; posedirs rows are VU 3 long).  Per frame the row is chosen from R = the world rotation of
 *   joint `neck` (root ... neck, pose mean included): e = atan2(-R[2][0], sqrt(R[0][0]^2 + R[1][0]^2)), y = rint(min(-e 180/pi,
 *   39)) (half to even), row = y if y >= 0, 78 if y < -39, else 39 - y.  Contour landmark l then is sum_k dyn_bary[row][l][k] x vertex
 *   row dyn_vrow[row][l][k], and replaces the weights and indices of model point dyn_point[l] (a pt_kind 1 entry of the rig; -1: the
 *   landmark feeds no keypoint).  The row is not differentiated.  rows_out [N] int32 or NULL receives the rows (written only with L_dyn > 0).
 *   pose_mean [55][3]: joint j with bit j of mean_mask set enters the body model as rodrigues(log(R_j) + mean_j) (optimised joints;
 *   log by the axial vector and atan2, a series below |a| = 1e-3, specified for angles up to 3.0 rad) or rodrigues(v_j + mean_j)
 *   (jaw, eyes); the other joints take the direct path.  The preserve and smooth terms are unchanged.  L_dyn = 0 and mean_mask = 0
 *   runs soar_smplify_objective itself.  Refuses N <= 0.  Same launches, same no-atomics guarantees as soar_smplify_objective. */
typedef struct SoarSmplifyBody {
    int32_t L_dyn, n_rows, neck, VU;   /* contour landmarks (<= 17, 0: none), table rows (79), the neck joint, gathered rows */
    const int32_t *dyn_vrow;      /* [79][L_dyn][3] rows of the gathered arrays, in [0, VU) */
    const float *dyn_bary;        /* [79][L_dyn][3] */
    const int32_t *dyn_point;     /* [L_dyn] model point in [0, P) or -1 */
    const float *pose_mean;       /* [55][3] or NULL with mean_mask = 0 */
    uint64_t mean_mask;
    int32_t *rows_out;            /* [N] or NULL */
} SoarSmplifyBody;
int soar_smplify_objective_body(const SoarSmplifyRig *rig, const SoarSmplifyBody *body, const SoarSmplifyArgs *args, void *stream);
int soar_smplify_target_scales(int32_t N, const float *target_kps, float img_w, float img_h, float *scales, void *stream);
/* The rig's static model points alone, forward only, one launch (a workgroup per frame): points [N][PA][3] float32, the 55 posed
 *   joints (point p < 55 is joint p), then the selected vertices and the static landmarks as sum_k mp_w[p][k] x gathered row
 *   mp_idx[p][k] (mp_idx in [0, VS), the caller's to check; rows p < 55 of both tables are not read), plus transl: what the objective
 *   computes before the OpenPose conversion and the camera, for all PA >= 55 points and not only the P mapped ones.  Of args the ten
 *   parameter pointers and N are read.  body = NULL: the static rig.  Otherwise VU gives the posedirs row length and
 *   mean_mask / pose_mean the pose mean; the contour table is not read: a rig with one returns its static points only.
 *   Refuses N <= 0.  No atomics; two calls give the same bits; the objective's kernels are untouched by it. */
int soar_smplify_model_points(const SoarSmplifyRig *rig, const SoarSmplifyBody *body, const SoarSmplifyArgs *args, int32_t PA,
                              const int32_t *mp_idx, const float *mp_w, float *points, void *stream);

/* ---- SMPL-X initialisation from keypoints alone (pose_init.hip, soar_amd/pose_init.py) ----
 * Stands in for the reference's SMPLer-X call and is a different algorithm: a bank of pose hypotheses, a closed-form camera
 * translation per hypothesis, the fit's keypoint term as the score, a shortest path through the frames.  The bank, the intrinsics
 * rule and the defaults are this project's definitions, not tuned on real video, and were compared neither with SMPLer-X nor with
 * the licensed SMPL-X model.
 * soar_pose_init_search, one launch (a workgroup per frame, a wavefront per state): state s = b H + h is base pose b turned by
 *   rotations[h] about pivot[b]: X = R_h (points0[b] - pivot[b]) + pivot[b]; then convert_kps by src_inds / dst_inds (an entry with
 *   src_inds >= PA is a contour landmark: its keypoint stays 0 and gets weight 0), Yc = R_w2c Y.  Weights c_k = confidence_k
 *   kp_mask[k], 0 for rows 25 .. 66 (the hands), for confidence_k < conf_min and for contour keypoints.  With (a_k, b_k, 1) =
 *   K^-1 (u_k, v_k, 1) (K upper triangular, skew honoured) the camera-space t' minimises sum_k c_k [(Yc_x + t'_x - a_k (Yc_z + t'_z))^2
 *   + (Yc_y + t'_y - b_k (Yc_z + t'_z))^2]: seven weighted sums and a closed-form 3 x 3 solve in double.  transl = R_w2c^T (t' - t_w2c).
 *   A state is invalid (cost +inf, transl 0) when fewer than min_points weights are positive, the determinant is not positive, or the
 *   smallest depth Yc_z + t'_z over the weighted keypoints is below z_min.  cost = sum_k c_k (gmof(e_kx) + gmof(e_ky)), e = (projection
 *   - target pixel) / scales[n] * 200, divisor max(z, 1e-5): the fit's keypoint term of the frame without the mean and the weight.
 *   valid[n] = 1 when any state of frame n is finite.  No atomics; a frame's outputs are the same bits alone, in any batch, in any
 *   order; nothing is read back.  Refuses N <= 0 and S = B H > 1024.
 * soar_pose_init_viterbi, one launch of one workgroup, S <= 1024: D[0] = U[0], D[n][s] = (min_s' (D[n-1][s'] + T[s'][s])) + U[n][s] in
 *   float32 in that order of additions; ties to the lowest s', the final minimum to the lowest s; a unary row that is all +inf
 *   counts as zeros.  backptr [N][S] int32 is the caller's scratch.  path [N] int64, total [1].  With transl [N][S][3], valid [N] and
 *   transl_path [N][3] (all three or none): the path's translations, linearly interpolated between the nearest valid frames on
 *   either side of a frame that is not valid, held at the ends, 0 when no frame is valid. */
typedef struct SoarPoseSearch {
    int32_t N, B, H, PA, P, min_points;
    const float *points0;         /* [B][PA][3] */
    const float *pivot;           /* [B][3] */
    const float *rotations;       /* [H][3][3] */
    const int32_t *src_inds;      /* [P] model point; >= PA: a contour landmark */
    const int32_t *dst_inds;      /* [P] distinct, in [0, 137) */
    const float *kp_mask;         /* [137] */
    const float *target_kps;      /* [N][137][3]: x / img_w, y / img_h, confidence */
    const float *Ks;              /* [N][3][3] */
    const float *w2c;             /* [4][4], rows 0 .. 2 are read */
    const float *scales;          /* [N] */
    float img_w, img_h, sigma, conf_min, z_min, pad_;
    float *cost;                  /* [N][B H] */
    float *transl;                /* [N][B H][3] */
    uint8_t *valid;               /* [N] */
} SoarPoseSearch;
int soar_pose_init_search(const SoarPoseSearch *args, void *stream);
int soar_pose_init_viterbi(int32_t N, int32_t S, const float *unary, const float *trans, int32_t *backptr, int64_t *path, float *total,
                           const float *transl, const uint8_t *valid, float *transl_path, void *stream);

/* ---- SMPL-X normal priors: an indexed triangle mesh drawn as a normal map (prior.hip, soar_amd/prior.py) ----
 * N frames of one topology: faces [F][3] (indices in [0, V): the caller's to check, soar_amd.prior.MeshTopology does, on the host)
 * and the vertex-to-corner table csr_offsets [V + 1], csr_corners [3 F] (3 face + corner of every corner that names the vertex,
 * ascending).  Every pointer is device memory but verts_stride (host, three element strides of verts [N][V][3]).
 * soar_prior_vertex_setup, one launch: per (frame, vertex) p = R v + t from w2c ([4][4], or [N][4][4] with w2c_per_frame != 0;
 *   rows 0 .. 2 are read), x = fx p.x / p.z + cx, y = fy p.y / p.z + cy with Ks [N][3][3] in un-contracted float32,
 *   snapped [N][V][2] = rint(256 (x, y)), inv_z [N][V] = 1 / p.z, normals [N][V][3] = R normalize(sum of the un-normalised cross
 *   products (v1 - v0) x (v2 - v0) of the vertex's faces), normalize(x) = x / max(|x|, 1e-12).  A vertex with p.z <= 1e-6 or more
 *   than 2^20 pixels from the origin has snapped = (INT32_MIN, INT32_MIN) and inv_z = 0.
 * soar_prior_face_boxes, one launch: boxes [N][F][4] int16 = the first and last pixel column and the first and last row whose sample
 *   (256 j + 128) lies inside the face's snapped bounding box, clamped to int16; (32767, -32768, 32767, -32768) for a face with an
 *   invalid vertex, of zero snapped area, or whose box holds no sample.  8 bytes a face instead of three indices and three vertices:
 *   what every tile of the raster launch reads of every face.
 * soar_prior_raster, one launch: both views of every frame from those arrays.  Pixel (i, j) is sampled at snapped
 *   (256 j + 128, 256 i + 128); exact int64 edge functions, ties on an edge by the edge's direction (towards +y, or along +x, owns
 *   it, on the face with vertices 1 and 2 swapped when its snapped area is negative); no culling; a face with an invalid vertex or
 *   of zero snapped area covers nothing.  b_k = float(e_k) / float(A), q = sum b_k inv_z_k; view 0 keeps the largest q, view 1 the
 *   smallest, the smaller face index among equal q.  prior [N][2][3][H][W] = normalize(sum (b_k inv_z_k) n_k), as (x, -y, -z) when
 *   opengl != 0, exactly 0 off the mesh; mask [N][2][H][W] 1 / 0; face [N][2][H][W] the winner or -1.  H, W <= 4096.
 * No float atomics, no host synchronisation, no allocation; the output does not depend on the order of execution, and a frame's
 * output depends neither on N nor on its place. */
int soar_prior_vertex_setup(int32_t N, int32_t V, int32_t F, const float *verts, const int64_t *verts_stride, const float *w2c,
                            int32_t w2c_per_frame, const float *Ks, const int32_t *faces, const int32_t *csr_offsets,
                            const int32_t *csr_corners, int32_t *snapped, float *inv_z, float *normals, void *stream);
int soar_prior_face_boxes(int32_t N, int32_t V, int32_t F, const int32_t *faces, const int32_t *snapped, int16_t *boxes, void *stream);
int soar_prior_raster(int32_t N, int32_t V, int32_t F, int32_t H, int32_t W, int32_t opengl, const int32_t *faces, const int32_t *snapped,
                      const float *inv_z, const float *normals, const int16_t *boxes, float *prior, uint8_t *mask, int32_t *face,
                      void *stream);

/* ---- mask clean-up: union of the segmenter's candidates, 5 x 5 open / close, largest component (masks.hip, soar_amd/masks.py;
 * DESIGN.md 9o) ----
 * N frames per call.  cand [N][K][H][W], K >= 1, contiguous: dtype 0 = uint8 / bool (non-zero is set), dtype 1 = float32
 * (value > threshold is set: 0.0, -0.0 and NaN are unset at threshold 0).  A pixel of the union is set where any candidate is.
 * OPEN (erode, dilate) then CLOSE (dilate, erode) with the 5 x 5 all-ones element, centre anchor, one iteration; an erosion reads
 * positions outside the image as set, a dilation as unset (OpenCV's default border value), each operation on its own input.
 * The largest component: 8-connectivity; a component's label is the smallest raster index y W + x of its pixels; the largest area
 * wins, the smallest label among equal areas.  out [N][H][W] uint8 in {0, 1}.  stats [N][4] int32 = union_area, cleaned_area,
 * n_components, kept_area (soar_masks_open_close leaves the last two 0; soar_masks_largest_component gives the input's area in the
 * first two).  A frame whose cleaned mask is empty gives zeros and n_components = 0.
 * soar_masks_open_close: the union, the four operations and the popcounts in one launch, one launch for the bytes.
 * soar_masks_largest_component: mask [N][H][W] uint8 (non-zero is set) -> pack, six launches of labelling and selection.
 * soar_masks_clean: both; the cleaned bit-plane stays in the workspace.  Seven launches and two memsets whatever the images hold.
 * Integer arithmetic and integer atomics only: two calls give the same bits.  No host synchronisation, no allocation; the
 * workspace (soar_masks_workspace_bytes, 256-byte aligned) is 4 bytes a pixel plus a bit a pixel.  H W < 2^31, N <= 65535. */
int soar_masks_workspace_bytes(int32_t N, int32_t H, int32_t W, size_t *bytes);
int soar_masks_open_close(int32_t N, int32_t K, int32_t H, int32_t W, const void *cand, int32_t dtype, float threshold, uint8_t *out,
                          int32_t *stats, void *workspace, size_t workspace_bytes, void *stream);
int soar_masks_largest_component(int32_t N, int32_t H, int32_t W, const uint8_t *mask, uint8_t *out, int32_t *stats, void *workspace,
                                 size_t workspace_bytes, void *stream);
int soar_masks_clean(int32_t N, int32_t K, int32_t H, int32_t W, const void *cand, int32_t dtype, float threshold, uint8_t *out,
                     int32_t *stats, void *workspace, size_t workspace_bytes, void *stream);

/* ---- the training step's remaining image terms (step_terms.hip, soar_amd/step_losses.py) ----
 * Current stream, no synchronisation, no read-back, no atomics: two calls give the same bits.  Every image is planar float32 and
 * 4-byte aligned; 16-byte accesses where the planes allow them, under the rule of soar_cos_loss / soar_masked_l1, whose values and
 * gradients these have bit for bit on the same images.  scratch: soar_step_terms_scratch_bytes() bytes, 8-byte aligned.
 *
 * soar_consistency_loss: cos_loss(a, b, mask = None, thrsh, weight) view by view over B <= 8 views [3,H,W] that lie a_stride /
 *   b_stride floats apart (>= 3 H W): stats [B][2] = {mean of 1 - cos over the view's selected pixels (NaN when none), their
 *   count}.  One launch and a finishing launch.  The backward gives BOTH gradients [B][3][H][W] in one launch: of a with b's
 *   values and of b with a's, each scaled by upstream_dev[view] / max(count, 1).  H W <= 2^28. */
int soar_step_terms_scratch_bytes(size_t *bytes);
int soar_consistency_loss(int32_t B, int32_t H, int32_t W, const float *a, int64_t a_stride, const float *b, int64_t b_stride,
                          float cos_thrsh, float weight, float *stats, float *scratch, void *stream);
int soar_consistency_loss_backward(int32_t B, int32_t H, int32_t W, const float *a, int64_t a_stride, const float *b, int64_t b_stride,
                                   float cos_thrsh, float weight, const float *stats, const float *upstream_dev, float *dL_da,
                                   float *dL_db, void *stream);
/* soar_normal_view_terms: the front and back normal views of the video frame (TS/system/gaussian_surfel_mvdream.py:332-399).
 *   normal: `views` (1: front only, 2) rendered views [3,R,R], normal_stride floats apart; mask0 [R,R] the front view's mask image;
 *   gt_F, gt_B [3,R,R] (gt_B NULL with views = 1); gt_mask [R,R] float.  sel = gt_mask > 1e-5.
 *   mode 1: values [3] = {0.2 cos_loss(view 0, gt_F, sel, 0), 0.2 cos_loss(view 1, gt_B, sel, 0), mean|mask0 - gt_mask|}, stats [6] the
 *   three {loss, count} pairs behind them, lpips_in [2 views][3][R][R] (16-byte aligned) = ((x * m) - 0.5) * 2 of the rendered views,
 *   then of the targets: m is the float gt_mask for the front view and (float)sel for the back view, as the reference has it.
 *   mode 2 (after mode 1, same stats): g_normal [views][3][R][R] = up[v] times the 0.2 cos term's gradient + (g_lpips * 2) * m
 *   (g_lpips [views][3][R][R], the upstream of the rendered views' LPIPS inputs, or NULL); g_mask0 [R,R] = up[2] times the L1
 *   term's.  up [3]: device.  One launch (mode 1: and a finishing launch).  R R <= 2^28. */
typedef struct SoarNormalViewArgs {
    int32_t R, views;
    const float *normal;
    int64_t normal_stride;
    const float *mask0, *gt_F, *gt_B, *gt_mask;
    float *values, *stats, *lpips_in, *scratch;
    const float *up, *g_lpips;
    float *g_normal, *g_mask0;
} SoarNormalViewArgs;
int soar_normal_view_terms(const SoarNormalViewArgs *args, int32_t mode, void *stream);
/* soar_frame_extra_terms: occ [3,H,W] planes, gt_mask [H,W]; gt_rgb and rand_bg through element strides {channel, pixel} (any
 *   layout whose rows follow each other: interleaved, planar, a broadcast colour with pixel stride 0).
 *   stats [2] = {mean of 1 - occ over the three channels of the pixels with gt_mask > 0 (float64 sums; NaN when none), the number of
 *   those elements}; blended [3,H,W] = gt_rgb * m + rand_bg * (1 - m), each operation rounded once.
 *   The backward: g_occ [3,H,W] = -(up[0] / stats[1]) at the selected pixels, 0 elsewhere.  H W <= 2^28.
 * soar_abs_mean: stats [2] = {mean|x| (float64 sums), n}; the backward: sign(x) * (upstream / n), sign(0) = 0.  n <= 2^30. */
typedef struct SoarFrameExtraArgs {
    int32_t H, W;
    const float *occ, *gt_rgb, *gt_mask, *rand_bg;
    int64_t rgb_stride[2], bg_stride[2];
    float *stats, *blended;
    void *scratch;
    const float *up;
    float *g_occ;
} SoarFrameExtraArgs;
int soar_frame_extra_terms(const SoarFrameExtraArgs *args, void *stream);
int soar_frame_extra_terms_backward(const SoarFrameExtraArgs *args, void *stream);
int soar_abs_mean(int64_t n, const float *x, float *stats, void *scratch, void *stream);
int soar_abs_mean_backward(int64_t n, const float *x, const float *upstream_dev, float *dL_dx, void *stream);

/* ---- SMPLify fit inspection: keypoint and body-normal strips (fitviz.hip, soar_amd/fitviz.py) ----
 * Current stream, no synchronisation, no allocation, no atomics; integer and un-contracted float32 arithmetic: two calls give the
 * same bits, and a frame's output depends neither on N nor on its place.  Every pointer is device memory but verts_stride (host).
 * N == 0 returns 0 without touching a pointer.
 *
 * soar_fitviz_yaw_views: verts [N][V][3] through three element strides, pivot [N][3], R [n_views - 1][3][3] ->
 *   out [N][n_views][V][3].  View 0 is verts, bit for bit.  View k >= 1: d = v - p, and component i is
 *   ((R[k-1][i][0] d0 + R[k-1][i][1] d1) + R[k-1][i][2] d2) + p_i, every operation rounded once.  1 <= n_views <= 16.
 *
 * soar_fitviz_strip: per frame a strip [H][5 W][3] uint8 of five panels H x W (or, with half != 0, [H / 2][(5 W) / 2][3]).
 *   Keypoints: target_px, fit_px [N][K][2] float32 pixels (x, y); kp_mask [K] uint8.  The centre of keypoint k is
 *   ((int)x, (int)y), truncated toward zero, and is drawn iff kp_mask[k] != 0, both coordinates are finite with |coord| < 2^20,
 *   and both integers are >= 1.  A disc covers pixel p iff dx dx + dy dy <= r r + 1 (r = radius, 1 .. 8).
 *   Limbs: limbs [L][2] int32 keypoint indices (a, b) with limb_rgb [L][3]; a limb is drawn in a set iff both of its keypoints
 *   are drawn in that set (an index outside [0, K) draws nothing).  With d = b - a, L2 = d . d, s = (p - a) . d, exact in integers:
 *   if 0 < s < L2, p is covered iff 4 cross(p - a, d)^2 <= t^2 L2; else iff 4 |p - e|^2 <= t^2, e = a when s <= 0 and b otherwise
 *   (t = thickness, 1 .. 64; a limb of length 0 is its end test).
 *   Panel 0: black; then, the last writer winning, the target set's limbs, its discs (target_rgb), the fit set's limbs, its discs
 *   (fit_rgb); limbs in the order of the table, discs in the order of the keypoints.  Drawing is clipped to the panel.  With imgs
 *   ([N][H][W][3] uint8 through four element strides; or NULL) every channel becomes rint(0.6f c + 0.4f img): two float32
 *   products, one float32 sum, half to even, clamped to 0 .. 255.
 *   Panels 2, 3, 4: yaw views 0, 1, 2 of prior [N][3][2][3][H][W] / mask [N][3][2][H][W] (soar_prior_raster's outputs for the 3 N
 *   bodies of soar_fitviz_yaw_views; only the front view, index 0 of the axis of 2, is read): where mask != 0 channel c is
 *   (uint8)((n_c * 0.5f + 0.5f) * 255.0f), clamped to 0 .. 255 and truncated; 0 elsewhere.
 *   Panel 1: panel 2 blended with imgs by the rule of panel 0; panel 2 itself without imgs.
 *   half: output pixel (i, j) is (a + b + c + d + 2) >> 2, per channel, of the full strip's pixels (2 i .. 2 i + 1, 2 j .. 2 j + 1);
 *   an odd last row or column of the full strip is dropped.  H, W <= 4096, K <= 512, L <= 512, N <= 65535.
 *
 * soar_fitviz_residuals: fit_px, target_px [N][K][2], conf [N][K], kp_mask [K] -> out [N][3] float32 = {count, mean, max} over
 *   the keypoints with kp_mask != 0, conf > thresh and four finite coordinates, of dist = sqrtf(dx dx + dy dy) (float32, every
 *   operation rounded once).  A keypoint outside the selection enters as 0.  Lane l of 64 adds its keypoints l, l + 64, ... in that
 *   order, then six butterfly steps x[l] += x[l ^ off], off = 32, 16, ..., 1; mean = sum / (float)count; a frame with none
 *   gives 0, 0, 0.  K <= 512. */
typedef struct SoarFitvizStripArgs {
    int32_t N, H, W, K, L;
    int32_t radius, thickness, half;
    const float *target_px, *fit_px;
    const uint8_t *kp_mask;
    const int32_t *limbs;             /* [L][2] or NULL with L = 0 */
    const uint8_t *limb_rgb;          /* [L][3] */
    const uint8_t *imgs;              /* or NULL */
    int64_t imgs_stride[4];           /* elements: frame, row, column, channel */
    const float *prior;
    const uint8_t *mask;
    uint8_t target_rgb[4], fit_rgb[4];   /* r, g, b, unused */
    uint8_t *out;
} SoarFitvizStripArgs;
int soar_fitviz_yaw_views(int32_t N, int32_t V, int32_t n_views, const float *verts, const int64_t *verts_stride, const float *pivot,
                          const float *R, float *out, void *stream);
int soar_fitviz_strip(const SoarFitvizStripArgs *args, void *stream);
int soar_fitviz_residuals(int32_t N, int32_t K, const float *fit_px, const float *target_px, const float *conf, const uint8_t *kp_mask,
                          float thresh, float *out, void *stream);

/* ---- MJPEG video output: a baseline JPEG encoder (video.hip, soar_amd/video.py) ----
 * B frames of uint8 pixels -> B complete JPEG files (SOI .. EOI), one after the other in one device buffer, with their byte offsets.
 * Baseline sequential, 8 bit, components 1, 2, 3 = Y, Cb, Cr, the four Annex K Huffman tables, restart markers.  Current stream, no
 * synchronisation, no allocation; integer arithmetic only: two calls give the same bytes, and a frame's bytes depend neither on B nor
 * on its place.  frames, workspace, offsets and out are device memory; args is host memory.
 *
 * frames: [B][H][W][channels] uint8, channels 3 (R, G, B) or 4 (the fourth is ignored); every frame contiguous, frame_stride bytes
 *   from frame to frame (>= H W channels).  1 <= H, W <= 65535, 0 <= B <= 65535.
 * qtables: [0] for Y, [1] for Cb and Cr; natural (row-major) order, entries 1 .. 255.
 * subsampling: 444, or 420 (2 x 2 luma blocks per MCU).  restart_interval: MCUs, 1 .. 65535.
 *
 * Colour: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16,
 *   Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16.
 * Padding at 444: the last column and row replicated up to a multiple of 8.  At 420: chroma columns replicated to a multiple of 16,
 *   the last row to an even height, then (a + b + c + d + bias) >> 2 with bias 1 in even and 2 in odd output columns, then the last
 *   DOWNSAMPLED row replicated down to the MCU grid.  Luma is replicated inside the ceil(W / 8) x ceil(H / 8) real blocks only; a luma
 *   block of an MCU beyond them is a dummy: its AC coefficients are 0 and its DC is that of the block coded before it in the MCU.
 * Forward DCT: libjpeg's jfdctint on samples - 128 (13-bit constants, PASS1_BITS = 2, rows first, DESCALE(x, n) =
 *   (x + (1 << (n - 1))) >> n, outputs scaled by 8).  Quantisation: q = 8 Q, (|c| + (q >> 1)) / q truncated, the sign restored.
 * Entropy coding: zigzag order, DC differences per component, (run, size) symbols with ZRL and EOB, a negative value v of size n coded
 *   as v + 2^n - 1, 0xFF followed by 0x00.  In front of MCU k restart_interval (k >= 1) the bit stream is padded with 1-bits to a
 *   byte, FF D0+((k - 1) & 7) is written and the three DC predictors are reset; the last interval is padded the same way before EOI.
 * Header (the same for every frame of a call, 629 bytes): SOI, APP0 (JFIF 1.01, no units, 1:1), DQT 0, DQT 1, SOF0 (sampling 1x1, or
 *   2x2 1x1 1x1; Tq 0 1 1), DHT DC0 AC0 DC1 AC1, DRI, SOS (Ss 0, Se 63, Ah/Al 0).
 *
 * soar_jpeg_workspace_bytes: what both calls need for these B, H, W, subsampling and restart_interval.
 * soar_jpeg_measure: transform, entropy coding as a count, scan.  offsets [B + 1] int64: frame b will occupy bytes
 *   offsets[b] .. offsets[b + 1] of the output; offsets[B] is its length.  Leaves the coefficients and the offsets in the workspace.
 * soar_jpeg_emit: the same args and the workspace soar_jpeg_measure left -> out.  If offsets[B] > capacity NOTHING is written (the
 *   caller reads the need from offsets); nothing is ever written at or behind out + capacity.
 * Both refuse bad arguments before any launch. */
typedef struct SoarJpegArgs {
    int32_t B, H, W, channels;
    int32_t subsampling;              /* 444 or 420 */
    int32_t restart_interval;         /* MCUs */
    const uint8_t *frames;
    int64_t frame_stride;             /* bytes */
    uint8_t qtables[2][64];
} SoarJpegArgs;
int soar_jpeg_workspace_bytes(const SoarJpegArgs *args, size_t *bytes);
int soar_jpeg_measure(const SoarJpegArgs *args, void *workspace, size_t workspace_bytes, int64_t *offsets, void *stream);
int soar_jpeg_emit(const SoarJpegArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int64_t capacity, void *stream);

/* ---- PNG output: filters, run-length deflate, CRC (png.hip, soar_amd/png.py) ----
 * B images of uint8 pixels -> B complete PNG files (signature, IHDR, IDAT ..., IEND), one after the other in one device buffer, with
 * their byte offsets.  8 bit, colour type 0, 2 or 6, no interlace, no ancillary chunks.  Current stream, no synchronisation, no
 * allocation; integer arithmetic and integer atomics only: two calls give the same bytes, and an image's bytes depend neither on B nor
 * on its place.  images, workspace, offsets and out are device memory; args is host memory.  The host adds nothing to the files.
 *
 * images: [B][H][W][channels] uint8, channels 1 (grey, colour type 0), 3 (RGB, type 2) or 4 (RGBA, type 6); every image contiguous,
 *   image_stride bytes from image to image (>= H W channels).  1 <= H, W <= 65535, 0 <= B <= 65535.
 * filter: 0 .. 4 forces None, Sub, Up, Average or Paeth (the PNG specification's, bytes beyond the image being 0) on every row; -1
 *   picks for every row the type with the smallest sum of |residual as int8|, ties to the lowest type.  A row is filtered against the
 *   RAW row above.  The filtered stream of an image is H rows of 1 + W channels bytes, the type first.
 * piece_bytes: 32 .. 65535.  The stream is cut into pieces of that many bytes (the last may be shorter); nothing in a piece refers to
 *   another, and at most B ceil(H (1 + W channels) / piece_bytes) <= 2^30 pieces are in a call.
 * Tokens: maximal runs of equal bytes inside a piece, from the left.  A run of N bytes is one literal, then with rest = N - 1: while
 *   rest >= 3 a match of min(rest, 258) at distance 1; then the rest (1 or 2) as literals.  No search, no hash table.
 * Code: counts over the 286 literal/length symbols, the end-of-block symbol counted once; T their sum, f = 1 + T / 32000, every used
 *   count raised to at least f, T' the raised counts' sum.  A used symbol's length is the smallest l with (count << l) >= T' (1 .. 15;
 *   the Kraft sum is at most 1).  Then sweeps: for L = 2 .. 15 in turn, of the symbols of length L the first min(their number,
 *   D >> (15 - L)) in symbol order are shortened to L - 1, D being 2^15 minus the sum of 2^(15 - length); sweeps repeat until D is 0:
 *   the code is complete.  Codes are RFC 1951's canonical ones.  The distance alphabet is one code of one bit.
 * Block: BFINAL 0, BTYPE 2, HLIT 29, HDIST 0, HCLEN 15; the code-length alphabet's lengths are 0 for 16, 17, 18 and 4 for 0 .. 15, so
 *   each of the 286 + 1 lengths follows as 4 bits of its own (1222 header bits; no run-length coding of the header); the tokens (a
 *   Huffman code goes most significant bit first, extra bits least significant first); end of block; an empty stored block (000,
 *   zeros to the byte, 00 00 FF FF), so that a piece ends on a byte.  If that is not smaller than 5 + n bytes the piece is ONE
 *   STORED BLOCK instead (00, n, ~n, the n bytes).
 * Framing: 89 'PNG' 0D 0A 1A 0A; IHDR; one IDAT per piece, the first beginning with the zlib header 78 01; an IDAT with the final
 *   empty fixed block 03 00 and the Adler-32 of the whole filtered stream, big-endian, joined from the pieces' values
 *   (A = A1 + A2 - 1, B = B1 + B2 + len2 (A1 - 1), modulo 65521); IEND.  Every chunk's CRC-32 is computed on the device.
 *
 * soar_png_workspace_bytes: what both calls need for these B, H, W, channels and piece_bytes.
 * soar_png_measure: filtering, tokens, codes and sizes, scan.  offsets [B + 1] int64: image b will occupy bytes
 *   offsets[b] .. offsets[b + 1] of the output; offsets[B] is its length.  Leaves the filtered streams, the codes and the offsets in
 *   the workspace.
 * soar_png_emit: the same args and the workspace soar_png_measure left -> out.  If offsets[B] > capacity NOTHING is written (the
 *   caller reads the need from offsets): every wavefront returns before its first store; nothing is ever written at or behind
 *   out + capacity.
 * Both refuse bad arguments before any launch. */
typedef struct SoarPngArgs {
    int32_t B, H, W, channels;
    int32_t filter;                   /* 0 .. 4, or -1: adaptive */
    int32_t piece_bytes;
    const uint8_t *images;
    int64_t image_stride;             /* bytes */
} SoarPngArgs;
int soar_png_workspace_bytes(const SoarPngArgs *args, size_t *bytes);
int soar_png_measure(const SoarPngArgs *args, void *workspace, size_t workspace_bytes, int64_t *offsets, void *stream);
int soar_png_emit(const SoarPngArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int64_t capacity, void *stream);

/* ---- PNG input: chunk walk, inflate, Adler-32, row filters (png_decode.hip, png_inflate.h, soar_amd/png.py) ----
 * B PNG files, one after the other in one device buffer -> B images of uint8 pixels, each with a status.  8 bit, colour type 0, 2
 * or 6, no interlace; ancillary chunks (and a PLTE) are skipped; any number of IDATs of any length; all of RFC 1951 and the zlib
 * framing of RFC 1950 (method 8, any window, no dictionary).  Current stream, no synchronisation, no allocation; integer arithmetic
 * and integer atomics only: two calls give the same bytes, and an image's bytes and status depend neither on B nor on its place.
 * data, offsets, workspace, out, status and segments are device memory; args is host memory.
 *
 * data: total_bytes bytes; file b is data[offsets[b], offsets[b + 1]).  offsets [B + 1] int64, ascending inside [0, total_bytes]: if
 *   they are not, every file of the call gets SOAR_PNG_BAD_STRUCTURE.  Every file must have this H, W and channels (1: colour type 0,
 *   3: type 2, 4: type 6); H (1 + W channels) < 2^31, a file is shorter than 2^31 bytes, 0 <= B <= 65535.
 * out: [B][H][W][channels].  status [B]: 0, or the first fault met in this order -- the chunk walk from the file's start (signature;
 *   a chunk that does not fit the file; IHDR first, its CRC-32, its fields; every IDAT's CRC-32; IEND), the zlib header, the deflate
 *   blocks, the bytes behind the final block, the output's length, the Adler-32, the rows' filter bytes.  The image of a failed
 *   file is all zeros.  Nothing is read outside a file's bytes, nothing is written outside its image and its parts of the workspace.
 * segments [B]: a file whose IDATs provably begin at block boundaries of the deflate stream is inflated segment by segment, a
 *   wavefront each.  A candidate is byte 2 of the joined IDAT data Z and every later start p of an IDAT's data, p < |Z|, in front of
 *   which lie 00 00 FF FF or an IDAT that is exactly one stored block that is not final.  A first pass decodes every candidate from
 *   its byte without a store: it succeeds if a block that is not final ends at bit 8 p' (p' the next candidate) or, for the last,
 *   the final block ends with four bytes left, and no match reaches before the segment's own first byte.  If all succeed and their
 *   lengths sum to H (1 + W channels), a second pass writes each at its offset, and segments[b] counts those that gave a byte;
 *   otherwise the file is ONE segment from byte 2 and its faults are that decode's. */
#define SOAR_PNG_OK 0
#define SOAR_PNG_BAD_STRUCTURE 1      /* signature, truncation, chunk order, no IDAT, a width or height of 0, bad offsets */
#define SOAR_PNG_UNSUPPORTED 2        /* interlace, depth, colour type 3 or 4, unknown critical chunk, FDICT, another H, W or channels */
#define SOAR_PNG_BAD_CRC 3            /* of IHDR or an IDAT */
#define SOAR_PNG_CORRUPT 4            /* the deflate stream: block type 3, LEN / NLEN, a bad code, symbol 286 / 287, distance code 30 / 31,
                                         a distance before the output's start, the input's end inside the stream */
#define SOAR_PNG_WRONG_LENGTH 5       /* more or fewer than H (1 + W channels) bytes, or other than 4 bytes behind the final block */
#define SOAR_PNG_BAD_ADLER 6
#define SOAR_PNG_BAD_FILTER 7         /* a row's filter byte above 4 */
typedef struct SoarPngDecodeArgs {
    int32_t B, H, W, channels;
    const uint8_t *data;
    const int64_t *offsets;
    int64_t total_bytes;
} SoarPngDecodeArgs;
int soar_png_decode_workspace_bytes(const SoarPngDecodeArgs *args, size_t *bytes);
int soar_png_decode(const SoarPngDecodeArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int32_t *status, int32_t *segments,
                    void *stream);

/* ---- JPEG input: marker walk, restart scan, Huffman decode, inverse DCT, upsampling, colour (jpeg_decode.hip, jpeg_entropy.h,
 *      soar_amd/jpeg.py) ----
 * B baseline JPEG files, one after the other in one device buffer -> B images of uint8 pixels, each with a status.  SOF0, 8 bit,
 * Huffman; one component (channels 1), or three (channels 3: YCbCr, luma sampled 1x1, 2x1 or 2x2, chroma 1x1); one interleaved scan;
 * any DQT (8-bit entries) and DHT tables, any restart interval; APPn, COM and fill bytes skipped, bytes after EOI ignored; a file
 * without any DHT gets Annex K's four tables (an MJPG chunk of an AVI).  The pixels are libjpeg's, exact in integers: dequantisation,
 * the slow-but-accurate inverse DCT (jidctint) with clamping to 0 .. 255, "fancy" triangle-filter upsampling with the true
 * downsampled size as the edge (plain replication where the downsampled width is 2 or less), and the fixed-point YCbCr -> RGB
 * tables.  Current stream, no synchronisation, no allocation; integer arithmetic only: two calls give the same bytes, and an image's
 * bytes and status depend neither on B nor on its place.  data, offsets, workspace, out, status and intervals are device memory;
 * args is host memory.
 *
 * data: total_bytes bytes; file b is data[offsets[b], offsets[b + 1]).  offsets [B + 1] int64, ascending inside [0, total_bytes]: if
 *   they are not, every file of the call gets SOAR_JPEG_BAD_STRUCTURE.  Every file must have this H, W and component count;
 *   1 <= H, W <= 65535, a file is shorter than 2^31 bytes, 0 <= B <= 65535.
 * out: [B][H][W][channels].  status [B]: 0, or the first fault of the walk from SOI to the end of SOS; then of the restart scan (inside
 *   the entropy-coded segment an FF followed by anything but 00 or FF is a marker; the first that is no RSTn ends the segment; the
 *   RSTn in front of it must number ceil(MCUs / Ri) - 1 and count 0 .. 7 cyclically); then of the intervals: CORRUPT if any interval
 *   is, else TRUNCATED.  The image of a failed file is all zeros.  Nothing is read outside a file's bytes, nothing is written outside
 *   its image and its parts of the workspace.
 * intervals [B]: the restart intervals the file's scan was decoded in, one lane each (1: no restart markers, one lane's serial work);
 *   0 for a file that failed before its scan was decoded. */
#define SOAR_JPEG_OK 0
#define SOAR_JPEG_BAD_STRUCTURE 1     /* no SOI, a segment running past the end, SOS before SOF, a width or height of 0, table ids or
                                         Huffman counts that are no code, bad offsets */
#define SOAR_JPEG_UNSUPPORTED 2       /* progressive, extended, lossless, arithmetic; 12 bit; 16-bit quantisers; other component counts or
                                         sampling factors; several scans; DNL; another H, W or channels than the call's */
#define SOAR_JPEG_MISSING_TABLE 3     /* the frame or the scan names a table that was never defined */
#define SOAR_JPEG_CORRUPT 4           /* an invalid Huffman code, a run past coefficient 63, a wrong, missing or misplaced restart marker */
#define SOAR_JPEG_TRUNCATED 5         /* the data ends before the last MCU */
typedef struct SoarJpegDecodeArgs {
    int32_t B, H, W, channels;
    const uint8_t *data;
    const int64_t *offsets;
    int64_t total_bytes;
} SoarJpegDecodeArgs;
int soar_jpeg_decode_workspace_bytes(const SoarJpegDecodeArgs *args, size_t *bytes);
int soar_jpeg_decode(const SoarJpegDecodeArgs *args, void *workspace, size_t workspace_bytes, uint8_t *out, int32_t *status, int32_t *intervals,
                     void *stream);

/* ---- resize of 8-bit images by Pillow's rule (image_resize.hip, soar_amd/jpeg.py resize_images) ----
 * images [B][H][W][channels] uint8 -> out [B][out_h][out_w][channels]: a horizontal pass into temp [B][H][out_w][channels], then a
 * vertical one.  Per output position of a pass the tables give the first input sample and the count (bounds [n][2] int32) and the
 * coefficients (coef [n][ksize] int32, 22-bit fixed point); an output is clamp((2^21 + sum sample * coefficient) >> 22, 0, 255).
 * The tables are the caller's (soar_amd/jpeg.py builds Pillow's bicubic ones: support widened by the scale when shrinking,
 * normalised in double); bounds that do not fit the axis or ksize give 0.  Everything but args is device memory; current stream,
 * no synchronisation, no allocation. */
typedef struct SoarResizeArgs {
    int32_t B, H, W, channels, out_h, out_w, ksize_h, ksize_v;
    const uint8_t *images;
    uint8_t *temp;
    const int32_t *bounds_h, *coef_h;     /* [out_w][2], [out_w][ksize_h] */
    const int32_t *bounds_v, *coef_v;     /* [out_h][2], [out_h][ksize_v] */
} SoarResizeArgs;
int soar_resize_u8(const SoarResizeArgs *args, uint8_t *out, void *stream);

/* ---- SAM point-prompt segmentation, forward only, float32 (sam.hip, soar_amd/sam.py) ----
 * The sizes of a model (what soar_amd/sam.py reads from a state dict).  window[b] = 0: block b attends over the whole grid.
 * Every width that feeds a matrix product (embed, mlp, out_chans, dec_mlp, out_chans / dec_down, iou_hidden, 3 patch patch) is a
 * multiple of 8, head_dim a multiple of 4 up to 96, a window or a global grid at most 64 tokens a side. */
#define SOAR_SAM_MAX_DEPTH 32
typedef struct SoarSamConfig {
    int32_t image_size, patch, grid;           /* grid = image_size / patch tokens a side */
    int32_t embed, depth, heads, head_dim, mlp;/* encoder: width, blocks, heads x head_dim = embed, MLP width */
    int32_t out_chans;                         /* neck / prompt / decoder width */
    int32_t window[SOAR_SAM_MAX_DEPTH];
    int32_t dec_layers, dec_heads, dec_down, dec_mlp, mask_tokens, hyper_depth, iou_depth, iou_hidden;
} SoarSamConfig;
/* The packed weights: `count` contiguous float32 device tensors in the order of soar_amd.sam.tensor_keys (segment_anything's
 * layouts), copied, with the 3 x 3 neck convolution and the two transposed convolutions re-laid for the kernels and the dense
 * positional encoding of the token grid computed behind them.  packed: soar_sam_weights_bytes bytes, 256-byte aligned. */
int soar_sam_weights_bytes(const SoarSamConfig *cfg, size_t *bytes, int32_t *count);
int soar_sam_pack_weights(const SoarSamConfig *cfg, const float *const *tensors, int32_t count, void *packed, size_t packed_bytes,
                          void *stream);
/* one workspace for encode and decode of B frames with up to max_points points each */
int soar_sam_workspace_bytes(const SoarSamConfig *cfg, int32_t B, int32_t max_points, size_t *bytes);
/* resized [B][nh][nw][3] uint8 (the longer side = image_size) -> patches [B][grid grid][3 patch patch] float32: (x - mean) / std,
 * zeros below and right of the frame, one row per token in the patch convolution's (channel, y, x) order */
int soar_sam_preprocess(const SoarSamConfig *cfg, int32_t B, int32_t nh, int32_t nw, const uint8_t *resized, float *patches, void *stream);
/* The image encoder, or a part of it.  patches != NULL: patch embedding + pos_embed first; else tokens_in [B][grid grid][embed] is
 * the input.  Blocks block_begin .. block_end - 1 run on it; tokens_out (or NULL) receives the tokens after them; embeddings (or
 * NULL: no neck) [B][grid][grid][out_chans] the neck's output. */
typedef struct SoarSamEncodeArgs {
    int32_t B, block_begin, block_end;
    const float *patches, *tokens_in;
    float *tokens_out, *embeddings;
} SoarSamEncodeArgs;
int soar_sam_encode(const SoarSamConfig *cfg, const void *packed, const SoarSamEncodeArgs *args, void *workspace, size_t workspace_bytes,
                    void *stream);
/* Prompt encoder and mask decoder.  points [B][max_points][2] (x, y) in pixels of the original frame, scaled here by scale_x,
 * scale_y; labels [B][max_points] int32 (1 / 0); counts [B] int32 in [0, max_points]: frame b has counts[b] points and one padding
 * point behind them, and slots past that take part in nothing.  low_res [B][mask_tokens - 1][4 grid][4 grid], iou
 * [B][mask_tokens - 1]: masks 1 .. (multimask output).  prompt_tokens / tokens_out (or NULL) [B][1 + mask_tokens + max_points + 1]
 * [out_chans]: the decoder's tokens before and after the two-way transformer (a frame's first 2 + mask_tokens + counts[b]; what lies
 * behind them is unspecified). */
typedef struct SoarSamDecodeArgs {
    int32_t B, max_points;
    float scale_x, scale_y;
    const float *embeddings, *points;
    const int32_t *labels, *counts;
    float *low_res, *iou, *prompt_tokens, *tokens_out;
} SoarSamDecodeArgs;
int soar_sam_decode(const SoarSamConfig *cfg, const void *packed, const SoarSamDecodeArgs *args, void *workspace, size_t workspace_bytes,
                    void *stream);
/* low_res [B][K][L][L] -> bilinear (align_corners = false) to image_size squared, cropped to nh x nw, bilinear to H x W:
 * logits [B][K][H][W] float32 and / or masks (logit > 0) uint8, either may be NULL */
int soar_sam_postprocess(int32_t B, int32_t K, int32_t L, int32_t image_size, int32_t nh, int32_t nw, int32_t H, int32_t W,
                         const float *low_res, float *logits, uint8_t *masks, void *stream);
/* Multi-head attention with the decomposed relative-position bias by itself: qkv [B][gh gw][3 heads hd] (q | k | v, head-major) ->
 * out [B][gh gw][heads hd].  window = 0: every token attends to the gh x gw grid; else inside window x window windows of the grid
 * zero-padded to a multiple of the window, where a padded key is bias's k and v ([3 heads hd]) and padded queries are dropped.
 * logit = (scale q) . k + q . rel_h[qy - ky + Sh - 1] + q . rel_w[qx - kx + Sw - 1]; rel_h [(2 Sh - 1)][hd], rel_w [(2 Sw - 1)][hd]
 * for the sequence Sh x Sw (the window or the grid), or both NULL. */
int soar_sam_attention(const float *qkv, const float *bias, const float *rel_h, const float *rel_w, float *out, int32_t B, int32_t gh,
                       int32_t gw, int32_t heads, int32_t hd, int32_t window, float scale, void *stream);

/* ---- The multi-view diffusion UNet of the SDS guidance, forward only, float32 (unet.hip, attention.hip, soar_amd/unet.py) ----
 * ldm's openaimodel.UNetModel with MVDream's / ImageDream's additions (camera embedding, self-attention over the views of a group,
 * image-token cross-attention), transformer depth 1, linear proj_in / proj_out.  The sizes are what soar_amd/unet.py reads from a
 * state dict.  model_channels times every multiplier is a multiple of 32 (GroupNorm) and of head_channels; context_dim, camera_dim
 * multiples of 8; head_channels a multiple of 4 up to 64.  attention[l] != 0: level l's blocks carry a transformer (the middle
 * block always does).  camera_dim = 0: no camera embedding.  with_ip: attn2 has to_k_ip / to_v_ip. */
#define SOAR_UNET_MAX_LEVELS 8
#define SOAR_UNET_MAX_PROBES 16
typedef struct SoarUnetConfig {
    int32_t in_channels, out_channels, model_channels, levels, num_res_blocks;
    int32_t channel_mult[SOAR_UNET_MAX_LEVELS], attention[SOAR_UNET_MAX_LEVELS];
    int32_t context_dim, camera_dim, with_ip, head_channels, n_view;
    int32_t precision;             /* of the products' operands: 0 float32 (what a zero-initialised struct asks for), 1 bf16, 2 f16 */
    int32_t attn_precision;        /* of the attentions' operands, independent of `precision`: 0 float32 (what a zero-initialised
                                      struct asks for), 1 bf16, 2 f16: soar_attention16's kernel and contract */
} SoarUnetConfig;
/* The packed weights: `count` contiguous float32 device tensors of sizes[i] floats in the order of soar_amd.unet.tensor_keys (ldm's
 * layouts; a size that is not the layout's is refused, naming the index), copied, the 3 x 3 convolutions re-laid as [Cout][tap][Cin]
 * (the first one's Cin padded to 8 with zeros).  floats (or NULL): the sum of the sizes.  packed: 256-byte aligned.
 * precision != 0: every tensor that is a product's B operand (the convolutions' and linear layers' weights) is laid as bf16 / f16,
 * rounded to nearest even, its start still 16-byte aligned; biases, norm gains and the rest stay float32.  The sources are the same
 * float32 tensors; `bytes` shrinks, `count` and `floats` do not change.  soar_unet_forward then runs every product on the 16-bit
 * matrix core with float32 accumulation, its activations rounded as they are loaded; activations in memory, GroupNorm, LayerNorm,
 * attention, inputs, outputs and probes stay float32, and the bit-exact promises below hold for each precision.
 * attn_precision != 0: both attentions of every transformer run as soar_attention16 (q scale, k, v and p rounded to the type inside
 * the kernel, every sum float32); it changes neither the packed weights nor the workspace, and the bit-exact promises hold for each
 * value.  A value outside 0 .. 2 is refused, naming the number. */
int soar_unet_weights_bytes(const SoarUnetConfig *cfg, size_t *bytes, int32_t *count, size_t *floats);
int soar_unet_pack_weights(const SoarUnetConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                           size_t packed_bytes, void *stream);
/* N latents of H x W with T context tokens and ip_tokens image tokens (0: none).  Refuses an H or W that is odd at a level that is
 * down-sampled, naming the level. */
int soar_unet_workspace_bytes(const SoarUnetConfig *cfg, int32_t N, int32_t H, int32_t W, int32_t T, int32_t ip_tokens, size_t *bytes);
/* eps = UNet(x, t, context, camera, ip_tokens).  x [N][in_channels][H][W] with any strides (floats); t [N] float32, read on the device;
 * context [N][T][context_dim]; camera [N][camera_dim] or NULL; ip_tokens [N][n_ip][context_dim] or NULL (n_ip = 0): the second key set
 * of every cross-attention, its result added times ip_weight.  N is a multiple of n_view: self-attention runs over the n_view latents
 * of a group, and a group's result does not depend on the other groups, bit for bit.  eps [N][H][W][out_channels] (channels last).
 * Probes: after the stage probe_code[i] names, that stage's channels-last activation is copied to probe_dst[i].  Code = 8 block +
 * stage; block = the index in input_blocks, then the middle block, then output_blocks; stage 0: the ResBlock's (or the block's
 * convolution's) output, 1 / 2 / 3: the transformer's tokens after attn1 / attn2 / ff, 4: the transformer's output, 5: the up-sampling
 * convolution's output, 6: the concatenated input of an output block; SOAR_UNET_PROBE_EMB: emb [N][4 model_channels].
 * No atomics, no host synchronisation, no allocation: two calls give the same bits. */
#define SOAR_UNET_PROBE_EMB 1000000
typedef struct SoarUnetArgs {
    int32_t N, H, W, T, n_ip;
    float ip_weight;
    const float *x;
    int64_t x_stride[4];
    const float *t, *context, *camera, *ip_tokens;
    float *eps;
    int32_t n_probes;
    int32_t probe_code[SOAR_UNET_MAX_PROBES];
    float *probe_dst[SOAR_UNET_MAX_PROBES];
} SoarUnetArgs;
int soar_unet_forward(const SoarUnetConfig *cfg, const void *packed, const SoarUnetArgs *args, void *workspace, size_t workspace_bytes,
                      void *stream);
/* Multi-head attention by itself: out [B][Lq][.] = softmax(scale q k^T) v per head, q [B][Lq][.], k, v [B][Lk][.] from their own
 * pointers with their own row pitches (ld*, floats, multiples of 4, at least heads hd); head j is channels j hd .. + hd of a row.
 * Lk is any count from 1; hd a multiple of 4 up to 64.  k2 / v2 [B][Lk2][.] (or both NULL): a second key / value set, whose
 * normalised result is added times w2 in the same launch. */
typedef struct SoarUnetAttnArgs {
    const float *q, *k, *v, *k2, *v2;
    float *out;
    int64_t ldq, ldk, ldv, ldk2, ldv2, ldo;
    int32_t B, Lq, Lk, Lk2, heads, hd;
    float scale, w2;
} SoarUnetAttnArgs;
int soar_unet_attention(const SoarUnetAttnArgs *args, void *stream);
/* The same attention on the 16-bit matrix core.  type: 1 bf16, 2 f16; hd a multiple of 4 up to 96; causal != 0: key j counts for query
 * i when j <= i (needs one key set and Lq = Lk).  Everything in memory stays float32.  Inside the kernel q * scale (computed in
 * float32), k and v are rounded to the type, nearest even; the scores are v_mfma_f32_32x32x16_{bf16,f16} sums in float32; the masks,
 * the running maximum, p = expf(s - m) and the running sum l (of the unrounded p) are float32 as in soar_unet_attention; p is rounded
 * to the type only as the operand of p v, which accumulates in float32; 1 / l, the w2 combination and the store are float32.
 * Operands that overflow or are denormal in the type are outside the contract.  No atomics; a (batch, head, 128-query tile)'s result
 * does not depend on the rest of the launch; two runs give the same bits.  Every refusal (a type outside 1 .. 2 and all of
 * soar_unet_attention's) comes before any launch. */
int soar_attention16(const SoarUnetAttnArgs *args, int32_t type, int32_t causal, void *stream);

/* ---- The SDS guidance's conditioning, forward only, float32 (clip.hip, attention.hip, soar_amd/clip.py) ----
 * One pre-LN transformer tower serves CLIP's text encoder (causal mask; token + position embedding in front) and its ViT image
 * encoder (patch product, class token, position embedding and ln_pre in front): x += out_proj(attn(ln_1 x)); x += c_proj(gelu_erf(
 * c_fc(ln_2 x))), LayerNorm eps 1e-5, scale head_dim^-0.5.  width and mlp are multiples of 8, head_dim = width / heads a multiple of
 * 4 up to 96.  tokens: the text context length, or 1 + grid^2.  A sizing call refuses what the kernels cannot run, naming the number. */
#define SOAR_CLIP_TEXT 0
#define SOAR_CLIP_VISION 1
#define SOAR_CLIP_MAX_LAYERS 64
#define SOAR_CLIP_MAX_PROBES 16
typedef struct SoarClipConfig {
    int32_t kind;                      /* SOAR_CLIP_TEXT or SOAR_CLIP_VISION */
    int32_t width, heads, layers, mlp, tokens;
    int32_t vocab;                     /* text */
    int32_t patch, grid;               /* vision: the image is grid patch pixels a side */
    int32_t precision;                 /* of the products' operands: 0 float32 (what a zero-initialised struct asks for), 1 bf16, 2 f16 */
    int32_t attn_precision;            /* of the attention's operands, independent of `precision`: 0 float32, 1 bf16, 2 f16
                                          (soar_attention16's kernel and contract) */
} SoarClipConfig;
/* The packed weights: `count` contiguous float32 device tensors of sizes[i] floats in the order of soar_amd.clip.tower_keys (open_clip's
 * layouts: q | k | v as one in_proj), copied; the patch convolution's rows are padded from 3 patch^2 to a multiple of 8 with zeros.
 * floats (or NULL): the sum of the sizes.  packed: 256-byte aligned.
 * precision != 0: every tensor that is a product's B operand (the patch convolution, in_proj, out_proj, c_fc and c_proj weights) is
 * laid as bf16 / f16, rounded to nearest even, its start still 16-byte aligned; the token table, the class and position rows, biases
 * and norm gains stay float32.  The sources are the same float32 tensors; `bytes` shrinks, `count` and `floats` do not change, nor
 * does the workspace.  soar_clip_forward then runs every product on the 16-bit matrix core with float32 accumulation, its
 * activations rounded as they are loaded; everything in memory stays float32.  attn_precision != 0: the attention runs as
 * soar_attention16.  The bit-exact promises below hold for every pair of values; one outside 0 .. 2 is refused, naming the number. */
int soar_clip_weights_bytes(const SoarClipConfig *cfg, size_t *bytes, int32_t *count, size_t *floats);
int soar_clip_pack_weights(const SoarClipConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                           size_t packed_bytes, void *stream);
/* B sequences of L tokens (text: 1 <= L <= tokens; vision: L = tokens) */
int soar_clip_workspace_bytes(const SoarClipConfig *cfg, int32_t B, int32_t L, size_t *bytes);
/* images [B][grid patch][grid patch][3] uint8 -> rows [B][grid^2][Kp] float32, Kp = 3 patch^2 rounded up to 8: element
 * (channel patch + y) patch + x of a token is its pixel's (byte / 255 - mean) / std with CLIP's constants; elements from 3 patch^2 zeros */
int soar_clip_preprocess(const SoarClipConfig *cfg, int32_t B, const uint8_t *images, float *rows, void *stream);
/* out [B][L][width]: the tokens after run_layers blocks (0 .. layers), through ln_final / ln_post when final_norm != 0.  Text: ids
 * [B][L] int32, each in [0, vocab) (the kernel clamps); vision: patches = soar_clip_preprocess's rows.  Probes: the tokens [B][L][width]
 * after the stage probe_code[i] names are copied to probe_dst[i]; 2 block: after the block's attention, 2 block + 1: after the block;
 * SOAR_CLIP_PROBE_EMBED: the embedding (vision: patch product, class row and positions), SOAR_CLIP_PROBE_PRE: after ln_pre (vision).
 * No atomics, no host synchronisation, no allocation; a sequence's result is the same bits alone and in any batch. */
#define SOAR_CLIP_PROBE_EMBED 1000000
#define SOAR_CLIP_PROBE_PRE 1000001
typedef struct SoarClipArgs {
    int32_t B, L, run_layers, final_norm;
    const int32_t *ids;
    const float *patches;
    float *out;
    int32_t n_probes;
    int32_t probe_code[SOAR_CLIP_MAX_PROBES];
    float *probe_dst[SOAR_CLIP_MAX_PROBES];
} SoarClipArgs;
int soar_clip_forward(const SoarClipConfig *cfg, const void *packed, const SoarClipArgs *args, void *workspace, size_t workspace_bytes,
                      void *stream);
/* The towers' attention by itself: soar_unet_attention's kernel with one key set, hd a multiple of 4 up to 96, and causal != 0:
 * key j counts for query i when j <= i (needs Lq = Lk). */
typedef struct SoarClipAttnArgs {
    const float *q, *k, *v;
    float *out;
    int64_t ldq, ldk, ldv, ldo;
    int32_t B, Lq, Lk, heads, hd, causal;
    float scale;
} SoarClipAttnArgs;
int soar_clip_attention(const SoarClipAttnArgs *args, void *stream);

/* IP-Adapter's Resampler: `queries` learned latents attend over proj_in(x) and themselves (one softmax over n + queries keys), `depth`
 * times, each followed by a bias-free feed-forward of width ff; then proj_out and norm_out.  dim, emb, ff and heads dim_head are
 * multiples of 8, dim_head a multiple of 4 up to 96.  Tensors in the order of soar_amd.clip.resampler_keys. */
typedef struct SoarResamplerConfig {
    int32_t dim, depth, heads, dim_head, queries, emb, out, ff;
    int32_t precision, attn_precision; /* as SoarClipConfig's: the B operands are proj_in, proj_out, to_q, to_kv, to_out and the two
                                          feed-forward matrices; the latents, biases and norm gains stay float32 */
} SoarResamplerConfig;
int soar_resampler_weights_bytes(const SoarResamplerConfig *cfg, size_t *bytes, int32_t *count, size_t *floats);
int soar_resampler_pack_weights(const SoarResamplerConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                                size_t packed_bytes, void *stream);
int soar_resampler_workspace_bytes(const SoarResamplerConfig *cfg, int32_t B, int32_t n, size_t *bytes);
/* x [B][n][emb] -> out [B][queries][out].  Probes [B][queries][dim]: 2 layer: the latents after the layer's attention, 2 layer + 1:
 * after its feed-forward. */
typedef struct SoarResamplerArgs {
    int32_t B, n;
    const float *x;
    float *out;
    int32_t n_probes;
    int32_t probe_code[SOAR_CLIP_MAX_PROBES];
    float *probe_dst[SOAR_CLIP_MAX_PROBES];
} SoarResamplerArgs;
int soar_resampler_forward(const SoarResamplerConfig *cfg, const void *packed, const SoarResamplerArgs *args, void *workspace,
                           size_t workspace_bytes, void *stream);

/* ---- body keypoint detection (pose.hip, soar_amd/pose.py).  Preprocessing; forward only, float32.
 * The BODY_25 network: a VGG front (conv1_1 .. conv4_2, three 2 x 2 max pools), conv4_3_CPM and conv4_4_CPM to `feat` features at 1/8
 * resolution, then n_paf stages of the part-affinity branch (L2, 52 channels) and n_heat stages of the heat-map branch (L1, 26
 * channels).  A stage is five blocks of three 3 x 3 convolutions (each with a PReLU; a block's output is the three outputs side by
 * side), a 1 x 1 convolution with a PReLU and a 1 x 1 convolution to the maps.  Widths: c1 .. c4 the VGG's, cpm conv4_3_CPM's, w0 / m0
 * the blocks' and the 1 x 1's in stage 0 of a branch, w1 / m1 in the later stages.  Every width is a multiple of 8.
 * Tensors in the order of soar_amd.pose.layer_keys: per convolution weight [Cout][Cin][k][k], bias [Cout] and, where a PReLU follows,
 * its slopes [Cout].  Stage inputs (the weights' Cin order): L2 stage 0 (features); L2 stage k (features, previous PAF); L1 stage 0
 * (features, last PAF); L1 stage k (features, previous heat maps, last PAF). */
#define SOAR_POSE_PAF 52
#define SOAR_POSE_HEAT 26
#define SOAR_POSE_PARTS 25
#define SOAR_POSE_PAIRS 26
#define SOAR_POSE_MAX_STAGES 8
#define SOAR_POSE_MAX_PEAKS 32
#define SOAR_POSE_MAX_PEOPLE 32
typedef struct SoarPoseConfig {
    int32_t c1, c2, c3, c4, cpm, feat, w0, w1, m0, m1, n_paf, n_heat;
} SoarPoseConfig;
/* The two sizing calls (bytes; *count: the tensors soar_pose_pack_weights takes). */
int soar_pose_weights_size(const SoarPoseConfig *cfg, size_t *bytes, int32_t *count);
int soar_pose_workspace_size(const SoarPoseConfig *cfg, int32_t B, int32_t H, int32_t W, size_t *bytes);
int soar_pose_pack_weights(const SoarPoseConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                           size_t packed_bytes, void *stream);
/* uint8 RGB [B][H][W][3] -> float32 BGR [B][H][W][3]: v / 256 - 0.5 */
int soar_pose_preprocess(int32_t B, int32_t H, int32_t W, const uint8_t *rgb, float *bgr, void *stream);
/* x: the image, [B][3][H][W] at x_stride (elements); H and W multiples of 16, at least 16.  stage_out[k]: stage k's maps, dense
 * [B][H/8][W/8][52] for k < n_paf, then [..][26]; NULL skips one, but the last stage of either branch is the result and must be given.
 * features: [B][H/8][W/8][feat] or NULL.  A frame's result does not depend on the batch it is in. */
typedef struct SoarPoseNetArgs {
    int32_t B, H, W, pad_;
    const float *x;
    int64_t x_stride[4];
    float *features;
    float *stage_out[2 * SOAR_POSE_MAX_STAGES];
} SoarPoseNetArgs;
int soar_pose_forward(const SoarPoseConfig *cfg, const void *packed, const SoarPoseNetArgs *args, void *workspace, size_t workspace_bytes,
                      void *stream);
/* heat [B][h][w][P] (P = 26: the last map is the background and is not read) -> peaks [B][P][max_peaks][3] (x, y, score) and
 * counts [B][P] (the true number; the background's is 0).  The map upsampled by 8 with the bicubic rule (a = -0.75,
 * source coordinate (X + 0.5) / 8 - 0.5, edge samples clamped; weights ((a (t+1) - 5a)(t+1) + 8a)(t+1) - 4a, ((a+2) t - (a+3)) t t + 1,
 * the same of 1 - t, and 1 - w0 - w1 - w2; each row's four products summed left to right, then the four rows top to bottom), evaluated
 * in LDS strip by strip with a halo of 4 and never stored.  A pixel is a peak if it exceeds `threshold` and is strictly greater than
 * its 8 neighbours (a plateau has none); pixels of the outermost ring are none.  Position: sum(X s) / sum(s) + 0.5 (and Y) over the
 * 7 x 7 window clipped to the map, samples s > 0 only, summed row-major.  Score: the peak's value.  Peaks in raster order; only the
 * first max_peaks (1 .. 32) are written, rows behind min(count, max_peaks) are left alone.  8 w <= 1800. */
int soar_pose_peaks(int32_t B, int32_t h, int32_t w, const float *heat, float threshold, int32_t max_peaks, float *peaks, int32_t *counts,
                    void *stream);
/* peaks, counts as above; paf [B][h][w][52], read at the cell (floor(x / 8), floor(y / 8)) of a sample, clamped: not upsampled.
 * -> people [B][max_people][25][3] (x, y, score in net-input pixels; a missing part and an unused row are zeros) and n_people [B] (the true
 * number).  One workgroup per frame.  Per pair of the BODY_25 table, every candidate (a, b): d = b - a, n = |d| (skipped below 1e-6),
 * m = min(max(5, floor(sqrt(5 n) + 0.5)), 25) samples a + d (i / max(m - 1, 1)); s_i = paf . (d / n); k = samples with s_i >
 * inter_threshold; valid if k / m > min_above; score = (sum of those s_i, in order) / k.  Connections in descending score, ties by
 * (a, b) ascending, no endpoint twice.  Assembly, pair by pair in table order, connection by connection: with persons holding a and b: the
 * two merge if they are different and share no part; with a person holding only one end: it gets the other unless it has that part;
 * with none: a new person.  A person's score is the sum of its peaks' and connections' scores; persons with fewer than min_parts
 * parts or score / parts below min_score are dropped; the others in order of creation, the first max_people (1 .. 32) written. */
typedef struct SoarPoseAssembleArgs {
    int32_t B, h, w, max_peaks, max_people, min_parts;
    float inter_threshold, min_above, min_score;
    int8_t pair_a[SOAR_POSE_PAIRS], pair_b[SOAR_POSE_PAIRS]; /* the limbs in the order they are assembled: parts (a, b) ... */
    int8_t paf_x[SOAR_POSE_PAIRS], paf_y[SOAR_POSE_PAIRS];   /* ... and the PAF channels of the limb's x and y components */
    const float *peaks;
    const int32_t *counts;
    const float *paf;
    float *people;
    int32_t *n_people;
} SoarPoseAssembleArgs;
int soar_pose_assemble(const SoarPoseAssembleArgs *args, void *stream);
/* people [n][3] in place: (x W / net_w, y H / net_h, score) */
int soar_pose_scale(int64_t n, float *people, float W, float net_w, float H, float net_h, void *stream);

/* ---- hand and face keypoint detection (pose_parts.hip, soar_amd/pose_parts.py).  Preprocessing; forward only, float32.
 * One convolutional pose machine (CPM) serves the hand network and the face network.  Its layers, in the order of
 * soar_amd.pose_parts.layer_keys: the front conv1_1 .. conv5_3_CPM (SOAR_CPM_FRONT = 15 convolutions; a 2 x 2 max pool behind front
 * layer i where bit i of pool_mask is set: three bits, so that the maps are at 1/8 resolution), whose last gives the features; stage 1:
 * conv6_1_CPM, conv6_2_CPM (the maps); every later stage: Mconv1 .. Mconv7, reading the previous stage's maps and the features side
 * by side (maps_first != 0: the weights' input channels are (maps, features), else (features, maps)).  n_layers = 17 + 7 (n_stages - 1).
 * ReLU behind every convolution except a stage's last.  width[i]: layer i's output channels, a multiple of 8 except the maps'
 * (n_maps >= 2, the same for every stage); side[i]: its kernel side, 1, 3 or 7, zero padding side / 2.
 * A 7 x 7 convolution runs through the shared implicit GEMM as seven launches, one per kernel row (seven taps each): the first carries
 * the bias, each later one adds to the output in place, a last pass applies the ReLU.  So its sum runs over the kernel's rows top to
 * bottom, inside a row over (tap left to right, input channel) in the GEMM's order.
 * Tensors: per convolution weight [Cout][Cin][side][side] and bias [Cout]. */
#define SOAR_CPM_FRONT 15
#define SOAR_CPM_MAX_STAGES 8
#define SOAR_CPM_MAX_LAYERS (17 + 7 * (SOAR_CPM_MAX_STAGES - 1))
typedef struct SoarCpmConfig {
    int32_t n_stages, n_maps, n_layers, pool_mask, maps_first, pad_;
    int32_t width[SOAR_CPM_MAX_LAYERS];
    int32_t side[SOAR_CPM_MAX_LAYERS];
} SoarCpmConfig;
/* The two sizing calls (bytes; *count: the tensors soar_cpm_pack_weights takes).  They refuse what the kernels cannot run: a width that
 * is no multiple of 8 in 8 .. 4096, a side other than 1, 3, 7, n_maps outside 2 .. 4096, n_stages outside 1 .. 8, a pool_mask without
 * exactly three bits below SOAR_CPM_FRONT - 1, an S that is no multiple of 8, M S S > 2^30. */
int soar_cpm_weights_size(const SoarCpmConfig *cfg, size_t *bytes, int32_t *count);
int soar_cpm_workspace_size(const SoarCpmConfig *cfg, int32_t M, int32_t S, size_t *bytes);
int soar_cpm_pack_weights(const SoarCpmConfig *cfg, const float *const *tensors, const int64_t *sizes, int32_t count, void *packed,
                          size_t packed_bytes, void *stream);
/* x: the crops, [M][3][S][S] at x_stride (elements).  stage_out[k]: stage k + 1's maps, dense [M][S/8][S/8][n_maps]; NULL skips one, but
 * the last stage's is the result and must be given.  features: [M][S/8][S/8][feat] or NULL.  A crop's result does not depend on its batch. */
typedef struct SoarCpmArgs {
    int32_t M, S;
    const float *x;
    int64_t x_stride[4];
    float *features;
    float *stage_out[SOAR_CPM_MAX_STAGES];
} SoarCpmArgs;
int soar_cpm_forward(const SoarCpmConfig *cfg, const void *packed, const SoarCpmArgs *args, void *workspace, size_t workspace_bytes,
                     void *stream);
/* The rectangles of the left hand, the right hand and the face of the first part_people persons of every frame, from their BODY_25
 * keypoints: people [B][max_people][25][3] (x, y, confidence in image pixels), n_people [B] -> boxes [B][part_people][3][4] =
 * (x0, y0, side, valid: 1 or 0), an invalid one all zeros.  A person index at or beyond min(n_people, max_people) is invalid.  One
 * thread per rectangle; float32, every expression as written here, |v| = sqrt(v.x v.x + v.y v.y).
 * Hand (left: shoulder 5, elbow 6, wrist 7; right: 2, 3, 4): c = wrist + 0.33 (wrist - elbow), side = 1.5 max(|wrist - elbow|,
 * 0.9 |elbow - shoulder|), x0 = c.x - side / 2, y0 = c.y - side / 2; valid if the three confidences exceed hand_min_conf, side > 1 and
 * side side > min_hand_area.
 * Face (neck 1, nose 0, right eye 15, left eye 16, right ear 17, left ear 18; present: confidence > face_min_conf): centre, size and
 * count start at 0.  With neck and nose: in profile (lEye == lEar, rEye == rEar, lEye != rEye as presence flags) centre +=
 * ((eye + ear) + nose) / 3 of the visible side and size += 0.85 ((|nose - eye| + |nose - ear|) + |neck - nose|), otherwise centre +=
 * (neck + nose) / 2 and size += 2 |neck - nose|; count + 1.  With both eyes: centre += (lEye + rEye) / 2, size += 3 |lEye - rEye|,
 * count + 1.  With both ears: centre += (lEar + rEar) / 2, size += 2 |lEar - rEar|, count + 1.  With count > 0 centre and size are
 * divided by it; x0 = centre.x - size / 2, y0 = centre.y - size / 2, side = size; valid if count > 0 and side side > min_face_area. */
typedef struct SoarPartBoxArgs {
    int32_t B, max_people, part_people, pad_;
    float hand_min_conf, min_hand_area, face_min_conf, min_face_area;
    const float *people;
    const int32_t *n_people;
    float *boxes;
} SoarPartBoxArgs;
int soar_part_boxes(const SoarPartBoxArgs *args, void *stream);
/* The two networks' inputs in one launch: images uint8 RGB [B][H][W][3], boxes [B][P][3][4] -> hands [B P 2][3][S][S] (left before
 * right) and faces [B P][3][S][S], either NULL to skip it.  With s = side / S, crop pixel (u, v) samples the image at x = x0 + u' s,
 * y = y0 + v s, u' = S - 1 - u for a left hand (mirrored) and u otherwise; integer coordinates are pixel centres.  Bilinear over the
 * four neighbours, a neighbour outside the image counting 0: ax = x - floor(x), ay likewise,
 * val = (p00 (1 - ax) + p01 ax) (1 - ay) + (p10 (1 - ax) + p11 ax) ay; a sample that is not inside (-1, W) x (-1, H) is 0.  Channels
 * reversed to BGR, val / 256 - 0.5.  An invalid box's crop is all -0.5.  No anti-aliasing when side > S. */
int soar_part_crop(int32_t B, int32_t H, int32_t W, int32_t P, int32_t S, const uint8_t *images, const float *boxes, float *hands,
                   float *faces, void *stream);
/* heat [M][h][w][n_maps] (the last map, the background, is not read), boxes as above -> out [M][n_maps - 1][3] in image pixels.
 * which 0: hand crops, crop m belongs to rectangle m % 2 (0 left, mirrored; 1 right) of person m / 2; which 1: face crops, rectangle
 * 2 of person m.  One workgroup per (crop, map): the map upsampled by 8 with soar_pose_peaks' bicubic rule (never stored: the source
 * map lies in LDS, h w <= 12288), its maximum over all 8 h x 8 w positions, ties to the smallest raster index.  The winner (X, Y)
 * with value m > 0 in a valid rectangle gives (x0 + X' s, y0 + Y s, m) with s = side / (8 w) and X' = 8 w - 1 - X for a left hand;
 * anything else (0, 0, 0).  No sub-pixel refinement. */
int soar_part_keypoints(int32_t M, int32_t h, int32_t w, int32_t n_maps, const float *heat, const float *boxes, int32_t which, float *out,
                        void *stream);

const char *soar_last_error(void);
int soar_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SOAR_HIP_H */
