"""Every caller-owned workspace held to its contract on the device ("What a workspace may hold"; tests/workspace_guard.py).

One case per Python module; a case calls every entry point of its module that takes a workspace, at the smallest shapes at which the
module's own GPU test runs off its tile grid, with that test's inputs.  A case runs four times: as the rest of the suite runs it, and
inside ``guarded("zeros")``, ``guarded("ones")`` and ``guarded("noise")``, where every workspace lies between two 64 KB bands of 0xA5,
has exactly the size its sizing call answered and starts as zeros, as 0xFF bytes (NaN as float and double, -1 as int32, the largest
unsigned counter) or as seeded noise.  Held: the bands are intact after every run (nothing is written outside
``[base, base + bytes)``); every float output is finite; the outputs under 0xFF and under noise equal those under zeros bit for bit
(nothing is read that this call did not write), and those equal the run outside any context.  The one tolerance is the field's:
its two hash-table gradients are float atomics, and tests/test_field_gpu.py::test_reproducible holds two runs of them to
``_rel <= 1e-5``; that bound is taken from there.

That the bands see an overrun was shown once by hand and is not a test: ``guarded("zeros", shorten=256)`` turns the last 256 bytes of
every slice into guard band while the entry points are still told the full size; the UNet case then reports 16 dead bytes at the end
of its packed weights, the mesh case 100 at the end of the marching-cubes workspace.  (The rasterizer's four buffers pass even then:
their sizing calls answer one spare 256-byte block behind the last one carved.)

What was read in the carves (csrc/*.hip) before the first run, one line per case: the blocks a kernel uses as an index, count, offset
or flag, and what writes each before it is read.  Everything not named is floats or doubles.

unet_f32, unet_bf16, clip_text, clip_vision, resampler, sam, lpips, normalnet, field, envmap, regularizers, evaluate:
    activations, packed weights and partial sums only (unet.hip carve_ws, clip.hip, sam.hip, lpips.hip / normalnet.hip layouts,
    field.hip de / partial, envmap.hip and geometry.hip and eval.hip blocks of doubles): no block holds an address.
mesh:   marching cubes packed / info by mc_count_kernel for every voxel, offs by the scan, totals by mc_totals_kernel, and soar_mc_emit
    reads the same workspace; filter parent / fcount / bbox / gbox / ref / totals by filt_init_kernel, vkeep / fkeep for every vertex
    and face by the keep kernels, voff / foff by the scans (mesh_common.h compact_mesh); simplify box / totals by simp_init_kernel,
    used / pbeg / pend by simp_vhead_kernel, cid / cstart by simp_vassign_kernel, every key, index and flag array by the kernel in
    front of its sort or scan; adjacency bad by a memset, keys by adj_keys_kernel; prune totals by a memset, flags by
    prune_flags_kernel; close holes totals and n_out / n_in by memsets, arrive only read where n_in == 1 (then written), leader /
    rank / loop_n / cnt_* for every half-edge by holes_walk_kernel; attribute transfer bad by a memset; the grid of the K <= 8 search
    (lbs_knn.hip: meta by grid_meta_kernel, cell_range by a memset and grid_ranges_kernel, sorted_verts for every vertex), whose
    query workspace that search does not touch.  rocPRIM's sort and scan temporaries are initialised by rocPRIM.
texture: level by atlas_levels_kernel, hist and bad by memsets, classes by atlas_classes_kernel in soar_mesh_atlas_place (same
    workspace), keys / vals by atlas_keys_kernel; counts for F + 1 faces by texel_counts_kernel, offsets by the scan, bad by a memset.
body:   totals by a memset, keys by edge_keys_kernel / corner_keys_kernel, head / uid / ukeys by head_kernel, the scan, compact_kernel;
    soar_mesh_subdivide reads ukeys of the same workspace and checks every index against V (midpoints_kernel).
masks:  key by a memset, plane for every word by masks_pack_morph_kernel, parent only at run starts, which ccl_init_kernel writes.
png, jpeg: sizes[0 .. n] by the measure / entropy kernel (sizes[n] = 0 by piece 0), offs by the scan; emit reads the same workspace
    and checks offs against the capacity.  png also adler / payload / lens per piece by measure_kernel.
png_decode: rec by scan_kernel for every file, seg_start = -1 for each file's entries by scan_kernel; segment_of() refuses an entry
    whose file, index or range does not check out, so the entries no file owns are never followed; seg_out / seg_len checked
    against S before use.  jpeg_decode: rec / lo / len by parse_kernel for every file (n_int = 0 on failure), mark clamped to the
    file, coef by a memset.
densify: flags / packed for every point by densify_plan_kernel, offs by the scan, totals by densify_totals_kernel.
rasterizer: geometry header: H_KMAX.. by bucket_count_kernel, H_NVIS by bucket_scan_kernel, H_TOTAL / H_OVERFLOW / H_BAND_OVERFLOW /
    H_BIN_WORK by band_place_kernel, the violation count by preprocess; blk_stats, depth_key, tiles_touched, rect per Gaussian by
    preprocess; bucket_mat / bucket_base / sort_slot by bucket_count / bucket_scan; band_cnt for every (band, chunk) by
    band_count_kernel, band_info rows 2-3 by bucket_scan_kernel, rows 0-1 by band_place_kernel; image: tile_count / ranges zeroed by
    band_place_kernel, bin_work by the same, tile_order / order_rec / bg_state by tile_order_block, bg_tiles only read for a
    decision that SoarRastParams.debug bit 2 (not set here) enables; binning: band lists and tile lists written below the counts
    just named, block masks cleared by the launch in front of the blend; backward workspace zeroed by launch_zero_ranges.
    include/soar_hip.h: "A freshly allocated buffer must be cleared (one call with reset) before its first frame" speaks of the two
    running maxima behind the header that only soar_rast_binning_status_sticky reads; this path never makes that call, so the words
    stay poisoned like the rest.
"""
import pytest
import torch

from workspace_guard import FILLS, guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# case -> the sizing calls whose buffers it runs through the guard (plain data: tests/test_workspace_contract_cpu.py reads it)
CASES = {
    "unet_f32": ("soar_unet_weights_bytes", "soar_unet_workspace_bytes"),
    "unet_bf16": ("soar_unet_weights_bytes", "soar_unet_workspace_bytes"),
    "clip_text": ("soar_clip_weights_bytes", "soar_clip_workspace_bytes"),
    "clip_vision": ("soar_clip_weights_bytes", "soar_clip_workspace_bytes"),
    "resampler": ("soar_resampler_weights_bytes", "soar_resampler_workspace_bytes"),
    "sam": ("soar_sam_weights_bytes", "soar_sam_workspace_bytes"),
    "lpips": ("soar_lpips_weights_bytes", "soar_lpips_workspace_bytes"),
    "normalnet": ("soar_normalnet_weights_bytes", "soar_normalnet_workspace_bytes"),
    "field": ("soar_field_workspace_bytes",),
    "envmap": ("soar_envmap_workspace_bytes",),
    "regularizers": ("soar_surfel_regularizers_workspace_bytes",),
    "mesh": ("soar_mc_workspace_bytes", "soar_mesh_filter_bytes", "soar_mesh_simplify_bytes", "soar_mesh_adjacency_bytes",
             "soar_mesh_smooth_bytes", "soar_mesh_prune_bytes", "soar_mesh_close_holes_bytes", "soar_mesh_attr_transfer_bytes"),
    "texture": ("soar_mesh_atlas_bytes", "soar_mesh_texels_bytes"),
    "body": ("soar_mesh_workspace_bytes",),
    "masks": ("soar_masks_workspace_bytes",),
    "png": ("soar_png_workspace_bytes",),
    "jpeg": ("soar_jpeg_workspace_bytes",),
    "png_decode": ("soar_png_decode_workspace_bytes",),
    "jpeg_decode": ("soar_jpeg_decode_workspace_bytes",),
    "evaluate": ("soar_eval_scratch_bytes",),
    "densify": ("soar_densify_plan_bytes",),
    "rasterizer": ("soar_rast_geometry_bytes", "soar_rast_image_bytes", "soar_rast_binning_bytes", "soar_rast_backward_workspace_bytes"),
}

_DIRECT = "allocated by torch.empty / torch.zeros directly, not through hip_lib._workspace"
NOT_COVERED = {
    "soar_lbs_knn_weights_bytes": _DIRECT + "; tests/test_lbs_knn_edges_gpu.py",
    "soar_lbs_knn_grid_bytes": _DIRECT + " on the skinning path (tests/test_lbs_knn_edges_gpu.py); the mesh and texture cases build a guarded grid for their K <= 8 search",
    "soar_lbs_knn_query_bytes": _DIRECT + " on the skinning path (tests/test_lbs_knn_edges_gpu.py); the K <= 8 search of the mesh and texture cases is handed one and does not touch it",
    "soar_lbs_knn_state_bytes": _DIRECT + "; tests/test_lbs_knn_edges_gpu.py",
    "soar_ssim_scratch_floats": _DIRECT + " (losses.py)",
    "soar_image_loss_scratch_floats": _DIRECT + " (losses.py)",
    "soar_avatar_loss_scratch_floats": _DIRECT + " (step_plan.py)",
    "soar_views_grad_scratch_floats": _DIRECT + " (renderer/fused_view.py)",
    "soar_step_terms_scratch_bytes": _DIRECT + " (step_losses.py)",
    "soar_view_buffer_bytes": "one pool of renderer/fused_view.py, which binds the rasterizer's allocator at import: guarded() does not reach it",
    "soar_normal_crop_bytes": "not a sizing call: it turns normals into bytes and takes no workspace",
    "soar_vae_weights_floats": "the VAE: tests/test_sds_gpu.py::test_workspace_contents_do_not_matter_and_its_neighbours_stay_untouched",
    "soar_vae_weights_bytes": "the VAE: tests/test_sds_gpu.py::test_workspace_contents_do_not_matter_and_its_neighbours_stay_untouched",
    "soar_vae_workspace_bytes": "the VAE: tests/test_sds_gpu.py::test_workspace_contents_do_not_matter_and_its_neighbours_stay_untouched",
}

# tests/test_field_gpu.py::test_reproducible: the scatter into the hash tables is float atomics; two runs are held to _rel <= 1e-5
FIELD_TABLE_REL = 1e-5
# outputs that are not compared between runs, only held finite: the rasterizer's default backward sums with float32 atomics in the
# hardware's order, and tests/test_rasterizer_gpu.py compares two runs only in the order-insensitive mode, which the case runs as well
FINITE_ONLY_PREFIX = "float32 atomics/"


def _t(a, **kw):
    return torch.as_tensor(a, **kw).to(DEV)


def _unet(precision):
    import unet_ref as R
    from soar_amd import unet
    cfg = R.CONFIG_A
    net = unet.MultiviewUNet(R.tiny_state_dict(cfg, 0), num_head_channels=cfg["num_head_channels"], ip_dim=cfg["ip_dim"],
                             ip_weight=cfg["ip_weight"], n_view=cfg["n_view"], precision=precision).to(DEV)
    x, t, ctx, cam, ip = (None if v is None else v.to(DEV) for v in R.inputs(cfg, 0))
    return {"eps": net(x, t, ctx, camera=cam, ip_tokens=ip)}


def case_unet_f32():
    return _unet("f32")


def case_unet_bf16():
    return _unet("bf16")


def case_clip_text():
    import clip_ref as R
    from soar_amd import clip
    cfg = R.TEXT_A
    net = clip.ClipTextEncoder(R.tiny_state_dict(R.text_shapes(cfg), 10), heads=cfg["heads"]).to(DEV)
    ids = torch.randint(0, cfg["vocab"], (2, 13), generator=torch.Generator().manual_seed(1300))
    return {"tokens": net(ids.to(DEV))}


def case_clip_vision():
    import clip_ref as R
    from soar_amd import clip
    cfg = R.VISION_A
    net = clip.ClipImageEncoder(R.tiny_state_dict(R.vision_shapes(cfg), 20), heads=cfg["heads"]).to(DEV)
    img = torch.stack([R.sample_image(41, 59, 3 + b) for b in range(2)])
    return {"tokens": net(img.to(DEV))}


def case_resampler():
    import clip_ref as R
    from soar_amd import clip
    cfg = R.RESAMPLER_A
    net = clip.Resampler(R.tiny_state_dict(R.resampler_shapes(cfg), 30), dim_head=cfg["dim_head"]).to(DEV)
    x = torch.randn(2, 26, cfg["emb"], generator=torch.Generator().manual_seed(26))
    return {"tokens": net(x.to(DEV))}


def case_sam():
    import numpy as np
    import sam_ref
    from soar_amd import sam
    cfg = sam_ref.CONFIG_A
    seg = sam.SamSegmenter(sam_ref.tiny_state_dict(cfg, 0), decoder_heads=cfg["dec_heads"]).to(DEV)
    H, W = 90, 160
    img = _t(sam_ref.synthetic_frame(H, W, 0))[None]
    pts = _t(np.asarray([[80, 45], [70, 30], [90, 60], [75, 50], [85.5, 40.25]], np.float32))[None]
    lab = _t(np.asarray([1, 1, 0, 1, 1]), dtype=torch.int32)[None]
    emb = seg.embed(img)
    low5, iou5 = seg.decode(emb, pts, None, (H, W), lab)
    low0, iou0 = seg.decode(emb, pts[:, :0], None, (H, W))
    return {"embeddings": emb, "low_res 5 points": low5, "iou 5 points": iou5, "low_res 0 points": low0, "iou 0 points": iou0}


def case_lpips():
    import lpips_ref as R
    from soar_amd.lpips import LPIPSVGG
    m = LPIPSVGG(R.lpips_state_dict(R.random_weights(0))).to(DEV)
    a = R.normal_images(2, 23, 37, 5)
    b = (a + 0.3 * R.normal_images(2, 23, 37, 105)).clamp(-1, 1)
    x, y = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    v = m(x, y)
    (v.view(-1) * _t([1.0, -0.5])).sum().backward()
    return {"value": v.detach(), "g_in0": x.grad, "g_in1": y.grad}


def case_normalnet():
    import normalnet_ref as R
    from soar_amd import normals
    c = R.make_case("bottom2x2", DEV)
    out = normals.NormalNet(c["sd"], *c["cfg"]).to(DEV)(c["image"], c["prior_F"], c["prior_B"])
    return {f"normal {i}": t for i, t in enumerate(out)}


def case_field():
    import test_field_gpu as T
    from soar_amd import synthetic as syn
    n = 257
    xyz = syn.make_surfels(n, 0).xyz
    f = T._field(T._aabb(xyz), seed=3)
    z = torch.tensor([0.1, 0.2], device=DEV, requires_grad=True)
    out, g = T._run_hip(f, xyz.to(DEV).contiguous(), z, T._upstream("all", n), True)
    res = {h: t.detach() for h, t in out.items()}
    res.update({"d " + k: t for k, t in g.items() if t is not None})
    return res


def case_envmap():
    from soar_amd.background import NeuralEnvironmentMapBackground as Env
    B, NC, H, W = 3, 2, 23, 37
    torch.manual_seed(0)
    m = Env({"random_aug": False}).to(DEV)
    g = torch.Generator().manual_seed(1)
    d = torch.randn(B, H, W, 3, generator=g)
    d = (d / d.norm(dim=-1, keepdim=True) * (0.5 + torch.rand(B, H, W, 1, generator=g))).to(DEV)
    r = torch.rand(NC, 3, H, W, generator=g).to(DEV).requires_grad_(True)
    k = (torch.rand(NC, 1, H, W, generator=g) * (torch.rand(NC, 1, H, W, generator=g) > 0.3)).to(DEV).requires_grad_(True)
    G, Gb = torch.randn(NC, H, W, 3, generator=g).to(DEV), torch.randn(1, H, W, 3, generator=g).to(DEV)
    comp, bg = m.composite(d, r, k, NC)
    ((comp * G).sum() + (bg[[-1]] * Gb).sum()).backward()
    res = {"comp": comp.detach(), "bg": bg.detach(), "background alone": m(d).detach(), "g_render": r.grad, "g_mask": k.grad}
    res.update({f"d_w{i}": m.network.layers[i].weight.grad for i in (0, 2, 4)})
    return res


def case_regularizers():
    import test_geometry_gpu as T
    from soar_amd.geometry import surfel_regularizers
    raw, _ = T.reg_inputs(4099, 3, 1, seed=4103)
    ins = [t.detach().clone() for t in raw]
    for k in (0, 2, 3, 4):
        ins[k].requires_grad_(True)
    loss, terms = surfel_regularizers(*ins, T.ALL)
    (loss * 1.7).backward()
    res = {"loss": loss.detach(), "terms": terms.detach()}
    res.update({f"d input {k}": ins[k].grad for k in (0, 3, 4)})
    return res


def case_mesh():
    import mesh_attr_ref as A
    import mesh_cases as MC
    import mesh_holes_ref as H
    import mesh_simplify_ref as S
    from soar_amd import mesh
    res = {}
    f, valid = MC.mc_field("xyz")
    res["mc verts"], res["mc faces"] = mesh.marching_cubes(_t(f), 0.0, _t(valid))
    c = MC.sized_case(257, 255, 74)
    res["filter verts"], res["filter faces"] = mesh.filter_components(_t(c.verts), _t(c.faces), min_faces=c.min_faces, min_diag_frac=c.min_diag_frac)
    c = next(c for c in S.cases() if c.name == "icosphere2_R4")
    res["simplify verts"], res["simplify faces"] = mesh.simplify(mesh.Mesh(_t(c.verts), _t(c.faces)), c.cell)
    # (the counting entry point: many cell sizes through one workspace, each after the other's remains)
    res["decimate verts"], res["decimate faces"] = mesh.decimate(mesh.Mesh(_t(c.verts), _t(c.faces)), target_faces=100)
    fx = next(fx for fx in A.fixtures() if fx.name == "disc257")
    m = mesh.Mesh(_t(fx.verts), _t(fx.faces))
    pts, col = A.surfels()
    res["color"], quality, res["idx"] = mesh.vertex_attributes(m.vertices, _t(pts), _t(col), k=4)
    res["quality"] = quality
    res["row_start"], res["nbr"], res["border"] = mesh.adjacency(m)
    res["smooth verts"] = mesh.smooth(m, 3).vertices
    pruned, res["prune keep"] = mesh.prune_by_quality(m, quality, float(quality.median()))
    res["prune verts"], res["prune faces"] = pruned.vertices, pruned.faces
    fx = H.fixture("a")
    closed, res["closed loops"] = mesh.close_holes(mesh.Mesh(_t(fx.verts), _t(fx.faces)), 300)
    res["holes verts"], res["holes faces"] = closed.vertices, closed.faces
    return res


def case_texture():
    import test_texture_gpu as T
    import texture_ref as R
    from soar_amd import mesh
    fx = R.fixture("g")
    m = T._mesh(fx)
    atlas = mesh.build_atlas(m, 16)
    pts, col = T._surfels(fx)
    texture, debug = mesh.bake_texture(m, atlas, pts, col, k=4, return_debug=True)
    res = {"uv": atlas.uv, "uv_faces": atlas.uv_faces, "cell": atlas.cell, "texture": texture}
    res.update(debug)
    return res


def case_body():
    import body_ref as R
    from soar_amd import body
    v, f = R.open_strip()
    v, f = _t(v), _t(f)
    sv, sf = body.subdivide(v, f, 1)
    return {"subdivided verts": sv, "subdivided faces": sf, "normals": body.vertex_normals(v, f, "angle")}


def case_masks():
    import masks_ref as R
    from soar_amd import masks
    H, W, sigma = R.BLOB_SHAPES[0]                       # 37 x 70: neither a multiple of the 32-pixel words nor of the tiles
    mask = R.blobs(H, W, sigma, R.NOISE_SEEDS[0])
    cand = _t(R.split_candidates(mask, 3, R.NOISE_SEEDS[0]))[None]
    res = {}
    for name, fn, x in (("open_close", masks.open_close, cand), ("largest", masks.largest_component, _t(mask.astype("uint8"))[None]),
                        ("clean", masks.clean_masks, cand)):
        res[name], res[name + " stats"] = fn(x, return_stats=True)
    return res


def _png():
    import test_png_cpu as T
    from soar_amd.png import encode_png
    H, W, C = 17, 23, 3
    data, offsets = encode_png(_t(T.make_image("blob", H, W, C))[None], filters="adaptive", piece_bytes=32)
    return (H, W, C), {"data": data, "offsets": offsets}


def case_png():
    return _png()[1]


def case_png_decode():
    from soar_amd.png import decode_png
    shape, res = _png()
    return {"image": decode_png(res["data"], res["offsets"], *shape)}


def _jpeg():
    import test_video_cpu as T
    from soar_amd.video import encode_jpeg
    H, W = 17, 23
    data, offsets = encode_jpeg(_t(T.make_image("noise", H, W))[None], quality=90, subsampling="420", restart_interval=3)
    return (H, W, 3), {"data": data, "offsets": offsets}


def case_jpeg():
    return _jpeg()[1]


def case_jpeg_decode():
    from soar_amd.jpeg import decode_jpeg
    shape, res = _jpeg()
    return {"image": decode_jpeg(res["data"], res["offsets"], *shape)}


def case_evaluate():
    import eval_ref as R
    from soar_amd import evaluate
    out = evaluate.image_metrics(*[_t(a) for a in R.make_case(1, 23, 37)], grid=True)
    return {k: v for k, v in out.items() if v is not None}


def case_densify():
    import densify_cases as dc
    from oracle import densify_oracle as do
    from soar_amd.densify import SurfelDensifier
    # (designated=False: the designated rows hold a zero rotation, whose split children are NaN by construction)
    case = dc.make_case(257, 15, designated=False)
    st = dc.oracle_state(case)
    dc.accumulate(case, st)
    d = SurfelDensifier({k: torch.nn.Parameter(case.params[k].clone().to(DEV)) for k in do.PARAMS}, None, percent_dense=case.percent_dense,
                        surface=case.surface)
    d.accum.copy_(dc.accum_matrix(st).to(DEV))
    res = {"flags": d.flags(True, True, case.min_opacity, case.extent, case.max_grad)}
    counts = d.prune_and_densify(case.min_opacity, case.max_grad, case.extent, noise=case.noise)
    assert counts["pruned"] and counts["split"] and counts["cloned"], counts
    res.update({k: d.params[k].detach() for k in do.PARAMS})
    return res


def case_rasterizer():
    import scenes as S
    from soar_amd import rasterizer
    scene = S.blob_scene()
    st = S.torch_settings(scene, DEV)
    grads = [_t(g) for g in S.upstream_grads(scene)]
    res = {}
    was = rasterizer.DETERMINISTIC_BACKWARD
    try:
        for exact in (True, False):
            rasterizer.DETERMINISTIC_BACKWARD = exact
            leaves = {k: _t(getattr(scene, k), dtype=torch.float32).requires_grad_(True) for k in ("means3D", "opacities", "colors", "scales", "rotations")}
            means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
            out = rasterizer.GaussianRasterizer(st)(leaves["means3D"], means2D, leaves["opacities"], colors_precomp=leaves["colors"],
                                                    scales=leaves["scales"], rotations=leaves["rotations"])
            sum((o * g).sum() for o, g in zip(out[:4], grads)).backward()
            pre = "" if exact else FINITE_ONLY_PREFIX
            if exact:
                res.update({k: t.detach() for k, t in zip(("color", "normal", "depth", "opac", "radii"), out)})
            res.update({pre + "d " + k: t.grad for k, t in leaves.items()})
            res[pre + "d means2D"] = means2D.grad
    finally:
        rasterizer.DETERMINISTIC_BACKWARD = was
    return res


def _run(name, fill=None):
    fn = globals()["case_" + name]
    if fill is None:
        out = fn()
        torch.cuda.synchronize()
        return out
    with guarded(fill) as g:
        out = fn()
        g.check()
        assert g.buffers, f"{name}: no workspace came through the guard"
    return out


def _same(case, name, got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (case, name, what)
    if name.startswith(FINITE_ONLY_PREFIX):
        return
    if case == "field" and "hash_table" in name:
        rel = float((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-300))
        assert rel <= FIELD_TABLE_REL, f"{case}: {name} {what}: relative L2 distance {rel:.3g} > {FIELD_TABLE_REL}"
        return
    if not torch.equal(got, want):
        diff = (got != want).nonzero()
        raise AssertionError(f"{case}: {name} {what}: {diff.shape[0]} of {got.numel()} elements differ, the first at {diff[0].tolist()}: "
                             f"{got[tuple(diff[0])].item()!r} against {want[tuple(diff[0])].item()!r}")


@pytest.mark.parametrize("name", list(CASES))
def test_workspace_contract(name):
    plain = _run(name)
    runs = {fill: _run(name, fill) for fill in FILLS}
    for fill, out in runs.items():
        assert list(out) == list(plain), (name, fill)
        for k, t in out.items():
            if t.is_floating_point():
                bad = int((~torch.isfinite(t)).sum())
                assert bad == 0, f"{name}: {k} has {bad} non-finite elements of {t.numel()} with the workspaces filled with {fill}"
    for k, t in runs["zeros"].items():
        _same(name, k, t, plain[k], "under zeros against the run outside the guard")
        for fill in ("ones", "noise"):
            _same(name, k, runs[fill][k], t, f"under {fill} against zeros")
