"""CPU tests of what every entry point that takes a caller's workspace refuses before any launch: a NULL, misaligned or too small
workspace (csrc/workspace.h: one carver and one check for all of them), and of the export path's sizing calls.  No kernel runs here:
the addresses are fakes that nothing reads before the checks fail."""
import ctypes as C

import pytest

P = 0x1000                                  # any 256-byte aligned non-NULL address
V, F = 81, 128                              # the 9 x 9 grid of tests/mesh_holes_ref.py; every call admits them
X, Y, Z = 5, 6, 7


def _lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def _struct(name, **fields):
    """-> a builder of hip_lib's args struct ``name``: scalars and pointers by name, a list fills an array field from its start"""
    def make():
        from soar_amd import hip_lib
        a = getattr(hip_lib, name)()
        for k, v in fields.items():
            if isinstance(v, list):
                for i, x in enumerate(v):
                    getattr(a, k)[i] = x
            else:
                setattr(a, k, v)
        return a
    return make


def _field_args():
    a = _struct("SoarFieldArgs", N=1, log2_T=1, normalized=1, res=[2.0] * 16, xyz=P, aabb=P, table=P, qtable=P, enc=P, qenc=P)()
    for h in a.head:
        h.w1 = h.b1 = h.w2 = h.b2 = P
    return a


def _jpeg_args():
    a = _struct("SoarJpegArgs", B=1, H=16, W=16, channels=3, subsampling=420, restart_interval=4, frames=P, frame_stride=768)()
    C.memset(a.qtables, 1, 128)
    return a


# configuration A of tests/sam_ref.py
_SAM = _struct("SoarSamConfig", image_size=112, patch=16, grid=7, embed=32, depth=4, heads=2, head_dim=16, mlp=64, out_chans=16,
               window=[3, 0, 3, 0], dec_layers=2, dec_heads=2, dec_down=2, dec_mlp=32, mask_tokens=4, hyper_depth=3, iou_depth=3, iou_hidden=16)
_VAE = _struct("SoarVaeArgs", N=1, H=8, W=8, image_size=8, weights=P)
_NORMALNET = _struct("SoarNormalNetArgs", N=1, H=4, W=4, ngf=8, n_down=1, n_blocks=0, image=P, prior_F=P, prior_B=P, weights_F=P, weights_B=P,
                     normal_F=P, normal_B=P)
_ENVMAP = _struct("SoarEnvmapArgs", B=1, H=4, W=4, dirs=P, w1=P, w2=P, w3=P)
_EVAL = _struct("SoarEvalArgs", N=1, H=7, W=7, pred=P, gt_rgb=P, gt_mask=P, gt_white=P, pred2=P, gt2=P, metrics=P)
_PNG = _struct("SoarPngArgs", B=1, H=16, W=16, channels=3, filter=-1, piece_bytes=64, images=P, image_stride=768)
_PNG_DECODE = _struct("SoarPngDecodeArgs", B=1, H=4, W=4, channels=3, total_bytes=100, data=P, offsets=P)
_JPEG_DECODE = _struct("SoarJpegDecodeArgs", B=2, H=17, W=33, channels=3, total_bytes=1000, data=P, offsets=P)


def _lpips(grads):
    return _struct("SoarLpipsArgs", N=1, H=16, W=16, grads=grads, in0=P, in1=P, weights=P)


# name -> (sizing call, its arguments, the call's arguments as (key, value) in the call's order; "ws" / "nb" are the workspace and
# its size, "counts" the host array the call fills, with its length).  A callable builds an args struct, filled so that the checks
# ahead of the workspace's pass.  A fourth entry is the alignment the call asks for where that is not 256 bytes.
CALLS = {
    "soar_mc_count": ("soar_mc_workspace_bytes", [X, Y, Z], [("X", X), ("Y", Y), ("Z", Z), ("values", P), ("valid", None), ("level", 0.0),
                                                             ("ws", P), ("nb", 0), ("counts", 2), ("st", None)]),
    "soar_mc_emit": ("soar_mc_workspace_bytes", [X, Y, Z], [("X", X), ("Y", Y), ("Z", Z), ("values", P), ("valid", None), ("level", 0.0),
                                                            ("ws", P), ("nb", 0), ("verts", 2 * P), ("faces", 3 * P), ("st", None)]),
    "soar_mesh_filter_components": ("soar_mesh_filter_bytes", [V, F], [("V", V), ("F", F), ("verts", P), ("faces", P), ("min_faces", 64),
                                                                       ("frac", 0.2), ("ws", P), ("nb", 0), ("vo", 2 * P), ("fo", 3 * P),
                                                                       ("counts", 2), ("st", None)]),
    "soar_mesh_simplify_count": ("soar_mesh_simplify_bytes", [V, F], [("V", V), ("F", F), ("verts", P), ("faces", P), ("cell", 0.1), ("ws", P),
                                                                      ("nb", 0), ("counts", 2), ("st", None)]),
    "soar_mesh_simplify": ("soar_mesh_simplify_bytes", [V, F], [("V", V), ("F", F), ("verts", P), ("faces", P), ("cell", 0.1), ("ws", P),
                                                                ("nb", 0), ("vo", 2 * P), ("fo", 3 * P), ("counts", 2), ("st", None)]),
    "soar_mesh_prune": ("soar_mesh_prune_bytes", [V, F], [("V", V), ("F", F), ("verts", P), ("faces", P), ("quality", P), ("thresh", 0.5),
                                                          ("ws", P), ("nb", 0), ("vo", 2 * P), ("fo", 3 * P), ("keep", 4 * P), ("counts", 2),
                                                          ("st", None)]),
    "soar_mesh_close_holes": ("soar_mesh_close_holes_bytes", [V, F], [("V", V), ("F", F), ("verts", P), ("faces", P), ("max_hole_edges", 100),
                                                                      ("ws", P), ("nb", 0), ("vo", 2 * P), ("fo", 3 * P), ("loops", 4 * P),
                                                                      ("counts", 4), ("st", None)]),
    "soar_mesh_attr_transfer": ("soar_mesh_attr_transfer_bytes", [V, 4], [("V", V), ("N", 9), ("K", 4), ("verts", P), ("points", P),
                                                                          ("colors", P), ("idx", P), ("ws", P), ("nb", 0), ("co", 2 * P),
                                                                          ("qo", 3 * P), ("d2", None), ("st", None)]),
    "soar_mesh_adjacency": ("soar_mesh_adjacency_bytes", [V, F], [("V", V), ("F", F), ("faces", P), ("ws", P), ("nb", 0), ("rows", 2 * P),
                                                                  ("nbr", 3 * P), ("border", 4 * P), ("st", None)]),
    "soar_mesh_smooth": ("soar_mesh_smooth_bytes", [V], [("V", V), ("nnz", 6 * F), ("verts", P), ("rows", P), ("nbr", P), ("border", P),
                                                         ("steps", 3), ("ws", P), ("nb", 0), ("vo", 2 * P), ("st", None)]),
    "soar_mesh_subdivide_edges": ("soar_mesh_workspace_bytes", [F], [("V", V), ("F", F), ("faces", P), ("ws", P), ("nb", 0), ("counts", 1),
                                                                     ("st", None)]),
    "soar_mesh_vertex_normals": ("soar_mesh_workspace_bytes", [F], [("V", V), ("F", F), ("verts", P), ("faces", P), ("weighting", 0),
                                                                    ("ws", P), ("nb", 0), ("normals", 2 * P), ("st", None)]),
    "soar_mesh_atlas_levels": ("soar_mesh_atlas_bytes", [F], [("V", V), ("F", F), ("verts", P), ("faces", P), ("ladder", P), ("n_ladder", 8),
                                                              ("ws", P), ("nb", 0), ("counts", 10), ("st", None)]),
    "soar_mesh_texel_offsets": ("soar_mesh_texels_bytes", [F], [("V", V), ("F", F), ("T", 256), ("faces", P), ("cell", P), ("ws", P),
                                                                ("nb", 0), ("counts", 1), ("st", None)]),
    # K = 30 neighbours of J = 55 joints: the path that sorts the queries in the workspace
    "soar_lbs_knn_query": ("soar_lbs_knn_query_bytes", [1], [("grid", P), ("V", V), ("vw", P), ("J", 55), ("xyz", P), ("P", 1), ("K", 30),
                                                             ("wo", 2 * P), ("io", None), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_vae_forward": ("soar_vae_workspace_bytes", [1, 8, 8, 8], [("a", _VAE), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_vae_backward": ("soar_vae_workspace_bytes", [1, 8, 8, 8], [("a", _VAE), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_lpips_forward": ("soar_lpips_workspace_bytes", [1, 16, 16, 0], [("a", _lpips(0)), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_lpips_backward": ("soar_lpips_workspace_bytes", [1, 16, 16, 3], [("a", _lpips(3)), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_normalnet_forward": ("soar_normalnet_workspace_bytes", [1, 4, 4, 8, 1, 0], [("a", _NORMALNET), ("ws", P), ("nb", 0), ("st", None)]),
    # soar_sam_workspace_bytes answers the larger of the encoder's and the decoder's needs: without points the encoder's, with the
    # most points a frame admits the decoder's (test_the_workspace_is_judged_before_any_launch makes sure of both)
    "soar_sam_encode": ("soar_sam_workspace_bytes", [_SAM, 1, 0], [
        ("cfg", _SAM), ("packed", P), ("a", _struct("SoarSamEncodeArgs", B=1, block_begin=0, block_end=4, patches=P, tokens_out=P)),
        ("ws", P), ("nb", 0), ("st", None)]),
    "soar_sam_decode": ("soar_sam_workspace_bytes", [_SAM, 1, 58], [
        ("cfg", _SAM), ("packed", P), ("a", _struct("SoarSamDecodeArgs", B=1, max_points=58, scale_x=1.0, scale_y=1.0, embeddings=P, points=P,
                                                    labels=P, counts=P, low_res=P, iou=P)),
        ("ws", P), ("nb", 0), ("st", None)]),
    "soar_masks_open_close": ("soar_masks_workspace_bytes", [1, 4, 4], [("N", 1), ("K", 1), ("H", 4), ("W", 4), ("cand", P), ("dtype", 0),
                                                                        ("thr", 0.5), ("out", 2 * P), ("stats", 3 * P), ("ws", P), ("nb", 0),
                                                                        ("st", None)]),
    "soar_masks_largest_component": ("soar_masks_workspace_bytes", [1, 4, 4], [("N", 1), ("H", 4), ("W", 4), ("mask", P), ("out", 2 * P),
                                                                               ("stats", 3 * P), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_masks_clean": ("soar_masks_workspace_bytes", [1, 4, 4], [("N", 1), ("K", 1), ("H", 4), ("W", 4), ("cand", P), ("dtype", 0),
                                                                   ("thr", 0.5), ("out", 2 * P), ("stats", 3 * P), ("ws", P), ("nb", 0),
                                                                   ("st", None)]),
    "soar_field_backward": ("soar_field_workspace_bytes", [1], [("a", _field_args), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_envmap_backward": ("soar_envmap_workspace_bytes", [1, 4, 4], [("a", _ENVMAP), ("ws", P), ("nb", 0), ("st", None)]),
    # one block of doubles: 8-byte alignment is all the regularizers ask for
    "soar_surfel_regularizers": ("soar_surfel_regularizers_workspace_bytes", [1], [
        ("P", 1), ("S", 3), ("K", 3), ("xyz", P), ("pos", P), ("scaling", P), ("opacity", P), ("scales", P), ("coef", P), ("up", P),
        ("terms", 2 * P), ("g_xyz", None), ("g_op", None), ("g_sc", None), ("ws", P), ("nb", 0), ("st", None)], 8),
    "soar_eval_image_metrics": ("soar_eval_scratch_bytes", [1, 7, 7], [("a", _EVAL), ("ws", P), ("nb", 0), ("st", None)]),
    "soar_png_measure": ("soar_png_workspace_bytes", [_PNG], [("a", _PNG), ("ws", P), ("nb", 0), ("offsets", 2 * P), ("st", None)]),
    "soar_png_emit": ("soar_png_workspace_bytes", [_PNG], [("a", _PNG), ("ws", P), ("nb", 0), ("out", 2 * P), ("cap", 16), ("st", None)]),
    "soar_jpeg_measure": ("soar_jpeg_workspace_bytes", [_jpeg_args], [("a", _jpeg_args), ("ws", P), ("nb", 0), ("offsets", 2 * P),
                                                                       ("st", None)]),
    "soar_jpeg_emit": ("soar_jpeg_workspace_bytes", [_jpeg_args], [("a", _jpeg_args), ("ws", P), ("nb", 0), ("out", 2 * P), ("cap", 16),
                                                                    ("st", None)]),
    "soar_png_decode": ("soar_png_decode_workspace_bytes", [_PNG_DECODE], [("a", _PNG_DECODE), ("ws", P), ("nb", 0), ("out", 2 * P),
                                                                            ("status", 3 * P), ("segments", 4 * P), ("st", None)]),
    "soar_jpeg_decode": ("soar_jpeg_decode_workspace_bytes", [_JPEG_DECODE], [("a", _JPEG_DECODE), ("ws", P), ("nb", 0), ("out", 2 * P),
                                                                               ("status", 3 * P), ("intervals", 4 * P), ("st", None)]),
}


def _sizing(L, sizing, sizes):
    from soar_amd import hip_lib
    return hip_lib._bytes(getattr(L, sizing), sizing, *[s() if callable(s) else s for s in sizes])


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_workspace_is_judged_before_any_launch(name):
    from soar_amd import hip_lib
    L = _lib()
    sizing, sizes, args, align = (CALLS[name] + (256,))[:4]
    need = _sizing(L, sizing, sizes)
    assert need > 0, (name, need)
    if sizing == "soar_sam_workspace_bytes":
        # a point more changes the decoder's need (its MLP's hidden block) and not the answer: the answer is the encoder's need
        assert _sizing(L, sizing, [_SAM, 1, 1]) == _sizing(L, sizing, [_SAM, 1, 0])
        # with 58 points the answer has grown: it is the decoder's need
        assert _sizing(L, sizing, [_SAM, 1, 58]) > _sizing(L, sizing, [_SAM, 1, 0])
    n_counts = dict(args).get("counts", 0)
    counts = (C.c_int64 * max(n_counts, 1))(*([-5] * max(n_counts, 1)))
    held = [v() if callable(v) else v for _, v in args]          # the structs live as long as the calls

    def call(**kw):
        vals = [counts if k == "counts" else kw.get(k, d) for (k, _), d in zip(args, held)]
        return getattr(L, name)(*vals)

    for kw, words in ((dict(ws=None), ["workspace"]), (dict(ws=P + (64 if align == 256 else align // 2)), ["aligned"]),
                      (dict(nb=need - 1), ["need", str(need), f"of {need - 1} bytes", sizing])):
        assert call(**kw) != 0, (name, kw)
        msg = hip_lib.last_error()
        assert all(w in msg for w in words), (name, kw, msg)
    assert list(counts) == [-5] * len(counts)


# every sizing call of the export path, and how it takes a mesh of V vertices and F faces (None: it does not admit that mesh)
SIZING = {
    "soar_mesh_filter_bytes": lambda v, f: (v, f) if f > 0 else None,
    "soar_mesh_simplify_bytes": lambda v, f: (v, f),
    "soar_mesh_attr_transfer_bytes": lambda v, f: (v, 4),
    "soar_mesh_adjacency_bytes": lambda v, f: (v, f),
    "soar_mesh_smooth_bytes": lambda v, f: (v,),
    "soar_mesh_prune_bytes": lambda v, f: (v, f),
    "soar_mesh_close_holes_bytes": lambda v, f: (v, f),
    "soar_mesh_atlas_bytes": lambda v, f: (f,) if f > 0 else None,
    "soar_mesh_texels_bytes": lambda v, f: (f,) if f > 0 else None,
    "soar_mesh_workspace_bytes": lambda v, f: (f,),
}


def test_the_sizing_calls():
    L = _lib()
    n = C.c_size_t(0)
    seen = 0
    for v, f in ((1, 0), (12, 20), (257, 510)):
        for name, sizes in SIZING.items():
            a = sizes(v, f)
            if a is None:
                continue
            n.value = 0
            assert getattr(L, name)(*a, C.byref(n)) == 0, (name, a)
            assert n.value % 256 == 0 and n.value > 0, (name, a, n.value)
            seen += 1
    assert seen == 3 * len(SIZING) - 3
    for dims in ((1, 1, 1), (X, Y, Z)):
        n.value = 0
        assert L.soar_mc_workspace_bytes(*dims, C.byref(n)) == 0
        assert n.value % 256 == 0 and n.value > 0, (dims, n.value)
