"""CPU tests of what the mesh-export entry points (csrc/mesh*.hip and the mesh half of csrc/body.hip) refuse before any launch: a
NULL, misaligned or too small workspace, and of their sizing calls.  No kernel runs here: the addresses are fakes that nothing
reads before the checks fail."""
import ctypes as C

import pytest

P = 0x1000                                  # any 256-byte aligned non-NULL address
V, F = 81, 128                              # the 9 x 9 grid of tests/mesh_holes_ref.py; every call admits them
X, Y, Z = 5, 6, 7


def _lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


# name -> (sizing call, arguments as (key, value) in the call's order; "ws" / "nb" are the workspace and its size, "counts" the
# host array the call fills, with its length)
CALLS = {
    "soar_mc_count": ("soar_mc_workspace_bytes", [("X", X), ("Y", Y), ("Z", Z), ("values", P), ("valid", None), ("level", 0.0), ("ws", P),
                                                  ("nb", 0), ("counts", 2), ("st", None)]),
    "soar_mc_emit": ("soar_mc_workspace_bytes", [("X", X), ("Y", Y), ("Z", Z), ("values", P), ("valid", None), ("level", 0.0), ("ws", P),
                                                 ("nb", 0), ("verts", 2 * P), ("faces", 3 * P), ("st", None)]),
    "soar_mesh_filter_components": ("soar_mesh_filter_bytes", [("V", V), ("F", F), ("verts", P), ("faces", P), ("min_faces", 64),
                                                               ("frac", 0.2), ("ws", P), ("nb", 0), ("vo", 2 * P), ("fo", 3 * P),
                                                               ("counts", 2), ("st", None)]),
    "soar_mesh_simplify_count": ("soar_mesh_simplify_bytes", [("V", V), ("F", F), ("verts", P), ("faces", P), ("cell", 0.1), ("ws", P),
                                                              ("nb", 0), ("counts", 2), ("st", None)]),
    "soar_mesh_simplify": ("soar_mesh_simplify_bytes", [("V", V), ("F", F), ("verts", P), ("faces", P), ("cell", 0.1), ("ws", P), ("nb", 0),
                                                        ("vo", 2 * P), ("fo", 3 * P), ("counts", 2), ("st", None)]),
    "soar_mesh_prune": ("soar_mesh_prune_bytes", [("V", V), ("F", F), ("verts", P), ("faces", P), ("quality", P), ("thresh", 0.5), ("ws", P),
                                                  ("nb", 0), ("vo", 2 * P), ("fo", 3 * P), ("keep", 4 * P), ("counts", 2), ("st", None)]),
    "soar_mesh_adjacency": ("soar_mesh_adjacency_bytes", [("V", V), ("F", F), ("faces", P), ("ws", P), ("nb", 0), ("rows", 2 * P),
                                                          ("nbr", 3 * P), ("border", 4 * P), ("st", None)]),
    "soar_mesh_smooth": ("soar_mesh_smooth_bytes", [("V", V), ("nnz", 6 * F), ("verts", P), ("rows", P), ("nbr", P), ("border", P),
                                                    ("steps", 3), ("ws", P), ("nb", 0), ("vo", 2 * P), ("st", None)]),
    "soar_mesh_subdivide_edges": ("soar_mesh_workspace_bytes", [("V", V), ("F", F), ("faces", P), ("ws", P), ("nb", 0), ("counts", 1),
                                                                ("st", None)]),
    "soar_mesh_vertex_normals": ("soar_mesh_workspace_bytes", [("V", V), ("F", F), ("verts", P), ("faces", P), ("weighting", 0), ("ws", P),
                                                               ("nb", 0), ("normals", 2 * P), ("st", None)]),
    "soar_mesh_atlas_levels": ("soar_mesh_atlas_bytes", [("V", V), ("F", F), ("verts", P), ("faces", P), ("ladder", P), ("n_ladder", 8),
                                                         ("ws", P), ("nb", 0), ("counts", 10), ("st", None)]),
    "soar_mesh_texel_offsets": ("soar_mesh_texels_bytes", [("V", V), ("F", F), ("T", 256), ("faces", P), ("cell", P), ("ws", P), ("nb", 0),
                                                           ("counts", 1), ("st", None)]),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_the_workspace_is_judged_before_any_launch(name):
    from soar_amd import hip_lib
    L = _lib()
    sizing, args = CALLS[name]
    n_counts = dict(args).get("counts", 0)
    counts = (C.c_int64 * max(n_counts, 1))(*([-5] * max(n_counts, 1)))

    def call(**kw):
        vals = [counts if k == "counts" else kw.get(k, d) for k, d in args]
        return getattr(L, name)(*vals)

    for kw, words in ((dict(ws=None), ["workspace"]), (dict(ws=P + 64), ["aligned"]), (dict(nb=0), ["need", sizing])):
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
