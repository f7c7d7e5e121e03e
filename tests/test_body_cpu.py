"""CPU tests of the avatar initialisation (soar_amd/body.py, csrc/body.hip): the restatements of tests/body_ref.py against the
golden vertices of the reference's own lbs() and against the invariants of midpoint subdivision, the argument checks of the C
entry points (nothing is launched), and the promise that SMPLGuidance is unchanged unless asked."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest
import torch

import body_ref as br

HERE = os.path.dirname(os.path.abspath(__file__))


def golden_body():
    g = np.load(os.path.join(HERE, "golden", "smplx_vertices.npz"))
    body = types.SimpleNamespace(v_template=torch.from_numpy(g["v_template"]), shapedirs=torch.from_numpy(g["shapedirs"]),
                                 posedirs=torch.from_numpy(br.posedirs_from_factors(g["posedirs_U"], g["posedirs_Wt"])),
                                 J_regressor=torch.from_numpy(g["J_regressor"]), parents=torch.from_numpy(g["parents"]),
                                 lbs_weights=torch.from_numpy(g["lbs_weights"]))
    return g, body


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_float64_restatement_reproduces_the_reference_vertices():
    g, body = golden_body()
    assert float(body.posedirs.abs().max()) > 1e-2                       # the correctives are exercised
    v = br.lbs_vertices(body, g["betas"], g["pose"], g["transl"], torch.float64).numpy()
    assert v.shape == g["verts_f64"].shape == (4, 96, 3)
    assert np.abs(v - g["verts_f64"]).max() <= 1e-12
    # and the float32 composition sits where the reference's own float32 run sits
    v32 = br.lbs_vertices(body, g["betas"], g["pose"], g["transl"], torch.float32).numpy()
    assert br.worst(v32, g["verts_f64"]) <= 4 * max(br.worst(g["verts_f32"], g["verts_f64"]), br.FLOOR)
    # without the correctives the vertices differ: the golden would catch a forward that drops them
    body0 = types.SimpleNamespace(**{**vars(body), "posedirs": torch.zeros_like(body.posedirs)})
    assert np.abs(br.lbs_vertices(body0, g["betas"], g["pose"], g["transl"]).numpy() - g["verts_f64"]).max() > 1e-3


MESHES = {"closed": lambda: br.icosphere(2), "open": br.open_strip, "nonmanifold": br.nonmanifold}


@pytest.mark.parametrize("name", sorted(MESHES))
def test_subdivision_restatement_keeps_the_surface(name):
    v, f = MESHES[name]()
    v = v.astype(np.float64)
    V, E, F, area, nrm = br.mesh_stats(v, f)
    v2, f2 = br.subdivide_np(v, f)
    V2, E2, F2, area2, nrm2 = br.mesh_stats(v2, f2)
    assert V2 == V + E and F2 == 4 * F and f2.dtype == np.int32
    assert V2 - E2 + F2 == V - E + F                                     # Euler characteristic
    assert abs(area2 - area) <= 1e-12 * area
    assert np.abs((nrm2.reshape(F, 4, 3) * nrm[:, None]).sum(-1) - 1.0).max() <= 1e-12      # children parallel to their parent
    assert np.array_equal(v2[:V], v)
    # new vertices in ascending key order, each the midpoint of its edge
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1).astype(np.int64)
    keys = np.unique((e[:, 0] << 32) | e[:, 1])
    assert np.array_equal(v2[V:], (v[keys >> 32] + v[keys & 0xffffffff]) * 0.5)
    if name == "closed":
        assert V - E + F == 2
    # float32 midpoints are numpy's float32 (a + b) * 0.5
    v32 = v.astype(np.float32)
    w2, _ = br.subdivide_np(v32, f)
    assert w2.dtype == np.float32 and np.array_equal(w2[V:], (v32[keys >> 32] + v32[keys & 0xffffffff]) * np.float32(0.5))


@pytest.mark.parametrize("weighting", ["angle", "area", "uniform"])
def test_restated_normals_of_an_icosphere_point_outwards(weighting):
    v, f = br.icosphere(3)
    n = br.vertex_normals_np(v, f, weighting)
    # a vertex normal of a sphere's inscribed mesh deviates from the radius by at most the angle its faces subtend:
    # edge length h ~ 1.2 / 2^levels on the unit sphere, face normals tilt by <= h, so 1 - cos <= h^2 / 2
    h = 1.3 / 2 ** 3
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-12
    assert (1 - (n * v.astype(np.float64)).sum(-1)).max() <= 0.5 * h * h
    # frames: right-handed orthonormal, third column the normal
    rd = np.random.default_rng(0).standard_normal(n.shape)
    M = br.frames_np(n, rd)
    assert np.abs(M.transpose(0, 2, 1) @ M - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(M) - 1).max() <= 1e-12
    assert np.array_equal(M[:, :, 2], n)
    # degenerate inputs follow normalize's epsilon: a parallel rand_dir gives zero in-plane axes, an unused vertex a zero normal
    assert np.array_equal(br.frames_np(n[:4], 2.0 * n[:4])[:, :, :2], np.zeros((4, 3, 2)))
    v2, f2 = br.open_strip()
    assert np.array_equal(br.vertex_normals_np(v2, f2, weighting)[-2:], np.zeros((2, 3)))


def test_the_body_entry_points_refuse_bad_arguments_before_any_launch(lib):
    from soar_amd import hip_lib
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)           # any non-NULL address: nothing reads it before the checks fail
    err = hip_lib.last_error
    V = lib.soar_smplx_vertices
    assert V(4, 96, 55, 20, p, 1, p, p, None, p, p, p, None, p, None) != 0 and "NULL" in err()
    assert V(4, 96, 55, 20, p, 1, p, p, p, p, p, None, None, p, None) != 0 and "NULL" in err()
    assert V(4, 96, 55, 20, None, 1, p, p, p, p, p, p, None, p, None) != 0 and "NULL" in err()
    assert V(4, 96, 65, 20, p, 1, p, p, p, p, p, p, None, p, None) != 0 and "J=65" in err()
    assert V(4, 96, 1, 20, p, 1, p, p, p, p, p, p, None, p, None) != 0
    assert V(4, 96, 55, 20, p, 3, p, p, p, p, p, p, None, p, None) != 0 and "betas_batch" in err()
    assert V(-1, 96, 55, 20, p, 1, p, p, p, p, p, p, None, p, None) != 0 and V(4, -1, 55, 20, p, 1, p, p, p, p, p, p, None, p, None) != 0
    assert V(0, 96, 55, 20, p, 1, p, p, p, p, p, None, None, p, None) != 0            # B == 0 does not excuse a NULL pointer
    assert V(0, 96, 55, 20, p, 1, p, p, p, p, p, p, None, p, None) == 0               # ... with valid pointers: a no-op
    assert V(4, 0, 55, 20, p, 1, p, p, p, p, p, p, None, p, None) == 0
    n = C.c_size_t(0)
    assert lib.soar_mesh_workspace_bytes(20480, C.byref(n)) == 0 and n.value >= 3 * 20480 * (3 * 8 + 2 * 4) and n.value % 256 == 0
    assert lib.soar_mesh_workspace_bytes(-1, C.byref(n)) != 0 and lib.soar_mesh_workspace_bytes(4, None) != 0
    ws = C.c_void_p(0x1000)                           # aligned and never touched: every call below fails or has nothing to do
    E = C.c_int64(7)
    S = lib.soar_mesh_subdivide_edges
    assert S(10, 4, None, ws, n.value, C.byref(E), None) != 0 and "NULL" in err()
    assert S(10, 4, p, None, n.value, C.byref(E), None) != 0 and "workspace" in err()
    assert S(10, 4, p, C.c_void_p(0x1010), n.value, C.byref(E), None) != 0 and "aligned" in err()
    assert S(10, 4, p, ws, 16, C.byref(E), None) != 0 and "need" in err()
    assert S(10, 4, p, ws, n.value, None, None) != 0
    assert S(0, 4, p, ws, n.value, C.byref(E), None) != 0 and "outside" in err()      # faces without vertices: out of range
    assert S(-1, 4, p, ws, n.value, C.byref(E), None) != 0 and S(10, -1, p, ws, n.value, C.byref(E), None) != 0
    assert S(10, 0, p, ws, n.value, C.byref(E), None) == 0 and E.value == 0          # no faces: no edges, no launch
    D = lib.soar_mesh_subdivide
    assert D(10, 4, 5, None, p, ws, n.value, p, p, None) != 0 and "NULL" in err()
    assert D(10, 4, 5, p, p, ws, n.value, None, p, None) != 0 and "NULL" in err()
    assert D(10, 4, 13, p, p, ws, n.value, p, p, None) != 0 and "edge count" in err()
    assert D(10, 4, -1, p, p, ws, n.value, p, p, None) != 0
    assert D(10, 4, 5, p, p, ws, 16, p, p, None) != 0
    N = lib.soar_mesh_vertex_normals
    assert N(10, 4, p, None, 0, ws, n.value, p, None) != 0 and "NULL" in err()
    assert N(10, 4, p, p, 3, ws, n.value, p, None) != 0 and "weighting" in err()
    assert N(10, 4, p, p, 0, ws, n.value, None, None) != 0
    assert N(10, 4, p, p, 0, None, n.value, p, None) != 0
    assert N(0, 0, p, p, 0, ws, n.value, p, None) == 0
    Fr = lib.soar_mesh_vertex_frames
    assert Fr(10, p, None, p, None) != 0 and "NULL" in err()
    assert Fr(-1, p, p, p, None) != 0
    assert Fr(0, p, p, p, None) == 0


def test_python_api_refuses_cpu_tensors():
    from soar_amd import body
    g, gb = golden_body()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        body.smplx_vertices(gb, torch.from_numpy(g["betas"]), torch.from_numpy(g["pose"]))
    v, f = br.nonmanifold()
    for fn in (lambda: body.subdivide(torch.from_numpy(v), torch.from_numpy(f)),
               lambda: body.vertex_normals(torch.from_numpy(v), torch.from_numpy(f)),
               lambda: body.surfel_frames(torch.from_numpy(v))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()
    with pytest.raises(ValueError, match="weighting"):
        body.vertex_normals(torch.from_numpy(v), torch.from_numpy(f), weighting="cotangent")


def test_guidance_is_unchanged_unless_asked():
    """The avatar initialisation is an opt-in: the old arguments keep their places, the new ones default to off, and the class itself
    carries no query_points / init_q / cano_mesh (GaussianSurfelModel.create_from_pcd looks for them with getattr).  An object
    needs a device; tests/test_body_gpu.py checks the instance."""
    from soar_amd.smpl_guidance import SMPLGuidance
    sig = inspect.signature(SMPLGuidance.__init__)
    assert list(sig.parameters)[:5] == ["self", "body", "smpl_parms", "device", "leg_angle"]
    d = {k: p.default for k, p in sig.parameters.items()}
    assert d["faces"] is None and d["num_subdiv"] == 2 and d["pose_correctives"] is False and d["generator"] is None
    assert not any(hasattr(SMPLGuidance, a) for a in ("query_points", "init_q", "cano_mesh"))
