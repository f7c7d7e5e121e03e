"""CPU tests of the mesh export (soar_amd/mesh.py, csrc/mesh.hip): the generated marching-cubes table, the argument checks of
the new entry points (nothing is launched) and the OBJ writer."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_committed_table_is_the_generators_output():
    gen = R.load_generator()
    with open(os.path.join(R.CSRC, "mcubes_table.h")) as f:
        assert f.read() == gen.render()
    corner, tris = R.load_table()
    assert tris[0] == [] and tris[255] == []
    assert [len(t) for t in tris] == [len(t) for t in gen.table()]


def test_ambiguous_faces_never_connect_inside_corners():
    """Two inside corners diagonal on a face (corners 0 and 3 of the z = 0 face): each is cut off on its own, as two
    triangles, whatever the other corners -- the face-local rule that makes neighbouring cells agree."""
    corner, tris = R.load_table()
    assert len(tris[0b1001]) == 2
    assert len(tris[0b0110]) == 2
    # complement: the two OUTSIDE corners on the diagonal are connected (one quad strip through the cell)
    f = np.ones((2, 2, 2), np.float32)
    f[0, 0, 0] = f[1, 1, 0] = -1.0
    v, fc = R.marching_cubes(f)
    assert R.n_components(len(v), fc) == 2


@pytest.mark.parametrize("padded", [False, True], ids=["cube", "padded"])
def test_every_case_is_manifold_and_oriented(padded):
    for case in range(256):
        f = np.array([1.0 if not (case >> c) & 1 else -1.0 for c in range(8)], np.float32)
        cube = np.zeros((2, 2, 2), np.float32)
        for c in range(8):
            cube[c & 1, (c >> 1) & 1, (c >> 2) & 1] = f[c] * (1.0 + 0.1 * c)
        if padded:
            g = np.ones((4, 4, 4), np.float32)
            g[1:3, 1:3, 1:3] = cube
            cube = g
        v, fc = R.marching_cubes(cube)
        R.check_vertices_on_crossings(v, cube)
        R.check_closed_manifold(v, fc, None if padded else cube.shape)
        if padded and len(fc):
            # closed around the inside corners: positive volume means outward-facing triangles
            assert R.enclosed_volume(v, fc) > 0, case


@pytest.mark.parametrize("seed", range(20))
def test_random_fields_are_closed_manifolds(seed):
    f = np.random.default_rng(seed).standard_normal((12, 12, 12)).astype(np.float32)
    v, fc = R.marching_cubes(f)
    R.check_vertices_on_crossings(v, f)
    R.check_closed_manifold(v, fc, f.shape)


def test_random_field_with_a_validity_mask():
    rng = np.random.default_rng(7)
    f = rng.standard_normal((10, 10, 10)).astype(np.float32)
    valid = rng.uniform(size=f.shape) > 0.15
    v, fc = R.marching_cubes(f, valid=valid)
    R.check_vertices_on_crossings(v, f, valid=valid)
    # every triangle's cell has 8 valid corners
    for face in fc:
        lo = np.floor(v[face].min(0)).astype(int)
        assert valid[lo[0]:lo[0] + 2, lo[1]:lo[1] + 2, lo[2]:lo[2] + 2].all()


def test_sphere_field_orientation_and_euler():
    g = np.stack(np.meshgrid(*[np.arange(16.0)] * 3, indexing="ij"), -1)
    f = (np.linalg.norm(g - 7.3, axis=-1) - 5.0).astype(np.float32)
    v, fc = R.marching_cubes(f)
    R.check_closed_manifold(v, fc)
    assert R.euler_characteristic(v, fc) == 2
    vol = R.enclosed_volume(v, fc)
    assert abs(vol - 4 / 3 * np.pi * 125) < 0.05 * 4 / 3 * np.pi * 125


def test_new_entry_points_refuse_bad_arguments(lib):
    from soar_amd import hip_lib
    err = hip_lib.last_error
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)           # any non-NULL address: nothing reads it before the checks fail
    n = C.c_size_t(0)
    cnt = (C.c_int64 * 2)()
    args = lambda nv=2, H=8, W=8, X=4, Y=4, Z=4, ptr=p: (nv, H, W, ptr, p, p, p, p, 0.0, 0.0, 0.0, 0.1, X, Y, Z, 0.3, 0.2, 0.5, p, p, None)
    assert lib.soar_tsdf_integrate(*args(nv=0)) != 0 and "n_views" in err()
    assert lib.soar_tsdf_integrate(*args(nv=65)) != 0 and "n_views" in err()
    assert lib.soar_tsdf_integrate(*args(H=0)) != 0 and "image size" in err()
    assert lib.soar_tsdf_integrate(*args(X=-1)) != 0 and "non-positive" in err()
    assert lib.soar_tsdf_integrate(*args(X=2048, Y=1024, Z=1024)) != 0 and "2^31" in err()
    assert lib.soar_tsdf_integrate(*args(ptr=None)) != 0 and "NULL" in err()
    assert lib.soar_mc_workspace_bytes(0, 4, 4, C.byref(n)) != 0 and "non-positive" in err()
    assert lib.soar_mc_workspace_bytes(1024, 1024, 2048, C.byref(n)) != 0 and "2^31" in err()
    assert lib.soar_mc_workspace_bytes(64, 64, 64, None) != 0 and "NULL" in err()
    assert lib.soar_mc_workspace_bytes(64, 64, 64, C.byref(n)) == 0 and n.value >= 64 ** 3 * 18 and n.value % 256 == 0
    need = n.value
    assert lib.soar_mc_count(64, 64, 64, None, None, 0.0, 0x1000, need, cnt, None) != 0 and "NULL" in err()
    assert lib.soar_mc_count(64, 64, 64, p, None, 0.0, 0x1000, need - 1, cnt, None) != 0 and "workspace" in err()
    assert lib.soar_mc_count(64, 64, 64, p, None, 0.0, 0x1001, need, cnt, None) != 0 and "aligned" in err()
    assert lib.soar_mc_count(64, 64, 64, p, None, 0.0, 0x1000, need, None, None) != 0 and "counts_host" in err()
    assert lib.soar_mc_count(64, 0, 64, p, None, 0.0, 0x1000, need, cnt, None) != 0 and "non-positive" in err()
    assert lib.soar_mc_emit(64, 64, 64, p, None, 0.0, 0x1000, need, None, p, None) != 0 and "NULL" in err()
    assert lib.soar_mc_emit(3000, 1000, 1000, p, None, 0.0, 0x1000, need, p, p, None) != 0 and "2^31" in err()
    assert lib.soar_mesh_filter_bytes(0, 10, C.byref(n)) != 0
    assert lib.soar_mesh_filter_bytes(10, 20, C.byref(n)) == 0 and n.value % 256 == 0
    need = n.value
    assert lib.soar_mesh_filter_components(10, 0, p, p, 64, 0.2, 0x1000, need, p, p, cnt, None) != 0 and "F > 0" in err()
    assert lib.soar_mesh_filter_components(10, 20, p, None, 64, 0.2, 0x1000, need, p, p, cnt, None) != 0 and "NULL" in err()
    assert lib.soar_mesh_filter_components(10, 20, p, p, 64, 0.2, 0x1000, need - 1, p, p, cnt, None) != 0 and "workspace" in err()


def test_python_api_has_no_cpu_fallback():
    from soar_amd import mesh
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.marching_cubes(torch.zeros(4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.fuse_depth(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.eye(4)[None], torch.eye(4)[None], torch.zeros(1, 2),
                        (0, 0, 0), 0.1, (4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mesh.extract_mesh(torch.zeros(4, 3), torch.zeros(4, 4), torch.zeros(4, 3), torch.ones(4, 1))


def test_export_cameras_see_the_whole_grid():
    from soar_amd import mesh
    means = torch.tensor([[-0.7, -1.0, -0.2], [0.7, 0.8, 0.2]])
    scales = torch.tensor([[0.02, 0.02, -1e10], [0.01, 0.01, -1e10]])
    origin, voxel, dims = mesh.export_grid(means, scales, 256)
    assert max(dims) == 256
    for k in range(3):                                   # the box plus the surfel radius plus 2t lies inside the grid
        assert origin[k] <= float(means[:, k].min()) - 0.06 - 6 * voxel + 1e-6
        assert origin[k] + (dims[k] - 1) * voxel >= float(means[:, k].max()) + 0.06 + 6 * voxel - 1e-6
    cams, fov = mesh.export_cameras(origin, voxel, dims, 48, 1024)
    corners = torch.tensor([[origin[k] + ((c >> k) & 1) * (dims[k] - 1) * voxel for k in range(3)] for c in range(8)])
    ph = torch.cat([corners, torch.ones(8, 1)], 1)
    for wv, full, _ in cams:
        z = (ph @ wv)[:, 2]
        h = ph @ full
        ndc = h[:, :2] / h[:, 3:]
        assert (z > mesh.ZNEAR).all()
        assert (ndc.abs() <= 1.0).all()


def test_save_obj_round_trip(tmp_path):
    from soar_amd import mesh
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.1234567, -2.5e-7, 3.0e5]])
    f = torch.tensor([[0, 1, 2], [0, 2, 3], [1, 3, 2]], dtype=torch.int32)
    path = tmp_path / "m.obj"
    mesh.save_obj(str(path), mesh.Mesh(v, f))
    vs, fs = [], []
    for line in path.read_text().splitlines():
        tag, *rest = line.split()
        (vs if tag == "v" else fs).append(rest)
    assert torch.equal(torch.tensor([[float(x) for x in r] for r in vs], dtype=torch.float32), v)
    assert torch.equal(torch.tensor([[int(x) - 1 for x in r] for r in fs], dtype=torch.int32), f)
