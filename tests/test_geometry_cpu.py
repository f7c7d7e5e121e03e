"""The host-only parts of the geometry model (soar_amd/geometry.py, ``"gaussiansurfel-base"``): configuration, the parameter-group
table, the positions' learning-rate schedule and the PLY reader / writer.  No device: the model is built from CPU tensors."""
import os

import numpy as np
import pytest
import torch

import geometry_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the geometry sections of gaussiansurfel_imagedream_s0.yaml / _s1.yaml (they differ in position_lr_final)
S0 = dict(position_lr_init=0.000016, position_lr_final=0.0000016, position_lr_delay_mult=0.01, position_lr_max_steps=1000, camera_lr=0.0,
          scale_lr=0.005, feature_lr=0.01, opacity_lr=0.01, background_lr=0.001, field_lr=0.01, rotation_lr=0.001, pred_normal=True,
          normal_lr=0.005, occ_lr=0.1, densification_interval=100, prune_interval=100, densify_from_iter=100, densify_until_iter=9000,
          prune_from_iter=300, prune_until_iter=9000, opacity_reset_interval=100000, densify_grad_threshold=0.0001, min_opac_prune=0.05,
          split_thresh=0.01, radii2d_thresh=1000, opacity_init=0.1, pc_init_radius=0.6)
S1 = dict(S0, position_lr_final=0.000016)


def make_model(P, cfg=None, sh_degree=0, S=1, seed=0, with_field=True):
    from soar_amd.field import HashMLPField
    from soar_amd.geometry import GaussianSurfelModel
    g = torch.Generator().manual_seed(seed)
    m = GaussianSurfelModel(dict(cfg or {}, sh_degree=sh_degree))
    n_rest = (sh_degree + 1) ** 2 - 1
    r = lambda *s: torch.randn(*s, generator=g)
    m.set_leaves(xyz=r(P, 3), f_dc=r(P, 1, 3), f_rest=r(P, n_rest, 3), color=r(P, 3), opacity=r(P, 1), scaling=r(P, S), rotation=r(P, 4),
                 occ=r(P, 1), original_pos=r(P, 3), max_radii2D=torch.zeros(P))
    if with_field:
        m.attribute_field = HashMLPField(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), log2_hashmap_size=8)
    m.latent_pose = torch.nn.Parameter(torch.zeros(4, 2))
    return m


def test_model_is_registered_and_exported_and_ignores_unknown_keys(caplog):
    import logging
    import soar_amd
    from soar_amd.renderer import registry
    cls = registry.find("gaussiansurfel-base")
    assert cls is soar_amd.GaussianSurfelModel
    with caplog.at_level(logging.INFO, logger="soar_amd"):
        m = cls(dict(S0, not_a_field=3, another=1))
    assert m.cfg.opacity_lr == 0.01 and m.cfg.max_num == 500000 and m.cfg.scaling_lr == 0.005 and m.cfg.latent_pose_lr == 0.01
    lines = [r.getMessage() for r in caplog.records if "unknown config keys" in r.getMessage()]
    assert len(lines) == 1 and "another" in lines[0] and "not_a_field" in lines[0]


@pytest.mark.parametrize("cfg,final", [(S0, 1.6e-6), (S1, 1.6e-5)], ids=["s0", "s1"])
def test_group_table_names_order_and_learning_rates(cfg, final):
    m = make_model(10, cfg)
    m.spatial_lr_scale = 10
    m.training_setup()
    got = [(g["name"], g["lr"]) for g in m.optimizer.param_groups]
    # literal values from training_setup (TS/geometry/surfel_base.py:596-673) with the config's numbers
    want = [("xyz", 0.000016 * 10), ("f_dc", 0.01), ("f_rest", 0.01 / 20.0), ("color", 0.01), ("attribute_field_encoding", 0.01),
            ("attribute_field_quat_encoding", 0.01), ("attribute_field_shs", 0.01), ("attribute_field_quats", 0.01),
            ("attribute_field_scales", 0.01 * 10), ("attribute_field_offests", 0.01 * 0.01), ("opacity", 0.01), ("scaling", 0.005),
            ("rotation", 0.001), ("occ", 0.1), ("latent_pose", 0.01)]
    assert [n for n, _ in got] == [n for n, _ in want]
    for (n, a), (_, b) in zip(got, want):
        assert a == pytest.approx(b, rel=1e-15), n
    assert got == gr.group_table(m.cfg, 10)
    # the tensors behind the names
    by = {g["name"]: g["params"] for g in m.optimizer.param_groups}
    assert by["xyz"][0] is m._xyz and by["color"][0] is m._colors and by["occ"][0] is m._occ and by["latent_pose"][0] is m.latent_pose
    f = m.attribute_field
    assert by["attribute_field_encoding"][0] is f.encoding.hash_table and by["attribute_field_quat_encoding"][0] is f.quat_encoding.hash_table
    assert [tuple(p.shape) for p in by["attribute_field_offests"]] == [(64, 34), (64,), (3, 64), (3,)]
    assert sum(len(p) for p in by.values()) == 27 and m.optimizer.eps == 1e-15 and m.optimizer.betas == (0.9, 0.999)
    # the camera flag joins the three mode flags (:675-679)
    assert m.config.tolist() == [1.0, 1.0, 1.0, 0.0]
    # the schedule ends where the config says
    assert m.update_learning_rate(10 ** 6) == pytest.approx(final * 10, rel=1e-12)
    assert m.optimizer.param_groups[0]["lr"] == m.update_learning_rate(10 ** 6)


@pytest.mark.parametrize("kw", [dict(lr_init=1.6e-4, lr_final=1.6e-5, lr_delay_mult=0.01, max_steps=1000),
                                dict(lr_init=1.6e-4, lr_final=1.6e-4, lr_delay_mult=0.01, max_steps=1000),
                                dict(lr_init=1e-2, lr_final=1e-5, lr_delay_steps=300, lr_delay_mult=0.01, max_steps=2000)])
def test_expon_lr_func_matches_the_closed_form(kw):
    from soar_amd.geometry import get_expon_lr_func
    f = get_expon_lr_func(**kw)
    for step in (0, 1, 500, 1000, 5000):
        want = gr.expon_lr(step, **kw)
        assert abs(float(f(step)) - want) <= 1e-12 * abs(want), (step, float(f(step)), want)
    assert f(-1) == 0.0 and get_expon_lr_func(0.0, 0.0)(5) == 0.0


def _header(path):
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"end_header\n") + len(b"end_header\n")]
    return head.decode("ascii").split("\n")[:-1], raw[len(head):]


def test_ply_header_is_the_committed_property_list(tmp_path):
    names = open(os.path.join(ROOT, "tests", "golden", "surfel_ply_properties.txt")).read().split()
    m = make_model(7, with_field=False)
    path = str(tmp_path / "sub" / "a.ply")
    m.save_ply(path)
    lines, body = _header(path)
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 7"] and lines[-1] == "end_header"
    assert lines[3:-1] == [f"property float {n}" for n in names]
    assert m.construct_list_of_attributes() == names and len(body) == 7 * 4 * len(names)
    # a degree-1 model with three scale columns: f_rest in channel-major order, three scales
    m3 = make_model(5, sh_degree=1, S=3, with_field=False)
    assert m3.construct_list_of_attributes() == (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{i}" for i in range(9)]
                                                 + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])


PLY_LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@pytest.mark.parametrize("P,deg,S", [(0, 0, 1), (1, 0, 1), (257, 0, 1), (33, 1, 3)])
def test_ply_round_trip_is_bit_exact(tmp_path, P, deg, S):
    from soar_amd.geometry import GaussianSurfelModel
    m = make_model(P, sh_degree=deg, S=S, seed=3, with_field=False)
    with torch.no_grad():
        if P:
            m._xyz[0, 0] = float("inf")            # any bit pattern survives
            m._opacity[-1, 0] = -0.0
    path = str(tmp_path / "m.ply")
    m.save_ply(path)
    b = GaussianSurfelModel({"sh_degree": deg})
    b.load_ply(path, device="cpu")
    for a in PLY_LEAVES:
        x, y = getattr(m, a).detach(), getattr(b, a).detach()
        assert x.shape == y.shape and y.dtype == torch.float32 and y.is_contiguous(), a
        assert np.array_equal(x.numpy().view(np.int32), y.numpy().view(np.int32)), a
        assert getattr(b, a).requires_grad
    assert b.active_sh_degree == deg and b.original_pos.shape == (P, 3) and b._occ.shape == (P, 1) and b._colors.shape == (P, 3)
    # a model that already has P rows keeps what the file does not hold
    m2 = make_model(P, sh_degree=deg, S=S, seed=4, with_field=False)
    keep = (m2._colors.detach().clone(), m2._occ.detach().clone(), m2.original_pos.clone())
    m2.load_ply(path, device="cpu")
    assert torch.equal(m2._colors.detach(), keep[0]) and torch.equal(m2._occ.detach(), keep[1]) and torch.equal(m2.original_pos, keep[2])
    assert np.array_equal(m2._rotation.detach().numpy().view(np.int32), m._rotation.detach().numpy().view(np.int32))


def test_ply_reader_accepts_crlf_and_comments_and_names_a_missing_property(tmp_path):
    from soar_amd.geometry import GaussianSurfelModel
    m = make_model(19, seed=5, with_field=False)
    path = str(tmp_path / "m.ply")
    m.save_ply(path)
    lines, body = _header(path)
    variant = lines[:2] + ["comment written by another tool", "comment  two"] + lines[2:5] + ["comment between properties"] + lines[5:]
    p2 = str(tmp_path / "crlf.ply")
    with open(p2, "wb") as f:
        f.write(("\r\n".join(variant) + "\r\n").encode("ascii") + body)
    b = GaussianSurfelModel({})
    b.load_ply(p2, device="cpu")
    for a in PLY_LEAVES:
        assert torch.equal(getattr(m, a).detach(), getattr(b, a).detach()), a
    # a column order other than ours, doubles and extra properties: read by name
    order = np.random.RandomState(0).permutation(len(lines[3:-1]))
    names = [lines[3:-1][i].split()[-1] for i in order]
    rows = np.frombuffer(body, "<f4").reshape(19, -1)[:, order]
    dt = np.dtype([(n, "<f8" if n == "opacity" else "<f4") for n in names] + [("extra", "u1")])
    arr = np.zeros(19, dt)
    for k, n in enumerate(names):
        arr[n] = rows[:, k]
    p3 = str(tmp_path / "perm.ply")
    with open(p3, "wb") as f:
        head = ["ply", "format binary_little_endian 1.0", "element vertex 19"] + \
               [f"property {'double' if n == 'opacity' else 'float'} {n}" for n in names] + ["property uchar extra", "element face 0",
                                                                                             "property list uchar int vertex_indices", "end_header"]
        f.write(("\n".join(head) + "\n").encode("ascii") + arr.tobytes())
    c = GaussianSurfelModel({})
    c.load_ply(p3, device="cpu")
    for a in PLY_LEAVES:
        assert torch.equal(getattr(m, a).detach(), getattr(c, a).detach()), a
    # refused, with the property named
    for missing in ("rot_2", "opacity", "f_dc_1", "scale_0", "z"):
        keep = [l for l in lines if l != f"property float {missing}"]
        cols = [i for i, l in enumerate(lines[3:-1]) if l != f"property float {missing}"]
        p4 = str(tmp_path / f"no_{missing}.ply")
        with open(p4, "wb") as f:
            f.write(("\n".join(keep) + "\n").encode("ascii") + np.ascontiguousarray(np.frombuffer(body, "<f4").reshape(19, -1)[:, cols]).tobytes())
        with pytest.raises(ValueError, match=f"'{missing}'"):
            GaussianSurfelModel({}).load_ply(p4, device="cpu")
    # a degree-1 model asks for its f_rest columns
    with pytest.raises(ValueError, match="'f_rest_0'"):
        GaussianSurfelModel({"sh_degree": 1}).load_ply(path, device="cpu")
    with open(str(tmp_path / "short.ply"), "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii") + body[:-4])
    with pytest.raises(ValueError, match="bytes present"):
        GaussianSurfelModel({}).load_ply(str(tmp_path / "short.ply"), device="cpu")


def test_computing_entry_points_refuse_cpu_tensors():
    from soar_amd import geometry
    m = make_model(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.get_rotation
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.regularizers({"lambda_delta": 1.0}, scales=torch.zeros(8, 1))
    m.training_setup()
    m._xyz.grad = torch.zeros_like(m._xyz)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.optimizer.step()
    with pytest.raises(ValueError, match="lambda_bogus"):
        geometry.surfel_regularizers(*[torch.zeros(1, 3)] * 5, {"lambda_bogus": 1.0})


def test_new_entry_points_check_their_arguments():
    import ctypes as C
    from soar_amd import build, hip_lib
    build.build()
    L = hip_lib.lib()
    assert L.soar_surfel_activations_forward(0, 1, *[None] * 10, None) == 0               # P = 0: success, no launch
    assert L.soar_surfel_activations_backward(0, 3, *[None] * 16, None) == 0
    assert L.soar_surfel_activations_forward(5, 4, *[None] * 10, None) != 0 and "S=4" in hip_lib.last_error()
    assert L.soar_surfel_activations_forward(5, 1, 0x1000, *[None] * 9, None) != 0 and "without its output" in hip_lib.last_error()
    n = C.c_size_t(0)
    assert L.soar_surfel_regularizers_workspace_bytes(100000, C.byref(n)) == 0 and n.value >= 391 * 5 * 8 and n.value % 256 == 0
    assert L.soar_surfel_regularizers(0, 1, 1, *[None] * 5, 0x1000, None, 0x1000, None, None, None, None, 0, None) == 0
    assert L.soar_surfel_regularizers(10, 1, 1, *[None] * 5, 0x1000, None, 0x1000, None, None, None, None, 0, None) != 0
    assert "workspace" in hip_lib.last_error()
    assert L.soar_surfel_regularizers(10, 1, 1, *[None] * 5, None, None, None, None, None, None, None, 0, None) != 0
    # a table of 41 rows is refused before anything is launched; the entry that was there before keeps its 8
    rows = (hip_lib.SoarAdamRow * 41)()
    assert L.soar_adam_step_rows_wide(41, rows, 0.9, 0.999, 1e-15, 0x1000, 1, None) != 0 and "40" in hip_lib.last_error()
    assert L.soar_adam_step_rows(9, rows, 0.9, 0.999, 1e-15, 0x1000, 1, None) != 0 and "<= 8" in hip_lib.last_error()
    assert L.soar_adam_step_rows_wide(0, None, 0.9, 0.999, 1e-15, None, 1, None) != 0
