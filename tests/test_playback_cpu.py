"""CPU tests of avatar playback (soar_amd/playback.py, csrc/playback.hip): the NumPy restatement of the two kernels
against scipy and against torch's expression, the checkpoint key mapping, and the C ABI of the two new symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import playback_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_bytes(x: torch.Tensor) -> torch.Tensor:
    """torchvision's save_image conversion, as the reference's files get it"""
    return x.clone().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)


# ---- the motion restatement against scipy ---------------------------------------------------------------------------------------
def test_float64_restatement_matches_scipy_rotations():
    pytest.importorskip("scipy")
    from scipy.spatial.transform import Rotation, Slerp
    kp, kt, ke, t, yaw = R.motion_case()
    K = kp.shape[0]
    # axis-angle round trip: rotvec -> quaternion -> rotvec gives the same rotation, also at the zero rotation and next to pi
    a = kp.reshape(-1, 3).astype(np.float64)
    back = R.axis_angle_of_quat(R.quat_of_axis_angle(a))
    assert np.linalg.norm(back, axis=1).max() <= np.pi + 1e-12
    np.testing.assert_allclose(Rotation.from_rotvec(back).as_matrix(), Rotation.from_rotvec(a).as_matrix(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(R.rotation_matrices(a), Rotation.from_rotvec(a).as_matrix(), rtol=0, atol=1e-12)
    # Ry on the right: R0 Ry(a) is scipy's intrinsic 'y' turn applied after R0's frame, i.e. R0.as_matrix() @ Ry
    ang = np.array([0.0, 0.7, np.pi, 6.1, -2.0])
    np.testing.assert_allclose(R.rot_y(ang), Rotation.from_euler("y", ang).as_matrix(), rtol=0, atol=1e-15)
    q0 = R.quat_of_axis_angle(a[:5])
    turned = R.axis_angle_of_quat(R.times_yaw(q0, ang))
    want = Rotation.from_rotvec(a[:5]).as_matrix() @ Rotation.from_euler("y", ang).as_matrix()
    np.testing.assert_allclose(R.rotation_matrices(turned), want, rtol=0, atol=1e-12)
    # interpolation, every joint and time of the case, with and without the turn of the root
    for yw in (None, yaw):
        pose, transl, expr = R.motion_resample(kp, kt, ke, t, yw, np.float64)
        for f in range(len(t)):
            tc = min(max(float(t[f]), 0.0), K - 1.0)
            i0 = int(np.floor(tc))
            i1, u = min(i0 + 1, K - 1), tc - int(np.floor(tc))
            r0, r1 = Rotation.from_rotvec(kp[i0].astype(np.float64)), Rotation.from_rotvec(kp[i1].astype(np.float64))
            for j in range(R.JOINTS):
                M = r0[j].as_matrix() if i1 == i0 else Slerp([0.0, 1.0], Rotation.concatenate([r0[j], r1[j]]))([u])[0].as_matrix()
                if j == 0 and yw is not None:
                    M = M @ Rotation.from_euler("y", float(yw[f])).as_matrix()
                # (scipy's Slerp goes through rotation vectors, the kernel through sin weights: the same arc; 1e-9 also covers the
                # normalised-lerp branch, whose deviation from the arc is below (1.5e-3)^3 / 60)
                np.testing.assert_allclose(R.rotation_matrices(pose[f, j]), M, rtol=0, atol=1e-9, err_msg=f"frame {f} joint {j}")
            np.testing.assert_allclose(transl[f], (1 - u) * kt[i0].astype(np.float64) + u * kt[i1].astype(np.float64), rtol=0, atol=1e-12)


def test_restatement_branches_and_keys():
    """the case really contains what it says, keys come back as they are, and float32 follows float64"""
    kp, kt, ke, t, yaw = R.motion_case()
    q = R.quat_of_axis_angle(kp.astype(np.float32))
    dot01 = (q[0] * q[1]).sum(-1)
    assert dot01[3] > np.float32(R.LERP_DOT) and dot01[4] < -0.5                      # the lerp branch and the flip
    assert abs(np.linalg.norm(kp[1, 5]) - np.pi) < 1e-3 and not kp[:, 6].any() and not kp[2, 7].any()
    p32, t32, e32 = R.motion_resample(kp, kt, ke, t, None, np.float32)
    p64, t64, e64 = R.motion_resample(kp, kt, ke, t, None, np.float64)
    assert p32.dtype == t32.dtype == e32.dtype == np.float32
    for f, k in ((0, 0), (1, 2), (2, 1)):                                              # integer times: the key's own numbers
        assert np.array_equal(p32[f], kp[k]) and np.array_equal(t32[f], kt[k]) and np.array_equal(e32[f], ke[k])
    assert np.isfinite(p32).all() and np.abs(R.rotation_matrices(p32) - R.rotation_matrices(p64)).max() < 1e-6
    # out-of-range and NaN times are clamped
    pc, _, _ = R.motion_resample(kp, kt, ke, np.array([-3.0, 7.5, np.nan], np.float32), None, np.float32)
    assert np.array_equal(pc[0], kp[0]) and np.array_equal(pc[1], kp[2])


# ---- the output stage -----------------------------------------------------------------------------------------------------------
def test_finish_restatement_equals_torch_bit_for_bit():
    rng = np.random.default_rng(3)
    x = rng.uniform(-0.2, 1.2, (2, 3, 9, 31)).astype(np.float32)
    assert np.array_equal(R.to_byte(x), torch_bytes(torch.from_numpy(x)).numpy())
    v = R.crafted_values()
    ok = ~np.isnan(v)
    assert np.array_equal(R.to_byte(v[ok]), torch_bytes(torch.from_numpy(v[ok])).numpy())
    assert R.to_byte(np.array([np.nan], np.float32))[0] == 0                           # NaN -> 0 (torch leaves it undefined)
    assert R.to_byte(np.array([-5.0, -np.inf, 1.7, np.inf], np.float32)).tolist() == [0, 0, 255, 255]
    # the rule is not "round(x * 255)" computed with a fused multiply-add, nor floor(x * 255): every k / 255 gives k
    k = np.arange(256)
    assert np.array_equal(R.to_byte((k / 255.0).astype(np.float32)), k.astype(np.uint8))
    # the whole stage: channel order, the mask as fourth channel, normal_as_rgb
    render, normal, occ = (rng.uniform(-0.1, 1.1, (2, 3, 5, 7)).astype(np.float32) for _ in range(3))
    mask = rng.uniform(0, 1, (2, 1, 5, 7)).astype(np.float32)
    rgb, nrm, oc, m = R.playback_finish(render, normal, mask, occ)
    tb = lambda a: torch_bytes(torch.from_numpy(a))
    want = lambda img: torch.cat([tb(img), tb(mask)], dim=1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(rgb, want(render)) and np.array_equal(nrm, want(normal)) and np.array_equal(oc, want(occ))
    assert np.array_equal(m, tb(mask)[:, 0].numpy())
    nrm2 = R.playback_finish(render, normal, mask, None, normal_as_rgb=True)
    assert nrm2[2] is None and np.array_equal(nrm2[1], want((torch.from_numpy(normal) * 0.5 + 0.5).numpy()))


# ---- the checkpoint key mapping -------------------------------------------------------------------------------------------------
def _state_dict(P=7, log2=4):
    from soar_amd import playback as pb
    sd = {"geometry._xyz": torch.zeros(P, 3), "geometry._rotation": torch.zeros(P, 4), "geometry._occ": torch.zeros(P, 1),
          "geometry._colors": torch.zeros(P, 3), "geometry._scaling": torch.zeros(P, 1), "geometry._opacity": torch.zeros(P, 1)}
    for k, shape in pb.field_state_keys().items():
        sd["geometry.attribute_field." + k] = torch.zeros((16 << log2, 2) if shape is None else shape)
    return sd


def test_checkpoint_mapping_names_what_is_missing_or_misshapen():
    from soar_amd import playback as pb
    sd = _state_dict()
    for ckpt in ({"state_dict": sd, "epoch": 3}, sd):
        m = pb.map_checkpoint(ckpt)
        assert m["xyz"] is sd["geometry._xyz"] and m["scaling"] is sd["geometry._scaling"] and m["log2_hashmap_size"] == 4
        assert m["aabb"] is sd["geometry.attribute_field.aabb"] and set(m["field"]) == set(pb.field_state_keys())
    needed = [k for k in sd if k != "geometry._opacity"]
    assert len(needed) == 5 + 6 + 20
    for k in needed:
        with pytest.raises(KeyError, match=re.escape(f"'{k}'")):
            pb.map_checkpoint({"state_dict": {a: b for a, b in sd.items() if a != k}})
    for k, bad in (("geometry._rotation", torch.zeros(7, 3)), ("geometry._occ", torch.zeros(6, 1)),
                   ("geometry.attribute_field.aabb", torch.zeros(6)), ("geometry.attribute_field.encoding.hash_table", torch.zeros(16 * 12, 2)),
                   ("geometry.attribute_field.quat_encoding.hash_table", torch.zeros(16 << 5, 2)),
                   ("geometry.attribute_field.mlp_base_offsets.layers.0.weight", torch.zeros(64, 32))):
        with pytest.raises(ValueError, match=re.escape(f"'{k}'")):
            pb.map_checkpoint({"state_dict": dict(sd, **{k: bad})})
    # the field's keys are the module's own
    from soar_amd.field import HashMLPField
    f = HashMLPField(torch.zeros(2, 3), log2_hashmap_size=4)
    assert {k: (tuple(v.shape) if "hash_table" not in k else None) for k, v in f.state_dict().items()} == pb.field_state_keys()


def test_player_is_exported_and_refuses_cpu_tensors():
    import soar_amd
    from soar_amd import playback as pb
    assert soar_amd.AvatarPlayer is pb.AvatarPlayer
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pb.motion_resample(torch.zeros(1, 165), torch.zeros(1, 3), torch.zeros(1, 10), torch.zeros(2))
    z = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pb.playback_finish(z, z, z[:, :1])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from soar_amd import build, hip_lib
    build.build()
    return hip_lib.lib()


def test_new_symbols_are_declared_exported_and_check_their_arguments(lib):
    from soar_amd import hip_lib
    text = open(os.path.join(ROOT, "include", "soar_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(soar_[a-z0-9_]+)\s*\(", text))
    for name in ("soar_motion_resample", "soar_playback_finish"):
        assert name in declared and name in hip_lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"typedef struct SoarPlaybackArgs \{.*?\} SoarPlaybackArgs;", text, flags=re.S)
    assert C.sizeof(hip_lib.SoarPlaybackArgs) == 16 + 4 * 8 + 4 * 8 + 4 * 8
    # refusals before any launch (no GPU here): bad counts, NULL pointers, a stride shorter than a frame; empty work is a no-op
    one = C.c_float(0.0)
    p = C.cast(C.pointer(one), C.c_void_p)
    assert lib.soar_motion_resample(0, 4, 10, p, p, p, p, None, p, p, p, None) != 0 and "K=0" in hip_lib.last_error()
    assert lib.soar_motion_resample(3, 4, 10, p, p, None, p, None, p, p, p, None) != 0 and "NULL" in hip_lib.last_error()
    assert lib.soar_motion_resample(3, 0, 10, None, None, None, None, None, None, None, None, None) == 0
    a = hip_lib.SoarPlaybackArgs()
    a.B, a.H, a.W = 2, 5, 67
    assert lib.soar_playback_finish(None, None) != 0
    assert lib.soar_playback_finish(C.byref(a), None) != 0 and "NULL" in hip_lib.last_error()
    a.render = a.normal = a.mask = a.rgb = a.normal_out = a.mask_out = p
    a.render_stride, a.normal_stride, a.mask_stride = 3 * 335, 3 * 335 - 1, 335
    assert lib.soar_playback_finish(C.byref(a), None) != 0 and "stride" in hip_lib.last_error()
    a.B, a.W = 0, 0
    assert lib.soar_playback_finish(C.byref(a), None) != 0 and "bad arguments" in hip_lib.last_error()
    a.W = 67
    assert lib.soar_playback_finish(C.byref(a), None) == 0                            # B == 0
