"""Build libsoar_hip.so (the C-ABI library declared in include/soar_hip.h) with hipcc for gfx950.

``python -m soar_amd.build`` or ``soar_amd.build.build()``.  hipcc cross-compiles without a GPU, so this also
runs in the CPU-only build container.  The library is written in-tree (``soar_amd/_lib/``) so that it travels
with the repository snapshot to the GPU box.
"""
from __future__ import annotations

import concurrent.futures as cf
import hashlib
import os
import subprocess
import sys
from typing import List

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
OUT_DIR = os.path.join(_HERE, "_lib")
OBJ_DIR = os.path.join(OUT_DIR, "obj")
LIB_PATH = os.path.join(OUT_DIR, "libsoar_hip.so")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

COMMON_FLAGS = [
    f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-munsafe-fp-atomics",
    "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function",
]
# per-file extra flags.  rast_preprocess / rast_binning feed integer decisions (radii, tile rectangles, sort keys):
# no FMA contraction there, so they evaluate exactly like an IEEE evaluation of the reference expressions.
EXTRA_FLAGS = {
    "rast_preprocess.hip": ["-ffp-contract=off"],
    "rast_binning.hip": ["-ffp-contract=off"],
    # the per-Gaussian backward has cancellation-prone expressions (quaternion gradient): keep the reference's
    # operation order un-contracted so that rounding follows an IEEE evaluation of the reference source
    "rast_geom_bwd.hip": ["-ffp-contract=off"],
    # differences of identical products must be exactly zero (replicate-padded borders), as in the reference's torch ops
    "postops.hip": ["-ffp-contract=off"],
    # thresholds decide the integer layout of the densified model
    "densify.hip": ["-ffp-contract=off"],
    # vertex positions and fused distances are checked bit for bit / to 1e-5 against CPU restatements (tests/)
    "mesh.hip": ["-ffp-contract=off"],
    # cell indices decide the clustering; the float64 quadric sums are restated operation by operation (tests/mesh_simplify_ref.py)
    "mesh_simplify.hip": ["-ffp-contract=off"],
    # colour means, squared distances and smoothing sums are restated operation by operation (tests/mesh_attr_ref.py)
    "mesh_attr.hip": ["-ffp-contract=off"],
    # the new vertices' float64 sums are restated operation by operation (tests/mesh_holes_ref.py)
    "mesh_holes.hip": ["-ffp-contract=off"],
    # the bits of the faces' squared areas decide which faces an edge loses; restated operation by operation (tests/mesh_repair_ref.py)
    "mesh_repair.hip": ["-ffp-contract=off"],
    # face areas decide the atlas' integer layout, and barycentrics and positions are restated operation by operation (tests/texture_ref.py)
    "mesh_texture.hip": ["-ffp-contract=off"],
    # the background's composite must equal torch's three separate operations bit for bit
    "envmap.hip": ["-ffp-contract=off"],
    # exactly zero gradients where a difference is exactly zero, and values that do not depend on what the compiler fuses
    "geometry.hip": ["-ffp-contract=off"],
    # frames, crops and rays are checked bit for bit / to 1e-6 against a torch-CPU restatement (tests/data_ref.py); where torch
    # itself fuses a multiply-add the source says fmaf
    "data.hip": ["-ffp-contract=off"],
    # PSNR / SSIM are checked to 1e-9 and the per-pixel outputs bit for bit against a NumPy restatement (tests/eval_ref.py)
    "eval.hip": ["-ffp-contract=off"],
    # the byte images equal torch's multiply-then-add bit for bit; the slerp chain is restated operation by operation (tests/playback_ref.py)
    "playback.hip": ["-ffp-contract=off"],
    # the normal maps' bytes equal torch's add, divide, multiply, multiply, truncate bit for bit (tests/test_normalnet_gpu.py)
    "normal_io.hip": ["-ffp-contract=off"],
    # the projection feeds integer coverage (snapped vertices), and depths decide winners: float32 expressions evaluate as written
    "prior.hip": ["-ffp-contract=off"],
    # integer image processing; the float32 candidates are only compared with the threshold, as written
    "masks.hip": ["-ffp-contract=off"],
    # the LPIPS inputs and the blended target equal torch's separate multiplies, subtracts and adds bit for bit (loss_pixel.h writes the
    # cosine term's roundings out, so that term has the bits image_losses.hip gives it under either flag)
    "step_terms.hip": ["-ffp-contract=off"],
    # the strips' bytes, the yaw views and the residual sums equal a NumPy restatement bit for bit (tests/fitviz_ref.py)
    "fitviz.hip": ["-ffp-contract=off"],
    # peaks, line integrals and the persons' scores equal a NumPy float32 restatement bit for bit (tests/pose_ref.py)
    "pose.hip": ["-ffp-contract=off"],
    # rectangles, crops and the maps' maxima equal a NumPy float32 restatement bit for bit (tests/pose_parts_ref.py)
    "pose_parts.hip": ["-ffp-contract=off"],
    # the frame's sums and the sign of the determinant equal a NumPy float64 restatement bit for bit (tests/pose_init_ref.py)
    "pose_init.hip": ["-ffp-contract=off"],
    # the SLP vectoriser pairs neighbouring float operations into v_pk_* and pays for it with register shuffles (v_mov, v_pk_mov);
    # a packed float instruction occupies the SIMD as long as the two plain ones it replaces (32 lanes per cycle either way)
    "rast_render_bwd.hip": ["-fno-slp-vectorize"],
    "rast_render_fwd.hip": ["-fno-slp-vectorize"],      # (round 4: 275 -> 249 us per 4-frame step of the forward blends)
}
SOURCES = ["api.hip", "rast_preprocess.hip", "rast_binning.hip", "rast_tilebin.hip", "rast_blockmask.hip", "rast_render_fwd.hip", "rast_render_bwd.hip",
           "rast_geom_bwd.hip", "lbs.hip", "lbs_knn.hip", "frame_loss.hip", "postops.hip", "ssim.hip", "image_losses.hip", "smplx_joints.hip", "densify.hip", "optim.hip", "view.hip",
           "mesh.hip", "mesh_simplify.hip", "mesh_attr.hip", "mesh_holes.hip", "mesh_repair.hip", "mesh_texture.hip", "field.hip", "envmap.hip", "conv_gemm.hip", "lpips.hip", "vae.hip", "geometry.hip", "body.hip", "data.hip", "eval.hip", "playback.hip",
           "normalnet.hip", "normal_io.hip", "smplify.hip", "prior.hip", "masks.hip", "step_terms.hip", "fitviz.hip", "video.hip", "png.hip", "png_decode.hip", "jpeg_decode.hip", "image_resize.hip", "attention.hip", "sam.hip", "unet.hip", "clip.hip", "pose.hip", "pose_parts.hip", "pose_init.hip"]
HEADERS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(_HERE, "..", "include", "soar_hip.h")]


def _digest(paths: List[str], flags: List[str]) -> str:
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as f:
            h.update(f.read())
    h.update(" ".join(flags).encode())
    return h.hexdigest()


def _compile_one(src: str, verbose: bool) -> str:
    path = os.path.join(CSRC, src)
    obj = os.path.join(OBJ_DIR, src.replace(".hip", ".o"))
    # SOAR_HIPCC_FLAGS: extra flags for development experiments (e.g. -DSOAR_FWD_WPE=8); part of the object's digest
    flags = COMMON_FLAGS + EXTRA_FLAGS.get(src, []) + os.environ.get("SOAR_HIPCC_FLAGS", "").split()
    stamp = obj + ".sha"
    dig = _digest([path] + HEADERS, flags)
    if os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == dig:
        return obj
    cmd = [HIPCC] + flags + ["-c", path, "-o", obj]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(dig)
    return obj


def source_digest() -> str:
    """sha256 over the kernel sources, the public header and the compile flags: what a profile of the library was taken from
    (profiles/*_hbm_traffic.json carry it; bench.py refuses counters of another build)."""
    paths = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    paths.append(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "soar_hip.h"))
    flags = COMMON_FLAGS + [f"{k}:{' '.join(v)}" for k, v in sorted(EXTRA_FLAGS.items())]
    return _digest(paths, flags)[:16]


def build(verbose: bool = False, force: bool = False) -> str:
    os.makedirs(OBJ_DIR, exist_ok=True)
    if force:
        for f in os.listdir(OBJ_DIR):
            os.remove(os.path.join(OBJ_DIR, f))
    with cf.ThreadPoolExecutor(max_workers=min(8, len(SOURCES))) as ex:
        objs = list(ex.map(lambda s: _compile_one(s, verbose), SOURCES))
    newest = max(os.path.getmtime(o) for o in objs)
    if force or not os.path.exists(LIB_PATH) or os.path.getmtime(LIB_PATH) < newest:
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB_PATH] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB_PATH


if __name__ == "__main__":
    print(build(verbose=True, force="--force" in sys.argv))
