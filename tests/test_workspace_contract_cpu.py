"""The guard of tests/workspace_guard.py itself, on the CPU: it sees a byte written next to a workspace and says where, it reaches every
module that allocates one, and every sizing call of the ABI is either run through it by a case of
tests/test_workspace_contract_gpu.py or listed there with the reason why not."""
import pytest
import torch

import test_workspace_contract_gpu as G
import workspace_guard as W
from soar_amd import hip_lib


def _bands(g, k=0):
    """the whole buffer of allocation k: guard, workspace, guard"""
    return g.buffers[k][3]


@pytest.mark.parametrize("fill", W.FILLS)
def test_the_slice_is_aligned_exact_and_filled(fill):
    with W.guarded(fill) as g:
        ws = hip_lib._workspace(1000, "cpu")
        other = hip_lib._workspace(1000, "cpu")
        assert ws.numel() == 1000 and ws.dtype == torch.uint8 and ws.data_ptr() % 256 == 0
        buf = _bands(g)
        assert buf.numel() == 1000 + 2 * W.GUARD and buf.data_ptr() + W.GUARD == ws.data_ptr()
        assert bool((buf[:W.GUARD] == W.GUARD_BYTE).all()) and bool((buf[W.GUARD + 1000:] == W.GUARD_BYTE).all())
        if fill == "zeros":
            assert bool((ws == 0).all())
        elif fill == "ones":
            assert bool((ws == 0xFF).all()) and bool(torch.isnan(ws[:992].view(torch.float32)).all()) and bool((ws[:992].view(torch.int32) == -1).all())
        else:
            assert len(ws.unique()) > 200 and not torch.equal(ws, other)           # a seed per allocation index
            with W.guarded(fill):
                assert torch.equal(hip_lib._workspace(1000, "cpu"), ws)            # ... and the same bytes in every context
        g.check()
        ws.fill_(7)                                                                # writes inside the slice pass
        g.check()


@pytest.mark.parametrize("offset,text", [(0, "0 bytes past the workspace's end"), (41, "41 bytes past the workspace's end"),
                                         (-1, "1 bytes before the workspace's start"), (-300, "300 bytes before the workspace's start")])
def test_a_byte_next_to_the_slice_fails_the_check_and_is_located(offset, text):
    with W.guarded("zeros") as g:
        hip_lib._workspace(512, "cpu")
        ws = hip_lib._workspace(777, "cpu")
        buf = _bands(g, 1)
        at = W.GUARD + 777 + offset if offset >= 0 else W.GUARD + offset
        assert buf[at] == W.GUARD_BYTE
        buf[at] = 0
        with pytest.raises(AssertionError) as e:
            g.check()
        msg = str(e.value)
        # the allocation's ordinal and size, who asked (this test calls hip_lib's name: the nearest soar_amd frame is none), where
        assert "workspace #1 (777 bytes" in msg and text in msg, msg
        buf[at] = W.GUARD_BYTE
        g.check()
        assert ws.numel() == 777


def test_the_asker_is_named():
    from soar_amd import body, masks
    with W.guarded("ones") as g:
        masks._workspace(64, "cpu")
        # (called from here, no soar_amd frame is above the allocator; through a module's own code its name stands there)
        assert g.buffers[0][:3] == (0, 64, "?")
        ws, nb = body._mesh_workspace(10, torch.device("cpu"))                     # the sizing call runs without a device
        assert g.buffers[1][:3] == (1, nb, "soar_amd.body") and ws.numel() == nb
        _bands(g, 1)[-1] = 1
        with pytest.raises(AssertionError, match=rf"workspace #1 \({nb} bytes, asked for by soar_amd.body, fill 'ones'\).*{W.GUARD - 1} bytes past"):
            g.check()


def test_the_patch_reaches_every_module_and_is_undone():
    import soar_amd.rasterizer as rasterizer
    mods = W.modules_with_workspace()
    names = {m.__name__ for m in mods}
    # hip_lib itself, the modules that import the name, and mesh, through which texture.py reaches it
    assert {"soar_amd.hip_lib", "soar_amd.mesh", "soar_amd.unet", "soar_amd.clip", "soar_amd.sam", "soar_amd.codec_io", "soar_amd.body",
            "soar_amd.densify", "soar_amd.field", "soar_amd.background", "soar_amd.geometry", "soar_amd.lpips", "soar_amd.normals",
            "soar_amd.masks", "soar_amd.evaluate", "soar_amd.sds"} <= names, sorted(names)
    original = {m.__name__: m._workspace for m in mods}
    scratch = rasterizer._scratch
    assert all(f is hip_lib._workspace for f in original.values())
    with W.guarded("zeros") as g:
        assert all(m._workspace == g.alloc for m in mods) and rasterizer._scratch == g.alloc
    assert all(m._workspace is original[m.__name__] for m in mods) and rasterizer._scratch is scratch
    with pytest.raises(KeyError):
        with W.guarded("noise") as g:
            assert rasterizer._scratch == g.alloc
            raise KeyError("inside")
    assert all(m._workspace is original[m.__name__] for m in mods) and rasterizer._scratch is scratch
    with pytest.raises(ValueError):
        with W.guarded("ffff"):
            pass
    assert all(m._workspace is original[m.__name__] for m in mods) and rasterizer._scratch is scratch


def test_every_sizing_call_is_claimed_or_listed():
    sizing = {n for n in hip_lib.SIGNATURES if n.endswith("_bytes") or n.endswith("_floats")}
    claimed = {n for calls in G.CASES.values() for n in calls}
    listed = set(G.NOT_COVERED)
    assert not claimed - sizing, f"a case claims what the ABI does not declare: {sorted(claimed - sizing)}"
    assert not listed - sizing, f"NOT_COVERED lists what the ABI does not declare: {sorted(listed - sizing)}"
    assert not claimed & listed, f"both claimed by a case and listed in NOT_COVERED: {sorted(claimed & listed)}"
    missing = sizing - claimed - listed
    assert not missing, (f"sizing calls that no case of tests/test_workspace_contract_gpu.py runs through the guard and NOT_COVERED does not "
                         f"list: {sorted(missing)}")
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in G.NOT_COVERED.values())
    # the table is the test: every case has its function and the other way round
    functions = {n[len("case_"):] for n in vars(G) if n.startswith("case_")}
    assert functions == set(G.CASES), (sorted(functions - set(G.CASES)), sorted(set(G.CASES) - functions))
