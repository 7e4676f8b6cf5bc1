"""A voxel store's state without a GPU: the new entry points — nos_voxel_map_export, the four of
nos_voxel_state and nos_voxel_map_import — are declared in include/nos.h, listed in C_ABI_SYMBOLS and exported; the checks
that come before any device is touched reject NULL arguments, a bad side, a bad mode and NULL arrays with n > 0, and write
none of their outputs; voxel_restore_kernel, the export's gather kernel and the add's run kernel are in the gfx950 code
object of csrc/nos_voxelmap.o and no kernel of the store spills or uses scratch."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_voxel_map_export", "nos_voxel_state_size", "nos_voxel_state_info", "nos_voxel_state_get", "nos_voxel_state_destroy",
           "nos_voxel_map_import")
INVALID = 1
RESTORE, ADD = 0, 1


def _lib():
    from nonlinear_optimizer_for_slam_amd import _lib
    return _lib.hip_lib()


def test_the_state_entry_points_are_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nos.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    lib = _lib.hip_lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
    for name, value in (("NOS_STATE_KEPT", 0), ("NOS_STATE_REMOVED", 1), ("NOS_IMPORT_RESTORE", 0), ("NOS_IMPORT_ADD", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text), name
        assert getattr(_lib, name) == value


def test_bad_calls_are_rejected_before_any_device_is_touched_and_write_nothing():
    from nonlinear_optimizer_for_slam_amd import _lib as L
    lib = _lib()
    block = ctypes.create_string_buffer(4096)  # stands in for a store: the checks below come before anything reads it
    fake = ctypes.c_void_p(ctypes.addressof(block))
    out = ctypes.c_void_p(0x1234)
    rule = L.NosVoxelPrune()
    rule.struct_size, rule.what, rule.max_age = ctypes.sizeof(L.NosVoxelPrune), L.NOS_PRUNE_AGE, 1
    # export: NULL map, NULL out_state, a side outside 0-1 (with and without a selection)
    assert lib.nos_voxel_map_export(None, None, 0, ctypes.byref(out)) == INVALID
    assert lib.nos_voxel_map_export(fake, None, 0, None) == INVALID
    for side in (-1, 2, 7):
        assert lib.nos_voxel_map_export(fake, None, side, ctypes.byref(out)) == INVALID
        assert lib.nos_voxel_map_export(fake, ctypes.byref(rule), side, ctypes.byref(out)) == INVALID
    # … and what a prune rejects in the selection
    bad = L.NosVoxelPrune()
    bad.struct_size, bad.what = ctypes.sizeof(L.NosVoxelPrune), 0
    assert lib.nos_voxel_map_export(fake, ctypes.byref(bad), 0, ctypes.byref(out)) == INVALID
    bad.what, bad.struct_size = L.NOS_PRUNE_AGE, 8
    assert lib.nos_voxel_map_export(fake, ctypes.byref(bad), 1, ctypes.byref(out)) == INVALID
    bad.struct_size, bad.what = ctypes.sizeof(L.NosVoxelPrune), L.NOS_PRUNE_BOX
    bad.center[0] = float("nan")
    assert lib.nos_voxel_map_export(fake, ctypes.byref(bad), 0, ctypes.byref(out)) == INVALID
    assert out.value == 0x1234
    # the state's own calls
    assert lib.nos_voxel_state_size(None) == 0
    assert lib.nos_voxel_state_info(None, None, None, None, None, None) == INVALID
    assert lib.nos_voxel_state_get(None, None, None, None, None) == INVALID
    assert lib.nos_voxel_state_destroy(None) == 0
    # import: NULL map, an unknown mode, NULL arrays with n > 0
    cells = (ctypes.c_int64 * 3)(1, 2, 3)
    counts = (ctypes.c_uint32 * 1)(5)
    sums = (ctypes.c_double * 9)(*([0.5] * 9))
    touched = ctypes.c_size_t(7)
    for mode in (RESTORE, ADD):
        assert lib.nos_voxel_map_import(None, mode, 1.0, 1, cells, counts, sums, None, 0, ctypes.byref(touched)) == INVALID
        assert lib.nos_voxel_map_import(fake, mode, 1.0, 1, None, counts, sums, None, 0, ctypes.byref(touched)) == INVALID
        assert lib.nos_voxel_map_import(fake, mode, 1.0, 1, cells, None, sums, None, 0, ctypes.byref(touched)) == INVALID
        assert lib.nos_voxel_map_import(fake, mode, 1.0, 1, cells, counts, None, None, 0, ctypes.byref(touched)) == INVALID
    for mode in (-1, 2, 100):
        assert lib.nos_voxel_map_import(fake, mode, 1.0, 1, cells, counts, sums, None, 0, ctypes.byref(touched)) == INVALID
        assert lib.nos_voxel_map_import(fake, mode, 1.0, 0, None, None, None, None, 0, ctypes.byref(touched)) == INVALID
    assert touched.value == 7
    assert block.raw == bytes(4096)  # nothing was written into the stand-in either


def test_state_kernels_are_in_the_object_and_no_store_kernel_spills_or_uses_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if k["name"].startswith(("nos::voxel_", "void nos::voxel_"))]
    for form in ("nos::voxel_restore_kernel(", "nos::voxel_state_gather_kernel(", "nos::voxel_state_runs_kernel("):
        mine = [k for k in kernels if form in k["name"]]
        assert len(mine) == 1, form
        print("%s %d VGPRs, %d spills, %d B scratch" % (form, mine[0]["vgpr"], mine[0]["spill"], mine[0]["scratch"]))
    bad = [(k["name"][:100], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
