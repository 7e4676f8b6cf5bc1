"""The voxel map's sliding window without a GPU: nos_voxel_map_prune and nos_voxel_map_memory are declared in
include/nos.h, listed in C_ABI_SYMBOLS and exported by libnos_hip.so, and — read from the gfx950 code object hipcc
cross-compiled into csrc/nos_voxelmap.o — voxel_keep_kernel and voxel_compact_kernel are there and no kernel of the store
spills or uses scratch memory."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_voxel_map_prune", "nos_voxel_map_memory")


def test_prune_and_memory_are_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = open(os.path.join(ROOT, "include", "nos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    lib = _lib.hip_lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+NOS_PRUNE_BOX\s+1\b", text) and re.search(r"#define\s+NOS_PRUNE_AGE\s+2\b", text)
    assert "} nos_voxel_prune;" in text
    assert (_lib.NOS_PRUNE_BOX, _lib.NOS_PRUNE_AGE) == (1, 2)


def test_the_python_struct_has_the_layout_of_the_header():
    """size_t, int (+ padding), double[3], double[3], unsigned long long on an LP64 target."""
    import ctypes
    from nonlinear_optimizer_for_slam_amd._lib import NosVoxelPrune
    assert ctypes.sizeof(NosVoxelPrune) == 72
    assert [getattr(NosVoxelPrune, f).offset for f, _ in NosVoxelPrune._fields_] == [0, 8, 16, 40, 64]


def test_window_kernels_are_in_the_object_and_no_store_kernel_spills_or_uses_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if k["name"].startswith(("nos::voxel_", "void nos::voxel_"))]
    for form in ("nos::voxel_keep_kernel(", "nos::voxel_compact_kernel("):
        assert any(form in k["name"] for k in kernels), form
    bad = [(k["name"][:100], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
