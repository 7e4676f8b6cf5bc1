"""The incremental voxel map without a GPU: its entry points are declared in include/nos.h and exported by
libnos_hip.so, and — read from the gfx950 code objects hipcc cross-compiled into csrc/nos_voxelmap.o and
csrc/nos_mapbuild.o — its kernels neither spill nor use scratch memory, and the one-shot build still carries
voxel_sums_kernel and voxel_eigen_kernel under their names (the store launches the build's own sums kernel and shares the
per-voxel finish with the build's eigen kernel)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_voxel_map_create", "nos_voxel_map_insert", "nos_voxel_map_insert_scan", "nos_voxel_map_info",
           "nos_voxel_map_snapshot", "nos_voxel_map_stats", "nos_voxel_map_destroy")


def test_voxel_map_entry_points_are_declared_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = open(os.path.join(ROOT, "include", "nos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    lib = _lib.hip_lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
    assert "typedef struct nos_voxel_map nos_voxel_map;" in text


def test_voxel_map_kernels_have_no_spills_and_no_scratch_and_the_build_kernels_keep_their_names():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if k["name"].startswith(("nos::voxel_", "void nos::voxel_"))]
    for form in ("nos::voxel_points_kernel<false>", "nos::voxel_points_kernel<true>", "nos::voxel_lookup_kernel(",
                 "nos::voxel_merge_kernel(", "nos::voxel_rehash_kernel("):
        assert any(form in k["name"] for k in kernels), form
    bad = [(k["name"][:100], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
    build = {k["name"].split("(")[0]: k for k in kernel_resources.kernel_resources(os.path.join(CSRC, "nos_mapbuild.o"))}
    assert "nos::voxel_sums_kernel" in build and "nos::voxel_eigen_kernel" in build
    for name in ("nos::voxel_sums_kernel", "nos::voxel_eigen_kernel"):
        assert build[name]["spill"] == 0 and build[name]["scratch"] == 0, name
    # one lane per voxel runs the 3x3 eigen-decomposition: at most 128 of a SIMD's 512 VGPRs per lane keeps four waves
    # resident per SIMD, which is what the build's eigen kernel has
    merge = [k for k in kernels if "voxel_merge_kernel" in k["name"]][0]
    assert merge["vgpr"] <= 128 and build["nos::voxel_eigen_kernel"]["vgpr"] <= 128
    # the store does not carry copies of the build's kernels: it launches the build's own
    assert not any("voxel_sums_kernel" in k["name"] or "voxel_eigen_kernel" in k["name"] for k in kernels)
