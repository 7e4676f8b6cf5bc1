"""Matching against the live voxel store without a GPU: nos_voxel_map_match is declared in include/nos.h, listed in
_lib.C_ABI_SYMBOLS and exported by libnos_hip.so, and — read from the gfx950 code objects hipcc cross-compiled into
csrc/nos_voxelmap.o and csrc/nos_match.o — nos::voxel_match_kernel<double> and <float> neither spill nor use scratch
memory and stay within 128 vector registers (four waves per SIMD, the bar test_voxel_map_resources.py sets for the merge
kernel), while match_kernel<double / float>, whose record writer the new kernel shares, keeps its name."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_voxel_map_match_is_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = open(os.path.join(ROOT, "include", "nos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    assert "nos_voxel_map_match" in declared
    assert "nos_voxel_map_match" in _lib.C_ABI_SYMBOLS
    assert hasattr(_lib.hip_lib(), "nos_voxel_map_match")


def test_voxel_match_kernels_fit_four_waves_per_simd_without_spills_or_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if "nos::voxel_match_kernel<" in k["name"]]
    for form in ("nos::voxel_match_kernel<double>", "nos::voxel_match_kernel<float>"):
        mine = [k for k in kernels if form in k["name"]]
        assert len(mine) == 1, (form, [k["name"][:80] for k in kernels])
        k = mine[0]
        print("%s: %d VGPRs, %d spills, %d B scratch" % (form, k["vgpr"], k["spill"], k["scratch"]))
        assert k["spill"] == 0 and k["scratch"] == 0, (form, k["spill"], k["scratch"])
        assert k["vgpr"] <= 128, (form, k["vgpr"])


def test_the_snapshot_matcher_keeps_its_kernels():
    import kernel_resources
    names = [k["name"] for k in kernel_resources.kernel_resources(os.path.join(CSRC, "nos_match.o"))]
    for form in ("nos::match_kernel<double>", "nos::match_kernel<float>"):
        assert any(form in n for n in names), form
