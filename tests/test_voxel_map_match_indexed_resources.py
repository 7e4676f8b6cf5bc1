"""Voxel-indexed matching against the live voxel store without a GPU: nos_voxel_map_match_indexed,
nos_indexed_dataset_info and nos_indexed_dataset_download are declared in include/nos.h, listed in _lib.C_ABI_SYMBOLS and
exported by libnos_hip.so; voxel_match_index_kernel — read from the gfx950 code object hipcc cross-compiled into
csrc/nos_voxelmap.o — neither spills nor uses scratch memory and stays within 128 vector registers, the bar
test_voxel_map_match_resources.py sets for the matcher whose search it shares, while voxel_match_kernel<double / float> are
still there once each; and the pipeline refuses the combinations of live_indexed that make no sense before it touches a
device."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_voxel_map_match_indexed", "nos_indexed_dataset_info", "nos_indexed_dataset_download")


def test_the_three_symbols_are_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = open(os.path.join(ROOT, "include", "nos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(_lib.hip_lib(), name), name


def _voxelmap_kernels():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    return kernel_resources.kernel_resources(obj)


def test_the_index_matcher_fits_four_waves_per_simd_without_spills_or_scratch():
    mine = [k for k in _voxelmap_kernels() if "voxel_match_index_kernel" in k["name"]]
    assert len(mine) == 1, [k["name"][:80] for k in mine]
    k = mine[0]
    print("voxel_match_index_kernel: %d VGPRs, %d spills, %d B scratch" % (k["vgpr"], k["spill"], k["scratch"]))
    assert k["spill"] == 0 and k["scratch"] == 0, (k["spill"], k["scratch"])
    assert k["vgpr"] <= 128, k["vgpr"]


def test_the_record_matcher_keeps_its_two_forms():
    names = [k["name"] for k in _voxelmap_kernels()]
    for form in ("nos::voxel_match_kernel<double>", "nos::voxel_match_kernel<float>"):
        assert sum(form in n for n in names) == 1, (form, [n[:80] for n in names])


def test_the_pipeline_refuses_what_live_indexed_cannot_be_combined_with():
    from nonlinear_optimizer_for_slam_amd import pipeline
    # scan_to_map: refused before the map, the scan or the context is looked at
    with pytest.raises(ValueError, match="keep_multiple"):
        pipeline.scan_to_map(None, None, None, live_indexed=True, keep_multiple=4)
    with pytest.raises(ValueError, match="indexed=True"):
        pipeline.scan_to_map(None, None, None, live_indexed=True, indexed=True)
    with pytest.raises(ValueError, match="VoxelMap"):
        pipeline.scan_to_map(None, object(), None, live_indexed=True)
    # odometry: its own two refusals need no frame; scan_to_map's two reach it through the first frame's call, which
    # refuses before it uses the map, the scan or the context
    with pytest.raises(ValueError, match="live_match=False"):
        pipeline.odometry(None, None, [], live_indexed=True, live_match=False)
    with pytest.raises(TypeError, match="live_indexed"):
        pipeline.odometry(None, None, [], live_indexed=True, one_launch=True)
    with pytest.raises(ValueError, match="keep_multiple"):
        pipeline.odometry(None, None, [None], live_indexed=True, keep_multiple=4)
    with pytest.raises(ValueError, match="indexed=True"):
        pipeline.odometry(None, None, [None], live_indexed=True, indexed=True)
