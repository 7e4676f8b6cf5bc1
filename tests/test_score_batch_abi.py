"""Pose scoring without a GPU: nos_ndt_score_batch and nos_voxel_map_score_batch are declared in include/nos.h, listed in
_lib.C_ABI_SYMBOLS and exported by libnos_hip.so; nos_pose_score is 32 bytes on both sides of the binding; the chunk
size Python names is the kernel's; and — read from the gfx950 code object hipcc cross-compiled into csrc/nos_score.o —
each of the six nos::score_batch_kernel<View, LOSS> instantiations exists exactly once, neither spills nor uses scratch
memory and stays within 128 vector registers (four waves per SIMD: the budget of voxel_match_kernel, whose nine probes
in flight per lane this kernel keeps)."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_ndt_score_batch", "nos_voxel_map_score_batch")
INVALID = 1


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nos.h")).read(), flags=re.S)


def test_score_entry_points_are_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", _header()))
    lib = _lib.hip_lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name


def test_nos_pose_score_is_32_bytes_in_the_header_and_in_the_binding():
    from nonlinear_optimizer_for_slam_amd import _lib, api
    body = re.search(r"typedef struct nos_pose_score \{(.*?)\} nos_pose_score;", _header(), flags=re.S).group(1)
    fields = re.findall(r"(uint64_t|double)\s+(\w+);", body)
    assert fields == [("uint64_t", "matches"), ("uint64_t", "matched_points"), ("double", "cost"), ("double", "reserved")]
    assert ctypes.sizeof(_lib.NosPoseScore) == 32
    assert [f[0] for f in _lib.NosPoseScore._fields_] == [f[1] for f in fields]
    assert api.SCORE_DTYPE.itemsize == 32 and list(api.SCORE_DTYPE.names) == [f[1] for f in fields]


def test_the_chunk_size_python_names_is_the_kernels():
    from nonlinear_optimizer_for_slam_amd import api
    text = open(os.path.join(CSRC, "score_kernels.hpp")).read()
    assert int(re.search(r"constexpr int kScoreChunkPoints = (\d+);", text).group(1)) == api.SCORE_CHUNK_POINTS
    assert int(re.search(r"constexpr int kScoreBlock = (\d+);", text).group(1)) == 256


def test_a_call_without_a_map_is_rejected_before_any_device_is_touched():
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    row = _lib.NosPoseScore(7, 7, 7.0, 7.0)
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)()
    scans = (ctypes.c_void_p * 1)()
    for name in SYMBOLS:
        fn = getattr(lib, name)
        assert fn(None, scans, 1, R, t, None, 2, ctypes.byref(row)) == INVALID, name
        assert fn(None, scans, -1, R, t, None, 2, ctypes.byref(row)) == INVALID, name
        assert fn(None, None, 0, None, None, None, 2, None) == 0, name  # n_problems == 0: nothing to do
    assert (row.matches, row.matched_points, row.cost, row.reserved) == (7, 7, 7.0, 7.0)


def test_score_kernels_fit_four_waves_per_simd_without_spills_or_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_score.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if "nos::score_batch_kernel<" in k["name"]]
    assert len(kernels) == 6, [k["name"][:80] for k in kernels]
    for view in ("nos::MapView", "nos::VoxelMatchView"):
        for loss in (0, 1, 2):
            form = "nos::score_batch_kernel<%s, %d>(" % (view, loss)
            mine = [k for k in kernels if form in k["name"]]
            assert len(mine) == 1, (form, [k["name"][:80] for k in kernels])
            k = mine[0]
            print("%s: %d VGPRs + %d AGPRs, %d spills, %d B scratch, %d B LDS" % (form, k["vgpr"], k["agpr"], k["spill"],
                                                                               k["scratch"], k["lds"]))
            assert k["spill"] == 0 and k["scratch"] == 0, (form, k["spill"], k["scratch"])
            assert k["vgpr"] + k["agpr"] <= 128, (form, k["vgpr"], k["agpr"])
