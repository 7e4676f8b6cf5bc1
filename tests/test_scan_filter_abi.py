"""The device voxel-grid scan filter without a GPU: nos_scan_filter and nos_scan_points are declared in include/nos.h,
exported by libnos_hip.so and listed in _lib.py; NULL arguments are rejected before any device is touched (and nothing is
written); and — read from the gfx950 code object hipcc cross-compiled into csrc/nos_scanfilter.o — the filter's kernels
neither spill nor use scratch memory."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_scan_filter", "nos_scan_points")
NOS_ERR_INVALID_ARGUMENT = 1


def test_scan_filter_entry_points_are_declared_exported_and_listed():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = open(os.path.join(ROOT, "include", "nos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    lib = _lib.hip_lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"int\s+nos_scan_filter\(nos_scan\*\s*scan,\s*double\s+voxel_size,\s*nos_scan\*\*\s*out_scan\);", text)
    assert re.search(r"int\s+nos_scan_points\(const\s+nos_scan\*\s*scan,\s*double\*\s*points_xyz_out\);", text)


def test_null_arguments_are_rejected_without_a_device_and_write_nothing():
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    sentinel = 12345
    out = ctypes.c_void_p(sentinel)
    assert lib.nos_scan_filter(None, ctypes.c_double(0.1), ctypes.byref(out)) == NOS_ERR_INVALID_ARGUMENT
    assert out.value == sentinel
    buf = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    assert lib.nos_scan_points(None, buf) == NOS_ERR_INVALID_ARGUMENT
    assert list(buf) == [1.0, 2.0, 3.0]
    assert b"NULL" in lib.nos_last_error()


def test_scan_filter_kernels_have_no_spills_and_no_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_scanfilter.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if "nos::scan_filter_" in k["name"]]
    for form in ("nos::scan_filter_claim_kernel(", "nos::scan_filter_gather_kernel("):
        assert any(form in k["name"] for k in kernels), form
    bad = [(k["name"][:100], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
    # one point per lane and nothing kept across a loop: far below the 128 registers per lane that still leave four waves
    # per SIMD, so the claim pass can hide its table latency behind other waves
    for k in kernels:
        assert k["vgpr"] <= 64 and k["lds"] == 0, k
    # the select's predicate (ScanFilterKeep) is compiled into rocPRIM's kernels of this object: they must not spill either
    rest = [k for k in kernel_resources.kernel_resources(obj) if "ScanFilterKeep" in k["name"]]
    assert rest, "the rocPRIM select over ScanFilterKeep is missing"
    bad = [(k["name"][:100], k["spill"], k["scratch"]) for k in rest if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
