"""The scan deskew without a GPU: nos_scan_deskew is declared in include/nos.h, listed in C_ABI_SYMBOLS and exported by
libnos_hip.so; arguments that can be judged on the host are rejected before any device is touched (and nothing is
written); the kernel's series threshold is the one pipeline.py and the tests use; and — read from the gfx950 code object
hipcc cross-compiled into csrc/nos_scandeskew.o — scan_deskew_kernel is there and neither spills nor uses scratch memory."""
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOS_ERR_INVALID_ARGUMENT = 1


def test_scan_deskew_is_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = open(os.path.join(ROOT, "include", "nos.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    lib = _lib.hip_lib()
    assert "nos_scan_deskew" in declared
    assert "nos_scan_deskew" in _lib.C_ABI_SYMBOLS
    assert hasattr(lib, "nos_scan_deskew")
    assert re.search(r"int\s+nos_scan_deskew\(nos_scan\*\s*scan,\s*const\s+double\*\s*times,\s*size_t\s+n_times,\s*"
                     r"double\s+reference_time,\s*const\s+double\s+twist\[6\],\s*nos_scan\*\*\s*out_scan\);", text)


def test_null_arguments_are_rejected_without_a_device_and_write_nothing():
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    sentinel = 12345
    out = ctypes.c_void_p(sentinel)
    times = (ctypes.c_double * 2)(0.0, 1.0)
    twist = (ctypes.c_double * 6)(0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert lib.nos_scan_deskew(None, times, 2, ctypes.c_double(1.0), twist, ctypes.byref(out)) == NOS_ERR_INVALID_ARGUMENT
    assert out.value == sentinel
    assert b"NULL" in lib.nos_last_error()


def test_the_series_threshold_is_one_number_everywhere():
    from nonlinear_optimizer_for_slam_amd import pipeline
    text = open(os.path.join(CSRC, "scan_deskew_kernels.hpp")).read()
    m = re.search(r"constexpr\s+double\s+kDeskewSeriesTheta\s*=\s*([0-9.eE+-]+)\s*;", text)
    assert m and float(m.group(1)) == pipeline._SERIES_THETA


def test_the_deskew_kernel_is_in_its_object_and_has_no_spills_and_no_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_scandeskew.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if "nos::scan_deskew_kernel(" in k["name"]]
    assert len(kernels) == 1, [k["name"][:100] for k in kernels]
    k = kernels[0]
    assert k["spill"] == 0 and k["scratch"] == 0, k
    # one point per lane, nothing kept across a loop: far below the 128 registers per lane that still leave four waves per
    # SIMD, so the streaming loads have other waves to hide behind
    assert k["vgpr"] <= 64 and k["lds"] == 0, k
