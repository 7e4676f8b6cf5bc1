"""The line-of-sight carve without a GPU: nos_voxel_map_carve is declared in include/nos.h, listed in
C_ABI_SYMBOLS and exported; the ctypes struct has the layout of the header's; every NOS_ERR_INVALID_ARGUMENT rejection is
returned on fake handles, before any device (or any handle's content beyond its context pointer) is touched, with no
output written; voxel_carve_walk_kernel and voxel_carve_keep_kernel are in the gfx950 code object of csrc/nos_voxelmap.o
and no kernel of the store spills or uses scratch."""
import ctypes
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

INVALID = 1
C_TYPES = {"size_t": ctypes.c_size_t, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nos.h")).read(), flags=re.S)


def test_carve_is_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", _header()))
    assert "nos_voxel_map_carve" in declared
    assert "nos_voxel_map_carve" in _lib.C_ABI_SYMBOLS
    assert hasattr(_lib.hip_lib(), "nos_voxel_map_carve")
    assert int(re.search(r"#define NOS_CARVE_MAX_CELLS (\d+)", _header()).group(1)) == _lib.NOS_CARVE_MAX_CELLS == 4096


def test_the_python_struct_has_the_layout_of_the_header():
    from nonlinear_optimizer_for_slam_amd._lib import NosVoxelCarve
    body = re.search(r"typedef struct nos_voxel_carve \{(.*?)\} nos_voxel_carve;", _header(), flags=re.S).group(1)
    fields = re.findall(r"(size_t|double|uint32_t|int)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert len(fields) == len(body.split(";")) - 1  # every member of the header was understood
    want = [(name, C_TYPES[ctype] * int(dim) if dim else C_TYPES[ctype]) for ctype, name, dim in fields]
    got = list(NosVoxelCarve._fields_)
    assert [n for n, _ in got] == [n for n, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and a._type_ == b._type_, name
    assert ctypes.sizeof(NosVoxelCarve) == 72
    assert [getattr(NosVoxelCarve, f).offset for f, _ in got] == [0, 8, 32, 40, 48, 56, 60, 64]


def test_invalid_arguments_are_rejected_on_fake_handles_before_any_device_is_touched():
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)()
    # zeroed blocks stand in for a store and a scan: the checks below come before anything reads more than the context
    # pointer both begin with
    block_a, block_b = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    vm, scan = ctypes.c_void_p(ctypes.addressof(block_a)), ctypes.c_void_p(ctypes.addressof(block_b))
    removed, skipped = ctypes.c_size_t(7), ctypes.c_size_t(9)
    crossings, hits = np.full(4, 5, dtype=np.uint32), np.full(4, 6, dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)

    def what(**kw):
        w = _lib.NosVoxelCarve()
        w.struct_size = ctypes.sizeof(_lib.NosVoxelCarve)
        w.end_margin, w.min_range, w.max_range, w.min_crossings, w.min_hits = 0.75, 0.0, 100.0, 2, 1
        for k, v in kw.items():
            if k == "origin":
                for a in range(3):
                    w.origin[a] = v[a]
            else:
                setattr(w, k, v)
        return w

    def call(vm=vm, scan=scan, R=R, t=t, w=what()):
        return lib.nos_voxel_map_carve(vm, scan, R, t, ctypes.byref(w) if w is not None else None, ctypes.byref(removed),
                                       ctypes.byref(skipped), crossings.ctypes.data_as(u32p), hits.ctypes.data_as(u32p))

    nan, inf = float("nan"), float("inf")
    assert call(vm=None) == INVALID and call(scan=None) == INVALID and call(R=None) == INVALID and call(t=None) == INVALID
    assert call(w=None) == INVALID
    assert call(w=what(struct_size=ctypes.sizeof(_lib.NosVoxelCarve) - 8)) == INVALID
    for k in range(9):
        for bad in (nan, inf):
            Rb = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
            Rb[k] = bad
            assert call(R=Rb) == INVALID
    for k in range(3):
        for bad in (nan, -inf):
            tb, ob = (ctypes.c_double * 3)(), [0.0, 0.0, 0.0]
            tb[k], ob[k] = bad, bad
            assert call(t=tb) == INVALID
            assert call(w=what(origin=ob)) == INVALID
    for field in ("end_margin", "min_range"):
        for bad in (nan, inf, -1e-300, -1.0):
            assert call(w=what(**{field: bad})) == INVALID, (field, bad)
    for bad in (nan, inf, 0.0, -0.0, -1.0):
        assert call(w=what(max_range=bad)) == INVALID, bad
    assert call(w=what(min_crossings=0)) == INVALID and call(w=what(min_hits=0)) == INVALID
    # a scan of another context: the two handles begin with different context pointers; nothing follows the pointers
    ctypes.memmove(block_a, ctypes.byref(ctypes.c_void_p(0x1000)), ctypes.sizeof(ctypes.c_void_p))
    assert call() == INVALID
    assert "different contexts" in lib.nos_last_error().decode()
    # no output was written by any of them
    assert (removed.value, skipped.value) == (7, 9)
    assert np.all(crossings == 5) and np.all(hits == 6)


def test_carve_kernels_are_in_the_object_and_no_store_kernel_spills_or_uses_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if k["name"].startswith(("nos::voxel_", "void nos::voxel_"))]
    for form in ("nos::voxel_carve_walk_kernel(", "nos::voxel_carve_keep_kernel("):
        mine = [k for k in kernels if form in k["name"]]
        assert len(mine) == 1, form
        print("%s %d VGPRs, %d spills, %d B scratch" % (form, mine[0]["vgpr"], mine[0]["spill"], mine[0]["scratch"]))
    bad = [(k["name"][:100], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad
