"""The C surface of the ray cast: nos_voxel_map_raycast is declared in include/nos.h, listed in
C_ABI_SYMBOLS and exported, api.ray_pattern is exported by the package; the ctypes struct has the layout of the header's;
every NOS_ERR_INVALID_ARGUMENT rejection is returned on fake handles, before any device (or any handle's content beyond
its context pointer) is touched, with no output written; the rejections that need a real store (a scan of another
context, a max_range that spans more than NOS_CARVE_MAX_CELLS cells) leave the outputs unwritten too; voxel_raycast_kernel
is in the gfx950 code object of csrc/nos_voxelmap.o and neither it nor the carve's walk spills or uses scratch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tests import voxel_carve_inputs as ci
from tests import voxel_raycast_inputs as ri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

INVALID, UNSUPPORTED = 1, 6
C_TYPES = {"size_t": ctypes.c_size_t, "double": ctypes.c_double, "uint32_t": ctypes.c_uint32, "int": ctypes.c_int}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nos.h")).read(), flags=re.S)


def _what(_lib, **kw):
    w = _lib.NosVoxelRaycast()
    w.struct_size = ctypes.sizeof(_lib.NosVoxelRaycast)
    w.min_range, w.max_range, w.max_mahalanobis_sq, w.min_points = 0.0, 40.0, 1.0, 0
    for k, v in kw.items():
        if k == "origin":
            for a in range(3):
                w.origin[a] = v[a]
        else:
            setattr(w, k, v)
    return w


class _Outputs:
    """the five outputs, filled with marks a write would disturb"""

    def __init__(self, n):
        self.voxels, self.ranges = np.full(n, 77, dtype=np.int32), np.full(n, 5.5)
        self.scan = ctypes.c_void_p(0xABC0)
        self.hits, self.skipped = ctypes.c_size_t(7), ctypes.c_size_t(9)

    def args(self):
        return (self.voxels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.ranges.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                ctypes.byref(self.scan), ctypes.byref(self.hits), ctypes.byref(self.skipped))

    def untouched(self):
        return (np.all(self.voxels == 77) and np.all(self.ranges == 5.5) and self.scan.value == 0xABC0
                and (self.hits.value, self.skipped.value) == (7, 9))


def test_raycast_is_declared_listed_and_exported():
    import nonlinear_optimizer_for_slam_amd as pkg
    from nonlinear_optimizer_for_slam_amd import _lib, api, pipeline
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", _header()))
    assert "nos_voxel_map_raycast" in declared
    assert "nos_voxel_map_raycast" in _lib.C_ABI_SYMBOLS
    assert hasattr(_lib.hip_lib(), "nos_voxel_map_raycast")
    assert pkg.ray_pattern is api.ray_pattern and "ray_pattern" in pkg.__all__
    assert callable(api.VoxelMap.raycast) and callable(pipeline.map_places)


def test_ray_pattern_is_elevation_major_unit_directions():
    from nonlinear_optimizer_for_slam_amd import api
    el = np.radians(np.linspace(-20.0, 20.0, 16))
    d = api.ray_pattern(120, el)
    assert d.shape == (1920, 3) and d.dtype == np.float64 and d.flags["C_CONTIGUOUS"]
    assert d.tobytes() == ri.pattern().tobytes()
    assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) < 1e-15)
    half = np.radians(1.5)  # the beams sit in the middle of their 3° azimuth cells
    assert np.allclose(d[0], [np.cos(el[0]) * np.cos(half), np.cos(el[0]) * np.sin(half), np.sin(el[0])])
    assert np.allclose(d[120], [np.cos(el[1]) * np.cos(half), np.cos(el[1]) * np.sin(half), np.sin(el[1])])
    assert np.allclose(d[30], [-np.cos(el[0]) * np.sin(half), np.cos(el[0]) * np.cos(half), np.sin(el[0])])  # a quarter turn on
    sector = np.arctan2(d[:, 1], d[:, 0]) % (2.0 * np.pi) * (60 / (2.0 * np.pi))
    assert np.all(np.abs(sector - np.round(sector)) > 0.2)  # far from the borders of 60 sectors
    assert np.allclose(api.ray_pattern(2, [0.0]), [[0.0, 1.0, 0.0], [0.0, -1.0, 0.0]])
    with pytest.raises(ValueError):
        api.ray_pattern(0, [0.0])


def test_the_python_struct_has_the_layout_of_the_header():
    from nonlinear_optimizer_for_slam_amd._lib import NosVoxelRaycast
    body = re.search(r"typedef struct nos_voxel_raycast \{(.*?)\} nos_voxel_raycast;", _header(), flags=re.S).group(1)
    fields = re.findall(r"(size_t|double|uint32_t|int)\s+(\w+)(?:\[(\d+)\])?;", body)
    assert len(fields) == len(body.split(";")) - 1  # every member of the header was understood
    want = [(name, C_TYPES[ctype] * int(dim) if dim else C_TYPES[ctype]) for ctype, name, dim in fields]
    got = list(NosVoxelRaycast._fields_)
    assert [n for n, _ in got] == [n for n, _ in want] == ["struct_size", "origin", "min_range", "max_range", "max_mahalanobis_sq",
                                                          "min_points"]
    for (name, a), (_, b) in zip(got, want):
        assert ctypes.sizeof(a) == ctypes.sizeof(b) and a._type_ == b._type_, name
    assert ctypes.sizeof(NosVoxelRaycast) == 64
    assert [getattr(NosVoxelRaycast, f).offset for f, _ in got] == [0, 8, 32, 40, 48, 56]


def test_invalid_arguments_are_rejected_on_fake_handles_before_any_device_is_touched():
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)()
    # zeroed blocks stand in for a store and a scan: the checks below come before anything reads more than the context
    # pointer both begin with
    block_a, block_b = ctypes.create_string_buffer(4096), ctypes.create_string_buffer(4096)
    vm, scan = ctypes.c_void_p(ctypes.addressof(block_a)), ctypes.c_void_p(ctypes.addressof(block_b))
    out = _Outputs(4)

    def call(vm=vm, scan=scan, R=R, t=t, w=_what(_lib)):
        return lib.nos_voxel_map_raycast(vm, scan, R, t, ctypes.byref(w) if w is not None else None, *out.args())

    nan, inf = float("nan"), float("inf")
    assert call(vm=None) == INVALID and call(scan=None) == INVALID and call(R=None) == INVALID and call(t=None) == INVALID
    assert call(w=None) == INVALID
    assert call(w=_what(_lib, struct_size=ctypes.sizeof(_lib.NosVoxelRaycast) - 8)) == INVALID
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
            assert call(w=_what(_lib, origin=ob)) == INVALID
    for bad in (nan, inf, 0.0, -0.0, -1.0):
        assert call(w=_what(_lib, max_range=bad)) == INVALID, bad
    for field in ("min_range", "max_mahalanobis_sq"):
        for bad in (nan, inf, -1e-300, -1.0):
            assert call(w=_what(_lib, **{field: bad})) == INVALID, (field, bad)
    # a scan of another context: the two handles begin with different context pointers; nothing follows the pointers
    ctypes.memmove(block_a, ctypes.byref(ctypes.c_void_p(0x1000)), ctypes.sizeof(ctypes.c_void_p))
    assert call() == INVALID
    assert "different contexts" in lib.nos_last_error().decode()
    assert out.untouched()  # no output was written by any of them


def test_raycast_kernels_are_in_the_object_and_neither_they_nor_the_carve_spill_or_use_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if k["name"].startswith(("nos::voxel_", "void nos::voxel_"))]
    for form in ("nos::voxel_raycast_kernel(", "nos::voxel_raycast_gather_kernel(", "nos::voxel_carve_walk_kernel("):
        mine = [k for k in kernels if form in k["name"]]
        assert len(mine) == 1, form
        print("%s %d VGPRs, %d spills, %d B scratch, %d B LDS" % (form, mine[0]["vgpr"], mine[0]["spill"], mine[0]["scratch"], mine[0]["lds"]))
        assert mine[0]["spill"] == 0 and mine[0]["scratch"] == 0 and mine[0]["lds"] == 0


@pytest.mark.gpu
def test_rejections_that_need_a_device_leave_the_outputs_unwritten(ctx):
    from nonlinear_optimizer_for_slam_amd import Context, _lib, api
    lib = _lib.hip_lib()
    _, pts = ri.exact_block_points()
    vm = api.VoxelMap(ctx, ci.RES, 1.0)
    vm.insert(pts)
    rays = np.array([(1.25, 0.25, 0.25), (0.25, 1.25, 0.25)])
    scan = api.Scan(ctx, rays)
    other = Context((0,))
    foreign = api.Scan(other, rays)
    R = np.ascontiguousarray(np.eye(3).reshape(9))
    t = np.zeros(3)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    out = _Outputs(2)

    def call(scan_h, max_range):
        w = _what(_lib, max_range=max_range, origin=(0.25, 0.25, 0.25))
        return lib.nos_voxel_map_raycast(vm._h, scan_h, dp(R), dp(t), ctypes.byref(w), *out.args())

    try:
        before, mem = vm.stats(), vm.memory()
        assert call(foreign._h, 2.0) == INVALID
        # 3 (ceil(max_range / res) + 1) > NOS_CARVE_MAX_CELLS = 4096 first at ceil(max_range / res) = 1365
        assert call(scan._h, 1364.5 * ci.RES) == UNSUPPORTED
        assert "NOS_CARVE_MAX_CELLS" in lib.nos_last_error().decode()
        assert call(scan._h, 1.0e9) == UNSUPPORTED
        assert out.untouched()
        after = vm.stats()
        for k in ("cells", "counts", "valid", "means", "sqrt_infos"):
            assert after[k].tobytes() == before[k].tobytes(), k
        assert vm.memory() == mem
        assert call(scan._h, 1364.0 * ci.RES) == 0  # the longest range the bound admits: 3 * 1365 = 4095
        assert (out.hits.value, out.skipped.value) == (2, 0) and np.all(out.voxels >= 0) and np.all(out.ranges == 0.0)
        hits = api.Scan._adopted(ctx, out.scan)
        assert len(hits) == 2
        hits.close()
        # every output pointer is optional
        w = _what(_lib, max_range=2.0)
        assert lib.nos_voxel_map_raycast(vm._h, scan._h, dp(R), dp(t), ctypes.byref(w), None, None, None, None, None) == 0
    finally:
        foreign.close()
        other.close()
        scan.close()
        vm.close()
