"""The voxel-store merge without a GPU: nos_voxel_map_merge and nos_debug_voxel_moments are declared in
include/nos.h, listed in C_ABI_SYMBOLS and exported; the call rejects NULL arguments and dst == src before any device is
touched; voxel_moments_kernel and voxel_moment_sums_kernel are in the gfx950 code object of csrc/nos_voxelmap.o and no
kernel of the store spills or uses scratch; and the moment transform as the HOST computes it (csrc/voxel_moments.hpp
through nos_debug_voxel_moments) — bit for bit on exact inputs, against 50 digits on general ones.

Bounds of the general case, from the arithmetic (L = √3 (2 res_src + res_dst) bounds every |d'|):
  mean o' + s'/n: 8 ulp of ‖o‖₁ + ‖t‖∞ + L — about eight roundings (the two warps, the corner, n b, the sum) on
    quantities of that size;
  scatter M' − s' s'ᵀ / n: 128 · 2^-52 · n L² per entry — about twenty roundings per entry on terms n L² bounds, the margin
    for the cancellation in the subtraction.  b cancels from the scatter exactly, whatever its rounding error."""
import ctypes
import os
import re
import sys

import mpmath
import numpy as np

from oracle import oracle_voxel_xp as vx
from tests import voxel_inputs as vi
from tests import voxel_merge_inputs as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_voxel_map_merge", "nos_debug_voxel_moments")
INVALID = 1


def _lib():
    from nonlinear_optimizer_for_slam_amd import _lib
    return _lib.hip_lib()


def test_merge_and_its_hook_are_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nos.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    lib = _lib.hip_lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name


def test_null_arguments_and_self_merge_are_rejected_before_any_device_is_touched():
    lib = _lib()
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)()
    n = ctypes.c_size_t(7)
    block = ctypes.create_string_buffer(4096)  # stands in for a store: the checks below come before anything reads it
    fake = ctypes.c_void_p(ctypes.addressof(block))
    assert lib.nos_voxel_map_merge(None, None, R, t, ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_merge(None, fake, R, t, ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_merge(fake, None, R, t, ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_merge(fake, fake, None, t, ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_merge(fake, fake, R, None, ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_merge(fake, fake, R, t, ctypes.byref(n)) == INVALID  # dst == src
    assert lib.nos_voxel_map_merge(fake, fake, R, t, None) == INVALID
    assert n.value == 7
    # the hook: NULL, an empty voxel, a bad resolution
    s, c = np.ones(9), np.zeros(3, dtype=np.int64)
    assert lib.nos_debug_voxel_moments(1, None, None, 1.0, R, t, 1.0, None, None) == INVALID
    assert mi.debug_voxel_moments(lib, 0, s, c, 1.0, np.eye(3), np.zeros(3), 1.0)[0] == INVALID
    assert mi.debug_voxel_moments(lib, 1, s, c, 0.0, np.eye(3), np.zeros(3), 1.0)[0] == INVALID
    assert mi.debug_voxel_moments(lib, 1, s, c, 1.0, np.eye(3), np.zeros(3), float("nan"))[0] == INVALID


def test_merge_kernels_are_in_the_object_and_no_store_kernel_spills_or_uses_scratch():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = [k for k in kernel_resources.kernel_resources(obj) if k["name"].startswith(("nos::voxel_", "void nos::voxel_"))]
    for form in ("nos::voxel_moments_kernel(", "nos::voxel_moment_sums_kernel("):
        mine = [k for k in kernels if form in k["name"]]
        assert len(mine) == 1, form
        print("%s %d VGPRs, %d spills, %d B scratch" % (form, mine[0]["vgpr"], mine[0]["spill"], mine[0]["scratch"]))
    bad = [(k["name"][:100], k["spill"], k["scratch"]) for k in kernels if k["spill"] != 0 or k["scratch"] != 0]
    assert not bad, bad


def test_identity_rotation_and_whole_cell_translation_keep_the_sums_bit_for_bit():
    """R = I, t = whole cells of a power-of-two grid (o + t and o' are then exact, b = 0): sums_out IS sums, whatever
    their bits — general sums here, not only exact ones — and the cell moves by t / res."""
    lib = _lib()
    rng = np.random.default_rng(3)
    for res in (0.25, 0.5, 1.0, 2.0):
        for _ in range(20):
            n = int(rng.integers(1, 41))
            cell = rng.integers(-64, 65, size=3)
            pts = (cell + rng.uniform(0.05, 0.95, size=(n, 3))) * res
            count, sums = vi.corner_sums(pts, cell, res)
            shift = rng.integers(-100, 101, size=3)
            rc, cell_out, sums_out = mi.debug_voxel_moments(lib, count, sums, cell, res, np.eye(3), shift * res, res)
            assert rc == 0
            assert np.array_equal(cell_out, cell + shift), (cell, shift, cell_out)
            assert sums_out.tobytes() == sums.tobytes(), (sums, sums_out)


def test_axis_rotations_of_exact_inputs_give_the_sums_of_the_transformed_points_exactly():
    lib = _lib()
    for res in (0.5, 1.0):
        pts, rows, cells = mi.exact_voxels(48, res, seed=21, half=64)
        for (R, t) in mi.axis_poses(res):
            for r, cell in zip(rows, cells):
                count, sums = vi.corner_sums(pts[r], cell, res)
                q = pts[r] @ R.T + t  # exact: a signed permutation and a whole-cell shift
                want_cell = np.floor(q[0] / res).astype(np.int64)
                assert np.all(np.floor(q / res) == want_cell)
                _, want = vi.corner_sums(q, want_cell, res)
                rc, cell_out, sums_out = mi.debug_voxel_moments(lib, count, sums, cell, res, R, t, res)
                assert rc == 0
                assert np.array_equal(cell_out, want_cell), (cell, cell_out, want_cell)
                assert sums_out.tobytes() == want.tobytes(), (R, t, cell, sums_out - want)


def test_a_general_pose_against_50_digits():
    lib = _lib()
    c = vi.cloud(0.3, range(7), True)
    assert len(c.voxels) == 7
    R, t = mi.general_pose()
    worst_mean, worst_scatter = 0.0, 0.0
    for res_dst in (0.3, 0.5):
        L = mi.bound_scale(0.3, res_dst)
        for v in c.voxels:
            p = c.points[v["idx"]]
            n, sums = vi.corner_sums(p, v["cell"], 0.3)
            rc, cell_out, out = mi.debug_voxel_moments(lib, n, sums, v["cell"], 0.3, R, t, res_dst)
            assert rc == 0
            with mpmath.workdps(vx.DPS):
                m, sc = mi.mean_and_scatter_xp(mi.warp_xp(p, R, t))
                cell, dist = mi.cell_of_xp(m, res_dst)
                assert dist >= 1e-6, (v["cell"], dist)  # the cell is not decided by rounding (6e-3 for these inputs)
                assert tuple(int(x) for x in cell_out) == cell
                # what the finish will make of the output: o' = fl(cell · res) as cell_origin forms it
                o = [mpmath.mpf(float(np.float64(cell[k]) * np.float64(res_dst))) for k in range(3)]
                s = [mpmath.mpf(float(x)) for x in out[:3]]
                M = [[mpmath.mpf(float(out[3 + i])) for i in row] for row in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
                mean_err = max(abs(o[k] + s[k] / n - m[k]) for k in range(3))
                scatter_err = max(abs(M[a][b] - s[a] * s[b] / n - sc[a][b]) for a in range(3) for b in range(3))
            ulp = mi.mean_ulp(v["cell"], 0.3, t, res_dst)
            worst_mean = max(worst_mean, float(mean_err) / ulp)
            worst_scatter = max(worst_scatter, float(scatter_err) / (2.0 ** -52 * n * L * L))
            print("dst %.1f cell %s -> %s: mean %.3f ulp, scatter %.3f x 2^-52 n L^2" % (
                res_dst, v["cell"], cell, float(mean_err) / ulp, float(scatter_err) / (2.0 ** -52 * n * L * L)))
            assert float(mean_err) <= 8.0 * ulp, (v["cell"], res_dst, float(mean_err) / ulp)
            assert float(scatter_err) <= 128.0 * 2.0 ** -52 * n * L * L, (v["cell"], res_dst, float(scatter_err))
    print("maxima: mean %.3f ulp (bound 8), scatter %.3f x 2^-52 n L^2 (bound 128)" % (worst_mean, worst_scatter))
