"""The map-to-map match without a GPU: nos_voxel_map_match_map and nos_debug_voxel_pair_information are
declared in include/nos.h, listed in C_ABI_SYMBOLS and exported; the combined information as the HOST computes it
(csrc/voxeld2d_kernels.hpp through the hook) against 50 digits and in closed forms; and — read from the gfx950 code
object of csrc/nos_voxelmap.o — voxel_match_map_kernel<double> and <float> neither spill nor use scratch memory.

Bound (tests/voxel_d2d_inputs.py): max|SᵀS − A_xp| / max|A_xp| of the hook is at most 4 x the worst such error of a plain
numpy float64 restatement (`inv`, `cholesky`) on the same 2 000 triples.  Measured: numpy 38.2 eps, the hook 34.8 eps
(bound 152.7 eps)."""
import ctypes
import os
import re
import sys

import mpmath
import numpy as np

from tests import voxel_d2d_inputs as di
from tests import voxel_merge_inputs as mi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

SYMBOLS = ("nos_voxel_map_match_map", "nos_debug_voxel_pair_information")
INVALID = 1


def _lib():
    from nonlinear_optimizer_for_slam_amd import _lib
    return _lib.hip_lib()


def test_match_map_and_its_hook_are_declared_listed_and_exported():
    from nonlinear_optimizer_for_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nos.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nos_[a-z0-9_]+)\s*\(", text))
    lib = _lib.hip_lib()
    for name in SYMBOLS:
        assert name in declared, name
        assert name in _lib.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name


def test_null_arguments_are_rejected_before_any_device_is_touched():
    lib = _lib()
    R = (ctypes.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    t = (ctypes.c_double * 3)()
    n = ctypes.c_size_t(7)
    out = ctypes.c_void_p(5)
    block = ctypes.create_string_buffer(4096)  # stands in for a store: the NULL checks come before anything reads it
    fake = ctypes.c_void_p(ctypes.addressof(block))
    assert lib.nos_voxel_map_match_map(None, None, R, t, 2, 0, ctypes.byref(out), ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_match_map(None, fake, R, t, 2, 0, ctypes.byref(out), ctypes.byref(n)) == INVALID
    assert n.value == 7 and out.value == 5
    S = np.eye(3).reshape(9)
    dp = ctypes.POINTER(ctypes.c_double)
    ok = ctypes.c_ubyte(9)
    assert lib.nos_debug_voxel_pair_information(None, S.ctypes.data_as(dp), R, S.ctypes.data_as(dp), ctypes.byref(ok)) == INVALID
    assert lib.nos_debug_voxel_pair_information(S.ctypes.data_as(dp), S.ctypes.data_as(dp), R, S.ctypes.data_as(dp), None) == INVALID
    assert ok.value == 9


def test_the_hook_against_50_digits_on_random_triples():
    lib = _lib()
    worst = 0.0
    with mpmath.workdps(di.DPS):
        for (St, Ss, R), A in zip(di.random_triples(), di.random_references()):
            rc, S, ok = di.debug_pair_information(lib, St, Ss, R)
            assert rc == 0 and ok == 1 and np.all(np.isfinite(S)), (rc, ok, S)
            worst = max(worst, di.information_error(S, A))
    print("worst max|S^T S - A| / max|A| over %d triples: numpy restatement %.1f eps, the hook %.1f eps (bound %.1f eps)" % (
        di.N_TRIPLES, di.numpy_worst_error() / di.EPS, worst / di.EPS, di.bound() / di.EPS))
    assert worst <= di.bound(), (worst / di.EPS, di.bound() / di.EPS)


def test_the_hook_refuses_zero_and_non_finite_inputs():
    lib = _lib()
    good, R = di.random_triples()[0][0], np.eye(3)
    bad = [np.zeros((3, 3))]
    for v in (np.nan, np.inf, -np.inf):
        S = good.copy()
        S[1, 2] = v
        bad.append(S)
    for S in bad:
        for args in ((S, good, R), (good, S, R)):
            rc, out, ok = di.debug_pair_information(lib, *args)
            assert rc == 0 and ok == 0 and not np.any(out), (S, out, ok)
    Rn = np.eye(3)
    Rn[0, 0] = np.nan
    rc, out, ok = di.debug_pair_information(lib, good, good, Rn)
    assert rc == 0 and ok == 0 and not np.any(out)


def test_equal_voxels_halve_the_information():
    """S_source = S_target = S, R = I: the combined covariance is 2 Σ, so S_outᵀ S_out = ½ SᵀS"""
    lib = _lib()
    with mpmath.workdps(di.DPS):
        for St, _, _ in di.random_triples()[:200]:
            rc, S, ok = di.debug_pair_information(lib, St, St, np.eye(3))
            assert rc == 0 and ok == 1
            M = di._mpm(St)
            assert di.information_error(S, (M.T * M) / 2) <= di.bound()


def test_an_axis_rotation_is_a_permutation_of_the_source():
    """(S Rᵀ)ᵀ (S Rᵀ) = R SᵀS Rᵀ, and S Rᵀ is exact for a signed permutation: the result for (S_s, R) equals the one for
    the explicitly permuted source (S_s Rᵀ, I) — both within the bound of the same 50-digit value"""
    lib = _lib()
    triples = di.random_triples()
    with mpmath.workdps(di.DPS):
        for k, R in enumerate(mi.axis_rotations()):
            for St, Ss, _ in triples[8 * k:8 * k + 8]:
                A = di.pair_information_xp(St, Ss, R)
                rc, S, ok = di.debug_pair_information(lib, St, Ss, R)
                rc2, S2, ok2 = di.debug_pair_information(lib, St, Ss @ R.T, np.eye(3))
                assert (rc, ok, rc2, ok2) == (0, 1, 0, 1)
                assert di.information_error(S, A) <= di.bound()
                assert di.information_error(S2, A) <= di.bound()
                M2 = di._mpm(S2)
                assert di.information_error(S, M2.T * M2) <= 2.0 * di.bound()  # two results, each within the bound of A


def test_match_map_kernels_neither_spill_nor_use_scratch_and_the_point_matcher_keeps_its_budget():
    import kernel_resources
    obj = os.path.join(CSRC, "nos_voxelmap.o")
    assert os.path.exists(obj), "build with python __graft_entry__.py"
    kernels = kernel_resources.kernel_resources(obj)
    for form in ("nos::voxel_match_map_kernel<double>", "nos::voxel_match_map_kernel<float>"):
        mine = [k for k in kernels if form in k["name"]]
        assert len(mine) == 1, (form, [k["name"][:80] for k in kernels if "match_map" in k["name"]])
        k = mine[0]
        print("%s: %d VGPRs, %d spills, %d B scratch" % (form, k["vgpr"], k["spill"], k["scratch"]))
        assert k["spill"] == 0 and k["scratch"] == 0, (form, k["spill"], k["scratch"])
    for form in ("nos::voxel_match_kernel<double>", "nos::voxel_match_kernel<float>"):
        mine = [k for k in kernels if form in k["name"]]
        assert len(mine) == 1, form
        assert mine[0]["spill"] == 0 and mine[0]["scratch"] == 0 and mine[0]["vgpr"] <= 128, (form, mine[0])
