"""The extended-precision voxel reference (oracle/oracle_voxel_xp.py) itself, the input families of tests/voxel_inputs.py,
and the per-voxel finish as the HOST computes it (nos_debug_voxel_finish: csrc/voxel_finish.hpp compiled for the CPU) —
all without a GPU.  The device code is held to the same bounds in test_voxel_stats_xprec.py."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_scene as scene
from oracle import oracle_voxel_xp as vx
from tests import voxel_inputs as VI


def test_longdouble_is_extended():
    assert np.finfo(np.longdouble).eps < 1.2e-19


CLOUDS = VI.CLOUDS


def test_the_oracle_agrees_with_a_longdouble_evaluation_on_every_family():
    """50 digits against longdouble sums about the corner and LAPACK's fp64 eigh: backward error a few eps ‖cov‖, times
    the condition number 100 that flooring leaves → 1e-13; the bound is 1e-12.  (The issue measured 4e-13.)"""
    worst = 0.0
    for key in CLOUDS:
        c = VI.cloud(*CLOUDS[key])
        for v, r in zip(c.voxels, VI.reference(c)):
            mean, wf, info, valid = vx.voxel_stats_ld(c.points[v["idx"]], v["cell"], c.resolution)
            assert valid == r["valid"], (key, v["name"], v["offset"])
            if not valid:
                continue
            assert np.abs(mean - r["mean"]).max() <= 4 * np.finfo(np.longdouble).eps * np.abs(c.points[v["idx"]]).max()
            assert np.abs(wf / r["eig_floored"] - 1.0).max() < 1e-13, (key, v["name"], v["offset"])
            e = np.linalg.norm(info - r["info"]) / np.linalg.norm(r["info"])
            worst = max(worst, e)
            assert e < 1e-12, (key, v["name"], v["offset"], e)
    print("oracle vs longdouble: worst information error %.2e" % worst)


def test_the_oracle_agrees_with_the_scene_oracle_on_the_room():
    """oracle_scene.build_ndt_map (fp64 numpy, raw sums: the harness formula as written) on the reference's room scene,
    every eighth of its 96 voxels: within 10 m of the origin raw sums cancel eps |p|² ≈ 1e-14, times the condition
    number 100 → 1e-12 on the information matrix; bound 1e-11.  Counts, validity and cells are equal."""
    pts = scene.generate_global_points()
    m = scene.build_ndt_map(pts, 1.0, proper_transpose=True)
    cells = np.floor(pts).astype(np.int64)
    assert len(m["valid"]) == 96
    for k in range(0, 96, 8):
        cell = m["cells"][k]
        mine = pts[np.all(cells == cell, axis=1)]
        r = vx.voxel_stats_xp(mine, cell, 1.0)
        assert r["n"] == m["count"][k] and r["valid"] == m["valid"][k]
        info, lam, ortho = vx.information_from_sqrt(m["sqrt_infos"][k], True)
        assert np.abs(m["means"][k] - r["mean"].astype(np.float64)).max() < 1e-13
        assert np.abs(np.maximum(m["eigvals"][k], 0.01 * m["eigvals"][k][2]) / r["eig_floored"] - 1.0).max() < 1e-11
        assert np.linalg.norm(info - r["info"]) / np.linalg.norm(r["info"]) < 1e-11
        assert ortho < 1e-13


def test_the_information_matrix_is_recovered_from_either_formula():
    """S = D^-1/2 Vᵀ (proper) and S = D^-1/2 V (harness formula) of one decomposition give the same information matrix
    and eigenvalues back, whatever the signs of the eigenvectors."""
    rng = np.random.default_rng(3)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.array([1.0, -1.0, 1.0])
    lam = np.array([0.002, 0.05, 0.2])
    want = (Q / lam) @ Q.T
    for proper, S in ((True, (Q / np.sqrt(lam)).T), (False, Q / np.sqrt(lam)[:, None])):
        info, got_lam, ortho = vx.information_from_sqrt(S, proper)
        assert np.allclose(info, want, rtol=1e-14, atol=1e-13) and np.allclose(got_lam, lam, rtol=1e-14) and ortho < 1e-14


def test_the_families_are_what_they_claim():
    c = VI.cloud(*CLOUDS["res1"])
    ref = VI.reference(c)
    fam = VI.families()
    at0 = {v["name"]: r for v, r in zip(c.voxels, ref) if v["offset"] == 0}
    rows = lambda a: a[np.lexsort(a.T[::-1])]
    # translation is exact for the lattice families: at every offset the statistics are those of offset 0, shifted
    for v, r in zip(c.voxels, ref):
        if VI.on_lattice(v["name"]):
            shift = np.array(v["cell"], dtype=np.float64)
            assert np.array_equal(rows(c.points[v["idx"]] - shift), rows(fam[v["name"]])), (v["name"], v["offset"])
            assert np.array_equal(r["eig"], at0[v["name"]]["eig"]) and r["valid"] == at0[v["name"]]["valid"]
    assert not at0["random_4"]["valid"] and at0["random_5"]["valid"]
    assert at0["lattice_plane"]["gaps"][1] == 0.0 and at0["lattice_plane"]["gaps"][0] > 0.1
    line = at0["lattice_line"]
    assert line["gaps"][0] == 0.0 and line["eig"][1] < line["eig_floored"][1] == line["eig_floored"][0] == 0.01 * line["eig"][2]
    assert at0["lattice_line_unfloored"]["gaps"][0] == 0.0
    assert at0["lattice_cube"]["gaps"] == (0.0, 0.0)
    # near-ties on both sides of the tie rule (gap <= 1e-9 of the largest eigenvalue)
    for g, inside in ((1e-12, True), (1e-10, True), (1e-8, False), (1e-6, False), (1e-4, False)):
        for name in ("near_tie_%g" % g, "near_tie_%g_rotated" % g):
            gap = at0[name]["gaps"][1]
            assert 0.2 * g < gap < 2.0 * g, (name, gap)
            assert (gap <= vx.TIE_RULE) == inside and (vx.merged_gap(at0[name]) > 0) == inside
    # slabs: the smallest eigenvalue within a few percent of the floor, one on each side
    above, below = at0["slab_above_floor"], at0["slab_below_floor"]
    assert 1.0 < above["eig"][0] / (0.01 * above["eig"][2]) < 1.03 and above["eig_floored"][0] == above["eig"][0]
    assert 0.97 < below["eig"][0] / (0.01 * below["eig"][2]) < 1.0 and below["eig_floored"][0] > below["eig"][0]
    # slivers: the largest eigenvalue at 0.01 (1 ± 1e-6)
    assert at0["sliver_valid"]["valid"] and abs(at0["sliver_valid"]["eig"][2] / 0.01 - 1.0 - 1e-6) < 1e-8
    assert not at0["sliver_invalid"]["valid"] and abs(at0["sliver_invalid"]["eig"][2] / 0.01 - 1.0 + 1e-6) < 1e-8
    # three batches split every voxel
    batches = VI.three_batches(c)
    assert sum(len(b) for b in batches) == len(c.points)
    for v in c.voxels:
        assert all(np.intersect1d(v["idx"], b).size > 0 for b in batches), v["name"]


def _host_finish(lib, c, proper):
    """every voxel of the cloud through nos_debug_voxel_finish, on numpy sums about the corner → a stats dict"""
    dp = ctypes.POINTER(ctypes.c_double)
    V = len(c.voxels)
    out = {"means": np.zeros((V, 3)), "sqrt_infos": np.zeros((V, 3, 3)), "valid": np.zeros(V, dtype=bool),
           "counts": np.zeros(V, dtype=np.uint32), "cells": np.zeros((V, 3), dtype=np.int64)}
    params = np.array([5.0, 0.01, 0.01])
    for k, v in enumerate(c.voxels):
        n, sums = VI.corner_sums(c.points[v["idx"]], v["cell"], c.resolution)
        cell = np.array(v["cell"], dtype=np.int64)
        mean, S, ok = np.zeros(3), np.zeros(9), ctypes.c_ubyte(7)
        rc = lib.nos_debug_voxel_finish(n, sums.ctypes.data_as(dp), cell.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        ctypes.c_double(c.resolution), params.ctypes.data_as(dp), int(proper),
                                        mean.ctypes.data_as(dp), S.ctypes.data_as(dp), ctypes.byref(ok))
        assert rc == 0
        out["means"][k], out["sqrt_infos"][k], out["valid"][k] = mean, S.reshape(3, 3), bool(ok.value)
        out["counts"][k], out["cells"][k] = n, cell
    return out


@pytest.mark.parametrize("proper", [True, False], ids=["proper", "harness_formula"])
@pytest.mark.parametrize("key", list(CLOUDS))
def test_the_host_finish_meets_the_bounds_on_every_family(key, proper):
    """voxel_finish and symmetric_eigen3 compiled for the host, fed with sums about the cell corner: counts, validity,
    mean within 2 ulp, floored eigenvalues within 1e-11, information matrix within 1e-10 + merged gap (voxel_inputs)."""
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    c = VI.cloud(*CLOUDS[key])
    worst = VI.compare(c, VI.reference(c), _host_finish(lib, c, proper), proper, "host finish")
    print("host finish, %s, %s: worst mean %.2f ulp, eigenvalues %.1e, information %.1e" %
          (key, "proper" if proper else "harness", max(w[0] for w in worst.values()), max(w[1] for w in worst.values()),
           max(w[2] for w in worst.values())))


def test_the_host_finish_rejects_bad_arguments():
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    dp = ctypes.POINTER(ctypes.c_double)
    sums, params, mean, S = np.zeros(9), np.array([5.0, 0.01, 0.01]), np.zeros(3), np.zeros(9)
    cell, ok = np.zeros(3, dtype=np.int64), ctypes.c_ubyte(0)
    args = lambda res, flags: (8, sums.ctypes.data_as(dp), cell.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.c_double(res),
                               params.ctypes.data_as(dp), flags, mean.ctypes.data_as(dp), S.ctypes.data_as(dp), ctypes.byref(ok))
    assert lib.nos_debug_voxel_finish(*args(1.0, 0)) == 0 and ok.value == 1   # eight points at the corner: cov = I / 8
    assert lib.nos_debug_voxel_finish(*args(0.0, 0)) != 0
    assert lib.nos_debug_voxel_finish(*args(1.0, 2)) != 0   # NOS_MAP_REFERENCE_EXACT has its own kernels
