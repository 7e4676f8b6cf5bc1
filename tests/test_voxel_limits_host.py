"""The voxel store at its 32-bit count limit, without a GPU: the per-voxel finish and the moment transform as the HOST
compiles them (nos_debug_voxel_finish, nos_debug_voxel_moments) at counts up to 2^32 − 1, against 50 digits; the
host-side tile cache on both sides of the stamp wrap; the shared model's rejection rule.

A conversion of the count through int or float anywhere on the way would show at 2^24 + 1, 2^31 and 2^32 − 1 and
nowhere below; the statistics had only been compared with extended precision at counts up to 1000."""
import ctypes
import functools

import mpmath
import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import pipeline
from oracle import oracle_voxel_xp as vx
from tests import voxel_inputs as vi
from tests import voxel_limit_inputs as li
from tests import voxel_merge_inputs as mi
from tests.voxel_store_model import COUNT_MAX, Model, Rejected

COUNTS = (5, 2 ** 24 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 2, 2 ** 32 - 1)
EDGE = (1 << 20) - 1
CELLS = ((0, 0, 0), (EDGE, -EDGE, EDGE), (-EDGE, EDGE, -EDGE))
RESOLUTIONS = (1.0, 0.5)
N_VOXELS, N_TIGHT = 50, 10


def _lib():
    from nonlinear_optimizer_for_slam_amd import _lib as L
    return L.hip_lib()


def _host_finish(lib, count, sums, cell, res, proper):
    dp = ctypes.POINTER(ctypes.c_double)
    params = np.array([5.0, 0.01, 0.01])
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    cell = np.array(cell, dtype=np.int64)
    mean, S, ok = np.zeros(3), np.zeros(9), ctypes.c_ubyte(7)
    rc = lib.nos_debug_voxel_finish(int(count), sums.ctypes.data_as(dp), cell.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    ctypes.c_double(res), params.ctypes.data_as(dp), int(proper), mean.ctypes.data_as(dp),
                                    S.ctypes.data_as(dp), ctypes.byref(ok))
    assert rc == 0
    return mean, S.reshape(3, 3), bool(ok.value)


def _numpy_finish(count, sums, cell, res):
    """the finish in plain float64 numpy from the same sums → (mean, information, valid): what the bounds must leave room for"""
    n = float(count)
    m = sums[:3] / n
    M = np.array([[sums[3], sums[4], sums[5]], [sums[4], sums[6], sums[7]], [sums[5], sums[7], sums[8]]])
    w, U = np.linalg.eigh((M + np.eye(3)) / n - np.outer(m, m))
    if count < 5 or w[2] < 0.01:
        return np.zeros(3), np.eye(3), False
    wf = np.maximum(w, 0.01 * w[2])
    return np.array(cell, dtype=np.float64) * res + m, (U / wf) @ U.T, True


@functools.lru_cache(maxsize=None)
def _voxels(count, res):
    """50 seeded lattice voxels of `count` points (the first 10 too thin to be valid at a huge count) → (sums [50,9], and
    per cell of CELLS the 50-digit finish of every voxel)"""
    rng = np.random.default_rng(1000 + COUNTS.index(count) if count in COUNTS else 999)
    mk, qk = li.lattice_moments(rng, N_VOXELS, tight=np.arange(N_VOXELS) < N_TIGHT)
    sums = li.exact_sums([count] * N_VOXELS, mk, qk, res)
    return sums, {cell: [li.finish_xp(count, sums[v], cell, res) for v in range(N_VOXELS)] for cell in CELLS}


@pytest.mark.parametrize("count", (4,) + COUNTS)
def test_the_host_finish_at_huge_counts_against_50_digits(count):
    """nos_debug_voxel_finish from a count and nine exact sums, both flags, at cell 0 and at ±(2^20 − 1), on 1 m and 0.5 m
    grids: validity EQUAL to the 50-digit finish (a voxel of 4 points is invalid, a thin one is valid at 5 points and
    invalid at 2^32 − 1), and for valid voxels the bounds of tests/voxel_inputs.py as they are.  A float64 numpy finish
    from the same sums is held to the same bounds, so they are known to leave room for a correct implementation."""
    lib = _lib()
    worst, worst_np, n_valid = [0.0, 0.0, 0.0], [0.0, 0.0], 0
    for res in RESOLUTIONS:
        sums, refs = _voxels(count, res)
        for cell in CELLS:
            for v in range(N_VOXELS):
                ref = refs[cell][v]
                assert abs(ref["eig"][2] - 0.01) > 1e-9  # validity is not decided by rounding
                np_mean, np_info, np_valid = _numpy_finish(count, sums[v], cell, res)
                assert np_valid == ref["valid"]
                for proper in (True, False):
                    mean, S, ok = _host_finish(lib, count, sums[v], cell, res, proper)
                    tag = (count, res, cell, v, proper)
                    assert ok == ref["valid"], tag
                    if not ok:
                        assert np.array_equal(S, np.eye(3)), tag
                        continue
                    e_mean, e_eig, e_ortho, e_info, gap = li.finish_errors(ref, mean, S, proper)
                    worst = [max(worst[0], e_mean), max(worst[1], e_eig), max(worst[2], e_info - gap)]
                    assert e_mean <= vi.MEAN_ULPS and e_eig <= vi.EIG_RTOL and e_ortho <= vi.ORTHO_TOL, (tag, e_mean, e_eig, e_ortho)
                    assert e_info <= vi.INFO_RTOL + gap, (tag, e_info, gap)
                if ref["valid"]:
                    n_valid += 1
                    ulp = np.spacing(float(np.abs(ref["mean"]).max()))
                    e = [float(np.abs(np_mean.astype(np.longdouble) - ref["mean"]).max() / ulp),
                         float(np.linalg.norm(np_info - ref["info"]) / np.linalg.norm(ref["info"]))]
                    worst_np = [max(worst_np[0], e[0]), max(worst_np[1], e[1])]
                    assert e[0] <= vi.MEAN_ULPS and e[1] <= vi.INFO_RTOL + vx.merged_gap(ref), (count, res, cell, v, e)
    total = len(RESOLUTIONS) * len(CELLS) * N_VOXELS
    thin_valid = sum(bool(refs[cell][v]["valid"]) for res in RESOLUTIONS for refs in [_voxels(count, res)[1]] for cell in CELLS
                     for v in range(N_TIGHT))
    if count < 5:
        assert n_valid == 0
    elif count == 5:
        assert n_valid == total  # I / 5 alone passes the 0.01 of the validity rule
    else:  # the thin ones are invalid without it; most of the others are valid (on the 0.5 m grid not all of them)
        assert thin_valid == 0 and n_valid >= total // 2
    print("host finish at %d points: %d valid of %d, worst mean %.2f ulp, eigenvalues %.1e, information %.1e "
          "(numpy float64: mean %.2f ulp, information %.1e)" % (count, n_valid, total, worst[0], worst[1], worst[2], worst_np[0], worst_np[1]))


# ------------------------------------------------------------------------------------------------ the moment transform

def _moments_xp(count, sums, cell, res_src, R, t):
    """mean and scatter of the transformed voxel from its count and sums, at 50 digits (inside workdps)"""
    n = int(count)
    s = [mpmath.mpf(float(x)) for x in sums[:3]]
    M = [[mpmath.mpf(float(sums[3 + i])) for i in row] for row in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
    o = [mpmath.mpf(int(c)) * mpmath.mpf(float(res_src)) for c in cell]
    Rm = [[mpmath.mpf(float(R[i][j])) for j in range(3)] for i in range(3)]
    mu = [o[k] + s[k] / n for k in range(3)]
    m = [Rm[i][0] * mu[0] + Rm[i][1] * mu[1] + Rm[i][2] * mu[2] + mpmath.mpf(float(t[i])) for i in range(3)]
    sc = [[M[a][b] - s[a] * s[b] / n for b in range(3)] for a in range(3)]
    out = [[sum(Rm[a][i] * sc[i][j] * Rm[b][j] for i in range(3) for j in range(3)) for b in range(3)] for a in range(3)]
    return m, out


@pytest.mark.parametrize("count", [2 ** 31, 2 ** 32 - 1])
def test_the_host_moment_transform_at_huge_counts_against_50_digits(count):
    """nos_debug_voxel_moments at 2^31 and 2^32 − 1 points under the identity, a translation by whole cells and a general
    rotation, with the yardstick of test_voxel_map_merge_abi.py as it is: the mean the finish will form within 8 ulp
    (voxel_merge_inputs.mean_ulp), the scatter within 128 · 2^-52 n L² (bound_scale).  That bound grows with n as the
    scatter itself does: it is asserted to stay below 1e-9 of the scatter here, so it cannot hide a failure.  Under the
    first two poses the sums come back bit for bit."""
    lib = _lib()
    res_src = 1.0
    rng = np.random.default_rng(count % 1000)
    mk, qk = li.lattice_moments(rng, 20)
    sums = li.exact_sums([count] * 20, mk, qk, res_src)
    cells = rng.integers(-64, 65, size=(20, 3))
    Rg, tg = mi.general_pose()
    poses = (("identity", np.eye(3), np.zeros(3), 1.0), ("whole cells", np.eye(3), np.array([7.0, -3.0, 5.0]), 1.0),
             ("general, to 0.5 m", Rg, tg, 0.5), ("general, to 1 m", Rg, tg, 1.0))
    worst = {}
    for name, R, t, res_dst in poses:
        L = mi.bound_scale(res_src, res_dst)
        w = worst.setdefault(name, [0.0, 0.0, 0.0])
        for v in range(20):
            rc, cell_out, out = mi.debug_voxel_moments(lib, count, sums[v], cells[v], res_src, R, t, res_dst)
            assert rc == 0
            with mpmath.workdps(vx.DPS):
                m, sc = _moments_xp(count, sums[v], cells[v], res_src, R, t)
                cell, dist = mi.cell_of_xp(m, res_dst)
                assert dist >= 1e-6, (name, v, dist)  # the cell is not decided by rounding
                assert tuple(int(x) for x in cell_out) == cell, (name, v)
                o = [mpmath.mpf(float(np.float64(cell[k]) * np.float64(res_dst))) for k in range(3)]
                s = [mpmath.mpf(float(x)) for x in out[:3]]
                M = [[mpmath.mpf(float(out[3 + i])) for i in row] for row in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
                mean_err = float(max(abs(o[k] + s[k] / count - m[k]) for k in range(3)))
                scatter_err = float(max(abs(M[a][b] - s[a] * s[b] / count - sc[a][b]) for a in range(3) for b in range(3)))
                scatter_size = float(max(abs(sc[a][a]) for a in range(3)))
            ulp = mi.mean_ulp(cells[v], res_src, t, res_dst)
            bound = 128.0 * 2.0 ** -52 * count * L * L
            w[0], w[1], w[2] = max(w[0], mean_err / ulp), max(w[1], scatter_err / bound), max(w[2], bound / scatter_size)
            assert bound / scatter_size < 1e-9, (name, v, bound / scatter_size)
            assert mean_err <= 8.0 * ulp, (name, v, mean_err / ulp)
            assert scatter_err <= bound, (name, v, scatter_err / bound)
            if name in ("identity", "whole cells"):
                assert out.tobytes() == sums[v].tobytes() and np.array_equal(cell_out, cells[v] + (t / res_dst).astype(np.int64))
    for name, w in worst.items():
        print("moments at %d points, %s: worst mean %.3f ulp (bound 8), scatter %.4f of its bound (the bound is %.1e of the scatter)"
              % (count, name, w[0], w[1], w[2]))


# ---------------------------------------------------------------------------------- the tile cache across the stamp wrap

def _cache_state(cells, stamps, epoch, seed):
    rng = np.random.default_rng(seed)
    n = len(cells)
    return {"cells": np.asarray(cells, dtype=np.int64), "counts": rng.integers(1, 50, size=n).astype(np.uint32),
            "sums": rng.normal(size=(n, 9)), "stamps": np.asarray(stamps, dtype=np.uint32), "epoch": epoch,
            "voxel_resolution": 0.5, "search_radius_sq": 1.0, "proper_sqrt_information": True}


def test_the_tile_cache_keeps_the_last_stamp_and_the_largest_epoch_across_the_wrap():
    """combine_cells: "stamp the last one's" holds when the earlier stamp is just below 2^32 and the later one just above
    0 — the later ARRIVAL wins, not the larger number —, and the other way round.  TileCache.take reports the largest
    64-bit epoch put() has seen when one state has epoch 2^32 − 1 and the next 2^32 + 2."""
    cells = np.array([[1, 2, 3], [4, 5, 6], [-7, 8, -9]])
    u, n, s, t = pipeline.combine_cells(np.concatenate([cells, cells]), [1] * 6, np.ones((6, 9)),
                                        [0xFFFFFFFE, 0xFFFFFFFF, 5, 1, 2, 0xFFFFFFFD])
    order = np.lexsort(cells.T[::-1])
    assert np.array_equal(u, cells[order]) and np.array_equal(n, [2, 2, 2])
    assert t.dtype == np.uint32 and np.array_equal(t, np.array([1, 2, 0xFFFFFFFD], dtype=np.uint32)[order])
    a = _cache_state(cells, [0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF], (1 << 32) - 1, 1)
    b = _cache_state(cells[:2], [0, 2], (1 << 32) + 2, 2)
    for first, second in ((a, b), (b, a)):
        cache = pipeline.TileCache(4)
        cache.put(first), cache.put(second)
        back = cache.take_all()
        assert back["epoch"] == (1 << 32) + 2 and back["stamps"].dtype == np.uint32
        row = {tuple(c): k for k, c in enumerate(back["cells"])}
        for k, c in enumerate(cells[:2]):  # the later arrival's stamp
            assert int(back["stamps"][row[tuple(c)]]) == int(second["stamps"][k] if second is b else a["stamps"][k]), (k, second is b)
            assert int(back["counts"][row[tuple(c)]]) == int(a["counts"][k]) + int(b["counts"][k])
        assert int(back["stamps"][row[tuple(cells[2])]]) == 0xFFFFFFFF
    # a cache that only ever saw the earlier state reports its epoch, all 32 bits and no more
    cache = pipeline.TileCache(4)
    cache.put(a)
    assert cache.take_all()["epoch"] == (1 << 32) - 1


# --------------------------------------------------------------------------------------------------- the model's own rule

def test_the_model_rejects_what_takes_a_voxel_past_the_count_limit_and_changes_nothing():
    res = 0.5
    rng = np.random.default_rng(5)
    cells = np.array([[0, 0, 0], [3, -2, 1], [-4, 4, 0]])
    model = Model(res)
    model.insert(np.concatenate([li.lattice_points(rng, c, 6, res) for c in cells]))
    at = model.slot[int(li._pack(cells[1:2])[0])]
    model.counts[at] = COUNT_MAX - 7  # as restore() takes counts: as given
    seven = li.lattice_points(rng, cells[1], 7, res)
    eight = np.concatenate([li.lattice_points(rng, cells[0], 5, res), li.lattice_points(rng, cells[1], 8, res),
                            li.lattice_points(rng, [9, 9, 9], 4, res)])
    source = Model(res)
    source.insert(eight)
    for name, call in (("insert", lambda m: m.insert(eight)), ("insert_scan", lambda m: m.insert_scan(eight, np.eye(3), np.zeros(3))),
                       ("merge", lambda m: m.merge(source)), ("add", lambda m: m.add(source))):
        m = model.clone()
        before = (m.observable(), m.stamp.tobytes(), m.sums.tobytes(), len(m.history))
        with pytest.raises(Rejected) as e:
            call(m)
        assert (m.observable(), m.stamp.tobytes(), m.sums.tobytes(), len(m.history)) == before, name
        assert len(e.value.rows) == 8, name
    m = model.clone()
    assert m.insert(seven) == 1 and int(m.counts[at]) == COUNT_MAX and m.epoch == model.epoch + 1  # landing on the limit
    with pytest.raises(Rejected):
        m.insert(seven[:1])
    assert m.insert(np.concatenate([eight[:5], eight[13:]])) == 2  # the batch without the offending points
