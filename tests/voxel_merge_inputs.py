"""Inputs and the 50-digit reference of the voxel-store merge (nos_voxel_map_merge) — TEST INFRASTRUCTURE
shared by test_voxel_map_merge_abi.py (CPU) and test_voxel_map_merge.py (GPU).

EXACT inputs: points are (cell + d) · resolution with every component of d a multiple of 2^-10 in [1/1024, 1023/1024] —
strictly inside the cell, because a 90° turn maps a lower face onto an upper one —, |cell| <= 64, at most 40 points per
voxel and a power-of-two resolution.  Under an axis rotation and a whole-cell translation every sum the merge forms is
then an integer multiple of 2^-20 res² below 2^53: exact in any order, so a merge must give the bits of an insert of the
transformed points.

GENERAL inputs are held against mpmath at 50 digits (the finish as oracle/oracle_voxel_xp.py states it, here on the union
of the TRANSFORMED points, which no float64 array holds)."""
import ctypes
import functools
import itertools

import mpmath
import numpy as np

from oracle import oracle_voxel_xp as vx

# rotation by 0.7 rad about (1, 2, 3) and a translation that is no multiple of any cell edge used below
GENERAL_AXIS, GENERAL_ANGLE = np.array([1.0, 2.0, 3.0]), 0.7
GENERAL_T = np.array([12.34, -5.67, 0.89])


def general_pose():
    a = GENERAL_AXIS / np.linalg.norm(GENERAL_AXIS)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(GENERAL_ANGLE) * K + (1.0 - np.cos(GENERAL_ANGLE)) * (K @ K), GENERAL_T.copy()


@functools.lru_cache(maxsize=None)
def axis_rotations():
    """the 24 proper rotations that map axes onto axes (signed permutation matrices of determinant +1)"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            R = np.zeros((3, 3))
            for i in range(3):
                R[i, perm[i]] = signs[i]
            if np.linalg.det(R) > 0:
                out.append(R)
    assert len(out) == 24
    return out


def axis_poses(resolution, seed=5):
    """every axis rotation with a whole-cell translation; both signs occur on every axis"""
    rng = np.random.default_rng(seed)
    shifts = rng.integers(-9, 10, size=(24, 3))
    shifts[0], shifts[1] = (7, -3, 5), (-7, 3, -5)
    return [(R, s.astype(np.float64) * resolution) for R, s in zip(axis_rotations(), shifts)]


def exact_points(cells, counts, resolution, seed):
    """→ points [N,3] (voxel after voxel), and the list of row ranges per voxel"""
    rng = np.random.default_rng(seed)
    pts, rows, start = [], [], 0
    for cell, n in zip(cells, counts):
        d = rng.integers(1, 1024, size=(n, 3)).astype(np.float64) / 1024.0
        pts.append((np.asarray(cell, dtype=np.float64) + d) * resolution)
        rows.append(np.arange(start, start + n))
        start += n
    return np.concatenate(pts), rows


def exact_voxels(n_voxels, resolution, seed, half=6):
    """n_voxels distinct cells of [-half, half)³ in random order, counts cycling through 1 … 40 (so voxels below
    min_points are among them) → (points, rows, cells [V,3])"""
    rng = np.random.default_rng(seed)
    side = np.arange(-half, half)
    grid = np.array(list(itertools.product(side, side, side)), dtype=np.int64)
    cells = grid[rng.permutation(len(grid))[:n_voxels]]
    counts = 1 + (np.arange(n_voxels) % 40)
    pts, rows = exact_points(cells, counts, resolution, seed + 1)
    return pts, rows, cells


@functools.lru_cache(maxsize=None)
def general_source():
    """320 voxels on the cells [-4, 4) x [-4, 4) x [-2, 3) of a 1 m grid, 3 … 40 points each, uniform in (0.1, 0.9) of the
    cell → (points [N,3], rows per voxel, cells [320,3])"""
    rng = np.random.default_rng(11)
    cells = np.array(list(itertools.product(range(-4, 4), range(-4, 4), range(-2, 3))), dtype=np.int64)
    pts, rows, start = [], [], 0
    for cell in cells:
        n = int(rng.integers(3, 41))  # drawn voxel by voxel, ahead of the voxel's points
        pts.append(cell + rng.uniform(0.1, 0.9, size=(n, 3)))
        rows.append(np.arange(start, start + n))
        start += n
    return np.concatenate(pts), rows, cells


def debug_voxel_moments(lib, count, sums, cell, res_src, R, t, res_dst):
    """nos_debug_voxel_moments → (status, cell_out [3] int64, sums_out [9])"""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    cell = np.ascontiguousarray(cell, dtype=np.int64)
    R = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(9))
    t = np.ascontiguousarray(t, dtype=np.float64)
    cell_out, sums_out = np.zeros(3, dtype=np.int64), np.zeros(9)
    rc = lib.nos_debug_voxel_moments(int(count), sums.ctypes.data_as(dp), cell.ctypes.data_as(ip), float(res_src),
                                     R.ctypes.data_as(dp), t.ctypes.data_as(dp), float(res_dst), cell_out.ctypes.data_as(ip),
                                     sums_out.ctypes.data_as(dp))
    return rc, cell_out, sums_out


# ---------------------------------------------------------------- 50 digits

def _mp(x):
    return mpmath.mpf(float(x))


def warp_xp(points, R, t):
    """R p + t of float64 points at 50 digits → list of [x, y, z] mpf rows (call inside mpmath.workdps(vx.DPS))"""
    Rm = [[_mp(R[i][j]) for j in range(3)] for i in range(3)]
    tm = [_mp(x) for x in t]
    return [[Rm[i][0] * _mp(p[0]) + Rm[i][1] * _mp(p[1]) + Rm[i][2] * _mp(p[2]) + tm[i] for i in range(3)] for p in points]


def mean_and_scatter_xp(q):
    """rows of mpf → (mean [3], scatter Σ (q − m)(q − m)ᵀ as a 3x3 list) at 50 digits"""
    n = len(q)
    m = [mpmath.fsum(r[k] for r in q) / n for k in range(3)]
    d = [[r[k] - m[k] for r in q] for k in range(3)]
    return m, [[mpmath.fdot(d[a], d[b]) for b in range(3)] for a in range(3)]


def cell_of_xp(m, resolution):
    """floor(m · inv_res) per axis with inv_res the float64 1.0 / resolution the library multiplies by → (cell, the
    smallest distance of m · inv_res from an integer, in cells)"""
    inv = _mp(1.0 / resolution)
    x = [m[k] * inv for k in range(3)]
    cell = tuple(int(mpmath.floor(v)) for v in x)
    return cell, float(min(min(v - mpmath.floor(v), mpmath.floor(v) + 1 - v) for v in x))


def finish_xp(q):
    """oracle_voxel_xp.voxel_stats_xp on rows of mpf (it takes float64 points; the transformed ones are not): the same
    dict — n, valid, mean (longdouble), eig, eig_floored, info, gaps.  The covariance is shift-invariant, so the corner
    voxel_stats_xp subtracts first is not needed at this precision."""
    n = len(q)
    out = {"n": n, "valid": False, "mean": np.zeros(3, dtype=np.longdouble), "eig": np.zeros(3), "eig_floored": np.zeros(3),
           "info": np.eye(3), "gaps": (np.inf, np.inf)}
    m, sc = mean_and_scatter_xp(q)
    out["mean"] = np.array([vx._to_ld(x) for x in m], dtype=np.longdouble)
    cov = mpmath.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            cov[a, b] = (sc[a][b] + (1 if a == b else 0)) / n
    w, U = mpmath.eigsy(cov)
    w = [w[k] for k in range(3)]
    out["eig"] = np.array([float(x) for x in w])
    out["gaps"] = (float((w[1] - w[0]) / w[2]), float((w[2] - w[1]) / w[2]))
    if n < vx.MIN_POINTS or w[2] < mpmath.mpf(vx.MIN_EIGENVALUE):
        return out
    floor = w[2] * mpmath.mpf(vx.EIG_FLOOR)
    wf = [max(w[0], floor), max(w[1], floor), w[2]]
    info = mpmath.matrix(3, 3)
    for k in range(3):
        for a in range(3):
            for b in range(3):
                info[a, b] += U[a, k] * U[b, k] / wf[k]
    out["valid"] = True
    out["eig_floored"] = np.array([float(x) for x in wf])
    out["info"] = np.array([[float(info[a, b]) for b in range(3)] for a in range(3)])
    return out


def bound_scale(res_src, res_dst):
    """L = √3 (2 res_src + res_dst): bounds every |d'| — |R d| <= √3 res_src, and b = (R o + t) − o' = (mu' − o') − R (s / n)
    with mu' inside the destination cell."""
    return np.sqrt(3.0) * (2.0 * res_src + res_dst)


def mean_ulp(cell_src, res_src, t, res_dst):
    """one ulp of ‖o‖₁ + ‖t‖∞ + L: the size of the quantities the mean's roundings happen on"""
    o = np.abs(np.asarray(cell_src, dtype=np.float64) * res_src).sum()
    return float(np.spacing(o + np.abs(t).max() + bound_scale(res_src, res_dst)))


@functools.lru_cache(maxsize=None)
def general_reference(res_dst):
    """The general pose on general_source(): per destination cell of a grid of edge res_dst, the 50-digit statistics of
    the union of the transformed points of the source voxels whose transformed MEAN falls there → dict cell → dict
    (finish_xp's keys + members: source voxel indices, ulp: the largest mean_ulp of its members), and the smallest
    distance of a transformed mean from a cell face (in cells)."""
    pts, rows, cells = general_source()
    R, t = general_pose()
    with mpmath.workdps(vx.DPS):
        groups, margin = {}, np.inf
        for v, r in enumerate(rows):
            q = warp_xp(pts[r], R, t)
            m, _ = mean_and_scatter_xp(q)
            cell, dist = cell_of_xp(m, res_dst)
            margin = min(margin, dist)
            g = groups.setdefault(cell, {"members": [], "q": []})
            g["members"].append(v)
            g["q"].extend(q)
        out = {}
        for cell, g in groups.items():
            st = finish_xp(g["q"])
            st["members"] = g["members"]
            st["ulp"] = max(mean_ulp(cells[v], 1.0, t, res_dst) for v in g["members"])
            out[cell] = st
    return out, margin
