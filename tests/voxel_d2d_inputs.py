"""Inputs and the 50-digit reference of the map-to-map match (nos_voxel_map_match_map) — TEST
INFRASTRUCTURE shared by test_voxel_map_match_map_abi.py (CPU) and test_voxel_map_match_map.py (GPU).

The quantity under test is the combined information of a voxel pair, A = (Σ_t + R Σ_s Rᵀ)⁻¹ with Σ_x = (S_xᵀ S_x)⁻¹.
Error measure: max|SᵀS − A_xp| / max|A_xp| for the S a routine returns, A_xp at 50 digits from the float64 inputs.
Yardstick: a plain numpy float64 restatement (inv, cholesky), scored against the same 50-digit values on the same
inputs.  BOUND: 4 x the restatement's worst error over random_triples() — the factor covers fused multiply-adds and a
different operation order; nothing in it comes from the code under test."""
import ctypes
import functools

import mpmath
import numpy as np

from tests import voxel_merge_inputs as mi

DPS = 50
EPS = 2.0 ** -52
N_TRIPLES = 2000


# ---------------------------------------------------------------- scenes

def shell_cells():
    """the cells of [-4,4) x [-4,4) x [-2,3) on its boundary: 212 of them"""
    cells = [(x, y, z) for x in range(-4, 4) for y in range(-4, 4) for z in range(-2, 3)
             if x in (-4, 3) or y in (-4, 3) or z in (-2, 2)]
    assert len(cells) == 212
    return np.array(cells, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def shell_points():
    """5 … 40 points per shell cell, uniform in (0.1, 0.9) of the cell and squeezed to (0.45, 0.55) along the wall normal
    (x for an x wall, else y for a y wall, else z): thin plates, every eigenvalue floor in use → points [N,3]"""
    rng = np.random.default_rng(17)
    pts = []
    for cell in shell_cells():
        n = int(rng.integers(5, 41))
        d = rng.uniform(0.1, 0.9, size=(n, 3))
        normal = 0 if cell[0] in (-4, 3) else 1 if cell[1] in (-4, 3) else 2
        d[:, normal] = rng.uniform(0.45, 0.55, size=n)
        pts.append(cell + d)
    return np.concatenate(pts)


def rot_axis(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def shell_pose():
    """T: 90° about z (entries exactly 0 and ±1), t = (3, −2, 1)"""
    return np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]), np.array([3.0, -2.0, 1.0])


def moved_by_inverse(points, R, t):
    """p → Rᵀ (p − t): the points as a frame at pose (R, t) sees them"""
    return (points - t) @ R


def shell_starts():
    """four starts: T perturbed by ≤ 0.15 m per axis and about 2°, fixed seeds"""
    R, t = shell_pose()
    out = []
    for seed in (1, 2, 3, 4):
        rng = np.random.default_rng(seed)
        axis = rng.normal(size=3)
        out.append((R @ rot_axis(axis, np.deg2rad(2.0)), t + rng.uniform(-0.15, 0.15, size=3)))
    return out


def general_pair():
    """target points = voxel_merge_inputs.general_source(), source points = the same moved by the inverse of
    general_pose(), and the pose to match at: general_pose() perturbed by 0.05 m and 0.5° → (target, source, R, t)"""
    pts, _, _ = mi.general_source()
    R, t = mi.general_pose()
    d = np.array([2.0, -1.0, 2.0]) / 3.0 * 0.05
    return pts, moved_by_inverse(pts, R, t), R @ rot_axis([3.0, -1.0, 2.0], np.deg2rad(0.5)), t + d


# ---------------------------------------------------------------- the pair information: 50 digits, numpy, the hook

def _mpm(M):
    M = np.asarray(M, dtype=np.float64).reshape(3, 3)
    return mpmath.matrix([[mpmath.mpf(float(M[i, j])) for j in range(3)] for i in range(3)])


def pair_information_xp(St, Ss, R):
    """A = ((StᵀSt)⁻¹ + R (SsᵀSs)⁻¹ Rᵀ)⁻¹ at 50 digits → mpmath matrix (call inside mpmath.workdps(DPS))"""
    St, Ss, R = _mpm(St), _mpm(Ss), _mpm(R)
    return mpmath.inverse(mpmath.inverse(St.T * St) + R * mpmath.inverse(Ss.T * Ss) * R.T)


def information_error(S, A_xp):
    """max|SᵀS − A_xp| / max|A_xp| with SᵀS formed at 50 digits from the float64 S (call inside mpmath.workdps(DPS))"""
    S = _mpm(S)
    D = S.T * S - A_xp
    return float(max(abs(D[i, j]) for i in range(3) for j in range(3)) / max(abs(A_xp[i, j]) for i in range(3) for j in range(3)))


def pair_information_np(St, Ss, R):
    """the yardstick: plain float64 numpy, `inv` and `cholesky` → S = Lᵀ with L Lᵀ = A = C⁻¹, C the combined covariance"""
    C = np.linalg.inv(St.T @ St) + R @ np.linalg.inv(Ss.T @ Ss) @ R.T
    return np.linalg.cholesky(np.linalg.inv(C)).T


def debug_pair_information(lib, St, Ss, R):
    """nos_debug_voxel_pair_information → (status, S_out [3,3], ok)"""
    dp = ctypes.POINTER(ctypes.c_double)
    a = [np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(9)) for x in (St, Ss, R)]
    out, ok = np.full(9, 7.0), ctypes.c_ubyte(9)
    rc = lib.nos_debug_voxel_pair_information(a[0].ctypes.data_as(dp), a[1].ctypes.data_as(dp), a[2].ctypes.data_as(dp),
                                              out.ctypes.data_as(dp), ctypes.byref(ok))
    return rc, out.reshape(3, 3), int(ok.value)


def _random_rotation(rng):
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


def random_sqrt_info(rng):
    """S = D^-1/2 Vᵀ as the voxel finish forms it: largest eigenvalue in [0.01, 3], the other two anywhere below it and
    floored at 0.01 of it (so about a third of them sit on the floor)"""
    top = rng.uniform(0.01, 3.0)
    w = np.array([max(top * 10.0 ** rng.uniform(-3.0, 0.0), 0.01 * top) for _ in range(2)] + [top])
    return np.diag(1.0 / np.sqrt(w)) @ _random_rotation(rng).T


@functools.lru_cache(maxsize=None)
def random_triples():
    """N_TRIPLES x (S_target, S_source, R), seed 3"""
    rng = np.random.default_rng(3)
    return [(random_sqrt_info(rng), random_sqrt_info(rng), _random_rotation(rng)) for _ in range(N_TRIPLES)]


@functools.lru_cache(maxsize=None)
def random_references():
    """the 50-digit A of every triple"""
    with mpmath.workdps(DPS):
        return [pair_information_xp(*tr) for tr in random_triples()]


@functools.lru_cache(maxsize=None)
def numpy_worst_error():
    """the worst information_error of pair_information_np over random_triples()"""
    with mpmath.workdps(DPS):
        return max(information_error(pair_information_np(*tr), A) for tr, A in zip(random_triples(), random_references()))


def bound():
    return 4.0 * numpy_worst_error()
