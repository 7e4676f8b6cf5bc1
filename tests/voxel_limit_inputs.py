"""Voxel stores at the two 32-bit limits of include/nos.h — a voxel holds at most 2^32 − 1 points, stamps are the low 32
bits of the epoch — TEST INFRASTRUCTURE shared by test_voxel_limits_host.py (CPU) and test_voxel_limits.py (GPU).  No test
lives here and nothing here needs a GPU.

Nobody can hold 2^32 points, so a voxel is made from its statistics.  About the corner of its cell, in units of the cell
edge: a mean m on the 2^-5 lattice in (0, 1) and second moments per point q = m mᵀ + c on the 2^-10 lattice, c symmetric
and strictly diagonally dominant (positive definite), every q below 1.  A voxel of N points has the sums N m res and
N q res².  Batch points are (cell + j / 1024) res.  Every first-moment sum is then an integer below 2^53 in units of
2^-10 res, every second-moment sum one in units of 2^-20 res² (N q < 2^32 · 2^20 units): store + batch is exact in
float64 in any order, and what export() must show is computed here in Python integers (apply_batch)."""
import fractions

import mpmath
import numpy as np

from oracle import oracle_voxel_xp as vx
from tests.voxel_store_model import COUNT_MAX, Rejected, _cells_of, _pack

WRAP = 1 << 32
# slot → k: the voxel holds COUNT_MAX − k points.  Slot 3 is full; 255 and 256 (the last lane of the first 256-lane block
# and the first lane of the second) sit 7 below the limit; 299 (the last lane of a partial block) holds 2^31 − 1
BRIM = {3: 0, 255: 7, 256: 7, 299: 1 << 31}
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
STATE_KEYS = ("cells", "counts", "sums", "stamps")


def sheet_cells(n_voxels, seed):
    """n_voxels distinct cells of a wavy sheet over 20 x 20 cells (heights within one cell), in the order a seeded draw
    of points meets them"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-10.0, 10.0, size=(40 * n_voxels, 2))
    z = 0.45 * np.sin(xy[:, 0] * 0.9) + 0.35 * np.cos(xy[:, 1] * 0.7) + rng.normal(scale=0.02, size=xy.shape[0])
    cells = np.floor(np.column_stack([xy, z])).astype(np.int64)
    _, first = np.unique(cells, axis=0, return_index=True)
    cells = cells[np.sort(first)]
    assert cells.shape[0] >= n_voxels
    return cells[:n_voxels]


def lattice_moments(rng, n, tight=None):
    """→ (mk [n,3], qk [n,6]): means mk / 32 and second moments per point qk / 1024 in units of the cell edge (PAIRS order),
    qk = mk mkᵀ + ck with ck diagonally dominant: diagonal 20 … 80 (tight[v]: 2 … 6, a voxel too thin to be valid once
    the 1 / N of the finish's identity is gone), off-diagonals within ±8 (tight: ±1)."""
    tight = np.zeros(n, dtype=bool) if tight is None else np.asarray(tight, dtype=bool)
    mk = rng.integers(1, 29, size=(n, 3))
    diag = np.where(tight[:, None], rng.integers(3, 7, size=(n, 3)), rng.integers(20, 81, size=(n, 3)))
    off = np.where(tight[:, None], rng.integers(-1, 2, size=(n, 3)), rng.integers(-8, 9, size=(n, 3)))  # xy, xz, yz
    ck = np.stack([diag[:, 0], off[:, 0], off[:, 1], diag[:, 1], off[:, 2], diag[:, 2]], axis=1)
    qk = np.stack([mk[:, a] * mk[:, b] for a, b in PAIRS], axis=1) + ck
    rows = np.stack([np.abs(off[:, 0]) + np.abs(off[:, 1]), np.abs(off[:, 0]) + np.abs(off[:, 2]),
                     np.abs(off[:, 1]) + np.abs(off[:, 2])], axis=1)
    assert qk.max() < 1024 and np.all(rows < diag)
    return mk.astype(np.int64), qk.astype(np.int64)


def sum_units(res):
    """→ [9] the units the nine sums are integers in: 2^-10 res for the first moments, 2^-20 res² for the second"""
    return np.array([res * 2.0 ** -10] * 3 + [res * res * 2.0 ** -20] * 6)


def exact_sums(counts, mk, qk, res):
    """→ sums [n,9] float64 = N m res | N q res², every one asserted to be exactly that number (fractions.Fraction)"""
    units = sum_units(res)
    out = np.zeros((len(counts), 9))
    for v, N in enumerate(counts):
        ints = [int(N) * int(k) * 32 for k in mk[v]] + [int(N) * int(k) * 1024 for k in qk[v]]
        for j, (i, u) in enumerate(zip(ints, units)):
            assert abs(i) < (1 << 53)
            out[v, j] = float(i) * u
            assert fractions.Fraction(float(out[v, j])) == i * fractions.Fraction(float(u)), (v, j)
    return out


def brim_state(res, n_voxels=300, seed=41, epoch=20, brim=BRIM, ordinary=None):
    """→ a state for VoxelMap.restore: n_voxels voxels on sheet_cells, counts 6 … 40 except COUNT_MAX − k at the slots of
    `brim`, exact sums, stamps within the last ten epochs.  ordinary = n: the TWIN of that state — the brim slots hold n
    points and sums that give the mean and (to rounding) the covariance c + I / N the huge voxel has, which takes
    second moments n (q + I / N) − I that are no longer on the lattice.  Extra keys: mk, qk (lattice_moments)."""
    assert res in (0.5, 1.0, 2.0) and n_voxels > max(brim, default=0)
    rng = np.random.default_rng(seed)
    cells = sheet_cells(n_voxels, seed + 1)
    counts = rng.integers(6, 41, size=n_voxels).astype(np.int64)
    mk, qk = lattice_moments(rng, n_voxels)
    stamps = rng.integers(epoch - 9, epoch + 1, size=n_voxels).astype(np.uint32)
    huge = counts.copy()
    for slot, k in brim.items():
        huge[slot] = COUNT_MAX - k
    if ordinary is None:
        counts = huge
    sums = exact_sums(counts, mk, qk, res)
    if ordinary is not None:
        for slot in brim:
            n, N = int(ordinary), int(huge[slot])
            q = qk[slot] / 1024.0
            for j, (a, b) in enumerate(PAIRS):
                sums[slot, 3 + j] = n * q[j] * res * res + ((n / N - 1.0) if a == b else 0.0)
            sums[slot, :3] = n * mk[slot] / 32.0 * res
            counts[slot] = n
    return {"cells": cells, "counts": counts.astype(np.uint32), "sums": sums, "stamps": stamps, "epoch": int(epoch),
            "voxel_resolution": float(res), "search_radius_sq": 1.0, "proper_sqrt_information": True, "mk": mk, "qk": qk}


def lattice_points(rng, cell, n, res):
    """n points of one cell on the 2^-10 lattice, strictly inside it"""
    return (np.asarray(cell, dtype=np.float64) + rng.integers(1, 1024, size=(n, 3)) / 1024.0) * res


def _terms_int(points, cells, res):
    """the nine terms of every point about the corner of its cell, as integers in sum_units"""
    j = points / res * 1024.0 - cells * 1024.0
    assert np.array_equal(j, np.round(j)) and j.min() >= 0 and j.max() < 1024
    j = j.astype(np.int64)
    return np.concatenate([j, np.stack([j[:, a] * j[:, b] for a, b in PAIRS], axis=1)], axis=1)


def apply_batch(state, points):
    """What an insert of `points` (on the lattice; a merge or an add of voxels made of such points is the same batch)
    makes of `state`, in Python integers → a new state (cells, counts, sums, stamps, epoch; the other keys as they
    were): counts and sums added, touched voxels stamped with epoch + 1 (low 32 bits), new cells appended in ascending
    packed cell.  Raises Rejected, with nothing changed, when a voxel would pass COUNT_MAX points."""
    res = state["voxel_resolution"]
    units = sum_units(res)
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    cells = _cells_of(points, res)
    keys = _pack(cells)
    terms = _terms_int(points, cells, res)
    slot = {int(k): s for s, k in enumerate(_pack(state["cells"]))}
    uniq = np.unique(keys)
    over = [int(k) for k in uniq if int(k) in slot and int(state["counts"][slot[int(k)]]) + int((keys == k).sum()) > COUNT_MAX]
    if over:
        raise Rejected(np.nonzero(np.isin(keys, over))[0])
    old = [[int(round(x / u)) for x, u in zip(row, units)] for row in state["sums"]]
    for row, ints in zip(state["sums"], old):
        assert all(float(i) * u == x for i, u, x in zip(ints, units, row))
    out_cells, counts, sums, stamps = [c for c in state["cells"]], [int(c) for c in state["counts"]], old, [int(s) for s in state["stamps"]]
    epoch = int(state["epoch"]) + 1
    for k in uniq:  # ascending packed cell: the order new voxels are appended in
        rows = np.nonzero(keys == k)[0]
        if int(k) not in slot:
            slot[int(k)] = len(counts)
            out_cells.append(cells[rows[0]]), counts.append(0), sums.append([0] * 9), stamps.append(0)
        s = slot[int(k)]
        counts[s] += len(rows)
        sums[s] = [a + int(b) for a, b in zip(sums[s], terms[rows].sum(axis=0))]
        stamps[s] = epoch & (WRAP - 1)
        assert counts[s] <= COUNT_MAX and all(abs(i) < (1 << 53) for i in sums[s])
    out = dict(state)
    out.update(cells=np.array(out_cells, dtype=np.int64).reshape(-1, 3), counts=np.array(counts, dtype=np.uint32),
               sums=np.array([[float(i) * u for i, u in zip(row, units)] for row in sums]).reshape(-1, 9),
               stamps=np.array(stamps, dtype=np.uint32), epoch=epoch)
    return out


def finish_xp(count, sums, cell, res, proper=True):
    """voxel_finish from a count and nine float64 sums about the corner of `cell`, at 50 digits (oracle_voxel_xp's
    statement, which starts from points): mean = corner + s / n, moment = I + Σ d dᵀ, cov = moment / n − m mᵀ, valid iff
    n >= 5 and the largest eigenvalue >= 0.01, eigenvalues floored at 0.01 of the largest, information = Σ u uᵀ / λ
    (= SᵀS; `proper` does not change it, see oracle_voxel_xp.information_from_sqrt) → voxel_stats_xp's dict."""
    del proper
    n = int(count)
    out = {"n": n, "valid": False, "mean": np.zeros(3, dtype=np.longdouble), "eig": np.zeros(3), "eig_floored": np.zeros(3),
           "info": np.eye(3), "gaps": (np.inf, np.inf)}
    with mpmath.workdps(vx.DPS):
        s = [mpmath.mpf(float(x)) for x in sums[:3]]
        M = [mpmath.mpf(float(x)) for x in sums[3:]]
        corner = [mpmath.mpf(int(c)) * mpmath.mpf(float(res)) for c in cell]
        m = [x / n for x in s]
        out["mean"] = np.array([vx._to_ld(corner[k] + m[k]) for k in range(3)], dtype=np.longdouble)
        cov = mpmath.matrix(3, 3)
        for j, (a, b) in enumerate(PAIRS):
            cov[a, b] = cov[b, a] = (M[j] + (1 if a == b else 0)) / n - m[a] * m[b]
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


def finish_errors(ref, mean, S, proper):
    """A valid voxel's mean [3] and sqrt-information [3,3] against finish_xp's dict → (mean error in ulps of the mean's
    largest coordinate — no larger than the largest point coordinate tests/voxel_inputs.py measures in —, floored
    eigenvalues relative, ‖V Vᵀ − I‖, information relative Frobenius, the gap the tie rule may add to it)."""
    ulp = np.spacing(float(np.abs(ref["mean"]).max()))
    mean_err = float(np.abs(np.asarray(mean, dtype=np.longdouble) - ref["mean"]).max() / ulp)
    info, lam, ortho = vx.information_from_sqrt(S, proper)
    eig = float(np.abs(lam / ref["eig_floored"] - 1.0).max())
    return mean_err, eig, ortho, float(np.linalg.norm(info - ref["info"]) / np.linalg.norm(ref["info"])), vx.merged_gap(ref)


def shifted(state, model, E0):
    """→ (state, model) moved E0 inserts into the future: E0 added to the state's epoch and to the model's epoch, stamp,
    birth and history epochs (int64, unmasked), E0 mod 2^32 to the state's uint32 stamps.  The arguments are not modified."""
    E0 = int(E0)
    st = dict(state)
    st["epoch"] = int(state["epoch"]) + E0
    st["stamps"] = ((state["stamps"].astype(np.uint64) + np.uint64(E0 % WRAP)) % np.uint64(WRAP)).astype(np.uint32)
    m = model.clone()
    m.epoch = int(model.epoch) + E0
    m.stamp = model.stamp.astype(np.int64) + E0
    m.birth = model.birth.astype(np.int64) + E0
    m.history = [(epoch + E0, pts, keys) for epoch, pts, keys in model.history]
    return st, m
