"""Scenes for the ray cast through the voxel store (nos_voxel_map_raycast) and the restatement of its
contract.  No tests here, and nothing here needs a GPU.

The ray and the walk are those of the carve and stand on tests/voxel_carve_inputs.py (warp, cell_of, the crossing
parameters from their index): in IEEE double, bit for bit what the device computes.  `cells_visited` walks lazily, as the
kernel does — the next crossing of an axis is formed when the previous one is taken — so that a ray that hits after
twenty cells costs twenty cells; test_voxel_raycast_host.py holds it against voxel_carve_inputs.walk in exact rational
arithmetic.  The hit test is NOT bit-defined (the device may fuse and reorder it): `hit_test` evaluates it in plain
double in the order the header states, `range_xp` evaluates the range of a given voxel and cell at 50 digits, and
`decision_margin` names the rays whose outcome a rounding error could change.

store_of(...) puts voxel statistics (the device's, from VoxelMap.stats(), or numpy_stats' own) into the form cast() reads.

Scenes: voxel_carve_inputs.generic_scene (rays end on the walls or on the box: the analytic range is the length of the
scan point) and the room with four boxes of the place tests."""
import math

import numpy as np

from tests import voxel_carve_inputs as ci

RES = ci.RES
QUERY_SHIFT = 0.3  # metres between a query's pose and the node it should find


# ---------------------------------------------------------------------------------------------------- the contract


def _fma(a, b, c):
    """voxel_carve_inputs.fma; where a factor is 0 or ±1 the product is exact and a * b + c IS rounded once"""
    if a in (0.0, 1.0, -1.0) or b in (0.0, 1.0, -1.0):
        return a * b + c
    return ci.fma(a, b, c)


def warp(R, t, p):
    """voxel_carve_inputs.warp, the same bits; quick for the axis rotations (no rational arithmetic where none is needed)"""
    R = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)]
    x, y, z = (float(v) for v in p)
    return [_fma(R[3 * r + 2], z, _fma(R[3 * r], x, R[3 * r + 1] * y)) + float(t[r]) for r in range(3)]


def ray(R, t, p, res, max_range, origin=(0.0, 0.0, 0.0), a=None):
    """→ None for a skipped ray, else dict a, b, e, w (points), ca, cb (cells), len.  a: warp(origin), if at hand."""
    inv_res = 1.0 / res
    a = warp(R, t, origin) if a is None else a
    e = warp(R, t, p)
    if not all(abs(v) <= 1.79e308 for v in e):  # a NaN fails
        return None
    d = [e[k] - a[k] for k in range(3)]
    len_sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    length = math.sqrt(len_sq) if len_sq >= 0.0 else float("nan")
    if not (length > 0.0):
        return None
    sc = max_range / length
    b = [a[k] + sc * d[k] for k in range(3)]
    ca, cb = ci.cell_of(a, inv_res), ci.cell_of(b, inv_res)
    if ca is None or cb is None:
        return None
    return {"a": a, "b": b, "e": e, "w": [b[k] - a[k] for k in range(3)], "ca": ca, "cb": cb, "len": length}


def _tau(ca, j, up, a, den, res):
    """voxel_carve_inputs.crossing_taus' quotient for one j"""
    g = float(ca + j if up else ca - j + 1) * res
    return (g - a) / den


def cells_visited(r, res):
    """the walk of ray r, lazily → (cell, tau_in, tau_out) for the 1 + n_x + n_y + n_z cells in walk order"""
    a, b, ca, cb = r["a"], r["b"], r["ca"], r["cb"]
    up = [cb[k] >= ca[k] for k in range(3)]
    n = [abs(cb[k] - ca[k]) for k in range(3)]
    den = [b[k] - a[k] for k in range(3)]
    j = [1, 1, 1]
    tau = [_tau(ca[k], 1, up[k], a[k], den[k], res) if n[k] > 0 else 0.0 for k in range(3)]
    c = list(ca)
    tau_in = 0.0
    for it in range(n[0] + n[1] + n[2] + 1):
        k = -1
        for axis in range(3):  # the pending crossing with the smallest tau; equal tau go to x before y before z
            if j[axis] <= n[axis] and (k < 0 or tau[axis] < tau[k]):
                k = axis
        best = tau[k] if k >= 0 else 1.0
        yield tuple(c), tau_in, best
        if k < 0:
            return
        c[k] += 1 if up[k] else -1
        j[k] += 1
        if j[k] <= n[k]:
            tau[k] = _tau(ca[k], j[k], up[k], a[k], den[k], res)
        tau_in = best


def hit_test(r, mean, S, tau_in, tau_out, max_range):
    """the test of one voxel in plain double, in the header's order → (m2, tau_c, range) or None when den is not > 0 or
    tau* is a NaN.  mean [3], S [9] row-major: Python floats."""
    a, w = r["a"], r["w"]
    m = [mean[k] - a[k] for k in range(3)]
    Sw = [S[3 * i] * w[0] + S[3 * i + 1] * w[1] + S[3 * i + 2] * w[2] for i in range(3)]
    Sm = [S[3 * i] * m[0] + S[3 * i + 1] * m[1] + S[3 * i + 2] * m[2] for i in range(3)]
    den = Sw[0] * Sw[0] + Sw[1] * Sw[1] + Sw[2] * Sw[2]
    if not (den > 0.0):
        return None
    tau_star = (Sw[0] * Sm[0] + Sw[1] * Sm[1] + Sw[2] * Sm[2]) / den
    if tau_star != tau_star:
        return None
    tau_c = min(max(tau_star, tau_in), tau_out)
    u = [tau_c * w[k] - m[k] for k in range(3)]
    rr = [S[3 * i] * u[0] + S[3 * i + 1] * u[1] + S[3 * i + 2] * u[2] for i in range(3)]
    return rr[0] * rr[0] + rr[1] * rr[1] + rr[2] * rr[2], tau_c, tau_c * max_range


def store_of(stats):
    """VoxelMap.stats() or numpy_stats() → what cast() reads: slot by cell, and counts, valid, means, S as Python lists"""
    cells = np.asarray(stats["cells"])
    return {"slot": {tuple(int(x) for x in c): v for v, c in enumerate(cells)},
            "counts": [int(x) for x in stats["counts"]], "valid": [bool(x) for x in stats["valid"]],
            "means": np.asarray(stats["means"], dtype=np.float64).reshape(-1, 3).tolist(),
            "S": np.asarray(stats["sqrt_infos"], dtype=np.float64).reshape(-1, 9).tolist()}


def cast(R, t, p, store, res, max_range, min_range=0.0, max_mahalanobis_sq=1.0, min_points=0, origin=(0.0, 0.0, 0.0), a=None):
    """One ray → dict: skipped; voxel (-1: none), range (0.0: none), len; tau_in, tau_out of the hit cell; ray (the dict of
    `ray`, None when skipped); tested: [(voxel, m2, range, tau_in, tau_out)] of every voxel the test was applied to, the
    hit included — what decision_margin reads."""
    r = ray(R, t, p, res, max_range, origin, a)
    out = {"skipped": r is None, "voxel": -1, "range": 0.0, "len": None, "ray": r, "tested": [], "tau_in": None, "tau_out": None}
    if r is None:
        return out
    out["len"] = r["len"]
    slot, counts, valid, means, S = store["slot"], store["counts"], store["valid"], store["means"], store["S"]
    for cell, tau_in, tau_out in cells_visited(r, res):
        v = slot.get(cell)
        if v is None or not valid[v] or counts[v] < min_points:
            continue
        got = hit_test(r, means[v], S[v], tau_in, tau_out, max_range)
        if got is None:
            continue
        m2, _, rng = got
        out["tested"].append((v, m2, rng, tau_in, tau_out))
        if m2 <= max_mahalanobis_sq and rng >= min_range:
            out["voxel"], out["range"], out["tau_in"], out["tau_out"] = v, rng, tau_in, tau_out
            break
    return out


def decision_margin(c, max_mahalanobis_sq=1.0, min_range=0.0):
    """a cast ray whose outcome a rounding error could change: a voxel it tested has |m2 - threshold| < 1e-9 (1 + threshold)
    or |range - min_range| < 1e-9"""
    return any(abs(m2 - max_mahalanobis_sq) < 1e-9 * (1.0 + max_mahalanobis_sq) or abs(rng - min_range) < 1e-9
               for _, m2, rng, _, _ in c["tested"])


def near_tie(r, res, eps=1e-9):
    """voxel_carve_inputs.near_tie over the whole segment a … b of a ray-cast ray (which has no endpoint cell of its own)"""
    return ci.near_tie({"a": r["a"], "b": r["b"], "e": r["b"], "ca": r["ca"], "cb": r["cb"]}, res, eps)


def range_xp(r, mean, S, tau_in, tau_out, max_range):
    """tau_c · max_range at 50 digits from the doubles as given (a, w, mean, S, tau_in, tau_out) → mpmath number"""
    import mpmath
    with mpmath.workdps(50):
        f = mpmath.mpf
        a, w = [f(x) for x in r["a"]], [f(x) for x in r["w"]]
        m = [f(mean[k]) - a[k] for k in range(3)]
        Sx = [f(x) for x in S]
        Sw = [Sx[3 * i] * w[0] + Sx[3 * i + 1] * w[1] + Sx[3 * i + 2] * w[2] for i in range(3)]
        Sm = [Sx[3 * i] * m[0] + Sx[3 * i + 1] * m[1] + Sx[3 * i + 2] * m[2] for i in range(3)]
        tau = (Sw[0] * Sm[0] + Sw[1] * Sm[1] + Sw[2] * Sm[2]) / (Sw[0] * Sw[0] + Sw[1] * Sw[1] + Sw[2] * Sw[2])
        tau = min(max(tau, f(tau_in)), f(tau_out))
        return tau * f(max_range)


def range_error(value, truth):
    """|value - truth| as a float, the difference taken at 50 digits"""
    import mpmath
    with mpmath.workdps(50):
        return float(abs(mpmath.mpf(value) - truth))


# ------------------------------------------------------------------------------------- voxel statistics in numpy


def numpy_stats(points, res=RES, min_points=5, min_eigenvalue=0.01, eig_floor=0.01):
    """The store's statistics of ONE insert of `points` into an empty store, in numpy (voxel_finish.hpp's rules: count >=
    5, covariance (I + Σ d dᵀ) / n − m mᵀ about the cell corner, largest eigenvalue >= 0.01, the others floored at 0.01 of
    it, the proper sqrt-information D^-1/2 Vᵀ) → dict as VoxelMap.stats(): cells (ascending), counts, valid, means,
    sqrt_infos.  The same rules, not the same bits: the host tests' yardstick for what a ray cast of such a map gives."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    c = np.floor(p * (1.0 / res)).astype(np.int64)
    cells, inverse, counts = np.unique(c, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    V = len(cells)
    d = p - c * res
    s1 = np.zeros((V, 3))
    np.add.at(s1, inverse, d)
    s2 = np.zeros((V, 3, 3))
    np.add.at(s2, inverse, d[:, :, None] * d[:, None, :])
    n = counts.astype(np.float64)
    m = s1 / n[:, None]
    cov = (s2 + np.eye(3)) / n[:, None, None] - m[:, :, None] * m[:, None, :]
    w, vec = np.linalg.eigh(cov)  # ascending
    valid = (counts >= min_points) & ~(w[:, 2] < min_eigenvalue)
    w = np.maximum(w, (w[:, 2] * eig_floor)[:, None])
    S = (1.0 / np.sqrt(w))[:, :, None] * np.transpose(vec, (0, 2, 1))  # row i = v_i / sqrt(w_i)
    means = cells * res + m
    S[~valid] = np.eye(3)
    means[~valid] = 0.0
    return {"cells": cells, "counts": counts.astype(np.uint32), "valid": valid.astype(np.uint8), "means": means,
            "sqrt_infos": S.reshape(V, 9)}


# (origin, point, max_range): all on the 2^-10 lattice, in the rays' frame.  Where len is rational and max_range / len a
# power of two, b is exact and the crossings of different axes tie exactly; on the main diagonal a, d and therefore b are
# the same number on all three axes, so every corner is a three-way tie whatever sqrt(3) rounds to.
EXACT_RAYS = [
    ((-1.25, -1.25, -1.25), (1.25, 1.25, 1.25), 4.0),
    ((1.25, 1.25, 1.25), (-1.25, -1.25, -1.25), 4.0),
    ((-1.25, -1.25, -0.875), (-0.25, -0.25, -0.375), 3.0),    # d = (2, 2, 1) / 2, len 1.5, sc = 2: x and y tie
    ((1.25, 1.0, -1.125), (0.5, 0.0, -1.125), 2.5),           # d = -(3, 4, 0) / 4, len 1.25, sc = 2
    ((0.25, 0.25, 0.25), (1.0, 0.25, 0.25), 1.5),             # along x, b on a cell face
    ((0.25, 0.25, 0.25), (-1.0, 0.25, 0.25), 1.25),           # the same going down
    ((0.25, 0.5, 0.25), (1.25, 0.5, 0.75), 1.0),              # in a face plane, no motion across it
    ((0.125, 0.125, 0.125), (0.375, 0.25, 0.125), 0.125),     # start and end in one cell
    ((-1.25, -1.0, -0.875), (-0.75, 0.0, 0.125), 3.0),        # d = (1, 2, 2) / 2, len 1.5, sc = 2: skew, off the corners
]


def exact_pose(k):
    """the k-th axis rotation of voxel_carve_inputs and a lattice translation: exact warps of lattice points"""
    return ci.axis_rotation(k), np.array([0.0, 0.0, 0.0]) if k == 0 else np.array([0.5, -0.5, 1.0]) * (1 if k == 1 else -1)


def exact_block_points(thin=()):
    """voxel_carve_inputs.block_cells with EIGHT lattice points per cell, a quarter and three quarters of an edge from the
    corner on every axis: count 8, the mean is the cell's centre and the covariance (1/8 + 1/64) I, both exactly — valid
    voxels with S = I / 0.375.  The cells in `thin` get only four of them (the lower z): fewer than 5 points, not valid."""
    cells, _ = ci.block_cells()
    off = np.array([(x, y, z) for z in (0.125, 0.375) for x in (0.125, 0.375) for y in (0.125, 0.375)])
    thin = {tuple(c) for c in thin}
    parts = [c * RES + (off[:4] if tuple(int(v) for v in c) in thin else off) for c in cells]
    return cells, np.concatenate(parts)


# ------------------------------------------------------------------------------------------------------ the scenes

BOXES = (((2.61, -0.12), (1.0, 1.0, 2.0)), ((-6.3, 3.1), (2.5, 1.2, 3.5)), ((5.2, -6.4), (1.5, 3.0, 1.2)),
         ((-3.4, -5.1), (0.8, 0.8, 5.0)))  # (x, y of the low corner), (size): they stand on the floor
NODE_HEIGHT = 1.7
QUERIES = ((7, 0.7), (2, -2.1), (13, 3.0), (10, 1.9))  # (node, yaw of the query's sensor)
PLACE = {"n_rings": 20, "n_sectors": 60, "max_range": 25.0, "z_floor": -2.0}
RAY_MAX_RANGE = 30.0


def box_bounds():
    """→ [(lo [3], hi [3])] of the four boxes"""
    out = []
    for (x, y), size in BOXES:
        lo = np.array([x, y, ci.ROOM_LO[2]])
        out.append((lo, lo + np.array(size)))
    return out


def pattern():
    """16 elevations in ±20° × 120 azimuths in the middle of their 3° cells, elevation-major: api.ray_pattern's rule
    (restated, so that the host tests need no package).  No beam lies on a border of the descriptor's 60 sectors."""
    el = np.radians(np.linspace(-20.0, 20.0, 16)).reshape(-1, 1)
    az = (2.0 * np.pi / 120) * (np.arange(120, dtype=np.float64) + 0.5).reshape(1, -1)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1)
    return np.ascontiguousarray(d.reshape(-1, 3))


def node_positions():
    """20 nodes, x-major: x ∈ {−8 … 8 step 4}, y ∈ {−6 … 6 step 4}, NODE_HEIGHT above the floor"""
    z = float(ci.ROOM_LO[2]) + NODE_HEIGHT
    return np.array([(x, y, z) for x in (-8.0, -4.0, 0.0, 4.0, 8.0) for y in (-6.0, -2.0, 2.0, 6.0)])


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def analytic_ranges(o, d):
    """distance from the point o inside the room (outside the boxes) along unit directions d [n, 3] to the first surface"""
    rng = ci._exit_distance(o, d, ci.ROOM_LO, ci.ROOM_HI)
    for lo, hi in box_bounds():
        rng = np.minimum(rng, ci._entry_distance(o, d, lo, hi))
    return rng


def place_scene(n_wall=300_000, n_box=12_000, seed=11):
    """→ dict: points (map frame: walls, then the boxes' faces), pattern, nodes [20, 3], queries: [(node, R, t, scan
    points in the query sensor's frame)] — analytic scans with 1 cm range noise, taken QUERY_SHIFT from their nodes"""
    rng = np.random.default_rng(seed)
    parts = [ci._on_faces(ci.ROOM_LO, ci.ROOM_HI, n_wall, rng)]
    for lo, hi in box_bounds():
        parts.append(ci._on_faces(lo, hi, n_box, rng))
    pat, nodes = pattern(), node_positions()
    queries = []
    for node, yaw in QUERIES:
        R = rot_z(yaw)
        t = nodes[node] + QUERY_SHIFT * np.array([0.6, 0.8, 0.0])
        d = pat @ R.T
        r = analytic_ranges(t, d) + 0.01 * rng.normal(size=len(pat))
        queries.append((node, R, t, np.ascontiguousarray(pat * r[:, None])))
    return {"points": np.concatenate(parts), "pattern": pat, "nodes": nodes, "queries": queries}


def render(store, R, t, pat, res=RES, max_range=RAY_MAX_RANGE, **kw):
    """the restatement's view from the pose (R, t) along `pat` → (hit points in the sensor frame [n_hit, 3], ranges [n],
    voxels [n], the number of rays at a decision margin): a hit point is range / len times the beam's point, the origin
    being 0"""
    a = warp(R, t, (0.0, 0.0, 0.0))
    pts, ranges, voxels, unsure = [], np.zeros(len(pat)), np.full(len(pat), -1, dtype=np.int64), 0
    for i, p in enumerate(pat):
        c = cast(R, t, p, store, res, max_range, a=a, **kw)
        ranges[i], voxels[i] = c["range"], c["voxel"]
        unsure += int(decision_margin(c, kw.get("max_mahalanobis_sq", 1.0), kw.get("min_range", 0.0)))
        if c["voxel"] >= 0:
            q = c["range"] / c["len"]
            pts.append([0.0 + q * (float(p[k]) - 0.0) for k in range(3)])
    return np.array(pts, dtype=np.float64).reshape(-1, 3), ranges, voxels, unsure
