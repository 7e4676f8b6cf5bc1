"""Scenes for the line-of-sight carve (nos_voxel_map_carve) and the restatement of its contract.

The restatement follows include/nos.h operation by operation in IEEE double: Python floats ARE doubles, math.sqrt and
`/` are correctly rounded, and the one fused operation of the contract, the warp's multiply-add, is formed exactly with
fractions.Fraction and rounded once.  On exact inputs it therefore gives the device's bits; on general inputs a ray can
differ only where two crossing parameters, or a coordinate and a cell face, are closer than a rounding error — the
near-ties `near_tie` finds.

The generic scene: a 20 x 16 x 6 m room (walls off the cell faces), a 1 x 1 x 2 m box in the middle, the sensor at
(1.3, -0.7, 0.4) inside it, under a general pose; resolution 0.5."""
import math
from fractions import Fraction

import numpy as np

RES = 0.5
LIMIT = 1 << 20
SENSOR = np.array([1.3, -0.7, 0.4])
ROOM_LO = np.array([-9.87, -8.21, -1.63])
ROOM_HI = ROOM_LO + np.array([20.0, 16.0, 6.0])
BOX_LO = np.array([2.61, -0.12, -0.63])
BOX_HI = BOX_LO + np.array([1.0, 1.0, 2.0])


# ---------------------------------------------------------------------------------------------------- the contract


def fma(a, b, c):
    """a * b + c rounded once"""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def warp(R, t, p):
    """R p + t with the multiply-adds of the matcher's warp (voxel_points_kernel<true>)"""
    R = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)]
    x, y, z = (float(v) for v in p)
    return [fma(R[3 * r + 2], z, fma(R[3 * r], x, R[3 * r + 1] * y)) + float(t[r]) for r in range(3)]


def cell_of(v, inv_res):
    """floor(v inv_res) per axis, or None when a cell lies outside the addressable grid"""
    out = []
    for k in range(3):
        f = v[k] * inv_res
        if not (f == f) or math.isinf(f):
            return None
        f = math.floor(f)
        if not (-LIMIT <= f < LIMIT):
            return None
        out.append(int(f))
    return out


def ray(R, t, p, res, end_margin, min_range, max_range, origin=(0.0, 0.0, 0.0)):
    """→ None for a skipped ray, else dict a, b, e (points), ca, cb, ce (cells)"""
    inv_res = 1.0 / res
    a, e = warp(R, t, origin), warp(R, t, p)
    if not all(abs(v) <= 1.79e308 for v in e):  # a NaN fails
        return None
    d = [e[k] - a[k] for k in range(3)]
    len_sq = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    length = math.sqrt(len_sq) if len_sq >= 0.0 else float("nan")
    if not (length > min_range) or not (length > end_margin):
        return None
    s = (length - end_margin) / length if length <= max_range else max_range / length
    b = [a[k] + s * d[k] for k in range(3)]
    ca, cb, ce = cell_of(a, inv_res), cell_of(b, inv_res), cell_of(e, inv_res)
    if ca is None or cb is None or ce is None:
        return None
    return {"a": a, "b": b, "e": e, "ca": ca, "cb": cb, "ce": ce}


def crossing_taus(a, b, ca, cb, res, number=float):
    """per axis the list of tau_j, j = 1 … n_k, each from j; number=Fraction: the same quotients, exact"""
    taus = []
    for k in range(3):
        n = abs(cb[k] - ca[k])
        up = cb[k] >= ca[k]
        row = []
        if n > 0:
            den = number(b[k]) - number(a[k])
            for j in range(1, n + 1):
                g = number(float(ca[k] + j if up else ca[k] - j + 1)) * number(res)
                row.append((g - number(a[k])) / den)
        taus.append(row)
    return taus


def walk(a, b, ca, cb, res, number=float):
    """→ the visited cells in order, 1 + n_x + n_y + n_z of them: the pending crossing with the smallest tau steps its
    axis, equal tau go to x before y before z"""
    taus = crossing_taus(a, b, ca, cb, res, number)
    c, j = list(ca), [0, 0, 0]
    cells = [tuple(c)]
    for _ in range(sum(len(r) for r in taus)):
        k = -1
        for axis in range(3):
            if j[axis] < len(taus[axis]) and (k < 0 or taus[axis][j[axis]] < taus[k][j[k]]):
                k = axis
        c[k] += 1 if cb[k] >= ca[k] else -1
        j[k] += 1
        cells.append(tuple(c))
    return cells


def near_tie(r, res, eps=1e-9):
    """a ray whose walk a rounding error could change: two tau of different axes closer than eps, or a coordinate of
    a inv_res, b inv_res (or e inv_res, for the hit) within eps of an integer"""
    inv_res = 1.0 / res
    for v in (r["a"], r["b"], r["e"]):
        for k in range(3):
            f = v[k] * inv_res
            if abs(f - round(f)) < eps:
                return True
    taus = crossing_taus(r["a"], r["b"], r["ca"], r["cb"], res)
    tagged = sorted((tau, k) for k in range(3) for tau in taus[k])
    return any(t1 - t0 < eps and k0 != k1 for (t0, k0), (t1, k1) in zip(tagged, tagged[1:]))


def counts(cells, R, t, points, res, end_margin, min_range=0.0, max_range=None, origin=(0.0, 0.0, 0.0)):
    """The counters of a carve of a store whose voxels are `cells` ([V][3], voxel-id order) by the scan `points` →
    (crossings [V], hits [V], skipped, the per-ray dicts or None)"""
    max_range = 1024.0 * res if max_range is None else max_range
    slot = {tuple(int(x) for x in c): v for v, c in enumerate(np.asarray(cells))}
    crossings, hits = np.zeros(len(slot), dtype=np.uint32), np.zeros(len(slot), dtype=np.uint32)
    skipped, rays = 0, []
    for p in np.asarray(points, dtype=np.float64).reshape(-1, 3):
        r = ray(R, t, p, res, end_margin, min_range, max_range, origin)
        rays.append(r)
        if r is None:
            skipped += 1
            continue
        v = slot.get(tuple(r["ce"]))
        if v is not None:
            hits[v] += 1
        for c in walk(r["a"], r["b"], r["ca"], r["cb"], res):
            v = slot.get(c)
            if v is not None:
                crossings[v] += 1
    return crossings, hits, skipped, rays


def removed(crossings, hits, min_crossings, min_hits):
    """the rule: a voxel goes iff crossings >= min_crossings and hits < min_hits → bool [V]"""
    return (crossings >= min_crossings) & (hits < min_hits)


# ------------------------------------------------------------------------------------------------------ the scenes


def general_pose():
    """→ (R, t): a general rotation (no axis alignment) and the sensor's place in the map"""
    ax, ay, az = 0.31, -0.22, 0.83
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx, SENSOR.copy()


def _on_faces(lo, hi, n, rng):
    """n random points on the six faces of the box lo … hi, by area"""
    ext = hi - lo
    areas = np.array([ext[1] * ext[2], ext[1] * ext[2], ext[0] * ext[2], ext[0] * ext[2], ext[0] * ext[1], ext[0] * ext[1]])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    pts = lo + rng.uniform(size=(n, 3)) * ext
    axis, side = face // 2, face % 2
    pts[np.arange(n), axis] = np.where(side == 0, lo[axis], hi[axis])
    return pts


def _exit_distance(o, d, lo, hi):
    """distance along unit directions d [n,3] from the inside point o to the faces of lo … hi"""
    with np.errstate(divide="ignore", invalid="ignore"):
        tt = np.where(d > 0, (hi - o) / d, np.where(d < 0, (lo - o) / d, np.inf))
    return tt.min(axis=1)


def _entry_distance(o, d, lo, hi):
    """distance to the box lo … hi from the outside point o, inf for a miss"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near, far = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
    return np.where((near <= far) & (near > 0), near, np.inf)


def generic_scene(n_wall=40000, n_box=2500, n_rays=4000, seed=7):
    """→ dict: wall_points, box_points (map frame), R, t, scan_free (rays to the walls, box gone) and scan_box (rays stop
    at the box), both in the scan's frame, box_cells (set of the cells that hold a box point)"""
    rng = np.random.default_rng(seed)
    walls = _on_faces(ROOM_LO, ROOM_HI, n_wall, rng)
    box = BOX_LO + rng.uniform(size=(n_box, 3)) * (BOX_HI - BOX_LO)
    R, t = general_pose()
    d = rng.normal(size=(n_rays, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    to_wall = _exit_distance(SENSOR, d, ROOM_LO, ROOM_HI)
    to_box = _entry_distance(SENSOR, d, BOX_LO, BOX_HI)
    ends_free = SENSOR + to_wall[:, None] * d
    ends_box = SENSOR + np.minimum(to_wall, to_box)[:, None] * d
    local = lambda ends: np.ascontiguousarray((ends - t) @ R)  # noqa: E731  Rᵀ (e - t), rounded: a general scan
    box_cells = {tuple(int(x) for x in c) for c in np.floor(box / RES).astype(np.int64)}
    return {"wall_points": walls, "box_points": box, "R": R, "t": t, "scan_free": local(ends_free), "scan_box": local(ends_box),
            "box_cells": box_cells, "n_box_rays": int(np.sum(to_box < to_wall))}


def cells_of_points(points, res=RES):
    """the cells an insert of `points` creates, in voxel-id order for ONE batch into an empty store: ascending cell"""
    c = np.unique(np.floor(np.asarray(points) / res).astype(np.int64), axis=0)
    return c  # np.unique sorts rows lexicographically: x, then y, then z — the packed key's order


def block_cells(side=6, lo=-3):
    """every cell of a side³ block from `lo` on each axis, and one point in the middle of each (exact at RES = 0.5)"""
    rng = range(lo, lo + side)
    cells = np.array([(x, y, z) for x in rng for y in rng for z in rng], dtype=np.int64)
    return cells, (cells + 0.5) * RES


def axis_rotation(k):
    """rotation by 90° about z (k = 1), about x (k = 2); the identity (k = 0): exact warps of lattice points"""
    return [np.eye(3), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
            np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])][k]
