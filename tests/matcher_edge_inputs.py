"""Inputs that put the scan matcher's decisions within rounding, and their reference (no tests here: test_matcher_edges.py
on the CPU, test_matcher_edges_gpu.py on the device).

ISLANDS.  An island is one query point and one to four voxel means, each of which differs from the query in ONE coordinate
only; the other two coordinates are bit-identical.  Then match_dist(ex, ey, ez) = fma(ez, ez, fma(ey, ey, ex ex)) has two
zero arguments and is fl(e e) with e = fl(q - m) whichever product is fused, and warp_point under the identity pose returns
the point's bits (1 x + 0 y + 0 z + 0).  So a numpy brute force has the device's bits: no tolerance anywhere.  Islands sit
at least 8 cells apart in the two other coordinates (64 radius_sq between a query and a foreign mean), and every query is
evaluated against ALL valid voxels of its map.

Families, each built along x, y and z (the dense lookup reads its three z cells as one run):
  face    q = step(fl((k+1) c), a), m = step(fl((k+2) c), b), c = sqrt(radius_sq), a, b in -6..6 ulps, and the mirrored pair
          (the lower value the mean); a zero or subnormal query is replaced by +-1e-200
  radius  m = step(q +- c, a): fl(e e) on both sides of radius_sq, and radius_sq itself for 1.0, 0.25 and 2.25 (no match:
          the test is strict)
  tie     means at +d and -d with the ids in both orders; three equidistant means (the third along another axis); a nearer
          voxel with valid = 0
  limits  the same families in cells +-(2^20 - 6..3); a query 2^21 cells from an occupied cell (pack_cell folds it onto that
          cell's key); queries of +-1e300, +-inf and NaN in one coordinate

One map per (radius_sq, region): the regions near the origin and around cells 1000, 4097 and -123457 are small enough in
cells for the dense lookup form, the two limit regions as well.

REFERENCE.  brute_force: every (query, valid voxel) pair by a distance good to 1e-6 (coordinates taken about the map's
centre, where the map is a few hundred cells wide), then every pair below 1.5 radius_sq exactly: fl(fl(q - m)^2) of the one
coordinate that differs (asserted), strict <, sorted by (distance, original id).
"""
import functools
import math

import numpy as np

RADII = (1.0, 0.25, 2.25, 2.0, 0.09, 0.3, 1.5, 3.0, 10.0)
EXACT_RADII = (1.0, 0.25, 2.25)  # sqrt exact: fl(e e) hits radius_sq itself
LIMIT = 1 << 20
REGIONS = {
    "origin-": (-3, -2, -1),  # the cells around the origin, in two maps so that each stays small enough for the dense form
    "origin+": (0, 1, 2),
    "k1000": (1000,),
    "k4097": (4097,),
    "k-123457": (-123457,),
    "limit+": tuple(range(LIMIT - 8, LIMIT - 4)),   # face means in cells 2^20 - 6 .. 2^20 - 3
    "limit-": tuple(range(-LIMIT + 3, -LIMIT + 7)),  # the lowest cell touched is -(2^20 - 3)
}
ULPS = tuple(range(-6, 7))
SPACING = 8          # cells between islands in the two other coordinates
MIN_NORMAL = 2.2250738585072014e-308


def step(x, n):
    """x moved by n ulps"""
    x = np.float64(x)
    for _ in range(abs(n)):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return float(x)


def _steps(x):
    return {a: step(x, a) for a in ULPS}


def _query_value(q, a):
    """a zero or subnormal query coordinate → +-1e-200"""
    if abs(q) < MIN_NORMAL:
        return -1e-200 if a < 0 else 1e-200
    return q


def dist_sq_1d(q, m):
    """fl(fl(q - m)^2): match_dist when the two other differences are zero"""
    e = np.float64(q) - np.float64(m)
    return float(e * e)


def sqrt_info_of(ids):
    """An upper-triangular integer S that names its voxel and is exact in fp32: S00 = 1 + id % 4096, S01 = id // 4096,
    S11 = S22 = 1 (its triangular factor U of S = QU is S itself)."""
    ids = np.asarray(ids, dtype=np.int64)
    S = np.zeros((ids.size, 9))
    S[:, 0] = 1 + ids % 4096
    S[:, 1] = ids // 4096
    S[:, 4] = S[:, 8] = 1.0
    return S


def id_of_sqrt_info(s00, s01):
    return (np.asarray(s00) - 1).astype(np.int64) + 4096 * np.asarray(s01).astype(np.int64)


class _Builder:
    """Collects islands: queries, means (a mean's original id is its row), valid flags, the family of every query and what
    the island was constructed to give (expected[i] = the ids of its up to two matches, nearest first)."""

    def __init__(self, r2, ks):
        self.r2, self.c = r2, math.sqrt(r2)
        self.base = ks[0]
        self.toward = -1 if self.base >= 1000 else 1  # the island grid grows towards the origin from a far region
        self.q, self.m, self.valid, self.family, self.expected, self.axis = [], [], [], [], [], []
        self.first_mean, self.n_means = [], []
        self.n_islands = [0, 0, 0]
        self.side = 1

    def reserve(self, n_per_axis):
        self.side = max(1, int(math.ceil(math.sqrt(n_per_axis))))

    def _others(self, axis):
        """the two other coordinates of the next island along `axis`: mid-cell, 16 cells and more from the region's base"""
        g = self.n_islands[axis]
        self.n_islands[axis] += 1
        assert g < self.side * self.side
        cell = [self.base + self.toward * (16 + SPACING * (g // self.side)), self.base + self.toward * (16 + SPACING * (g % self.side))]
        return [_on_lattice((cu + 0.5) * self.c) for cu in cell]

    def island(self, family, axis, q, means, second_axis=None):
        """means: list of (coordinate along `axis`, valid) — or ((coordinate, True), on second_axis) through `second_axis`:
        the LAST mean then differs from the query along second_axis instead (by the same amount as the first)"""
        u, v = self._others(axis)
        other = [k for k in range(3) if k != axis]
        point = [0.0, 0.0, 0.0]
        point[axis], point[other[0]], point[other[1]] = q, u, v
        first_id = len(self.m)
        cand = []
        for j, (x, ok) in enumerate(means):
            mean = list(point)
            if second_axis is not None and j == len(means) - 1:
                mean[second_axis] = point[second_axis] + (x - q)
                d = dist_sq_1d(point[second_axis], mean[second_axis])
            else:
                mean[axis] = x
                d = dist_sq_1d(q, x)
            self.m.append(mean)
            self.valid.append(bool(ok))
            if ok and d < self.r2:  # strict
                cand.append((d, first_id + j))
        cand.sort()
        self.first_mean.append(first_id)
        self.n_means.append(len(means))
        self.q.append(point)
        self.family.append(family)
        self.axis.append(axis)
        self.expected.append([i for _, i in cand[:2]])

    def lone_query(self, family, point):
        self.q.append(list(point))
        self.family.append(family)
        self.axis.append(-1)
        self.expected.append([])
        self.first_mean.append(0)
        self.n_means.append(0)


def _on_lattice(x):
    """x rounded to a multiple of 2^-24 (exact for |x| < 2^28)"""
    return round(x * 2.0 ** 24) / 2.0 ** 24


def _tie_values(q, c):
    """q on a 2^-24 lattice and d a power of two near c / 4: q + d and q - d are exact for |q| < 2^22"""
    q = _on_lattice(q)
    d = 2.0 ** math.floor(math.log2(c / 4.0))
    assert (q + d) - q == d and q - (q - d) == d
    return q, d


@functools.lru_cache(maxsize=None)
def snapshot_case(r2, region):
    """→ dict: queries [n][3], means [V][3], sqrt_infos [V][9], valid [V], family [n] (str), axis [n], expected [n][2]
    (original ids by construction, -1 = none), first_mean / n_means [n] (the island's means are rows first_mean ..
    first_mean + n_means - 1)."""
    ks = REGIONS[region]
    b = _Builder(r2, ks)
    c = b.c
    per_k = 2 * len(ULPS) ** 2 + 2 * len(ULPS) + 5
    b.reserve(per_k * len(ks) + 4)
    for k in ks:
        lo, hi = _steps((k + 1) * c), _steps((k + 2) * c)
        mid = (k + 0.5) * c
        for axis in range(3):
            # face: the query just below / above the face between cells k and k+1, the mean around the next face
            for a in ULPS:
                for bb in ULPS:
                    b.island("face", axis, _query_value(lo[a], a), [(hi[bb], True)])
                    b.island("face", axis, _query_value(hi[bb], bb), [(lo[a], True)])  # mirrored: the mean below the query
            # radius: fl(e e) around radius_sq (mid is exact in c for the exact radii, so a = 0 hits it)
            for sign in (1.0, -1.0):
                for a in ULPS:
                    b.island("radius", axis, mid, [(step(mid + sign * c, a), True)])
            # ties
            q, d = _tie_values(mid, c)
            b.island("tie", axis, q, [(q + d, True), (q - d, True)])
            b.island("tie", axis, q, [(q - d, True), (q + d, True)])
            b.island("tie", axis, q, [(q + d, True), (q - d, True), (q + d, True)], second_axis=(axis + 1) % 3)
            b.island("tie", axis, q, [(q - d, True), (q + d, True), (q - d, True)], second_axis=(axis + 2) % 3)
            b.island("tie", axis, q, [(q + d / 2, False), (q + d, True), (q - d, True)])
    # limits: queries folded onto an occupied cell's key, and queries no cell can hold
    home = b.q[b.family.index("tie")]  # mid-cell in all three coordinates; its cell holds the island's means at +-d
    for axis in range(3):
        for sign in (1.0, -1.0):
            far = list(home)
            far[axis] = home[axis] + sign * float(1 << 21) * c
            b.lone_query("fold", far)
        for value in (1e300, -1e300, np.inf, -np.inf, np.nan):
            odd = list(b.q[0])
            odd[axis] = value
            b.lone_query("nonfinite", odd)
    n = len(b.q)
    expected = -np.ones((n, 2), dtype=np.int64)
    for i, ids in enumerate(b.expected):
        expected[i, :len(ids)] = ids
    means = np.array(b.m, dtype=np.float64)
    return {"r2": r2, "region": region, "queries": np.array(b.q, dtype=np.float64), "means": means,
            "sqrt_infos": sqrt_info_of(np.arange(len(means))), "valid": np.array(b.valid, dtype=bool),
            "family": np.array(b.family), "axis": np.array(b.axis), "expected": expected,
            "first_mean": np.array(b.first_mean), "n_means": np.array(b.n_means)}


@functools.lru_cache(maxsize=None)
def snapshot_reference(r2, region):
    """→ idx [n][2] of brute_force on snapshot_case(r2, region): computed once, shared, not to be written to"""
    case = snapshot_case(r2, region)
    idx, _ = brute_force(case["queries"], case["means"], case["valid"], r2)
    idx.setflags(write=False)
    return idx


def radius_sides(case):
    """→ how many radius islands have fl(e e) below, above and equal to radius_sq"""
    rows = np.nonzero(case["family"] == "radius")[0]
    q = case["queries"][rows, case["axis"][rows]]
    m = case["means"][case["first_mean"][rows], case["axis"][rows]]
    e = q - m
    d = e * e
    return {"below": int((d < case["r2"]).sum()), "above": int((d > case["r2"]).sum()), "equal": int((d == case["r2"]).sum())}


def nearer_invalid(case):
    """→ the number of islands with matches in both slots and an invalid mean nearer than the first of them"""
    n = 0
    for i in np.nonzero((case["n_means"] > 0) & (case["expected"][:, 1] >= 0))[0]:
        rows = np.arange(case["first_mean"][i], case["first_mean"][i] + case["n_means"][i])
        e = case["queries"][i][None, :] - case["means"][rows]
        d = (e * e).sum(axis=1)
        first = d[case["expected"][i, 0] - rows[0]]
        n += int(((d < first) & ~case["valid"][rows]).any())
    return n


def left_out(queries, means, valid, r2):
    """→ mask [n] of the queries a bit-for-bit comparison has to leave out: those with a candidate (a valid mean below 1.5
    radius_sq) that differs from the query in more than one coordinate — match_dist then rounds more than once, in an
    order the brute force above does not restate.  The islands are built so that there is none."""
    ids = np.nonzero(valid)[0]
    out = np.zeros(len(queries), dtype=bool)
    if ids.size == 0:
        return out
    m = means[ids]
    centre = 0.5 * (m.min(axis=0) + m.max(axis=0))
    mc = m - centre
    mm = np.einsum("ij,ij->i", mc, mc)
    finite = np.isfinite(queries).all(axis=1) & (np.abs(queries) < 1e100).all(axis=1)
    for a in range(0, len(queries), 1024):
        rows = np.arange(a, min(a + 1024, len(queries)))
        ok = finite[rows]
        qc = np.where(ok[:, None], queries[rows] - centre, 0.0)
        approx = np.einsum("ij,ij->i", qc, qc)[:, None] + mm[None, :] - 2.0 * (qc @ mc.T)
        approx[~ok] = np.inf
        qi, mi = np.nonzero(approx < 1.5 * r2)
        many = ((queries[rows][qi] - m[mi]) != 0.0).sum(axis=1) > 1
        out[rows[qi[many]]] = True
    return out


def brute_force(queries, means, valid, r2, take=2):
    """→ (idx [n][take] original ids of the nearest valid means with fl(fl(q - m)^2) < r2 by (distance, id), -1 = none;
    d2 [n][take], inf-padded).  All pairs; the candidates must be single-coordinate pairs (asserted), see the module's text."""
    n = len(queries)
    idx = -np.ones((n, take), dtype=np.int64)
    d2 = np.full((n, take), np.inf)
    ids = np.nonzero(valid)[0]
    if ids.size == 0 or n == 0:
        return idx, d2
    m = means[ids]
    finite = np.isfinite(queries).all(axis=1) & (np.abs(queries) < 1e100).all(axis=1)
    centre = 0.5 * (m.min(axis=0) + m.max(axis=0))
    mc = m - centre
    mm = np.einsum("ij,ij->i", mc, mc)
    with np.errstate(all="ignore"):
        for a in range(0, n, 1024):
            rows = np.arange(a, min(a + 1024, n))
            q = queries[rows]
            ok = finite[rows]
            qc = np.where(ok[:, None], q - centre, 0.0)
            approx = np.einsum("ij,ij->i", qc, qc)[:, None] + mm[None, :] - 2.0 * (qc @ mc.T)
            approx[~ok] = np.inf
            qi, mi = np.nonzero(approx < 1.5 * r2)
            # a query that is not finite (or beyond 1e100): every pair exactly — nothing is below the radius
            for r in np.nonzero(~ok)[0]:
                e = q[r][None, :] - m
                assert not ((e * e).sum(axis=1) < r2).any()
            e = q[qi] - m[mi]
            differs = e != 0.0
            assert (differs.sum(axis=1) <= 1).all(), "a candidate pair differs in more than one coordinate"
            d = (e * e).sum(axis=1)  # two exact zeros and one product: fl(e e)
            for r in np.unique(qi):
                sel = qi == r
                cand = sorted((dd, int(ids[j])) for dd, j in zip(d[sel], mi[sel]) if dd < r2)
                for s, (dd, j) in enumerate(cand[:take]):
                    idx[rows[r], s], d2[rows[r], s] = j, dd
    return idx, d2


def expected_planes(queries, means, sqrt_infos, idx, k):
    """→ (the 15 planes [15][2 n] of NdtMap.match at the identity pose for matches idx[:, :k], the match count)"""
    n = len(queries)
    want = np.zeros((15, 2 * n))
    for s in range(k):
        hit = idx[:, s] >= 0
        cols = 2 * np.nonzero(hit)[0] + s
        j = idx[hit, s]
        want[0:3, cols] = queries[hit].T
        want[3:6, cols] = means[j].T
        want[6:15, cols] = sqrt_infos[j].T
    return want, int((idx[:, :k] >= 0).sum())


def parent_cell_rule_misses(case, widen=1.0):
    """The cell rule as it stood: cell = floor(x (1 / sqrt(radius_sq))), a query looks at the 27 cells around its own.
    → the number of constructed matches (query, mean) whose cells lie two or more apart on an axis, i.e. that this search
    cannot see.  widen: the factor on the cell edge."""
    inv = 1.0 / (math.sqrt(case["r2"]) * widen)
    q, m, exp = case["queries"], case["means"], case["expected"]
    missed = 0
    with np.errstate(all="ignore"):
        for s in range(2):
            hit = exp[:, s] >= 0
            cq = np.floor(q[hit] * inv)
            cm = np.floor(m[exp[hit, s]] * inv)
            missed += int((np.abs(cq - cm) >= 2).any(axis=1).sum())
    return missed


# ---------------------------------------------------------------------------------------------- the live voxel store

LIVE_CONFIGS = ((1.0, 1.0), (0.3, 1.0), (1.0, 0.3), (0.5, 3.0))  # (voxel resolution, radius_sq)
LIVE_SPACING = 12     # cells between clusters: more than sqrt(1.5 radius_sq) at every configuration
LIVE_SPREAD = 2.0 ** -6
SINGLE, LOWER, UPPER, THIRD, NEARER = range(5)  # a voxel's role in its cluster


def voxel_points(mu, spread):
    """eight points mu + (+-sx, +-sy, +-sz): count 8, every sum exact, mean = mu exactly"""
    s = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)
    return np.asarray(mu, dtype=np.float64) + s * np.asarray(spread, dtype=np.float64)


def _lattice10(x):
    return np.round(np.asarray(x, dtype=np.float64) * 1024.0) / 1024.0


@functools.lru_cache(maxsize=None)
def live_layout(res, shifted):
    """A store of about 200 exact voxels (voxel_points on a 2^-10 lattice, so a mean is its mu) in clusters LIVE_SPACING
    cells apart: 96 single voxels, and 36 tie clusters around a point p at fraction 0.9 of its cell on every axis — a voxel
    at p - d and one at p + d along the cluster's axis (d = the largest power of two <= res / 2: different cells), in a
    third of them a voxel at p + d along the next axis, in another third also an INVALID voxel at p + d / 2 along the third
    axis (128 points: the largest eigenvalue 1 / 128 + spread^2 is below the 0.01 a valid voxel needs).  Half the clusters
    put their upper voxels into the first batch, so the lower slot is now the lower, now the upper mean.  shifted: half the
    clusters reach cell +(2^20 - 16), half cell -(2^20 - 16).
    → dict: batches (two point arrays), mu [V][3], cell [V][3], role [V], cluster [V], axis [n_clusters], centre [n_clusters][3]"""
    d = 2.0 ** math.floor(math.log2(res / 2.0))
    mu, role, cluster, batch, axis_of, centre = [], [], [], [], [], []
    n_clusters = 96 + 36
    for g in range(n_clusters):
        gx, gy = LIVE_SPACING * (g % 12), LIVE_SPACING * (g // 12)
        if not shifted:
            corner = np.array([-60 + gx, -70 + gy, -2 + (g % 3)])
        elif g % 2 == 0:
            corner = np.array([LIMIT - 17 - gx, LIMIT - 17 - gy, LIMIT - 17 - (g % 3)])   # the cluster's upper cells: 2^20 - 16
        else:
            corner = np.array([-(LIMIT - 16) + gx, -(LIMIT - 16) + gy, -(LIMIT - 16) + (g % 3)])
        axis = g % 3
        axis_of.append(axis)
        if g < 96:
            p = _lattice10((corner + np.array([0.5, 0.3, 0.7])) * res)
            members = [(SINGLE, p, 1)]
        else:
            kind = (g - 96) // 3 % 3  # pair, triple, triple with a nearer invalid voxel
            upper_first = (g - 96) // 9 % 2
            p = _lattice10((corner + 0.9) * res)
            e = np.eye(3)
            members = [(LOWER, p - d * e[axis], 1 - upper_first), (UPPER, p + d * e[axis], upper_first)]
            if kind >= 1:
                members.append((THIRD, p + d * e[(axis + 1) % 3], upper_first))
            if kind == 2:
                members.append((NEARER, p + 0.5 * d * e[(axis + 2) % 3], 1))
        centre.append(p)
        for r, m, b in members:
            mu.append(m), role.append(r), cluster.append(g), batch.append(b)
    mu = np.array(mu)
    role, cluster, batch = np.array(role), np.array(cluster), np.array(batch)
    points = []
    for b in (0, 1):
        sets = [np.tile(voxel_points(m, LIVE_SPREAD), (16, 1)) if r == NEARER else voxel_points(m, LIVE_SPREAD)
                for m, r, bb in zip(mu, role, batch) if bb == b]
        points.append(np.concatenate(sets))
    return {"res": res, "d": d, "batches": points, "mu": mu, "cell": np.floor(mu / res).astype(np.int64), "role": role,
            "cluster": cluster, "batch": batch, "axis": np.array(axis_of), "centre": np.array(centre)}


def live_queries(layout, r2, means, cells):
    """Radius and tie islands around the means READ BACK from the store (means [S][3], cells [S][3] of stats()): per single
    voxel, along its cluster's axis, step(m +- sqrt(radius_sq), a) for a in -6..6; per tie cluster the midpoint of its
    lower and upper mean.  → (queries [n][3], family [n], slot [n]: the store slot of the single / lower voxel)"""
    slot_of = {tuple(c): s for s, c in enumerate(np.asarray(cells).tolist())}
    c = math.sqrt(r2)
    q, family, slots = [], [], []
    for v in np.nonzero(layout["role"] == SINGLE)[0]:
        s = slot_of[tuple(layout["cell"][v].tolist())]
        axis = layout["axis"][layout["cluster"][v]]
        for sign in (1.0, -1.0):
            for a in ULPS:
                p = means[s].copy()
                p[axis] = step(means[s][axis] + sign * c, a)
                q.append(p), family.append("radius"), slots.append(s)
    for v in np.nonzero(layout["role"] == LOWER)[0]:
        g = layout["cluster"][v]
        s = slot_of[tuple(layout["cell"][v].tolist())]
        up = slot_of[tuple(layout["cell"][np.nonzero((layout["cluster"] == g) & (layout["role"] == UPPER))[0][0]].tolist())]
        axis = layout["axis"][g]
        p = means[s].copy()
        p[axis] = 0.5 * (means[s][axis] + means[up][axis])
        q.append(p), family.append("tie"), slots.append(s)
    return np.array(q), np.array(family), np.array(slots)
