"""Inputs and yardsticks of the place-recognition tests (tests/test_place_host.py, test_place_descriptor.py,
test_place_search.py, test_place_pipeline.py).  No tests here, and nothing here needs a GPU.

descriptor / distance   the rule of include/nos.h and DESIGN.md §27 in plain numpy float64, operation by operation in the
                        order the rule states (sums over the rings and over the columns are sequential, ascending).
descriptor_slow / distance_slow   the same as pure-Python double loops over scalars: what the numpy forms are checked against.
scan_points             points drawn by rejection so that every point's r R / max_range and a S / 2 pi lie at least MARGIN
                        from an integer: a device atan2 or a fused x x + y y that differs from numpy in the last bits
                        (1e-13 of a bin at most) cannot move a point to another bin.
random_descriptors      descriptors for the search tests: random heights, empty bins, empty columns.
place_cloud / query_cloud   the "places" of the pipeline test."""
import math

import numpy as np

TWO_PI = 2.0 * np.pi
MARGIN = 1e-9
PARAM_SETS = ((1, 1), (3, 5), (20, 60), (64, 128))  # (n_rings, n_sectors)
MAX_RANGE = 80.0
Z_FLOOR = -2.0
SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 100_003)


# ------------------------------------------------------------------------------ the rule, in numpy

def bins_of(points, n_rings, n_sectors, max_range, z_floor):
    """→ (used [n] bool, ring [n_used], sector [n_used], z [n_used], ring product [n_finite], sector product [n_finite])."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r = np.sqrt(x * x + y * y)
        used = finite & (z >= z_floor) & (r < max_range)
        ring_product = r * (n_rings / max_range)
        a = np.arctan2(y, x)
        a = np.where(a < 0.0, a + TWO_PI, a)
        sector_product = a * (n_sectors / TWO_PI)
    ring = np.minimum(np.floor(ring_product[used]).astype(np.int64), n_rings - 1)
    sector = np.floor(sector_product[used]).astype(np.int64) % n_sectors
    sector[(x[used] == 0.0) & (y[used] == 0.0)] = 0
    return used, ring, sector, z[used], ring_product[finite], sector_product[finite]


def descriptor(points, n_rings=20, n_sectors=60, max_range=MAX_RANGE, z_floor=Z_FLOOR):
    """→ (desc [n_rings, n_sectors], n_used)."""
    used, ring, sector, z, _, _ = bins_of(points, n_rings, n_sectors, max_range, z_floor)
    zmax = np.full(n_rings * n_sectors, -np.inf)
    np.maximum.at(zmax, ring * n_sectors + sector, z)
    empty = zmax == -np.inf
    desc = np.where(empty, 0.0, np.where(empty, 0.0, zmax) - z_floor)  # one subtraction per bin, after the maximum
    return desc.reshape(n_rings, n_sectors), int(np.count_nonzero(used))


def column_norms(a):
    """[..., R, S] → [..., S]: sqrt(sum_i a[i][j]^2), rings ascending."""
    a = np.asarray(a, dtype=np.float64)
    acc = np.zeros(a.shape[:-2] + a.shape[-1:])
    for i in range(a.shape[-2]):
        acc = acc + a[..., i, :] * a[..., i, :]
    return np.sqrt(acc)


def shift_distances(q, cands):
    """q [R, S], cands [n, R, S] → d [n, S]: d_s of every candidate at every shift."""
    q = np.asarray(q, dtype=np.float64)
    cands = np.asarray(cands, dtype=np.float64)
    n, R, S = cands.shape
    nq, nc = column_norms(q), column_norms(cands)
    table = np.zeros((n, S, S))  # table[c, j, k] = sum_i q[i][j] * cand[c][i][k], rings ascending
    for i in range(R):
        table = table + q[i][None, :, None] * cands[:, i, None, :]
    j = np.arange(S)
    d = np.ones((n, S))
    for s in range(S):
        k = (j + s) % S
        valid = (nq[None, :] > 0.0) & (nc[:, k] > 0.0)
        with np.errstate(all="ignore"):
            term = np.where(valid, 1.0 - table[:, j, k] / (nq[None, :] * nc[:, k]), 0.0)
        total = np.zeros(n)
        for col in range(S):  # columns ascending; an invalid column adds an exact zero
            total = total + term[:, col]
        m = np.count_nonzero(valid, axis=1)
        d[:, s] = np.where(m > 0, total / np.maximum(m, 1), 1.0)
    return d


def distance(q, cands):
    """q [R, S], cands [n, R, S] → (d [n], shift [n] int32, gap [n]): the minimum over the shifts, the smallest shift that
    attains it, and how far the second-best shift's d_s lies above it (inf when there is one shift)."""
    d = shift_distances(q, cands)
    shift = np.argmin(d, axis=1)  # the first occurrence: the smallest shift
    best = d[np.arange(len(d)), shift]
    if d.shape[1] > 1:
        gap = np.sort(d, axis=1)[:, 1] - best
    else:
        gap = np.full(len(d), np.inf)
    return best, shift.astype(np.int32), gap


# ------------------------------------------------------------------------------ the rule, in scalar loops

def descriptor_slow(points, n_rings, n_sectors, max_range, z_floor):
    zmax = [[None] * n_sectors for _ in range(n_rings)]
    n_used = 0
    for x, y, z in np.asarray(points, dtype=np.float64).reshape(-1, 3).tolist():
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        if not z >= z_floor:
            continue
        r = math.sqrt(x * x + y * y)
        if not r < max_range:
            continue
        i = min(int(math.floor(r * (n_rings / max_range))), n_rings - 1)
        if x == 0.0 and y == 0.0:
            j = 0
        else:
            a = math.atan2(y, x)
            if a < 0.0:
                a = a + 2.0 * math.pi
            j = int(math.floor(a * (n_sectors / (2.0 * math.pi)))) % n_sectors
        n_used += 1
        if zmax[i][j] is None or z > zmax[i][j]:
            zmax[i][j] = z
    desc = [[0.0 if v is None else v - z_floor for v in row] for row in zmax]
    return np.array(desc, dtype=np.float64).reshape(n_rings, n_sectors), n_used


def distance_slow(q, c):
    """q, c [R, S] → (d, shift)."""
    q, c = np.asarray(q, dtype=np.float64).tolist(), np.asarray(c, dtype=np.float64).tolist()
    R, S = len(q), len(q[0])

    def norm(a, j):
        acc = 0.0
        for i in range(R):
            acc = acc + a[i][j] * a[i][j]
        return math.sqrt(acc)

    nq = [norm(q, j) for j in range(S)]
    nc = [norm(c, j) for j in range(S)]
    best, best_s = None, None
    for s in range(S):
        total, m = 0.0, 0
        for j in range(S):
            k = (j + s) % S
            if nq[j] > 0.0 and nc[k] > 0.0:
                dot = 0.0
                for i in range(R):
                    dot = dot + q[i][j] * c[i][k]
                total = total + (1.0 - dot / (nq[j] * nc[k]))
                m += 1
        d = total / m if m > 0 else 1.0
        if best is None or d < best:
            best, best_s = d, s
    return best, best_s


# ------------------------------------------------------------------------------ scans

def _margin_ok(points, n_rings, n_sectors, max_range):
    _, _, _, _, rp, sp = bins_of(points, n_rings, n_sectors, max_range, -np.inf)
    ok = np.ones(len(points), dtype=bool)
    finite = np.all(np.isfinite(points), axis=1)
    bad = (np.abs(rp - np.rint(rp)) < MARGIN) | (np.abs(sp - np.rint(sp)) < MARGIN)
    ok[finite] = ~bad
    return ok


def scan_points(n, n_rings, n_sectors, max_range=MAX_RANGE, z_floor=Z_FLOOR, seed=0, specials=True):
    """→ (points [n, 3], n_rejected draws).  Range to 1.15 max_range (some points beyond it), z from 1 m below the floor to
    6 m above it (negative z above the floor, points below it); with specials, every 17th point from the 5th on has a NaN,
    +inf or -inf coordinate.  Drawn by rejection: see the module docstring."""
    rng = np.random.default_rng(1000 + seed)

    def draw(k):
        r = rng.uniform(0.0, 1.15 * max_range, size=k)
        a = rng.uniform(-np.pi, np.pi, size=k)
        return np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(z_floor - 1.0, z_floor + 6.0, size=k)], axis=1)

    pts = draw(n)
    rejected = 0
    while True:
        bad = np.flatnonzero(~_margin_ok(pts, n_rings, n_sectors, max_range))
        if bad.size == 0:
            break
        rejected += bad.size
        pts[bad] = draw(bad.size)
    if specials:
        values = (np.nan, np.inf, -np.inf)
        for k, idx in enumerate(range(5, n, 17)):
            pts[idx, k % 3] = values[(k // 3) % 3]
    return pts, rejected


# ------------------------------------------------------------------------------ descriptors for the search

def random_descriptors(n, n_rings, n_sectors, seed=0):
    """→ [n, R, S]: heights in [0, 6), about a third of the bins empty, about one column in eight empty."""
    rng = np.random.default_rng(2000 + seed)
    d = rng.uniform(0.0, 6.0, size=(n, n_rings, n_sectors))
    d[rng.uniform(size=d.shape) < 0.33] = 0.0
    d = d * (rng.uniform(size=(n, 1, n_sectors)) >= 0.125)
    return np.ascontiguousarray(d)


# ------------------------------------------------------------------------------ places

N_PLACES = 12
PLACE_POINTS = 4000
SENSOR_HEIGHT = 1.7


def place_cloud(place):
    """→ [4000, 3], sensor frame: a 24 x 24 m ground patch under the sensor and 30 vertical pillars within 40 m."""
    rng = np.random.default_rng(3000 + place)
    n_ground = PLACE_POINTS - 30 * 70
    ground = np.stack([rng.uniform(-12.0, 12.0, n_ground), rng.uniform(-12.0, 12.0, n_ground),
                       -SENSOR_HEIGHT + rng.normal(0.0, 0.01, n_ground)], axis=1)
    parts = [ground]
    for _ in range(30):
        r, a = rng.uniform(4.0, 38.0), rng.uniform(-np.pi, np.pi)
        height, radius = rng.uniform(1.5, 9.0), rng.uniform(0.2, 0.6)
        b = rng.uniform(-np.pi, np.pi, 70)
        parts.append(np.stack([r * np.cos(a) + radius * np.cos(b), r * np.sin(a) + radius * np.sin(b),
                               -SENSOR_HEIGHT + rng.uniform(0.0, height, 70)], axis=1))
    return np.concatenate(parts)


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


QUERY_SHIFT = np.array([0.25, -0.15, 0.05])  # 0.3 m


def query_cloud(place, whole_sectors, n_sectors=60):
    """The place seen again from a sensor yawed by +phi = (whole_sectors + 1/3) sectors and moved by QUERY_SHIFT: 20 % of the
    points dropped, 2 cm of noise.  → (points in the query's sensor frame, phi).  A stored point p is
    Rz(phi) p_query + QUERY_SHIFT: the query's true pose in the stored frame is (Rz(phi), QUERY_SHIFT)."""
    rng = np.random.default_rng(4000 + 100 * place + whole_sectors)
    phi = (whole_sectors + 1.0 / 3.0) * TWO_PI / n_sectors
    p = place_cloud(place)
    p = p[rng.uniform(size=len(p)) >= 0.2]
    q = (p - QUERY_SHIFT) @ rot_z(phi)  # rows: Rz(-phi) (p - d)
    return q + rng.normal(0.0, 0.02, q.shape), phi


QUERIES = ((2, 7), (5, 31), (9, 52))  # (place, whole sectors of yaw)
