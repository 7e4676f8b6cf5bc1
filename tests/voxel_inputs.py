"""Point sets of single NDT voxels at the places where the per-voxel finish (csrc/voxel_finish.hpp) and the sums that
feed it can go wrong — TEST INFRASTRUCTURE shared by test_voxel_oracle.py (CPU) and test_voxel_stats_xprec.py (GPU).

A family is the point set of ONE voxel inside the unit cell [0, 1)³ of a grid of edge 1.  cloud() places every family at
every cell offset of OFFSETS: local point = family point + a small integer shift that gives the voxel a cell of its own,
map point = fl(local + offset · resolution).  Families on a coarse binary lattice survive that addition exactly at every
offset; the others (near-ties, tiny rotations) are what they claim to be at offset 0 and are rounded to the grid of the
far cell elsewhere — the reference (oracle/oracle_voxel_xp.py) is always evaluated on the points the kernel is handed.
"""
import functools

import numpy as np

LATTICE = 2.0 ** -30   # fl(x + c) is exact for x on this lattice in [0, 1) and every integer |c| <= 2^20 (ulp 2^-32 there)
CENTER = np.array([0.5, 0.5, 0.5])


def _snap(p):
    return np.round(np.asarray(p, dtype=np.float64) / LATTICE) * LATTICE


def _rot(axis, angle):
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _corners(half, R=None):
    """the eight points CENTER ± (sx, sy, sz), optionally rotated about CENTER"""
    signs = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)
    d = signs * np.asarray(half, dtype=np.float64)
    return CENTER + (d if R is None else d @ R.T)


def _lam_max(pts):
    """largest eigenvalue of (Σ d dᵀ + I)/n − m mᵀ in longdouble sums (design aid; the tests ask the 50-digit oracle)"""
    d = pts.astype(np.longdouble) - np.longdouble(0.5)
    n = len(d)
    m = d.sum(axis=0) / n
    cov = ((d[:, :, None] * d[:, None, :]).sum(axis=0) + np.eye(3)) / n - np.outer(m, m)
    return np.linalg.eigvalsh(cov.astype(np.float64))


def _scaled_to(shape, want, what):
    """shape [n,3] about 0, scaled so that what(eigenvalues of the snapped point set) = want (bisection on the scale)"""
    lo, hi = 1e-3, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if what(_lam_max(_snap(CENTER + mid * shape))) < want:
            lo = mid
        else:
            hi = mid
    return _snap(CENTER + hi * shape), _snap(CENTER + lo * shape)  # just above, just below


@functools.lru_cache(maxsize=None)
def families():
    """→ dict name → points [n,3] in [0,1)³ (insertion-ordered)."""
    rng = np.random.default_rng(20261018)
    fam = {}
    # both sides of min_points = 5 and of the 64-lane stride of voxel_sums_kernel, and many rounds of it
    for n in (4, 5, 63, 64, 65, 1000):
        fam["random_%d" % n] = _snap(rng.uniform(0.05, 0.95, size=(n, 3)))
    # eight lattice points: every sum exact, eigenvalues EXACTLY tied
    fam["lattice_plane"] = _corners([0.25, 0.25, 2.0 ** -7])      # the two large eigenvalues tie
    # the two small ones tie and are both floored.  The identity the moment starts from leaves 1/n in every eigenvalue, so
    # nothing of an eight-point voxel is floored (1/8 > 0.01 λmax in a unit cell): each lattice point 128 times, still exact
    fam["lattice_line"] = np.tile(_corners([2.0 ** -8, 2.0 ** -8, 0.4375]), (128, 1))
    fam["lattice_line_unfloored"] = _corners([0.125, 0.125, 0.375])  # the two small ones tie above the floor
    fam["lattice_cube"] = _corners([0.25, 0.25, 0.25])            # three-way tie
    # near-ties on both sides of the 1e-9 tie rule, axis-aligned and rotated by fixed angles about two axes
    R2 = _rot(2, 0.3) @ _rot(0, -0.7)
    for g in (1e-12, 1e-10, 1e-8, 1e-6, 1e-4):
        half = [0.2, 0.2 * (1.0 + g), 0.05]
        fam["near_tie_%g" % g] = _corners(half)
        fam["near_tie_%g_rotated" % g] = _corners(half, R2)
    # a box turned about z by angles that straddle the 1e-13 off-diagonal skip of the Jacobi sweep
    for a in (1e-15, 1e-13, 1e-11):
        fam["box_rot_z_%g" % a] = _corners([0.3, 0.15, 0.05], _rot(2, a))
    # thin slabs of 1000 points, tilted: I/n + σ² against the floor 0.01 λmax, one just above and one just below
    n = 1000
    xi = rng.uniform(0.5, 1.0, size=n) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)   # two bands: a large in-plane variance
    slab = np.stack([xi, rng.uniform(-0.5, 0.5, size=n), np.zeros(n)], axis=1)
    thick = rng.normal(0.0, 0.002, size=n)
    tilt = _rot(0, 0.05)

    def slab_points(scale):
        return _snap(CENTER + (np.stack([scale * slab[:, 0], 0.5 * slab[:, 1], thick], axis=1)) @ tilt.T)

    def slab_ratio(scale):  # smallest eigenvalue over the floor
        w = _lam_max(slab_points(scale))
        return w[0] / (0.01 * w[2])

    for name, want in (("slab_above_floor", 1.02), ("slab_below_floor", 0.98)):
        lo, hi = 0.2, 0.49  # the ratio falls as the slab grows
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if slab_ratio(mid) > want:
                lo = mid
            else:
                hi = mid
        fam[name] = slab_points(hi)
    # slivers of 200 points (I/n = 0.005): the true largest eigenvalue at 0.01 (1 ± 1e-6), one valid and one invalid
    u = np.linspace(-1.0, 1.0, 200)
    shape = np.stack([u, 0.05 * np.sin(7.0 * u), 0.02 * np.cos(5.0 * u)], axis=1) @ _rot(2, 0.4).T @ _rot(1, 0.2).T
    fam["sliver_valid"] = _scaled_to(shape, 0.01 * (1.0 + 1e-6), lambda w: w[2])[0]
    fam["sliver_invalid"] = _scaled_to(shape, 0.01 * (1.0 - 1e-6), lambda w: w[2])[1]
    for name, p in fam.items():
        assert p.min() >= 0.0 and p.max() < 1.0, name
    return fam


# on-lattice families: fl(point + integer) is exact at every offset (test_voxel_oracle.py asserts it)
def on_lattice(name):
    return name.startswith(("random_", "lattice_", "slab_", "sliver_"))


B10, B15, B19, B20 = 1 << 10, 1 << 15, 1 << 19, 1 << 20
# cell offsets (in cells), with the axis along which the voxels of one offset are lined up
OFFSETS = (
    ((0, 0, 0), 0),
    ((B10, -B10, B10), 0),
    ((-B10, B10, -B10), 1),
    ((B15, B15, -B15), 2),
    ((-B15, -B15, B15), 0),
    ((B19, -B19, -B19), 1),
    ((-B19, B19, B19), 2),
    ((B20 - 1, 0, 0), 1),     # the last addressable cell on x
    ((0, 0, -B20), 0),        # the first one on z
)


class Cloud:
    """points [N,3] (map frame, shuffled); voxels: list of dicts name / offset (index) / cell / idx (rows of points);
    local [N,3] and shift [N,3] with points == fl(local + shift) (what insert_scan needs); group [N] = offset index."""


@functools.lru_cache(maxsize=None)
def cloud(resolution=1.0, offsets=None, generic=False):
    """Every family at every offset (offsets: indices into OFFSETS, default all) on a grid of edge `resolution` — a power
    of two, so that scaling the unit cell and the offsets is exact.  generic=True: one family of 40 random points per
    offset at a resolution that need not be a power of two; cells are then what floor(p · (1 / resolution)) says."""
    offsets = tuple(range(len(OFFSETS))) if offsets is None else tuple(offsets)
    rng = np.random.default_rng(7)
    local, shift, group, names, cells = [], [], [], [], []
    inv_res = 1.0 / resolution
    for oi in offsets:
        off, axis = OFFSETS[oi]
        fams = {"generic_40": None} if generic else families()
        for j, (name, p) in enumerate(fams.items()):
            step = np.zeros(3)
            step[axis] = 2.0 * j  # every other cell along the line: no two voxels share or touch a cell
            if generic:
                base = (np.array(off, dtype=np.float64) + step) * resolution
                pts = base + rng.uniform(0.1, 0.9, size=(40, 3)) * resolution  # well inside one cell
                c = np.floor(pts * inv_res).astype(np.int64)
                assert np.all(c == c[0]), "a generic voxel straddles cells"
                loc, sh, cell = pts, np.zeros(3), c[0]
            else:
                loc = (p + step) * resolution
                sh = np.array(off, dtype=np.float64) * resolution
                cell = np.array(off, dtype=np.int64) + step.astype(np.int64)
            local.append(loc)
            shift.append(np.broadcast_to(sh, loc.shape))
            group.append(np.full(len(loc), oi))
            names.append((name, oi, len(loc)))
            cells.append(cell)
    local, shift, group = np.concatenate(local), np.concatenate(shift), np.concatenate(group)
    order = rng.permutation(len(local))  # voxels interleaved: the sort has work to do
    where = np.empty(len(local), dtype=np.int64)
    where[order] = np.arange(len(local))
    c = Cloud()
    c.resolution = resolution
    c.local, c.shift, c.group = local[order], shift[order], group[order]
    c.points = c.local + c.shift
    c.voxels = []
    start = 0
    for (name, oi, n), cell in zip(names, cells):
        c.voxels.append({"name": name, "offset": oi, "cell": tuple(int(x) for x in cell), "idx": np.sort(where[start:start + n])})
        start += n
    got = np.floor(c.points * inv_res).astype(np.int64)
    for v in c.voxels:
        assert np.all(got[v["idx"]] == np.array(v["cell"])), (v["name"], v["offset"])
    return c


@functools.lru_cache(maxsize=None)
def reference(c):
    """The 50-digit statistics of every voxel of a cloud (oracle_voxel_xp.voxel_stats_xp), in the order of c.voxels,
    computed once per session."""
    from oracle import oracle_voxel_xp as vx
    return [vx.voxel_stats_xp(c.points[v["idx"]], v["cell"], c.resolution) for v in c.voxels]


def three_batches(c):
    """Row indices of three batches that split EVERY voxel of the cloud (its points dealt round-robin)."""
    batch = np.zeros(len(c.points), dtype=np.int64)
    for v in c.voxels:
        batch[v["idx"]] = np.arange(len(v["idx"])) % 3
    return [np.nonzero(batch == b)[0] for b in range(3)]


def corner_sums(points, cell, resolution):
    """count and the nine fp64 sums sx sy sz | mxx mxy mxz myy myz mzz of d = p − cell · resolution: what the sum kernels
    hand the finish, formed here in numpy (pairwise sums: another order than the kernels')."""
    d = np.asarray(points, dtype=np.float64) - np.array(cell, dtype=np.float64) * resolution
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    return len(d), np.array([d[:, 0].sum(), d[:, 1].sum(), d[:, 2].sum()] + [(d[:, a] * d[:, b]).sum() for a, b in pairs])


# ---------------------------------------------------------------- the bounds every path is held to

MEAN_ULPS = 2.0      # one rounding in the corner, one in the final add
EIG_RTOL = 1e-11     # floored eigenvalues, from 1 / diag(S Sᵀ)
INFO_RTOL = 1e-10    # information matrix, Frobenius, + the gap of a pair the tie rule merges (oracle_voxel_xp.merged_gap).
# Where 1e-10 comes from: the Jacobi sweep neglects off-diagonals up to 1e-13 relative and stops at 1e-26, i.e. it
# returns the exact decomposition of cov + E with ‖E‖ ≲ 3e-13 ‖cov‖; flooring caps the condition number of
# cov → information at 100; the product is about 3e-11.
ORTHO_TOL = 1e-13    # ‖V Vᵀ − I‖_F of the eigenvector matrix recovered from S: rotations accumulate a few eps


def errors(c, ref, got, proper):
    """got: dict with means [V,3], sqrt_infos [V,3,3], valid [V], counts [V], cells [V,3] of a superset of the cloud's
    voxels, in any order; ref = reference(c) → one dict per voxel of the cloud: name, offset, cell, found, count_equal,
    valid_equal, identity (S of an invalid voxel is I), and for valid ones mean (ulps of the voxel's largest coordinate),
    eig (floored eigenvalues, relative), ortho, info (relative Frobenius), gap (what the tie rule may add to it)."""
    from oracle import oracle_voxel_xp as vx
    row = {tuple(int(x) for x in cell): k for k, cell in enumerate(np.asarray(got["cells"]))}
    out = []
    for v, r in zip(c.voxels, ref):
        e = {"name": v["name"], "offset": v["offset"], "cell": v["cell"], "found": v["cell"] in row, "ref_valid": r["valid"]}
        out.append(e)
        if not e["found"]:
            continue
        k = row[v["cell"]]
        e["count_equal"] = int(got["counts"][k]) == r["n"]
        e["valid_equal"] = bool(got["valid"][k]) == r["valid"]
        S = np.asarray(got["sqrt_infos"][k], dtype=np.float64).reshape(3, 3)
        e["identity"] = bool(np.array_equal(S, np.eye(3)))
        if not (r["valid"] and bool(got["valid"][k])):
            continue
        ulp = np.spacing(np.abs(c.points[v["idx"]]).max())
        e["mean"] = float(np.abs(np.asarray(got["means"][k], dtype=np.longdouble) - r["mean"]).max() / ulp)
        info, lam, e["ortho"] = vx.information_from_sqrt(S, proper)
        e["eig"] = float(np.abs(lam / r["eig_floored"] - 1.0).max())
        e["gap"] = vx.merged_gap(r)
        e["info"] = float(np.linalg.norm(info - r["info"]) / np.linalg.norm(r["info"]))
    return out


def compare(c, ref, got, proper, what):
    """Asserts the bounds above for every voxel of the cloud (errors()) → {family name: [mean error in ulps, eigenvalue
    error, information error − allowed gap]} maxima."""
    worst = {}
    for e in errors(c, ref, got, proper):
        tag = "%s: %s at offset %d, cell %s" % (what, e["name"], e["offset"], e["cell"])
        assert e["found"] and e["count_equal"], tag
        assert e["valid_equal"], tag
        if not e["ref_valid"]:
            assert e["identity"], tag  # what an invalid voxel carries
            continue
        w = worst.setdefault(e["name"], [0.0, 0.0, 0.0])
        w[0], w[1], w[2] = max(w[0], e["mean"]), max(w[1], e["eig"]), max(w[2], e["info"] - e["gap"])
        assert e["mean"] <= MEAN_ULPS, (tag, e["mean"])
        assert e["eig"] <= EIG_RTOL, (tag, e["eig"])
        assert e["ortho"] <= ORTHO_TOL, (tag, e["ortho"])
        assert e["info"] <= INFO_RTOL + e["gap"], (tag, e["info"], e["gap"])
    return worst


# ---------------------------------------------------------------- the clouds and the paths the statistics take

# (resolution, offsets, generic): every family at every offset on a 1 m grid; at three offsets on a 0.5 m grid (exact
# too); one generic family per offset at 0.3 m, where neither the cell edge nor its inverse is a binary fraction
CLOUDS = {
    "res1": (1.0, None, False),
    "res0.5": (0.5, (0, 6, 8), False),
    "res0.3": (0.3, None, True),
}

PATHS = ("build_compact_keys", "build_packed_keys", "insert_one_batch", "insert_three_batches", "insert_scan", "insert_then_prune")


def run_path(api, ctx, c, path, proper):
    """The statistics of the cloud's voxels as one path of the library computes them (a GPU is needed) → stats dict."""
    res = c.resolution
    if path.startswith("build"):
        # search radius 2 m: the MATCHER's table (cells of one search radius) takes cells up to ±(2^20 − 2), and the voxels
        # at 2^20 − 1 and −2^20 m have to fit it; the statistics do not depend on it
        with ctx.options(map_compact_keys=1 if path == "build_compact_keys" else 0):
            m, st = api.NdtMap.build(ctx, c.points, res, 4.0, proper_sqrt_information=proper)
        m.close()
        return st
    vm = api.VoxelMap(ctx, res, 1.0, proper_sqrt_information=proper)
    try:
        if path == "insert_one_batch":
            vm.insert(c.points)
        elif path == "insert_three_batches":  # every voxel is created by one batch and merged into by two more
            for rows in three_batches(c):
                vm.insert(c.points[rows])
        elif path == "insert_scan":  # R = I and t = the offset: the warp gives fl(local + t), the map point itself
            for oi in np.unique(c.group):
                rows = np.nonzero(c.group == oi)[0]
                t = c.shift[rows[0]]
                assert np.all(c.shift[rows] == t)
                scan = api.Scan(ctx, c.local[rows])
                vm.insert_scan(scan, np.eye(3), t)
                scan.close()
        elif path == "insert_then_prune":  # a voxel of an older insert goes: every survivor moves to a fresh block
            vm.insert(np.array([3.0, 3.0, 3.0]) * res + 0.5 * res * np.random.default_rng(1).uniform(size=(9, 3)))
            vm.insert(c.points)
            before = vm.memory()["generation"]
            assert vm.prune(max_age=0) == 1 and vm.memory()["generation"] == before + 1
        else:
            raise ValueError(path)
        return vm.stats()
    finally:
        vm.close()
