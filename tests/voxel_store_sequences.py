"""Seeded programs of operations on two voxel stores — TEST INFRASTRUCTURE shared by test_voxel_store_model_host.py (CPU)
and test_voxel_store_life.py (GPU).

program(seed, res_a, res_b) → a list of about 40 operations (dicts, key "op") on store A (resolution res_a, created with
capacity=0: 16 slots, it has to grow) and store B (resolution res_b).  SETUPS are (1.0, 1.0) and (1.0, 0.5): in the second
the merges go into the coarser grid.

Every truth is bit exact because of what is emitted:
  * every point and every sensor origin has coordinates that are ODD multiples of 2^-10, so none is ever on a cell face at
    either resolution, an axis rotation cannot move one across a face, and the live matcher's guard band holds;
  * points lie in [-12, 12) x [-12, 12) x [-2, 2), batches hold 1 500 – 4 000 of them;
  * poses are the 24 axis rotations with translations of whole destination cells, at most 9 per axis;
  * |x| <= 64 for everything, moved points included (asserted): every sum is exact in any order.
A carve's rays whose walk a rounding could change (voxel_carve_inputs.near_tie; only the shortened end point b can be
general) are left out of the scan before anybody sees it; "drawn" and "dropped" say how many, and at most 1 % may be.

The kinds are drawn with fixed weights (KINDS); the slots of SCRIPT that name a kind are the situations every program has
to contain (a carve that takes the store below a quarter of its capacity, a merge after the destination was carved, a
merge from a source that was carved and pruned, an age prune after a merge, a box small enough to shrink the store, the
empty merge, the dry run, the short max_range).  Where a situation depends on the state — the box that leaves just more
than a quarter of the capacity — the generator runs the model along and picks it; the program is still a function of
(seed, res_a, res_b, scale) alone."""
import functools

import numpy as np

from tests import voxel_carve_inputs as ci
from tests.voxel_merge_inputs import axis_rotations
from tests.voxel_store_model import Model

SEEDS = (1, 2, 3)
SETUPS = ((1.0, 1.0), (1.0, 0.5))
LO, HI = np.array([-12, -12, -2]), np.array([12, 12, 2])
TOO_MANY = 4500  # voxels: the next drawn operation on that store becomes a box prune

KINDS = (("insert_A", 4), ("insert_B", 3), ("scan_plain", 1), ("scan_sort", 1), ("scan_filter", 1), ("box_A", 2), ("box_B", 1),
         ("age_A", 2), ("age_B", 1), ("carve_A", 3), ("carve_B", 2), ("merge", 3))
SCRIPT = ("insert_A_small", "insert_A_full", None, None, "insert_B", None, "carve_A", None, "merge", None,
          "quarter_A", "carve_A_shrinks", "insert_B", "merge", "age_A_0",
          None, "scan_plain", None, "insert_B", "carve_B", "box_B", "merge", "age_A_2",
          None, "merge_empty", "small_box_A", "insert_A_full", "scan_filter", None, "carve_dry", None, "carve_short",
          "scan_sort", "age_B", "insert_A_full", "insert_B", "carve_B", "merge", "age_A_5", "insert_A")
CARVE_RULES = ((2, 1), (5, 1), (50, 2))
BOXES = (((0.0, 0.0, 0.0), (8.0, 8.0, 2.0)),  # faces exactly on cell boundaries at both resolutions
         ((-2.0, 1.0, 0.0), (10.25, 7.5, 3.0)), ((1.5, -2.5, 0.0), (6.0, 6.0, 2.0)), ((0.3, -0.7, 0.1), 9.3),
         ((-4.0, 4.0, 0.0), (6.0, 6.0, 1.0)))  # faces on cell boundaries again, off centre


def is_odd_lattice(x):
    """every coordinate an odd multiple of 2^-10, |x| <= 64"""
    k = np.asarray(x, dtype=np.float64) * 1024.0
    return bool(np.all(k == np.round(k)) and np.all(np.mod(k, 2.0) == 1.0) and np.all(np.abs(x) <= 64))


def _odd(rng, lo, hi, n):
    lo, hi = np.asarray(lo, dtype=np.float64) * 512, np.asarray(hi, dtype=np.float64) * 512
    assert np.array_equal(lo, np.round(lo)) and np.array_equal(hi, np.round(hi))
    k = rng.integers(lo.astype(np.int64), hi.astype(np.int64), size=(n, 3))
    return (2 * k + 1).astype(np.float64) / 1024.0


def _pose(rng, res):
    return axis_rotations()[int(rng.integers(24))].copy(), rng.integers(-9, 10, size=3).astype(np.float64) * res


def first_per_voxel(points, edge):
    """nos_scan_filter's rule on a never-sorted scan: the first point of every voxel of that edge, in input order"""
    cells = np.floor(points * (1.0 / edge)).astype(np.int64)
    _, first = np.unique(cells, axis=0, return_index=True)
    return points[np.sort(first)]


def apply(op, A, B):
    """one operation on the models → what the store's call returns (a carve: removed, skipped, crossings, hits)"""
    kind = op["op"]
    m = A if op.get("store", "A") == "A" else B
    if kind == "insert":
        return m.insert(op["points"])
    if kind == "insert_scan":
        return A.insert_scan(op["stored"], op["R"], op["t"])
    if kind == "prune":
        return m.prune(op["center"], op["half_extent"], op["max_age"])
    if kind == "carve":
        return m.carve(op["points"], op["R"], op["t"], **op["how"])
    if kind == "merge":
        return A.merge(B, op["R"], op["t"])
    assert kind == "merge_empty"
    return A.merge(Model(op["res"]), op["R"], op["t"])


class _Generator:
    def __init__(self, seed, res_a, res_b, scale):
        self.rng = np.random.default_rng([seed, int(res_a * 16), int(res_b * 16)])
        self.scale = scale
        self.A, self.B = Model(res_a, capacity=0), Model(res_b)
        self.ops = []
        self.rule = 0  # the carve rules and margins go round
        names, weights = zip(*KINDS)
        self.names, self.p = names, np.array(weights, dtype=np.float64) / sum(weights)

    def model(self, store):
        return self.A if store == "A" else self.B

    def emit(self, op):
        for key in ("points", "stored", "origin_map"):
            if key in op:
                assert is_odd_lattice(op[key]), (op["op"], key)
        result = apply(op, self.A, self.B)
        if op["op"] == "merge" and result:
            assert is_odd_lattice(self.A.history[-1][1])  # the moved points of the source
        self.ops.append(op)
        return result

    def size(self, lo=1500, hi=4000):
        return max(8, int(self.rng.integers(lo, hi + 1) * self.scale))

    # ------------------------------------------------------------------------------------------------- the kinds

    def batch(self, store, full=False, small=False):
        res = self.model(store).res
        if full:
            return _odd(self.rng, LO, HI, self.size(3000, 4000))
        half = (2 if small else int(self.rng.choice([3, 4, 6]))) * res  # a sub-box of 4 … 12 cells across, the whole height
        c = self.rng.integers(np.ceil(LO[:2] + half).astype(np.int64), np.floor(HI[:2] - half).astype(np.int64) + 1, size=2)
        return _odd(self.rng, [c[0] - half, c[1] - half, LO[2]], [c[0] + half, c[1] + half, HI[2]], self.size())

    def insert(self, store, **kw):
        self.emit({"op": "insert", "store": store, "points": self.batch(store, **kw)})

    def scan(self, sort_cell=None, filter_voxel=None):
        R, t = _pose(self.rng, self.A.res)
        pts = self.batch("A")
        stored = first_per_voxel(pts, filter_voxel) if filter_voxel else pts
        moved = stored @ R.T + t
        assert is_odd_lattice(moved)
        self.emit({"op": "insert_scan", "points": pts, "stored": stored, "R": R, "t": t, "sort_cell": sort_cell,
                   "filter_voxel": filter_voxel})

    def box(self, store, box=None):
        if box is None:
            box = BOXES[int(self.rng.integers(len(BOXES)))]
        self.emit({"op": "prune", "store": store, "center": box[0], "half_extent": box[1], "max_age": None})

    def age(self, store, max_age=None):
        max_age = int(self.rng.choice([0, 2, 5])) if max_age is None else max_age
        self.emit({"op": "prune", "store": store, "center": None, "half_extent": None, "max_age": max_age})

    def carve_op(self, store, rule=None, end_margin=None, max_range=None, dry_run=False, around=None, rng=None):
        """rays from an origin near `around` (map frame) to lattice points of the region, seen under an axis pose"""
        rng = self.rng if rng is None else rng
        m = self.model(store)
        if rule is None:
            rule, end_margin = CARVE_RULES[self.rule % 3], (1.5 * m.res, 0.0)[(self.rule // 3) % 2]
            self.rule += 1
        R, t = _pose(rng, m.res)
        around = np.zeros(3) if around is None else np.asarray(around, dtype=np.float64)
        origin_map = _odd(rng, around + [-2, -2, -1], around + [2, 2, 1], 1)[0]
        n = int(rng.integers(310, 601))
        ends_map = _odd(rng, LO, HI, n)
        local = lambda q: (q - t) @ R  # noqa: E731  Rᵀ (q − t): exact for an axis rotation and a lattice
        origin, points = local(origin_map), local(ends_map)
        assert is_odd_lattice(origin) and is_odd_lattice(points) and np.array_equal(points @ R.T + t, ends_map)
        how = {"origin": tuple(origin), "min_crossings": rule[0], "min_hits": rule[1], "end_margin": end_margin, "min_range": 0.0,
               "max_range": 1024.0 * m.res if max_range is None else max_range, "dry_run": dry_run}
        rays = [ci.ray(R, t, p, m.res, end_margin, 0.0, how["max_range"], origin) for p in points]
        keep = np.array([r is None or not ci.near_tie(r, m.res) for r in rays])
        return {"op": "carve", "store": store, "points": np.ascontiguousarray(points[keep]), "R": R, "t": t, "how": how,
                "origin_map": origin_map, "drawn": n, "dropped": int((~keep).sum())}

    def carve(self, store, **kw):
        self.emit(self.carve_op(store, **kw))

    def merge(self):
        R, t = _pose(self.rng, self.A.res)
        self.emit({"op": "merge", "R": R, "t": t})

    def merge_empty(self):
        R, t = _pose(self.rng, self.A.res)
        self.emit({"op": "merge_empty", "R": R, "t": t, "res": self.B.res})

    # ------------------------------------------------------------------------------------------- the situations

    def quarter(self):
        """a box prune of A that leaves just more than a quarter of the capacity (when A holds that many)"""
        A = self.A
        if A.cells.shape[0] <= A.capacity // 4:
            return self.box("A", BOXES[0])
        c = np.round(np.median(A.cells, axis=0) * A.res)
        for h in np.arange(0.5, 40.0, 0.5):
            box = (tuple(c), (float(h), float(h), 30.0))
            if int(A.keep_mask(*box).sum()) > A.capacity // 4:
                return self.box("A", box)
        raise AssertionError("no box keeps more than a quarter")

    def carve_shrinks(self):
        """a carve of A after which the survivors fit in a quarter of the capacity: the capacity rule's turn"""
        A = self.A
        around = np.round(np.median(A.cells, axis=0) * A.res) if A.cells.shape[0] else np.zeros(3)
        for attempt in range(8):
            op = self.carve_op("A", rule=(2, 1), end_margin=0.0, around=around, rng=np.random.default_rng([int(self.rng.integers(1 << 30)), attempt]))
            trial = A.clone()
            before = trial.capacity
            removed = trial.carve(op["points"], op["R"], op["t"], **op["how"])[0]
            if removed and trial.capacity < before:
                return self.emit(op)
        raise AssertionError("no carve took the store below a quarter of its capacity")

    def small_box(self):
        before = self.A.capacity
        self.box("A", ((0.0, 0.0, 0.0), (2.0, 2.0, 1.0)))
        assert self.A.capacity < before, "the small box did not shrink the store"

    # ----------------------------------------------------------------------------------------------------- run

    def drawn(self):
        kind = self.names[int(self.rng.choice(len(self.names), p=self.p))]
        store = "B" if kind.endswith("_B") else "A"
        if self.model(store).cells.shape[0] > TOO_MANY:
            return self.box(store, ((0.0, 0.0, 0.0), (5.0, 5.0, 2.0) if self.model(store).res < 1.0 else (10.0, 10.0, 3.0)))
        self.named(kind)

    def named(self, kind):
        {"insert_A": lambda: self.insert("A", full=bool(self.rng.integers(2))), "insert_B": lambda: self.insert("B"),
         "insert_A_small": lambda: self.insert("A", small=True), "insert_A_full": lambda: self.insert("A", full=True),
         "scan_plain": self.scan, "scan_sort": lambda: self.scan(sort_cell=1.0), "scan_filter": lambda: self.scan(filter_voxel=0.5),
         "box_A": lambda: self.box("A"), "box_B": lambda: self.box("B"), "age_A": lambda: self.age("A"), "age_B": lambda: self.age("B"),
         "age_A_0": lambda: self.age("A", 0), "age_A_2": lambda: self.age("A", 2), "age_A_5": lambda: self.age("A", 5),
         "carve_A": lambda: self.carve("A"), "carve_B": lambda: self.carve("B"), "merge": self.merge, "merge_empty": self.merge_empty,
         "quarter_A": self.quarter, "carve_A_shrinks": self.carve_shrinks, "small_box_A": self.small_box,
         "carve_dry": lambda: self.carve("A", dry_run=True),
         "carve_short": lambda: self.carve("A", rule=(2, 1), end_margin=0.0, max_range=4.0)}[kind]()

    def run(self):
        for kind in SCRIPT:
            self.drawn() if kind is None else self.named(kind)
        return self.ops


@functools.lru_cache(maxsize=None)
def program(seed, res_a, res_b, scale=1.0):
    """→ the list of operations; scale < 1 shrinks the batches, not the carves (for the slow definition's small program)"""
    return tuple(_Generator(seed, res_a, res_b, scale).run())
