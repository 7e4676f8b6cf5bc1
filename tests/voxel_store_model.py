"""A model of the incremental voxel store (nos_voxel_map_*, api.VoxelMap) for every call that changes it — TEST
INFRASTRUCTURE shared by test_voxel_map_window.py, test_voxel_store_model_host.py (CPU) and test_voxel_store_life.py (GPU).

The contract is the text of include/nos.h.  The model keeps cell → slot and, per slot, count, the nine sums, the stamp and
the epoch of birth, in slot order; every batch that ever went in is kept with its epoch, and a point belongs to a live
voxel iff its cell is live and it arrived at or after that voxel's birth.  Mean and sqrt-information have no bit-exact CPU
form; for EXACT inputs (coordinates that are multiples of 2^-10 with |x| <= 64: every sum is exact in any order, see
test_voxel_map.py::test_exact_inputs_give_the_same_bits_for_any_split) the expected statistics are those of ONE
nos_ndt_map_build over exactly the points the model says its live voxels hold — a path that shares nothing with the
store's merge, prune and compaction.

    insert        a batch: epoch + 1, touched voxels stamped, new cells appended in ascending cell
    insert_scan   an insert of points Rᵀ-rows + t (exact for an axis rotation and lattice points)
    merge         the source model's live points, grouped by source cell, moved by the pose and inserted as ONE batch; every
                  source voxel must land whole in one destination cell (asserted: the exactness condition of nos.h)
    add           the exported state of another model of the same grid: a merge under the identity
    Rejected      raised by any of the four, with nothing changed, when a voxel would pass 2^32 − 1 points
    prune         box and / or age; survivors keep their order, renumbered by rank
    carve         voxel_carve_inputs.counts on the cells in slot order, voxel_carve_inputs.removed, then the prune's removal;
                  epoch and stamps untouched
    capacity      capacity_after is the documented rule of a prune and a carve.  How far an insert GROWS the store the
                  header leaves open ("double as needed"); the model doubles until the voxels before the batch plus the
                  voxels the batch touches fit, which is what the store reserves, and no test holds a device to it."""
import numpy as np

from tests import voxel_carve_inputs as ci

KEYS = ("cells", "counts", "valid", "means", "sqrt_infos")
LIM = 1 << 20
COUNT_MAX = 0xFFFFFFFF  # the points a voxel holds at most


class Rejected(Exception):
    """An insert, a merge or an add would take a voxel past COUNT_MAX points: the call is rejected as a whole and the
    model is as it was.  rows: the positions, in the batch, of the points that fall into such voxels."""

    def __init__(self, rows):
        Exception.__init__(self, "%d points fall into voxels that would pass 2^32 - 1 points" % len(rows))
        self.rows = rows


def _same_bits(a, b, keys=KEYS):
    for key in keys:
        assert np.array_equal(a[key], b[key]), key


def _pack(cells):
    c = cells.astype(np.int64) + LIM
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def _cells_of(points, res):
    return np.floor(points * (1.0 / res)).astype(np.int64)  # the store's own factor: one multiply, then floor


def _box_bounds(center, half, res):
    """The documented rule: floor((c -+ h) * inv_res) in double, clamped to the addressable cells."""
    inv_res = 1.0 / res
    center, half = np.asarray(center, dtype=np.float64), np.broadcast_to(np.asarray(half, dtype=np.float64), (3,))
    lo = np.clip(np.floor((center - half) * inv_res), -LIM, LIM).astype(np.int64)
    hi = np.clip(np.floor((center + half) * inv_res), -LIM - 1, LIM - 1).astype(np.int64)
    return lo, hi


def _box_keep(cells, center, half, res):
    lo, hi = _box_bounds(center, half, res)
    return np.all((cells >= lo) & (cells <= hi), axis=1)


def _pow2_at_least(n, floor=16):
    c = floor
    while c < n:
        c *= 2
    return c


def capacity_after(removed, kept, capacity_before, initial_capacity):
    """The capacity after a prune or a carve that removed `removed` voxels and kept `kept`: when something went and the
    survivors fit in a quarter, the smallest power of two >= 2 * kept, never below 16 nor below the capacity the store was
    created with; otherwise unchanged."""
    if removed and kept <= capacity_before // 4:
        return max(_pow2_at_least(2 * kept), initial_capacity)
    return capacity_before


def _terms(p):
    return np.stack([p[:, 0], p[:, 1], p[:, 2], p[:, 0] * p[:, 0], p[:, 0] * p[:, 1], p[:, 0] * p[:, 2],
                     p[:, 1] * p[:, 1], p[:, 1] * p[:, 2], p[:, 2] * p[:, 2]], axis=1)


class Model:
    """cell → (count, nine sums, stamp), in slot order; every point ever inserted is kept with its insert's epoch, and a
    point belongs to a live voxel iff its cell is live and it arrived at or after that voxel's birth."""

    def __init__(self, res, capacity=0):
        self.res, self.epoch = res, 0
        self.initial_capacity = self.capacity = _pow2_at_least(capacity)
        self.slot = {}  # packed key → slot
        self.cells = np.zeros((0, 3), dtype=np.int64)
        self.counts = np.zeros(0, dtype=np.int64)
        self.sums = np.zeros((0, 9))
        self.stamp = np.zeros(0, dtype=np.int64)
        self.birth = np.zeros(0, dtype=np.int64)
        self.history = []  # (epoch, points, packed keys)

    def clone(self):
        """→ an independent model in the same state (arrays are replaced, never written in place, except by insert)"""
        other = type(self).__new__(type(self))
        other.__dict__.update(self.__dict__)
        other.slot, other.history = dict(self.slot), list(self.history)
        other.counts, other.sums, other.stamp = self.counts.copy(), self.sums.copy(), self.stamp.copy()
        return other

    # ------------------------------------------------------------------------------------------------ what adds

    def _new_cells(self, uniq, first_cells, keys):
        """→ indices into uniq (ascending cell) of the cells the store does not hold, in the order they are appended"""
        return np.array([u for u in range(uniq.size) if int(uniq[u]) not in self.slot], dtype=np.int64)  # ascending cell

    def _start_of(self, key):
        """→ (count, sums [9]) a new voxel of this cell starts from"""
        return 0, np.zeros(9)

    def insert(self, pts, stamp=True):
        if pts.shape[0] == 0:
            return 0
        cells = _cells_of(pts, self.res)
        keys = _pack(cells)
        order = np.argsort(keys, kind="stable")
        uniq, first, n = np.unique(keys[order], return_index=True, return_counts=True)
        # the rule of nos.h: a call that would take a voxel past 2^32 - 1 points is rejected as a whole, nothing changes
        over = [int(k) for k, c in zip(uniq, n) if int(k) in self.slot and int(self.counts[self.slot[int(k)]]) + int(c) > COUNT_MAX]
        if over:
            raise Rejected(np.nonzero(np.isin(keys, over))[0])
        self.epoch += 1
        self.history.append((self.epoch, pts, keys))
        seg = np.add.reduceat(_terms(pts[order]), first, axis=0)
        new = self._new_cells(uniq, cells[order][first], keys)
        V = self.cells.shape[0]
        self.capacity = _pow2_at_least(V + uniq.size, self.capacity)
        start = [self._start_of(int(uniq[u])) for u in new]
        for r, u in enumerate(new):
            self.slot[int(uniq[u])] = V + r
        self.cells = np.concatenate([self.cells, cells[order][first][new]])
        self.counts = np.concatenate([self.counts, np.array([s[0] for s in start], dtype=np.int64)])
        self.sums = np.concatenate([self.sums, np.array([s[1] for s in start]).reshape(-1, 9)])
        self.stamp = np.concatenate([self.stamp, np.zeros(len(new), dtype=np.int64)])
        self.birth = np.concatenate([self.birth, np.full(len(new), self.epoch, dtype=np.int64)])
        slots = np.array([self.slot[int(k)] for k in uniq], dtype=np.int64)
        self.counts[slots] += n
        self.sums[slots] += seg
        if stamp:
            self.stamp[slots] = self.epoch
        return uniq.size

    def insert_scan(self, points, R, t):
        return self.insert(np.asarray(points, dtype=np.float64) @ np.asarray(R, dtype=np.float64).reshape(3, 3).T + np.asarray(t))

    def merge_batch(self, src, R, t):
        """→ the batch a merge of `src` under (R, t) is: its live points voxel after voxel in SOURCE slot order, moved by
        the pose.  A source voxel goes whole to the cell of its transformed mean; an insert of its points agrees with that
        iff they all land in one cell, which is asserted."""
        R, t = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64)
        pts = src.live_points()
        if pts.shape[0] == 0:
            return pts
        at = np.array([src.slot[int(k)] for k in _pack(_cells_of(pts, src.res))], dtype=np.int64)
        order = np.argsort(at, kind="stable")
        pts, at = pts[order], at[order]
        moved = pts @ R.T + t
        first = np.concatenate([[0], np.nonzero(np.diff(at))[0] + 1])
        assert first.size == src.cells.shape[0] and np.array_equal(np.diff(np.append(first, at.size)), src.counts)
        dst_keys = _pack(_cells_of(moved, self.res))
        assert np.array_equal(dst_keys, np.repeat(dst_keys[first], src.counts)), "a source voxel straddles destination cells"
        mean = np.add.reduceat(moved, first, axis=0) / src.counts[:, None]
        assert np.array_equal(_pack(_cells_of(mean, self.res)), dst_keys[first])
        return moved

    def merge(self, src, R=None, t=None):
        """→ destination voxels touched; an empty source is a no-op that leaves the epoch alone"""
        return self.insert(self.merge_batch(src, np.eye(3) if R is None else R, np.zeros(3) if t is None else t))

    def add(self, other):
        """VoxelMap.add of other's exported state: on exact inputs an insert of its live points as one batch, which is
        what a merge under the identity is → voxels touched"""
        assert other.res == self.res
        return self.merge(other)

    # ---------------------------------------------------------------------------------------------- what removes

    def keep_mask(self, center=None, half_extent=None, max_age=None):
        keep = np.ones(self.cells.shape[0], dtype=bool)
        if center is not None:
            keep &= _box_keep(self.cells, center, half_extent, self.res)
        if max_age is not None:
            keep &= (self.epoch - self.stamp) <= max_age
        return keep

    def _remove(self, keep, shrink=True):
        removed = int((~keep).sum())
        self.cells, self.counts, self.sums = self.cells[keep], self.counts[keep], self.sums[keep]
        self.stamp, self.birth = self.stamp[keep], self.birth[keep]
        self.slot = {int(k): s for s, k in enumerate(_pack(self.cells))}
        if shrink:
            self.capacity = capacity_after(removed, self.cells.shape[0], self.capacity, self.initial_capacity)
        return removed

    def prune(self, center=None, half_extent=None, max_age=None):
        return self._remove(self.keep_mask(center, half_extent, max_age))

    def carve(self, points, R, t, origin=(0.0, 0.0, 0.0), min_crossings=2, min_hits=1, end_margin=None, min_range=0.0,
              max_range=None, dry_run=False):
        """→ (removed — with dry_run, the voxels that would go —, skipped, crossings, hits), the counters in the slot
        order before the call"""
        end_margin = 1.5 * self.res if end_margin is None else end_margin
        crossings, hits, skipped, _ = ci.counts(self.cells, R, t, points, self.res, end_margin, min_range, max_range, origin)
        gone = ci.removed(crossings, hits, min_crossings, min_hits)
        removed = int(gone.sum()) if dry_run else self._carve_remove(~gone)
        return removed, skipped, crossings, hits

    def _carve_remove(self, keep):
        return self._remove(keep)

    # ----------------------------------------------------------------------------------------------- what reads

    def live_points(self):
        keys_live = _pack(self.cells)
        order = np.argsort(keys_live)
        out = [np.zeros((0, 3))]
        for epoch, pts, keys in self.history:
            pos = np.searchsorted(keys_live[order], keys)
            pos = np.minimum(pos, max(keys_live.size - 1, 0))
            hit = keys_live[order][pos] == keys if keys_live.size else np.zeros(keys.size, dtype=bool)
            hit &= self.birth[order][pos] <= epoch if keys_live.size else hit
            out.append(pts[hit])
        return np.concatenate(out)

    def observable(self):
        """what a caller can see without the statistics: cells in slot order, counts, len, n_points, epoch, capacity"""
        return (self.cells.tobytes(), self.counts.tobytes(), self.cells.shape[0], int(self.counts.sum()), self.epoch, self.capacity)

    def expected(self, ctx, proper=True):
        """The model's live voxels in slot order with the statistics of a one-shot build over their points (exact inputs)."""
        from nonlinear_optimizer_for_slam_amd import api
        pts = self.live_points()
        assert pts.shape[0] == int(self.counts.sum())
        if pts.shape[0] == 0:
            return {"cells": np.zeros((0, 3), dtype=np.int64), "counts": np.zeros(0, dtype=np.uint32), "valid": np.zeros(0, dtype=bool),
                    "means": np.zeros((0, 3)), "sqrt_infos": np.zeros((0, 3, 3))}
        gm, want = api.NdtMap.build(ctx, pts, self.res, 1.0, proper_sqrt_information=proper)
        gm.close()
        keys = _pack(want["cells"])
        assert np.all(np.diff(keys) > 0) and keys.size == self.cells.shape[0]
        at = np.searchsorted(keys, _pack(self.cells))
        want = {k: want[k][at] for k in KEYS}
        assert np.array_equal(want["cells"], self.cells) and np.array_equal(want["counts"], self.counts)
        ok = want["valid"]  # a voxel below five points gets no mean from the finish
        np.testing.assert_allclose(want["means"][ok], (self.sums[:, :3] / self.counts[:, None])[ok], rtol=0, atol=1e-12)
        return want


def _assert_is_model(ctx, vm, model, proper=True):
    want = model.expected(ctx, proper)
    _same_bits(vm.stats(), want)
    assert len(vm) == model.cells.shape[0] and vm.n_points == int(model.counts.sum())
    assert vm.n_valid == int(want["valid"].sum())
    assert vm.memory()["epoch"] == model.epoch
    return want
