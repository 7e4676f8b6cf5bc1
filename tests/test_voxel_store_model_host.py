"""The voxel-store model and its programs, without a GPU (tests/voxel_store_model.py, tests/voxel_store_sequences.py;
DESIGN.md §30): the programs contain what they are meant to contain, the model's incremental bookkeeping equals the slow
definition — every operation applied to an explicit list of (point, epoch) pairs, everything recounted from scratch in
fractions.Fraction —, and the programs tell the model from five mutants of it, one planted mistake each."""
import collections
from fractions import Fraction

import numpy as np
import pytest

from tests import voxel_carve_inputs as ci
from tests import voxel_store_sequences as vs
from tests.voxel_store_model import Model, _box_keep, _cells_of, _pack, capacity_after

PROGRAMS = [(seed, ra, rb) for ra, rb in vs.SETUPS for seed in vs.SEEDS]


def _model_of(op, A, B):
    return A if op.get("store", "A") == "A" else B


# ------------------------------------------------------------------------------ 1. what every program contains

@pytest.mark.parametrize("seed,res_a,res_b", PROGRAMS)
def test_a_program_contains_what_it_is_meant_to(seed, res_a, res_b):
    ops = vs.program(seed, res_a, res_b)
    assert 35 <= len(ops) <= 45
    # the lattice conditions
    rotations = [R.tobytes() for R in vs.axis_rotations()]
    for op in ops:
        for key in ("points", "stored", "origin_map"):
            if key in op:
                assert vs.is_odd_lattice(op[key]), (op["op"], key)
        if op["op"] in ("insert", "insert_scan"):
            assert 1500 <= len(op["points"]) <= 4000
            assert np.all(op["points"] >= vs.LO) and np.all(op["points"] < vs.HI)
        if "R" in op:
            res = res_b if op.get("store") == "B" else res_a  # the destination's cells
            shift = op["t"] / res
            assert op["R"].tobytes() in rotations and np.array_equal(shift, np.round(shift)) and np.abs(shift).max() <= 9
        if op["op"] == "carve":
            assert vs.is_odd_lattice(np.asarray(op["how"]["origin"])) and vs.is_odd_lattice(op["points"] @ op["R"].T + op["t"])
            assert 300 <= op["drawn"] <= 600 and len(op["points"]) == op["drawn"] - op["dropped"]
            assert op["dropped"] <= op["drawn"] // 100  # the cap on rays left out
            res = res_b if op["store"] == "B" else res_a
            how = op["how"]
            rays = [ci.ray(op["R"], op["t"], p, res, how["end_margin"], how["min_range"], how["max_range"], how["origin"])
                    for p in op["points"]]
            assert not any(r is not None and ci.near_tie(r, res) for r in rays)
            assert (how["min_crossings"], how["min_hits"]) in vs.CARVE_RULES and how["end_margin"] in (1.5 * res, 0.0)
    # every kind at least twice; the empty merge, the dry run and the short max_range once
    kinds = collections.Counter()
    for op in ops:
        kinds[op["op"] + "_" + op.get("store", "A")] += 1
        if op["op"] == "prune":
            kinds["age" if op["max_age"] is not None else "box"] += 1
        if op["op"] == "insert_scan":
            kinds["scan sort" if op["sort_cell"] else "scan filter" if op["filter_voxel"] else "scan plain"] += 1
    for kind in ("insert_A", "insert_B", "insert_scan_A", "prune_A", "prune_B", "carve_A", "carve_B", "merge_A", "age", "box"):
        assert kinds[kind] >= 2, (kind, kinds)
    assert kinds["scan sort"] >= 1 and kinds["scan filter"] >= 1 and kinds["scan plain"] >= 1
    assert kinds["merge_empty_A"] == 1
    assert sum(op["op"] == "carve" and op["how"]["dry_run"] for op in ops) == 1
    assert sum(op["op"] == "carve" and op["how"]["max_range"] < 100.0 for op in ops) == 1
    assert {op["max_age"] for op in ops if op["op"] == "prune" and op["max_age"] is not None} == {0, 2, 5}
    assert any(op["op"] == "prune" and op["center"] is not None and np.array_equal(np.asarray(op["center"]) * 2, np.round(np.asarray(op["center"]) * 2))
               and np.array_equal(np.asarray(op["half_extent"]) * 2, np.round(np.asarray(op["half_extent"]) * 2)) for op in ops)
    # on the model alone
    A, B = Model(res_a, capacity=0), Model(res_b)
    assert A.capacity == 16
    grown = shrunk = shrunk_by_carve = recreated = age_after_merge = 0
    carved = {"A": set(), "B": set()}
    changed_since_insert = {"A": False, "B": False}  # carved or pruned since its last insert
    merge_after = {"A": 0, "B": 0}
    merge_touched = None
    for step, op in enumerate(ops):
        m, store = _model_of(op, A, B), op.get("store", "A")
        cap, keys_before, stamp_keep = A.capacity, set(m.slot), None
        if op["op"] == "merge":
            for s in "AB":
                merge_after[s] += changed_since_insert[s]
            merge_touched = set(int(k) for k in _pack(_cells_of(A.merge_batch(B, op["R"], op["t"]), A.res)))
        if op["op"] == "prune" and op["max_age"] is not None and store == "A" and merge_touched is not None:
            stamp_keep = A.keep_mask(max_age=op["max_age"])
            keys = [int(k) for k in _pack(A.cells)]
            untouched_gone = any(not keep and k not in merge_touched for k, keep in zip(keys, stamp_keep))
            touched_kept = any(keep and k in merge_touched for k, keep in zip(keys, stamp_keep))
            age_after_merge += untouched_gone and touched_kept
        result = vs.apply(op, A, B)
        assert np.abs(m.live_points()).max(initial=0.0) <= 64
        keys_after = set(m.slot)
        if op["op"] in ("insert", "insert_scan", "merge"):
            recreated += len((keys_after - keys_before) & carved[store])
            carved[store] -= keys_after
            changed_since_insert[store] = False
            if op["op"] != "merge":
                merge_touched = None if store == "A" else merge_touched
        elif op["op"] in ("prune", "carve") and keys_after != keys_before:
            changed_since_insert[store] = True
            if op["op"] == "carve":
                carved[store] |= keys_before - keys_after
        grown += A.capacity > cap
        shrunk += A.capacity < cap
        shrunk_by_carve += A.capacity < cap and op["op"] == "carve"
        assert len(A.cells) <= 6000 and len(B.cells) <= 6000, step
        del result
    print("seed %d (%g, %g): A grew %d times, shrank %d (by a carve %d), %d carved cells recreated, %d age prunes split a merge; "
          "merges after A / B changed: %d / %d; A ends with %d voxels" % (seed, res_a, res_b, grown, shrunk, shrunk_by_carve, recreated,
                                                                        age_after_merge, merge_after["A"], merge_after["B"], len(A.cells)))
    assert grown >= 2 and shrunk >= 1 and shrunk_by_carve >= 1
    assert recreated >= 20
    assert age_after_merge >= 1
    assert merge_after["A"] >= 1 and merge_after["B"] >= 1
    assert len(A.cells) >= 300


def test_capacity_after_is_the_documented_rule():
    assert capacity_after(0, 3, 4096, 16) == 4096  # nothing removed: nothing moves
    assert capacity_after(5, 1025, 4096, 16) == 4096 and capacity_after(5, 1024, 4096, 16) == 2048  # a quarter, inclusive
    assert capacity_after(5, 1023, 4096, 16) == 2048 and capacity_after(5, 513, 4096, 16) == 2048 and capacity_after(5, 512, 4096, 16) == 1024
    assert capacity_after(9, 0, 64, 16) == 16 and capacity_after(9, 3, 64, 16) == 16 and capacity_after(9, 9, 64, 16) == 32
    assert capacity_after(9, 3, 1 << 14, 1 << 14) == 1 << 14 and capacity_after(9, 3, 1 << 15, 1 << 14) == 1 << 14


# ------------------------------------------------------------------------------ 2. the slow definition

class Slow:
    """The definition: the live (point, epoch) pairs and the live cells in slot order, nothing else.  Counts, sums and
    stamps are recounted from the pairs whenever somebody asks."""

    def __init__(self, res):
        self.res, self.epoch, self.order, self.pairs = res, 0, [], []

    def cell(self, p):
        return tuple(int(np.floor(x * (1.0 / self.res))) for x in p)

    def insert(self, pts):
        if len(pts) == 0:
            return 0
        self.epoch += 1
        cells = {self.cell(p) for p in pts}
        self.pairs += [(tuple(float(x) for x in p), self.epoch) for p in pts]
        self.order += sorted(cells - set(self.order))  # tuples sort as the packed key does
        return len(cells)

    def recount(self):
        """→ per live cell in slot order: (count, nine sums as Fractions, stamp)"""
        acc = {c: [0, [Fraction(0)] * 9, 0] for c in self.order}
        for p, epoch in self.pairs:
            x, y, z = (Fraction(v) for v in p)
            a = acc[self.cell(p)]
            a[0] += 1
            a[1] = [s + term for s, term in zip(a[1], (x, y, z, x * x, x * y, x * z, y * y, y * z, z * z))]
            a[2] = max(a[2], epoch)
        return [tuple(acc[c]) for c in self.order]

    def remove(self, gone):
        gone = {c for c, g in zip(self.order, gone) if g}
        self.order = [c for c in self.order if c not in gone]
        self.pairs = [(p, e) for p, e in self.pairs if self.cell(p) not in gone]
        return len(gone)

    def prune(self, center, half_extent, max_age):
        stamps = [s for _, _, s in self.recount()]
        gone = np.zeros(len(self.order), dtype=bool)
        if center is not None:
            gone |= ~_box_keep(np.array(self.order, dtype=np.int64).reshape(-1, 3), center, half_extent, self.res)
        if max_age is not None:
            gone |= np.array([self.epoch - s > max_age for s in stamps], dtype=bool)
        return self.remove(gone)

    def carve(self, points, R, t, origin, min_crossings, min_hits, end_margin, min_range, max_range, dry_run):
        crossings, hits, skipped, _ = ci.counts(np.array(self.order, dtype=np.int64).reshape(-1, 3), R, t, points, self.res, end_margin,
                                                min_range, max_range, origin)
        gone = (crossings >= min_crossings) & (hits < min_hits)
        return (int(gone.sum()) if dry_run else self.remove(gone)), skipped

    def merge(self, src, R, t):
        by_cell = collections.defaultdict(list)
        for p, _ in src.pairs:
            by_cell[src.cell(p)].append(p)
        moved = []
        for c in src.order:  # voxel after voxel; each lands whole in one cell of this grid
            q = np.array(by_cell[c]) @ R.T + t
            assert len({self.cell(x) for x in q}) == 1
            moved.append(q)
        return self.insert(np.concatenate(moved)) if moved else 0


def _slow_apply(op, A, B):
    m = _model_of(op, A, B)
    if op["op"] == "insert":
        return m.insert(op["points"])
    if op["op"] == "insert_scan":
        return A.insert(op["stored"] @ op["R"].T + op["t"])
    if op["op"] == "prune":
        return m.prune(op["center"], op["half_extent"], op["max_age"])
    if op["op"] == "carve":
        return m.carve(op["points"], op["R"], op["t"], **op["how"])
    return A.merge(B if op["op"] == "merge" else Slow(op["res"]), op["R"], op["t"])


def test_the_model_equals_the_slow_definition_after_every_step():
    ops = vs.program(1, 1.0, 0.5, scale=0.08)
    A, B, sA, sB = Model(1.0, capacity=0), Model(0.5), Slow(1.0), Slow(0.5)
    removed_something = 0
    for step, op in enumerate(ops):
        got, want = vs.apply(op, A, B), _slow_apply(op, sA, sB)
        if op["op"] == "carve":
            assert got[:2] == want, (step, op["op"])
            removed_something += got[0] > 0
        else:
            assert got == want, (step, op["op"])
        for m, s in ((A, sA), (B, sB)):
            assert m.epoch == s.epoch and [tuple(int(x) for x in c) for c in m.cells] == s.order, (step, op["op"])
            rows = s.recount()
            assert [int(n) for n in m.counts] == [r[0] for r in rows], (step, op["op"])
            assert [int(x) for x in m.stamp] == [r[2] for r in rows], (step, op["op"])
            assert all(Fraction(float(x)) == f for row, r in zip(m.sums, rows) for x, f in zip(row, r[1])), (step, op["op"])
            assert sorted(map(tuple, m.live_points())) == sorted(p for p, _ in s.pairs), (step, op["op"])
    assert removed_something >= 2 and len(sA.order) > 100 and len(sB.order) > 20


# ------------------------------------------------------------------------------ 3. the programs discriminate

class MergeDoesNotStamp(Model):
    def merge(self, src, R=None, t=None):
        return self.insert(self.merge_batch(src, R, t), stamp=False)


class RecreatedCellKeepsItsPast(Model):
    def _remove(self, keep, shrink=True):
        self.__dict__.setdefault("grave", {}).update({int(k): (int(n), s.copy()) for k, n, s in
                                                      zip(_pack(self.cells[~keep]), self.counts[~keep], self.sums[~keep])})
        return super()._remove(keep, shrink)

    def _start_of(self, key):
        return self.__dict__.get("grave", {}).get(key, (0, np.zeros(9)))


class CarveSortsTheSurvivors(Model):
    def _carve_remove(self, keep):
        removed = self._remove(keep)
        order = np.argsort(_pack(self.cells))
        self.cells, self.counts, self.sums = self.cells[order], self.counts[order], self.sums[order]
        self.stamp, self.birth = self.stamp[order], self.birth[order]
        self.slot = {int(k): s for s, k in enumerate(_pack(self.cells))}
        return removed


class MergeAppendsInSourceOrder(Model):
    def merge(self, src, R=None, t=None):
        self.in_batch_order = True
        try:
            return super().merge(src, R, t)
        finally:
            self.in_batch_order = False

    def _new_cells(self, uniq, first_cells, keys):
        new = super()._new_cells(uniq, first_cells, keys)
        if not self.__dict__.get("in_batch_order") or new.size == 0:
            return new
        _, first_seen = np.unique(keys, return_index=True)  # the batch is in source-voxel order
        return new[np.argsort(first_seen[new], kind="stable")]


class CarveForgetsTheCapacityRule(Model):
    def _carve_remove(self, keep):
        return self._remove(keep, shrink=False)


MUTANTS = (MergeDoesNotStamp, RecreatedCellKeepsItsPast, CarveSortsTheSurvivors, MergeAppendsInSourceOrder, CarveForgetsTheCapacityRule)


@pytest.mark.parametrize("seed,res_a,res_b", PROGRAMS)
def test_every_program_catches_every_mutant(seed, res_a, res_b):
    ops = vs.program(seed, res_a, res_b)
    A, B = Model(res_a, capacity=0), Model(res_b)
    mutants = [(cls(res_a, capacity=0), cls(res_b)) for cls in MUTANTS]
    caught = [None] * len(MUTANTS)
    for step, op in enumerate(ops):
        vs.apply(op, A, B)
        for i, (mA, mB) in enumerate(mutants):
            if caught[i] is None:
                vs.apply(op, mA, mB)
                if (mA.observable(), mB.observable()) != (A.observable(), B.observable()):
                    caught[i] = step
    print("seed %d (%g, %g): first step that differs: %s" % (seed, res_a, res_b, ", ".join(
        "%s %s (%s)" % (cls.__name__, s, ops[s]["op"] if s is not None else "-") for cls, s in zip(MUTANTS, caught))))
    assert all(s is not None for s in caught), caught
