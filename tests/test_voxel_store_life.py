"""The voxel store through seeded programs of ALL its mutating calls — insert, insert_scan, prune by box and by age, carve,
merge — following one another (tests/voxel_store_sequences.py), against the model of tests/voxel_store_model.py after
EVERY operation; DESIGN.md §30.

Three stores run each program: A (16 slots at the start), its twin with room for 2^14 voxels from the start, and B, which
A merges from.  After every operation: the call's return values are the model's (a carve's counters entry for entry);
stats() is bit for bit ONE nos_ndt_map_build over the model's live points, in the model's slot order; len, n_valid,
n_points and the epoch are the model's; the capacity and the generation follow the documented rules; a call that must not
change a store (a dry run, a removal of nothing, the empty merge, the SOURCE of a merge) left its bytes and memory() as they
were; A and its twin hold the same bytes in the same order.  After every fifth operation the live readers on A — match,
match_indexed, score, register6_batch — are compared bit for bit with the same calls on A.snapshot(); at the end
A.match_map(B) is compared with A.match_map(a store built by one insert of B's live points).

Everything is exact (the programs emit odd multiples of 2^-10 under axis poses), so nothing here has a tolerance except
the cost of the final match_map when B's slot order differs from the fresh store's: the same m non-negative terms in
another order, |Δ| <= m · 2^-52 · cost.

Not reachable: NOS_ERR_HIP on a broken store and the probe-error return (the table is never more than half full)."""
import time

import numpy as np
import pytest

from tests import helpers
from tests import voxel_store_sequences as vs
from tests.test_voxel_map_register import _bits, _guard_holds, _same_call
from tests.voxel_store_model import KEYS, Model, _assert_is_model, _pack, _same_bits, capacity_after

pytestmark = pytest.mark.gpu

EXP = ("exponential", 1.0, 1.0)
LOSSES = (None, EXP, ("huber", 0.7))  # those of tests/test_score_batch.py
POSE = (helpers.rot_xyz(0.01, -0.02, 0.05), np.array([0.1, -0.2, 0.05]))
TWIN_CAPACITY = 1 << 14
PROGRAMS = [(seed, ra, rb) for ra, rb in vs.SETUPS for seed in vs.SEEDS]


def _state(vm):
    st = vm.stats()
    return {"bytes": tuple(st[k].tobytes() for k in KEYS), "memory": vm.memory(), "counts": (len(vm), vm.n_valid, vm.n_points)}


def _rows(ds):
    """what the ids of a voxel-indexed dataset name: table()[ids], zeros where the id is -1 → (present [K, n], rows [K, n, 16])"""
    ids, table = ds.ids(), ds.table()
    rows = np.zeros(ids.shape + (16,))
    rows[ids >= 0] = table[ids[ids >= 0]]
    return ids >= 0, rows


def _readers_equal_the_snapshot_route(ctx, api, vm, res, scans, where):
    """match, match_indexed, score and register6_batch on the live store against the same calls on its snapshot → matches"""
    _guard_holds(vm, res)
    before = _state(vm)
    snap = vm.snapshot()
    big = scans[-1]
    total = 0
    for k in (1, 2):
        for dtype in ("f64", "f32"):
            (dl, nl), (ds, ns) = vm.match(big, POSE[0], POSE[1], k, dtype), snap.match(big, POSE[0], POSE[1], k, dtype)
            assert nl == ns, (where, k, dtype)
            assert dl.accumulate6(POSE[0], POSE[1], EXP).tobytes() == ds.accumulate6(POSE[0], POSE[1], EXP).tobytes(), (where, k, dtype)
            total += nl
            dl.close(), ds.close()
            (dl, nl), (ds, ns) = (m.match_indexed(big, POSE[0], POSE[1], k, dtype, sort_by_voxel=False) for m in (vm, snap))
            assert nl == ns, (where, k, dtype)
            (pl, rl), (ps, rs) = _rows(dl), _rows(ds)
            assert np.array_equal(pl, ps) and rl.tobytes() == rs.tobytes(), (where, k, dtype)
            assert dl.accumulate6(POSE[0], POSE[1], EXP).tobytes() == ds.accumulate6(POSE[0], POSE[1], EXP).tobytes(), (where, k, dtype)
            dl.close(), ds.close()
        for loss in LOSSES:
            got, want = vm.score(big, POSE[0], POSE[1], loss, k), snap.score(big, POSE[0], POSE[1], loss, k)
            assert [_bits(x) for x in got] == [_bits(x) for x in want], (where, k, loss, got, want)
    R0, t0 = np.tile(POSE[0].reshape(9), (len(scans), 1)), np.tile(POSE[1], (len(scans), 1))
    _same_call(api.register6_batch(vm, scans, R0, t0, EXP, keep_multiple=4), api.register6_batch(snap, scans, R0, t0, EXP, keep_multiple=4), where)
    snap.close()
    assert _state(vm) == before, where  # the readers leave the store alone
    return total


def _match_map_equals_a_fresh_source(ctx, api, A, B, model_b):
    """A.match_map(B) against A.match_map(one insert of B's live points): B's voxels are the fresh store's, in B's order"""
    fresh = api.VoxelMap(ctx, model_b.res, 1.0)
    live = model_b.live_points()
    fresh.insert(live)
    sb, sf = B.stats(), fresh.stats()
    assert len(sb["cells"]) == len(sf["cells"]) == model_b.cells.shape[0]
    at = np.searchsorted(_pack(sf["cells"]), _pack(sb["cells"]))  # a fresh store's cells ascend
    _same_bits(sb, {k: sf[k][at] for k in KEYS})
    (db, nb), (df, nf) = A.match_map(B, POSE[0], POSE[1], 2, "f64"), A.match_map(fresh, POSE[0], POSE[1], 2, "f64")
    assert nb == nf
    rb, rf = api.download(db), api.download(df)
    same_order = np.array_equal(at, np.arange(at.size))
    if same_order:
        assert rb.tobytes() == rf.tobytes()
    else:  # slots 2v and 2v + 1 belong to source voxel v: the same records under the permutation of the voxels …
        slots = np.stack([2 * at, 2 * at + 1], axis=1).reshape(-1)
        assert rb.shape == rf.shape and rb.shape[-1] >= 2 * at.size, (rb.shape, at.size)
        assert np.ascontiguousarray(rb[..., :2 * at.size]).tobytes() == np.ascontiguousarray(rf[..., slots]).tobytes()
        # … and sums that differ by the order of the same nb non-negative terms alone
        for loss in (None, EXP):
            cb, cf = db.accumulate6(POSE[0], POSE[1], loss)[27], df.accumulate6(POSE[0], POSE[1], loss)[27]
            assert abs(cb - cf) <= nb * 2.0 ** -52 * cf, (loss, cb, cf)
    print("match_map: %d source voxels, %d matches, slot order %s" % (at.size, nb, "equal" if same_order else "differs"))
    for h in (db, df, fresh):
        h.close()
    return nb


@pytest.mark.parametrize("seed,res_a,res_b", PROGRAMS)
def test_the_stores_equal_the_model_after_every_operation(ctx, seed, res_a, res_b):
    from nonlinear_optimizer_for_slam_amd import api
    started = time.perf_counter()
    ops = vs.program(seed, res_a, res_b)
    generated = time.perf_counter() - started
    rng = np.random.default_rng(1000 + seed)
    scans = [api.Scan(ctx, rng.uniform(vs.LO, vs.HI, size=(n, 3))) for n in (1, 63, 513)]
    stores = {"A": api.VoxelMap(ctx, res_a, 1.0, capacity=0), "twin": api.VoxelMap(ctx, res_a, 1.0, capacity=TWIN_CAPACITY),
              "B": api.VoxelMap(ctx, res_b, 1.0)}
    models = {"A": Model(res_a, capacity=0), "B": Model(res_b)}
    initial = {name: vm.memory()["capacity"] for name, vm in stores.items()}
    assert initial["A"] == 16 and initial["twin"] == TWIN_CAPACITY
    last = {name: _state(vm) for name, vm in stores.items()}
    grown = shrunk = shrunk_by_carve = matched = 0
    to_close = []

    def run(op, name):
        """one operation on the store `name` → (what the model's call returns, or its first entries; for a carve the info)"""
        vm, kind = stores[name], op["op"]
        if kind == "insert":
            return vm.insert(op["points"]), None
        if kind == "insert_scan":
            return vm.insert_scan(op["scan"], op["R"], op["t"]), None
        if kind == "prune":
            return vm.prune(center=op["center"], half_extent=op["half_extent"], max_age=op["max_age"]), None
        if kind == "carve":
            return vm.carve(op["scan"], op["R"], op["t"], counts=True, **op["how"])
        return vm.merge(stores["B"] if kind == "merge" else op["empty"], op["R"], op["t"]), None

    for step, op in enumerate(ops):
        op, kind = dict(op), op["op"]
        where = (step, kind, op.get("store", "A"))
        names = ("B",) if op.get("store") == "B" else ("A", "twin")
        model = models[names[0]]
        if kind == "insert_scan":
            op["scan"] = api.Scan(ctx, op["points"], sort_cell=op["sort_cell"], filter_voxel=op["filter_voxel"])
            op["stored"] = op["scan"].points()  # what the device holds goes to the model; the program's prediction is its set
            assert sorted(map(tuple, op["stored"])) == sorted(map(tuple, ops[step]["stored"])), where
            if not op["sort_cell"]:
                assert np.array_equal(op["stored"], ops[step]["stored"]), where
        elif kind == "carve":
            op["scan"] = api.Scan(ctx, op["points"])
        elif kind == "merge_empty":
            op["empty"] = api.VoxelMap(ctx, op["res"], 1.0)
        to_close += [op[k] for k in ("scan", "empty") if k in op]
        want = vs.apply(op, models["A"], models["B"])
        for name in names:
            vm, before = stores[name], last[name]
            got, info = run(op, name)
            now = _state(vm)
            removes = kind in ("prune", "carve")
            # return values
            if kind == "carve":
                assert (got, info["skipped"]) == want[:2], (where, name, got, info["skipped"], want[:2])
                assert np.array_equal(info["crossings"], want[2]) and np.array_equal(info["hits"], want[3]), (where, name)
            else:
                assert got == want, (where, name, got, want)
            really_removed = got if removes and not (kind == "carve" and op["how"]["dry_run"]) else 0
            # the store is the model
            if name != "twin":
                expected = _assert_is_model(ctx, vm, model)
            else:
                assert now["bytes"] == last["A"]["bytes"] and now["counts"] == last["A"]["counts"], where
                assert now["memory"]["epoch"] == last["A"]["memory"]["epoch"], where
            assert now["counts"] == (model.cells.shape[0], int(expected["valid"].sum()), int(model.counts.sum())), where
            assert now["memory"]["epoch"] == model.epoch, where
            # capacity
            cap0, cap1 = before["memory"]["capacity"], now["memory"]["capacity"]
            if removes:
                assert cap1 == capacity_after(really_removed, now["counts"][0], cap0, initial[name]), (where, name, cap0, cap1)
            else:
                assert cap1 >= now["counts"][0] and cap1 >= cap0, (where, name, cap0, cap1)
            # generation
            gen0, gen1 = before["memory"]["generation"], now["memory"]["generation"]
            if really_removed:
                assert gen1 == gen0 + 1, (where, name)
            elif cap1 > cap0:
                assert gen1 >= gen0 + 1, (where, name)
            else:
                assert gen1 == gen0, (where, name)
            # what must not change
            if (removes and not really_removed) or kind == "merge_empty":
                assert now == before, (where, name)
            if name == "A":
                grown += cap1 > cap0
                shrunk += cap1 < cap0
                shrunk_by_carve += cap1 < cap0 and kind == "carve"
            last[name] = now
        if kind == "merge":
            assert _state(stores["B"]) == last["B"], where  # the source, memory() included
        if step % 5 == 4 or step == len(ops) - 1:
            matched += _readers_equal_the_snapshot_route(ctx, api, stores["A"], res_a, scans, where)
    assert grown >= 2 and shrunk >= 1 and shrunk_by_carve >= 1, (grown, shrunk, shrunk_by_carve)  # the device went where the model went
    assert matched > 1000 and len(stores["A"]) >= 300
    assert _match_map_equals_a_fresh_source(ctx, api, stores["A"], stores["B"], models["B"]) > 0
    for h in to_close + scans + list(stores.values()):
        h.close()
    print("seed %d (%g, %g): %d operations, A %d voxels, B %d; A grew %d times, shrank %d (by a carve %d); program %.2f s, "
          "all of it %.2f s" % (seed, res_a, res_b, len(ops), models["A"].cells.shape[0], models["B"].cells.shape[0], grown, shrunk,
                                shrunk_by_carve, generated, time.perf_counter() - started))
