"""The voxel store at its two 32-bit limits, on the GPU (inputs and models: tests/voxel_limit_inputs.py).

A voxel holds at most 2^32 − 1 points: insert, insert_scan, merge and add accept a call that lands exactly on that
count and reject, as a whole, one that would pass it — the store is then bit for bit what it was.  Stamps are the low
32 bits of the epoch: ages, the window of the odometry, paging and files are followed across epoch 2^32 against the
shared model, which keeps 64-bit stamps.

1. landing on the limit and one point more, for every mutator; 2. the full voxel, 64-bit point totals; 3. readers at huge
counts; 4. across the stamp wrap; 5. the odometry's window across it; 6. the tally of an insert and a merge."""
import ctypes
import re

import numpy as np
import pytest

from tests import voxel_inputs as vi
from tests import voxel_limit_inputs as li
from tests import voxel_store_sequences as vs
from tests.voxel_store_model import Model, Rejected, _assert_is_model, _cells_of, _pack

pytestmark = pytest.mark.gpu

RES = 1.0
UNSUPPORTED = 6
EXP = ("exponential", 1.0, 1.0)
ROT_Z = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])  # an exact axis rotation
COUNT_MAX = li.COUNT_MAX


def _same_state(got, want, where=None):
    for k in li.STATE_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (where, k)
        assert np.array_equal(got[k], want[k]), (where, k)
    assert got["epoch"] == want["epoch"], where


def _visible(vm):
    """everything a rejected call must leave as it was (memory()'s capacity, bytes and generation aside)"""
    st, ex = vm.stats(), vm.export()
    return (tuple(st[k].tobytes() for k in ("cells", "counts", "valid", "means", "sqrt_infos")),
            tuple(ex[k].tobytes() for k in li.STATE_KEYS), ex["epoch"], len(vm), vm.n_valid, vm.n_points, vm.memory()["epoch"])


def _batch(state, seed, brim_points):
    """A shuffled lattice batch: brim_points[slot] = (a, b) points in two opposite octants of that voxel's cell (two
    voxels of a grid of half the edge), 3 points in each of the 40 ordinary cells of slots 10 … 49, 4 in each of 10 cells
    the state does not hold → (points, the packed cells of the brim slots)"""
    rng = np.random.default_rng(seed)
    res = state["voxel_resolution"]
    parts = []
    for slot, (a, b) in brim_points.items():
        cell = state["cells"][slot].astype(np.float64)
        parts.append((cell + rng.integers(1, 512, size=(a, 3)) / 1024.0) * res)
        parts.append((cell + rng.integers(513, 1024, size=(b, 3)) / 1024.0) * res)
    for slot in range(10, 50):
        parts.append(li.lattice_points(rng, state["cells"][slot], 3, res))
    for slot in range(10):
        parts.append(li.lattice_points(rng, state["cells"][slot] + [0, 0, 7], 4, res))
    held = set(_pack(state["cells"]).tolist())
    assert not held & set(_pack(state["cells"][:10] + [0, 0, 7]).tolist())
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))], _pack(state["cells"][list(brim_points)])


class _Mutator:
    """One way of bringing a lattice batch into a store.  run(vm, pts) → voxels touched; afterwards named(index) → the
    packed destination cell of what an error message names by `index`."""

    def __init__(self, ctx, kind):
        self.ctx, self.kind, self.held = ctx, kind, []

    def run(self, vm, pts):
        from nonlinear_optimizer_for_slam_amd import api
        kind, ctx = self.kind, self.ctx
        if kind == "insert":
            self.named = lambda i: _pack(_cells_of(pts[i:i + 1], RES))[0]
            return vm.insert(pts)
        if kind.startswith("insert_scan"):
            R, t = (np.eye(3), np.zeros(3)) if kind == "insert_scan" else (ROT_Z, np.array([3.0, -2.0, 1.0]) * RES)
            # a cell-sorted scan under the identity: the message must name the ORIGINAL index (Scan.order)
            scan = api.Scan(ctx, (pts - t) @ R, sort_cell=2.0 * RES if kind == "insert_scan" else None)
            self.held.append(scan)
            if kind == "insert_scan":
                assert not np.array_equal(scan.order, np.arange(len(pts)))
            self.named = lambda i: _pack(_cells_of(pts[i:i + 1], RES))[0]
            return vm.insert_scan(scan, R, t)
        if kind.startswith("merge"):
            shift = np.array([3.0, -3.0, 3.0]) * RES if kind == "merge_shifted" else np.zeros(3)
            src = api.VoxelMap(ctx, RES / 2 if kind == "merge_finer" else RES, 1.0)
            self.held.append(src)
            src.insert(pts - shift)
            cells = src.export()["cells"]
            if kind == "merge_finer":
                self.named = lambda i: _pack(np.floor_divide(cells[i:i + 1], 2))[0]
            else:
                self.named = lambda i: _pack(cells[i:i + 1] + (shift / RES).astype(np.int64))[0]
            return vm.merge(src, np.eye(3), shift)
        assert kind == "add"
        src = api.VoxelMap(ctx, RES, 1.0)
        self.held.append(src)
        src.insert(pts)
        state = src.export()
        self.named = lambda i: _pack(state["cells"][i:i + 1])[0]
        return vm.add(state)

    def close(self):
        for h in self.held:
            h.close()
        self.held = []


MUTATORS = ("insert", "insert_scan", "insert_scan_rotated", "merge", "merge_shifted", "merge_finer", "add")
TARGETS = {"lane_255": (255,), "lane_0_of_block_1": (256,), "both": (255, 256)}


# ------------------------------------------------------------------- 1. landing on the limit, and one point more

@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("kind", MUTATORS)
def test_landing_on_the_count_limit_is_accepted_and_one_point_more_is_rejected(ctx, kind, target):
    """Slots 255 and 256 hold 2^32 − 8 points.  7 more (3 + 4, two source voxels for the merge from the finer grid: neither
    is near the limit, only run + destination is) land on 2^32 − 1: accepted, export() is the integer arithmetic.  8 more
    (3 + 5): NOS_ERR_UNSUPPORTED, nothing changed — not the brim voxel, not the 40 ordinary and the 10 new cells of the
    batch —, the message names a member of the batch in the brim cell, and the batch without those points goes in."""
    from nonlinear_optimizer_for_slam_amd import api
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    slots = TARGETS[target]
    state = li.brim_state(RES)
    how = _Mutator(ctx, kind)
    try:
        # ---- accepted
        vm = api.VoxelMap.from_state(ctx, state)
        before_points = vm.n_points
        assert before_points == int(state["counts"].astype(np.uint64).sum())
        pts, brim_keys = _batch(state, 7, {s: (3, 4) for s in slots})
        want = li.apply_batch(state, pts)
        touched = how.run(vm, pts)
        got = vm.export()
        assert [int(got["counts"][s]) for s in slots] == [COUNT_MAX] * len(slots), got["counts"][list(slots)]
        _same_state(got, want, "accepted")
        assert touched == len(slots) + 50 and len(vm) == 310
        assert all(int(got["stamps"][s]) == got["epoch"] == state["epoch"] + 1 for s in slots)
        assert vm.n_points == before_points + len(pts) == int(got["counts"].astype(np.uint64).sum())
        st = vm.stats()
        for s in slots:
            ref = li.finish_xp(COUNT_MAX, got["sums"][s], got["cells"][s], RES)
            assert ref["valid"] and bool(st["valid"][s]) and int(st["counts"][s]) == COUNT_MAX
            e_mean, e_eig, e_ortho, e_info, gap = li.finish_errors(ref, st["means"][s], st["sqrt_infos"][s], True)
            print("%s, slot %d at 2^32 - 1 points: mean %.2f ulp, eigenvalues %.1e, information %.1e" % (kind, s, e_mean, e_eig, e_info))
            assert e_mean <= vi.MEAN_ULPS and e_eig <= vi.EIG_RTOL and e_ortho <= vi.ORTHO_TOL and e_info <= vi.INFO_RTOL + gap
        vm.close()
        how.close()
        # ---- rejected
        vm = api.VoxelMap.from_state(ctx, state)
        pts, brim_keys = _batch(state, 8, {s: (3, 5) for s in slots})
        with pytest.raises(Rejected) as model_says:
            li.apply_batch(state, pts)
        assert len(model_says.value.rows) == 8 * len(slots)
        before, memory = _visible(vm), vm.memory()
        _same_state(vm.export(), state, "restored")
        error = None
        try:
            how.run(vm, pts)
        except NosError as e:
            error = e
        _same_state(vm.export(), state, "export() after a %s that had to be rejected" % kind)  # first: what a wrapped count shows in
        assert error is not None and error.status == UNSUPPORTED, error
        assert "2^32 - 1 points" in str(error), str(error)
        assert _visible(vm) == before, "a rejected %s changed the store" % kind
        if kind == "insert":  # *n_touched is unwritten
            n = ctypes.c_size_t(12345)
            rc = vm._lib.nos_voxel_map_insert(vm._h, len(pts), pts.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(n))
            assert rc == UNSUPPORTED and n.value == 12345 and _visible(vm) == before
        if kind == "add":  # the add's own check runs ahead of the reservation
            assert vm.memory() == memory
        index = int(re.search(r"(?:point|voxel) (\d+)", str(error)).group(1))
        assert how.named(index) in brim_keys, (index, str(error))
        how.close()
        # ---- the next call, the same batch without the offending points
        rest = np.delete(pts, model_says.value.rows, axis=0)
        want = li.apply_batch(state, rest)
        assert how.run(vm, rest) == 50
        _same_state(vm.export(), want, "after the rejection")
        assert vm.n_points == before_points + len(rest) and len(vm) == 310
        vm.close()
    finally:
        how.close()


# ----------------------------------------------------------------------- 2. the full voxel, 64-bit point totals

def test_the_full_voxel_takes_nothing_and_leaves_with_all_its_points(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    state = li.brim_state(RES)
    state["stamps"] = state["stamps"].copy()
    state["stamps"][3] = state["epoch"] - 15  # the only voxel older than 10 inserts
    rng = np.random.default_rng(9)
    cell = state["cells"][3]
    vm = api.VoxelMap.from_state(ctx, state)
    total = int(state["counts"].astype(np.uint64).sum())
    assert int(state["counts"][3]) == COUNT_MAX and vm.n_points == total > 3 * (1 << 32)
    around, _ = _batch(state, 21, {})
    one = np.concatenate([around, li.lattice_points(rng, cell, 1, RES)])
    src = api.VoxelMap(ctx, RES, 1.0)
    src.insert(one)
    scan = api.Scan(ctx, one)
    before = _visible(vm)
    for name, call in (("insert", lambda: vm.insert(one)), ("insert_scan", lambda: vm.insert_scan(scan, np.eye(3), np.zeros(3))),
                       ("merge", lambda: vm.merge(src)), ("add", lambda: vm.add(src.export()))):
        error = None
        try:
            call()
        except NosError as e:
            error = e
        _same_state(vm.export(), state, "export() after a %s into the full voxel" % name)
        assert error is not None and error.status == UNSUPPORTED, (name, error)
        assert _visible(vm) == before, name
    want = li.apply_batch(state, around)
    assert vm.insert(around) == 50  # a batch around it
    _same_state(vm.export(), want, "around the full voxel")
    assert vm.n_points == total + len(around)
    # a prune that removes it: the removed points are one 64-bit total
    twin = api.VoxelMap.from_state(ctx, want)
    assert vm.prune(max_age=11) == 1 and vm.n_points == total + len(around) - COUNT_MAX
    assert not (_pack(vm.export()["cells"]) == _pack(cell[None])[0]).any()
    assert int(vm.export()["counts"].astype(np.uint64).sum()) == vm.n_points
    # a carve that removes it: three rays straight up through its cell from two cells below to three above
    centre = (cell + 0.5) * RES
    origin = centre - [0.0, 0.0, 2.0 * RES]
    ends = centre + np.array([[0.0, 0.0, 3.0], [0.01, 0.0, 3.0], [0.0, 0.01, 3.0]]) * RES
    rays = api.Scan(ctx, ends)
    had = twin.export()
    removed, _ = twin.carve(rays, np.eye(3), np.zeros(3), origin=origin)
    left = twin.export()
    gone = ~np.isin(_pack(had["cells"]), _pack(left["cells"]))
    assert removed == int(gone.sum()) >= 1 and gone[3]
    assert twin.n_points == total + len(around) - int(had["counts"][gone].astype(np.uint64).sum()) < total + len(around) - COUNT_MAX + 200
    for h in (vm, twin, src, scan, rays):
        h.close()


def test_a_store_of_more_than_2_to_the_33_points_reports_their_number(ctx, tmp_path):
    from nonlinear_optimizer_for_slam_amd import api
    state = li.brim_state(RES, brim={3: 0, 255: 0, 256: 0, 299: 1 << 31})
    total = sum(int(c) for c in state["counts"])
    assert total > (1 << 33)
    vm = api.VoxelMap.from_state(ctx, state)
    got = vm.export()
    assert vm.n_points == total == sum(int(c) for c in got["counts"])
    _same_state(got, state)
    back = api.VoxelMap.from_state(ctx, got)
    assert back.n_points == total and back.n_valid == vm.n_valid == 300
    path = tmp_path / "huge.npz"
    vm.save(path)
    loaded = api.VoxelMap.load(ctx, path)
    assert loaded.n_points == total
    _same_state(loaded.export(), state)
    for h in (vm, back, loaded):
        h.close()


# ---------------------------------------------------------------------------------------- 3. readers at huge counts

def test_readers_do_not_see_the_count_but_for_the_ray_casts_threshold(ctx):
    """The brim store against its twin: the four huge counts replaced by 1000 points with the same mean and (to rounding)
    the same covariance.  stats() at those voxels agree to the bounds every finish is held to (each is within them of
    the truth: twice the bound between the two), everywhere else bit for bit; match and score count the same matches and
    the costs agree to 4 x INFO_RTOL (a cost term is at most linear in the information matrix; twice the two-sided bound);
    register6_batch ends within 1e-5 of the twin's pose (both stop at a parameter tolerance of 1e-6).  Where the
    statistics happen to be bit-equal, so is everything.  raycast(min_points=2^31) sees exactly the voxels of at least
    2^31 points: an unsigned compare."""
    from nonlinear_optimizer_for_slam_amd import api
    brim_state, twin_state = li.brim_state(RES), li.brim_state(RES, ordinary=1000)
    brim, twin = api.VoxelMap.from_state(ctx, brim_state), api.VoxelMap.from_state(ctx, twin_state)
    a, b = brim.stats(), twin.stats()
    huge = np.zeros(300, dtype=bool)
    huge[list(li.BRIM)] = True
    assert a["valid"].all() and b["valid"].all() and brim.n_valid == twin.n_valid == 300
    for k in ("cells", "valid", "means", "sqrt_infos"):
        assert np.array_equal(a[k][~huge], b[k][~huge]), k
    for s in li.BRIM:
        ref = li.finish_xp(brim_state["counts"][s], brim_state["sums"][s], brim_state["cells"][s], RES)
        for name, st in (("brim", a), ("twin", b)):
            e_mean, e_eig, e_ortho, e_info, gap = li.finish_errors(ref, st["means"][s], st["sqrt_infos"][s], True)
            print("slot %d, %s (%d points): mean %.2f ulp, eigenvalues %.1e, information %.1e" % (s, name, int(st["counts"][s]), e_mean, e_eig, e_info))
            assert e_mean <= vi.MEAN_ULPS and e_eig <= vi.EIG_RTOL and e_ortho <= vi.ORTHO_TOL and e_info <= vi.INFO_RTOL + gap
    same_bits = all(np.array_equal(a[k], b[k]) for k in ("means", "sqrt_infos"))
    # a scan of the voxels' own neighbourhoods, the brim voxels among them
    rng = np.random.default_rng(3)
    rows = np.concatenate([list(li.BRIM), rng.choice(300, size=96, replace=False)])
    pts = (brim_state["cells"][rows] + rng.uniform(0.1, 0.9, size=(len(rows), 3))) * RES
    scan = api.Scan(ctx, np.repeat(pts, 3, axis=0) + rng.normal(scale=0.02, size=(3 * len(rows), 3)))
    R, t = np.eye(3), np.array([0.02, -0.01, 0.01])
    (da, na), (db, nb) = brim.match(scan, R, t), twin.match(scan, R, t)
    assert na == nb > len(rows)
    sa, sb = brim.score(scan, R, t, EXP), twin.score(scan, R, t, EXP)
    assert sa[:2] == sb[:2] and abs(sa[2] - sb[2]) <= 4.0 * vi.INFO_RTOL * abs(sb[2]), (sa, sb)
    Ra, ta, repa = api.register6_batch(brim, [scan], R, t, EXP)
    Rb, tb, repb = api.register6_batch(twin, [scan], R, t, EXP)
    assert repa[0]["ok"] and repb[0]["ok"]
    assert np.abs(Ra - Rb).max() <= 1e-5 and np.abs(ta - tb).max() <= 1e-5, (ta, tb)
    if same_bits:
        assert api.download(da).tobytes() == api.download(db).tobytes() and sa == sb
        assert Ra.tobytes() == Rb.tobytes() and ta.tobytes() == tb.tobytes() and repa == repb
    print("brim against twin: statistics %s, cost %.17g against %.17g, |dt| %.1e" %
          ("bit-equal" if same_bits else "equal to rounding", sa[2], sb[2], np.abs(ta - tb).max()))
    da.close(), db.close()
    # the ray cast: one beam at every voxel's mean from far above
    origin = np.array([0.0, 0.0, 40.0])
    beams = api.Scan(ctx, a["means"] - origin)
    for min_points, want in ((1 << 31, {3, 255, 256}), ((1 << 31) - 1, {3, 255, 256, 299}), (COUNT_MAX, {3}), (COUNT_MAX - 7, {3, 255, 256})):
        voxels, _, info = brim.raycast(beams, np.eye(3), origin, max_range=80.0, min_points=min_points)
        assert set(voxels[voxels >= 0].tolist()) == want, (min_points, sorted(set(voxels.tolist())))
        assert all(voxels[s] == s for s in want) and info["hits"] >= len(want)
        voxels, _, _ = twin.raycast(beams, np.eye(3), origin, max_range=80.0, min_points=min_points)
        assert (voxels == -1).all()
    for h in (brim, twin, scan, beams):
        h.close()


# ---------------------------------------------------------------------------------------- 4. across the stamp wrap

AGES = (0, 1, 4, 9)


def _check_ages(ctx, vm, model, clone_prune):
    from nonlinear_optimizer_for_slam_amd import api
    st = vm.export()
    assert vm.memory()["epoch"] == model.epoch == st["epoch"]
    assert np.array_equal(st["stamps"], (model.stamp & 0xFFFFFFFF).astype(np.uint32))
    for age in AGES:
        keep = model.keep_mask(max_age=age)
        kept, removed = vm.export(max_age=age), vm.export(max_age=age, removed=True)
        assert np.array_equal(kept["cells"], model.cells[keep]) and np.array_equal(removed["cells"], model.cells[~keep]), age
        assert np.array_equal(kept["stamps"], st["stamps"][keep]) and np.array_equal(removed["counts"], st["counts"][~keep]), age
        if clone_prune:
            clone, m = api.VoxelMap.from_state(ctx, st), model.clone()
            assert clone.prune(max_age=age) == m.prune(max_age=age) == int((~keep).sum())
            assert np.array_equal(clone.export()["cells"], m.cells) and clone.memory()["epoch"] == model.epoch
            clone.close()
    for age in ((1 << 32) - 1, 1 << 32, 1 << 40):  # every live voxel is younger than 2^32 inserts
        assert len(vm.export(max_age=age)["counts"]) == len(vm) and len(vm.export(max_age=age, removed=True)["counts"]) == 0


def test_ages_stay_exact_across_the_stamp_wrap(ctx, tmp_path):
    """A store and its model built by three inserts, moved to epoch 2^32 − 2 (shifted, restore), then ten steps across
    2^32: insert, insert_scan, merge, a real prune(max_age=3) at epoch 2^32 + 1 with what it removes paged out, the add of
    the cache's take.  After every step the epoch is the model's 64-bit one, the stamps its low 32 bits, the kept and
    removed sets of four ages the model's, and the statistics those of a build over the model's live points."""
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    rng = np.random.default_rng(17)
    lo, hi = np.array([-4.0, -4.0, -2.0]), np.array([4.0, 4.0, 2.0])

    def points(n, part):  # part of the region along x, so that voxels differ in age
        a, b = part
        return vs._odd(rng, [lo[0] + a * 8.0, lo[1], lo[2]], [lo[0] + b * 8.0, hi[1], hi[2]], n)

    small, model0 = api.VoxelMap(ctx, RES, 1.0), Model(RES)
    for part in ((0.0, 0.5), (0.25, 0.75), (0.5, 1.0)):
        p = points(400, part)
        small.insert(p), model0.insert(p)
    state, model = li.shifted(small.export(), model0, (1 << 32) - 5)
    assert state["epoch"] == (1 << 32) - 2 == model.epoch and state["stamps"].max() == 0xFFFFFFFE
    vm = api.VoxelMap.from_state(ctx, state)
    _check_ages(ctx, vm, model, True)
    _assert_is_model(ctx, vm, model)
    cache, paged_points, held = pipeline.TileCache(4), None, []
    steps = ("insert", "insert_scan", "merge", "prune", "insert", "add", "insert_scan", "merge", "insert", "insert")
    for k, step in enumerate(steps):
        part = ((k % 3) * 0.25, (k % 3) * 0.25 + 0.5)
        if step == "insert":
            p = points(150, part)
            assert vm.insert(p) == model.insert(p)
        elif step == "insert_scan":
            R, t = ROT_Z, np.array([1.0, -1.0, 0.0]) * RES
            p = points(150, part)
            scan = api.Scan(ctx, (p - t) @ R)
            held.append(scan)
            assert vm.insert_scan(scan, R, t) == model.insert_scan((p - t) @ R, R, t)
        elif step == "merge":
            src, src_model = api.VoxelMap(ctx, RES, 1.0), Model(RES)
            held.append(src)
            p = points(150, part)
            src.insert(p), src_model.insert(p)
            shift = np.array([0.0, 1.0, 0.0]) * RES
            assert vm.merge(src, np.eye(3), shift) == model.merge(src_model, np.eye(3), shift)
        elif step == "prune":
            assert model.epoch == (1 << 32) + 1
            keep = model.keep_mask(max_age=3)
            assert 0 < int((~keep).sum()) < len(keep)
            gone = model.clone()
            gone._remove(~keep)
            paged_points = gone.live_points()
            assert cache.put(vm.export(max_age=3, removed=True)) == int((~keep).sum())
            assert vm.prune(max_age=3) == model.prune(max_age=3) == int((~keep).sum())
        else:
            assert step == "add" and model.epoch == (1 << 32) + 2
            paged = cache.take_all()
            assert paged["epoch"] == (1 << 32) + 1
            assert vm.add(paged) == model.insert(paged_points)
            assert model.epoch == (1 << 32) + 3
            path = tmp_path / "wrapped.npz"
            vm.save(path)
            back = api.VoxelMap.load(ctx, path)
            _same_state(back.export(), vm.export(), "save and load at epoch 2^32 + 3")
            assert back.memory()["epoch"] == (1 << 32) + 3
            back.close()
        _check_ages(ctx, vm, model, clone_prune=k in (1, 2, 5))
        _assert_is_model(ctx, vm, model)
    assert model.epoch == (1 << 32) + 7 and (model.stamp > (1 << 32)).any() and (model.stamp < (1 << 32)).any()
    for h in held + [vm, small]:
        h.close()


# ---------------------------------------------------------------------------- 5. the odometry's window across the wrap

def _world(rng, n, centre):
    xy = rng.uniform(-6.0, 6.0, size=(n, 2)) + centre[:2]
    z = 0.45 * np.sin(xy[:, 0] * 0.9) + 0.35 * np.cos(xy[:, 1] * 0.7) - 1.5
    floor = np.column_stack([xy, z + rng.normal(scale=0.02, size=n)])
    wall = np.column_stack([xy[:, 0], 4.0 + 0.3 * np.sin(1.1 * xy[:, 0]), rng.uniform(-1.5, 2.0, size=n)])
    rib = np.column_stack([np.round(xy[:, 0]) + 0.5, xy[:, 1], rng.uniform(-1.5, 2.0, size=n)])
    return np.concatenate([floor, wall[:n // 2], rib[:n // 2]])


def test_the_odometry_window_does_not_see_the_stamp_wrap(ctx):
    """Six frames of 300 points with max_voxel_age=2 and a tile cache, from a store restored at epoch 2^32 − 3 and from
    the same store at epoch 3: poses and rounds bit for bit, and stores that differ in the epoch and — by the shift
    mod 2^32 — in the stamps alone."""
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    rng = np.random.default_rng(23)
    first = api.VoxelMap(ctx, RES, 1.0)
    for _ in range(3):
        first.insert(_world(rng, 3000, np.zeros(3)))
    state = first.export()
    assert state["epoch"] == 3
    shift = (1 << 32) - 6
    late, _ = li.shifted(state, Model(RES), shift)
    assert late["epoch"] == (1 << 32) - 3
    clouds = []
    for k in range(6):
        t = np.array([0.2 * k, 0.0, 0.0])
        near = _world(rng, 400, t)
        clouds.append(near[rng.choice(len(near), size=300, replace=False)] - t)

    def run(st):
        vm = api.VoxelMap.from_state(ctx, st)
        scans = [api.Scan(ctx, c) for c in clouds]
        cache = pipeline.TileCache(4)
        poses, rounds = pipeline.odometry(ctx, vm, scans, loss=EXP, window_half_extent=(5.0, 5.0, 3.0), max_voxel_age=2, tiles=cache)
        out = vm.export()
        cached = cache.take_all()
        for h in scans + [vm]:
            h.close()
        return poses, rounds, out, cached

    p0, r0, s0, c0 = run(state)
    p1, r1, s1, c1 = run(late)
    assert len(p0) == 6 and r0 == r1
    for a, b in zip(p0, p1):
        assert a.R.tobytes() == b.R.tobytes() and a.t.tobytes() == b.t.tobytes()
    assert s0["epoch"] > 3 + 6 - 1 and s1["epoch"] == s0["epoch"] + shift > (1 << 32)
    for got, want in ((s1, s0), (c1, c0)):
        for k in ("cells", "counts", "sums"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["stamps"], ((want["stamps"].astype(np.uint64) + np.uint64(shift)) % np.uint64(1 << 32)).astype(np.uint32))
    assert len(s0["counts"]) > 0 and (s1["stamps"] < 100).any()  # stamps from beyond the wrap
    first.close()


# ------------------------------------------------------------------------------------------------------- 6. the tally

def test_an_insert_and_a_merge_cost_the_same_launches_at_the_limit(ctx):
    """The bracket profiler's tally is the library's own count, and nos_voxel_map_insert and nos_voxel_map_merge report
    nothing to it: the figure is 0 for both calls, on the brim store as on its twin, as before the limit was checked.
    (That the check added no launch and no wait is read from store_merge_runs: the same two kernels, one closing wait.)"""
    from nonlinear_optimizer_for_slam_amd import api
    counts = {}
    for name, state in (("brim", li.brim_state(RES)), ("twin", li.brim_state(RES, ordinary=1000))):
        vm = api.VoxelMap.from_state(ctx, state)
        pts, _ = _batch(state, 31, {255: (3, 4)})
        src = api.VoxelMap(ctx, RES, 1.0)
        src.insert(pts)
        ctx.profile_begin(sample_every=0)
        vm.insert(pts[:200])
        counts[(name, "insert")] = ctx.profile_end()[0]
        ctx.profile_begin(sample_every=0)
        vm.merge(src, np.eye(3), np.array([0.0, 0.0, 9.0]))
        counts[(name, "merge")] = ctx.profile_end()[0]
        vm.close(), src.close()
    print("tally:", counts)
    assert set(counts.values()) == {0}, counts
