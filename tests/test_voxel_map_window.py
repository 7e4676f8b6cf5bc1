"""The sliding window of the incremental voxel map (VoxelMap.prune / memory, nos_voxel_map_prune / _memory): voxels are
removed by a box around a point and / or by age, the survivors are compacted on the device, the store can shrink.

CPU truth is the dict model below: cell → slot, and per slot count, the nine sums, the stamp and the epoch of birth, kept in
slot order and pruned with the documented keep rule in numpy.  Mean and sqrt-information have no bit-exact CPU form; for
EXACT inputs (coordinates that are multiples of 2^-10 with |x| <= 64: every sum is exact in any order, see
test_voxel_map.py::test_exact_inputs_give_the_same_bits_for_any_split) the model's expected statistics are those of ONE
nos_ndt_map_build over exactly the points the model says its live voxels hold — a path that shares nothing with the
store's merge, prune and compaction — and "same" means np.array_equal on cells, counts, valid, means and sqrt_infos."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import helpers
from tests.voxel_store_model import (KEYS, Model, _assert_is_model, _box_bounds, _box_keep, _cells_of, _pack, _pow2_at_least,
                                      _same_bits)

pytestmark = pytest.mark.gpu

LOSS = ("exponential", 1.0, 1.0)


def _take(stats, mask):
    return {k: stats[k][mask] for k in KEYS}


def _exact(rng, lo, hi, n):
    pts = rng.integers(np.asarray(lo) * 1024, np.asarray(hi) * 1024, size=(n, 3)).astype(np.float64) / 1024.0
    assert np.max(np.abs(pts)) <= 64 and np.array_equal(pts * 1024, np.round(pts * 1024))
    return pts


# ------------------------------------------------------------------------------ 1. a prune removes the rule's voxels

@pytest.mark.parametrize("res", [1.0, 0.5, 0.3])
def test_a_box_prune_removes_exactly_the_rules_voxels_and_copies_the_rest(ctx, res):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(101)
    pts = _exact(rng, [-16, -16, -2], [16, 16, 2], 150_000)
    boxes = [((0.0, 0.0, 0.0), (5.25, 3.5, 1.0)),
             ((-8.0, -8.0, 0.0), (4.0, 4.0, 1.0)),  # faces exactly on cell boundaries at res 1.0 and 0.5: inclusive on both sides
             ((3.3, -2.7, 0.4), 6.1),               # a cube
             ((40.0, 0.0, 0.0), (2.0, 2.0, 2.0))]   # beyond the data: everything goes
    for center, half in boxes:
        vm = api.VoxelMap(ctx, res, 1.0)
        for b in np.array_split(pts, 3):
            vm.insert(b)
        before = vm.stats()
        assert len(before["counts"]) >= 1000 and before["cells"].min() < 0
        keep = _box_keep(before["cells"], center, half, res)
        if center == (-8.0, -8.0, 0.0) and res in (1.0, 0.5):
            lo, hi = _box_bounds(center, half, res)
            assert np.array_equal(lo, np.array([-12, -12, -1]) / res) and np.array_equal(hi, np.array([-4, -4, 1]) / res)
            # the cells that only touch the box's upper faces are there and are kept
            assert np.any(keep & (before["cells"][:, 0] == hi[0])) and np.any(keep & (before["cells"][:, 2] == hi[2]))
        gen = vm.memory()["generation"]
        removed = vm.prune(center=center, half_extent=half)
        print("res %.1f box %r: %d voxels, %d removed (model %d)" % (res, (center, half), keep.size, removed, (~keep).sum()))
        assert removed == int((~keep).sum()) and 0 < removed
        after = vm.stats()
        _same_bits(after, _take(before, keep))  # same relative order, bit for bit
        assert len(vm) == int(keep.sum()) and vm.n_valid == int(before["valid"][keep].sum())
        assert vm.n_points == int(before["counts"][keep].astype(np.int64).sum())
        assert vm.memory()["generation"] == gen + 1
        vm.close()


def test_a_box_prune_equals_the_model_on_exact_inputs(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(103)
    for res in (1.0, 0.5):
        vm, model = api.VoxelMap(ctx, res, 1.0), Model(res)
        for b in np.array_split(_exact(rng, [-16, -16, -2], [16, 16, 2], 150_000), 4):
            assert vm.insert(b) == model.insert(b)
        assert vm.prune(center=(-2.0, 1.0, 0.0), half_extent=(6.0, 7.0, 1.0)) == model.prune((-2.0, 1.0, 0.0), (6.0, 7.0, 1.0))
        _assert_is_model(ctx, vm, model)
        vm.close()


# ------------------------------------------------------------------------------ 2. a store after a prune is a store

@pytest.mark.parametrize("exact", [True, False])
def test_a_pruned_store_takes_the_next_batch_like_any_store(ctx, exact):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(107)

    def cloud(lo, hi, n):
        return _exact(rng, lo, hi, n) if exact else rng.uniform(lo, hi, size=(n, 3))

    A = [cloud([-12, -12, -2], [12, 12, 2], 40_000) for _ in range(3)]
    B = cloud([-4, -4, -2], [20, 20, 2], 60_000)  # surviving cells, removed cells and cells never seen
    center, half = (-3.0, -3.0, 0.0), (6.5, 6.5, 2.0)
    full, pruned = api.VoxelMap(ctx, 1.0, 1.0), api.VoxelMap(ctx, 1.0, 1.0)
    for a in A:
        full.insert(a), pruned.insert(a)
    before = pruned.stats()
    keep = _box_keep(before["cells"], center, half, 1.0)
    assert pruned.prune(center=center, half_extent=half) == int((~keep).sum())
    survivors = before["cells"][keep]
    b_cells = np.unique(_cells_of(B, 1.0), axis=0)  # ascending lexicographic = ascending cell
    s_keys, a_keys, b_keys = _pack(survivors), _pack(before["cells"]), _pack(b_cells)
    reseen = b_cells[np.isin(b_keys, a_keys) & ~np.isin(b_keys, s_keys)]
    fresh = b_cells[~np.isin(b_keys, a_keys)]
    touched_survivors = int(np.isin(b_keys, s_keys).sum())
    assert touched_survivors > 50 and len(reseen) > 50 and len(fresh) > 50 and int(np.isin(s_keys, b_keys).sum()) < len(s_keys)
    assert pruned.insert(B) == len(b_cells) == full.insert(B)
    got, ref = pruned.stats(), full.stats()
    # no duplicate out of the rebuilt table; slot order = survivors in their old order, then B's new cells ascending
    new_cells = b_cells[~np.isin(b_keys, s_keys)]
    assert len(pruned) == len(survivors) + len(new_cells) == len(np.unique(got["cells"], axis=0))
    assert np.array_equal(got["cells"], np.concatenate([survivors, new_cells]))
    # surviving cells: both stores computed store + batch on the same bits
    at = {int(k): s for s, k in enumerate(_pack(ref["cells"]))}
    idx = np.array([at[int(k)] for k in s_keys])
    _same_bits(_take(got, np.arange(len(survivors))), _take(ref, idx))
    assert pruned.n_points == int(got["counts"].astype(np.int64).sum())
    assert pruned.n_valid == int(got["valid"].sum())
    if exact:  # a removed cell seen again starts from zero: a fresh store given only B's points of those cells
        in_reseen = np.isin(_pack(_cells_of(B, 1.0)), _pack(reseen))
        alone = api.VoxelMap(ctx, 1.0, 1.0)
        assert alone.insert(B[in_reseen]) == len(reseen)
        pos = np.nonzero(np.isin(_pack(got["cells"]), _pack(reseen)))[0]
        _same_bits(_take(got, pos), alone.stats())
        alone.close()
    for h in (full, pruned):
        h.close()


# ------------------------------------------------------------------------------ 3. the snapshot follows

def test_a_snapshot_after_a_prune_matches_like_a_map_of_the_filtered_statistics(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(109)
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for _ in range(3):
        vm.insert(rng.uniform([-15, -15, -2], [15, 15, 2], size=(80_000, 3)))
    before = vm.stats()
    center, half = (2.0, -1.0, 0.0), (7.0, 6.0, 1.5)
    keep = _box_keep(before["cells"], center, half, 1.0)
    assert vm.prune(center=center, half_extent=half) == int((~keep).sum()) > 0
    want = _take(before, keep)
    direct = api.NdtMap(ctx, want["means"], want["sqrt_infos"], want["valid"])
    snap = vm.snapshot()
    assert len(snap) == len(direct)
    sc = api.Scan(ctx, rng.uniform([-12, -12, -2], [12, 12, 2], size=(30_000, 3)))
    R, t = helpers.rot_xyz(0.01, -0.02, 0.05), np.array([0.1, -0.2, 0.05])
    da, na = direct.match(sc, R, t, 2, "f64")
    db, nb = snap.match(sc, R, t, 2, "f64")
    assert na == nb and 0 < na
    assert np.array_equal(api.download(da), api.download(db))
    for h in (da, db, sc, snap, direct, vm):
        h.close()


# ------------------------------------------------------------------------------ 4. age

def _drifting_batches(rng):
    return [_exact(rng, [-30 + 5 * k, -6, -2], [-18 + 5 * k, 6, 2], 15_000) for k in range(10)]


@pytest.mark.parametrize("max_age", [0, 1, 3])
def test_an_age_prune_equals_the_model_and_a_rejected_insert_does_not_age_the_store(ctx, max_age):
    from nonlinear_optimizer_for_slam_amd import api
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    rng = np.random.default_rng(113)
    vm, model = api.VoxelMap(ctx, 1.0, 1.0), Model(1.0)
    assert vm.memory()["epoch"] == 0
    for k, b in enumerate(_drifting_batches(rng)):
        assert vm.insert(b) == model.insert(b)
        if k == 6:
            bad = b.copy()
            bad[77, 2] = np.nan
            with pytest.raises(NosError):
                vm.insert(bad)
            assert vm.insert(np.zeros((0, 3))) == 0  # an empty insert is no insert either
        assert vm.memory()["epoch"] == k + 1
    keep = model.keep_mask(max_age=max_age)
    removed = vm.prune(max_age=max_age)
    print("max_age %d: %d voxels, %d removed" % (max_age, keep.size, removed))
    assert removed == model.prune(max_age=max_age) == int((~keep).sum()) and 0 < removed < keep.size
    _assert_is_model(ctx, vm, model)
    assert vm.prune(max_age=max_age) == 0 and vm.memory()["epoch"] == 10  # a prune is not an insert
    vm.close()


def test_box_and_age_together_are_the_conjunction(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(127)
    vm, model = api.VoxelMap(ctx, 1.0, 1.0), Model(1.0)
    for b in _drifting_batches(rng):
        vm.insert(b), model.insert(b)
    center, half, age = (8.0, -2.0, 0.0), (9.0, 3.0, 2.0), 3
    box, old = model.keep_mask(center, half), model.keep_mask(max_age=age)
    both = model.keep_mask(center, half, age)
    assert np.array_equal(both, box & old) and (box & ~old).any() and (old & ~box).any() and both.any()
    assert vm.prune(center=center, half_extent=half, max_age=age) == model.prune(center, half, age) == int((~both).sum())
    _assert_is_model(ctx, vm, model)
    vm.close()


# ------------------------------------------------------------------------------ 5. nothing to remove: no side effects

def test_a_prune_that_removes_nothing_leaves_the_store_and_its_generation_alone(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(131)
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for _ in range(3):
        vm.insert(rng.uniform([-20, -20, -3], [20, 20, 3], size=(50_000, 3)))
    before, mem, info = vm.stats(), vm.memory(), (len(vm), vm.n_valid, vm.n_points)
    assert mem["epoch"] == 3 and mem["capacity"] >= len(vm) and mem["bytes"] >= 185 * mem["capacity"]
    assert vm.prune(center=(0.0, 0.0, 0.0), half_extent=1000.0) == 0
    assert vm.prune(max_age=3) == 0
    assert vm.prune(center=(0.0, 0.0, 0.0), half_extent=(20.0, 20.0, 3.0), max_age=10 ** 12) == 0
    assert vm.memory() == mem and (len(vm), vm.n_valid, vm.n_points) == info
    _same_bits(vm.stats(), before)
    empty = api.VoxelMap(ctx, 1.0, 1.0)
    assert empty.prune(max_age=0) == 0 and len(empty) == 0 and empty.memory()["generation"] == 0
    for h in (vm, empty):
        h.close()


def test_prune_arguments_of_the_python_surface(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for kwargs in ({}, {"center": (0, 0, 0)}, {"half_extent": 3.0}, {"half_extent": (1, 2, 3), "max_age": 2},
                   {"center": (0, 0), "half_extent": 1.0}, {"max_age": -1}):
        with pytest.raises(ValueError):
            vm.prune(**kwargs)
    assert set(vm.memory()) == {"capacity", "bytes", "epoch", "generation"}
    vm.close()


# ------------------------------------------------------------------------------ 6. shrink and regrow

def test_a_store_shrinks_and_regrows_and_equals_a_roomy_twin_in_slot_order(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(11)
    batches = [rng.uniform([-100, -100, -5], [100, 100, 5], size=(20_000, 3)) for _ in range(25)]
    rounds = [(np.array([3.0 * r, 2.0 * r, 0.0]), rng.uniform([-30, -30, -5], [30, 30, 5], size=(20_000, 3))) for r in range(25)]
    runs = []
    for capacity in (16, 1 << 19, 16):
        vm = api.VoxelMap(ctx, 1.0, 1.0, capacity=capacity)
        for b in batches:
            vm.insert(b)
        grown = vm.memory()
        assert len(vm) >= 100_000 and grown["capacity"] >= len(vm) and grown["capacity"] >= capacity
        removed = vm.prune(center=(0.0, 0.0, 0.0), half_extent=(4.0, 4.0, 5.0))
        kept = len(vm)
        assert 0 < kept < 1000 and removed + kept >= 100_000
        shrunk = vm.memory()
        assert shrunk["capacity"] == max(_pow2_at_least(2 * kept), capacity)  # the survivors fit in a quarter
        assert shrunk["generation"] == grown["generation"] + 1
        if capacity == 16:
            assert shrunk["capacity"] < grown["capacity"] and shrunk["bytes"] < grown["bytes"] // 32
        log = [(removed, kept, vm.stats())]
        for center, local in rounds:
            touched = vm.insert(local + center)
            before = len(vm)
            cap = vm.memory()["capacity"]
            removed = vm.prune(center=center, half_extent=(20.0, 20.0, 5.0))
            kept = len(vm)
            assert removed + kept == before and kept <= 42 * 42 * 12
            want_cap = max(_pow2_at_least(2 * kept), capacity) if (removed and kept <= cap // 4) else cap
            assert vm.memory()["capacity"] == want_cap
            log.append((touched, removed, kept, vm.n_valid, vm.n_points, vm.stats() if len(log) % 6 == 0 else None))
        log.append(vm.stats())
        runs.append(log)
        vm.close()
    for other in runs[1:]:
        assert len(other) == len(runs[0])
        for a, b in zip(runs[0], other):
            if isinstance(a, dict):
                _same_bits(a, b)
                continue
            assert a[:-1] == b[:-1]
            if a[-1] is not None:
                _same_bits(a[-1], b[-1])  # identical statistics in identical slot order


# ------------------------------------------------------------------------------ 7. bounded on a long trajectory

def test_a_windowed_store_stays_bounded_over_eighty_frames_and_equals_the_model(ctx):
    """80 frames of exact-coordinate points in a 30 x 30 x 4 m slab around a sensor that advances 1.5 m per frame along
    (0.8, 0.6, 0) — the diagonal keeps every coordinate within |x| <= 64 — pruned to center +- (20, 20, 4) per frame."""
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(137)
    res, half = 1.0, (20.0, 20.0, 4.0)
    bound = int(np.prod([2 * h / res + 2 for h in half]))
    vm, twin, model = api.VoxelMap(ctx, res, 1.0), api.VoxelMap(ctx, res, 1.0), Model(res)
    step = np.array([1.2, 0.9, 0.0])
    assert abs(np.linalg.norm(step) - 1.5) < 1e-12
    start = -39.5 * step
    largest = 0
    for f in range(80):
        center = start + f * step
        c = np.round(center * 1024) / 1024
        pts = c + rng.integers([-15 * 1024, -15 * 1024, -2 * 1024], [15 * 1024, 15 * 1024, 2 * 1024], size=(30_000, 3)) / 1024.0
        assert np.max(np.abs(pts)) <= 64 and np.array_equal(pts * 1024, np.round(pts * 1024))
        assert vm.insert(pts) == model.insert(pts) == twin.insert(pts)
        largest = max(largest, len(vm))
        assert vm.prune(center=center, half_extent=half) == model.prune(center, half)
        mem = vm.memory()
        assert len(vm) <= bound and mem["capacity"] <= 4 * _pow2_at_least(largest + 1)
        lo, hi = _box_bounds(center, half, res)
        if f % 10 == 9:
            got = vm.stats()
            assert np.all((got["cells"] >= lo) & (got["cells"] <= hi))
            _assert_is_model(ctx, vm, model)
            print("frame %d: window %d voxels (bound %d), capacity %d, twin %d voxels" % (f + 1, len(vm), bound, mem["capacity"], len(twin)))
    assert len(twin) > 2 * len(vm)
    assert twin.memory()["epoch"] == vm.memory()["epoch"] == 80
    for h in (vm, twin):
        h.close()


# ------------------------------------------------------------------------------ 8. pipeline.odometry with a window

@pytest.fixture(scope="module")
def room():
    pts = scene.generate_global_points()
    filtered = scene.filter_points(pts, 0.1)
    c, s = np.cos(0.1), np.sin(0.1)
    Rt = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    tt = np.array([-0.2, 0.123, 0.3])  # true pose, MDM/tests/simple_optimization_test.cc:85-88
    # second pose: 0.05 m / 0.02 rad away from the true one (the two-scan setup of test_voxel_map.py)
    R2 = Rt @ helpers.rot_xyz(0.0, 0.0, 0.02)
    t2 = tt + np.array([0.03, -0.04, 0.0])
    locals_ = [(Rt.T @ (filtered - tt).T).T, (R2.T @ (filtered - t2).T).T]
    return {"points": pts, "locals": locals_}


def _room_store(ctx, room):
    from nonlinear_optimizer_for_slam_amd import api
    vm = api.VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    for b in np.array_split(room["points"], 8):
        vm.insert(b)
    return vm


def _same_run(a, b):
    assert len(a[0]) == len(b[0]) == 2
    for pa, pb in zip(a[0], b[0]):
        assert np.array_equal(pa.R, pb.R) and np.array_equal(pa.t, pb.t)
    assert a[1] == b[1]


def test_odometry_with_a_window(ctx, room):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    scans = [api.Scan(ctx, p) for p in room["locals"]]
    # a window larger than the scene, an age no voxel reaches: the windowless call's poses and rounds
    plain = _room_store(ctx, room)
    base = pipeline.odometry(ctx, plain, scans, loss=LOSS)
    wide = _room_store(ctx, room)
    _same_run(pipeline.odometry(ctx, wide, scans, loss=LOSS, window_half_extent=1000.0, max_voxel_age=1000), base)
    _same_bits(wide.stats(), plain.stats())
    assert wide.memory() == plain.memory()  # the inserts grew both alike; no prune replaced the block
    # a small window: the hand-written loop of the public calls
    half = (3.0, 2.5, 2.0)
    small, by_hand = _room_store(ctx, room), _room_store(ctx, room)
    n_before = len(small)
    got = pipeline.odometry(ctx, small, scans, loss=LOSS, window_half_extent=half)
    pose, poses, rounds = Pose(), [], []
    for sc in scans:
        snap = by_hand.snapshot()
        pose, r, _ = pipeline.scan_to_map(ctx, snap, sc, initial_pose=pose, loss=LOSS)
        snap.close()
        by_hand.insert_scan(sc, pose.R, pose.t)
        by_hand.prune(center=pose.t, half_extent=half)
        poses.append(Pose(pose.R, pose.t))
        rounds.append(r)
    _same_run(got, (poses, rounds))
    stats = small.stats()
    _same_bits(stats, by_hand.stats())
    lo, hi = _box_bounds(got[0][-1].t, half, 1.0)
    assert 0 < len(small) < n_before and np.all((stats["cells"] >= lo) & (stats["cells"] <= hi))
    assert len(got[1][1]) > 0 and got[1][1][0]["matches"] < base[1][1][0]["matches"]  # the second scan saw the window only
    for h in scans + [plain, wide, small, by_hand]:
        h.close()


# ------------------------------------------------------------------------------ 9. rejected calls write nothing

def test_rejected_prunes_write_nothing(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    from nonlinear_optimizer_for_slam_amd._lib import NOS_PRUNE_AGE, NOS_PRUNE_BOX, NosVoxelPrune
    lib = ctx._lib
    INVALID = 1
    rng = np.random.default_rng(19)
    vm, twin = api.VoxelMap(ctx, 1.0, 1.0), api.VoxelMap(ctx, 1.0, 1.0)
    first = rng.uniform(-6, 6, size=(40_000, 3))
    vm.insert(first), twin.insert(first)
    before, mem, info = vm.stats(), vm.memory(), (len(vm), vm.n_valid, vm.n_points)
    sentinel = 12345
    n = ctypes.c_size_t(sentinel)

    def rule(what=NOS_PRUNE_BOX, size=ctypes.sizeof(NosVoxelPrune), center=(0.0, 0.0, 0.0), half=(1.0, 1.0, 1.0), age=0):
        r = NosVoxelPrune()
        r.struct_size, r.what, r.max_age = size, what, age
        for k in range(3):
            r.center[k], r.half_extent[k] = center[k], half[k]
        return r

    assert ctypes.sizeof(NosVoxelPrune) == 72
    bad = [rule(what=0), rule(what=4), rule(what=NOS_PRUNE_BOX | 8), rule(what=-1), rule(size=ctypes.sizeof(NosVoxelPrune) - 8),
           rule(size=0), rule(center=(0.0, np.nan, 0.0)), rule(center=(np.inf, 0.0, 0.0)), rule(half=(1.0, 1.0, np.nan)),
           rule(half=(1.0, np.inf, 1.0)), rule(half=(1.0, -0.5, 1.0)), rule(what=NOS_PRUNE_BOX | NOS_PRUNE_AGE, half=(-1.0, 1.0, 1.0))]
    for r in bad:
        assert lib.nos_voxel_map_prune(vm._h, ctypes.byref(r), ctypes.byref(n)) == INVALID
        assert n.value == sentinel
    assert lib.nos_voxel_map_prune(vm._h, None, ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_prune(None, ctypes.byref(rule()), ctypes.byref(n)) == INVALID
    assert lib.nos_voxel_map_memory(None, None, None, None, None) == INVALID
    assert n.value == sentinel
    _same_bits(vm.stats(), before)
    assert vm.memory() == mem and (len(vm), vm.n_valid, vm.n_points) == info
    # the age test does not read the box: NaNs there are not looked at; n_removed may be NULL; every output of memory too
    assert lib.nos_voxel_map_prune(vm._h, ctypes.byref(rule(what=NOS_PRUNE_AGE, center=(np.nan,) * 3, age=5)), None) == 0
    assert lib.nos_voxel_map_memory(vm._h, None, None, None, None) == 0
    _same_bits(vm.stats(), before)
    assert vm.memory() == mem
    # a following insert gives what it gives a store that saw none of this
    second = rng.uniform(-8, 8, size=(20_000, 3))
    assert vm.insert(second) == twin.insert(second)
    _same_bits(vm.stats(), twin.stats())
    assert vm.memory() == twin.memory()
    # and a real prune through the C entry point reports what it removed
    assert lib.nos_voxel_map_prune(vm._h, ctypes.byref(rule(half=(2.0, 2.0, 2.0))), ctypes.byref(n)) == 0
    assert n.value == len(twin) - len(vm) > 0
    for h in (vm, twin):
        h.close()
