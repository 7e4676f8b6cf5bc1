"""Matching a scan against the LIVE voxel store (VoxelMap.match / nos_voxel_map_match): the dataset and the
match count are, bit for bit, what snapshot() followed by NdtMap.match gives — without the snapshot's sort, gather and
table build, and without touching the store.

Three kinds of truth: (1) the snapshot route on the same store (bytes of api.download and n_matches); (2) for EXACT inputs
(coordinates on a 2^-10 lattice, voxels of eight points placed symmetrically around their mean, so count = 8, 1 / 8 and every
sum, mean and squared distance are exact in any order) a numpy brute force over stats(), ties by slot number; (3) for
general inputs the same brute force with every point left out whose decision hangs on less than 1e-9 (at most 1 %).

The guard band: the live matcher looks for a voxel in its own cell, widened by g = resolution / 1024
(nos::kVoxelMatchGuard).  _guard_holds asserts, for every store compared below, that every valid voxel's mean lies
inside its cell widened by g — so an equality failure is never that.

Not reachable from a test: NOS_ERR_UNSUPPORTED for a multi-device context (a store cannot be created on one) and
NOS_ERR_HIP for a `broken` store (only a failed merge sets it)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import helpers, matcher_edge_inputs

pytestmark = pytest.mark.gpu

LOSS = ("exponential", 1.0, 1.0)
GUARD = 1.0 / 1024.0  # of a voxel edge
POSE = (helpers.rot_xyz(0.01, -0.02, 0.05), np.array([0.1, -0.2, 0.05]))
IDENTITY = (np.eye(3), np.zeros(3))
INVALID, HIP, UNSUPPORTED = 1, 3, 6


def _guard_holds(vm, res):
    st = vm.stats()
    ok = st["valid"]
    if not ok.any():
        return 0.0
    lo = st["cells"][ok] * res
    m = st["means"][ok]
    outside = np.maximum(np.maximum(lo - m, m - (lo + res)), 0.0).max()
    assert np.all(m >= lo - GUARD * res) and np.all(m <= lo + res + GUARD * res), outside
    return float(outside)


def _live(vm, sc, pose, k=2, dtype="f64"):
    ds, n = vm.match(sc, pose[0], pose[1], k, dtype)
    out = _download(ds)
    ds.close()
    return out, n


def _snap(vm, sc, pose, k=2, dtype="f64"):
    snap = vm.snapshot()
    ds, n = snap.match(sc, pose[0], pose[1], k, dtype)
    out = _download(ds)
    ds.close()
    snap.close()
    return out, n


def _download(ds):
    from nonlinear_optimizer_for_slam_amd import api
    return api.download(ds)


def _same_as_snapshot(vm, sc, pose, k=2, dtype="f64", res=None):
    if res is not None:
        _guard_holds(vm, res)
    a, na = _live(vm, sc, pose, k, dtype)
    b, nb = _snap(vm, sc, pose, k, dtype)
    assert a.shape == b.shape == (15, 2 * len(sc))
    assert na == nb, (na, nb)
    assert a.tobytes() == b.tobytes(), int(np.sum(a != b))
    return a, na


def _all_scan_forms(ctx, vm, pts, res):
    """unsorted and cell-sorted, a non-identity pose and the identity, f64 and f32, max_neighbors 1 and 2 → matches (f64, 2)"""
    from nonlinear_optimizer_for_slam_amd import api
    plain, by_cell = api.Scan(ctx, pts), api.Scan(ctx, pts, sort_cell=res)
    _guard_holds(vm, res)
    n = None
    for sc in (plain, by_cell):
        for pose in (POSE, IDENTITY):
            for dtype in ("f64", "f32"):
                for k in (2, 1):
                    _, got = _same_as_snapshot(vm, sc, pose, k, dtype)
                    if dtype == "f64" and k == 2 and pose is POSE:
                        assert n is None or n == got  # the order of the scan does not change what matches
                        n = got
    plain.close(), by_cell.close()
    return n


# ------------------------------------------------------------------------------ 1. equality with the snapshot route

@pytest.mark.parametrize("res,r2", [(1.0, 1.0), (0.5, 1.0), (2.0, 1.0), (1.0, 0.25)])
def test_a_live_match_equals_the_snapshot_route_through_the_life_of_a_store(ctx, res, r2):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(211)
    lo, hi = np.array([-8.0, -8.0, -2.0]), np.array([8.0, 8.0, 2.0])
    pts = rng.uniform(lo - 1.0, hi + 1.0, size=(12_000, 3))
    vm = api.VoxelMap(ctx, res, r2, capacity=0)  # 16 slots: the inserts below grow it
    assert vm.memory()["capacity"] == 16
    # an empty store: all-zero records, no matches
    sc = api.Scan(ctx, pts[:500])
    got, n = _same_as_snapshot(vm, sc, POSE)
    assert n == 0 and not got.any()
    sc.close()
    # one insert (growth from 16 slots)
    vm.insert(rng.uniform(lo, hi, size=(60_000, 3)))
    assert vm.memory()["generation"] >= 1 and vm.memory()["capacity"] > 16
    assert _all_scan_forms(ctx, vm, pts, res) > 1000
    # five inserts with overlapping frames
    for f in range(4):
        shift = np.array([2.0 * (f + 1), -1.0 * (f + 1), 0.0])
        vm.insert(rng.uniform(lo, hi, size=(40_000, 3)) + shift)
    assert vm.memory()["epoch"] == 5
    assert _all_scan_forms(ctx, vm, pts, res) > 1000
    # a box prune, an age prune
    assert vm.prune(center=(1.0, -1.0, 0.0), half_extent=(6.0, 5.0, 2.0)) > 0
    after_box = _all_scan_forms(ctx, vm, pts, res)
    vm.insert(rng.uniform([-3, -3, -2], [0, 0, 2], size=(20_000, 3)))
    assert vm.prune(max_age=0) > 0
    after_age = _all_scan_forms(ctx, vm, pts, res)
    assert 0 < after_age < after_box
    # an insert that re-creates removed cells
    vm.insert(rng.uniform(lo, hi, size=(60_000, 3)))
    assert _all_scan_forms(ctx, vm, pts, res) > after_age
    # an empty scan; a scan wholly outside the map
    empty = api.Scan(ctx, np.zeros((0, 3)))
    got, n = _same_as_snapshot(vm, empty, POSE)
    assert n == 0 and got.shape == (15, 0)
    far = api.Scan(ctx, rng.uniform([100, 100, 100], [120, 120, 104], size=(5_000, 3)))
    got, n = _same_as_snapshot(vm, far, POSE)
    assert n == 0 and not got.any()
    for h in (empty, far, vm):
        h.close()


# ------------------------------------------------------------------------------ 2. exact inputs

_voxel_points = matcher_edge_inputs.voxel_points  # shared with test_matcher_edges_gpu.py: the exact 8-point voxel


def _brute(means, valid, q, stable):
    """→ idx [n][3] of the three nearest valid means by (d2, slot), d2 [n][3] (inf-padded)"""
    ids = np.nonzero(valid)[0]
    n = q.shape[0]
    idx = np.full((n, 3), -1, dtype=np.int64)
    d2 = np.full((n, 3), np.inf)
    if ids.size == 0:
        return idx, d2
    m = means[ids]
    take = min(3, ids.size)
    for a in range(0, n, 2000):
        e = q[a:a + 2000, None, :] - m[None, :, :]
        d = e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1] + e[:, :, 2] * e[:, :, 2]
        if stable:
            order = np.argsort(d, axis=1, kind="stable")[:, :take]  # ties: lower slot first (ids ascend)
        else:
            part = np.argpartition(d, take - 1, axis=1)[:, :take] if ids.size > take else np.tile(np.arange(ids.size), (d.shape[0], 1))
            order = np.take_along_axis(part, np.argsort(np.take_along_axis(d, part, axis=1), axis=1, kind="stable"), axis=1)
        idx[a:a + 2000, :take] = ids[order]
        d2[a:a + 2000, :take] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def _expected_planes(stats, local, idx, d2, r2, k):
    n = local.shape[0]
    want = np.zeros((15, 2 * n))
    count = 0
    for s in range(k):
        hit = d2[:, s] < r2  # strict
        j = idx[hit, s]
        cols = 2 * np.nonzero(hit)[0] + s
        want[0:3, cols] = local[hit].T
        want[3:6, cols] = stats["means"][j].T
        want[6:15, cols] = stats["sqrt_infos"][j].reshape(-1, 9).T
        count += int(hit.sum())
    return want, count


def test_exact_inputs_faces_the_radius_itself_and_ties(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    res, r2 = 1.0, 1.0
    vm = api.VoxelMap(ctx, res, r2)
    # batch 1: B (5.5, .5, .5) — inserted before A although its cell comes later: slot order is not cell order
    vm.insert(_voxel_points((5.5, 0.5, 0.5), (0.125, 0.125, 0.125)))
    # batch 2: A (4.5, .5, .5), C (5, 1.5, .5) ON the x face of its cell (no spread in x), D (2, 0.5, 0.5) on a face,
    # E (2, 2, 2) on a cell corner (a single point eight times), F (7.5, 0.5, 0.5)
    batch = [_voxel_points((4.5, 0.5, 0.5), (0.125, 0.125, 0.125)), _voxel_points((5.0, 1.5, 0.5), (0.0, 0.125, 0.125)),
             _voxel_points((2.0, 0.5, 0.5), (0.0, 0.25, 0.25)), _voxel_points((2.0, 2.0, 2.0), (0.0, 0.0, 0.0)),
             _voxel_points((7.5, 0.5, 0.5), (0.25, 0.25, 0.25))]
    # a lattice of voxels whose means sit on quarter positions, faces (fraction 0) included
    rng = np.random.default_rng(223)
    for cx in range(-4, 0):
        for cy in range(-3, 3):
            for cz in range(-1, 2):
                frac = rng.integers(0, 4, size=3) / 4.0
                batch.append(_voxel_points(np.array([cx, cy, cz]) + frac, np.where(frac == 0.0, 0.0, 0.125)))
    vm.insert(np.concatenate(batch))
    st = vm.stats()
    assert st["valid"].all() and np.all(st["counts"] == 8) and len(vm) == 6 + 4 * 6 * 3
    assert np.array_equal(st["means"][0], [5.5, 0.5, 0.5]) and np.array_equal(st["cells"][0], [5, 0, 0])
    assert np.array_equal(st["means"] * 4, np.round(st["means"] * 4))  # exact means
    assert _guard_holds(vm, res) == 0.0
    slot = {tuple(m): s for s, m in enumerate(st["means"])}
    A, B, C = slot[(4.5, 0.5, 0.5)], slot[(5.5, 0.5, 0.5)], slot[(5.0, 1.5, 0.5)]
    assert B == 0 and B < A < C
    named = np.array([
        [5.0, 0.5, 0.5],    # A and B at d2 = 0.25 (C at 1.0: out): the lower slot B first, then A
        [5.0, 1.0, 0.5],    # A, B at 0.5 and C at 0.25: C first, then B (tie A / B by slot)
        [5.0, 1.0, 1.0],    # A, B at 0.75, C at 0.5
        [3.0, 0.5, 0.5],    # exactly the radius from D (2, .5, .5): no match from it
        [2.0, 1.5, 0.5],    # exactly the radius from D along y
        [2.0, 0.5, -0.5],   # exactly the radius from D along z
        [2.0, 2.0, 3.0],    # exactly the radius from the corner voxel E
        [2.0, 2.0, 2.0],    # on E itself: d2 = 0
        [8.5, 0.5, 0.5],    # exactly the radius from F, nothing else near
        [8.25, 0.5, 0.5],   # F at 0.5625
    ])
    lattice = rng.integers([-5 * 4, -4 * 4, -2 * 4], [9 * 4, 4 * 4, 4 * 4], size=(6000, 3)) / 4.0
    q = np.concatenate([named, lattice])
    idx, d2 = _brute(st["means"], st["valid"], q, stable=True)
    assert list(idx[0, :2]) == [B, A] and list(idx[1, :3]) == [C, B, A] and list(d2[1]) == [0.25, 0.5, 0.5]
    assert d2[3, 0] == 1.0 and d2[8, 0] == 1.0 and d2[7, 0] == 0.0
    # the cases are there in numbers: exact-radius candidates, two- and three-way ties, queries on cell faces
    assert int((d2 == r2).any(axis=1).sum()) > 20
    assert int((d2[:, 0] == d2[:, 1]).sum()) > 50 and int(((d2[:, 0] == d2[:, 2]) & (d2[:, 2] < r2)).sum()) > 5
    assert int((q == np.floor(q)).any(axis=1).sum()) > 1000
    sc, by_cell = api.Scan(ctx, q), api.Scan(ctx, q, sort_cell=res)
    for k in (2, 1):
        want, count = _expected_planes(st, q, idx, d2, r2, k)
        got, n = _same_as_snapshot(vm, sc, IDENTITY, k, "f64", res)
        assert n == count and np.array_equal(got, want)
        order = by_cell.order.astype(np.int64)
        want_s, _ = _expected_planes(st, q[order], idx[order], d2[order], r2, k)
        got, n = _same_as_snapshot(vm, by_cell, IDENTITY, k, "f64")
        assert n == count and np.array_equal(got, want_s)
    got, _ = _live(vm, sc, IDENTITY)
    assert not got[:, 2 * 3:2 * 3 + 2].any() and not got[:, 2 * 8:2 * 8 + 2].any()  # at the radius: strict, so nothing
    for h in (sc, by_cell, vm):
        h.close()


# ------------------------------------------------------------------------------ 3. general inputs, independent brute force

@pytest.mark.parametrize("res,r2,seed", [(1.0, 1.0, 227), (0.5, 1.0, 229), (2.0, 1.0, 233), (1.0, 0.25, 239)])
def test_general_inputs_against_a_numpy_brute_force(ctx, res, r2, seed):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(seed)
    vm = api.VoxelMap(ctx, res, r2)
    for _ in range(3):
        vm.insert(rng.uniform([-6, -6, -2], [6, 6, 2], size=(50_000, 3)))
    _guard_holds(vm, res)
    st = vm.stats()
    local = rng.uniform([-6.5, -6.5, -2.5], [6.5, 6.5, 2.5], size=(20_000, 3))
    R, t = POSE
    q = local @ R.T + t
    idx, d2 = _brute(st["means"], st["valid"], q, stable=False)
    margin = 1e-9
    risky = (np.abs(d2 - r2) < margin).any(axis=1) | (d2[:, 1] - d2[:, 0] < margin) | (d2[:, 2] - d2[:, 1] < margin)
    print("res %g r2 %g: %d voxels (%d valid), %d of %d points left out" % (res, r2, len(vm), st["valid"].sum(), risky.sum(), len(q)))
    assert risky.mean() <= 0.01
    keep = ~risky
    sc = api.Scan(ctx, local)
    got, n = _live(vm, sc, POSE)
    want, _ = _expected_planes(st, local, idx, d2, r2, 2)
    cols = np.stack([2 * np.nonzero(keep)[0], 2 * np.nonzero(keep)[0] + 1], axis=1).ravel()
    assert np.array_equal(got[3:6, cols], want[3:6, cols])  # the matched means ARE the truth's
    assert np.array_equal(got[6:15, cols], want[6:15, cols]) and np.array_equal(got[0:3, cols], want[0:3, cols])
    real = lambda planes: int(planes[6:15, cols].any(axis=0).sum())  # noqa: E731
    assert real(got) == real(want) == int((d2[keep, :2] < r2).sum()) > 1000
    assert abs(n - int((d2[:, :2] < r2).sum())) <= 2 * int(risky.sum())
    sc.close(), vm.close()


# ------------------------------------------------------------------------------ 5. independence

def test_the_dataset_is_independent_of_the_store_and_the_store_is_untouched(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(241)
    first, second = rng.uniform(-6, 6, size=(40_000, 3)), rng.uniform(-8, 8, size=(30_000, 3))
    vm, twin = api.VoxelMap(ctx, 1.0, 1.0), api.VoxelMap(ctx, 1.0, 1.0)
    vm.insert(first), twin.insert(first)
    sc = api.Scan(ctx, rng.uniform(-6, 6, size=(10_000, 3)))
    before, mem, info = vm.stats(), vm.memory(), (len(vm), vm.n_valid, vm.n_points)
    ds, n = vm.match(sc, *POSE)
    assert n > 1000
    assert vm.memory() == mem == twin.memory() and (len(vm), vm.n_valid, vm.n_points) == info  # epoch, generation, bytes
    after = vm.stats()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    held = api.download(ds).copy()
    # an insert after a match gives the store an insert without one gives
    assert vm.insert(second) == twin.insert(second)
    a, b = vm.stats(), twin.stats()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert vm.memory() == twin.memory()
    assert np.array_equal(api.download(ds), held)
    assert vm.prune(center=(0.0, 0.0, 0.0), half_extent=2.0) > 0
    assert np.array_equal(api.download(ds), held)
    vm.close()
    assert np.array_equal(api.download(ds), held)
    twin.close()
    for h in (ds, sc):
        h.close()


# ------------------------------------------------------------------------------ 6. work per call

def test_a_match_costs_the_same_launches_whatever_the_store_holds(ctx):
    """The launch count between profile_begin and profile_end is the library's own tally of what nos_voxel_map_match
    issues (one kernel, plus the padding kernel when the dataset has pads) — self-reported, so it documents the call's
    shape rather than policing it; that nothing map-sized is allocated is what memory() and the same count at 1 k and
    200 k voxels show."""
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(251)
    small, large = api.VoxelMap(ctx, 1.0, 1.0), api.VoxelMap(ctx, 1.0, 1.0)
    small.insert(rng.uniform([-5, -5, -5], [5, 5, 5], size=(20_000, 3)))
    for _ in range(25):
        large.insert(rng.uniform([-100, -100, -5], [100, 100, 5], size=(20_000, 3)))
    assert 500 <= len(small) <= 1100 and len(large) >= 200_000
    counts = {}
    for n_points in (4096, 5000):  # a dataset without and with padding behind its records
        sc = api.Scan(ctx, rng.uniform([-5, -5, -5], [5, 5, 5], size=(n_points, 3)))
        for name, vm in (("small", small), ("large", large)):
            mem = vm.memory()
            ctx.profile_begin(sample_every=0)
            ds, n = vm.match(sc, *POSE)
            launches = ctx.profile_end()[0]
            kernel = ctx.last_kernel()
            assert "voxel_match_kernel<double>" in kernel, kernel
            assert vm.memory() == mem  # nothing allocated in the store, nothing replaced
            assert n > 0
            counts[(n_points, name)] = launches
            ds.close()
        sc.close()
        assert counts[(n_points, "small")] == counts[(n_points, "large")] and 1 <= counts[(n_points, "small")] <= 2
    print("launches per match:", counts)
    small.close(), large.close()


# ------------------------------------------------------------------------------ 7. pipeline

@pytest.fixture(scope="module")
def room():
    pts = scene.generate_global_points()
    filtered = scene.filter_points(pts, 0.1)
    c, s = np.cos(0.1), np.sin(0.1)
    Rt = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    tt = np.array([-0.2, 0.123, 0.3])  # true pose, MDM/tests/simple_optimization_test.cc:85-88
    locals_ = []
    for f in range(12):  # a sensor that turns 0.01 rad and moves about 3 cm per frame
        Rf = Rt @ helpers.rot_xyz(0.0, 0.0, 0.01 * f)
        tf = tt + f * np.array([0.02, -0.02, 0.005])
        locals_.append((Rf.T @ (filtered - tf).T).T)
    return {"points": pts, "locals": locals_}


def _room_store(ctx, room):
    from nonlinear_optimizer_for_slam_amd import api
    vm = api.VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    for b in np.array_split(room["points"], 8):
        vm.insert(b)
    return vm


@pytest.mark.parametrize("dof", [6, 3])
@pytest.mark.parametrize("keep_multiple", [None, 4])
def test_scan_to_map_takes_a_voxel_map(ctx, room, dof, keep_multiple):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    vm = _room_store(ctx, room)
    _guard_holds(vm, 1.0)
    sc = api.Scan(ctx, room["locals"][0])
    snap = vm.snapshot()
    want = pipeline.scan_to_map(ctx, snap, sc, loss=LOSS, dof=dof, keep_multiple=keep_multiple)
    got = pipeline.scan_to_map(ctx, vm, sc, loss=LOSS, dof=dof, keep_multiple=keep_multiple)
    assert np.array_equal(got[0].R, want[0].R) and np.array_equal(got[0].t, want[0].t)
    assert got[1] == want[1] and got[2] == want[2] and len(got[1]) >= 1 and got[1][0]["matches"] > 1000
    with pytest.raises(ValueError):
        pipeline.scan_to_map(ctx, vm, sc, loss=LOSS, dof=dof, indexed=True)
    for h in (snap, sc, vm):
        h.close()


@pytest.mark.parametrize("kwargs", [{}, {"window_half_extent": (3.0, 2.5, 2.0), "max_voxel_age": 6}, {"filter_voxel_size": 0.3}],
                         ids=["plain", "window", "filter"])
def test_odometry_with_live_match_equals_odometry_with_snapshots(ctx, room, kwargs):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    scans = [api.Scan(ctx, p) for p in room["locals"]]
    a, b = _room_store(ctx, room), _room_store(ctx, room)
    want = pipeline.odometry(ctx, a, scans, loss=LOSS, **kwargs)
    got = pipeline.odometry(ctx, b, scans, loss=LOSS, live_match=True, **kwargs)
    assert len(got[0]) == len(want[0]) == 12
    for pa, pb in zip(got[0], want[0]):
        assert np.array_equal(pa.R, pb.R) and np.array_equal(pa.t, pb.t)
    assert got[1] == want[1] and all(len(r) >= 1 for r in got[1])
    sa, sb = a.stats(), b.stats()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert a.memory() == b.memory()
    _guard_holds(b, 1.0)
    for h in scans + [a, b]:
        h.close()


# ------------------------------------------------------------------------------ 8. rejections

def test_rejected_matches_return_their_status_and_write_nothing(ctx):
    from nonlinear_optimizer_for_slam_amd import Context, api
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    lib = ctx._lib
    rng = np.random.default_rng(257)
    pts = rng.uniform(-4, 4, size=(30_000, 3))
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    vm.insert(pts)
    sc = api.Scan(ctx, pts[:2000])
    other = Context((0,))
    foreign = api.Scan(other, pts[:100])
    R = np.ascontiguousarray(np.eye(3).reshape(9))
    t = np.zeros(3)
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))  # noqa: E731
    sentinel = 0xABCDE0
    out, n = ctypes.c_void_p(sentinel), ctypes.c_size_t(777)
    mem, before = vm.memory(), vm.stats()

    def call(vm_h=vm._h, sc_h=sc._h, Rp=dp(R), tp=dp(t), k=2, dtype=0, out_p=ctypes.byref(out)):
        return lib.nos_voxel_map_match(vm_h, sc_h, Rp, tp, k, dtype, out_p, ctypes.byref(n))

    cases = [(dict(vm_h=None), INVALID, "NULL"), (dict(sc_h=None), INVALID, "NULL"), (dict(Rp=None), INVALID, "NULL"),
             (dict(tp=None), INVALID, "NULL"), (dict(out_p=None), INVALID, "NULL"),
             (dict(sc_h=foreign._h), INVALID, "different contexts"), (dict(dtype=2), INVALID, "dtype 2"),
             (dict(dtype=-1), INVALID, "dtype -1"), (dict(k=0), UNSUPPORTED, "max_neighbors"), (dict(k=3), UNSUPPORTED, "max_neighbors")]
    for kwargs, status, text in cases:
        assert lib.nos_voxel_map_info(None, None, None, None) == INVALID  # another message in between: the text is sticky
        assert "voxel map is NULL" in lib.nos_last_error().decode()
        assert call(**kwargs) == status, kwargs
        assert text in lib.nos_last_error().decode(), (kwargs, lib.nos_last_error().decode())
        assert out.value == sentinel and n.value == 777, kwargs
    # the 9-cell span limit: 2 r / resolution + 2 > 9
    fine = api.VoxelMap(ctx, 0.25, 1.0)
    fine.insert(pts)
    assert call(vm_h=fine._h) == UNSUPPORTED and "9" in lib.nos_last_error().decode()
    assert out.value == sentinel and n.value == 777
    with pytest.raises(NosError) as err:
        fine.match(sc, R, t)
    assert err.value.status == UNSUPPORTED
    fine.close()
    coarse_enough = api.VoxelMap(ctx, 0.3, 1.0)
    coarse_enough.insert(pts)
    for form in (sc, api.Scan(ctx, pts[:2000], sort_cell=0.3)):
        _, got = _same_as_snapshot(coarse_enough, form, POSE, 2, "f64", 0.3)
        assert got > 1000
    coarse_enough.close()
    # nothing above touched the store; n_matches may be NULL in a call that succeeds
    assert vm.memory() == mem
    after = vm.stats()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    assert lib.nos_voxel_map_match(vm._h, sc._h, dp(R), dp(t), 2, 0, ctypes.byref(out), None) == 0
    assert out.value not in (None, sentinel)
    lib.nos_dataset_destroy(out)
    for h in (foreign, other, sc, vm):
        h.close()
