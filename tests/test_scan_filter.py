"""The voxel-grid scan filter on the device (api.Scan.filtered / nos_scan_filter, api.Scan.points / nos_scan_points):
the first point of every voxel, in stored order, bit for bit.

The truth is stated here (`_truth`): first occurrence per INTEGER cell floor(p * (1 / voxel_size)), in index order — what
FilterPoints of the reference's harness computes (MDM/tests/simple_optimization_test.cc:206-223) wherever its Cantor-paired
key does not overflow.  On the room (0.1, 0.05, 0.25 m) and on the outlier cloud of tests/test_voxel_map.py (0.5, 0.1 m)
the oracle's restatement, oracle_scene.filter_points, is asserted to agree with it; at finer resolutions of the outlier
cloud the oracle's int64 Cantor key overflows and only the truth is used.  Everything is compared with np.array_equal: the
filter moves points, it computes none."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import helpers

pytestmark = pytest.mark.gpu

LOSS = ("exponential", 1.0, 1.0)
INVALID, UNSUPPORTED = 1, 6


def _truth(p, vs):
    """→ ascending indices of the points FilterPoints keeps."""
    c = np.floor(p * (1.0 / vs)).astype(np.int64)
    _, first = np.unique(c, axis=0, return_index=True)
    return np.sort(first)


def _outlier_cloud():
    """The cloud of tests/test_voxel_map.py::_outlier_cloud: 200 000 random points, negative cells, a far outlier cluster."""
    rng = np.random.default_rng(20261005)
    pts = np.concatenate([rng.uniform([-37, -12, -4], [41, 29, 6], size=(200_000, 3)),
                          rng.uniform(0, 1, size=(300, 3)) + np.array([-900.0, 1500.0, 77.0])])
    rng.shuffle(pts)
    return pts


@pytest.fixture(scope="module")
def room_points():
    return scene.generate_global_points()


@pytest.fixture(scope="module")
def clouds(room_points):
    return {"room": room_points, "outlier": _outlier_cloud()}


def _close(*handles):
    for h in handles:
        h.close()


def _assert_is_truth(ctx, pts, vs):
    from nonlinear_optimizer_for_slam_amd import api
    keep = _truth(pts, vs)
    s = api.Scan(ctx, pts)
    f = s.filtered(vs)
    assert len(f) == keep.size
    assert np.array_equal(f.order, keep)
    assert np.array_equal(f.points(), pts[keep])
    assert len(s) == pts.shape[0] and np.array_equal(s.points(), pts)  # the source is unchanged
    _close(f, s)
    return keep


# ------------------------------------------------------------------------------ 1. the room and the outlier cloud

CASES = [("room", 0.1, 9356), ("room", 0.05, 37711), ("room", 0.25, 1463), ("outlier", 0.5, 138432), ("outlier", 0.1, 199631)]


@pytest.mark.parametrize("cloud,vs,count", CASES)
def test_filtered_scan_is_the_first_point_per_cell_in_index_order(ctx, clouds, cloud, vs, count):
    pts = clouds[cloud]
    keep = _assert_is_truth(ctx, pts, vs)
    assert keep.size == count
    assert np.array_equal(scene.filter_points(pts, vs), pts[keep])  # the oracle's restatement agrees on these inputs


def test_outlier_cloud_where_the_oracles_cantor_key_overflows(ctx, clouds):
    """0.05 m puts the outlier cluster at cells near 3e4: the oracle's int64 Cantor pairing overflows there, the integer
    cells do not."""
    _assert_is_truth(ctx, clouds["outlier"], 0.05)


# ------------------------------------------------------------------------------ 2. sort invariance

@pytest.mark.parametrize("cloud,vs", [("room", 0.1), ("room", 0.05), ("outlier", 0.5)])
def test_a_cell_sorted_scan_keeps_the_same_points_in_its_own_order(ctx, clouds, cloud, vs):
    from nonlinear_optimizer_for_slam_amd import api
    pts = clouds[cloud]
    keep = _truth(pts, vs)
    s = api.Scan(ctx, pts, sort_cell=1.0)
    stored = s.order
    assert not np.array_equal(stored, np.arange(pts.shape[0]))
    f = s.filtered(vs)
    order = f.order
    assert np.array_equal(np.sort(order), keep)  # the same set
    is_kept = np.zeros(pts.shape[0], dtype=bool)
    is_kept[keep] = True
    assert np.array_equal(order, stored[is_kept[stored]])  # in the cell-sorted scan's stored order
    assert np.array_equal(f.points(), pts[order])
    _close(f, s)


def test_constructor_filters_then_sorts(ctx, clouds):
    from nonlinear_optimizer_for_slam_amd import api
    pts, vs = clouds["room"], 0.1
    keep = _truth(pts, vs)
    a = api.Scan(ctx, pts, sort_cell=1.0, filter_voxel=vs)
    b = api.Scan(ctx, pts[keep], sort_cell=1.0)
    assert len(a) == keep.size
    assert np.array_equal(a.order, keep[b.order])  # the sort composes with the filter's order
    assert np.array_equal(a.points(), b.points()) and np.array_equal(a.points(), pts[a.order])
    c = api.Scan(ctx, pts, filter_voxel=vs)
    assert np.array_equal(c.order, keep) and np.array_equal(c.points(), pts[keep])
    _close(a, b, c)


# ------------------------------------------------------------------------------ 3. idempotence, repeatability

@pytest.mark.parametrize("sort_cell", [None, 1.0])
def test_filtering_twice_changes_nothing_and_runs_repeat_bit_for_bit(ctx, clouds, sort_cell):
    from nonlinear_optimizer_for_slam_amd import api
    pts, vs = clouds["outlier"], 0.5
    s = api.Scan(ctx, pts, sort_cell=sort_cell)
    f1 = s.filtered(vs)
    f2 = s.filtered(vs)
    p1, o1 = f1.points(), f1.order
    assert p1.tobytes() == f2.points().tobytes() and o1.tobytes() == f2.order.tobytes()  # repeatable
    ff = f1.filtered(vs)
    assert np.array_equal(ff.points(), p1) and np.array_equal(ff.order, o1)  # idempotent, order composed to the source
    _close(ff, f2, f1, s)
    # the room at 0.25 m: 954 605 points (a table of 2^21 entries) → 1 463, filtered again through a table of 2^12
    room = clouds["room"]
    s = api.Scan(ctx, room, sort_cell=sort_cell)
    f1 = s.filtered(0.25)
    ff = f1.filtered(0.25)
    assert len(ff) == 1463 and np.array_equal(ff.points(), f1.points()) and np.array_equal(ff.order, f1.order)
    _close(ff, f1, s)


def test_empty_scan_filters_to_an_empty_scan(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    s = api.Scan(ctx, np.zeros((0, 3)))
    f = s.filtered(0.1)
    assert len(f) == 0 and f.points().shape == (0, 3) and f.order.size == 0
    _close(f, s)


# ------------------------------------------------------------------------------ 4. the voxel store sees the same voxels

@pytest.mark.parametrize("cloud,vs", [("room", 0.1), ("room", 0.05), ("outlier", 0.5), ("outlier", 0.05)])
def test_kept_count_is_the_voxel_count_of_a_store_at_that_resolution(ctx, clouds, cloud, vs):
    from nonlinear_optimizer_for_slam_amd import api
    pts = clouds[cloud]
    s = api.Scan(ctx, pts)
    f = s.filtered(vs)
    vm = api.VoxelMap(ctx, voxel_resolution=vs)
    vm.insert(pts)
    assert len(f) == len(vm) == _truth(pts, vs).size
    _close(vm, f, s)


# ------------------------------------------------------------------------------ 5. duplicates, adversarial order

def _duplicated():
    rng = np.random.default_rng(64)
    base = rng.uniform([-30, -30, -3], [30, 30, 3], size=(20_000, 3))
    return np.repeat(base, 64, axis=0)  # every point 64 times in a row: one run per wave


@pytest.mark.parametrize("form", ["aligned", "offset", "shuffled", "interleaved"])
def test_duplicates_and_adversarial_orders_match_the_truth(ctx, form):
    """aligned: a wave holds 64 copies of one point; offset: the runs straddle wave boundaries; shuffled: the copies of a
    point are scattered over the whole cloud (every lane of a wave has a cell of its own, the minimum is found in the
    table); interleaved: a b c d a b c d …, cells recur in a wave with other cells in between."""
    pts = _duplicated()
    if form == "offset":
        pts = pts[13:]
    elif form == "shuffled":
        pts = pts[np.random.default_rng(5).permutation(pts.shape[0])]
    elif form == "interleaved":
        pts = np.tile(pts[::64].reshape(-1, 1, 4, 3), (1, 64, 1, 1)).reshape(-1, 3)
    for vs in (0.5, 2.0):
        keep = _assert_is_truth(ctx, pts, vs)
        assert keep.size <= 20_000


# ------------------------------------------------------------------------------ 6. negative cells, points on cell faces

@pytest.mark.parametrize("vs", [0.1, 0.05, 0.25, 1.0])
def test_points_on_cell_faces_negative_cells_and_negative_zero(ctx, vs):
    k = np.arange(-9, 10).astype(np.float64)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * vs  # exactly k * vs on every axis
    below, above = np.nextafter(g, -np.inf), np.nextafter(g, np.inf)
    zeros = np.array([[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]])
    rng = np.random.default_rng(11)
    inner = g + rng.uniform(0, vs, size=g.shape)
    pts = np.concatenate([g, below, zeros, above, inner, -g, g[::-1]])
    pts = pts[rng.permutation(pts.shape[0])]
    assert np.any(np.signbit(pts) & (pts == 0.0)) and pts.min() < -8 * vs
    keep = _assert_is_truth(ctx, pts, vs)
    assert keep.size < pts.shape[0]


# ------------------------------------------------------------------------------ 7. rejected calls

def test_rejected_calls_produce_no_scan_and_leave_the_source_usable(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    lib = ctx._lib
    sentinel = 12345
    rng = np.random.default_rng(23)
    pts = rng.uniform(-6, 6, size=(5000, 3))
    keep = _truth(pts, 0.5)

    def usable(s, p):
        f = s.filtered(0.5)
        k = _truth(p, 0.5) if not np.array_equal(p, pts) else keep
        assert np.array_equal(f.order, k) and np.array_equal(f.points(), p[k])
        f.close()

    # bad coordinates: the whole call is rejected
    for bad, status in ((np.nan, INVALID), (np.inf, INVALID), (-np.inf, INVALID), (0.5 * 2.0 ** 20, UNSUPPORTED),
                        (-0.5 * 2.0 ** 20 - 0.25, UNSUPPORTED)):
        p = pts.copy()
        p[3217, 1] = bad
        s = api.Scan(ctx, p)
        with pytest.raises(NosError) as err:
            s.filtered(0.5)
        assert err.value.status == status, bad
        out = ctypes.c_void_p(sentinel)
        assert lib.nos_scan_filter(s._h, ctypes.c_double(0.5), ctypes.byref(out)) == status
        assert out.value == sentinel
        assert len(s) == 5000 and np.array_equal(s.points(), p, equal_nan=True)
        if status == UNSUPPORTED:  # the same point is inside the grid of a coarser filter
            f = s.filtered(1.0)
            assert np.array_equal(f.order, _truth(p, 1.0))
            f.close()
        s.close()
    # the last addressable cells on both sides are accepted
    p = pts.copy()
    p[10], p[11] = [0.5 * (2.0 ** 20 - 1), 0.0, 0.0], [0.0, -0.5 * 2.0 ** 20, 0.0]
    s = api.Scan(ctx, p)
    usable(s, p)
    s.close()
    # bad voxel sizes, NULL arguments
    s = api.Scan(ctx, pts)
    for vs in (0.0, -0.1, np.nan, np.inf, -np.inf):
        with pytest.raises(NosError) as err:
            s.filtered(vs)
        assert err.value.status == INVALID, vs
        out = ctypes.c_void_p(sentinel)
        assert lib.nos_scan_filter(s._h, ctypes.c_double(vs), ctypes.byref(out)) == INVALID
        assert out.value == sentinel
        usable(s, pts)
    out = ctypes.c_void_p(sentinel)
    assert lib.nos_scan_filter(None, ctypes.c_double(0.5), ctypes.byref(out)) == INVALID
    assert lib.nos_scan_filter(s._h, ctypes.c_double(0.5), None) == INVALID
    assert lib.nos_scan_points(s._h, None) == INVALID
    assert out.value == sentinel
    usable(s, pts)
    s.close()


# ------------------------------------------------------------------------------ 8. downstream: odometry

def _frames(room_points):
    """Three raw frames: the room seen from three true poses (the first is the harness's, MDM/…/simple_optimization_test.cc:85-88)."""
    c, s = np.cos(0.1), np.sin(0.1)
    R1 = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    t1 = np.array([-0.2, 0.123, 0.3])
    R2, t2 = R1 @ helpers.rot_xyz(0.0, 0.0, 0.02), t1 + np.array([0.03, -0.04, 0.0])
    R3, t3 = R2 @ helpers.rot_xyz(0.005, -0.004, 0.015), t2 + np.array([0.02, 0.03, -0.01])
    return [(R.T @ (room_points - t).T).T for R, t in ((R1, t1), (R2, t2), (R3, t3))]


def _store(ctx, room_points):
    from nonlinear_optimizer_for_slam_amd import api
    vm = api.VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    vm.insert(room_points)
    return vm


def _same_run(a, b):
    poses_a, rounds_a = a
    poses_b, rounds_b = b
    assert len(poses_a) == len(poses_b) and rounds_a == rounds_b
    for pa, pb in zip(poses_a, poses_b):
        assert np.array_equal(pa.R, pb.R) and np.array_equal(pa.t, pb.t)


def _same_store(a, b):
    sa, sb = a.stats(), b.stats()
    for key in ("cells", "counts", "valid", "means", "sqrt_infos"):
        assert np.array_equal(sa[key], sb[key]), key


def test_odometry_with_the_device_filter_is_odometry_on_host_filtered_scans(ctx, room_points):
    """Both runs feed identical points in identical order to identical code: poses, round lists and the final stores are
    the same bits.  The device run filters every raw frame on the GPU and inserts the full frame; the second run gets the
    frames filtered on the host with the truth and inserts each full frame by hand."""
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    frames = _frames(room_points)
    raw = [api.Scan(ctx, p) for p in frames]
    host = [api.Scan(ctx, p[_truth(p, 0.1)]) for p in frames]
    assert all(5000 < len(h) < 60000 for h in host)
    # the device filter inside odometry, full frames inserted
    vm_a = _store(ctx, room_points)
    got = pipeline.odometry(ctx, vm_a, raw, filter_voxel_size=0.1, loss=LOSS)
    assert all(len(s) == 954605 for s in raw)  # the raw scans survive, the filtered ones were closed inside
    # by hand on a fresh store
    vm_b = _store(ctx, room_points)
    pose, poses, rounds = Pose(), [], []
    for full, small in zip(raw, host):
        snap = vm_b.snapshot()
        pose, r, _ = pipeline.scan_to_map(ctx, snap, small, initial_pose=pose, loss=LOSS)
        snap.close()
        vm_b.insert_scan(full, pose.R, pose.t)
        poses.append(Pose(pose.R, pose.t))
        rounds.append(r)
    _same_run(got, (poses, rounds))
    _same_store(vm_a, vm_b)
    assert vm_a.n_points == 4 * 954605
    assert len(got[0]) == 3 and all(len(r) >= 1 for r in got[1])
    _close(vm_a, vm_b)
    # insert_filtered=True is plain odometry on the host-filtered scans
    vm_c, vm_d = _store(ctx, room_points), _store(ctx, room_points)
    got_c = pipeline.odometry(ctx, vm_c, raw, filter_voxel_size=0.1, insert_filtered=True, loss=LOSS)
    got_d = pipeline.odometry(ctx, vm_d, host, loss=LOSS)
    _same_run(got_c, got_d)
    _same_store(vm_c, vm_d)
    assert vm_c.n_points == 954605 + sum(len(h) for h in host)
    _same_run((got_c[0][:1], got_c[1][:1]), (got[0][:1], got[1][:1]))  # the first frame meets the same map either way
    # filter_voxel_size=None is today's loop: snapshot, scan_to_map, insert the scan that was registered
    vm_e = _store(ctx, room_points)
    pose, poses, rounds = Pose(), [], []
    for small in host:
        snap = vm_e.snapshot()
        pose, r, _ = pipeline.scan_to_map(ctx, snap, small, initial_pose=pose, loss=LOSS)
        snap.close()
        vm_e.insert_scan(small, pose.R, pose.t)
        poses.append(Pose(pose.R, pose.t))
        rounds.append(r)
    _same_run(got_d, (poses, rounds))
    _same_store(vm_d, vm_e)
    _close(vm_c, vm_d, vm_e, *raw, *host)
