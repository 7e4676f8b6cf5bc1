"""Motion compensation of a scan on the device (api.Scan.deskewed / nos_scan_deskew, pipeline.odometry(sweep_times=...);
DESIGN.md §24), on the GPU.

The device result is held against 50 digits (tests/scan_deskew_inputs.py::truth) with 4 x the error a plain numpy
restatement of the rule makes on the same inputs, and at least 4 eps — the margin the project grants a device restatement
over numpy: the two differ in the rounding of sincos and in fused multiply-adds.  The error measure is
max_k |got_k - truth_k| / (max_k |p_k| + |tau| max_k |v_k|) in eps = 2^-52.

Measured on an MI355X, worst over s_ref in {0, 0.5, 1}, device (numpy restatement; smallest bound): typ 0.55 eps (1.72; 5.96),
fast 5.06 (4.64; 9.14 at s_ref 0.5, where the device had 2.37), tiny 0.49 (1.20; 4.51), thr 1.26 (2.28; 6.25), denorm 0.45
(0.45; 4), big 22.08 (21.36; 40.20 at s_ref 0.5, where the device had 10.01), pure_t 0.51 (0.51; 4).  Shapes 1 ... 100 003:
device - restatement at most 2.34 eps (granted 8.34).  The simulated sweep, skewed by up to 0.966 m, comes back to the
static scan within 1.93 eps (granted 10.3 ... 12.6).  Registration from the identity against the room store ends, in
translation and |vec q| from the true pose: static 3.618e-4 m, 1.116e-5 (outer 2); deskewed the same, 3e-17 m from the static
pose; raw 1.554e-1 m, 3.084e-2 (outer 3).  Each test prints its figures ("worst ... eps (bound ... eps)")."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import scan_deskew_inputs as di

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 6
LOSS = ("exponential", 1.0, 1.0)
EPS = di.EPS
I3, Z3 = np.eye(3), np.zeros(3)
XI = np.array([0.3, -0.2, 0.05, 0.02, -0.01, 0.15])  # the sensor's twist in the physical tests: v, then w


def _api():
    from nonlinear_optimizer_for_slam_amd import api
    return api


def _deskew(ctx, p, s, twist, s_ref=1.0, **scan_kwargs):
    """→ (points, order) of Scan(p).deskewed(s, twist, s_ref)."""
    scan = _api().Scan(ctx, p, **scan_kwargs)
    out = scan.deskewed(s, twist, s_ref)
    got, order = out.points(), out.order
    out.close()
    scan.close()
    return got, order


def _scale(p, s, s_ref, twist):
    """[n] the denominator of the error measure."""
    return np.max(np.abs(p), axis=1) + np.abs(s - s_ref) * float(np.max(np.abs(twist[:3])))


# ------------------------------------------------------------------------------ 1. against 50 digits

@pytest.mark.parametrize("name", list(di.FAMILIES))
def test_device_result_against_50_digits(ctx, name):
    for s_ref in di.S_REFS:
        c = di.case(name, s_ref)
        got, _ = _deskew(ctx, c["p"], c["s"], c["twist"], s_ref)
        worst = float(np.max(di.errors_eps(got, c["truth"], c["p"], c["s"], s_ref, c["twist"])))
        bound = max(4.0 * c["restate_eps"], 4.0)
        print("%s at s_ref %.1f: worst %.2f eps (bound %.2f eps; restate %.2f eps)" % (name, s_ref, worst, bound, c["restate_eps"]))
        assert worst <= bound
        if name == "thr":
            assert di.thr_straddles(c["s"], s_ref)


# ------------------------------------------------------------------------------ 2. shapes

SHAPES = (0, 1, 63, 64, 65, 255, 256, 257, 100_003)


@pytest.fixture(scope="module")
def long_cloud():
    """100 003 points with times, the numpy restatement of their deskew, and the restatement's worst error on the first
    300, the last 300 and 400 random points (every shorter shape is a prefix, so all of its points are in the subset)."""
    rng = np.random.default_rng(77)
    n = SHAPES[-1]
    p = rng.uniform(-100.0, 100.0, size=(n, 3))
    s = rng.uniform(0.0, 1.0, size=n)
    twist = di.twist_of("typ")
    re = di.restate(p, s, 1.0, twist)
    sub = np.unique(np.concatenate([np.arange(300), np.arange(n - 300, n), rng.integers(300, n - 300, size=400)]))
    want = di.truth(p[sub], s[sub], 1.0, twist)
    e_r = float(np.max(di.errors_eps(re[sub], want, p[sub], s[sub], 1.0, twist)))
    return {"p": p, "s": s, "twist": twist, "restate": re, "restate_eps": e_r}


@pytest.mark.parametrize("n", SHAPES)
def test_every_point_of_every_shape_is_written_once(ctx, long_cloud, n):
    p, s, twist = long_cloud["p"][:n], long_cloud["s"][:n], long_cloud["twist"]
    got, order = _deskew(ctx, p, s, twist)
    assert got.shape == (n, 3) and np.array_equal(order, np.arange(n))
    if n == 0:
        return
    allowed = 5.0 * long_cloud["restate_eps"] * EPS * _scale(p, s, 1.0, twist)  # 4 x for the device + 1 x for the restatement
    off = np.max(np.abs(got - long_cloud["restate"][:n]), axis=1)
    print("n = %d: device - restate worst %.2f eps (bound %.2f eps)" % (
        n, float(np.max(off / (EPS * _scale(p, s, 1.0, twist)))), 5.0 * long_cloud["restate_eps"]))
    assert np.all(off <= allowed)
    # a cell-sorted copy goes through the gather: a point written twice or not at all shows here too
    if n > 1:
        got_sorted, order = _deskew(ctx, p, s, twist, sort_cell=10.0)
        assert np.array_equal(np.sort(order), np.arange(n)) and np.array_equal(got_sorted, got[order])


# ------------------------------------------------------------------------------ 3. exact properties

def test_points_at_the_reference_instant_and_under_a_zero_twist_come_back_equal(ctx):
    api = _api()
    p, s, twist = di.family("fast")
    p = p.copy()
    p[:4] = [[-0.0, 0.0, -0.0], [0.0, 0.0, 0.0], [1e-310, -1e-310, 5e-324], [1e300, -1e300, 1e-300]]
    for s_ref in (0.0, 0.5, 1.0, 0.3):
        got, _ = _deskew(ctx, p, np.full(p.shape[0], s_ref), twist, s_ref)
        assert np.array_equal(got, p), s_ref  # == : a -0.0 may come back as +0.0
    got, _ = _deskew(ctx, p, s, np.zeros(6), 1.0)
    assert np.array_equal(got, p)
    # every third time at the reference instant: those rows are equal, the others move
    mixed = s.copy()
    mixed[::3] = 0.5
    mixed[1::3] = np.where(mixed[1::3] == 0.5, 0.25, mixed[1::3])
    mixed[2::3] = np.where(mixed[2::3] == 0.5, 0.75, mixed[2::3])
    scan = api.Scan(ctx, p)
    a = scan.deskewed(mixed, twist, 0.5)
    b = scan.deskewed(mixed, twist, 0.5)
    pa, pb = a.points(), b.points()
    assert np.array_equal(pa[::3], p[::3])
    moved = np.any(pa != p, axis=1)
    assert not moved[::3].any() and moved[1::3].all() and moved[2::3].all()
    assert pa.tobytes() == pb.tobytes() and a.order.tobytes() == b.order.tobytes()  # two runs, the same bytes
    assert len(scan) == p.shape[0] and np.array_equal(scan.points(), p) and np.array_equal(scan.order, np.arange(p.shape[0]))
    for h in (a, b, scan):
        h.close()


# ------------------------------------------------------------------------------ 4. order

def test_sorted_and_filtered_scans_take_the_source_arrays_times(ctx):
    api = _api()
    rng = np.random.default_rng(4)
    pts = rng.uniform([-30, -30, -3], [30, 30, 3], size=(20_000, 3))
    times = rng.uniform(0.0, 1.0, size=20_000)
    plain, _ = _deskew(ctx, pts, times, XI)
    for make in (lambda: api.Scan(ctx, pts, sort_cell=1.0), lambda: api.Scan(ctx, pts, filter_voxel=0.5),
                 lambda: api.Scan(ctx, pts, filter_voxel=0.5, sort_cell=1.0)):
        src = make()
        order = src.order
        assert not np.array_equal(order, np.arange(order.size))
        before = src.points()
        d = src.deskewed(times, XI)
        assert len(d) == len(src) and np.array_equal(d.order, order)
        assert np.array_equal(d.points(), plain[order])  # bit for bit
        assert np.array_equal(src.points(), before) and np.array_equal(src.order, order)  # the source is unchanged
        d.close()
        src.close()
    raw = api.Scan(ctx, pts)
    f = raw.filtered(0.5)
    assert 0 < len(f) < 20_000  # its order indexes a times array longer than the scan
    d = f.deskewed(times, XI)
    assert np.array_equal(d.order, f.order) and np.array_equal(d.points(), plain[f.order])
    # a deskewed scan is a scan like any other: filter, sort, match, insert
    ff = d.filtered(2.0)
    assert 0 < len(ff) < len(d) and np.all(np.isin(ff.order, f.order))
    d.sort_by_cell(1.0)
    assert np.array_equal(np.sort(d.order), f.order) and np.array_equal(d.points(), plain[d.order])
    vm = api.VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    vm.insert_scan(d, I3, Z3)
    assert vm.n_points == len(d) and len(vm) > 0
    ds, n_matches = vm.match(d, I3, Z3)
    assert len(ds) == 2 * len(d) and 0 < n_matches <= 2 * len(d)
    for h in (ds, vm, ff, d, f, raw):
        h.close()


# ------------------------------------------------------------------------------ 5. - 7. the room, seen while moving

def _true_pose():
    c, s = np.cos(0.1), np.sin(0.1)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.array([-0.2, 0.123, 0.3])  # tests/test_voxel_map_match.py::room


@pytest.fixture(scope="module")
def room():
    pts = scene.generate_global_points()
    return {"points": pts, "filtered": scene.filter_points(pts, 0.1)}


def _room_store(ctx, room):
    vm = _api().VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    for b in np.array_split(room["points"], 8):
        vm.insert(b)
    return vm


def _sweep(room, R, t, s_ref, seed, twist=XI):
    """The room seen from a sensor whose pose at s_ref is (R, t) and which moves with `twist`: → (static scan q at s_ref,
    skewed scan p as measured, times).  p_i = Exp(-tau_i xi) q_i, by the numpy restatement with the negated twist."""
    q = (R.T @ (room["filtered"] - t).T).T
    times = np.random.default_rng(seed).uniform(0.0, 1.0, size=q.shape[0])
    return q, di.restate(q, times, s_ref, -twist), times


@pytest.mark.parametrize("s_ref", di.S_REFS)
def test_deskewing_a_simulated_sweep_gives_the_static_scan(ctx, room, s_ref):
    """Sign and convention: a wrong sign or a swapped v / w block is off by decimetres."""
    R, t = _true_pose()
    q, p, times = _sweep(room, R, t, s_ref, 5)
    assert np.max(np.linalg.norm(p - q, axis=1)) > 0.1  # the skew is decimetres
    got, _ = _deskew(ctx, p, times, XI, s_ref)
    sub = np.arange(0, p.shape[0], 20)
    want = di.truth(p[sub], times[sub], s_ref, XI)
    e_r = float(np.max(di.errors_eps(di.restate(p[sub], times[sub], s_ref, XI), want, p[sub], times[sub], s_ref, XI)))
    bound = 2.0 * max(4.0 * e_r, 4.0)  # the bound of test 1, once for the simulation's own rounding and once for the device's
    off = np.max(np.abs(got - q), axis=1) / (EPS * _scale(p, times, s_ref, XI))
    print("s_ref %.1f: deskewed - static worst %.2f eps (bound %.2f eps; restate %.2f eps), skew up to %.3f m" % (
        s_ref, float(np.max(off)), bound, e_r, float(np.max(np.linalg.norm(p - q, axis=1)))))
    assert np.all(off <= bound)


def _pose_distance(pose, R, t):
    from nonlinear_optimizer_for_slam_amd import pipeline
    return float(np.linalg.norm(pose.t - t)), pipeline._quat_vec_norm(pose.R.T @ R)


def test_deskewing_helps_the_registration_it_was_built_for(ctx, room):
    from nonlinear_optimizer_for_slam_amd import pipeline
    api = _api()
    R, t = _true_pose()
    q, p, times = _sweep(room, R, t, 1.0, 5)
    vm = _room_store(ctx, room)
    static, raw = api.Scan(ctx, q), api.Scan(ctx, p)
    deskewed = raw.deskewed(times, XI, 1.0)
    pose_s, _, outer_s = pipeline.scan_to_map(ctx, vm, static, loss=LOSS)
    pose_d, _, outer_d = pipeline.scan_to_map(ctx, vm, deskewed, loss=LOSS)
    pose_r, _, outer_r = pipeline.scan_to_map(ctx, vm, raw, loss=LOSS)
    for h in (deskewed, raw, static, vm):
        h.close()
    ds, dd, dr = _pose_distance(pose_s, R, t), _pose_distance(pose_d, R, t), _pose_distance(pose_r, R, t)
    between = _pose_distance(pose_d, pose_s.R, pose_s.t)
    print("distance from the true pose (translation, |vec q|): static %.3e %.3e (outer %d), deskewed %.3e %.3e (outer %d), "
          "raw %.3e %.3e (outer %d); deskewed from static %.3e %.3e" % (ds + (outer_s,) + dd + (outer_d,) + dr + (outer_r,) + between))
    assert outer_s < 10  # the static route meets the stopping test
    assert between[0] < 1e-4 and between[1] < 1e-4  # ten times the outer loop's own threshold
    assert dr[0] > dd[0] and dr[1] > dd[1]  # the skew costs accuracy, the deskew gives it back


N_FRAMES = 6


@pytest.fixture(scope="module")
def frames(room):
    """Six sweeps of the room under the constant twist XI: the pose at frame k's reference instant (1.0) is
    T_ref Exp(k XI).  → (skewed point arrays, time arrays)."""
    from nonlinear_optimizer_for_slam_amd import pipeline
    R0, t0 = _true_pose()
    pts, times = [], []
    for k in range(N_FRAMES):
        e = pipeline.twist_pose(k * XI)
        _, p, s = _sweep(room, R0 @ e.R, R0 @ e.t + t0, 1.0, 100 + k)
        pts.append(p)
        times.append(s)
    return pts, times


def _odometry_store(ctx, room):
    vm = _api().VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    vm.insert(room["points"])
    return vm


def _by_hand(ctx, vm, scans, times, filter_voxel_size=None):
    """The loop odometry(sweep_times=times) stands for, written out (times=None: without the deskew)."""
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    pose, poses, rounds = Pose(), [], []
    for k, scan in enumerate(scans):
        used = scan
        if times is not None:
            twist = pipeline.pose_twist(poses[k - 2], poses[k - 1]) if k >= 2 else np.zeros(6)
            used = scan.deskewed(times[k], twist)
        registered = used if filter_voxel_size is None else used.filtered(filter_voxel_size)
        pose, r, _ = pipeline.scan_to_map(ctx, vm, registered, initial_pose=pose, loss=LOSS)
        vm.insert_scan(used, pose.R, pose.t)
        if registered is not used:
            registered.close()
        if used is not scan:
            used.close()
        poses.append(Pose(pose.R, pose.t))
        rounds.append(r)
    return poses, rounds


def _same_run(a, b):
    assert len(a[0]) == len(b[0]) == N_FRAMES and a[1] == b[1]
    for pa, pb in zip(a[0], b[0]):
        assert np.array_equal(pa.R, pb.R) and np.array_equal(pa.t, pb.t)


def _same_store(a, b):
    sa, sb = a.stats(), b.stats()
    for key in ("cells", "counts", "valid", "means", "sqrt_infos"):
        assert np.array_equal(sa[key], sb[key]), key


@pytest.mark.parametrize("route", ["deskew", "deskew_filter_live", "plain"])
def test_odometry_with_sweep_times_is_the_loop_written_out(ctx, room, frames, monkeypatch, route):
    from nonlinear_optimizer_for_slam_amd import pipeline
    api = _api()
    pts, times = frames
    scans = [api.Scan(ctx, p) for p in pts]
    made = []  # every scan odometry makes on the way, kept alive so that only an explicit close() can close it
    for method in ("deskewed", "filtered"):
        inner = getattr(api.Scan, method)

        def keep(self, *args, _inner=inner, **kwargs):
            out = _inner(self, *args, **kwargs)
            made.append(out)
            return out
        monkeypatch.setattr(api.Scan, method, keep)
    kwargs = {"deskew": dict(sweep_times=times), "deskew_filter_live": dict(sweep_times=times, filter_voxel_size=0.3, live_match=True),
              "plain": {}}[route]
    vm_a, vm_b = _odometry_store(ctx, room), _odometry_store(ctx, room)
    got = pipeline.odometry(ctx, vm_a, scans, loss=LOSS, **kwargs)
    n_made = len(made)
    assert n_made == {"deskew": N_FRAMES, "deskew_filter_live": 2 * N_FRAMES, "plain": 0}[route]
    assert all(s._h is None for s in made)  # no scan handle is left open
    monkeypatch.undo()
    want = _by_hand(ctx, vm_b, scans, None if route == "plain" else times, kwargs.get("filter_voxel_size"))
    _same_run(got, want)
    _same_store(vm_a, vm_b)
    assert all(len(r) >= 1 for r in got[1])
    if route != "plain":  # the constant-velocity twist is used from the third frame on: the poses differ from the plain run's
        vm_c = _odometry_store(ctx, room)
        plain = pipeline.odometry(ctx, vm_c, scans, loss=LOSS, **{k: v for k, v in kwargs.items() if k != "sweep_times"})
        assert any(not np.array_equal(a.t, b.t) for a, b in zip(got[0], plain[0]))
        vm_c.close()
    for s, p in zip(scans, pts):  # the caller's scans are still usable and unchanged
        assert len(s) == p.shape[0] and np.array_equal(s.points(), p)
        s.close()
    vm_a.close()
    vm_b.close()


def test_an_exception_inside_a_frame_still_closes_the_deskewed_scan(ctx, room, frames, monkeypatch):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    api = _api()
    pts, times = frames
    scans = [api.Scan(ctx, p) for p in pts[:2]]
    made = []
    inner = api.Scan.deskewed

    def keep(self, *args, **kwargs):
        out = inner(self, *args, **kwargs)
        made.append(out)
        return out
    monkeypatch.setattr(api.Scan, "deskewed", keep)
    vm = _odometry_store(ctx, room)
    with pytest.raises(NosError):  # filter_voxel_size < 0 is rejected by the filter, after the deskew
        pipeline.odometry(ctx, vm, scans, sweep_times=times[:2], filter_voxel_size=-1.0, loss=LOSS)
    assert len(made) == 1 and made[0]._h is None
    for h in scans + [vm]:
        h.close()


# ------------------------------------------------------------------------------ 8. rejections

def test_rejected_calls_write_nothing_and_leave_the_context_usable(ctx):
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    api = _api()
    lib = ctx._lib
    sentinel = 12345
    rng = np.random.default_rng(8)
    pts = rng.uniform(-20.0, 20.0, size=(5000, 3))
    times = rng.uniform(0.0, 1.0, size=5000)
    want = di.restate(pts, times, 1.0, XI)
    scan = api.Scan(ctx, pts)
    filtered = scan.filtered(2.0)
    forder = filtered.order
    assert 0 < forder.size < 5000 and forder[-1] > forder.size

    def dp(a):
        return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def rejected(s, tm, twist, s_ref, status, text=None):
        with pytest.raises(NosError) as err:
            s.deskewed(tm, twist, s_ref)
        assert err.value.status == status
        if text is not None:
            assert text in str(err.value), str(err.value)
        tm = np.ascontiguousarray(tm, dtype=np.float64)
        twist = np.ascontiguousarray(twist, dtype=np.float64)
        out = ctypes.c_void_p(sentinel)
        assert lib.nos_scan_deskew(s._h, dp(tm), tm.size, ctypes.c_double(s_ref), dp(twist), ctypes.byref(out)) == status
        assert out.value == sentinel  # the handle it would have written is untouched
        d = scan.deskewed(times, XI)  # the context is usable: a valid call straight after
        assert np.max(np.abs(d.points() - want)) < 1e-12
        d.close()

    rejected(scan, times[:4999], XI, 1.0, INVALID, "position 4999")  # times shorter than the scan
    cut = int(forder[-1])  # the last kept point's original index is the first one without a time stamp
    rejected(filtered, times[:cut], XI, 1.0, INVALID, "position %d" % (forder.size - 1))
    bad = times.copy()
    bad[int(forder[7])] = np.nan
    rejected(filtered, bad, XI, 1.0, INVALID, "position 7")  # a NaN time at a referenced index
    rejected(scan, bad, XI, 1.0, INVALID, "position %d" % int(forder[7]))
    bad[int(forder[7])] = np.inf
    rejected(scan, bad, XI, 1.0, INVALID, "position %d" % int(forder[7]))
    for k in (0, 4):
        twist = XI.copy()
        twist[k] = np.inf if k == 0 else np.nan
        rejected(scan, times, twist, 1.0, INVALID)  # an inf / a NaN in the twist
    rejected(scan, times, XI, np.nan, INVALID)  # a NaN reference_time
    rejected(scan, times, XI, np.inf, INVALID)
    # NULL arguments
    out = ctypes.c_void_p(sentinel)
    twist = XI.copy()
    assert lib.nos_scan_deskew(scan._h, None, 5000, ctypes.c_double(1.0), dp(twist), ctypes.byref(out)) == INVALID
    assert lib.nos_scan_deskew(scan._h, dp(times), 5000, ctypes.c_double(1.0), None, ctypes.byref(out)) == INVALID
    assert lib.nos_scan_deskew(scan._h, dp(times), 5000, ctypes.c_double(1.0), dp(twist), None) == INVALID
    assert out.value == sentinel
    # a NaN at an index that no stored point refers to is accepted
    unused = np.setdiff1d(np.arange(5000), forder)
    ok = times.copy()
    ok[unused] = np.nan
    d = filtered.deskewed(ok, XI)
    assert np.max(np.abs(d.points() - want[forder])) < 1e-12 and np.array_equal(d.order, forder)
    d.close()
    # an empty scan takes no times at all
    empty = api.Scan(ctx, np.zeros((0, 3)))
    d = empty.deskewed(np.zeros(0), XI)
    assert len(d) == 0 and d.points().shape == (0, 3) and d.order.size == 0
    for h in (d, empty, filtered, scan):
        h.close()


def test_a_two_device_context_is_rejected(ctx):
    """The deskew needs a single-device context, as the scan itself does: nos_scan_create already refuses such a context
    with NOS_ERR_UNSUPPORTED, so no scan can reach nos_scan_deskew's own check of it through the public interface."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    from nonlinear_optimizer_for_slam_amd import Context
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    two = Context((0, 1))
    with pytest.raises(NosError) as err:
        _api().Scan(two, np.zeros((4, 3)))
    assert err.value.status == UNSUPPORTED
    two.close()
    d, _ = _deskew(ctx, np.ones((4, 3)), np.zeros(4), XI, 0.0)  # the single-device context is as usable as before
    assert np.array_equal(d, np.ones((4, 3)))
