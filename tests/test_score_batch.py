"""Pose scoring on the GPU (api.score_batch / nos_ndt_score_batch / nos_voxel_map_score_batch): per
(scan, pose) the number of matches, the points with a match and the cost Σ ρ, in one call and with nothing written in
between — against the route that exists already, match(..., "f64") + accumulate6(...)[27], and against the CPU oracle.

The maps: an NdtMap of 300 given means and sqrt-informations, and a VoxelMap (400 cells) filled by two inserts.  Scans
are seeded.  C = api.SCORE_CHUNK_POINTS is the number of points one workgroup sums; the sizes straddle the block (256)
and the chunk.

Bounds.  Terms are the existing route's bits (test 1: a sum of two terms has one order).  For more terms both routes
add the same m = 2 · points non-negative fp64 terms (absent slots add +0) in different orders; each order errs by at most
(m − 1) · 2⁻⁵³ · Σ, so |Δ| ≤ m · 2⁻⁵² · cost: derived, not measured.  The CPU oracle evaluates the S form in numpy's
order: RTOL_F64 = 1e-10 of tests/test_gpu_parity.py.

Not reachable from a test: NOS_ERR_UNSUPPORTED for a multi-device context (neither a map nor a scan can be created on
one) and NOS_ERR_HIP for a `broken` store (only a failed merge sets it)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import helpers

pytestmark = pytest.mark.gpu

LOSSES = {"none": None, "exponential": ("exponential", 1.0, 1.0), "huber": ("huber", 0.7)}
POSE = (helpers.rot_xyz(0.01, -0.02, 0.05), np.array([0.1, -0.2, 0.05]))
RADIUS_SQ = 1.0
RTOL_F64 = 1e-10
GUARD = 1.0 / 1024.0  # of a voxel edge (nos::kVoxelMatchGuard)
INVALID, HIP, UNSUPPORTED = 1, 3, 6
LO, HI = np.array([-5.0, -5.0, -1.5]), np.array([5.0, 5.0, 1.5])


def _api():
    from nonlinear_optimizer_for_slam_amd import api
    return api


def _sizes():
    C = _api().SCORE_CHUNK_POINTS
    return [1, 2, 255, 256, 257, C - 1, C, C + 1, 3 * C + 5]


def _given_voxels():
    rng = np.random.default_rng(1201)
    means = rng.uniform(LO, HI, size=(300, 3))
    S = rng.normal(0.0, 0.3, size=(300, 3, 3)) + np.eye(3) * rng.uniform(0.5, 3.0, size=(300, 3))[:, None, :]
    return means, S.reshape(300, 9)


def _fill(vm, seed=1202):
    rng = np.random.default_rng(seed)
    for _ in range(2):
        vm.insert(rng.uniform(LO, HI, size=(30_000, 3)))


def _guard_holds(vm, res=1.0):
    st = vm.stats()
    ok = st["valid"]
    lo = st["cells"][ok] * res
    m = st["means"][ok]
    assert np.all(m >= lo - GUARD * res) and np.all(m <= lo + res + GUARD * res)


@pytest.fixture(scope="module")
def maps(ctx):
    """kind → (map handle, means, sqrt_infos [V, 9], valid) — made once, only read by the tests that share them."""
    api = _api()
    means, S = _given_voxels()
    ndt = api.NdtMap(ctx, means, S, search_radius_sq=RADIUS_SQ)
    vm = api.VoxelMap(ctx, 1.0, RADIUS_SQ)
    _fill(vm)
    _guard_holds(vm)
    st = vm.stats()
    assert 200 <= len(vm) <= 400 and st["valid"].sum() >= 200
    out = {"ndt": (ndt, means, S, None), "voxel": (vm, st["means"], st["sqrt_infos"].reshape(-1, 9), st["valid"])}
    yield out
    ndt.close()
    vm.close()


def _points(n, seed):
    return np.random.default_rng(seed).uniform(LO - 1.0, HI + 1.0, size=(n, 3))


def _existing_route(m, sc, pose, k, losses):
    """match(..., "f64") + accumulate6 → (n_matches, {loss name: cost})"""
    ds, n = m.match(sc, pose[0], pose[1], k, "f64")
    costs = {name: float(ds.accumulate6(pose[0], pose[1], LOSSES[name])[27]) for name in losses}
    ds.close()
    return n, costs


def _matched_points(m, sc, pose, k):
    ds, _ = m.match_indexed(sc, pose[0], pose[1], k, "f64", sort_by_voxel=False)
    ids = ds.ids()
    ds.close()
    return int(np.count_nonzero(ids[0] >= 0))


def _bits(x):
    return np.float64(x).tobytes()


# ------------------------------------------------------------------------------ 1. the terms are the existing route's bits

@pytest.mark.parametrize("kind", ["ndt", "voxel"])
def test_the_cost_of_one_point_with_two_matches_is_the_existing_routes_bits(ctx, maps, kind):
    api = _api()
    m = maps[kind][0]
    sc = api.Scan(ctx, np.array([[0.31, -0.42, 0.17]]))
    n, want = _existing_route(m, sc, POSE, 2, LOSSES)
    assert n == 2, "the test needs a point with two matches"
    for name, loss in LOSSES.items():
        matches, points, cost = m.score(sc, POSE[0], POSE[1], loss)
        print(kind, name, "cost", repr(cost), "existing route", repr(want[name]))
        assert matches == 2 and points == 1
        assert cost > 0.0
        assert _bits(cost) == _bits(want[name]), (name, cost, want[name])
    sc.close()


# ------------------------------------------------------------------------------ 2. sizes around the block and the chunk

@pytest.mark.parametrize("kind", ["ndt", "voxel"])
@pytest.mark.parametrize("k", [1, 2])
def test_counts_are_exact_and_the_cost_is_within_the_reordering_bound_at_every_size(ctx, maps, kind, k):
    api = _api()
    m = maps[kind][0]
    sizes = _sizes()
    scans = [api.Scan(ctx, _points(n, 1300 + i)) for i, n in enumerate(sizes)]
    B = len(scans)
    R = np.tile(POSE[0].reshape(9), (B, 1))
    t = np.tile(POSE[1], (B, 1))
    got = {name: api.score_batch(m, scans, R, t, loss, max_neighbors=k) for name, loss in LOSSES.items()}
    for i, (n, sc) in enumerate(zip(sizes, scans)):
        n_matches, want = _existing_route(m, sc, POSE, k, LOSSES)
        n_points = _matched_points(m, sc, POSE, k)
        for name in LOSSES:
            row = got[name][i]
            assert int(row["matches"]) == n_matches, (n, name)
            assert int(row["matched_points"]) == n_points, (n, name)
            bound = 2 * n * 2.0 ** -52 * want[name]
            delta = abs(float(row["cost"]) - want[name])
            print(kind, k, n, name, "cost %.17g existing %.17g delta %.3g bound %.3g" % (row["cost"], want[name], delta, bound))
            assert delta <= bound, (n, name, delta, bound)
        if n >= 255:
            assert n_matches > 0 and 0 < n_points <= n
    for sc in scans:
        sc.close()


# ------------------------------------------------------------------------------ 3. the CPU oracle

def _decisions_are_clear(means, valid, pts, pose, radius_sq):
    """No candidate's squared distance within 1e-9 · r² of r², and the second and third nearest further apart than that:
    then the set of matches of every point is the same in any rounding of the warp and of the distance."""
    ok = np.ones(len(means), dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    q = pts @ pose[0].T + pose[1]
    d = ((q[:, None, :] - means[ok][None, :, :]) ** 2).sum(axis=2)
    margin = 1e-9 * radius_sq
    assert np.abs(d - radius_sq).min() > margin
    d.sort(axis=1)
    assert (d[:, 2] - d[:, 1]).min() > margin


@pytest.mark.parametrize("kind", ["ndt", "voxel"])
def test_scores_agree_with_the_cpu_oracle(ctx, oracle, maps, kind):
    api = _api()
    m, means, S, valid = maps[kind]
    pts = _points(700, 1400)
    _decisions_are_clear(means, valid, pts, POSE, RADIUS_SQ)
    sc = api.Scan(ctx, pts)
    for k in (1, 2):
        planes, n_matches, idx = scene.match_point_cloud(means, S, valid, pts, POSE[0], POSE[1], RADIUS_SQ, k)
        assert n_matches > 300
        for name, loss in LOSSES.items():
            want = float(oracle.ndt6_accumulate(planes, POSE[0], POSE[1], loss)[27])
            matches, points, cost = m.score(sc, POSE[0], POSE[1], loss, max_neighbors=k)
            print(kind, k, name, "cost %.17g oracle %.17g" % (cost, want))
            assert matches == n_matches
            assert points == int(np.count_nonzero(idx[:, 0] >= 0))
            assert abs(cost - want) <= RTOL_F64 * want, (name, cost, want)
    sc.close()


# ------------------------------------------------------------------------------ 4. a row does not depend on the batch

@pytest.mark.parametrize("kind", ["ndt", "voxel"])
def test_a_row_is_the_same_bytes_alone_in_a_batch_and_from_run_to_run(ctx, maps, kind):
    api = _api()
    m = maps[kind][0]
    C = api.SCORE_CHUNK_POINTS
    pool = [api.Scan(ctx, _points(n, 1500 + i)) for i, n in enumerate([0, 3 * C + 5, 300, C + 1, 1, 2 * C, 77])]
    rng = np.random.default_rng(1501)
    B = 70
    scans = [pool[(3 * i + 2) % len(pool)] for i in range(B)]
    assert any(len(s) == 0 for s in scans) and any(len(s) == 3 * C + 5 for s in scans)
    assert len(scans[37]) == 3 * C + 5  # the row looked at spans several chunks
    R = np.array([helpers.rot_xyz(*rng.normal(0, 0.03, size=3)).reshape(9) for _ in range(B)])
    t = rng.normal(0, 0.2, size=(B, 3))
    loss = LOSSES["exponential"]
    alone = api.score_batch(m, [scans[37]], R[37:38], t[37:38], loss)
    first = api.score_batch(m, scans, R, t, loss)
    again = api.score_batch(m, scans, R, t, loss)
    assert first[37]["matches"] > 1000 and first[37]["cost"] > 0.0
    assert alone[0].tobytes() == first[37].tobytes()
    assert first.tobytes() == again.tobytes()
    # the same problem at another position, among other rows
    moved = api.score_batch(m, [pool[2], scans[37]], np.stack([R[0], R[37]]), np.stack([t[0], t[37]]), loss)
    assert moved[1].tobytes() == first[37].tobytes()
    empty_rows = [i for i in range(B) if len(scans[i]) == 0]
    for i in empty_rows:
        assert first[i]["matches"] == 0 and first[i]["matched_points"] == 0 and first[i]["cost"] == 0.0
    for sc in pool:
        sc.close()


# ------------------------------------------------------------------------------ 5. the live store and its snapshot

def test_live_store_rows_equal_snapshot_rows_and_the_store_is_untouched(ctx):
    api = _api()
    C = api.SCORE_CHUNK_POINTS
    vm = api.VoxelMap(ctx, 1.0, RADIUS_SQ)
    _fill(vm, seed=1600)
    scans = [api.Scan(ctx, _points(n, 1601 + i)) for i, n in enumerate([3 * C + 5, 500, 1])]
    rng = np.random.default_rng(1602)
    B = 12
    batch = [scans[i % 3] for i in range(B)]
    R = np.array([helpers.rot_xyz(*rng.normal(0, 0.03, size=3)).reshape(9) for _ in range(B)])
    t = rng.normal(0, 0.2, size=(B, 3))

    def compare():
        _guard_holds(vm)
        before = (vm.memory(), len(vm), vm.n_valid, vm.n_points)
        total = 0
        for name, loss in LOSSES.items():
            for k in (1, 2):
                live = api.score_batch(vm, batch, R, t, loss, max_neighbors=k)
                assert (vm.memory(), len(vm), vm.n_valid, vm.n_points) == before
                snap = vm.snapshot()
                want = api.score_batch(snap, batch, R, t, loss, max_neighbors=k)
                snap.close()
                assert live.tobytes() == want.tobytes(), (name, k)
                total += int(live["matches"].sum())
        return total

    after_insert = compare()
    assert after_insert > 1000
    assert vm.prune(center=(1.0, -1.0, 0.0), half_extent=(3.0, 2.5, 2.0)) > 0
    after_prune = compare()
    assert 0 < after_prune < after_insert
    for h in scans + [vm]:
        h.close()


# ------------------------------------------------------------------------------ 6. rejections and what is not an error

def _call(name, map_h, scan_hs, n, R, t, loss, k, rows):
    from nonlinear_optimizer_for_slam_amd import _lib
    lib = _lib.hip_lib()
    handles = (ctypes.c_void_p * max(len(scan_hs), 1))(*scan_hs) if scan_hs is not None else None
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p) if a is not None else None  # noqa: E731
    sp = rows.ctypes.data_as(ctypes.POINTER(_lib.NosPoseScore)) if rows is not None else None
    l = ctypes.byref(loss) if loss is not None else None
    return getattr(lib, name)(map_h, handles, n, dp(R), dp(t), l, k, sp)


def _prefilled(n):
    rows = np.zeros(n, dtype=_api().SCORE_DTYPE)
    rows["matches"], rows["matched_points"], rows["cost"], rows["reserved"] = 11, 12, 13.5, 14.5
    return rows


@pytest.mark.parametrize("kind", ["ndt", "voxel"])
def test_rejected_calls_leave_the_scores_untouched(ctx, maps, kind):
    from nonlinear_optimizer_for_slam_amd import Context, _lib
    api = _api()
    name = {"ndt": "nos_ndt_score_batch", "voxel": "nos_voxel_map_score_batch"}[kind]
    m = maps[kind][0]
    sc = api.Scan(ctx, _points(10, 1700))
    other_ctx = Context((0,))
    foreign = api.Scan(other_ctx, _points(10, 1701))
    R = np.tile(np.eye(3).reshape(9), (2, 1))
    t = np.zeros((2, 3))
    exp = _lib.NosLoss(_lib.NOS_LOSS_EXPONENTIAL, 0, 1.0, 1.0)
    rows = _prefilled(2)
    untouched = rows.tobytes()
    both = [sc._h, sc._h]
    cases = [
        (INVALID, (m._h, None, 2, R, t, exp, 2, rows)),            # NULL scans
        (INVALID, (m._h, both, 2, None, t, exp, 2, rows)),         # NULL R
        (INVALID, (m._h, both, 2, R, None, exp, 2, rows)),         # NULL t
        (INVALID, (m._h, both, 2, R, t, exp, 2, None)),            # NULL scores
        (INVALID, (None, both, 2, R, t, exp, 2, rows)),            # NULL map
        (INVALID, (m._h, [sc._h, None], 2, R, t, exp, 2, rows)),   # a NULL scan
        (INVALID, (m._h, both, -1, R, t, exp, 2, rows)),           # n_problems < 0
        (INVALID, (m._h, [sc._h, foreign._h], 2, R, t, exp, 2, rows)),  # a scan of another context
        (INVALID, (m._h, both, 2, R, t, _lib.NosLoss(7, 0, 1.0, 1.0), 2, rows)),  # an unknown loss kind
        (UNSUPPORTED, (m._h, both, 2, R, t, exp, 0, rows)),
        (UNSUPPORTED, (m._h, both, 2, R, t, exp, 3, rows)),
    ]
    for status, args in cases:
        assert _call(name, *args) == status, args[1:]
        assert rows.tobytes() == untouched
    if kind == "voxel":  # 2 r / resolution + 2 = 10 cells per axis
        wide = api.VoxelMap(ctx, 0.25, RADIUS_SQ)
        wide.insert(_points(1000, 1702))
        assert _call(name, wide._h, both, 2, R, t, exp, 2, rows) == UNSUPPORTED
        assert rows.tobytes() == untouched
        with pytest.raises(_lib.NosError) as err:
            api.score_batch(wide, [sc], R[:1], t[:1], LOSSES["exponential"])
        assert err.value.status == UNSUPPORTED
        wide.close()
    # through the Python interface: a status becomes NosError
    with pytest.raises(_lib.NosError) as err:
        api.score_batch(m, [sc], R[:1], t[:1], LOSSES["exponential"], max_neighbors=3)
    assert err.value.status == UNSUPPORTED
    foreign.close()
    other_ctx.close()
    sc.close()


def test_no_problems_an_empty_scan_and_an_empty_map_are_not_errors(ctx, maps):
    api = _api()
    sc = api.Scan(ctx, _points(300, 1800))
    empty_scan = api.Scan(ctx, np.zeros((0, 3)))
    R = np.tile(POSE[0].reshape(9), (2, 1))
    t = np.tile(POSE[1], (2, 1))
    empty_store = api.VoxelMap(ctx, 1.0, RADIUS_SQ)
    empty_map = api.NdtMap(ctx, np.zeros((0, 3)), np.zeros((0, 9)), search_radius_sq=RADIUS_SQ)
    for kind, name in (("ndt", "nos_ndt_score_batch"), ("voxel", "nos_voxel_map_score_batch")):
        m = maps[kind][0]
        rows = _prefilled(2)
        untouched = rows.tobytes()
        assert _call(name, m._h, [sc._h, sc._h], 0, R, t, None, 2, rows) == 0  # n_problems == 0
        assert _call(name, m._h, None, 0, None, None, None, 2, None) == 0
        assert rows.tobytes() == untouched
        assert len(api.score_batch(m, [], np.zeros((0, 9)), np.zeros((0, 3)), None)) == 0
        got = api.score_batch(m, [empty_scan, sc], R, t, LOSSES["exponential"])
        assert got[0]["matches"] == 0 and got[0]["matched_points"] == 0 and got[0]["cost"] == 0.0
        assert got[1]["matches"] > 0 and got[1]["cost"] > 0.0
        assert _call(name, m._h, [empty_scan._h, sc._h], 2, R, t, None, 2, rows) == 0  # loss == NULL: none
        assert rows["matches"][0] == 0 and rows["cost"][0] == 0.0 and rows["reserved"].tolist() == [0.0, 0.0]
        assert rows["matches"][1] == got[1]["matches"]
    for m in (empty_store, empty_map):
        got = api.score_batch(m, [sc, empty_scan], R, t, LOSSES["huber"])
        assert not got["matches"].any() and not got["matched_points"].any() and not got["cost"].any()
    for h in (sc, empty_scan, empty_store, empty_map):
        h.close()
