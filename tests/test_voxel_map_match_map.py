"""One voxel store matched against another (VoxelMap.match_map / nos_voxel_map_match_map, pipeline.map_to_map; DESIGN.md
§23), on the GPU.

The search is the point matcher's, so p and mu are held bit for bit against VoxelMap.match on a scan of the source's means;
the information matrix of every record is held against 50 digits with the bound of the host hook
(tests/voxel_d2d_inputs.py: 4 x the worst error of a plain numpy restatement); the U planes, which no download returns,
are held through what reads them: accumulate6 streams p, mu and U only, and must agree with the numpy sums over the
downloaded p, mu and S to the 1e-10 of tests/test_gpu_parity.py, and bit for bit between two matches.

Measured on an MI355X.  Information of the 710 records of the general pair: worst error 3.8 eps (bound 152.7 eps).
Registration of the shell from the four starts: max_neighbors=1 ends below 1e-6 in translation (0 to the six digits
printed) and 1e-15 … 5e-13 in ‖R − R_T‖_F, in 2 rounds; max_neighbors=2 ends 1.05e-3 … 1.14e-3 and 3.4e-4 … 3.9e-4 away (the
second neighbours' pull, expected), in 4 rounds.

levels=(2, 1) ends 4e-16 … 4e-15 and 4e-16 … 1.2e-15 away, in 2 coarse rounds and 1 fine round.

That last test is what decides how a coarse level is made.  t = (3, −2, 1) has odd components, so the 2 m cells of
source.coarsened(2), seen in the target's frame, are offset by half a cell in x and z from those of target.coarsened(2):
the two partition the shell differently (44 and 54 voxels), their nearest means do not coincide at T, the coarse level
started AT T moves to dt = (0.09, 0.07, −0.25), ‖R − R_T‖_F 0.2, and three of the four starts end one cell (0.993 … 0.997 m)
off.  map_to_map therefore merges the source onto the coarse TARGET grid under the level's start pose: both coarse maps
then have the same 44 voxels, and the pose after the 2 m level is 1.5e-13 … 9.5e-13 from T."""
import ctypes

import mpmath
import numpy as np
import pytest

from tests import helpers
from tests import voxel_d2d_inputs as di

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 6
LOSS = ("exponential", 1.0, 1.0)
I3, Z3 = np.eye(3), np.zeros(3)


def _api():
    from nonlinear_optimizer_for_slam_amd import api
    return api


def _store(ctx, points, res=1.0, radius_sq=1.0):
    vm = _api().VoxelMap(ctx, res, radius_sq)
    vm.insert(points)
    return vm


@pytest.fixture(scope="module")
def general(ctx):
    tp, sp, R, t = di.general_pair()
    target, source = _store(ctx, tp), _store(ctx, sp)
    yield target, source, R, t
    target.close()
    source.close()


@pytest.fixture(scope="module")
def shell(ctx):
    R, t = di.shell_pose()
    target, source = _store(ctx, di.shell_points()), _store(ctx, di.moved_by_inverse(di.shell_points(), R, t))
    yield target, source
    target.close()
    source.close()


def _planes(ds):
    return _api().download(ds)


def _StS(planes, i):
    S = planes[6:15, i].reshape(3, 3)
    return S.T @ S


def test_the_general_pair_has_what_the_tests_need(general):
    target, source, R, t = general
    st = source.stats()
    assert len(target) == 320 and 0 < target.n_valid < 320
    assert len(source) > 256 and len(source) % 256 != 0  # more than one block, a partial last block
    assert source.n_valid >= 200 and source.n_valid < len(source)
    ds, n = target.match_map(source, R, t, 2, "f64")
    P = _planes(ds)
    ds.close()
    full = np.any(P[6:15] != 0.0, axis=0)
    per_voxel = full[0::2].astype(int) + full[1::2].astype(int)
    assert n == int(full.sum())
    assert np.any(per_voxel[st["valid"]] < 2), "a valid source voxel with no match or only one"
    assert not np.any(per_voxel[~st["valid"]])


@pytest.mark.parametrize("dtype", ("f64", "f32"))
@pytest.mark.parametrize("k", (1, 2))
def test_same_search_as_the_point_matcher_bit_for_bit(ctx, general, k, dtype):
    api = _api()
    target, source, R, t = general
    st = source.stats()
    idx = np.flatnonzero(st["valid"])
    scan = api.Scan(ctx, st["means"][idx])
    try:
        a, na = target.match(scan, R, t, k, dtype)
        b, nb = target.match_map(source, R, t, k, dtype)
        A, B, slots = _planes(a), _planes(b), len(b)
        a.close()
        b.close()
    finally:
        scan.close()
    assert na == nb and na > 0
    assert slots == 2 * len(source)
    for s in (0, 1):
        assert A[:6, s::2].tobytes() == np.ascontiguousarray(B[:6, 2 * idx + s]).tobytes(), (k, dtype, s)
    invalid = np.flatnonzero(~st["valid"])
    assert len(invalid) > 0
    assert not np.any(B[:, 2 * invalid]) and not np.any(B[:, 2 * invalid + 1])
    if k == 1:
        assert not np.any(B[:, 1::2])
    assert nb == int(np.any(B[6:15] != 0.0, axis=0).sum())


def test_information_of_every_record_against_50_digits_and_the_sums(general):
    from oracle import oracle_np
    target, source, R, t = general
    ts, ss = target.stats(), source.stats()
    by_mean = {ts["means"][j].tobytes(): j for j in range(len(target)) if ts["valid"][j]}
    ds, n = target.match_map(source, R, t, 2, "f64")
    try:
        P = _planes(ds)
        got = [ds.accumulate6(R, t, loss) for loss in (None, LOSS)]
        got_moved = ds.accumulate6(helpers.rot_xyz(0.01, -0.02, 0.05) @ R, t + np.array([-0.1, 0.05, 0.2]), LOSS)
    finally:
        ds.close()
    full = np.flatnonzero(np.any(P[6:15] != 0.0, axis=0))
    assert len(full) == n and n >= 200
    worst = 0.0
    with mpmath.workdps(di.DPS):
        for i in full:
            v, j = i // 2, by_mean[P[3:6, i].tobytes()]
            assert ss["valid"][v] and P[:3, i].tobytes() == ss["means"][v].tobytes()
            A = di.pair_information_xp(ts["sqrt_infos"][j], ss["sqrt_infos"][v], R)
            worst = max(worst, di.information_error(P[6:15, i].reshape(3, 3), A))
    print("worst max|S^T S - A| / max|A| over %d records: %.1f eps (bound %.1f eps)" % (n, worst / di.EPS, di.bound() / di.EPS))
    assert worst <= di.bound()
    # U through the sums: accumulate6 reads p, mu, U; the numpy sums read p, mu, S
    for g, loss in zip(got, (None, LOSS)):
        helpers.assert_normal_equations_close(g, oracle_np.ndt6_accumulate(P, R, t, loss), 6, 1e-10)
    helpers.assert_normal_equations_close(
        got_moved, oracle_np.ndt6_accumulate(P, helpers.rot_xyz(0.01, -0.02, 0.05) @ R, t + np.array([-0.1, 0.05, 0.2]), LOSS),
        6, 1e-10)
    # without a loss the translation block of H is Σ UᵀU: against Σ SᵀS from the S planes
    H = helpers.unpack(got[0], 6)[0]
    want = sum(_StS(P, i) for i in full)
    assert np.max(np.abs(H[:3, :3] - want)) <= 1e-10 * np.max(np.abs(want))


def test_self_match_on_the_shell(shell):
    target, _ = shell
    st = target.stats()
    assert len(target) == 212 and target.n_valid == 212
    ds, n = target.match_map(target, I3, Z3, 1, "f64")
    P = _planes(ds)
    ds.close()
    assert n == target.n_valid
    first = P[:, 0::2]
    assert first[:3].tobytes() == first[3:6].tobytes()
    assert np.ascontiguousarray(first[:3].T).tobytes() == st["means"].tobytes()
    with mpmath.workdps(di.DPS):
        for v in range(len(target)):
            M = di._mpm(st["sqrt_infos"][v])
            assert di.information_error(first[6:15, v].reshape(3, 3), (M.T * M) / 2) <= di.bound(), v
    ds, n2 = target.match_map(target, I3, Z3, 2, "f64")
    P2 = _planes(ds)
    ds.close()
    assert P2[:, 0::2].tobytes() == first.tobytes() and n2 > n


def test_read_only_and_deterministic(general):
    target, source, R, t = general
    before = [(vm.stats(), vm.memory(), len(vm), vm.n_valid, vm.n_points) for vm in (target, source)]
    out = []
    for _ in range(2):
        for dtype in ("f64", "f32"):
            ds, n = target.match_map(source, R, t, 2, dtype)
            out.append((n, _planes(ds).tobytes(), ds.accumulate6(R, t, LOSS).tobytes(), ds.accumulate6(R, t, None).tobytes()))
            ds.close()
    assert out[0] == out[2] and out[1] == out[3]  # p, mu, S by download; U by the sums that stream it
    after = [(vm.stats(), vm.memory(), len(vm), vm.n_valid, vm.n_points) for vm in (target, source)]
    for b, a in zip(before, after):
        assert b[1:] == a[1:]
        for key in b[0]:
            assert b[0][key].tobytes() == a[0][key].tobytes(), key


def _pose_errors(pose):
    R, t = di.shell_pose()
    return float(np.linalg.norm(pose.t - t)), float(np.linalg.norm(pose.R - R))


@pytest.mark.parametrize("start", range(4))
def test_registration_recovers_a_known_pose(ctx, shell, start):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    target, source = shell
    R0, t0 = di.shell_starts()[start]
    assert np.max(np.abs(t0 - di.shell_pose()[1])) <= 0.15
    pose, rounds, outer, info = pipeline.map_to_map(ctx, target, source, Pose(R0, t0), loss=LOSS, max_neighbors=1)
    et, eR = _pose_errors(pose)
    print("start %d, max_neighbors=1: |dt| %.2e, |dR|_F %.2e, %d rounds" % (start, et, eR, len(rounds)))
    assert et < 1e-5 and eR < 1e-5, (et, eR)
    assert outer < 10 and len(rounds) == outer + 1
    assert "level" not in rounds[0] and info["sums"].shape == (28,)

    pose, rounds, outer, info = pipeline.map_to_map(ctx, target, source, Pose(R0, t0), loss=LOSS, max_neighbors=2)
    et, eR = _pose_errors(pose)
    print("start %d, max_neighbors=2: |dt| %.2e, |dR|_F %.2e, %d rounds" % (start, et, eR, len(rounds)))
    assert et < 1e-2 and eR < 1e-2, (et, eR)
    ds, n = target.match_map(source, pose.R, pose.t, 2, "f64")
    fresh = ds.accumulate6(pose.R, pose.t, LOSS)
    ds.close()
    assert info["sums"].tobytes() == fresh.tobytes() and info["matches"] == n


@pytest.mark.parametrize("start", range(4))
def test_registration_coarse_to_fine_recovers_the_pose(ctx, shell, start):
    """levels=(2, 1) from the same starts, the same 1e-5 bound; neither store is changed by the coarse level."""
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    target, source = shell
    R0, t0 = di.shell_starts()[start]
    before = (len(target), len(source), target.memory(), source.memory())
    pose, rounds, outer, info = pipeline.map_to_map(ctx, target, source, Pose(R0, t0), loss=LOSS, max_neighbors=1, levels=(2, 1))
    et, eR = _pose_errors(pose)
    print("start %d, levels (2, 1): |dt| %.2e, |dR|_F %.2e, %d rounds" % (start, et, eR, len(rounds)))
    lv = [r["level"] for r in rounds]
    assert lv[0] == 2 and lv[-1] == 1 and lv == sorted(lv, reverse=True)
    assert before == (len(target), len(source), target.memory(), source.memory())
    assert info["sums"].shape == (28,)
    assert et < 1e-5 and eR < 1e-5, (et, eR)
    assert outer < 10


@pytest.mark.parametrize("levels", ((), (2,), (1, 2), (4, 2)))
def test_levels_end_at_the_stores_themselves(ctx, shell, levels):
    """info["sums"] and the pose belong to the stores themselves: a last factor other than 1 is refused"""
    from nonlinear_optimizer_for_slam_amd import pipeline
    target, source = shell
    with pytest.raises(ValueError):
        pipeline.map_to_map(ctx, target, source, levels=levels)


def test_errors_leave_the_output_untouched(ctx, general):
    api = _api()
    from nonlinear_optimizer_for_slam_amd import Context
    target, source, R, t = general
    lib = target._lib
    dp = ctypes.POINTER(ctypes.c_double)
    Rv, tv = np.ascontiguousarray(R.reshape(9)), np.ascontiguousarray(t)

    def call(tgt, src, k, dtype):
        out, n = ctypes.c_void_p(5), ctypes.c_size_t(7)
        rc = lib.nos_voxel_map_match_map(tgt._h, src._h, Rv.ctypes.data_as(dp), tv.ctypes.data_as(dp), k, dtype,
                                         ctypes.byref(out), ctypes.byref(n))
        assert out.value == 5 and n.value == 7
        return rc

    assert call(target, source, 0, 0) == UNSUPPORTED
    assert call(target, source, 3, 0) == UNSUPPORTED
    assert call(target, source, 2, 2) == INVALID
    assert call(target, source, 2, -1) == INVALID
    other = Context((0,))
    try:
        foreign = _store(other, di.shell_points()[:50])
        assert call(target, foreign, 2, 0) == INVALID
        assert call(foreign, target, 2, 0) == INVALID
        foreign.close()
    finally:
        other.close()
    # a search ball of more than 9 target cells per axis: what nos_voxel_map_match returns for it
    wide = api.VoxelMap(ctx, 0.25, 1.0)
    scan = api.Scan(ctx, di.shell_points()[:10])
    try:
        wide.insert(di.shell_points()[:100])
        out, n = ctypes.c_void_p(5), ctypes.c_size_t(7)
        rc_point = lib.nos_voxel_map_match(wide._h, scan._h, Rv.ctypes.data_as(dp), tv.ctypes.data_as(dp), 2, 0,
                                           ctypes.byref(out), ctypes.byref(n))
        assert rc_point == UNSUPPORTED and out.value == 5
        assert call(wide, source, 2, 0) == rc_point
        ds, _ = source.match_map(wide, R, t)  # the limit is the TARGET's: as a source the fine store is fine
        assert len(ds) == 2 * len(wide)
        ds.close()
    finally:
        scan.close()
        wide.close()
    with pytest.raises(KeyError):
        target.match_map(source, R, t, 2, "f16")
    # an empty source: an empty dataset, as an empty scan gives
    empty = api.VoxelMap(ctx, 1.0, 1.0)
    try:
        ds, n = target.match_map(empty, R, t)
        assert len(ds) == 0 and n == 0
        ds.close()
    finally:
        empty.close()
