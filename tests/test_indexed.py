"""Voxel-indexed NDT datasets (additive layout): same sums as the flat layout / the oracle."""
import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import exact_inputs, helpers

pytestmark = pytest.mark.gpu
LOSSES = [None, ("exponential", 1.0, 1.0), ("huber", 1.2)]
R_TEST = helpers.rot_xyz(0.01, -0.02, 0.05)
T_TEST = np.array([-0.1, 0.05, 0.2])


def _random_indexed(n, v, k, seed, frac_missing=0.1):
    rng = np.random.default_rng(seed)
    means = rng.uniform(-20, 20, size=(v, 3))
    S = rng.normal(size=(v, 3, 3)) * 3.0
    idx = rng.integers(0, v, size=(k, n)).astype(np.int32)
    idx[rng.uniform(size=(k, n)) < frac_missing] = -1
    pts = (means[np.maximum(idx[0], 0)] + rng.normal(scale=0.3, size=(n, 3))).T.copy()
    # the equivalent flat planes (one column per (point, slot) with a valid voxel)
    cols = []
    for kk in range(k):
        ok = idx[kk] >= 0
        cols.append(np.concatenate([pts[:, ok], means[idx[kk, ok]].T, S[idx[kk, ok]].reshape(-1, 9).T], axis=0))
    return pts, idx, means, S, np.concatenate(cols, axis=1)


@pytest.mark.parametrize("n,v,k", [(1, 1, 1), (1000, 7, 1), (50_003, 900, 2)])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("sort", [False, True])
def test_indexed_matches_oracle(ctx, oracle, n, v, k, loss, sort):
    from nonlinear_optimizer_for_slam_amd import NdtIndexedDataset
    pts, idx, means, S, flat = _random_indexed(n, v, k, n + v)
    for dtype, rtol in (("f64", 1e-10), ("f32", 1e-4)):  # fp32 table (A = S^T S then, U of S = QU now): 2.4e-5 on a single item with A
        ds = NdtIndexedDataset.from_arrays(ctx, pts, idx, means, S, dtype, sort)
        assert len(ds) == n and ds.stream_bytes == n * ((24 if dtype == "f64" else 12) + 4 * k)
        helpers.assert_normal_equations_close(ds.accumulate6(R_TEST, T_TEST, loss),
                                              oracle.ndt6_accumulate(flat, R_TEST, T_TEST, loss), 6, rtol)
        c, s = np.cos(0.07), np.sin(0.07)
        R2, t2 = np.array([[c, -s], [s, c]]), np.array([-0.15, 0.1])
        helpers.assert_normal_equations_close(ds.accumulate3(R2, t2, loss), oracle.ndt3_accumulate(flat, R2, t2, loss), 3, rtol)
        ds.close()


def test_indexed_all_slots_missing_gives_zero(ctx):
    from nonlinear_optimizer_for_slam_amd import NdtIndexedDataset
    pts = np.random.default_rng(0).normal(size=(3, 500))
    idx = -np.ones((2, 500), dtype=np.int32)
    ds = NdtIndexedDataset.from_arrays(ctx, pts, idx, np.zeros((3, 3)), np.tile(np.eye(3), (3, 1, 1)))
    assert np.all(ds.accumulate6(np.eye(3), np.zeros(3), ("exponential", 1.0, 1.0)) == 0.0)
    ds.close()


def test_indexed_matcher_equals_flat_matcher(ctx, oracle):
    """nos_ndt_match_indexed and nos_ndt_match describe the same correspondences: identical sums (to rounding),
    identical match counts — on the reference's room scene and through a whole scan-to-map solve."""
    from nonlinear_optimizer_for_slam_amd import api, solvers
    pts = scene.generate_global_points()
    m = scene.build_ndt_map(pts, 1.0)
    local = scene.filter_points(pts, 0.1) + np.array([0.1, -0.05, 0.02])
    gm = api.NdtMap(ctx, m["means"], m["sqrt_infos"], m["valid"], 1.0)
    sc = api.Scan(ctx, local)
    loss = ("exponential", 1.0, 1.0)
    flat, n_flat = gm.match(sc, np.eye(3), np.zeros(3), 2, "f64")
    for sort in (False, True):
        ind, n_ind = gm.match_indexed(sc, np.eye(3), np.zeros(3), 2, "f64", sort)
        assert n_ind == n_flat and len(ind) == local.shape[0]
        helpers.assert_normal_equations_close(ind.accumulate6(R_TEST, T_TEST, loss), flat.accumulate6(R_TEST, T_TEST, loss), 6, 1e-11)
        ind.close()
    ind, _ = gm.match_indexed(sc, np.eye(3), np.zeros(3), 2, "f64", True)
    solver = solvers.MahalanobisDistanceMinimizerHip()
    solver.SetLossFunction(loss)
    pa, pb = solvers.Pose(), solvers.Pose()
    assert solver.SolveDataset(solvers.Options(), flat, pa)
    it_flat = solver.report.iterations
    assert solver.SolveDataset(solvers.Options(), ind, pb)
    assert solver.report.iterations == it_flat
    dt, dq = helpers.pose_delta(pa.R, pa.t, pb.R, pb.t)
    assert dt < 1e-9 and dq < 1e-9
    for h in (flat, ind, sc, gm):
        h.close()


def test_indexed_full_size_matches_flat(ctx):
    """configs[1] shape (10 M points / 200 k voxels): the indexed dataset built from the synthetic scene's voxel
    assignment gives the flat dataset's sums."""
    from nonlinear_optimizer_for_slam_amd import NdtDataset, NdtIndexedDataset, synth
    n, v = 10_000_000, 200_000
    planes = synth.ndt_planes(n, v)
    # recover the voxel table / ids of the generator from the flat planes (mean_x identifies the voxel)
    uniq, first, inv = np.unique(planes[3], return_index=True, return_inverse=True)
    means = planes[3:6, first].T.copy()
    S = planes[6:15, first].T.copy()
    idx = inv.astype(np.int32)[None, :]
    loss = ("exponential", 1.0, 1.0)
    flat = NdtDataset.from_planes(ctx, planes, "f64")
    want = flat.accumulate6(R_TEST, T_TEST, loss)
    flat.close()
    ind = NdtIndexedDataset.from_arrays(ctx, planes[0:3], idx, means, S, "f64", True)
    helpers.assert_normal_equations_close(ind.accumulate6(R_TEST, T_TEST, loss), want, 6, 1e-11)
    ind.close()


def test_indexed_empty_and_download(ctx):
    from nonlinear_optimizer_for_slam_amd import NdtIndexedDataset, api
    ds = NdtIndexedDataset.from_arrays(ctx, np.zeros((3, 0)), np.zeros((1, 0), dtype=np.int32), np.zeros((1, 3)),
                                       np.eye(3)[None])
    assert len(ds) == 0 and np.all(ds.accumulate6(np.eye(3), np.zeros(3), None) == 0.0)
    ds.close()
    pts = np.arange(30, dtype=np.float64).reshape(3, 10)
    idx = np.array([[3, 1, 2, 0, 1, 3, 2, 0, -1, 1]], dtype=np.int32)
    ds = NdtIndexedDataset.from_arrays(ctx, pts, idx, np.zeros((4, 3)), np.tile(np.eye(3), (4, 1, 1)), "f64", True)
    got = api.download(ds)            # points come back in voxel-sorted order (ids 0,0,1,1,1,2,2,3,3,none)
    order = np.argsort(np.where(idx[0] < 0, 1 << 30, idx[0]), kind="stable")
    assert np.array_equal(got, pts[:, order])
    ds.close()


def _exact_lattice_case():
    """A 4 x 4 x 4 lattice of voxels with means on quarter positions (cell faces included) and the integer, upper-triangular
    S of exact_inputs (U of S = QU is then S itself, so a table row holds the flat record's numbers), three of them
    invalid; about 300 world points: named ones at the radius itself, one ulp-scale step inside and outside it, on ties,
    far away, and a quarter lattice that brings ties and exact-radius candidates in numbers; the pose: a quarter turn
    about z and a dyadic translation, so local = R^T (world - t) and the device's warp back are both exact.
    → (means, S, valid, r2, local, R, t, idx [n][2] original voxel ids by (d2, id) or -1, d2 [n][2])"""
    rng = np.random.default_rng(1812)
    cells = np.array([[x, y, z] for x in range(4) for y in range(4) for z in range(4)], dtype=np.float64)
    means = cells + rng.integers(0, 4, size=cells.shape) / 4.0
    means[0] = [0.5, 0.5, 0.5]  # the corner voxel the named points probe from outside the lattice, and its neighbours
    means[1] = [0.5, 0.5, 1.5]
    means[4], means[16], means[20] = [0.75, 1.75, 0.75], [1.75, 0.75, 0.75], [1.75, 1.75, 0.75]
    _, _, S = exact_inputs._ndt_chunk(5, 0, len(means), 3)
    S = np.ascontiguousarray(np.moveaxis(S, 2, 0), dtype=np.float64)
    valid = np.ones(len(means), dtype=bool)
    valid[[7, 21, 40]] = False
    r2, tiny = 1.0, 2.0 ** -40
    a = means[0]
    named = np.array([
        a - [1.0, 0, 0], a - [0, 1.0, 0],                    # the radius itself: d2 = 1 is no match
        a - [1.0 - tiny, 0, 0], a - [0, 0, 1.0 - tiny],      # just inside: d2 rounds to 1 - 2^-39
        a - [1.0 + tiny, 0, 0], a - [0, 1.0 + tiny, 0],      # just outside
        [0.5, 0.5, 1.0],                                     # equidistant from voxels 0 and 1: the lower id first
        [40.0, 40.0, 40.0], [-9.0, 2.0, 2.0],                # nothing near
    ])
    world = np.concatenate([named, rng.integers(-4, 21, size=(290, 3)) / 4.0])
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([0.5, -0.25, 0.125])
    local = (world - t) @ R  # rows R^T (w - t)
    assert np.array_equal(local @ R.T + t, world)
    e = world[:, None, :] - means[None, :, :]
    d = e[:, :, 0] * e[:, :, 0] + e[:, :, 1] * e[:, :, 1] + e[:, :, 2] * e[:, :, 2]  # one product is inexact at the most
    d[:, ~valid] = np.inf
    order = np.argsort(d, axis=1, kind="stable")[:, :2]  # ties: the lower id first
    d2 = np.take_along_axis(d, order, axis=1)
    idx = np.where(d2 < r2, order, -1)  # strict
    assert idx[:9].tolist() == [[-1, -1], [-1, -1], [0, -1], [0, -1], [-1, -1], [-1, -1], [0, 1], [-1, -1], [-1, -1]]
    assert d2[0, 0] == 1.0 and d2[2, 0] < 1.0 < d2[4, 0] and d2[6, 0] == d2[6, 1] == 0.25
    assert int((d == r2).any(axis=1).sum()) > 5 and int(((d2[:, 0] == d2[:, 1]) & (d2[:, 0] < r2)).sum()) > 5  # and more of both
    assert (idx[:, 0] < 0).sum() > 10 and ((idx[:, 0] >= 0) & (idx[:, 1] < 0)).sum() > 10
    return means, S, valid, r2, local, R, t, idx, d2


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", [1, 2])
def test_snapshot_indexed_names_the_voxels_the_flat_matcher_writes(ctx, k, dtype):
    """On a snapshot map, under a pose that is not the identity, nos_ndt_match_indexed names — through its table — exactly
    the voxels whose records nos_ndt_match writes: same count; table row ids[s][i] = the mean and sqrt-information planes
    of flat record 2i + s, bit for bit (fp32: both narrowed the same way); -1 exactly where the flat record is all zero.
    Both are the numpy brute force's voxels, with no tolerance."""
    from nonlinear_optimizer_for_slam_amd import api
    means, S, valid, r2, local, R, t, idx, _ = _exact_lattice_case()
    n = len(local)
    gm = api.NdtMap(ctx, means, S, valid, r2)
    sc = api.Scan(ctx, local)
    flat, n_flat = gm.match(sc, R, t, k, dtype)
    ind, n_ind = gm.match_indexed(sc, R, t, k, dtype, sort_by_voxel=False)
    planes, ids, table = api.download(flat), ind.ids(), ind.table()
    for h in (flat, ind, sc, gm):
        h.close()
    assert planes.shape == (15, 2 * n) and ids.shape == (k, n) and table.shape == (int(valid.sum()), 16)
    want = idx[:, :k]
    assert n_flat == n_ind == int((want >= 0).sum())
    upper, lower = [0, 1, 2, 4, 5, 8], [3, 6, 7]  # of the row-major S: the table holds U = S, the triangle
    for s in range(2):
        rec = planes[:, s::2]  # records 2i + s
        empty = ~rec.any(axis=0)
        if s >= k:
            assert empty.all()
            continue
        assert np.array_equal(ids[s] < 0, empty) and np.array_equal(empty, want[:, s] < 0)
        hit = ~empty
        rows = table[ids[s][hit]]
        assert rows[:, :3].tobytes() == np.ascontiguousarray(rec[3:6, hit].T).tobytes()
        assert rows[:, 3:9].tobytes() == np.ascontiguousarray(rec[6:15, hit][upper].T).tobytes()
        assert not rec[6:15][lower].any() and not rows[:, 9:].any()
        assert np.array_equal(rec[0:3, hit].T, local[hit].astype(np.float32 if dtype == "f32" else np.float64))  # as stored
        # the brute force's voxel: means are distinct, so the mean names it
        assert np.array_equal(rows[:, :3], means[want[hit, s]]) and np.array_equal(rows[:, 3:9], S[want[hit, s]].reshape(-1, 9)[:, upper])
