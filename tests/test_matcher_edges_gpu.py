"""find_two_nearest where it can go wrong (tests/matcher_edge_inputs.py): points within a few ulps of a cell face, distances
within a few ulps of the radius, exact ties, cells at the +-2^20 limit, keys that fold, queries no cell can hold — against a
numpy brute force over all voxels that has the device's bits (the module's text says why), at the identity pose.  Every
comparison is of bits or integers.

Snapshot maps: one per (radius_sq, region), in the dense and the hash lookup form.  Live store: below."""
import math

import numpy as np
import pytest

from tests import matcher_edge_inputs as mei

pytestmark = pytest.mark.gpu

LOSS = ("exponential", 1.0, 1.0)
EYE, ZERO = np.eye(3), np.zeros(3)


def _voxels_of_records(planes):
    """[15][2 n] planes → [n][2] original voxel ids from the S that names them, -1 for an all-zero record"""
    empty = ~planes.any(axis=0)
    ids = np.where(empty, -1, mei.id_of_sqrt_info(planes[6], planes[7]))
    return ids.reshape(-1, 2)


def snapshot_differences(ctx, r2, region, dense):
    """Runs every form of the snapshot matcher on the (r2, region) map in one lookup form → list of (what, number of
    queries or integers that differ), empty when the device gives the reference."""
    from nonlinear_optimizer_for_slam_amd import api
    case, idx = mei.snapshot_case(r2, region), mei.snapshot_reference(r2, region)
    q, means, S, valid = case["queries"], case["means"], case["sqrt_infos"], case["valid"]
    n = len(q)
    bad = []

    def note(what, count):
        if count:
            bad.append((what, int(count)))

    with ctx.options(match_dense=int(dense)):
        gm = api.NdtMap(ctx, means, S, valid, r2)
    plain, by_cell = api.Scan(ctx, q), api.Scan(ctx, q, sort_cell=math.sqrt(r2))
    order = by_cell.order.astype(np.int64)
    try:
        for k in (2, 1):
            want, count = mei.expected_planes(q, means, S, idx, k)
            ds, got_n = gm.match(plain, EYE, ZERO, k, "f64")
            got = api.download(ds)
            ds.close()
            note("match f64 k=%d n_matches" % k, got_n != count)
            differs = (got.view(np.uint64) != want.view(np.uint64)).any(axis=0).reshape(n, 2).any(axis=1)
            note("match f64 k=%d records" % k, differs.sum())
            for fam in np.unique(case["family"][differs]):
                note("  of them %s" % fam, (case["family"][differs] == fam).sum())
            # a cell-sorted scan: the same records in the scan's order
            want_s, _ = mei.expected_planes(q[order], means, S, idx[order], k)
            ds, got_n = gm.match(by_cell, EYE, ZERO, k, "f64")
            got = api.download(ds)
            ds.close()
            note("sorted scan k=%d n_matches" % k, got_n != count)
            note("sorted scan k=%d records" % k, (got.view(np.uint64) != want_s.view(np.uint64)).any(axis=0).sum())
            # an fp32 dataset: the same slots occupied, by the same voxels
            ds, got_n = gm.match(plain, EYE, ZERO, k, "f32")
            got = api.download(ds)
            ds.close()
            want_ids = np.where(np.arange(2)[None, :] < k, idx, -1)
            note("match f32 k=%d n_matches" % k, got_n != count)
            note("match f32 k=%d voxels" % k, (_voxels_of_records(got) != want_ids).any(axis=1).sum())
            # voxel ids instead of records: the table row names the voxel (U of this S is S)
            ind, got_n = gm.match_indexed(plain, EYE, ZERO, k, "f64", sort_by_voxel=False)
            ids, table = ind.ids(), ind.table()
            ind.close()
            note("match_indexed k=%d n_matches" % k, got_n != count)
            named = np.where(ids < 0, -1, mei.id_of_sqrt_info(table[np.maximum(ids, 0), 3], table[np.maximum(ids, 0), 4]))
            note("match_indexed k=%d voxels" % k, (named.T != idx[:, :k]).any(axis=1).sum())
            hit = ids >= 0
            note("match_indexed k=%d means" % k, (table[ids[hit], :3] != means[named[hit]]).any(axis=1).sum())
            # the score of the identity pose counts the same matches
            matches, matched_points, _ = gm.score(plain, EYE, ZERO, LOSS, k)
            note("score k=%d matches" % k, matches != count)
            note("score k=%d matched_points" % k, matched_points != int((idx[:, 0] >= 0).sum()))
    finally:
        for h in (plain, by_cell, gm):
            h.close()
    return bad


@pytest.mark.parametrize("region", list(mei.REGIONS))
@pytest.mark.parametrize("r2", mei.RADII)
def test_snapshot_matcher_at_faces_radius_ties_and_limits(ctx, r2, region):
    """NdtMap.match (f64 records bit for bit and n_matches, max_neighbors 2 and 1; fp32: same slots, same voxels),
    match_indexed (the same voxels), score (the same counts) and a cell-sorted scan, with the dense and with the hash lookup."""
    for dense in (1, 0):
        bad = snapshot_differences(ctx, r2, region, dense)
        assert not bad, (r2, region, "dense" if dense else "hash", bad)


# ---------------------------------------------------------------------------------------------- the live voxel store

@pytest.mark.parametrize("shifted", [False, True], ids=["origin", "limit"])
@pytest.mark.parametrize("res,r2", mei.LIVE_CONFIGS)
def test_live_matcher_at_the_radius_on_ties_and_at_the_grid_limit(ctx, res, r2, shifted):
    """VoxelMap.match, match_indexed and score on a store of exact voxels (mei.live_layout: resolutions and radii that are
    no powers of two, cells up to +-(2^20 - 16)), with radius and tie islands around the means stats() reads back: the
    brute force's records bit for bit, its voxels, its counts; and the snapshot route on the same store, bit for bit."""
    from nonlinear_optimizer_for_slam_amd import api
    from nonlinear_optimizer_for_slam_amd._lib import NosError
    from tests.test_voxel_map_match import UNSUPPORTED, _guard_holds, _live, _same_as_snapshot
    lay = mei.live_layout(res, shifted)
    vm = api.VoxelMap(ctx, res, r2)
    for pts in lay["batches"]:
        vm.insert(pts)
    _guard_holds(vm, res)
    st = vm.stats()
    means, valid, S = st["means"], st["valid"], st["sqrt_infos"].reshape(-1, 9)
    assert len(vm) == len(lay["mu"]) and int((~valid).sum()) == int((lay["role"] == mei.NEARER).sum())
    q, family, slot = mei.live_queries(lay, r2, means, st["cells"])
    left = mei.left_out(q, means, valid, r2)
    assert left.mean() <= 0.01
    keep = ~left
    idx, d2 = mei.brute_force(q[keep], means, valid, r2, take=3)
    full = -np.ones((len(q), 3), dtype=np.int64)
    full[keep] = idx
    tie = (family == "tie")[keep]
    # the islands came out as islands on the means the device computed: ties of two and three, both slot orders, both sides
    assert tie.sum() == 36 and np.all(d2[tie, 0] == d2[tie, 1]) and np.all(idx[tie, 1] >= 0) and int((d2[tie, 2] == d2[tie, 0]).sum()) == 24
    assert 6 <= int((idx[tie, 0] == slot[keep][tie]).sum()) <= 30
    assert (idx[~tie, 0] >= 0).sum() > 500 and (idx[~tie, 0] < 0).sum() > 500
    cols = np.stack([2 * np.nonzero(keep)[0], 2 * np.nonzero(keep)[0] + 1], axis=1).ravel()
    # the snapshot route on the same store — where a snapshot exists: its cells have the edge of the RADIUS, and at
    # (1.0, 0.3) the shifted store lies beyond the +-2^20 of them (NOS_ERR_UNSUPPORTED); the live route alone then
    if np.abs(means[valid]).max() / math.sqrt(r2) < mei.LIMIT - 3:
        _same_as_snapshot_or_live = _same_as_snapshot
    else:
        assert shifted and (res, r2) == (1.0, 0.3)
        with pytest.raises(NosError) as err:
            vm.snapshot()
        assert err.value.status == UNSUPPORTED
        _same_as_snapshot_or_live = _live
    plain, by_cell = api.Scan(ctx, q), api.Scan(ctx, q, sort_cell=res)
    order = by_cell.order.astype(np.int64)
    for k in (2, 1):
        want, count = mei.expected_planes(q, means, S, full, k)
        got, n = _same_as_snapshot_or_live(vm, plain, (EYE, ZERO), k, "f64")  # the live route, equal to the snapshot route
        assert got[:, cols].tobytes() == want[:, cols].tobytes(), int((got[:, cols] != want[:, cols]).any(axis=0).sum())
        assert n == count or left.any()
        want_s, _ = mei.expected_planes(q[order], means, S, full[order], k)
        got, n = _same_as_snapshot_or_live(vm, by_cell, (EYE, ZERO), k, "f64")
        keep_s = np.repeat(keep[order], 2)
        assert got[:, keep_s].tobytes() == want_s[:, keep_s].tobytes() and (n == count or left.any())
        got, n = _same_as_snapshot_or_live(vm, plain, (EYE, ZERO), k, "f32")  # fp32: the same slots, the same voxels (by their mean)
        assert np.array_equal(got[3:6, cols], want[3:6, cols].astype(np.float32)) and np.array_equal(got[6:15, cols].any(axis=0), want[6:15, cols].any(axis=0))
        # the voxel-indexed form: a compact table, one row per matched voxel — the mean names the voxel
        ind, n_ind = vm.match_indexed(plain, EYE, ZERO, k, "f64", sort_by_voxel=False)
        ids, table = ind.ids(), ind.table()
        ind.close()
        assert n_ind == n
        for s in range(k):
            hit = (ids[s] >= 0) & keep
            assert np.array_equal((ids[s] >= 0)[keep], full[keep, s] >= 0)
            assert np.array_equal(table[ids[s][hit], :3], means[full[hit, s]])
        matches, matched_points, _ = vm.score(plain, EYE, ZERO, LOSS, k)
        assert matches == n and (left.any() or matched_points == int((full[:, 0] >= 0).sum()))
    for h in (plain, by_cell, vm):
        h.close()
