"""Ray casting through the voxel store (VoxelMap.raycast / nos_voxel_map_raycast), on the GPU.

Truth is the restatement of the contract in tests/voxel_raycast_inputs.py (checked on its own in
test_voxel_raycast_host.py), fed with the DEVICE's voxel statistics (VoxelMap.stats()), so that the only differences left
are those the contract leaves open: the hit test may be fused and reordered.  On the generic scene a ray whose walk a
rounding error could change (near_tie over the whole segment) or whose hit decision one could (decision_margin) is not
uploaded — at most 1 % may be; the voxel ids are then compared entry for entry and the ranges against a 50-digit
evaluation for the same voxel and cell: the device may err 4 × as far as the plain-double restatement does, with a floor
of 4 ulp of max_range (the convention of DESIGN.md §23).  On the exact inputs (2^-10 lattice, resolution 0.5, axis
rotations) every ray is compared, ties included: ids only.

Not reachable from a test: NOS_ERR_UNSUPPORTED for a multi-device context and for a scan of 2^32 - 1 points, NOS_ERR_HIP
for a `broken` store."""
import numpy as np
import pytest

from tests import voxel_carve_inputs as ci
from tests import voxel_raycast_inputs as ri

pytestmark = pytest.mark.gpu

MAX_RANGE = 40.0
KEYS = ("cells", "counts", "valid", "means", "sqrt_infos")
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)


def _api():
    from nonlinear_optimizer_for_slam_amd import api
    return api


def _cast_all(R, t, points, store, max_range, **kw):
    a = ci.warp(R, t, kw.get("origin", (0.0, 0.0, 0.0)))
    return [ri.cast(R, t, p, store, ci.RES, max_range, a=a, **kw) for p in points]


@pytest.fixture(scope="module")
def world(ctx):
    """the generic scene in a store, the restatement's result for every ray that is uploaded, and the device's"""
    api = _api()
    s = ci.generic_scene()
    vm = api.VoxelMap(ctx, ci.RES, 1.0)
    vm.insert(np.concatenate([s["wall_points"], s["box_points"]]))
    s["vm"] = vm
    s["stats"] = vm.stats()
    s["store"] = ri.store_of(s["stats"])
    casts = _cast_all(s["R"], s["t"], s["scan_box"], s["store"], MAX_RANGE)
    geometric = np.array([c["skipped"] or ri.near_tie(c["ray"], ci.RES) for c in casts])
    margin = np.array([ri.decision_margin(c) for c in casts])
    keep = ~(geometric | margin)
    print("rays left out: %d geometric near-ties, %d at a decision margin, of %d" % (int(geometric.sum()), int(margin.sum()), keep.size))
    assert geometric.sum() == 0
    assert (~keep).sum() <= keep.size // 100
    s["scan"] = np.ascontiguousarray(s["scan_box"][keep])
    s["want"] = [c for c, k in zip(casts, keep) if k]
    s["want_voxels"] = np.array([c["voxel"] for c in s["want"]], dtype=np.int32)
    scan = api.Scan(ctx, s["scan"])
    s["got"] = vm.raycast(scan, s["R"], s["t"], MAX_RANGE)
    scan.close()
    yield s
    vm.close()


def test_voxels_hits_and_skipped_equal_the_restatement(world):
    voxels, ranges, info = world["got"]
    want = world["want_voxels"]
    assert voxels.dtype == np.int32 and ranges.dtype == np.float64 and voxels.shape == ranges.shape == want.shape
    print("rays %d, hits %d (%.1f %%)" % (want.size, int((want >= 0).sum()), 100.0 * (want >= 0).mean()))
    assert np.array_equal(voxels, want), int(np.sum(voxels != want))
    assert info == {"hits": int((want >= 0).sum()), "skipped": 0}
    assert np.all(ranges[want < 0] == 0.0)
    assert (want >= 0).mean() >= 0.97


def test_ranges_against_50_digits(world):
    voxels, ranges, _ = world["got"]
    store = world["store"]
    ulp = float(np.spacing(MAX_RANGE))
    worst_device = worst_numpy = 0.0
    for c, v, got in zip(world["want"], voxels, ranges):
        if c["voxel"] < 0:
            continue
        assert v == c["voxel"]
        truth = ri.range_xp(c["ray"], store["means"][v], store["S"][v], c["tau_in"], c["tau_out"], MAX_RANGE)
        worst_device = max(worst_device, ri.range_error(float(got), truth))
        worst_numpy = max(worst_numpy, ri.range_error(c["range"], truth))
    print("worst range error: device %.3g (%.2f ulp of max_range), restatement %.3g (%.2f ulp); ratio %.2f"
          % (worst_device, worst_device / ulp, worst_numpy, worst_numpy / ulp, worst_device / max(worst_numpy, 1e-300)))
    assert worst_device <= max(4.0 * worst_numpy, 4.0 * ulp)


@pytest.mark.parametrize("n", COUNTS)
def test_ray_counts_give_the_batch_bits_and_the_counts(ctx, world, n):
    api = _api()
    voxels, ranges, _ = world["got"]
    scan = api.Scan(ctx, world["scan"][:n])
    try:
        v, r, info = world["vm"].raycast(scan, world["R"], world["t"], MAX_RANGE, points=True)
        assert v.shape == (n,) and r.shape == (n,)
        assert v.tobytes() == voxels[:n].tobytes() and r.tobytes() == ranges[:n].tobytes()  # alone as in the batch
        assert info["hits"] == int((voxels[:n] >= 0).sum()) and info["skipped"] == 0
        assert len(info["scan"]) == info["hits"]
        assert np.array_equal(info["scan"].order, np.flatnonzero(voxels[:n] >= 0).astype(np.uint32))
        info["scan"].close()
    finally:
        scan.close()


def test_order_of_rays_batch_and_repetition_do_not_matter_and_the_store_is_untouched(ctx, world):
    api = _api()
    vm, R, t = world["vm"], world["R"], world["t"]
    voxels, ranges, info = world["got"]
    before, mem = vm.stats(), vm.memory()
    perm = np.random.default_rng(5).permutation(len(world["scan"]))
    shuffled, plain = api.Scan(ctx, world["scan"][perm]), api.Scan(ctx, world["scan"])
    try:
        v, r, i = vm.raycast(shuffled, R, t, MAX_RANGE)
        assert v.tobytes() == voxels[perm].tobytes() and r.tobytes() == ranges[perm].tobytes() and i == info
        for _ in range(2):  # a second call, and a third
            v, r, i = vm.raycast(plain, R, t, MAX_RANGE)
            assert v.tobytes() == voxels.tobytes() and r.tobytes() == ranges.tobytes() and i == info
        after = vm.stats()
        for k in KEYS:
            assert after[k].tobytes() == before[k].tobytes(), k
        assert vm.memory() == mem  # bytes, epoch and generation
    finally:
        shuffled.close()
        plain.close()


def test_a_cell_sorted_scan_maps_back_to_the_original_indices(ctx, world):
    api = _api()
    voxels, ranges, _ = world["got"]
    ordered = api.Scan(ctx, world["scan"], sort_cell=1.0)
    try:
        order = ordered.order
        assert not np.array_equal(order, np.arange(len(order)))  # the sort moved something
        v, r, info = world["vm"].raycast(ordered, world["R"], world["t"], MAX_RANGE, points=True)
        assert v.tobytes() == voxels[order].tobytes() and r.tobytes() == ranges[order].tobytes()  # indexed like the stored positions
        hits = info["scan"]
        assert np.array_equal(hits.order, order[v >= 0])  # composed with the input's order, as the filter composes it
        info["scan"].close()
    finally:
        ordered.close()


def test_hit_points_and_their_descriptor(ctx, world):
    api = _api()
    vm, R, t = world["vm"], world["R"], world["t"]
    origin = (0.125, -0.25, 0.0625)
    pts = world["scan"][:1000]
    scan = api.Scan(ctx, pts)
    try:
        v, r, info = vm.raycast(scan, R, t, MAX_RANGE, origin=origin, points=True)
        hits = info["scan"]
        assert info["hits"] == len(hits) == int((v >= 0).sum()) > 0
        a = ci.warp(R, t, origin)
        idx = np.flatnonzero(v >= 0)
        assert np.array_equal(hits.order, idx.astype(np.uint32))
        length = np.array([ri.ray(R, t, pts[i], ci.RES, MAX_RANGE, origin, a)["len"] for i in idx])
        o = np.array(origin)
        want = o + (r[idx] / length)[:, None] * (pts[idx] - o)  # quotient, difference, product, sum: each rounded once
        got = hits.points()
        assert np.all(np.abs(got - want) <= 2.0 * np.spacing(np.abs(want)))
        # the hit scan is a scan like any other: its descriptor is the descriptor of its points uploaded again
        again = api.Scan(ctx, got)
        d0, n0 = hits.descriptor(20, 60, 25.0, -2.0)
        d1, n1 = again.descriptor(20, 60, 25.0, -2.0)
        again.close()
        assert n0 == n1 > 0 and d0.tobytes() == d1.tobytes()
        hits.close()
    finally:
        scan.close()


def test_max_range_short_of_every_surface_gives_no_hit(ctx, world):
    api = _api()
    scan = api.Scan(ctx, world["scan"][:257])
    try:
        want = _cast_all(world["R"], world["t"], world["scan"][:257], world["store"], 0.5)
        assert all(c["voxel"] == -1 and not c["skipped"] for c in want)
        v, r, info = world["vm"].raycast(scan, world["R"], world["t"], 0.5, points=True)
        assert np.all(v == -1) and np.all(r == 0.0) and info["hits"] == 0 and info["skipped"] == 0
        assert len(info["scan"]) == 0 and info["scan"].points().shape == (0, 3)
        info["scan"].close()
    finally:
        scan.close()


def test_an_empty_store_and_an_empty_scan_are_no_ops(ctx, world):
    api = _api()
    empty = api.VoxelMap(ctx, ci.RES, 1.0)
    pts = np.array([(1.0, 0.0, 0.0), (float("nan"), 0.0, 0.0), (0.0, 0.0, 0.0)])
    scan, nothing = api.Scan(ctx, pts), api.Scan(ctx, np.zeros((0, 3)))
    try:
        v, r, info = empty.raycast(scan, np.eye(3), np.zeros(3), 10.0, points=True)
        assert np.all(v == -1) and np.all(r == 0.0) and info["hits"] == 0 and info["skipped"] == 0
        assert len(info["scan"]) == 0
        info["scan"].close()
        assert empty.memory()["generation"] == 0
        v, r, info = world["vm"].raycast(nothing, world["R"], world["t"], MAX_RANGE, points=True)
        assert v.shape == (0,) and r.shape == (0,) and info["hits"] == 0 and info["skipped"] == 0 and len(info["scan"]) == 0
        info["scan"].close()
    finally:
        for h in (scan, nothing, empty):
            h.close()


# ------------------------------------------------------------------------------------------------ the exact inputs

THIN = (1, 0, 0)  # this cell of the block holds four points: fewer than 5, not valid


@pytest.fixture(scope="module")
def block(ctx):
    api = _api()
    _, pts = ri.exact_block_points(thin=[THIN])
    vm = api.VoxelMap(ctx, ci.RES, 1.0)
    vm.insert(pts)
    stats = vm.stats()
    store = ri.store_of(stats)
    assert len(store["slot"]) == 216 and sum(store["valid"]) == 215 and not store["valid"][store["slot"][THIN]]
    assert store["counts"][store["slot"][THIN]] == 4 and store["counts"][store["slot"][(0, 0, 0)]] == 8
    yield {"vm": vm, "store": store}
    vm.close()


@pytest.mark.parametrize("pose", (0, 1, 2))
def test_ties_and_edges_on_exact_inputs(ctx, block, pose):
    api = _api()
    R, t = ri.exact_pose(pose)
    hits = 0
    for origin, p, max_range in ri.EXACT_RAYS:
        scan = api.Scan(ctx, np.array([p], dtype=np.float64))
        for max_m2, min_range in ((0.7, 0.0), (0.05, 0.0), (0.7, 0.6)):
            want = ri.cast(R, t, p, block["store"], ci.RES, max_range, min_range, max_m2, 0, origin)
            # no tested voxel is near the threshold (the nearest m2 lies 0.016 away), so the ids are the contract's
            assert all(abs(m2 - max_m2) > 1e-6 and (min_range == 0.0 or abs(rng - min_range) > 1e-6) for _, m2, rng, _, _ in want["tested"])
            v, r, info = block["vm"].raycast(scan, R, t, max_range, min_range=min_range, max_mahalanobis_sq=max_m2, origin=origin)
            assert v[0] == want["voxel"], (origin, p, max_m2, min_range, pose)
            assert info == {"hits": int(want["voxel"] >= 0), "skipped": 0}
            assert abs(r[0] - want["range"]) <= 4.0 * np.spacing(max_range)
            hits += int(want["voxel"] >= 0)
        scan.close()
    assert hits >= 15


def test_start_inside_a_voxel_min_range_min_points_and_a_thin_voxel(ctx, block):
    api = _api()
    vm, store = block["vm"], block["store"]
    slot = store["slot"]
    R, t = ri.exact_pose(0)
    origin = (0.25, 0.25, 0.25)  # the centre of cell (0, 0, 0), which is its voxel's mean
    scan = api.Scan(ctx, np.array([(1.25, 0.25, 0.25)]))

    def both(**kw):
        want = ri.cast(R, t, (1.25, 0.25, 0.25), store, ci.RES, 2.0, origin=origin, **kw)
        v, r, info = vm.raycast(scan, R, t, 2.0, origin=origin, **kw)
        assert v[0] == want["voxel"] and info["hits"] == int(want["voxel"] >= 0) and info["skipped"] == 0
        return int(v[0]), float(r[0])

    try:
        # the ray starts inside a valid voxel, at its mean: a hit at range 0 — the voxel id tells it from no hit
        assert both() == (slot[(0, 0, 0)], 0.0)
        # min_range passes over that hit; the next cell, (1, 0, 0), holds four points and is not valid: passed through;
        # (2, 0, 0) has its mean 1.0 along the ray
        assert both(min_range=0.25) == (slot[(2, 0, 0)], 1.0)
        # eight points per voxel: min_points = 8 changes nothing, 9 passes every voxel through
        assert both(min_range=0.25, min_points=8) == (slot[(2, 0, 0)], 1.0)
        assert both(min_points=9) == (-1, 0.0)
        # min_points = 4 admits the thin voxel's count, but it is not valid and stays passed through
        assert both(min_range=0.25, min_points=4) == (slot[(2, 0, 0)], 1.0)
    finally:
        scan.close()


def test_a_zero_length_ray_a_nan_point_and_a_far_cell_are_skipped_and_counted(ctx, block):
    api = _api()
    R = np.eye(3)
    t = np.array([float((1 << 19) - 1), 0.0, 0.0])  # the sensor sits one metre inside the addressable grid's upper x face
    pts = np.array([(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (float("nan"), 0.0, 0.0), (0.0, 1.0, 0.0)])
    scan = api.Scan(ctx, pts)
    try:
        want = [ri.cast(R, t, p, block["store"], ci.RES, 2.0) for p in pts]
        assert [c["skipped"] for c in want] == [True, False, True, True, False]  # b beyond 2^20 cells, len = 0, NaN
        v, r, info = block["vm"].raycast(scan, R, t, 2.0, points=True)
        assert np.all(v == -1) and np.all(r == 0.0)
        assert info["hits"] == 0 and info["skipped"] == 3 and len(info["scan"]) == 0
        info["scan"].close()
    finally:
        scan.close()
