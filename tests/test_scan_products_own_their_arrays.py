"""A scan that the device produces — by the filter, the deskew or the hit points of a ray cast — owns its two device arrays
(csrc/nos_internal.hpp, NewScan): it outlives the scan it was made from, in its empty form too, on the GPU.

Shapes: source scans of 0, 1, 65 and 257 points (empty, one lane, a wave plus one, a block plus one), sorted by cell so that
they carry an order array, and a store of 17 voxels, one past the minimum capacity of 16.  The source is destroyed FIRST;
then every product's points(), order and len are held against values computed beforehand and the product is inserted into
a store.

References.  Filter: the first point (smallest original index) of every unit cell, in stored order — exact, with an edge
of 1 the device's floor(p * (1 / edge)) is numpy's floor(p).  Deskew: tests/scan_deskew_inputs.py::restate within 1e-12, what
test_scan_deskew.py::test_rejected_calls_write_nothing_and_leave_the_context_usable grants it at these magnitudes.  Hit
points: (range / len) p from the ranges the same cast returned, within 2 ulp per component — quotient and product are
rounded once each on either side, the bound of test_voxel_map_raycast.py::test_hit_points_and_their_descriptor.

Left to existing tests: a deskew rejected for a missing time stamp (it fails after its output arrays exist) followed at once
by a correct call on the same context — test_scan_deskew.py::test_rejected_calls_write_nothing_and_leave_the_context_usable
asserts status, text, the untouched handle and the follow-up call's points."""
import ctypes

import numpy as np
import pytest

from tests import scan_deskew_inputs as di

pytestmark = pytest.mark.gpu

I3, Z3 = np.eye(3), np.zeros(3)
XI = np.array([0.3, -0.2, 0.05, 0.02, -0.01, 0.15])
SIZES = (0, 1, 65, 257)
N_VOXELS = 17
MAX_RANGE = 40.0


def _api():
    from nonlinear_optimizer_for_slam_amd import api
    return api


def _has_order_array(scan):
    """struct nos_scan (csrc/nos_internal.hpp) is {ctx, n, d_planes, d_order}: four 8-byte words; the last is NULL or not."""
    words = (ctypes.c_size_t * 4).from_address(scan._h.value)
    assert words[1] == len(scan) and words[2] != 0  # n and a planes block, which even the empty form has
    return words[3] != 0


@pytest.fixture(scope="module")
def world():
    """17 voxels of 8 points each around the sensor, and 257 points: three of four aim at a voxel's mean (a sure hit, at
    the mean the beam is at Mahalanobis distance 0), every fourth goes up, where there is nothing."""
    rng = np.random.default_rng(17)
    cells = np.array([(3 + (k % 6) * 2, -6 + (k // 6) * 5, (k % 3) - 1) for k in range(N_VOXELS)], dtype=np.float64)
    assert len({tuple(c) for c in cells}) == N_VOXELS
    store_points = (cells[:, None, :] + 0.5 + rng.uniform(-0.3, 0.3, size=(N_VOXELS, 8, 3))).reshape(-1, 3)
    means = store_points.reshape(N_VOXELS, 8, 3).mean(axis=1)
    n = SIZES[-1]
    pts = means[np.arange(n) % N_VOXELS] * rng.uniform(0.6, 1.4, size=(n, 1))
    pts[3::4] = np.array([0.1, 0.2, 5.0]) * rng.uniform(0.6, 1.4, size=(len(pts[3::4]), 1))
    times = rng.uniform(0.0, 1.0, size=n)
    return {"store_points": store_points, "points": pts, "times": times}


def _store(ctx, world):
    vm = _api().VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    vm.insert(world["store_points"])
    assert len(vm) == vm.n_valid == N_VOXELS and vm.memory()["capacity"] == 32
    return vm


def _filter_reference(stored, order):
    """→ positions kept by a unit-cell filter of a scan with these stored points and original indices."""
    cells = [tuple(c) for c in np.floor(stored).astype(np.int64)]
    first = {}
    for j, c in enumerate(cells):
        if c not in first or order[j] < order[first[c]]:
            first[c] = j
    return np.array(sorted(first.values()), dtype=np.int64)


def _check_insert(ctx, product, want_points):
    """one insert of the product into a fresh store: as many points, the cells of the reference"""
    vm = _api().VoxelMap(ctx, 1.0, 1.0)
    touched = vm.insert_scan(product, I3, Z3)
    n_cells = len({tuple(c) for c in np.floor(want_points).astype(np.int64)})
    assert vm.n_points == len(want_points) and len(vm) == n_cells
    assert touched == n_cells
    vm.close()


@pytest.mark.parametrize("n", SIZES)
def test_products_outlive_their_source(ctx, world, n):
    api = _api()
    pts, times = world["points"][:n], world["times"][:n]
    vm = _store(ctx, world)
    source = api.Scan(ctx, pts, sort_cell=1.0) if n > 0 else api.Scan(ctx, pts)
    order = source.order.astype(np.int64)
    stored = pts[order]
    assert np.array_equal(source.points(), stored) and _has_order_array(source) == (n > 0)
    filtered = source.filtered(1.0)
    deskewed = source.deskewed(times, XI)
    voxels, ranges, info = vm.raycast(source, I3, Z3, MAX_RANGE, points=True)
    hits = info["scan"]
    # the references, all before the source goes
    keep = _filter_reference(stored, order)
    want_deskewed = di.restate(pts, times, 1.0, XI)[order] if n > 0 else np.zeros((0, 3))
    hit = np.flatnonzero(voxels >= 0)
    length = np.sqrt((stored[hit, 0] ** 2 + stored[hit, 1] ** 2) + stored[hit, 2] ** 2)
    want_hits = (ranges[hit] / length)[:, None] * stored[hit]
    if n > 0:
        aimed = (order % 4) != 3
        assert np.all(voxels[aimed] >= 0) and np.all(voxels[~aimed] == -1) and info["hits"] == int(aimed.sum()) > 0
        assert 0 < len(keep) <= n
    source.close()
    # a second allocation of the sizes just freed, filled with something else, so that a product that still pointed
    # into the source's arrays would read it
    decoy = api.Scan(ctx, np.full((max(n, 1), 3), 777.0), sort_cell=1.0)
    try:
        assert len(filtered) == len(keep) and np.array_equal(filtered.points(), stored[keep])
        assert np.array_equal(filtered.order, order[keep].astype(np.uint32))
        assert len(deskewed) == n and np.array_equal(deskewed.order, order.astype(np.uint32))
        got = deskewed.points()
        assert got.shape == (n, 3) and (n == 0 or np.max(np.abs(got - want_deskewed)) < 1e-12)
        assert len(hits) == len(hit) and np.array_equal(hits.order, order[hit].astype(np.uint32))
        assert np.all(np.abs(hits.points() - want_hits) <= 2.0 * np.spacing(np.abs(want_hits)))
        # which of them carries an order array: a filtered scan and a hit scan always, a deskewed one as its source did,
        # the empty form never
        assert _has_order_array(filtered) == _has_order_array(hits) == _has_order_array(deskewed) == (n > 0)
        _check_insert(ctx, filtered, stored[keep])
        _check_insert(ctx, deskewed, want_deskewed)
        _check_insert(ctx, hits, want_hits)
    finally:
        for h in (decoy, hits, deskewed, filtered, vm):
            h.close()


def test_a_cast_in_which_no_ray_hits_gives_the_empty_form(ctx, world):
    api = _api()
    vm = _store(ctx, world)
    rays = np.array([0.1, 0.2, 5.0]) * np.linspace(0.6, 1.4, 65)[:, None]  # the direction in which `world` has nothing
    up = api.Scan(ctx, rays, sort_cell=1.0)
    voxels, ranges, info = vm.raycast(up, I3, Z3, MAX_RANGE, points=True)
    hits = info["scan"]
    assert len(up) == 65 and np.all(voxels == -1) and info["hits"] == 0 and info["skipped"] == 0
    up.close()
    try:
        assert len(hits) == 0 and hits.points().shape == (0, 3) and hits.order.size == 0 and not _has_order_array(hits)
        _check_insert(ctx, hits, np.zeros((0, 3)))
    finally:
        hits.close()
        vm.close()


def test_which_products_carry_an_order_array(ctx, world):
    api = _api()
    pts, times = world["points"][:65], world["times"][:65]
    plain, empty = api.Scan(ctx, pts), api.Scan(ctx, np.zeros((0, 3)))
    made = [plain, empty]
    try:
        assert not _has_order_array(plain) and not _has_order_array(empty)
        made.append(plain.deskewed(times, XI))  # an unsorted source has none to copy
        assert not _has_order_array(made[-1]) and np.array_equal(made[-1].order, np.arange(65))
        made.append(plain.filtered(1.0))  # a filtered scan names the points it kept
        assert _has_order_array(made[-1]) and 0 < len(made[-1]) < 65
        for product in (empty.filtered(1.0), empty.deskewed(np.zeros(0), XI)):
            made.append(product)
            assert len(product) == 0 and not _has_order_array(product)
    finally:
        for h in reversed(made):
            h.close()
