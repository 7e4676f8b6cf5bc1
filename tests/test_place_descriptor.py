"""The Scan Context descriptor on the device (api.Scan.descriptor, PlaceDatabase.add / get), on the GPU:
bit for bit (np.array_equal) the numpy restatement of the rule (tests/place_inputs.py), n_used included.

The inputs are drawn by rejection so that no point lies within 1e-9 of a bin boundary in either index (place_inputs:
scan_points), so a device atan2 or a fused x x + y y that differs from numpy in the last bits cannot move a point; the
conventions at the boundaries themselves are pinned with exactly representable inputs."""
import numpy as np
import pytest

from tests import place_inputs as pi

pytestmark = pytest.mark.gpu

INVALID = 1


def _api():
    from nonlinear_optimizer_for_slam_amd import api
    return api


def _descriptor(ctx, pts, R, S, max_range=pi.MAX_RANGE, z_floor=pi.Z_FLOOR, **scan_kwargs):
    scan = _api().Scan(ctx, pts, **scan_kwargs)
    out = scan.descriptor(R, S, max_range, z_floor)
    scan.close()
    return out


def _same(got, want):
    assert got[1] == want[1], (got[1], want[1])
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), int(np.count_nonzero(got[0] != want[0]))


@pytest.mark.parametrize("params", pi.PARAM_SETS)
@pytest.mark.parametrize("n", pi.SHAPES)
def test_descriptor_equals_the_restatement_bit_for_bit(ctx, params, n):
    R, S = params
    pts, _ = pi.scan_points(n, R, S, seed=n)
    want = pi.descriptor(pts, R, S)
    got = _descriptor(ctx, pts, R, S)
    _same(got, want)
    if n >= 255:
        assert 0 < got[1] < n and np.count_nonzero(got[0]) > 0


def test_point_order_does_not_matter_and_two_calls_give_equal_bits(ctx):
    R, S = 20, 60
    pts, _ = pi.scan_points(100_003, R, S, seed=100_003)
    first = _descriptor(ctx, pts, R, S)
    again = _descriptor(ctx, pts, R, S)
    perm = np.random.default_rng(7).permutation(len(pts))
    shuffled = _descriptor(ctx, pts[perm], R, S)
    assert first[0].tobytes() == again[0].tobytes() and first[1] == again[1]
    assert first[0].tobytes() == shuffled[0].tobytes() and first[1] == shuffled[1]


def test_conventions_at_exactly_representable_inputs(ctx):
    # max_range / n_rings = 4: a power of two, so r and the ring product of the 3-4-5 points below are exact
    R, S, max_range, z_floor = 16, 8, 64.0, -2.0
    pts = np.array([
        [4.0, 0.0, 1.0],        # +x axis, r = 4 = a ring boundary: ring 1 (the outer one), atan2 exactly 0: sector 0
        [0.0, 0.0, 0.5],        # the origin: ring 0, sector 0
        [3.0, 4.0, 2.0],        # r = 5: ring 1
        [6.0, 8.0, 3.0],        # r = 10: ring 2
        [12.0, 16.0, 4.0],      # r = 20 = a ring boundary: ring 5
        [24.0, 32.0, 5.0],      # r = 40 = a ring boundary: ring 10
        [0.75, 1.0, -0.5],      # r = 1.25: ring 0, a negative z above the floor
        [64.0, 0.0, 9.0],       # r == max_range: not used
        [1.0, -3.0, -2.0],      # z == z_floor: used, and the bin holds 0.0 (sector 6.41: far from a boundary)
        [2.0, 0.0, 0.25],       # +x axis again, ring 0
    ])
    got = _descriptor(ctx, pts, R, S, max_range, z_floor)
    want = pi.descriptor(pts, R, S, max_range, z_floor)
    _same(got, want)
    d = got[0]
    sector_345 = int(np.floor(np.arctan2(4.0, 3.0) * (S / pi.TWO_PI)))
    assert d[1, 0] == 3.0 and d[0, 0] == 2.5
    assert d[1, sector_345] == 4.0 and d[2, sector_345] == 5.0 and d[5, sector_345] == 6.0 and d[10, sector_345] == 7.0
    assert d[0, sector_345] == 1.5
    assert d[15, 0] == 0.0               # nothing reached the last ring of sector 0: r == max_range is excluded
    assert sector_345 == 1 and d[0, 6] == 0.0  # (1, -3, z_floor): the bin holds max(z) - z_floor = 0.0 ...
    assert got[1] == 9                   # ... and the point was used: all but r == max_range
    # only that point in its bin: used, value exactly 0.0
    alone = _descriptor(ctx, np.array([[1.0, -3.0, -2.0]]), R, S, max_range, z_floor)
    assert alone[1] == 1 and not alone[0].any()
    # just below the floor: not used
    below = _descriptor(ctx, np.array([[1.0, -3.0, np.nextafter(-2.0, -np.inf)]]), R, S, max_range, z_floor)
    assert below[1] == 0 and not below[0].any()


def test_an_empty_scan_gives_zeros(ctx):
    got = _descriptor(ctx, np.zeros((0, 3)), 20, 60)
    assert got[1] == 0 and got[0].shape == (20, 60) and not got[0].any()


def test_defaults_are_twenty_by_sixty_to_eighty_metres_above_minus_two(ctx):
    pts, _ = pi.scan_points(257, 20, 60, seed=9)
    scan = _api().Scan(ctx, pts)
    got = scan.descriptor()
    scan.close()
    _same(got, pi.descriptor(pts, 20, 60, 80.0, -2.0))


@pytest.mark.parametrize("params", pi.PARAM_SETS)
def test_add_scan_then_get_equals_the_descriptor(ctx, params):
    R, S = params
    api = _api()
    pts, _ = pi.scan_points(257, R, S, seed=11)
    scan = api.Scan(ctx, pts)
    want = scan.descriptor(R, S)
    db = api.PlaceDatabase(ctx, n_rings=R, n_sectors=S)
    assert len(db) == 0
    assert db.add(scan) == 0 and db.add(want[0]) == 1 and len(db) == 2
    assert db.get(0).tobytes() == want[0].tobytes() and db.get(1).tobytes() == want[0].tobytes()
    with pytest.raises(api._lib.NosError) as err:
        db.get(2)
    assert err.value.status == INVALID
    db.close()
    scan.close()


def test_sorted_and_filtered_scans_give_the_descriptor_of_their_own_points(ctx):
    R, S = 20, 60
    api = _api()
    pts, _ = pi.scan_points(5000, R, S, seed=13, specials=False)  # the filter rejects non-finite coordinates
    plain = api.Scan(ctx, pts)
    want = plain.descriptor(R, S)
    cell_sorted = api.Scan(ctx, pts, sort_cell=2.0)
    _same(cell_sorted.descriptor(R, S), want)
    filtered = plain.filtered(1.5)
    kept = filtered.points()
    assert 0 < len(kept) < len(pts)
    _same(filtered.descriptor(R, S), pi.descriptor(kept, R, S))
    for h in (filtered, cell_sorted, plain):
        h.close()


def test_a_scan_of_another_context_is_rejected(ctx):
    api = _api()
    from nonlinear_optimizer_for_slam_amd import Context
    other = Context((0,))
    scan = api.Scan(other, np.zeros((4, 3)))
    db = api.PlaceDatabase(ctx)
    for call in (lambda: db.add(scan), lambda: db.search(scan)):
        with pytest.raises(api._lib.NosError) as err:
            call()
        assert err.value.status == INVALID
    assert len(db) == 0
    db.close()
    other.close()
