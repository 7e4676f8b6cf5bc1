"""The yardsticks of the place-recognition tests, without a GPU: the numpy restatement of the rule (tests/place_inputs.py)
against pure-Python scalar loops on small inputs, and every condition the GPU tests rest on, for their fixed seeds:
the scan generator rejects under 1 % of its draws; at least 95 % of the seeded search pairs have a best shift that is more
than 1e-9 ahead of the second best; the places of the pipeline test are recognised by the restatement with a margin."""
import numpy as np
import pytest

from tests import place_inputs as pi


@pytest.mark.parametrize("params", pi.PARAM_SETS)
def test_descriptor_restatement_equals_the_scalar_loop(params):
    R, S = params
    pts, _ = pi.scan_points(700, R, S, seed=1)
    got, used = pi.descriptor(pts, R, S)
    want, want_used = pi.descriptor_slow(pts, R, S, pi.MAX_RANGE, pi.Z_FLOOR)
    assert np.array_equal(got, want) and used == want_used
    assert 0 < used < len(pts)
    # points beyond the range, below the floor and non-finite ones are among the inputs
    assert np.any(np.hypot(pts[:, 0], pts[:, 1]) >= pi.MAX_RANGE) and np.any(pts[:, 2] < pi.Z_FLOOR)
    assert np.any(np.isnan(pts)) and np.any(np.isposinf(pts)) and np.any(np.isneginf(pts))
    assert np.any((pts[:, 2] < 0.0) & (pts[:, 2] >= pi.Z_FLOOR))


def test_descriptor_conventions_in_the_restatement():
    # +x axis -> sector 0; the origin -> ring 0, sector 0; a ring boundary belongs to the outer ring; r == max_range is out
    d, used = pi.descriptor([[4.0, 0.0, 1.0], [0.0, 0.0, 0.5], [80.0, 0.0, 9.0], [1.0, 1.0, -2.0]], 20, 60)
    assert used == 3 and d[1, 0] == 3.0 and d[0, 0] == 2.5 and d[0, 7] == 0.0 and np.count_nonzero(d) == 2
    # the sector of -y is three quarters of the way round; an empty scan is all zeros
    d, used = pi.descriptor([[0.1, -1.0, 0.0]], 3, 4)
    assert used == 1 and d[0, 3] == 2.0
    d, used = pi.descriptor(np.zeros((0, 3)), 3, 5)
    assert used == 0 and not d.any()


@pytest.mark.parametrize("params", pi.PARAM_SETS)
def test_the_generator_rejects_under_one_percent(params):
    R, S = params
    for n in pi.SHAPES:
        _, rejected = pi.scan_points(n, R, S, seed=n)
        assert rejected <= 0.01 * max(n, 1), (n, rejected)


@pytest.mark.parametrize("params", pi.PARAM_SETS)
def test_distance_restatement_equals_the_scalar_loop(params):
    R, S = params
    descs = pi.random_descriptors(4, R, S, seed=3)
    descs[2] = 0.0
    d, shift, _ = pi.distance(descs[0], descs)
    for k in range(4):
        want_d, want_s = pi.distance_slow(descs[0], descs[k])
        assert d[k] == want_d and shift[k] == want_s, (k, d[k], want_d, shift[k], want_s)
    assert abs(d[0]) <= 1e-12 and shift[0] == 0 and d[2] == 1.0 and shift[2] == 0


def test_shift_convention_in_the_restatement():
    # q_j = c_(j+k): the query is the candidate rolled by -k along the sectors, and the shift is k
    R, S = 20, 60
    c = pi.random_descriptors(1, R, S, seed=5)[0]
    for k in (1, S - 1, S // 2):
        q = np.roll(c, -k, axis=1)
        d, shift, gap = pi.distance(q, c[None])
        assert abs(d[0]) <= 1e-12 and shift[0] == k and gap[0] > 1e-3


@pytest.mark.parametrize("params", pi.PARAM_SETS)
def test_most_seeded_pairs_have_a_clear_best_shift(params):
    R, S = params
    n = 257  # the stored descriptors and the three queries of tests/test_place_search.py
    descs = pi.random_descriptors(n + 3, R, S, seed=0)
    clear = 0
    for q in descs[n:]:
        _, _, gap = pi.distance(q, descs[:n])
        clear += int(np.count_nonzero(gap > 1e-9))
    assert clear >= 0.95 * 3 * n, (clear, 3 * n)


def test_the_places_are_recognised_by_the_restatement_with_a_margin():
    stored = np.array([pi.descriptor(pi.place_cloud(k))[0] for k in range(pi.N_PLACES)])
    for place, whole in pi.QUERIES:
        cloud, phi = pi.query_cloud(place, whole)
        q, used = pi.descriptor(cloud)
        d, shift, _ = pi.distance(q, stored)
        ranked = np.argsort(d, kind="stable")
        print("place %d: d %.4f, second %.4f (place %d), shift %d, used %d" % (place, d[ranked[0]], d[ranked[1]], ranked[1],
                                                                              shift[place], used))
        assert ranked[0] == place and d[ranked[1]] - d[place] >= 0.05
        assert shift[place] == int(round(phi * 60 / pi.TWO_PI)) == whole
