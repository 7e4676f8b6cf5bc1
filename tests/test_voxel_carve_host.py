"""The restatement of the carve's contract (tests/voxel_carve_inputs.py) checked on its own, without a GPU: the walk
visits 1 + n_x + n_y + n_z cells, starts in ca, ends in cb, moves one cell along one axis per step, and on the generic
scene agrees with the same walk in exact rational arithmetic (fractions.Fraction) for every ray that has no near-tie;
the scene itself is what the GPU tests take it for (few near-ties, the box seen through, the cap far away)."""
from fractions import Fraction

import numpy as np
import pytest

from tests import voxel_carve_inputs as ci


@pytest.fixture(scope="module")
def scene():
    return ci.generic_scene()


@pytest.fixture(scope="module")
def rays(scene):
    out = [ci.ray(scene["R"], scene["t"], p, ci.RES, 1.5 * ci.RES, 0.0, 1024 * ci.RES) for p in scene["scan_free"]]
    assert all(r is not None for r in out)
    return out


def test_fma_rounds_once():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
    assert a * b == 1.0 and ci.fma(a, b, -1.0) == -2.0 ** -60  # the product's low part survives only when fused
    assert ci.fma(3.0, 4.0, 5.0) == 17.0
    assert np.isnan(ci.fma(float("nan"), 1.0, 1.0))


def test_the_walk_visits_one_plus_the_steps_cells_and_ends_in_cb(rays):
    longest, total = 0, 0
    for r in rays:
        cells = ci.walk(r["a"], r["b"], r["ca"], r["cb"], ci.RES)
        n = sum(abs(r["cb"][k] - r["ca"][k]) for k in range(3))
        assert len(cells) == 1 + n and len(set(cells)) == len(cells)
        assert cells[0] == tuple(r["ca"]) and cells[-1] == tuple(r["cb"])
        for c0, c1 in zip(cells, cells[1:]):
            assert sorted(abs(c1[k] - c0[k]) for k in range(3)) == [0, 0, 1]
        longest, total = max(longest, len(cells)), total + len(cells)
    print("cells per ray: mean %.1f, max %d" % (total / len(rays), longest))
    assert 3 * (longest + 1) < 4096  # NOS_CARVE_MAX_CELLS never binds here


def test_the_double_walk_agrees_with_the_exact_walk_where_there_is_no_near_tie(rays):
    near = 0
    for r in rays:
        if ci.near_tie(r, ci.RES):
            near += 1
            continue
        exact = ci.walk(r["a"], r["b"], r["ca"], r["cb"], ci.RES, number=Fraction)
        assert ci.walk(r["a"], r["b"], r["ca"], r["cb"], ci.RES) == exact
    print("near-ties: %d of %d rays" % (near, len(rays)))
    assert near <= len(rays) // 100


def test_exact_ties_go_to_x_before_y_before_z():
    # the main diagonal of the lattice: every corner is a three-way tie
    for sign in (1.0, -1.0):
        a, b = [0.25 * sign] * 3, [1.75 * sign] * 3
        ca, cb = ci.cell_of(a, 2.0), ci.cell_of(b, 2.0)
        cells = ci.walk(a, b, ca, cb, 0.5)
        assert cells == ci.walk(a, b, ca, cb, 0.5, number=Fraction)
        s = int(sign)
        c = ca[0]
        want = [(c, c, c)]
        for _ in range(3):
            want += [(c + s, c, c), (c + s, c + s, c), (c + s, c + s, c + s)]
            c += s
        assert cells == want


def test_the_scene_is_what_the_gpu_tests_take_it_for(scene):
    cells = ci.cells_of_points(np.concatenate([scene["wall_points"], scene["box_points"]]))
    have = {tuple(int(x) for x in c) for c in cells}
    assert scene["box_cells"] <= have and len(scene["box_cells"]) >= 16
    assert 50 <= scene["n_box_rays"] < len(scene["scan_free"]) // 4  # some rays stop at the box, most do not
    R, t = scene["R"], scene["t"]
    crossings, hits, skipped, _ = ci.counts(cells, R, t, scene["scan_free"], ci.RES, 1.5 * ci.RES)
    assert skipped == 0
    gone = ci.removed(crossings, hits, 2, 1)
    gone_cells = {tuple(int(x) for x in c) for c in cells[gone]}
    assert scene["box_cells"] <= gone_cells  # the sensor sees through every box voxel at least twice
    print("voxels %d, removed by the rule %d, of them box %d" % (len(cells), int(gone.sum()), len(scene["box_cells"])))
    # with the box in place no box voxel goes: the rays stop on it, end_margin before its surface
    crossings, hits, _, _ = ci.counts(cells, R, t, scene["scan_box"], ci.RES, 1.5 * ci.RES)
    kept = ~ci.removed(crossings, hits, 2, 1)
    front = {tuple(int(x) for x in c) for c in cells[hits > 0]} & scene["box_cells"]
    assert front and all(kept[v] for v, c in enumerate(cells) if tuple(int(x) for x in c) in front)
