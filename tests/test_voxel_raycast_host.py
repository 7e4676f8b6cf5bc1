"""The restatement of the ray cast's contract (tests/voxel_raycast_inputs.py) checked on its own, without a GPU
(DESIGN.md §32): its lazy walk visits the cells of the carve's walk in exact rational arithmetic on the exact inputs, ties
included, with consistent tau_in / tau_out; on the carve's generic scene the rule finds the walls and the box (at least
97 % of the rays hit, the median range error against the analytic distance is at most half a cell edge); on the room with
four boxes, places rendered from the map alone rank the true node of an analytic query scan among their first two."""
from fractions import Fraction

import numpy as np
import pytest

from tests import place_inputs as pi
from tests import voxel_carve_inputs as ci
from tests import voxel_raycast_inputs as ri


@pytest.mark.parametrize("pose", (0, 1, 2))
def test_the_lazy_walk_visits_the_cells_of_the_exact_walk_ties_included(pose):
    R, t = ri.exact_pose(pose)
    ties = 0
    for origin, p, max_range in ri.EXACT_RAYS:
        r = ri.ray(R, t, p, ci.RES, max_range, origin)
        assert r is not None
        visited = list(ri.cells_visited(r, ci.RES))
        exact = ci.walk(r["a"], r["b"], r["ca"], r["cb"], ci.RES, number=Fraction)
        assert [c for c, _, _ in visited] == exact, (origin, p)
        assert [c for c, _, _ in visited] == ci.walk(r["a"], r["b"], r["ca"], r["cb"], ci.RES)
        # tau_in / tau_out: 0 at the start, 1 at the end, each crossing shared by the two cells it parts, never decreasing
        assert visited[0][1] == 0.0 and visited[-1][2] == 1.0
        for (_, _, out), (_, tin, _) in zip(visited, visited[1:]):
            assert out == tin
        inner = [tin for _, tin, _ in visited]
        assert all(x <= y for x, y in zip(inner, inner[1:]))
        flat = sorted((tau, k) for k, row in enumerate(ci.crossing_taus(r["a"], r["b"], r["ca"], r["cb"], ci.RES, Fraction)) for tau in row)
        ties += sum(1 for (t0, k0), (t1, k1) in zip(flat, flat[1:]) if t0 == t1 and k0 != k1)
    assert ties >= 20  # the ties are there, and exact


def test_the_quick_warp_gives_the_bits_of_the_carves():
    rng = np.random.default_rng(3)
    poses = [ri.exact_pose(k) for k in range(3)] + [ci.general_pose(), (ri.rot_z(0.7), np.array([0.3, -8.0, 0.07]))]
    for R, t in poses:
        for p in rng.normal(size=(50, 3)) * 7.0:
            assert ri.warp(R, t, p) == ci.warp(R, t, p)


def test_skipped_rays():
    R, t = ri.exact_pose(0)
    nan = float("nan")
    assert ri.ray(R, t, (0.25, 0.25, 0.25), ci.RES, 1.0, (0.25, 0.25, 0.25)) is None  # zero length
    assert ri.ray(R, t, (nan, 0.0, 0.0), ci.RES, 1.0) is None
    assert ri.ray(R, t, (1.0, 0.0, 0.0), ci.RES, 0.5 * (1 << 20) + 1.0) is None  # b leaves the addressable grid
    assert ri.ray(R, t, (1.0, 0.0, 0.0), ci.RES, 0.5 * (1 << 20) - 1.0) is not None


@pytest.fixture(scope="module")
def generic():
    s = ci.generic_scene()
    s["store"] = ri.store_of(ri.numpy_stats(np.concatenate([s["wall_points"], s["box_points"]])))
    return s


def test_the_rule_finds_the_surfaces_of_the_generic_scene(generic):
    s = generic
    counts = np.array(s["store"]["counts"])
    print("voxels %d, median points per voxel %d" % (len(counts), int(np.median(counts))))
    n = 1500
    analytic = np.linalg.norm(s["scan_box"][:n], axis=1)  # the rays end on the wall or on the box
    a = ci.warp(s["R"], s["t"], (0.0, 0.0, 0.0))
    hit, err, visited = 0, [], 0
    for p, want in zip(s["scan_box"][:n], analytic):
        c = ri.cast(s["R"], s["t"], p, s["store"], ci.RES, 40.0, a=a)
        assert not c["skipped"]
        if c["voxel"] >= 0:
            hit += 1
            err.append(abs(c["range"] - want))
    err = np.array(err)
    print("hits %d of %d (%.1f %%); |range - analytic|: median %.3f m, 95th percentile %.3f m"
          % (hit, n, 100.0 * hit / n, float(np.median(err)), float(np.percentile(err, 95))))
    assert hit >= 0.97 * n
    assert np.median(err) <= 0.5 * ci.RES


def test_geometric_near_ties_are_rare_over_the_whole_segment(generic):
    s = generic
    a = ci.warp(s["R"], s["t"], (0.0, 0.0, 0.0))
    rays = [ri.ray(s["R"], s["t"], p, ci.RES, 40.0, a=a) for p in s["scan_box"]]
    near = sum(1 for r in rays if ri.near_tie(r, ci.RES))
    print("near-ties over the whole segment: %d of %d" % (near, len(rays)))
    assert near <= len(rays) // 100


@pytest.fixture(scope="module")
def places():
    """the room with four boxes: the map's statistics in numpy, the 20 places rendered from them by the restatement"""
    s = ri.place_scene()
    store = ri.store_of(ri.numpy_stats(s["points"]))
    desc = []
    for node in s["nodes"]:
        pts, _, _, _ = ri.render(store, np.eye(3), node, s["pattern"])
        desc.append(pi.descriptor(pts, **ri.PLACE)[0])
    s["descriptors"] = np.array(desc)
    return s


def test_places_rendered_from_the_map_rank_the_true_node_among_the_first_two(places):
    for node, R, t, scan in places["queries"]:
        q, used = pi.descriptor(scan, **ri.PLACE)
        d, shift, _ = pi.distance(q, places["descriptors"])
        order = sorted(range(len(d)), key=lambda i: (d[i], i))
        rank = order.index(node) + 1
        yaw = 2.0 * np.pi * int(shift[node]) / ri.PLACE["n_sectors"]
        print("node %d: rank %d; distances %s, third - second %.3f; yaw found %.3f, true %.3f"
              % (node, rank, ["%d: %.3f" % (i, d[i]) for i in order[:3]], d[order[2]] - d[order[1]], yaw,
                 float(np.arctan2(R[1, 0], R[0, 0])) % (2.0 * np.pi)))
        assert rank <= 2, (node, order[:3])
