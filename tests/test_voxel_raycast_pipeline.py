"""Places from a map nobody scanned (pipeline.map_places), on the GPU: the room with four boxes of
tests/voxel_raycast_inputs.py goes into a store, through save() and load(), and is ray-cast from 20 node poses into a
PlaceDatabase.  An analytic scan taken 0.3 m from a node, at another yaw, must then find that node among its first two
candidates (the other is the room's 180° twin), with the distances the restatement gives for places rendered from the
same statistics; relocalize from the candidates' poses must end in the true node's basin, as near the true pose as a
registration started AT the true pose ends."""
import math

import numpy as np
import pytest

from tests import place_inputs as pi
from tests import voxel_carve_inputs as ci
from tests import voxel_raycast_inputs as ri

pytestmark = pytest.mark.gpu

LOSS = ("exponential", 1.0, 1.0)


@pytest.fixture(scope="module")
def built(ctx, tmp_path_factory):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    s = ri.place_scene()
    first = api.VoxelMap(ctx, ci.RES, 1.0)
    first.insert(s["points"])
    path = str(tmp_path_factory.mktemp("raycast") / "map.npz")
    first.save(path)
    first.close()
    vmap = api.VoxelMap.load(ctx, path)  # a map built by "another process": no scan stands behind it
    s["vmap"] = vmap
    s["node_poses"] = [Pose(np.eye(3), node) for node in s["nodes"]]
    beams = api.ray_pattern(120, np.radians(np.linspace(-20.0, 20.0, 16)))
    assert beams.tobytes() == s["pattern"].tobytes()
    s["db"], s["hits"] = pipeline.map_places(ctx, vmap, s["node_poses"], beams, max_range=ri.RAY_MAX_RANGE,
                                             n_rings=ri.PLACE["n_rings"], n_sectors=ri.PLACE["n_sectors"],
                                             descriptor_max_range=ri.PLACE["max_range"], z_floor=ri.PLACE["z_floor"])
    s["store"] = ri.store_of(vmap.stats())
    s["scans"] = [api.Scan(ctx, q[3]) for q in s["queries"]]
    s["found"] = [pipeline.loop_candidates(s["db"], scan, top_k=3) for scan in s["scans"]]
    s["rendered"] = {}
    yield s
    for h in s["scans"] + [s["db"], vmap]:
        h.close()


def _rendered(built, node):
    """the restatement's descriptor of place `node`, from the device's voxel statistics (computed once per node)"""
    if node not in built["rendered"]:
        pts, _, voxels, unsure = ri.render(built["store"], np.eye(3), built["nodes"][node], built["pattern"])
        built["rendered"][node] = (pi.descriptor(pts, **ri.PLACE)[0], int((voxels >= 0).sum()), unsure)
    return built["rendered"][node]


def test_the_database_is_indexed_like_the_poses(ctx, built):
    from nonlinear_optimizer_for_slam_amd import api
    db, vmap = built["db"], built["vmap"]
    assert len(db) == len(built["hits"]) == 20
    print("hits per pose:", built["hits"])
    assert all(0 < h <= 1920 for h in built["hits"])
    node = 7
    beams = api.Scan(ctx, built["pattern"])
    try:
        _, _, info = vmap.raycast(beams, np.eye(3), built["nodes"][node], ri.RAY_MAX_RANGE, points=True)
        desc, used = info["scan"].descriptor(ri.PLACE["n_rings"], ri.PLACE["n_sectors"], ri.PLACE["max_range"], ri.PLACE["z_floor"])
        info["scan"].close()
        assert info["hits"] == built["hits"][node] and used > 0
        assert db.get(node).tobytes() == desc.tobytes()
        want, want_hits, unsure = _rendered(built, node)
        print("place %d: %d hits, the restatement %d, %d rays at a decision margin" % (node, info["hits"], want_hits, unsure))
        assert unsure <= 19  # 1 % of the beams
        assert abs(info["hits"] - want_hits) <= unsure  # a ray at a decision margin may go either way
        # such a ray's point leaves one bin and enters another; every other bin holds the same maximum, to the rounding of
        # a range (a height changes by |sin 20°| of it at most)
        assert np.count_nonzero(np.abs(desc - want) > 1e-12) <= 2 * unsure
    finally:
        beams.close()


def test_a_query_scan_finds_its_node_among_the_first_two(built):
    for (node, R, t, points), found in zip(built["queries"], built["found"]):
        assert len(found) == 3
        ids = [f[0] for f in found]
        q = pi.descriptor(points, **ri.PLACE)[0]
        want, shift, _ = pi.distance(q, np.array([_rendered(built, i)[0] for i in ids]))
        print("node %d: found %s; the restatement's distances for them %s"
              % (node, ["%d: %.4f (yaw %.3f)" % f for f in found], ["%.4f" % d for d in want]))
        assert node in ids[:2], (node, ids)
        for (_, d, _), w in zip(found, want):
            assert abs(d - w) <= 0.01


def test_relocalize_ends_in_the_true_nodes_basin(ctx, built):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    vmap = built["vmap"]
    for (node, R, t, _), found, scan in zip(built["queries"], built["found"], built["scans"]):
        candidates = pipeline.candidate_poses(found, built["node_poses"])
        pose, info = pipeline.relocalize(ctx, vmap, scan, candidates, loss=LOSS)
        ref, _, _ = pipeline.scan_to_map(ctx, vmap, scan, initial_pose=Pose(R, t), loss=LOSS)
        d, d_ref = float(np.linalg.norm(pose.t - t)), float(np.linalg.norm(ref.t - t))
        rel = R.T @ pose.R
        dyaw = abs(math.atan2(rel[1, 0], rel[0, 0]))
        print("node %d: winner candidate %d (node %d); |t - t_true| = %.4f m, from the true pose %.4f m; |yaw - yaw_true| = %.4f rad"
              % (node, info["winner"], found[info["winner"]][0], d, d_ref, dyaw))
        assert found[info["winner"]][0] == node and dyaw < 0.5  # not the 180° twin
        assert d <= max(2.0 * d_ref, 0.01)
