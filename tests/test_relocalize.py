"""pipeline.relocalize on the GPU: every candidate pose scored in one call (api.score_batch), the best few registered in one
launch (scan_to_map_batch), the final poses scored again, the best returned.

The scene is the reference's room (synth.room_points, a 7 x 5 x 2.5 m box without a ceiling) and every fifth point of its
"simple" scan (synth.room_scan, about 1 900 points).  Candidates: one 4 cm and 0.02 rad from the true pose, and twelve at
least 1.5 m or 0.5 rad away.  The room maps onto itself under a half turn about its axis, so the true pose has a mirror
twin at yaw + π: no candidate is within a quarter turn of it.  Before anything is asked of the GPU result, the CPU oracle
(match_point_cloud + ndt6_accumulate on the map's own voxel statistics) must give the near candidate a fitness at least
1 % above the second best, so that no rounding can reorder them."""
import numpy as np
import pytest

from oracle import oracle_scene as scene

pytestmark = pytest.mark.gpu

LOSS = ("exponential", 1.0, 1.0)
FAR = [(1.5, 0.0, 0.0), (-1.5, 0.0, 0.0), (0.0, 1.5, 0.0), (0.0, -1.5, 0.0), (2.0, 1.0, 0.0), (0.0, 0.0, 0.5),
       (0.0, 0.0, -0.5), (0.0, 0.0, 1.0), (0.0, 0.0, -1.2), (1.5, 0.0, 0.5), (-1.6, 0.3, -0.7), (0.0, 0.0, 1.57)]


def _yaw(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def room():
    from nonlinear_optimizer_for_slam_amd import synth
    points = synth.room_points()
    local, R_true, t_true = synth.room_scan(points)
    return points, local[::5].copy(), R_true, t_true


def _candidates(t_true, yaw_true=0.1):
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    out = [Pose(_yaw(yaw_true + 0.02), t_true + np.array([0.03, -0.02, 0.01]))]
    for dx, dy, dyaw in FAR:
        assert np.hypot(dx, dy) >= 1.5 or abs(dyaw) >= 0.5
        assert abs(dyaw) <= np.pi / 2 + 1e-9  # at least a quarter turn from the mirror twin
        out.append(Pose(_yaw(yaw_true + dyaw), t_true + np.array([dx, dy, 0.0])))
    return out


def _oracle_fitness(oracle, stats, pts, pose):
    planes, n, _ = scene.match_point_cloud(stats["means"], stats["sqrt_infos"].reshape(-1, 9), stats["valid"], pts, pose.R, pose.t,
                                           1.0, 2)
    return LOSS[1] * n - float(oracle.ndt6_accumulate(planes, pose.R, pose.t, LOSS)[27])


@pytest.mark.parametrize("kind", ["ndt", "voxel"])
def test_relocalize_picks_the_near_candidate_and_returns_its_registration(ctx, oracle, room, kind):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    points, local, R_true, t_true = room
    assert 1500 <= len(local) <= 2500
    if kind == "ndt":
        m, stats = api.NdtMap.build(ctx, points, 1.0, 1.0)
    else:
        m = api.VoxelMap(ctx, 1.0, 1.0)
        m.insert(points)
        stats = m.stats()
    scan = api.Scan(ctx, local)
    # the intended use: stage 1 on a coarser scan (the live store), or on the scan itself (the snapshot map)
    score_scan = scan.filtered(0.3) if kind == "voxel" else None
    stage1_points = score_scan.points() if score_scan is not None else local
    assert len(stage1_points) >= 300
    candidates = _candidates(t_true)
    want = np.array([_oracle_fitness(oracle, stats, stage1_points, c) for c in candidates])
    second = np.sort(want)[-2]
    print(kind, "oracle fitness: near %.6g, second %.6g" % (want[0], second))
    assert want[0] >= 1.01 * second and second > 0.0, want

    pose, info = pipeline.relocalize(ctx, m, scan, candidates, loss=LOSS, top_k=4, score_scan=score_scan)
    # stage 1
    assert len(info["scores"]) == len(candidates) and len(info["chosen"]) == 4
    assert info["chosen"][0] == 0
    np.testing.assert_allclose(info["fitness"], want, rtol=1e-6)
    assert list(info["chosen"]) == sorted(range(len(candidates)), key=lambda i: (-info["fitness"][i], i))[:4]
    # the winner: bit for bit its scan_to_map_batch row, and no other row's final fitness is above its own
    k = info["chosen"].index(info["winner"])
    row = info["registrations"][k]
    assert row is not None
    assert pose.R.tobytes() == row[0].R.tobytes() and pose.t.tobytes() == row[0].t.tobytes()
    assert np.all(info["final_fitness"][k] >= info["final_fitness"])
    ties = [info["chosen"][j] for j in range(4) if info["final_fitness"][j] == info["final_fitness"][k]]
    assert info["winner"] == min(ties)
    fs = info["final_scores"][k]
    assert info["final_fitness"][k] == LOSS[1] * float(fs["matches"]) - float(fs["cost"])
    # the rows are what the two calls underneath give
    again = pipeline.scan_to_map_batch(ctx, m, [scan] * 4, [candidates[i] for i in info["chosen"]], loss=LOSS)
    assert again[k][0].R.tobytes() == pose.R.tobytes() and again[k][0].t.tobytes() == pose.t.tobytes()
    dt = float(np.linalg.norm(pose.t - t_true))
    dyaw = float(abs(np.arctan2(pose.R[1, 0], pose.R[0, 0]) - 0.1))
    print(kind, "winner %d, |t - t_true| = %.3g m, |yaw - yaw_true| = %.3g rad" % (info["winner"], dt, dyaw))
    assert dt < 0.1 and dyaw < 0.05  # it started 0.04 m and 0.02 rad away
    # a custom key (fewest unmatched points first) and another loss
    pose_h, info_h = pipeline.relocalize(ctx, m, scan, candidates, loss=("huber", 1.0), top_k=2,
                                         key=lambda s: s["matched_points"].astype(np.float64))
    assert len(info_h["chosen"]) == 2 and info_h["winner"] in info_h["chosen"]
    with pytest.raises(ValueError):
        pipeline.relocalize(ctx, m, scan, candidates, loss=("huber", 1.0))
    with pytest.raises(ValueError):
        pipeline.relocalize(ctx, m, scan, candidates, loss=None)
    for h in (score_scan, scan, m):
        if h is not None:
            h.close()
