"""Cost of batched registration against the live voxel store (api.register6_batch on a VoxelMap,
nos_voxel_map_register6_batch) and of pipeline.odometry(one_launch=True), against the routes the parent of this feature
runs: snapshot() of the store followed by register6_batch on the NdtMap, and pipeline.odometry(live_match=True).

usage: python tools/measure_voxel_map_register.py      (output kept as profiles/voxel_map_register.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), the two routes
alternated in one session.  (a) B = 1, 64 and 1 024 scans of 500 points against a store of ~100 k voxels: snapshot() +
register6_batch against register6_batch on the store; the results are checked to be the same bits first.  (b) per-frame
time of pipeline.odometry over a 40-frame windowed trajectory at 500 and 5 000 points per scan, live_match=True against
one_launch=True (one workgroup runs a whole frame there: the large scan is expected to favour the lone path, DESIGN.md
§12)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api, pipeline  # noqa: E402
from nonlinear_optimizer_for_slam_amd.solvers import Pose  # noqa: E402

REPEATS = 5
LOSS = ("exponential", 1.0, 1.0)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def surface(rng, n, lo, hi):
    """points of a wavy sheet with 2 cm of noise: a map a scan can be registered to"""
    xy = rng.uniform(lo, hi, size=(n, 2))
    z = 0.45 * np.sin(0.9 * xy[:, 0]) + 0.35 * np.cos(0.7 * xy[:, 1]) + rng.normal(scale=0.02, size=n)
    return np.column_stack([xy, z])


def snapshot_route(vm, scans, R0, t0):
    snap = vm.snapshot()
    try:
        return api.register6_batch(snap, scans, R0, t0, LOSS, keep_multiple=4)
    finally:
        snap.close()


def live_route(vm, scans, R0, t0):
    return api.register6_batch(vm, scans, R0, t0, LOSS, keep_multiple=4)


def batches(ctx, rng):
    half = 160.0
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for _ in range(4):
        vm.insert(surface(rng, 1_000_000, -half, half))
    print("\n== (a) register6_batch, scans of 500 points, store of %d voxels (%d valid) ==" % (len(vm), vm.n_valid))
    Rt = np.array([[np.cos(0.02), -np.sin(0.02), 0.0], [np.sin(0.02), np.cos(0.02), 0.0], [0.0, 0.0, 1.0]])
    scans = []
    for _ in range(64):  # 64 different scans around different places; B = 1 024 repeats them from other start poses
        c = rng.uniform(-half + 20, half - 20, size=2)
        world = surface(rng, 500, -8.0, 8.0) + np.array([c[0], c[1], 0.0])
        world[:, 2] = 0.45 * np.sin(0.9 * world[:, 0]) + 0.35 * np.cos(0.7 * world[:, 1]) + rng.normal(scale=0.02, size=500)
        tt = np.array([c[0] + 0.05, c[1] - 0.04, 0.02])
        scans.append((api.Scan(ctx, (Rt.T @ (world - tt).T).T), np.array([c[0], c[1], 0.0])))
    for B in (1, 64, 1024):
        batch = [scans[i % 64][0] for i in range(B)]
        R0 = np.tile(np.eye(3).reshape(9), (B, 1))
        t0 = np.array([scans[i % 64][1] for i in range(B)]) + rng.uniform(-0.05, 0.05, size=(B, 3)) * (np.arange(B)[:, None] >= 64)
        a, b = snapshot_route(vm, batch, R0, t0), live_route(vm, batch, R0, t0)  # warm-up, and the same answer
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and repr(a[2]) == repr(b[2]), "the two routes differ"
        rounds = sum(len(r["rounds"]) for r in b[2])
        ta, tb = [], []
        for _ in range(REPEATS):  # alternated
            ta.append(timed(lambda: snapshot_route(vm, batch, R0, t0))[0])
            tb.append(timed(lambda: live_route(vm, batch, R0, t0))[0])
        print("B = %4d  (a) snapshot + register6_batch(NdtMap) : %s" % (B, best_and_spread(ta)))
        print("B = %4d  (b) register6_batch(VoxelMap)          : %s   (a) / (b) = %.2f, %d of %d ok, %d rounds" % (
            B, best_and_spread(tb), min(ta) / min(tb), sum(r["ok"] for r in b[2]), B, rounds))
    for sc, _ in scans:
        sc.close()
    vm.close()


def trajectory(ctx, n_points, one_launch):
    """40 frames along a wavy sheet, window +-(20, 20, 4) m, registered and inserted by pipeline.odometry per frame"""
    rng = np.random.default_rng(137)
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    step = np.array([0.25, 0.15, 0.0])
    per_frame, rounds = [], 0
    pose = Pose(np.eye(3), np.zeros(3))
    for f in range(40):
        center = f * step
        world = surface(rng, n_points, -15.0, 15.0) + np.array([center[0], center[1], 0.0])
        world[:, 2] = 0.45 * np.sin(0.9 * world[:, 0]) + 0.35 * np.cos(0.7 * world[:, 1]) + rng.normal(scale=0.02, size=n_points)
        if f == 0:
            vm.insert(surface(rng, 200_000, -20.0, 20.0))
        scan = api.Scan(ctx, world - center)  # the sensor moves without turning
        kw = dict(one_launch=True) if one_launch else dict(live_match=True)
        ms, (poses, r) = timed(lambda: pipeline.odometry(ctx, vm, [scan], initial_pose=pose, loss=LOSS, keep_multiple=4,
                                                         window_half_extent=(20.0, 20.0, 4.0), **kw))
        pose = poses[0]
        scan.close()
        if f >= 5:
            per_frame.append(ms)
            rounds += len(r[0])
    n = len(vm)
    vm.close()
    return per_frame, rounds, n, pose


def main():
    rng = np.random.default_rng(20261017)
    ctx = Context((0,))
    print("best of %d, spread = max - min; host clock, every call ends in a synchronisation" % REPEATS)
    batches(ctx, rng)
    for n_points in (500, 5000):
        print("\n== (b) pipeline.odometry per frame, %d points per scan, 40-frame windowed trajectory ==" % n_points)
        for one_launch in (False, True, False, True):  # alternated
            ms, rounds, n, pose = trajectory(ctx, n_points, one_launch)
            print("%-16s: per frame best %8.3f ms  median %8.3f ms  mean %8.3f ms over %d frames, %d rounds, %d voxels at the "
                  "end, final t = (%.4f, %.4f, %.4f)" % ("one_launch=True" if one_launch else "live_match=True", min(ms),
                                                        float(np.median(ms)), float(np.mean(ms)), len(ms), rounds, n, *pose.t))
    ctx.close()


if __name__ == "__main__":
    main()
