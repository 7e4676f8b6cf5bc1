"""Cost of matching a frame against the live voxel store (VoxelMap.match, nos_voxel_map_match) against the route the
parent of this feature runs: snapshot() of the whole store, then NdtMap.match on the snapshot's dense grid.

usage: python tools/measure_voxel_map_match.py [--single-match]      (output kept as profiles/voxel_map_match.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), the two routes
alternated in one session on the two stores of DESIGN.md §13's table (100 k and 796 k voxels), a 100 000-point frame,
unsorted and cell-sorted: (a) snapshot + k rounds of NdtMap.match, (b) k rounds of VoxelMap.match, k = 1, 4, 10; one
round of each on a 10 M-point scan; and the 80-frame windowed trajectory of tests/test_voxel_map_window.py run through
pipeline.odometry per frame with live_match off and on.  --single-match: one warmed-up VoxelMap.match and nothing else
after the set-up, for a kernel-trace run of its own
(rocprofv3 --kernel-trace --stats -- python tools/measure_voxel_map_match.py --single-match)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api, pipeline  # noqa: E402
from nonlinear_optimizer_for_slam_amd.solvers import Pose  # noqa: E402

FRAME = 100_000
REPEATS = 5
LOSS = ("exponential", 1.0, 1.0)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %8.3f ms  spread %7.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def fill(ctx, box, n_points, rng):
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for _ in range(n_points // 1_000_000):
        vm.insert(rng.uniform([0, 0, 0], box, size=(1_000_000, 3)))
    return vm


def snapshot_route(vm, scan, R, t, rounds):
    snap = vm.snapshot()
    n = 0
    for _ in range(rounds):
        ds, n = snap.match(scan, R, t)
        ds.close()
    snap.close()
    return n


def live_route(vm, scan, R, t, rounds):
    n = 0
    for _ in range(rounds):
        ds, n = vm.match(scan, R, t)
        ds.close()
    return n


def compare(vm, scan, R, t, rounds, label):
    na, nb = snapshot_route(vm, scan, R, t, rounds), live_route(vm, scan, R, t, rounds)  # warm-up, and the same answer
    assert na == nb, (na, nb)
    a, b = [], []
    for _ in range(REPEATS):  # alternated
        a.append(timed(lambda: snapshot_route(vm, scan, R, t, rounds))[0])
        b.append(timed(lambda: live_route(vm, scan, R, t, rounds))[0])
    print("%s k = %2d  (a) snapshot + k x NdtMap.match : %s" % (label, rounds, best_and_spread(a)))
    print("%s k = %2d  (b) k x VoxelMap.match          : %s   (a) - (b) = %+.3f ms, %d matches" % (
        label, rounds, best_and_spread(b), min(a) - min(b), nb))


def match_only(vm, scan, R, t, label):
    """one round on an existing snapshot against one round on the store: what a round costs on either structure"""
    snap = vm.snapshot()
    snap.match(scan, R, t)[0].close()
    vm.match(scan, R, t)[0].close()
    a, b = [], []
    for _ in range(REPEATS):
        ms, (ds, _) = timed(lambda: snap.match(scan, R, t))
        ds.close()
        a.append(ms)
        ms, (ds, _) = timed(lambda: vm.match(scan, R, t))
        ds.close()
        b.append(ms)
    snap.close()
    print("%s one round, snapshot already there: NdtMap.match   %s" % (label, best_and_spread(a)))
    print("%s one round                        : VoxelMap.match %s   live - dense = %+.3f ms" % (
        label, best_and_spread(b), min(b) - min(a)))


def trajectory(ctx, live):
    """the 80 frames of test_voxel_map_window.py's bounded-window test, registered and inserted by pipeline.odometry"""
    rng = np.random.default_rng(137)
    half = (20.0, 20.0, 4.0)
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    step = np.array([1.2, 0.9, 0.0])
    start = -39.5 * step
    per_frame, rounds = [], 0
    for f in range(80):
        center = np.round((start + f * step) * 1024) / 1024
        local = rng.integers([-15 * 1024, -15 * 1024, -2 * 1024], [15 * 1024, 15 * 1024, 2 * 1024], size=(30_000, 3)) / 1024.0
        scan = api.Scan(ctx, local)
        if f == 0:
            vm.insert(local + center)
        ms, (_, r) = timed(lambda: pipeline.odometry(ctx, vm, [scan], initial_pose=Pose(np.eye(3), center), loss=LOSS,
                                                     window_half_extent=half, live_match=live))
        scan.close()
        if f >= 5:  # the window has filled
            per_frame.append(ms)
            rounds += len(r[0])
    n = len(vm)
    vm.close()
    return per_frame, rounds, n


def main():
    single = "--single-match" in sys.argv
    rng = np.random.default_rng(20261017)
    ctx = Context((0,))
    R = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
    frame_local = rng.uniform([-20, -20, 0], [20, 20, 8], size=(FRAME, 3))  # a scan: 100 k points around the sensor
    if single:
        vm = fill(ctx, [100.0, 100.0, 10.0], 1_000_000, rng)
        scan = api.Scan(ctx, frame_local, sort_cell=1.0)
        t = np.array([50.0, 50.0, 1.0])
        vm.match(scan, R, t)[0].close()
        ctx.synchronize()
        ms, (ds, n) = timed(lambda: vm.match(scan, R, t))
        print("single VoxelMap.match of %d points: %.3f ms, %d matches, %d voxels in the store" % (FRAME, ms, n, len(vm)))
        return
    print("frame = %d points; best of %d, spread = max - min; host clock, every call ends in a synchronisation" % (FRAME, REPEATS))
    for label, box in (("100 k", [100.0, 100.0, 10.0]), ("796 k", [199.0, 200.0, 20.0])):
        t = np.array([box[0] / 2, box[1] / 2, 1.0])
        vm = fill(ctx, box, 10_000_000, rng)
        print("\n== store of %d voxels (%s) after %d points ==" % (len(vm), label, vm.n_points))
        for sort_cell, name in ((None, "unsorted   "), (1.0, "cell-sorted")):
            scan = api.Scan(ctx, frame_local, sort_cell=sort_cell)
            for rounds in (1, 4, 10):
                compare(vm, scan, R, t, rounds, name)
            match_only(vm, scan, R, t, name)
            scan.close()
        big_local = rng.uniform([-box[0] / 2, -box[1] / 2, 0], [box[0] / 2, box[1] / 2, 8], size=(10_000_000, 3))
        for sort_cell, name in ((None, "10 M unsorted   "), (1.0, "10 M cell-sorted")):
            big = api.Scan(ctx, big_local, sort_cell=sort_cell)
            compare(vm, big, np.eye(3), t, 1, name)
            match_only(vm, big, np.eye(3), t, name)
            big.close()
        del big_local
        vm.close()
    print("\n== 80-frame windowed trajectory (30 000 points per frame, window +-(20, 20, 4) m), pipeline.odometry per frame ==")
    for live in (False, True, False, True):  # alternated
        ms, rounds, n = trajectory(ctx, live)
        print("live_match=%-5s: per frame best %7.3f ms  median %7.3f ms  mean %7.3f ms over %d frames, %d rounds, %d voxels at the end" % (
            live, min(ms), float(np.median(ms)), float(np.mean(ms)), len(ms), rounds, n))
    ctx.close()


if __name__ == "__main__":
    main()
