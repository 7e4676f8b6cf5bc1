"""Cost of registering one voxel store against another (VoxelMap.match_map, pipeline.map_to_map) next to
what one has to do without it — upload the source's raw POINTS as a Scan and run scan_to_map on the target — and the error
maxima of the pair information.

usage: python tools/measure_voxel_map_match_map.py      (writes profiles/voxel_map_match_map.txt and prints it)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), one untimed call
first.  Target: about 500 k voxels of a 1 m grid at 40 points per voxel.  Sources: about 10 k and 500 k voxels, the
target's own points (of a corner box / all of them) seen from a frame at a general pose, so the stores overlap where the
pose says.  One round = one match and 40 LM iterations (tolerances 0: none stops early); a whole registration = the outer
loop from a start 0.05 m and 0.2° off.  The point route is charged the Scan's creation (upload included) once per
registration, as a caller holding only the submap's points pays it; its one-round line excludes it."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api, pipeline  # noqa: E402
from nonlinear_optimizer_for_slam_amd.solvers import Pose  # noqa: E402

REPEATS = 5
POINTS_PER_VOXEL = 40
LOSS = ("exponential", 1.0, 1.0)
OUT = os.path.join(ROOT, "profiles", "voxel_map_match_map.txt")
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def timed(ctx, call):
    """call() REPEATS + 1 times (the first one warms up) → (times in ms, the last result)"""
    ms, out = [], None
    for k in range(REPEATS + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        t = (time.perf_counter() - t0) * 1e3
        if k > 0:
            ms.append(t)
    return ms, out


def store_of(ctx, pts):
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for k in range(0, len(pts), 4_000_000):
        vm.insert(pts[k:k + 4_000_000])
    return vm


def rot_z(a):
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def one_round(dataset_of, R, t):
    ds, n = dataset_of()
    try:
        _, _, report = ds.solve6(R, t, LOSS, max_iterations=40, gradient_tolerance=0.0, parameter_tolerance=0.0)
    finally:
        ds.close()
    return n, report


def timings(ctx):
    rng = np.random.default_rng(20261019)
    R, t = rot_z(0.3), np.array([3.3, -1.7, 0.4])
    R0, t0 = R @ rot_z(np.deg2rad(0.2)), t + np.array([0.03, -0.03, 0.03])
    box = np.array([250.0, 250.0, 8.0])
    pts = rng.uniform([0.0, 0.0, 0.0], box, size=(int(box.prod()) * POINTS_PER_VOXEL, 3))
    target = store_of(ctx, pts)
    say("best of %d, spread = max - min; host clock, every call ends in a synchronisation; %d points per voxel" % (
        REPEATS, POINTS_PER_VOXEL))
    say("target: %d voxels (%d valid), %d points" % (len(target), target.n_valid, len(pts)))
    for corner in (np.array([50.0, 50.0, 4.0]), box):
        part = pts[np.all(pts < corner, axis=1)]
        local = (part - t) @ R  # Rᵀ (p − t)
        source = store_of(ctx, local)
        say("\n== source of %d voxels (%d valid), %d points ==" % (len(source), source.n_valid, len(local)))
        ms, (n, rep) = timed(ctx, lambda: one_round(lambda: target.match_map(source, R0, t0, 2, "f64"), R0, t0))
        say("one round, voxels:  match_map + 40 LM iterations       %8d matches: %s" % (n, best_and_spread(ms)))
        ms, _ = timed(ctx, lambda: target.match_map(source, R0, t0, 2, "f64")[0].close())
        say("            of which match_map alone                                     %s" % best_and_spread(ms))
        ms, out = timed(ctx, lambda: pipeline.map_to_map(ctx, target, source, Pose(R0, t0), loss=LOSS))
        say("registration, voxels: map_to_map                        %d rounds, |dt| %.1e: %s" % (
            len(out[1]), np.linalg.norm(out[0].t - t), best_and_spread(ms)))
        scan = api.Scan(ctx, local)
        ms, (n, rep) = timed(ctx, lambda: one_round(lambda: target.match(scan, R0, t0, 2, "f64"), R0, t0))
        say("one round, points:  match + 40 LM iterations           %8d matches: %s" % (n, best_and_spread(ms)))
        scan.close()

        def by_points():
            sc = api.Scan(ctx, local)
            try:
                return pipeline.scan_to_map(ctx, target, sc, Pose(R0, t0), loss=LOSS)
            finally:
                sc.close()
        ms, out = timed(ctx, by_points)
        say("registration, points: Scan(points) + scan_to_map        %d rounds, |dt| %.1e: %s" % (
            len(out[1]), np.linalg.norm(out[0].t - t), best_and_spread(ms)))
        source.close()
        del part, local
    target.close()


def error_maxima():
    """the random triples of tests/test_voxel_map_match_map_abi.py (host)"""
    import mpmath
    from nonlinear_optimizer_for_slam_amd import _lib
    from tests import voxel_d2d_inputs as di
    lib = _lib.hip_lib()
    worst = 0.0
    with mpmath.workdps(di.DPS):
        for tr, A in zip(di.random_triples(), di.random_references()):
            worst = max(worst, di.information_error(di.debug_pair_information(lib, *tr)[1], A))
    say("\n== pair information against 50 digits, %d random triples: max|S^T S - A| / max|A| ==" % di.N_TRIPLES)
    say("numpy restatement %.1f eps, voxel_pair_information (host) %.1f eps, bound %.1f eps" % (
        di.numpy_worst_error() / di.EPS, worst / di.EPS, di.bound() / di.EPS))


def main():
    ctx = Context((0,))
    timings(ctx)
    ctx.close()
    error_maxima()
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
