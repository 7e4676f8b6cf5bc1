"""Cost of ray casting the voxel store (VoxelMap.raycast) next to a carve's walk and a match of the same frame.

usage: python tools/measure_voxel_map_raycast.py      (writes profiles/voxel_map_raycast.txt and prints it)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), one untimed call
first.  Stores of 100 k and 796 k voxels at 1 m (every cell of a box filled, a million points per 100 k voxels and more:
every voxel valid and every visited cell found — a ray hits within a cell or two, the cheap end), and the same boxes as
SHELLS (only the cells on the faces filled: a ray crosses the empty inside before it hits, the walk's full cost), frames
of 100 k and 1 M rays around a sensor in the middle of the store, a general yaw.
raycast: ids and ranges copied back.  raycast, points: the hit points as a resident scan as well (select, gather, the
second wait).  carve, dry_run: the carve's walk over the same frame (it never stops early, and counts by atomics).
match: VoxelMap.match of the same frame."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

REPEATS = 5
OUT = os.path.join(ROOT, "profiles", "voxel_map_raycast.txt")
LINES = []
MAX_RANGE = 120.0


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def repeat(fn):
    fn()
    return [timed(fn)[0] for _ in range(REPEATS)]


def close_scan(result):
    result[2]["scan"].close()


def filled(rng, box):
    return [rng.uniform([0, 0, 0], box, size=(1_000_000, 3)) for _ in range(10)]


def shell(rng, box):
    """points in the one-cell layer inside the six faces of the box"""
    box = np.array(box)
    out = []
    for _ in range(4):
        p = rng.uniform([0, 0, 0], box, size=(1_000_000, 3))
        axis, side = rng.integers(0, 3, size=len(p)), rng.integers(0, 2, size=len(p))
        depth = rng.uniform(0.0, 1.0, size=len(p))
        p[np.arange(len(p)), axis] = np.where(side == 0, depth, box[axis] - depth)
        out.append(p)
    return out


def main():
    rng = np.random.default_rng(20261020)
    ctx = Context((0,))
    R = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
    say("best of %d, spread = max - min; host clock, every call ends in a synchronisation; max_range %g m" % (REPEATS, MAX_RANGE))
    for label, box, fill in (("100 k voxels, filled", [100.0, 100.0, 10.0], filled), ("796 k voxels, filled", [199.0, 200.0, 20.0], filled),
                             ("shell of the 100 k box", [100.0, 100.0, 10.0], shell), ("shell of the 796 k box", [199.0, 200.0, 20.0], shell)):
        vm = api.VoxelMap(ctx, 1.0, 1.0)
        for batch in fill(rng, box):
            vm.insert(batch)
        t = np.array([box[0] / 2, box[1] / 2, box[2] / 2])
        for n_frame in (100_000, 1_000_000):
            local = rng.uniform([-20, -20, -4], [20, 20, 4], size=(n_frame, 3))  # a scan around the sensor
            scan = api.Scan(ctx, local)
            voxels, ranges, info = vm.raycast(scan, R, t, MAX_RANGE)
            say("\n== store of %d voxels (%d valid; %s), frame of %d rays: %d hit at a mean range of %.1f m, %d skipped ==" % (
                len(vm), vm.n_valid, label, n_frame, info["hits"], float(ranges[voxels >= 0].mean()) if info["hits"] else 0.0,
                info["skipped"]))
            ms = repeat(lambda: vm.raycast(scan, R, t, MAX_RANGE))
            say("raycast                                   : %s" % best_and_spread(ms))
            ms = repeat(lambda: close_scan(vm.raycast(scan, R, t, MAX_RANGE, points=True)))
            say("raycast, points=True (hit scan, then freed): %s" % best_and_spread(ms))
            ms = repeat(lambda: vm.carve(scan, R, t, dry_run=True, max_range=MAX_RANGE))
            say("carve, dry_run, of the same frame         : %s" % best_and_spread(ms))
            ms = repeat(lambda: vm.match(scan, R, t)[0].close())
            say("VoxelMap.match of the same frame          : %s" % best_and_spread(ms))
            scan.close()
        vm.close()
    ctx.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
