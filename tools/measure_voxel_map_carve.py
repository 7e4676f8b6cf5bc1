"""Cost of line-of-sight carving (VoxelMap.carve) next to what a frame already costs.

usage: python tools/measure_voxel_map_carve.py      (writes profiles/voxel_map_carve.txt and prints it)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), one untimed call
first.  Stores of 100 k and 796 k voxels at 1 m (every cell of a box filled: the worst case for the walk, every visited
cell is found and counted), frames of 100 k and 1 M points around a sensor in the middle of the store, a general yaw.
carve, nothing to remove: min_crossings above any count — the walk, the keep pass, the scan, one wait.
carve, dry_run: the default rule, counted only.
carve, a few hundred removed: min_crossings chosen from a dry run's counters so that about 300 voxels reach it, min_hits
above any count; every timed call works on a fresh copy of the store (merge of the original into an empty store).
The three orders of the same frame answer whether sorting the rays pays: as generated (random), sorted by cell
(Scan(sort_cell=...)), sorted by ray length on the host."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

REPEATS = 5
OUT = os.path.join(ROOT, "profiles", "voxel_map_carve.txt")
LINES = []
NEVER = 2 ** 31


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


def copy_of(ctx, vm):
    out = api.VoxelMap(ctx, vm.voxel_resolution, vm.search_radius_sq, capacity=len(vm))
    out.merge(vm)
    return out


def main():
    rng = np.random.default_rng(20261020)
    ctx = Context((0,))
    R = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
    say("best of %d, spread = max - min; host clock, every call ends in a synchronisation" % REPEATS)
    for label, box in (("100 k voxels", [100.0, 100.0, 10.0]), ("796 k voxels", [199.0, 200.0, 20.0])):
        vm = api.VoxelMap(ctx, 1.0, 1.0)
        for _ in range(10):
            vm.insert(rng.uniform([0, 0, 0], box, size=(1_000_000, 3)))
        t = np.array([box[0] / 2, box[1] / 2, 1.0])
        everything = (np.array(box) / 2, np.array(box))
        for n_frame in (100_000, 1_000_000):
            local = rng.uniform([-20, -20, 0], [20, 20, 8], size=(n_frame, 3))  # a scan around the sensor
            scan = api.Scan(ctx, local)
            n, info = vm.carve(scan, R, t, dry_run=True, counts=True)
            cells = int(info["crossings"].astype(np.int64).sum())
            say("\n== store of %d voxels (%s), frame of %d points: %.1f cells found per ray, %d rays skipped ==" % (
                len(vm), label, n_frame, cells / n_frame, info["skipped"]))
            ms = repeat(lambda: vm.carve(scan, R, t, min_crossings=NEVER))
            say("carve, nothing to remove                      : %s" % best_and_spread(ms))
            ms = repeat(lambda: vm.carve(scan, R, t, dry_run=True))
            say("carve, dry_run (default rule, %6d would go)  : %s" % (n, best_and_spread(ms)))
            ms = repeat(lambda: vm.carve(scan, R, t, dry_run=True, counts=True))
            say("carve, dry_run with the counters copied back  : %s" % best_and_spread(ms))
            by_cell = api.Scan(ctx, local, sort_cell=1.0)
            ms = repeat(lambda: vm.carve(by_cell, R, t, min_crossings=NEVER))
            say("carve, nothing to remove, scan sorted by cell : %s" % best_and_spread(ms))
            by_cell.close()
            by_length = api.Scan(ctx, local[np.argsort(np.linalg.norm(local, axis=1))])
            ms = repeat(lambda: vm.carve(by_length, R, t, min_crossings=NEVER))
            say("carve, nothing to remove, rays sorted by length: %s" % best_and_spread(ms))
            by_length.close()
            threshold = int(np.sort(info["crossings"])[-300])
            ms, removed = [], 0
            for k in range(REPEATS + 1):
                fresh = copy_of(ctx, vm)
                ctx.synchronize()
                one, (removed, _) = timed(lambda: fresh.carve(scan, R, t, min_crossings=threshold, min_hits=NEVER))
                fresh.close()
                if k > 0:
                    ms.append(one)
            say("carve removing %4d voxels (crossings >= %5d) : %s" % (removed, threshold, best_and_spread(ms)))
            ms = repeat(lambda: vm.match(scan, R, t)[0].close())
            say("VoxelMap.match of the same frame              : %s" % best_and_spread(ms))
            ms = repeat(lambda: vm.prune(center=everything[0], half_extent=everything[1]))
            say("prune, nothing to remove                      : %s" % best_and_spread(ms))
            work = copy_of(ctx, vm)
            ms = repeat(lambda: work.insert_scan(scan, R, t))
            say("insert_scan of the same frame                 : %s" % best_and_spread(ms))
            work.close()
            scan.close()
        vm.close()
    ctx.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
