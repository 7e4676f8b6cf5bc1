"""Cost of the voxel map's sliding window (VoxelMap.prune) next to the calls a frame already makes (insert_scan, snapshot),
at the two stores tools/measure_voxel_map.py uses, and frame time over the 80-frame trajectory of
tests/test_voxel_map_window.py with and without the window.

usage: python tools/measure_voxel_map_window.py [--single-prune]      (output kept as profiles/voxel_map_window.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min).  A prune that removes
something changes the store, so each of its repeats runs on a store filled afresh from the same points (and one more,
before the timed ones, warms the call up).  --single-prune: one warmed-up removing prune and nothing else after the set-up,
for a kernel-trace run of its own (rocprofv3 --kernel-trace --stats -- python tools/measure_voxel_map_window.py --single-prune)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

FRAME = 100_000
REPEATS = 5


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %8.3f ms  spread %7.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def fill(ctx, chunks):
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for p in chunks:
        vm.insert(p)
    return vm


def x_box(box, fraction_kept):
    """The box that keeps the cells with x below fraction_kept of the store's extent (all of y and z)."""
    half = np.array([box[0] * fraction_kept / 2, box[1], box[2]])
    return np.array([half[0], box[1] / 2, box[2] / 2]), half


def removing_prune(ctx, chunks, center, half):
    """→ (times, voxels before, removed, capacity before, capacity after, the last pruned store)."""
    ms, vm = [], None
    for k in range(REPEATS + 1):  # the first one warms up
        if vm is not None:
            vm.close()
        vm = fill(ctx, chunks)
        before, cap = len(vm), vm.memory()["capacity"]
        t, removed = timed(lambda: vm.prune(center=center, half_extent=half))
        if k > 0:
            ms.append(t)
    return ms, before, removed, cap, vm.memory()["capacity"], vm


def snapshot_times(vm):
    vm.snapshot().close()
    out = []
    for _ in range(REPEATS):
        ms, snap = timed(vm.snapshot)
        out.append(ms)
        snap.close()
    return out


def trajectory(ctx, windowed, rng_seed=137):
    """The run of test_a_windowed_store_stays_bounded_over_eighty_frames…: per frame (insert, prune, snapshot) times and
    the voxel count the snapshot saw."""
    rng = np.random.default_rng(rng_seed)
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    step, half = np.array([1.2, 0.9, 0.0]), (20.0, 20.0, 4.0)
    rows = []
    for f in range(80):
        center = -39.5 * step + f * step
        c = np.round(center * 1024) / 1024
        pts = c + rng.integers([-15 * 1024, -15 * 1024, -2 * 1024], [15 * 1024, 15 * 1024, 2 * 1024], size=(30_000, 3)) / 1024.0
        t_ins = timed(lambda: vm.insert(pts))[0]
        t_prune = timed(lambda: vm.prune(center=center, half_extent=half))[0] if windowed else 0.0
        t_snap, snap = timed(vm.snapshot)
        snap.close()
        rows.append((t_ins, t_prune, t_snap, len(vm)))
    vm.close()
    return rows


def main():
    single = "--single-prune" in sys.argv
    rng = np.random.default_rng(20261017)
    ctx = Context((0,))
    if single:
        box = [199.0, 200.0, 20.0]
        chunks = [rng.uniform([0, 0, 0], box, size=(1_000_000, 3)) for _ in range(4)]
        center, half = x_box(box, 0.95)
        warm = fill(ctx, chunks)
        warm.prune(center=center, half_extent=half)
        warm.close()
        vm = fill(ctx, chunks)
        ctx.synchronize()
        before = len(vm)
        ms, removed = timed(lambda: vm.prune(center=center, half_extent=half))
        print("single prune of a store of %d voxels: %.3f ms, %d removed, %d kept" % (before, ms, removed, len(vm)))
        return
    R = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
    frame_local = rng.uniform([-20, -20, 0], [20, 20, 8], size=(FRAME, 3))  # a scan: 100 k points around the sensor
    print("frame = %d points; best of %d, spread = max - min; host clock, every call ends in a synchronisation" % (FRAME, REPEATS))
    for label, box in (("100 k voxels", [100.0, 100.0, 10.0]), ("796 k voxels", [199.0, 200.0, 20.0])):
        chunks = [rng.uniform([0, 0, 0], box, size=(1_000_000, 3)) for _ in range(10)]
        vm = fill(ctx, chunks)
        mem = vm.memory()
        print("\n== store of %d voxels (%s) after %d points; capacity %d, %.1f MB on the device ==" % (
            len(vm), label, vm.n_points, mem["capacity"], mem["bytes"] / 1e6))
        # what a frame already costs, in this run
        t = np.array([box[0] / 2, box[1] / 2, 1.0])
        scan = api.Scan(ctx, frame_local)
        vm.insert_scan(scan, R, t)
        scan_ms = [timed(lambda: vm.insert_scan(scan, R, t))[0] for _ in range(REPEATS)]
        scan.close()
        snap_before = snapshot_times(vm)
        print("insert_scan (device-resident scan, pose only)        : %s" % best_and_spread(scan_ms))
        print("snapshot (matcher tables over all %7d voxels)     : %s" % (len(vm), best_and_spread(snap_before)))
        # a prune that removes nothing
        everything = (np.array(box) / 2, np.array(box))
        assert vm.prune(center=everything[0], half_extent=everything[1]) == 0
        none_ms = []
        for _ in range(REPEATS):
            ms, removed = timed(lambda: vm.prune(center=everything[0], half_extent=everything[1]))
            assert removed == 0
            none_ms.append(ms)
        print("prune, nothing to remove (keep + scan + one wait)    : %s" % best_and_spread(none_ms))
        vm.close()
        for share, kept in (("5 %", 0.95), ("90 %", 0.10)):
            center, half = x_box(box, kept)
            ms, before, removed, cap0, cap1, pruned = removing_prune(ctx, chunks, center, half)
            print("prune, about %-4s removed (%7d of %7d voxels, capacity %7d -> %7d): %s" % (
                share, removed, before, cap0, cap1, best_and_spread(ms)))
            if kept == 0.10:
                print("snapshot after it (matcher tables over %7d voxels) : %s" % (len(pruned), best_and_spread(snapshot_times(pruned))))
            pruned.close()
        del chunks
    # frame time over a trajectory: does it follow the window's voxel count or the trajectory's length?
    print("\n== 80 frames of 30 000 points, the sensor advancing 1.5 m per frame; window = sensor +- (20, 20, 4) m ==")
    print("per frame: insert + prune + snapshot, host clock; best of 3 passes per frame")
    runs = {w: [trajectory(ctx, w) for _ in range(3)] for w in (True, False)}
    best = {w: np.min(np.array([[r[0] + r[1] + r[2] for r in run] for run in runs[w]]), axis=0) for w in runs}
    parts = {w: np.min(np.array([[r[:3] for r in run] for run in runs[w]]), axis=0) for w in runs}
    print("frame | windowed: voxels  insert  prune  snapshot  total | unpruned: voxels  insert  snapshot  total   (ms)")
    for f in (0, 9, 19, 29, 39, 49, 59, 69, 79):
        a, b = runs[True][0][f], runs[False][0][f]
        print("%5d | %16d  %6.3f %6.3f  %8.3f %6.3f | %16d  %6.3f  %8.3f %6.3f" % (
            f + 1, a[3], parts[True][f][0], parts[True][f][1], parts[True][f][2], best[True][f],
            b[3], parts[False][f][0], parts[False][f][2], best[False][f]))
    for w, name in ((True, "windowed"), (False, "unpruned")):
        print("%s: mean frame time, frames 11-20: %.3f ms; frames 71-80: %.3f ms (ratio %.2f)" % (
            name, best[w][10:20].mean(), best[w][70:80].mean(), best[w][70:80].mean() / best[w][10:20].mean()))
    ctx.close()


if __name__ == "__main__":
    main()
