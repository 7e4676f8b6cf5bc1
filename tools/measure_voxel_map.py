"""Per-frame cost of the incremental voxel map (api.VoxelMap) against the only alternative without it: rebuilding the
whole map from every point seen so far (nos_ndt_map_build, whose code this feature leaves as it was).

usage: python tools/measure_voxel_map.py [--single-insert]      (output kept as profiles/voxel_map_ab.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), the two sides
alternated in one session.  --single-insert: one warmed-up insert_scan and nothing else after the set-up, for a
kernel-trace run of its own (rocprofv3 --kernel-trace --stats -- python tools/measure_voxel_map.py --single-insert)."""
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


def fill(ctx, box, n_points, rng):
    """A store that absorbed n_points uniform points of `box`, 1 M per insert; the points are returned too."""
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    chunks = []
    for _ in range(n_points // 1_000_000):
        p = rng.uniform([0, 0, 0], box, size=(1_000_000, 3))
        vm.insert(p)
        chunks.append(p)
    return vm, np.concatenate(chunks)


def frame_times(ctx, vm, frame_local, R, t):
    """→ (insert_scan times, insert times, snapshot times); every call warmed up once."""
    warped = (R @ frame_local.T).T + t
    scan = api.Scan(ctx, frame_local)
    vm.insert_scan(scan, R, t)
    vm.insert(warped)
    vm.snapshot().close()
    a, b, c = [], [], []
    for _ in range(REPEATS):
        a.append(timed(lambda: vm.insert_scan(scan, R, t))[0])
        b.append(timed(lambda: vm.insert(warped))[0])
        ms, snap = timed(vm.snapshot)
        c.append(ms)
        snap.close()
    scan.close()
    return a, b, c


def main():
    single = "--single-insert" in sys.argv
    rng = np.random.default_rng(20261016)
    ctx = Context((0,))
    R = np.array([[np.cos(0.3), -np.sin(0.3), 0.0], [np.sin(0.3), np.cos(0.3), 0.0], [0.0, 0.0, 1.0]])
    frame_local = rng.uniform([-20, -20, 0], [20, 20, 8], size=(FRAME, 3))  # a scan: 100 k points around the sensor
    if single:
        vm, _ = fill(ctx, [100.0, 100.0, 10.0], 1_000_000, rng)
        scan = api.Scan(ctx, frame_local)
        t = np.array([50.0, 50.0, 1.0])
        vm.insert_scan(scan, R, t)
        ctx.synchronize()
        print("single insert_scan of %d points: %.3f ms, %d voxels in the store" % (
            FRAME, timed(lambda: vm.insert_scan(scan, R, t))[0], len(vm)))
        return
    print("frame = %d points; best of %d, spread = max - min; host clock, every call ends in a synchronisation" % (FRAME, REPEATS))
    for label, box in (("100 k voxels", [100.0, 100.0, 10.0]), ("796 k voxels", [199.0, 200.0, 20.0])):
        t = np.array([box[0] / 2, box[1] / 2, 1.0])
        vm, absorbed = fill(ctx, box, 10_000_000, rng)
        print("\n== store of %d voxels (%s) after %d points ==" % (len(vm), label, vm.n_points))
        everything = np.concatenate([absorbed, (R @ frame_local.T).T + t])
        api.NdtMap.build(ctx, everything, 1.0, 1.0, return_stats=False)[0].close()
        rebuild, scan_ms, ins_ms, snap_ms = [], [], [], []
        for _ in range(REPEATS):  # alternated: rebuild, then the incremental frame
            ms, (gm, _) = timed(lambda: api.NdtMap.build(ctx, everything, 1.0, 1.0, return_stats=False))
            gm.close()
            rebuild.append(ms)
            a, b, c = frame_times(ctx, vm, frame_local, R, t)
            scan_ms.append(min(a)), ins_ms.append(min(b)), snap_ms.append(min(c))
        print("rebuild from all %d points (nos_ndt_map_build, map included): %s" % (everything.shape[0], best_and_spread(rebuild)))
        print("insert_scan (device-resident scan, pose only)              : %s" % best_and_spread(scan_ms))
        print("insert (host points, 2.4 MB upload)                         : %s" % best_and_spread(ins_ms))
        print("snapshot (matcher tables over all voxels)                   : %s" % best_and_spread(snap_ms))
        print("ratio rebuild / (insert_scan + snapshot) = %.1f" % (min(rebuild) / (min(scan_ms) + min(snap_ms))))
        vm.close()
        del absorbed, everything
    # independence from history: same voxel count, 1 M against 10 M absorbed points
    print("\n== the same frame into stores with the same voxel count after 1 M and after 10 M absorbed points ==")
    box = [100.0, 100.0, 10.0]
    t = np.array([50.0, 50.0, 1.0])
    res = {}
    stores = {n: fill(ctx, box, n, rng)[0] for n in (1_000_000, 10_000_000)}
    for _ in range(2):  # alternated
        for n, vm in stores.items():
            a, b, _ = frame_times(ctx, vm, frame_local, R, t)
            res.setdefault(n, ([], []))
            res[n][0].extend(a), res[n][1].extend(b)
    for n, vm in stores.items():
        print("%8d points absorbed, %d voxels: insert_scan %s" % (n, len(vm), best_and_spread(res[n][0][:REPEATS])))
        print("%8s                              insert      %s" % ("", best_and_spread(res[n][1][:REPEATS])))
    a1, a10 = res[1_000_000][0], res[10_000_000][0]
    diff = abs(min(a1) - min(a10))
    spread = max(max(a1) - min(a1), max(a10) - min(a10))
    print("insert_scan: |best(1 M) - best(10 M)| = %.3f ms, larger run-to-run spread of the two = %.3f ms → %s" % (
        diff, spread, "independent of history" if diff <= spread else "DEPENDS ON HISTORY"))
    ctx.close()


if __name__ == "__main__":
    main()
