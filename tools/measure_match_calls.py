"""Host time per call of the four match entry points — NdtMap.match, NdtMap.match_indexed, VoxelMap.match,
VoxelMap.match_indexed — at scans small enough (500 and 5000 points) that the call is host work and launch latency, not
kernel time.

usage: python tools/measure_match_calls.py [label]        (results kept in profiles/matcher_unification.txt)

Host clock around the call alone (it ends in a stream synchronisation; the dataset is closed outside the clock); per entry
point and size BLOCKS blocks of CALLS calls, alternated between the entry points; printed: the median of each block, and
over the blocks the best median and the spread (max - min) of the medians.  fp64, 2 neighbours, sort_by_voxel off.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

BLOCKS, CALLS = 5, 200


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else ""
    rng = np.random.default_rng(20261017)
    ctx = Context((0,))
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    vm.insert(rng.uniform([0, 0, 0], [40, 40, 8], size=(400_000, 3)))
    snap = vm.snapshot()
    R, t = np.eye(3), np.array([0.05, -0.03, 0.02])
    print("%s: store of %d voxels; us per call, median of %d calls, %d blocks" % (label, len(vm), CALLS, BLOCKS))
    for n in (500, 5000):
        scan = api.Scan(ctx, rng.uniform([0, 0, 0], [40, 40, 8], size=(n, 3)), sort_cell=1.0)
        routes = (("NdtMap.match", lambda: snap.match(scan, R, t, 2, "f64")),
                  ("NdtMap.match_indexed", lambda: snap.match_indexed(scan, R, t, 2, "f64", sort_by_voxel=False)),
                  ("VoxelMap.match", lambda: vm.match(scan, R, t, 2, "f64")),
                  ("VoxelMap.match_indexed", lambda: vm.match_indexed(scan, R, t, 2, "f64", sort_by_voxel=False)))
        medians = [[] for _ in routes]
        for block in range(BLOCKS + 1):  # block 0 warms up
            for k, (_, call) in enumerate(routes):
                us = []
                for _ in range(CALLS):
                    t0 = time.perf_counter()
                    ds, _n = call()
                    us.append((time.perf_counter() - t0) * 1e6)
                    ds.close()
                if block > 0:
                    medians[k].append(statistics.median(us))
        for (name, _), m in zip(routes, medians):
            print("  %5d points  %-24s best %8.1f  spread %6.1f   blocks: %s" % (
                n, name, min(m), max(m) - min(m), " ".join("%.1f" % x for x in m)))
        scan.close()
    snap.close()
    vm.close()
    ctx.close()


if __name__ == "__main__":
    main()
