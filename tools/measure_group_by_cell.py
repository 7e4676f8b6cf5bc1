"""Host time per call of the paths that group by cell through csrc/group_host.hpp and that tools/measure_voxel_map.py does
not time: the map build, the scan sort, the store's prune.

usage: python tools/measure_group_by_cell.py        (NOS_HIP_LIB selects another build of the library; output kept in
                                                     profiles/group_by_cell.txt)

Host clock around calls that end in a stream synchronisation; every call warmed up once, best of 5 and the spread."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

REPEATS = 5


def row(label, fn, setup=lambda: None):
    """fn(setup()) timed REPEATS times after one warm-up; what fn returns is closed."""
    ms = []
    for i in range(REPEATS + 1):
        arg = setup()
        t0 = time.perf_counter()
        out = fn(arg)
        dt = (time.perf_counter() - t0) * 1e3
        if i > 0:
            ms.append(dt)
        for o in (out, arg):
            if hasattr(o, "close"):
                o.close()
    print("%-34s best %8.3f ms  spread %7.3f ms  (%s)" % (label, min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms)))


def main():
    rng = np.random.default_rng(20261018)
    ctx = Context((0,))
    small = rng.uniform([0, 0, 0], [10, 10, 4], size=(1_000, 3))
    large = rng.uniform([0, 0, 0], [100, 100, 10], size=(1_000_000, 3))
    scan_points = rng.uniform([-20, -20, 0], [20, 20, 8], size=(100_000, 3))
    print("best of %d, spread = max - min; host clock, every call ends in a synchronisation" % REPEATS)
    row("build_1k (stats included)", lambda _: api.NdtMap.build(ctx, small, 1.0, 1.0)[0])
    row("build_1M (stats included)", lambda _: api.NdtMap.build(ctx, large, 1.0, 1.0)[0])
    row("scan_sort_100k", lambda _: api.Scan(ctx, scan_points, sort_cell=1.0))

    def store():
        vm = api.VoxelMap(ctx, 1.0, 1.0)
        vm.insert(large)
        return vm

    def prune(vm, half_x):
        vm.prune(center=[half_x, 50.0, 5.0], half_extent=[half_x, 50.0, 5.0])

    row("prune_nothing (100 k voxels)", lambda vm: prune(vm, 50.0), store)
    row("prune_half (100 k voxels)", lambda vm: prune(vm, 25.0), store)
    ctx.close()


if __name__ == "__main__":
    main()
