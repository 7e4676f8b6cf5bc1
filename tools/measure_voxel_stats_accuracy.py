"""Accuracy of the per-voxel NDT statistics against the 50-digit reference, per cell offset and per path, and the cost
of the two calls that compute them.  Works with any build of the library (NOS_HIP_LIB selects one, e.g. the parent
commit's), so that two builds can be measured the same way and alternated.

usage: python tools/measure_voxel_stats_accuracy.py accuracy [--label NAME]
       python tools/measure_voxel_stats_accuracy.py time [--label NAME] [--repeats 20]
       (outputs kept together as profiles/voxel_stats_accuracy.txt)

accuracy: the cloud of tests/voxel_inputs.py on the 1 m grid (every family at every offset) through every path of
tests/voxel_inputs.PATHS with NOS_MAP_PROPER_SQRT_INFORMATION; per offset and path the largest error of the information
matrix (relative Frobenius, less the gap the tie rule may add), of the mean (ulps) and of the floored eigenvalues, and
the number of voxels whose validity differs from the reference's; then the largest errors per family over the paths.
Nothing is asserted here: tests/test_voxel_stats_xprec.py does that.

time: ONE block — after a warm-up, `repeats` map builds and `repeats` single inserts into a fresh store of the 200 300-point
cloud of test_compact_sort_keys_give_the_same_map_…, host clock around calls that end in a stream synchronisation;
median, minimum and maximum of the block in ms.  Run several blocks per build, alternating the builds."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402
from tests import voxel_inputs as VI  # noqa: E402


def accuracy(ctx, label):
    c = VI.cloud(*VI.CLOUDS["res1"])
    ref = VI.reference(c)
    print("# accuracy [%s]: %d voxels, %d points, 1 m grid, proper sqrt-information" % (label, len(c.voxels), len(c.points)))
    print("# per offset and path: information error (max over voxels valid on both sides) | mean, ulp | eigenvalues | validity flips")
    by_family = {}
    for path in VI.PATHS:
        rows = VI.errors(c, ref, VI.run_path(api, ctx, c, path, True), True)
        for oi, (off, _) in enumerate(VI.OFFSETS):
            mine = [e for e in rows if e["offset"] == oi]
            ok = [e for e in mine if "info" in e]
            flips = sum(1 for e in mine if not (e["found"] and e["valid_equal"] and e["count_equal"]))
            print("%-22s offset %-28s info %.2e  mean %5.2f  eig %.2e  flips %d" %
                  (path, str(off), max(e["info"] - e["gap"] for e in ok), max(e["mean"] for e in ok),
                   max(e["eig"] for e in ok), flips))
        for e in rows:
            if "info" in e:
                w = by_family.setdefault(e["name"], [0.0, 0.0, 0.0])
                w[0], w[1], w[2] = max(w[0], e["info"] - e["gap"]), max(w[1], e["mean"]), max(w[2], e["eig"])
    print("# per family, max over paths and offsets: information error | mean, ulp | eigenvalues")
    for name, w in by_family.items():
        print("%-26s info %.2e  mean %5.2f  eig %.2e" % (name, w[0], w[1], w[2]))


def timing(ctx, label, repeats):
    rng = np.random.default_rng(20261005)
    pts = np.concatenate([rng.uniform([-37, -12, -4], [41, 29, 6], size=(200_000, 3)),
                          rng.uniform(0, 1, size=(300, 3)) + np.array([-900.0, 1500.0, 77.0])])
    rng.shuffle(pts)

    def build():
        t0 = time.perf_counter()
        m, _ = api.NdtMap.build(ctx, pts, 1.0, 1.0, return_stats=False)
        dt = time.perf_counter() - t0
        m.close()
        return dt * 1e3

    def insert():
        vm = api.VoxelMap(ctx, 1.0, 1.0, capacity=1 << 16)
        t0 = time.perf_counter()
        vm.insert(pts)
        dt = time.perf_counter() - t0
        vm.close()
        return dt * 1e3

    for fn in (build, insert):
        for _ in range(5):
            fn()
    for name, fn in (("map build", build), ("store insert", insert)):
        ms = np.array([fn() for _ in range(repeats)])
        print("time [%s] %-12s %d points: median %.3f ms  min %.3f  max %.3f  (%d repeats)" %
              (label, name, len(pts), np.median(ms), ms.min(), ms.max(), repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("accuracy", "time"))
    ap.add_argument("--label", default=os.environ.get("NOS_HIP_LIB") or "in-tree build")
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    ctx = Context((0,))
    if args.what == "accuracy":
        accuracy(ctx, args.label)
    else:
        timing(ctx, args.label, args.repeats)
    ctx.close()


if __name__ == "__main__":
    main()
