"""Host time per call of the five batched entry points — solve6_batch, register6_batch against an NdtMap and against a
VoxelMap, score_batch against either — at B = 1 and B = 16 with 500-point scans and 500-correspondence datasets on a small
map, where the call is host work (staging, launch latency, the copy back), not kernel time.

usage: python tools/measure_batch_calls.py [label]        (results kept in profiles/batch_host_unification.txt)

Host clock around the call alone (it ends in a stream synchronisation); per entry point and B BLOCKS blocks of CALLS
calls, alternated between the entry points; printed: the median of each block, and over the blocks the best median and
the spread (max - min) of the medians.  fp64, exponential loss, 2 neighbours; registrations of 2 rounds of at most 10
iterations, solves of at most 10 iterations.
"""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api, synth  # noqa: E402

BLOCKS, CALLS = 5, 200
LOSS = ("exponential", 1.0, 1.0)


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else ""
    rng = np.random.default_rng(20261019)
    lo, hi = [0, 0, 0], [10, 10, 3]
    ctx = Context((0,))
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    vm.insert(rng.uniform(lo, hi, size=(30_000, 3)))
    snap = vm.snapshot()
    scans = [api.Scan(ctx, rng.uniform(lo, hi, size=(500, 3))) for _ in range(16)]
    datasets = [api.NdtDataset.from_planes(ctx, synth.ndt_planes(500, 20, seed=s), "f64") for s in range(16)]
    R = np.tile(np.eye(3).reshape(9), (16, 1))
    t = np.tile([0.05, -0.03, 0.02], (16, 1))
    print("%s: store of %d voxels; us per call, median of %d calls, %d blocks" % (label, len(vm), CALLS, BLOCKS))
    for B in (1, 16):
        def register(m):
            return lambda: api.register6_batch(m, scans[:B], R[:B], t[:B], LOSS, max_outer_iterations=2, max_iterations=10)
        routes = (("solve6_batch", lambda: api.solve6_batch(datasets[:B], R[:B], t[:B], LOSS, max_iterations=10)),
                  ("register6_batch NdtMap", register(snap)),
                  ("register6_batch VoxelMap", register(vm)),
                  ("score_batch NdtMap", lambda: api.score_batch(snap, scans[:B], R[:B], t[:B], LOSS)),
                  ("score_batch VoxelMap", lambda: api.score_batch(vm, scans[:B], R[:B], t[:B], LOSS)))
        medians = [[] for _ in routes]
        for block in range(BLOCKS + 1):  # block 0 warms up
            for k, (_, call) in enumerate(routes):
                us = []
                for _ in range(CALLS):
                    t0 = time.perf_counter()
                    call()
                    us.append((time.perf_counter() - t0) * 1e6)
                if block > 0:
                    medians[k].append(statistics.median(us))
        for (name, _), m in zip(routes, medians):
            print("  B = %2d  %-26s best %8.1f  spread %6.1f   blocks: %s" % (
                B, name, min(m), max(m) - min(m), " ".join("%.1f" % x for x in m)))
    for h in scans + datasets + [snap, vm]:
        h.close()
    ctx.close()


if __name__ == "__main__":
    main()
