"""Cost of one scan-to-map round — a match and 40 LM iterations — through the voxel-indexed match against the live voxel
store (VoxelMap.match_indexed, nos_voxel_map_match_indexed) against the two routes its parent has.

usage: python tools/measure_voxel_map_match_indexed.py [--no-10m]   (output kept as profiles/voxel_map_match_indexed.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min); the routes alternated
in one session, their results checked equal first.  Stores: the 100 k- and 796 k-voxel stores of DESIGN.md §13's table.
Scans: 100 k, 1 M and 10 M points, cell-sorted, fp64, max_neighbors = 2, sort_by_voxel off (what pipeline.scan_to_map
asks for).  Per round:
  (a) NdtMap.match_indexed on a snapshot() taken ONCE outside the clock, + solve6  — the snapshot's own cost is printed apart
  (b) VoxelMap.match_indexed                                                + solve6
  (c) VoxelMap.match (flat, 120 B per correspondence)                       + solve6
and time_kernel6 on the dataset of (a) against that of (b): the same points in the same order, a whole-map table against a
compact one.  (a) and (c) exist without this feature and are the baselines."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

REPEATS = 5
LM_ITERATIONS = 40
LOSS = ("exponential", 1.0, 1.0)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms" % (min(ms), max(ms) - min(ms))


def fill(ctx, box, n_points, rng):
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for _ in range(n_points // 1_000_000):
        vm.insert(rng.uniform([0, 0, 0], box, size=(1_000_000, 3)))
    return vm


def one_round(match, R, t):
    """match + 40 LM iterations (tolerances 0: the loop runs its iterations) → (pose R, t, iterations, matches, table rows)"""
    ds, n = match()
    try:
        Rs, ts, rep = ds.solve6(R, t, LOSS, max_iterations=LM_ITERATIONS, gradient_tolerance=0.0, parameter_tolerance=0.0)
        rows = ds.n_voxels if isinstance(ds, api.NdtIndexedDataset) else 0
    finally:
        ds.close()
    return Rs, ts, rep["iterations"], n, rows


def measure(vm, snap, scan, R, t, label):
    routes = (("(a) snapshot, NdtMap.match_indexed ", lambda: snap.match_indexed(scan, R, t, 2, "f64", sort_by_voxel=False)),
              ("(b) VoxelMap.match_indexed         ", lambda: vm.match_indexed(scan, R, t, 2, "f64", sort_by_voxel=False)),
              ("(c) VoxelMap.match, flat           ", lambda: vm.match(scan, R, t, 2, "f64")))
    first = [one_round(m, R, t) for _, m in routes]  # warm-up, and the same answer
    (Ra, ta, ia, na, va), (Rb, tb, ib, nb, vb), (Rc, tc, ic, nc, _) = first
    assert na == nb == nc and ia == ib, (na, nb, nc, ia, ib)
    assert Ra.tobytes() == Rb.tobytes() and ta.tobytes() == tb.tobytes(), "(a) and (b) must agree bit for bit"
    flat_diff = max(float(np.abs(Ra - Rc).max()), float(np.abs(ta - tc).max()))  # another summation order: to rounding
    ms = [[] for _ in routes]
    match_ms = [[] for _ in routes]
    for _ in range(REPEATS):  # alternated
        for k, (_, m) in enumerate(routes):
            ms[k].append(timed(lambda: one_round(m, R, t))[0])
            dt, (ds, _) = timed(m)
            ds.close()
            match_ms[k].append(dt)
    print("%s: %d matches, %d LM iterations, (a) = (b) bit for bit, |pose (c) - pose (a)| <= %.1e; table rows (a) %d, (b) %d" % (
        label, nb, ib, flat_diff, va, vb))
    for k, (name, _) in enumerate(routes):
        print("  %s round %s | match alone %s" % (name, best_and_spread(ms[k]), best_and_spread(match_ms[k])))
    best = [min(x) for x in ms]
    print("  round: (b) - (a) = %+.3f ms, (b) - (c) = %+.3f ms; fastest: %s" % (
        best[1] - best[0], best[1] - best[2], "abc"[int(np.argmin(best))]))
    # the assemble kernel alone on the two indexed datasets: whole-map table against compact table
    da, _ = routes[0][1]()
    db, _ = routes[1][1]()
    ka, kb = [], []
    for _ in range(REPEATS):  # alternated
        ka.append(da.time_kernel6(R, t, LOSS, repeats=20)[0])
        kb.append(db.time_kernel6(R, t, LOSS, repeats=20)[0])
    print("  time_kernel6: whole-map table (%d rows) %s | compact table (%d rows) %s | compact - whole = %+.4f ms" % (
        da.n_voxels, best_and_spread(ka), db.n_voxels, best_and_spread(kb), min(kb) - min(ka)))
    da.close(), db.close()


def main():
    sizes = [100_000, 1_000_000] + ([] if "--no-10m" in sys.argv else [10_000_000])
    rng = np.random.default_rng(20261017)
    ctx = Context((0,))
    print("best of %d, spread = max - min; host clock, every timed call ends in a synchronisation; fp64, 2 neighbours, "
          "cell-sorted scans, sort_by_voxel off" % REPEATS)
    for label, box in (("100 k", [100.0, 100.0, 10.0]), ("796 k", [199.0, 200.0, 20.0])):
        vm = fill(ctx, box, 10_000_000, rng)
        t = np.array([box[0] / 2, box[1] / 2, 1.0])
        snaps = []
        for _ in range(REPEATS):
            dt, snap = timed(vm.snapshot)
            snaps.append(dt)
            snap.close()
        snap = vm.snapshot()
        print("\n== store of %d voxels (%s) after %d points; snapshot() alone: %s ==" % (len(vm), label, vm.n_points, best_and_spread(snaps)))
        for n in sizes:
            # 100 k: a frame around the sensor; larger scans cover the map
            half = [20.0, 20.0] if n == 100_000 else [box[0] / 2, box[1] / 2]
            local = rng.uniform([-half[0], -half[1], 0], [half[0], half[1], 8], size=(n, 3))
            scan = api.Scan(ctx, local, sort_cell=1.0)
            del local
            c, s = np.cos(0.002), np.sin(0.002)  # a start slightly off the truth (identity rotation, translation t)
            R0 = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
            measure(vm, snap, scan, R0, t + np.array([0.05, -0.03, 0.02]), "%s store, %8d points" % (label, n))
            scan.close()
        snap.close()
        vm.close()
    ctx.close()


if __name__ == "__main__":
    main()
