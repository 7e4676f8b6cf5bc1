"""Cost of scoring B candidate poses of one scan against the live voxel store: api.score_batch (ONE call,
nos_voxel_map_score_batch) against the route that existed before it, a loop of VoxelMap.match + accumulate6 per pose —
and, for scale, one api.register6_batch of the same B.

usage: python tools/measure_score_batch.py [--out FILE]      (output kept as profiles/score_batch.txt)

Host clock around calls that end in a stream synchronisation; every shape is warmed up first, then best of 5 and the
spread (max - min), the two routes alternated in one process.  One scan of 500 points and one of 5 000 points against a
store of ~100 k voxels, B = 1, 16, 256 and 4 096 poses scattered around the scan's true pose.  Before anything is timed the
two routes are compared: matches equal, costs within the reordering bound 2 n · 2^-52 · cost.  register6_batch is timed
once per shape (a registration is ten rounds of matching and LM per pose: it is there to show what a score call is cheap
against, not to be compared run by run); a shape it cannot run is reported as such."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, _lib, api  # noqa: E402

REPEATS = 5
LOSS = ("exponential", 1.0, 1.0)
BATCHES = (1, 16, 256, 4096)
SCAN_POINTS = (500, 5000)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %10.3f ms  spread %9.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def surface(rng, n, lo, hi):
    """points of a wavy sheet with 2 cm of noise: a map a scan can be registered to"""
    xy = rng.uniform(lo, hi, size=(n, 2))
    z = 0.45 * np.sin(0.9 * xy[:, 0]) + 0.35 * np.cos(0.7 * xy[:, 1]) + rng.normal(scale=0.02, size=n)
    return np.column_stack([xy, z])


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def loop_route(vm, scan, R, t):
    """the existing route: per pose a match (records written, one wait) and an accumulate (28 sums, one wait)"""
    out = np.zeros(len(R), dtype=[("matches", np.uint64), ("cost", np.float64)])
    for i in range(len(R)):
        ds, n = vm.match(scan, R[i], t[i], 2, "f64")
        out[i] = (n, ds.accumulate6(R[i], t[i], LOSS)[27])
        ds.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_batch.txt"))
    args = ap.parse_args()
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    rng = np.random.default_rng(20261018)
    ctx = Context((0,))
    half = 160.0
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    for _ in range(4):
        vm.insert(surface(rng, 1_000_000, -half, half))
    say("score_batch against the loop of match + accumulate6; store of %d voxels (%d valid); loss %r" % (len(vm), vm.n_valid, LOSS))
    say("best of %d after a warm-up of every shape, spread = max - min; host clock, every call ends in a synchronisation;" % REPEATS)
    say("the two routes alternated; register6_batch timed once per shape")
    ratios = {}
    for n_points in SCAN_POINTS:
        center = np.array([31.0, -17.0, 0.0])
        world = surface(rng, n_points, -8.0, 8.0) + center
        world[:, 2] = 0.45 * np.sin(0.9 * world[:, 0]) + 0.35 * np.cos(0.7 * world[:, 1]) + rng.normal(scale=0.02, size=n_points)
        R_true, t_true = rot_z(0.02), center + np.array([0.05, -0.04, 0.02])
        scan = api.Scan(ctx, (R_true.T @ (world - t_true).T).T)
        say("\n== one scan of %d points ==" % n_points)
        for B in BATCHES:
            R = np.array([(rot_z(0.02 + a)).reshape(9) for a in rng.normal(0.0, 0.05, size=B)])
            t = t_true + rng.normal(0.0, 0.5, size=(B, 3)) * np.array([1.0, 1.0, 0.1])
            a, b = loop_route(vm, scan, R, t), api.score_batch(vm, [scan] * B, R, t, LOSS)  # warm-up, and the same answer
            assert np.array_equal(a["matches"], b["matches"]), "the two routes count different matches"
            assert np.all(np.abs(a["cost"] - b["cost"]) <= 2 * n_points * 2.0 ** -52 * a["cost"]), "costs beyond the reordering bound"
            ta, tb = [], []
            for _ in range(REPEATS):  # alternated
                ta.append(timed(lambda: loop_route(vm, scan, R, t))[0])
                tb.append(timed(lambda: api.score_batch(vm, [scan] * B, R, t, LOSS))[0])
            ratio = min(ta) / min(tb)
            ratios[(n_points, B)] = ratio
            say("B = %4d  (a) loop of match + accumulate6 : %s" % (B, best_and_spread(ta)))
            say("B = %4d  (b) score_batch                 : %s   (a) / (b) = %.2f%s; mean matches %.0f" % (
                B, best_and_spread(tb), ratio, "" if ratio >= 1.0 else "  (the batched call LOSES here)", float(b["matches"].mean())))
            try:
                if B == BATCHES[0]:
                    api.register6_batch(vm, [scan], R[:1], t[:1], LOSS, keep_multiple=4)  # loads the kernel
                ms, (_, _, reps) = timed(lambda: api.register6_batch(vm, [scan] * B, R, t, LOSS, keep_multiple=4))
                say("B = %4d  (c) register6_batch, one call    :      %10.3f ms   %d of %d ok" % (B, ms, sum(r["ok"] for r in reps), B))
            except _lib.NosError as err:
                say("B = %4d  (c) register6_batch              : not measured (%s)" % (B, err))
        scan.close()
    vm.close()
    ctx.close()
    say("\n(a) / (b) by shape: " + ", ".join("%d x %d: %.2f" % (n, B, r) for (n, B), r in sorted(ratios.items())))
    below = ["%d x %d" % k for k, r in sorted(ratios.items()) if r < 1.0]
    say("score_batch is slower than the loop at: %s" % (", ".join(below) if below else "no measured shape"))
    need = ratios[(500, 256)]
    say("requirement (B = 256 x 500 points: the batched call faster than the loop): %s (%.2f x)" % ("met" if need > 1.0 else "NOT MET", need))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if need > 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
