"""Cost of merging one voxel store into another (VoxelMap.merge) next to what one has to do without it —
insert the submap's POINTS again — and the error maxima of the merge's tests.

usage: python tools/measure_voxel_map_merge.py      (writes profiles/voxel_map_merge.txt and prints it)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), one untimed call
first.  Every timed call fills a store created afresh (with room for the voxels, so that no repeat pays for growth), since
a merge or an insert changes its destination.  Two submaps of about 10 k and 500 k voxels at 40 points per voxel; the pose
is a general one.  insert_scan is timed on a device-resident scan: the upload of the points is not charged to it.
coarsened(2) is timed against an insert of the same points at twice the resolution."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

REPEATS = 5
POINTS_PER_VOXEL = 40
OUT = os.path.join(ROOT, "profiles", "voxel_map_merge.txt")
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def timed_on_fresh_stores(ctx, res, capacity, fill):
    """fill(store) on REPEATS + 1 fresh stores (the first one warms up) → (times in ms, voxels of the last store)"""
    ms, n = [], 0
    for k in range(REPEATS + 1):
        vm = api.VoxelMap(ctx, res, res * res, capacity=capacity)
        ctx.synchronize()
        t0 = time.perf_counter()
        fill(vm)
        t = (time.perf_counter() - t0) * 1e3
        if k > 0:
            ms.append(t)
        n = len(vm)
        vm.close()
    return ms, n


def submap(rng, box):
    """about box[0] · box[1] · box[2] voxels of a 1 m grid, POINTS_PER_VOXEL points each on average"""
    n = int(box[0] * box[1] * box[2]) * POINTS_PER_VOXEL
    return rng.uniform([0.0, 0.0, 0.0], box, size=(n, 3))


def timings(ctx):
    rng = np.random.default_rng(20261019)
    a = 0.3
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    t = np.array([3.3, -1.7, 0.4])
    say("best of %d, spread = max - min; host clock, every call ends in a synchronisation; %d points per voxel" % (
        REPEATS, POINTS_PER_VOXEL))
    for box in ([50.0, 50.0, 4.0], [250.0, 250.0, 8.0]):
        pts = submap(rng, box)
        src = api.VoxelMap(ctx, 1.0, 1.0)
        for k in range(0, len(pts), 4_000_000):
            src.insert(pts[k:k + 4_000_000])
        scan = api.Scan(ctx, pts)
        V = len(src)
        say("\n== submap of %d voxels, %d points ==" % (V, len(pts)))
        ms, n_merge = timed_on_fresh_stores(ctx, 1.0, 2 * V, lambda vm: vm.merge(src, R, t))
        say("merge(submap, R, t) into an empty store            -> %7d voxels: %s" % (n_merge, best_and_spread(ms)))
        ms, n_ins = timed_on_fresh_stores(ctx, 1.0, 2 * V, lambda vm: vm.insert_scan(scan, R, t))
        say("insert_scan(its points, R, t) into an empty store  -> %7d voxels: %s" % (n_ins, best_and_spread(ms)))
        ms, n_coarse = timed_on_fresh_stores(ctx, 2.0, V, lambda vm: vm.merge(src))
        say("coarsened(2): merge into an empty 2 m store        -> %7d voxels: %s" % (n_coarse, best_and_spread(ms)))
        ms, n_ci = timed_on_fresh_stores(ctx, 2.0, V, lambda vm: vm.insert_scan(scan, np.eye(3), np.zeros(3)))
        say("insert_scan(its points) into an empty 2 m store    -> %7d voxels: %s" % (n_ci, best_and_spread(ms)))
        assert n_coarse == n_ci
        scan.close()
        src.close()
        del pts


def error_maxima(ctx):
    """the general-pose cases of tests/test_voxel_map_merge_abi.py (host) and tests/test_voxel_map_merge.py (device)"""
    import mpmath
    from oracle import oracle_voxel_xp as vx
    from nonlinear_optimizer_for_slam_amd import _lib
    from tests import voxel_inputs as vi
    from tests import voxel_merge_inputs as mi
    lib = _lib.hip_lib()
    R, t = mi.general_pose()
    say("\n== error maxima against 50 digits; pose: %.1f rad about (1, 2, 3), t = (%s) ==" % (
        mi.GENERAL_ANGLE, ", ".join("%g" % x for x in t)))
    c = vi.cloud(0.3, range(7), True)
    for res_dst in (0.3, 0.5):
        L = mi.bound_scale(0.3, res_dst)
        worst = [0.0, 0.0]
        for v in c.voxels:
            p = c.points[v["idx"]]
            n, sums = vi.corner_sums(p, v["cell"], 0.3)
            _, cell_out, out = mi.debug_voxel_moments(lib, n, sums, v["cell"], 0.3, R, t, res_dst)
            with mpmath.workdps(vx.DPS):
                m, sc = mi.mean_and_scatter_xp(mi.warp_xp(p, R, t))
                o = [mpmath.mpf(float(np.float64(cell_out[k]) * np.float64(res_dst))) for k in range(3)]
                s = [mpmath.mpf(float(x)) for x in out[:3]]
                M = [[mpmath.mpf(float(out[3 + i])) for i in row] for row in ((0, 1, 2), (1, 3, 4), (2, 4, 5))]
                mean_err = float(max(abs(o[k] + s[k] / n - m[k]) for k in range(3)))
                scatter_err = float(max(abs(M[a][b] - s[a] * s[b] / n - sc[a][b]) for a in range(3) for b in range(3)))
            worst[0] = max(worst[0], mean_err / mi.mean_ulp(v["cell"], 0.3, t, res_dst))
            worst[1] = max(worst[1], scatter_err / (2.0 ** -52 * n * L * L))
        say("host transform, 7 voxels of the 0.3 m cloud into %.1f m: mean %.3f ulp (bound 8), scatter %.3f x 2^-52 n L^2 "
            "(bound 128)" % (res_dst, worst[0], worst[1]))
    pts, _, _ = mi.general_source()
    src = api.VoxelMap(ctx, 1.0, 1.0)
    src.insert(pts)
    for res in (1.0, 2.0):
        ref, margin = mi.general_reference(res)
        dst = api.VoxelMap(ctx, res, res * res)
        dst.merge(src, R, t)
        st = dst.stats()
        dst.close()
        row = {tuple(int(x) for x in cell): k for k, cell in enumerate(st["cells"])}
        worst = [0.0, 0.0, 0.0]
        for cell, r in ref.items():
            if not r["valid"]:
                continue
            k = row[cell]
            info, lam, _ = vx.information_from_sqrt(st["sqrt_infos"][k], True)
            worst[0] = max(worst[0], float(np.abs(st["means"][k].astype(np.longdouble) - r["mean"]).max() / r["ulp"]))
            worst[1] = max(worst[1], float(np.abs(lam / r["eig_floored"] - 1.0).max()))
            worst[2] = max(worst[2], float(np.linalg.norm(info - r["info"]) / np.linalg.norm(r["info"])) - vx.merged_gap(r))
        say("device merge, 320 voxels at 1 m into %.0f m (%d cells, up to %d source voxels each, nearest face %.1e cells): "
            "mean %.3f ulp (bound 8), eigenvalues %.2e (bound %.0e), information %.2e (bound %.0e)" % (
                res, len(ref), max(len(r["members"]) for r in ref.values()), margin, worst[0], worst[1], vi.EIG_RTOL,
                worst[2], vi.INFO_RTOL))
    src.close()


def main():
    ctx = Context((0,))
    timings(ctx)
    error_maxima(ctx)
    ctx.close()
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
