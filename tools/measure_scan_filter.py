"""Cost of the device voxel-grid scan filter (Scan.filtered / nos_scan_filter) on an already-resident scan, next to
 (a) the host route a caller had before it: filter on the host (numpy: one packed int64 key per point, np.unique), then
     upload the kept points (Scan(ctx, kept)) — reported as a ratio, and
 (b) nos_ndt_map_build of the same points at the same resolution (NdtMap.build, statistics not downloaded): the filter reads
     the same points and does strictly less, so it must not take longer — the acceptance condition.

usage: python tools/measure_scan_filter.py [--single CLOUD]      (output kept as profiles/scan_filter.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min); the filter and the map
build alternate in the same process (filter, build, filter, build, …) after one warm-up call of each.  --single CLOUD
(room, synth10m or dup64): one warmed-up filter of that cloud and nothing else after the set-up, for a kernel-trace run
of its own (rocprofv3 --kernel-trace --stats -- python tools/measure_scan_filter.py --single synth10m)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api, synth  # noqa: E402

REPEATS = 5


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def host_filter(pts, vs):
    """First point per integer cell in index order, as fast as numpy does it: one int64 key per point (21 bits per axis,
    the library's packing) and a 1-D np.unique."""
    c = np.floor(pts * (1.0 / vs)).astype(np.int64) + (1 << 20)
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    _, first = np.unique(key, return_index=True)
    return pts[np.sort(first)]


def clouds():
    rng = np.random.default_rng(3)  # the cloud of bench_stages.py::stage_mapbuild
    synth10m = rng.uniform(-0.5, 0.5, size=(10_000_000, 3)) * np.array([100.0, 100.0, 10.0])
    base = np.random.default_rng(64).uniform([-30, -30, -3], [30, 30, 3], size=(20_000, 3))
    return {"room": (synth.room_points(), (0.1, 0.05)),            # 954 605 points: 9 356 / 37 711 kept
            "synth10m": (synth10m, (1.0, 0.5)),                    # about 100 k / 796 k cells
            "dup64": (np.repeat(base, 64, axis=0), (0.5,))}         # every point 64 times in a row


def measure(ctx, name, pts, vs):
    n = pts.shape[0]
    scan = api.Scan(ctx, pts)
    f = scan.filtered(vs)  # warm-up (and the arena's slab)
    kept = len(f)
    f.close()
    m, _ = api.NdtMap.build(ctx, pts, voxel_resolution=vs, return_stats=False)
    m.close()
    t_filter, t_build = [], []
    for _ in range(REPEATS):  # alternate
        ms, f = timed(lambda: scan.filtered(vs))
        t_filter.append(ms)
        f.close()
        ms, (m, _) = timed(lambda: api.NdtMap.build(ctx, pts, voxel_resolution=vs, return_stats=False))
        t_build.append(ms)
        m.close()
    t_host = []
    for _ in range(3):
        def host_route():
            s = api.Scan(ctx, host_filter(pts, vs))
            assert len(s) == kept
            return s
        ms, s = timed(host_route)
        t_host.append(ms)
        s.close()
    scan.close()
    fb, bb = min(t_filter), min(t_build)
    spread = max(max(t_filter) - fb, max(t_build) - bb)
    moved = n * (24 + 12 + 4) + kept * 28
    print("\n== %s: %d points at %.2f m -> %d kept ==" % (name, n, vs, kept))
    print("device filter (resident scan)         : %s" % best_and_spread(t_filter))
    print("(b) nos_ndt_map_build, same points     : %s" % best_and_spread(t_build))
    print("(a) host route, numpy filter + upload  : %s" % best_and_spread(t_host))
    print("filter / map build = %.3f   host route / filter = %.1f x   condition (b) filter <= build + spread: %s" % (
        fb / bb, min(t_host) / fb, "met" if fb <= bb + spread else "NOT met"))
    print("bytes moved (24 B read + 12 B table + 4 B entry per point, 28 B per kept point) = %.1f MB -> %.0f GB/s" % (
        moved / 1e6, moved / (fb * 1e-3) / 1e9))


def main():
    ctx = Context((0,))
    all_clouds = clouds()
    if "--single" in sys.argv:
        name = sys.argv[sys.argv.index("--single") + 1]
        pts, resolutions = all_clouds[name]
        scan = api.Scan(ctx, pts)
        scan.filtered(resolutions[0]).close()
        ctx.synchronize()
        ms, f = timed(lambda: scan.filtered(resolutions[0]))
        print("single filter of %s (%d points at %.2f m): %.3f ms, %d kept" % (name, pts.shape[0], resolutions[0], ms, len(f)))
        return
    print("best of %d, spread = max - min; host clock, every call ends in a synchronisation; filter and build alternate" % REPEATS)
    for name in ("room", "synth10m", "dup64"):
        pts, resolutions = all_clouds[name]
        for vs in resolutions:
            measure(ctx, name, pts, vs)
    ctx.close()


if __name__ == "__main__":
    main()
