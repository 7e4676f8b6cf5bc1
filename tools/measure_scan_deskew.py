"""Cost of the device scan deskew (Scan.deskewed / nos_scan_deskew) on an already-resident scan, next to the route it
replaces: copy the raw frame back (scan.points()), correct it on the host (the numpy restatement of the rule, DESIGN.md
§24), upload it again (api.Scan(ctx, ...)).

usage: python tools/measure_scan_deskew.py      (output kept as profiles/scan_deskew.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min) after one warm-up call,
at 100 k, 1 M and 10 M points.  The device call includes the upload of the time stamps (8 B per point over the host link),
which the 64 B per point of device traffic (24 in, 8 time, 4 order, 24 out, 4 order out; a scan without an order moves
56) do not count: the GB/s figure is 64 B per point over the whole call, not the kernel's own rate."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402
from nonlinear_optimizer_for_slam_amd.pipeline import _SERIES_THETA  # noqa: E402

REPEATS = 5
TWIST = np.array([1.5, -0.2, 0.05, 0.01, -0.02, 0.3])  # a car
BYTES_PER_POINT = 64


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def host_deskew(p, s, s_ref, twist):
    """The rule in numpy float64, as a caller without the device call would write it."""
    v, w = twist[:3], twist[3:]
    tau = (s - s_ref)[:, None]
    phi, u = tau * w, tau * v
    q = np.sum(phi * phi, axis=1, keepdims=True)
    theta = np.sqrt(q)
    th = np.where(q == 0.0, 1.0, theta)
    a = np.where(q == 0.0, 1.0, np.sin(th) / th)
    b = np.where(q == 0.0, 0.5, 2.0 * np.sin(0.5 * th) ** 2 / (th * th))
    series = 1 / 6 + q * (-1 / 120 + q * (1 / 5040 + q * (-1 / 362880 + q * (1 / 39916800 - q / 6227020800))))
    c = np.where(theta < _SERIES_THETA, series, (th - np.sin(th)) / (th * th * th))
    pp, pu = np.cross(phi, p), np.cross(phi, u)
    return p + a * pp + b * np.cross(phi, pp) + u + b * pu + c * np.cross(phi, pu)


def measure(ctx, n, sort_cell=None):
    rng = np.random.default_rng(n)
    pts = rng.uniform(-0.5, 0.5, size=(n, 3)) * np.array([100.0, 100.0, 10.0])
    times = rng.uniform(0.0, 1.0, size=n)
    scan = api.Scan(ctx, pts, sort_cell=sort_cell)
    scan.deskewed(times, TWIST).close()  # warm-up (and the arena's slab)
    t_dev, t_host = [], []
    for _ in range(REPEATS):
        ms, d = timed(lambda: scan.deskewed(times, TWIST))
        t_dev.append(ms)
        d.close()
    for _ in range(REPEATS if n <= 1_000_000 else 2):
        def host_route():
            raw = scan.points()
            return api.Scan(ctx, host_deskew(raw, times[scan.order] if sort_cell else times, 1.0, TWIST))
        ms, s = timed(host_route)
        t_host.append(ms)
        s.close()
    scan.close()
    best = min(t_dev)
    per_point = BYTES_PER_POINT
    print("\n== %d points%s ==" % (n, ", cell-sorted (with an order)" if sort_cell else ""))
    print("device deskew (resident scan)                 : %s" % best_and_spread(t_dev))
    print("host route: points(), numpy, upload a new scan : %s" % best_and_spread(t_host))
    print("host route / device = %.1f x   %d B per point = %.1f MB -> %.1f GB/s over the whole call" % (
        min(t_host) / best, per_point, n * per_point / 1e6, n * per_point / (best * 1e-3) / 1e9))


def main():
    ctx = Context((0,))
    print("best of %d, spread = max - min; host clock, every call ends in a synchronisation" % REPEATS)
    for n in (100_000, 1_000_000, 10_000_000):
        measure(ctx, n)
    measure(ctx, 1_000_000, sort_cell=1.0)
    ctx.close()


if __name__ == "__main__":
    main()
