"""Cost of place recognition on the device (Scan.descriptor, PlaceDatabase.search), next to what one had
to do before: copy the scan back (scan.points()) and build the descriptor on the host, and compare descriptors on the
host (both by the numpy restatement of the rule, tests/place_inputs.py).

usage: python tools/measure_place_search.py      (output kept as profiles/place_search.txt)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min) after one warm-up
call.  Descriptor: 100 k and 1 M points at the default 20 x 60.  Search: 1 and 64 queries against 1 k, 10 k and 100 k
stored places (1 000 distinct descriptors, stored over and over: the arithmetic does not depend on the values).  The host
search is run against HOST_PLACES places and SCALED to the stored count (it is linear in it); the line says so."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, PlaceDatabase, api  # noqa: E402
from tests import place_inputs as pi  # noqa: E402

REPEATS = 5
R, S = 20, 60
HOST_PLACES = 200
SLOT_BYTES = (R + 1) * S * 8


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def measure_descriptor(ctx, n):
    rng = np.random.default_rng(n)
    pts = rng.uniform(-0.5, 0.5, size=(n, 3)) * np.array([180.0, 180.0, 10.0])
    scan = api.Scan(ctx, pts)
    scan.descriptor()  # warm-up (and the arena's slab)
    t_dev = [timed(scan.descriptor)[0] for _ in range(REPEATS)]
    t_host = [timed(lambda: pi.descriptor(scan.points(), R, S))[0] for _ in range(REPEATS)]
    scan.close()
    print("\n== descriptor of %d points (%d x %d) ==" % (n, R, S))
    print("device (resident scan)            : %s" % best_and_spread(t_dev))
    print("host route: points(), then numpy  : %s" % best_and_spread(t_host))
    print("host route / device = %.1f x   24 B per point = %.1f MB -> %.1f GB/s over the whole call" % (
        min(t_host) / min(t_dev), n * 24 / 1e6, n * 24 / (min(t_dev) * 1e-3) / 1e9))


def measure_search(ctx, db, descs, n_places, n_queries, host_ms_per_pair):
    queries = descs[:n_queries] if n_queries > 1 else descs[0]
    db.search(queries, 0, n_places)  # warm-up
    t_dev = [timed(lambda: db.search(queries, 0, n_places))[0] for _ in range(REPEATS)]
    best = min(t_dev)
    flop = 2.0 * S * S * R * n_places * n_queries
    print("%3d quer%s x %6d places : %s   %.1f MB read, %.2f GFLOP -> %.1f GFLOP/s; host (scaled) %.0f ms = %.0f x" % (
        n_queries, "y  " if n_queries == 1 else "ies", n_places, best_and_spread(t_dev), n_places * SLOT_BYTES / 1e6, flop / 1e9,
        flop / (best * 1e-3) / 1e9, host_ms_per_pair * n_places * n_queries, host_ms_per_pair * n_places * n_queries / best))


def main():
    ctx = Context((0,))
    print("best of %d, spread = max - min; host clock, every call ends in a synchronisation" % REPEATS)
    for n in (100_000, 1_000_000):
        measure_descriptor(ctx, n)
    descs = pi.random_descriptors(1000, R, S, seed=0)
    t_host = [timed(lambda: pi.distance(descs[0], descs[:HOST_PLACES]))[0] for _ in range(REPEATS)]
    host_ms_per_pair = min(t_host) / HOST_PLACES
    print("\n== search (%d x %d), one launch and one wait per call ==" % (R, S))
    print("host restatement, 1 query x %d places: %s -> %.4f ms per pair, SCALED linearly below" % (
        HOST_PLACES, best_and_spread(t_host), host_ms_per_pair))
    db = PlaceDatabase(ctx, n_rings=R, n_sectors=S, reserve=100_000)
    for n_places in (1_000, 10_000, 100_000):
        t_add, _ = timed(lambda: [db.add(descs[k % len(descs)]) for k in range(len(db), n_places)])
        print("(stored up to %d places: %.1f ms, one add and one wait each)" % (n_places, t_add))
        for n_queries in (1, 64):
            measure_search(ctx, db, descs, n_places, n_queries, host_ms_per_pair)
    # the query as a resident scan: descriptor and search in one call, nothing visits the host but the result
    scan = api.Scan(ctx, np.random.default_rng(1).uniform(-0.5, 0.5, size=(100_000, 3)) * np.array([180.0, 180.0, 10.0]))
    db.search(scan, 0, 10_000)
    t_scan = [timed(lambda: db.search(scan, 0, 10_000))[0] for _ in range(REPEATS)]
    print("scan of 100 k points x  10000 places : %s   (descriptor + search, one wait)" % best_and_spread(t_scan))
    scan.close()
    db.close()
    ctx.close()


if __name__ == "__main__":
    main()
