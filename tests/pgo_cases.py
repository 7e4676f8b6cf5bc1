"""The graphs on which the pose-graph preconditioner is compared with its explicit restatement
(oracle/oracle_pgo.py: two_level, pcr_twin) — shared by tests/test_pgo_preconditioner.py and
tools/measure_pgo_preconditioner.py.  Every case is built once per process and then left unchanged.

A case is the smallest graph that reaches one path of the coarse level; the span structure of the cyclic
reduction (oracle_pgo.pcr_spans) at its aggregate count is part of its description."""
import functools

import numpy as np

from oracle import oracle_pgo as op

MARGIN = 32.0        # GPU tolerance = MARGIN * max(e_twin, FLOOR): rounding only (fma, Cholesky inverse, butterfly sums)
FLOOR = 1e-14
TWIN_CAP = 1e-7      # the float64 cyclic reduction itself must stay this close to the sparse LU answer


def _realistic(n=600, seed=21):
    """Chain + loop edges 2…5 poses ahead + 20 loop edges a quarter of the graph long; poses 0, 1, 2 (a whole aggregate
    of 3) and 301 (part of one) fixed."""
    d = op.random_graph(n, 0, seed=seed)
    rng = np.random.default_rng(seed + 1)
    pairs = []
    for i in range(n):
        for _ in range(2):
            j = i + int(rng.integers(2, 6))
            if j < n:
                pairs.append((i, j))
    for a in rng.integers(0, n - n // 4, 20):
        pairs.append((int(a), int(a) + n // 4))
    d = op.with_edges(d, pairs, seed=seed + 2)
    d["fixed"][[1, 2, 301]] = 1
    return d


def _ragged(n=797, seed=22):
    d = op.random_graph(n, 3, seed=seed)
    rng = np.random.default_rng(seed + 1)
    a = rng.integers(0, n // 2, 10)
    b = a + rng.integers(n // 4, n // 2, 10)
    return op.with_edges(d, [(int(x), int(y)) for x, y in zip(a, b)], seed=seed + 2)


def _free_switches(d, value):
    free = (np.arange(d["ref"].size) % 3 == 1).astype(np.uint8)
    out = dict(d)
    out["switch_free"] = free
    out["switch_init"] = np.where(free, value, 1.0)
    return out


# name → (graph builder, pgo_agg, lambda, pgo_precond, the coarse level takes part)
_SPECS = {
    "stiff_one_halo_span": (lambda: op.random_graph(600, 0, seed=31), 3, 0.0, 1, True),
    "stiff_two_halo_spans": (lambda: op.random_graph(4200, 0, seed=32), 2, 0.0, 1, True),
    "realistic_1e-3": (_realistic, 3, 1e-3, 1, True),
    "realistic_1e-6": (_realistic, 3, 1e-6, 1, True),
    "ragged_default_aggregate": (_ragged, 48, 1e-6, 1, True),
    "free_switches": (lambda: _free_switches(_realistic(), 0.7), 3, 1e-3, 1, True),
    "below_threshold": (lambda: op.random_graph(150, 3, seed=33), 48, 1e-3, 1, False),
    "block_jacobi_only": (_realistic, 3, 1e-3, 0, False),
}
NAMES = tuple(_SPECS)
STIFF = ("stiff_one_halo_span", "stiff_two_halo_spans")


class Case:
    def __init__(self, name):
        build, self.agg, self.lam, self.precond, self.coarse = _SPECS[name]
        self.name = name
        d = self.d = build()
        self.n, self.m = d["init"].shape[0], d["ref"].size
        self.graph = op.Graph(d["init"], d["ref"], d["qry"], d["meas"], d.get("switch_init"), d.get("switch_free"),
                              d["fixed"])
        self.H, self.g, self.cost = self.graph.linearize()
        self.tl = op.two_level(self.graph, self.H, self.lam, self.agg)
        self.r = self.vector(7)
        if self.coarse:
            self.z_ref = self.tl.apply(self.r)
            self.z_twin = self.tl.apply(self.r, op.pcr_twin)
            self.e_twin = self.distance(self.z_twin)
        else:
            self.z_ref = self.tl.apply_block_jacobi(self.r)
            self.z_twin, self.e_twin = self.z_ref, 0.0
        self.tol = MARGIN * max(self.e_twin, FLOOR)

    def vector(self, seed):
        """Seeded normal vector, zero on fixed poses and on switches that are not free."""
        v = np.random.default_rng(seed).normal(size=6 * self.n + self.m)
        for i in np.nonzero(self.d["fixed"])[0]:
            v[[k * self.n + i for k in range(6)]] = 0.0
        free = self.d.get("switch_free")
        if free is None:
            v[6 * self.n:] = 0.0
        else:
            v[6 * self.n:][np.asarray(free) == 0] = 0.0
        return v

    def distance(self, z):
        """max|z - z_ref| / max|z_ref|, taken over the pose rows and over the switch rows separately (the larger of the
        two): a switch row r_s / h_s can be orders of magnitude above every pose row and would hide them otherwise."""
        cut = 6 * self.n
        parts = [slice(0, cut)] + ([slice(cut, None)] if self.d.get("switch_free") is not None else [])
        return float(max(np.max(np.abs(z[p] - self.z_ref[p])) / np.max(np.abs(self.z_ref[p])) for p in parts))

    def gpu_graph(self, ctx):
        from nonlinear_optimizer_for_slam_amd import pgo
        d = self.d
        return pgo.PoseGraph(ctx, d["init"], d["ref"], d["qry"], d["meas"], d.get("switch_init"), d.get("switch_free"),
                             d["fixed"])

    def options(self, ctx, probe=0, agg=None):
        return ctx.options(pgo_agg=self.agg if agg is None else agg, pgo_precond=self.precond, pgo_coarse_probe=probe)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)
