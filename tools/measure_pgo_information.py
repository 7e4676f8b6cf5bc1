"""What a 6x6 information matrix per constraint costs: the product of a PCG iteration, the linearisation
sweeps and one solve on a 1 M-pose / ~4 M-constraint graph, weighted against unweighted with the block-local product
(pgo_block=1) and with the owner-computes product (pgo_block=0) — the form a weighted graph always takes.

    python tools/measure_pgo_information.py [n_poses] > profiles/pgo_information.txt

Sweeps: nos_pgo_time_sweep (HIP events around `repeats` launches); create and solve: host clock around the call, as the
other measure_* tools use it.  Nothing here is asserted anywhere."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nonlinear_optimizer_for_slam_amd import Context, pgo, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
d = synth.pose_graph(n, 3)
m = d["ref"].size
print("%d poses, %d constraints" % (n, m), flush=True)
# one seeded full-rank information per constraint: Q^T diag(10^U[0, 3]) Q from 64 distinct matrices
rng = np.random.default_rng(5)
bank = np.zeros((64, 21))
for k in range(64):
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    A = Q.T @ np.diag(10.0 ** rng.uniform(0.0, 3.0, size=6)) @ Q
    bank[k] = (0.5 * (A + A.T))[np.triu_indices(6)]
information = bank[rng.integers(0, 64, size=m)]
ctx = Context((0,))
LAM = 1e-3
for label, block, info in (("unweighted, block-local product (pgo_block=1)", 1, None),
                           ("unweighted, owner-computes product (pgo_block=0)", 0, None),
                           ("weighted (owner-computes product, probed coarse operator)", 1, information)):
    with ctx.options(pgo_block=block):
        t0 = time.perf_counter()
        g = pgo.PoseGraph(ctx, d["init"], d["ref"], d["qry"], d["meas"], None, None, d["fixed"], information=info)
        create_ms = 1e3 * (time.perf_counter() - t0)
        cost, gnorm = g.linearize()
        lin = g.time_sweep("linearize", LAM, 20)
        mv = g.time_sweep("matvec", LAM, 20)
        t0 = time.perf_counter()
        it, res, _ = g.solve(LAM, 300, 1e-6)
        solve_ms = 1e3 * (time.perf_counter() - t0)
        layout = g.layout_info()
        g.close()
    print("%s\n  create %.1f ms; entries %d; cost %.6g |g| %.4g\n  linearize %.3f ms/sweep; matvec %.3f ms/product; "
          "solve(lambda %g, tol 1e-6): %d PCG iterations in %.1f ms (%.3f ms/iteration), residual %.2e"
          % (label, create_ms, layout["entries"], cost, gnorm, lin, mv, LAM, it, solve_ms, solve_ms / max(it, 1), res), flush=True)
ctx.close()
