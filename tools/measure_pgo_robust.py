"""What a robust loss on the constraints costs: the product of a PCG iteration, the linearisation sweeps
and one solve on a 1 M-pose / ~4 M-constraint graph with information, without a loss and under either loss kind —
alternated on ONE graph (set_loss, linearize, measure), several rounds, so that the run-to-run spread stands next to the
difference.

    python tools/measure_pgo_robust.py [n_poses] [rounds] [none] > profiles/pgo_robust.txt

A library without nos_pgo_set_loss (an older build named by NOS_HIP_LIB) measures the rows without a loss alone: the same
tool gives the weighted product of the commit before.  `none` as third argument makes this build do the same — rounds
without a loss back to back, the schedule the older build is measured under (the first sweeps after a change of loss run
at another clock than sweeps that repeat the round before).  Sweeps: nos_pgo_time_sweep (HIP events around `repeats` launches);
solve: host clock around the call.  Nothing here is asserted anywhere."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nonlinear_optimizer_for_slam_amd import Context, pgo, synth  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
d = synth.pose_graph(n, 3)
m = d["ref"].size
print("%d poses, %d constraints, %d rounds" % (n, m, rounds), flush=True)
# one seeded full-rank information per constraint: Q^T diag(10^U[0, 3]) Q from 64 distinct matrices (measure_pgo_information.py)
rng = np.random.default_rng(5)
bank = np.zeros((64, 21))
for k in range(64):
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    A = Q.T @ np.diag(10.0 ** rng.uniform(0.0, 3.0, size=6)) @ Q
    bank[k] = (0.5 * (A + A.T))[np.triu_indices(6)]
information = bank[rng.integers(0, 64, size=m)]
ctx = Context((0,))
LAM = 1e-3
g = pgo.PoseGraph(ctx, d["init"], d["ref"], d["qry"], d["meas"], None, None, d["fixed"], information=information)
has_loss = hasattr(ctx._lib, "nos_pgo_set_loss") and (len(sys.argv) < 4 or sys.argv[3] != "none")
losses = [("no loss", None)]
if has_loss:
    # thresholds at the scale of the graph's own q: sqrt(cost / m) is the root-mean-square sqrt(q)
    cost, _ = g.linearize()
    rms = float(np.sqrt(cost / m))
    losses += [("huber(%.3g)" % rms, ("huber", rms)), ("exponential(1, %.3g)" % (1.0 / rms ** 2), ("exponential", 1.0, 1.0 / rms ** 2))]
else:
    print("the rows without a loss only (asked for, or this library has no nos_pgo_set_loss)", flush=True)
rows = {label: [] for label, _ in losses}
for r in range(rounds):
    for label, loss in losses:
        if has_loss:
            g.set_loss(loss)
        cost, gnorm = g.linearize()
        lin = g.time_sweep("linearize", LAM, 20)
        mv = g.time_sweep("matvec", LAM, 20)
        t0 = time.perf_counter()
        it, res, _ = g.solve(LAM, 300, 1e-6)
        solve_ms = 1e3 * (time.perf_counter() - t0)
        rows[label].append((lin, mv, solve_ms / max(it, 1)))
        rejected = int(np.sum(g.edge_weights() < 0.5)) if has_loss else 0
        print("round %d  %-28s cost %.6g |g| %.4g  linearize %.3f ms/sweep  matvec %.3f ms/product  solve(lambda %g, tol 1e-6): "
              "%d PCG iterations in %.1f ms (%.3f ms/iteration), residual %.2e; weights below 0.5: %d"
              % (r, label, cost, gnorm, lin, mv, LAM, it, solve_ms, solve_ms / max(it, 1), res, rejected), flush=True)
g.close()
ctx.close()
print("\nmedian [min … max] over the rounds")
for label, _ in losses:
    a = np.array(rows[label])
    print("  %-28s " % label + "  ".join("%s %.3f [%.3f … %.3f]" % (what, np.median(a[:, k]), a[:, k].min(), a[:, k].max())
                                         for k, what in enumerate(("linearize ms", "matvec ms", "PCG iteration ms"))))
