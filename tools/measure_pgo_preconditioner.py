"""Accuracy of the pose-graph preconditioner (PoseGraph.precondition) against its explicit restatement, per case of
tests/pgo_cases.py and per form of the coarse operator (assembled, probed).

usage: python tools/measure_pgo_preconditioner.py [--out profiles/pgo_preconditioner_accuracy.txt]

Per case: aggregates and spans of the cyclic reduction, e_twin (distance of a float64 cyclic reduction from the sparse-LU
answer), the GPU's distance from the sparse-LU answer with either operator form, and the bound 32 max(e_twin, 1e-14);
distance = max|z - z_lu| / max|z_lu|, pose rows and switch rows taken separately.  Nothing is asserted here:
tests/test_pgo_preconditioner.py does that."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context  # noqa: E402
from oracle import oracle_pgo as op  # noqa: E402
from tests import pgo_cases as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = Context((0,))
    lines = ["# pose-graph preconditioner: distance from the explicit operator (sparse LU), max|z - z_lu| / max|z_lu|",
             "# %-26s %6s %5s %7s %-34s %10s %10s %10s %10s" % ("case", "poses", "agg", "lambda", "spans (first, end, halo)", "e_twin",
                                                               "assembled", "probed", "bound")]
    for name in pc.NAMES:
        c = pc.case(name)
        got = []
        for probe in (0, 1):
            g = c.gpu_graph(ctx)
            g.linearize()
            with c.options(ctx, probe):
                got.append(c.distance(g.precondition(c.lam, c.r)))
            g.close()
        spans = str(op.pcr_spans(c.tl.n_agg)) if c.coarse else "block-Jacobi alone"
        lines.append("  %-26s %6d %5d %7.0e %-34s %10.3e %10.3e %10.3e %10.3e" % (name, c.n, c.agg, c.lam, spans, c.e_twin, got[0],
                                                                                  got[1], c.tol))
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
