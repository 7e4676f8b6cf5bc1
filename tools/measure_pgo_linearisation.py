"""Accuracy of the pose-graph linearisation, products and retraction against the 50-digit reference of
tests/pgo_hard_inputs.py, per family, quantity and product form (owner-computes, block-local).

usage: python tools/measure_pgo_linearisation.py [--out profiles/pgo_linearisation_accuracy.txt]

Error = max |got - reference| / scale in units of 2^-52, the scale being the expression with every operand replaced by
its absolute value; yardstick = the float64 scipy assembly of oracle/oracle_pgo.py in the same measure; bound =
max(4 x yardstick, 8).  `differ` counts the product entries in which the two forms do not agree bit for bit (they round
s J^T v in different places).  Nothing is asserted here: tests/test_pgo_xprec_gpu.py does that."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, pgo  # noqa: E402
from tests import pgo_hard_inputs as hi  # noqa: E402

MEASURED = [q for q in hi.QUANTITIES if q != "switch_curvature"]


def _graph(ctx, st, block):
    with ctx.options(pgo_block=block):
        return pgo.PoseGraph(ctx, st["poses"], st["ref"], st["qry"], st["meas"], st["sw"], st["free"], st["fixed"])


def _gpu(g, st, x):
    cost, gnorm = g.linearize()
    products = {lam: g.matvec(lam, x) for lam in hi.LAMBDAS}
    return hi.split_gpu(st["poses"].shape[0], cost, g.vector("gradient"), g.vector("hdiag"), products), gnorm, products


def _rows(lines, label, st, x, ref, yard, got):
    """got: [(quantities, gnorm, products)] for the owner-computes and the block-local form"""
    xp, scale = ref
    bound = hi.bounds(yard)
    differ = sum(int(np.sum(got[0][2][lam] != got[1][2][lam])) for lam in hi.LAMBDAS)
    for q in MEASURED:
        err = [max(hi.error_eps(g[0][q][lam], xp[q][lam], scale[q][lam]) for lam in hi.LAMBDAS) if q.endswith("product")
               else hi.error_eps(g[0][q], xp[q], scale[q]) for g in got]
        lines.append("  %-24s %6d %7d  %-16s %9.2f %9.2f %9.2f %7.1f %7s" % (
            label, st["poses"].shape[0], st["ref"].size, q, yard[q], err[0], err[1], bound[q],
            differ if q == "product" else ""))
    err = [hi.gnorm_error_eps(g[1], ref) for g in got]
    lines.append("  %-24s %6d %7d  %-16s %9s %9.2f %9.2f %7.1f" % (label, st["poses"].shape[0], st["ref"].size, "gnorm", "-",
                                                                  err[0], err[1], 8.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = Context((0,))
    lines = ["# pose-graph linearisation, product (lambda 0 and 1e-3, the worse) and retraction against 50 digits:",
             "# max |got - reference| / scale in units of 2^-52 (scale: the expression on absolute values)",
             "# %-24s %6s %7s  %-16s %9s %9s %9s %7s %7s" % ("state", "poses", "constr", "quantity", "yardstick", "owner", "block",
                                                            "bound", "differ")]
    for name in hi.FAMILIES:
        st = hi.family(name)
        x = hi.masked_x(st)
        got = []
        for block in (0, 1):
            g = _graph(ctx, st, block)
            got.append(_gpu(g, st, x))
            g.close()
        _rows(lines, name, st, x, hi.family_reference(name), hi.family_yardstick(name), got)
    # the state after a retraction: each form on the state its own step led to
    for name in ("baseline", "switches"):
        st = hi.family(name)
        for block in (0, 1):
            g = _graph(ctx, st, block)
            g.linearize()
            g.solve(1e-3, 200, 1e-10)
            g.retract()
            poses, sw = g.state()
            new = dict(st, poses=poses, sw=sw)
            x = hi.masked_x(new, seed=1)
            one = _gpu(g, new, x)
            g.close()
            ref = hi.reference(new, x)
            yard, (xp, scale) = hi.yardstick(new, x, ref), ref
            for q in MEASURED:
                err = (max(hi.error_eps(one[0][q][lam], xp[q][lam], scale[q][lam]) for lam in hi.LAMBDAS)
                       if q.endswith("product") else hi.error_eps(one[0][q], xp[q], scale[q]))
                cols = ("%9.2f %9s" % (err, "-")) if block == 0 else ("%9s %9.2f" % ("-", err))
                lines.append("  %-24s %6d %7d  %-16s %9.2f %s %7.1f" % (name + " after retract", st["poses"].shape[0],
                                                                       st["ref"].size, q, yard[q], cols, hi.bounds(yard)[q]))
    # retraction from the step read back
    st = hi.retraction_graph()
    n, free_pose = st["poses"].shape[0], st["fixed"] == 0
    g = _graph(ctx, st, 1)
    g.linearize()
    g.solve(hi.RETRACT_LAMBDA, 50, 1e-13)
    before, _ = g.state()
    step = g.vector("step")
    g.retract()
    after, _ = g.state()
    g.close()
    dw = hi.rotation_steps(n, step)
    xp = hi.retract_xp(before[free_pose, 3:], dw[free_pose])
    yard = hi.quaternion_error_eps(hi.oracle_retract(st, step)[0][free_pose, 3:], xp)
    err = hi.quaternion_error_eps(after[free_pose, 3:], xp)
    lines.append("# retraction of %d poses, |dw| from %.1e to %.2f rad, %d / %d of them just below / at or above the 1e-6 branch:"
                 % ((int(np.sum(free_pose)), np.min(np.linalg.norm(dw[free_pose], axis=1)), np.max(np.linalg.norm(dw[free_pose], axis=1)))
                    + hi.branch_counts(dw)))
    lines.append("# largest absolute quaternion component error in units of 2^-52, and | |q| - 1 |")
    lines.append("  %-24s %6d %7d  %-16s %9.2f %9s %9.2f %7.1f" % ("retraction", n, st["ref"].size, "quaternion", yard, "-", err,
                                                                  max(4 * yard, 8.0)))
    lines.append("  %-24s %6d %7d  %-16s %9s %9s %9.2f %7.1f" % ("retraction", n, st["ref"].size, "norm", "-", "-",
                                                                hi.norm_error_eps(after[free_pose, 3:]), 4.0))
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
