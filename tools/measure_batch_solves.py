"""Batched solve (nos_*_solve_batch) against a Python loop of lone solves (nos_*_solve): wall time and problems per second.

B = 1, 16, 64, 256, 1 024, 4 096 problems of 20 LM iterations each (tolerances 0), four workloads: the reference's
reprojection size (630 points), 1 000 NDT correspondences (both inside the default batch_max_elements), and 4 000 / 20 000
NDT correspondences with batch_max_elements raised so that they run in the batch launch too — one workgroup looping over
all chunks of its problem — while their lone solves take the one-launch form across all CUs.  The problems cycle through 16
datasets of different seeds; every start pose is its own.  Time = best of 3 calls on the host clock, each call ending in
its own device synchronisation.  Every workload runs in a child process of its own under `timeout`; the first one that
fails ends the run.

usage: python tools/measure_batch_solves.py [--out FILE]   (one JSON line per workload and B; FILE gets the same lines)
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = (1, 16, 64, 256, 1024, 4096)
ITERATIONS = 20
WORKLOADS = {  # name: (problem, correspondences, batch_max_elements raised to cover them)
    "reproj630": ("reproj", 630, False),
    "ndt1000": ("ndt6", 1000, False),
    "ndt4000": ("ndt6", 4000, True),
    "ndt20000": ("ndt6", 20000, True),
}
CHILD_TIMEOUT_S = 240


def run_workload(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    from nonlinear_optimizer_for_slam_amd import Context, NdtDataset, ReprojDataset, synth
    from nonlinear_optimizer_for_slam_amd.api import reproj_solve_batch, solve6_batch
    problem, n, raised = WORKLOADS[name]
    ctx = Context((0,))
    loss = ("exponential", 1.0, 1.0)
    args = dict(max_iterations=ITERATIONS, gradient_tolerance=0.0, parameter_tolerance=0.0)
    if problem == "reproj":
        sets = [ReprojDataset.from_planes(ctx, synth.reproj_planes(n, seed=s), "f64") for s in range(16)]
        batch = lambda order, R, t: reproj_solve_batch(order, R, t, synth.REPROJ_INTR4, loss, **args)  # noqa: E731
        lone = lambda ds, R, t: ds.solve(R, t, synth.REPROJ_INTR4, loss, **args)  # noqa: E731
    else:
        sets = [NdtDataset.from_planes(ctx, synth.ndt_planes(n, max(1, n // 30), seed=s), "f64") for s in range(16)]
        batch = lambda order, R, t: solve6_batch(order, R, t, loss, **args)  # noqa: E731
        lone = lambda ds, R, t: ds.solve6(R, t, loss, **args)  # noqa: E731
    if raised:
        ctx.set_option("batch_max_elements", n * (5 if problem == "reproj" else 15))

    def best_of(fn, repeats=3):
        fn()  # warm-up: code objects, pools, pinned staging
        best = 1e30
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = fn()
            best = min(best, time.perf_counter() - t0)
        return best, out

    for B in BATCHES:
        order = [sets[i % len(sets)] for i in range(B)]
        R0, t0 = synth.random_poses(B, seed=B)
        tb, (_, _, reps) = best_of(lambda: batch(order, R0, t0))
        kernel = ctx.last_kernel()
        tl, lone_reps = best_of(lambda: [lone(order[i], R0[i], t0[i])[2] for i in range(B)])
        row = {"workload": name, "n": n, "B": B, "iterations": ITERATIONS,
               "batch_max_elements": ctx.get_option("batch_max_elements"),
               "batch_ms": round(tb * 1e3, 4), "loop_ms": round(tl * 1e3, 4),
               "batch_problems_per_s": round(B / tb, 1), "loop_problems_per_s": round(B / tl, 1),
               "speedup": round(tl / tb, 3),
               "batch_launches": sorted({r["launches"] for r in reps}), "loop_launches": sorted({r["launches"] for r in lone_reps}),
               "iterations_done": sorted({r["iterations"] for r in reps}),
               "batch_kernel": kernel.split("(")[0]}
        print(json.dumps(row), flush=True)
    for ds in sets:
        ds.close()
    ctx.close()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--workload":
        run_workload(sys.argv[2])
        return 0
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    sink = open(out, "w") if out else None
    for name in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--workload", name]
        p = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        if sink:
            sink.write(p.stdout)
            sink.flush()
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            print("workload %s ended with status %d: stopping" % (name, p.returncode), file=sys.stderr)
            return p.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
