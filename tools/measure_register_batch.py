"""Wall time of B scan-to-map registrations: one batched call (pipeline.scan_to_map_batch, one launch) against a loop of
lone pipeline.scan_to_map calls.

Host clock around a call that ends in a synchronisation, best of 3.  Scenes: the reference's room map built on the device
(reference-exact), and
  small: B in {1, 16, 64, 256, 1024} scans of 500 points (random subsets of the simple_6dof scan), from identity,
  large: the simple_6dof scan itself (9 356 points, keep_multiple = 4) for B in {1, 16, 64},
both with the exponential loss and at most 10 outer rounds.

  python tools/measure_register_batch.py --impl batch            # this tree
  python tools/measure_register_batch.py --impl loop [--root DIR] # lone loop; DIR = a checkout of another revision

One JSON line per (scene, B) on stdout.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["batch", "loop"], required=True)
    ap.add_argument("--root", default=ROOT, help="repository whose package is imported")
    ap.add_argument("--label", default="")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    import numpy as np
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Options, Pose
    from oracle import oracle_scene as scene

    loss = ("exponential", 1.0, 1.0)
    ctx = api.Context((0,))
    pts = scene.generate_global_points()
    gm, _ = api.NdtMap.build(ctx, pts, 1.0, 1.0, reference_exact=True, return_stats=False)
    local, _, _ = scene.captured_run_scan(pts, "simple_6dof")
    rng = np.random.default_rng(1)
    small = [api.Scan(ctx, local[np.sort(rng.choice(local.shape[0], 500, replace=False))]) for _ in range(1024)]
    large = api.Scan(ctx, local)

    def run(scans, keep):
        if a.impl == "batch":
            return pipeline.scan_to_map_batch(ctx, gm, scans, None, loss, Options(), keep_multiple=keep)
        return [pipeline.scan_to_map(ctx, gm, s, Pose(), loss, Options(), keep_multiple=keep) for s in scans]

    cases = [("small500", B, small[:B], None) for B in (1, 16, 64, 256, 1024)]
    cases += [("simple_6dof_9356", B, [large] * B, 4) for B in (1, 16, 64)]
    for name, B, scans, keep in cases:
        run(scans, keep)  # warm-up: kernels loaded, pool filled
        best = np.inf
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = run(scans, keep)
            best = min(best, time.perf_counter() - t0)
        rounds = sum(len(r[1]) for r in out if r is not None)
        print(json.dumps({"impl": a.impl, "label": a.label, "scene": name, "B": B, "best_ms": round(best * 1e3, 3),
                          "ms_per_problem": round(best * 1e3 / B, 4), "rounds": rounds}), flush=True)
    for s in small + [large]:
        s.close()
    gm.close()
    ctx.close()


if __name__ == "__main__":
    main()
