#!/usr/bin/env python3
"""The numbers of profiles/matcher_edges.txt, with the library NOS_HIP_LIB names (default: the tree's own build).

  measure_matcher_edges.py count LABEL   per radius_sq and lookup form: the constructed pairs of tests/matcher_edge_inputs.py,
                                         the pairs the library misses and the pairs it reports beyond them (fp64,
                                         max_neighbors 2, identity pose), one JSON line each
  measure_matcher_edges.py time LABEL    the three matcher_* rows of the benchmark (bench_stages.stage_matcher), twice

To compare two builds, run the two alternately in fresh processes: one library per process."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def count(label):
    from nonlinear_optimizer_for_slam_amd import Context, api
    from tests import matcher_edge_inputs as mei
    ctx = Context((0,))
    for r2 in mei.RADII:
        for dense in (1, 0):
            pairs = missed = extra = 0
            where = {}
            for region in mei.REGIONS:
                case, idx = mei.snapshot_case(r2, region), mei.snapshot_reference(r2, region)
                with ctx.options(match_dense=dense):
                    gm = api.NdtMap(ctx, case["means"], case["sqrt_infos"], case["valid"], r2)
                sc = api.Scan(ctx, case["queries"])
                ds, _ = gm.match(sc, np.eye(3), np.zeros(3), 2, "f64")
                planes = api.download(ds)
                for h in (ds, sc, gm):
                    h.close()
                got = np.where(~planes.any(axis=0), -1, mei.id_of_sqrt_info(planes[6], planes[7])).reshape(-1, 2)
                for i in range(len(idx)):
                    w, g = set(idx[i][idx[i] >= 0].tolist()), set(got[i][got[i] >= 0].tolist())
                    pairs += len(w)
                    extra += len(g - w)
                    if w - g:
                        missed += len(w - g)
                        key = "%s/%s" % (case["family"][i], region)
                        where[key] = where.get(key, 0) + len(w - g)
            print(json.dumps({"library": label, "radius_sq": r2, "form": "dense" if dense else "hash", "pairs": pairs,
                              "missed": missed, "extra": extra, "where": where}), flush=True)
    ctx.close()


def time_rows(label):
    import bench_stages
    from nonlinear_optimizer_for_slam_amd import Context, api, synth
    planes = synth.ndt_planes(10_000_000, 200_000)
    ctx = Context((0,))
    for rep in range(2):
        out = bench_stages.stage_matcher(ctx, {"api": api, "synth": synth}, planes, False)
        print(json.dumps({"library": label, "rep": rep, **{k: v["ms"] for k, v in out.items()},
                          "matches": out["matcher_10M_cell_sorted"]["matches"],
                          "map_tables_ms": out["matcher_10M_cell_sorted"]["map_tables_ms"]}), flush=True)
    ctx.close()


if __name__ == "__main__":
    {"count": count, "time": time_rows}[sys.argv[1]](sys.argv[2] if len(sys.argv) > 2 else "build")
