"""One call of each voxel-store, scan-filter and scan-deskew entry point at small shapes, each inside the context's profile
bracket (Context.profile_begin(.., sample_every=0) / profile_end): prints the launch count the library reports for it.

usage: python tools/measure_voxel_store_calls.py      (output kept in profiles/voxel_store_host.txt)

Shapes: a cell-sorted scan of 257 points (a block plus one), a store of 17 voxels from 136 points (one past the minimum
capacity of 16), a second store holding the scan.  Calls, in this order: insert, insert_scan, merge, export with a box,
prune, carve, raycast without and with hit points, restore, add, filter, deskew.  NOS_HIP_LIB selects another build of the
library, so two builds can be compared.  The bracket counts only what a path reports to it (assemble, match, registration,
score); for the whole sequence of device work run the script under a kernel trace and order the dispatches by start time:

    rocprofv3 --kernel-trace --output-format csv -d OUT -o trace -- python tools/measure_voxel_store_calls.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

I3, Z3 = np.eye(3), np.zeros(3)
rng = np.random.default_rng(17)
cells = np.array([(3 + (k % 6) * 2, -6 + (k // 6) * 5, (k % 3) - 1) for k in range(17)], dtype=np.float64)
store_points = (cells[:, None, :] + 0.5 + rng.uniform(-0.3, 0.3, size=(17, 8, 3))).reshape(-1, 3)
means = store_points.reshape(17, 8, 3).mean(axis=1)
pts = means[np.arange(257) % 17] * rng.uniform(0.6, 1.4, size=(257, 1))
pts[3::4] = np.array([0.1, 0.2, 5.0]) * rng.uniform(0.6, 1.4, size=(len(pts[3::4]), 1))
times = rng.uniform(0.0, 1.0, size=257)
XI = np.array([0.3, -0.2, 0.05, 0.02, -0.01, 0.15])

ctx = Context((0,))
rows = []


def bracket(name, fn):
    ctx.profile_begin(4096, 0)
    out = fn()
    n = ctx.profile_end()[0]
    rows.append((name, n))
    return out


scan = api.Scan(ctx, pts, sort_cell=1.0)
vm = api.VoxelMap(ctx, 1.0, 1.0)
other = api.VoxelMap(ctx, 1.0, 1.0)
bracket("insert (136 points, 17 voxels)", lambda: vm.insert(store_points))
bracket("insert_scan (257 points)", lambda: other.insert_scan(scan, I3, Z3))
bracket("merge (into 17 voxels)", lambda: vm.merge(other, I3, np.array([0.25, 0.0, 0.0])))
state = bracket("export with a selection (box)", lambda: vm.export(center=(6, 0, 0), half_extent=(4, 8, 3)))
bracket("prune (box)", lambda: vm.prune(center=(6, 0, 0), half_extent=(6, 8, 3)))
bracket("carve (257 rays)", lambda: vm.carve(scan, I3, Z3, max_range=40.0))
bracket("raycast without hit points", lambda: vm.raycast(scan, I3, Z3, 40.0))
hit = bracket("raycast with hit points", lambda: vm.raycast(scan, I3, Z3, 40.0, points=True))[2]["scan"]
fresh = api.VoxelMap(ctx, 1.0, 1.0)
bracket("restore", lambda: fresh.restore(state))
bracket("add", lambda: vm.add(state))
f = bracket("filter (257 points)", lambda: scan.filtered(1.0))
d = bracket("deskew (257 points)", lambda: scan.deskewed(times, XI))
print("lib: %s" % (os.environ.get("NOS_HIP_LIB") or "in-tree"))
print("sizes: store %d voxels, other %d, state %d, hit scan %d, filtered %d, deskewed %d, fresh %d" % (
    len(vm), len(other), len(state["counts"]) if isinstance(state, dict) else -1, len(hit), len(f), len(d), len(fresh)))
for name, n in rows:
    print("%-36s %d" % (name, n))
ctx.close()
