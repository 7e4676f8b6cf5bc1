"""Cost of moving a voxel store's state off the device and back (VoxelMap.export / restore / add / save / load,
DESIGN.md §31) next to the only route that existed before: inserting the points again.

usage: python tools/measure_voxel_map_state.py      (writes profiles/voxel_map_state.txt and prints it)

Host clock around calls that end in a stream synchronisation; best of 5 and the spread (max - min), one untimed call
first.  Stores of 100 k and 796 k voxels at 1 m (every cell of a box filled, as tools/measure_voxel_map_carve.py builds
them), 10 M points each, plus a block of 300 voxels 50 m away from the body: what a box around the body leaves out.
export(): every voxel, one wait.  restore: a fresh empty store with room for the voxels takes the exported state.
page out / in: export(box, removed=True) + prune(box) + add of what was exported, for a box that leaves out the 300
voxels of the block and one that also leaves out a tenth of the body; every timed round works on the same store, which
is whole again after the add (the voxels that travelled are appended, so the ids change; the work does not).
insert of the store's points: ONE insert of 40 points per voxel into an empty store of the same capacity — what a caller
who had kept the points (nobody does) would pay to rebuild the map.
save / load: wall time of the .npz round trip on the local file system, export and restore included."""
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nonlinear_optimizer_for_slam_amd import Context, api  # noqa: E402

REPEATS = 5
OUT = os.path.join(ROOT, "profiles", "voxel_map_state.txt")
LINES = []


def say(line=""):
    print(line, flush=True)
    LINES.append(line)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def best_and_spread(ms):
    return "best %9.3f ms  spread %8.3f ms  (%s)" % (min(ms), max(ms) - min(ms), " ".join("%.3f" % x for x in ms))


def repeat(fn):
    fn()
    return [timed(fn)[0] for _ in range(REPEATS)]


def main():
    rng = np.random.default_rng(20261020)
    ctx = Context((0,))
    say("best of %d, spread = max - min; host clock, every call ends in a synchronisation" % REPEATS)
    for label, box in (("100 k voxels", [100.0, 100.0, 10.0]), ("796 k voxels", [199.0, 200.0, 20.0])):
        vm = api.VoxelMap(ctx, 1.0, 1.0)
        for _ in range(10):
            vm.insert(rng.uniform([0, 0, 0], box, size=(1_000_000, 3)))
        vm.insert(rng.uniform([box[0] + 50, 0, 0], [box[0] + 60, 10, 3], size=(12_000, 3)))  # 300 voxels apart from the body
        V = len(vm)
        state = vm.export()
        nbytes = sum(state[k].nbytes for k in ("cells", "counts", "sums", "stamps"))
        say("\n== store of %d voxels (%s), %d points; a state of %.1f MB ==" % (V, label, vm.n_points, nbytes / 1e6))
        ms = repeat(vm.export)
        say("export(), every voxel                          : %s" % best_and_spread(ms))
        ms = []
        for k in range(REPEATS + 1):
            fresh = api.VoxelMap(ctx, 1.0, 1.0, capacity=V)
            ctx.synchronize()
            one, _ = timed(lambda: fresh.restore(state))
            assert len(fresh) == V
            fresh.close()
            if k > 0:
                ms.append(one)
        say("restore into an empty store (capacity given)   : %s" % best_and_spread(ms))
        ms = []
        for k in range(REPEATS + 1):
            one, fresh = timed(lambda: api.VoxelMap.from_state(ctx, state))
            fresh.close()
            if k > 0:
                ms.append(one)
        say("from_state (create, grow from 16 slots, restore): %s" % best_and_spread(ms))
        # what goes out: the outlying block alone (the box is the main body), or the last tenth of the body's layers in x too
        centre = np.array(box) / 2
        for what, layers in (("about 300", 0), ("about 10 %", int(round(box[0] / 10)))):
            kept_x = box[0] - layers  # cells 0 … kept_x - 1 stay
            center, half = centre.copy(), centre.copy()
            center[0], half[0] = kept_x / 2, kept_x / 2 - 0.25
            gone = len(vm.export(center=center, half_extent=half, removed=True)["counts"])

            def page():
                out = vm.export(center=center, half_extent=half, removed=True)
                vm.prune(center=center, half_extent=half)
                vm.add(out)

            ms = repeat(page)
            assert len(vm) == V
            say("page out / in, %-10s (%7d voxels)       : %s" % (what, gone, best_and_spread(ms)))
            ms = repeat(lambda: vm.export(center=center, half_extent=half, removed=True))
            say("  export(box, removed=True) alone              : %s" % best_and_spread(ms))
        points = (np.repeat(state["cells"], 40, axis=0) + rng.uniform(0.0, 1.0, size=(40 * V, 3)))
        ms = []
        for k in range(REPEATS + 1):
            fresh = api.VoxelMap(ctx, 1.0, 1.0, capacity=V)
            ctx.synchronize()
            one, _ = timed(lambda: fresh.insert(points))
            assert len(fresh) == V
            fresh.close()
            if k > 0:
                ms.append(one)
        say("ONE insert of 40 points per voxel (%9d)   : %s" % (len(points), best_and_spread(ms)))
        del points
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "map.npz")
            ms = repeat(lambda: vm.save(path))
            say("save (export + np.savez, %.1f MB on disk)       : %s" % (os.path.getsize(path) / 1e6, best_and_spread(ms)))
            ms = []
            for k in range(REPEATS + 1):
                one, fresh = timed(lambda: api.VoxelMap.load(ctx, path))
                fresh.close()
                if k > 0:
                    ms.append(one)
            say("load (np.load + from_state)                    : %s" % best_and_spread(ms))
        vm.close()
    ctx.close()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
