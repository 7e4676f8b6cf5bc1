"""Voxel statistics of the GPU against the 50-digit reference (oracle/oracle_voxel_xp.py), on the input families of
tests/voxel_inputs.py: counts 4 / 5 / 63 / 64 / 65 / 1000, exact and near ties of eigenvalues on both sides of the tie rule,
rotations that straddle the Jacobi sweep's off-diagonal skip, slabs at the eigenvalue floor, slivers at the validity
threshold — each at cell offsets 0, ±2^10, ±2^15, ±2^19, 2^20 − 1 and −2^20, on 1 m, 0.5 m and 0.3 m grids, through every
path a voxel's numbers can take: the one-shot build with compact and with packed sort keys, the store's insert in one
batch, in three batches that split every voxel (the merge), insert_scan (the warp) and the compaction copy of a prune.

Bounds (voxel_inputs.compare): cells, counts and validity equal; mean within 2 ulp of the voxel's largest coordinate;
floored eigenvalues within 1e-11; information matrix within 1e-10 (+ the true gap of a pair the tie rule merges).  With
sums of raw p and p pᵀ, as the harness has them, the information matrix was off by 3e-8 at 2^10 cells, 2.5e-4 at 2^15 and
4e-2 at 2^19, and validity flipped from 2^15 on (profiles/voxel_stats_accuracy.txt); the sums are taken about the cell
corner (csrc/voxel_finish.hpp), and the measured maxima are 0.5 ulp, 8e-14 and 1.8e-13 at every offset."""
import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import api
from tests import voxel_inputs as VI

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("proper", [True, False], ids=["proper", "harness_formula"])
@pytest.mark.parametrize("path", VI.PATHS)
@pytest.mark.parametrize("key", list(VI.CLOUDS))
def test_voxel_statistics_meet_the_extended_precision_bounds(ctx, key, path, proper):
    c = VI.cloud(*VI.CLOUDS[key])
    got = VI.run_path(api, ctx, c, path, proper)
    assert len(got["counts"]) == len(c.voxels)  # nothing else is there (the voxel a prune removed included)
    worst = VI.compare(c, VI.reference(c), got, proper, "%s, %s" % (key, path))
    print("%s %s %s: worst mean %.2f ulp, eigenvalues %.1e, information %.1e" %
          (key, path, "proper" if proper else "harness", max(w[0] for w in worst.values()),
           max(w[1] for w in worst.values()), max(w[2] for w in worst.values())))


@pytest.mark.parametrize("proper", [True, False], ids=["proper", "harness_formula"])
@pytest.mark.parametrize("key", list(VI.CLOUDS))
def test_build_and_one_batch_insert_are_bit_identical_on_this_cloud(ctx, key, proper):
    """Same sort order, same sums kernel, same finish: the one-shot build and one insert into an empty store agree bit for
    bit, voxel by voxel in ascending cell order — far from the origin as near it."""
    c = VI.cloud(*VI.CLOUDS[key])
    a = VI.run_path(api, ctx, c, "build_compact_keys", proper)
    b = VI.run_path(api, ctx, c, "insert_one_batch", proper)
    for k in ("cells", "counts", "valid", "means", "sqrt_infos"):
        assert np.array_equal(a[k], b[k]), k
