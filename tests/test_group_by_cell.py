"""Grouping points by cell and voxels by matcher cell (csrc/group_host.hpp) against numpy.

The map build, the scan sort, the voxel store's insert and the matcher's tables share one host-side sequence — keys,
stable radix sort, run-length encoding, scan over the runs.  Each is checked here against numpy alone, not against another
route of the library: the distinct cells in lexicographic order, their counts, the stable permutation of the points by
cell.  Points sit at cell + 0.5 and the resolution is 1.0, so floor() is exact and every comparison is integer equality.
Sizes: 1, 2; 255 / 256 / 257, the edges of the 256-thread grids; one run and as many runs as points; 1024·256 + 1, the
first size at which voxel_box_kernel's capped grid strides."""
import functools

import numpy as np
import pytest

CASES = ("n1", "n2", "n255", "n256", "n257", "one_cell", "own_cells", "n262145")


@functools.lru_cache(maxsize=None)
def case(name):
    """→ (points [n,3], distinct cells in lexicographic order, their counts, stable permutation of the points by cell)."""
    rng = np.random.default_rng(20261018)
    if name == "one_cell":
        cells = np.tile(np.array([-2, 3, 0], dtype=np.int64), (1000, 1))
    elif name == "own_cells":
        g = np.arange(10, dtype=np.int64) - 4  # a 10 x 10 x 10 block around the origin, every cell once, shuffled
        cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        cells = cells[rng.permutation(1000)]
    else:
        n = int(name[1:])
        cells = rng.integers([-5, -3, -2], [12, 9, 4], size=(n, 3), dtype=np.int64)
    points = cells.astype(np.float64) + 0.5
    floored = np.floor(points).astype(np.int64)
    distinct, inverse, counts = np.unique(floored, axis=0, return_inverse=True, return_counts=True)
    order = np.argsort(inverse.reshape(-1), kind="stable")
    for a in (points, distinct, counts, order):
        a.setflags(write=False)
    return points, distinct, counts, order


@pytest.mark.parametrize("name", CASES)
def test_the_numpy_reference_is_sound(name):
    points, distinct, counts, order = case(name)
    n = points.shape[0]
    assert np.array_equal(np.floor(points), points - 0.5)
    assert np.array_equal(np.sort(order), np.arange(n))  # a permutation
    assert counts.sum() == n and len(counts) == len(distinct) and np.all(counts > 0)
    assert np.all(np.lexsort((distinct[:, 2], distinct[:, 1], distinct[:, 0])) == np.arange(len(distinct)))
    sorted_cells = np.floor(points[order]).astype(np.int64)
    assert np.array_equal(sorted_cells, np.repeat(distinct, counts, axis=0))  # grouped, groups in order
    for lo, c in zip(np.cumsum(counts) - counts, counts):  # stable: original order inside a group
        assert np.all(np.diff(order[lo:lo + c]) > 0)
    if name in ("n257", "n262145"):
        assert np.any(distinct < 0)
    assert {"one_cell": 1, "own_cells": n}.get(name, len(distinct)) == len(distinct)


@pytest.mark.gpu
@pytest.mark.parametrize("compact", (1, 0))
@pytest.mark.parametrize("name", CASES)
def test_map_build_lists_numpys_cells_and_counts(ctx, name, compact):
    from nonlinear_optimizer_for_slam_amd import api
    points, distinct, counts, _ = case(name)
    with ctx.options(map_compact_keys=compact):
        gm, st = api.NdtMap.build(ctx, points, 1.0, 1.0)
    gm.close()
    assert st["cells"].dtype == np.int64 and np.array_equal(st["cells"], distinct)
    assert np.array_equal(st["counts"].astype(np.int64), counts)


@pytest.mark.gpu
@pytest.mark.parametrize("compact", (1, 0))
@pytest.mark.parametrize("name", CASES)
def test_scan_sort_gives_numpys_stable_permutation(ctx, name, compact):
    from nonlinear_optimizer_for_slam_amd import api
    points, _, _, order = case(name)
    with ctx.options(map_compact_keys=compact):
        sc = api.Scan(ctx, points, sort_cell=1.0)
    got = np.asarray(sc.order).astype(np.int64)
    sc.close()
    assert np.array_equal(got, order)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_store_insert_touches_numpys_cells(ctx, name):
    from nonlinear_optimizer_for_slam_amd import api
    points, distinct, counts, _ = case(name)
    vm = api.VoxelMap(ctx, 1.0, 1.0)
    n_touched = vm.insert(points)
    st = vm.stats()
    n_voxels = len(vm)
    vm.close()
    assert n_touched == len(distinct) and n_voxels == len(distinct)
    by_cell = np.lexsort((st["cells"][:, 2], st["cells"][:, 1], st["cells"][:, 0]))
    assert np.array_equal(st["cells"][by_cell], distinct)
    assert np.array_equal(st["counts"][by_cell].astype(np.int64), counts)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("all_valid", "some_invalid", "all_invalid"))
@pytest.mark.parametrize("V", (1, 256, 257))
def test_map_tables_keep_the_valid_voxels(ctx, V, which):
    """The matcher's tables from V voxels: the invalid ones form the last run of the sort and are left out; all V invalid
    leaves an empty map."""
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(20261019 + V)
    means = rng.integers(-6, 7, size=(V, 3)).astype(np.float64) + 0.5
    S = np.tile(np.eye(3), (V, 1, 1))
    valid = {"all_valid": np.ones(V, dtype=bool), "some_invalid": rng.random(V) < 0.5, "all_invalid": np.zeros(V, dtype=bool)}[which]
    if which == "some_invalid":
        valid[0] = False  # at least one goes, V = 1 included
    gm = api.NdtMap(ctx, means, S, valid, 1.0)
    n = len(gm)
    gm.close()
    assert n == int(valid.sum())
