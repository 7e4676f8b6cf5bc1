"""pipeline.TileCache, the host-side cache of paged-out voxels, and the file format's version check — no GPU.

The cache's grouping is a plain function over arrays (pipeline.combine_cells, pipeline.tiles_of_cells), so it is tested on
arrays: a state put and taken back is the same set of voxels, a cell put twice comes back once with counts and sums added
in arrival order, a box takes exactly the tiles that meet it, negative cells land in the tile floor() puts them in."""
import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import pipeline


def _state(cells, seed=0, epoch=7, res=0.5):
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    n = cells.shape[0]
    return {"cells": cells, "counts": rng.integers(1, 50, size=n).astype(np.uint32), "sums": rng.normal(size=(n, 9)),
            "stamps": rng.integers(0, epoch + 1, size=n).astype(np.uint32), "epoch": epoch, "voxel_resolution": res,
            "search_radius_sq": 1.0, "proper_sqrt_information": True}


def _by_cell(state):
    order = np.lexsort(state["cells"].T[::-1])
    return {k: state[k][order] for k in ("cells", "counts", "sums", "stamps")}


def _same_voxels(a, b):
    a, b = _by_cell(a), _by_cell(b)
    for k in ("cells", "counts", "sums", "stamps"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def _distinct_cells(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return rng.permutation(np.unique(rng.integers(lo, hi, size=(n, 3)), axis=0))


def test_put_then_take_of_everything_returns_the_same_voxels():
    st = _state(_distinct_cells(700, -50, 50, 1))
    cache = pipeline.TileCache()
    assert len(cache) == 0 and cache.put(st) == len(st["counts"])
    assert len(cache) == len(st["counts"])
    back = cache.take((-10 ** 6,) * 3, (10 ** 6,) * 3)
    assert len(cache) == 0
    _same_voxels(back, st)
    assert back["epoch"] == 7 and back["voxel_resolution"] == 0.5 and back["search_radius_sq"] == 1.0
    assert back["proper_sqrt_information"] is True
    assert len(cache.take_all()["counts"]) == 0  # taken is gone


def test_a_cell_put_twice_comes_back_once_with_counts_and_sums_added_in_arrival_order():
    cells = _distinct_cells(300, -20, 20, 2)
    a, b, c = _state(cells, 3, epoch=4), _state(cells[::3], 4, epoch=9), _state(cells[::6], 5, epoch=6)
    for s in (a, b, c):  # magnitudes that make the order of the additions visible in the last bits
        s["sums"] *= 10.0 ** np.random.default_rng(6).integers(-8, 9, size=s["sums"].shape)
    cache = pipeline.TileCache(tile_cells=8)
    for s in (a, b, c):
        cache.put(s)
    assert len(cache) == cells.shape[0]
    back = _by_cell(cache.take_all())
    want = {tuple(cell): [int(n), s.copy(), int(t)] for cell, n, s, t in zip(a["cells"], a["counts"], a["sums"], a["stamps"])}
    for later in (b, c):
        for cell, n, s, t in zip(later["cells"], later["counts"], later["sums"], later["stamps"]):
            w = want[tuple(cell)]
            w[0], w[1], w[2] = w[0] + int(n), w[1] + s, int(t)  # (a + b) + c, the later stamp
    assert back["cells"].shape[0] == len(want)
    for cell, n, s, t in zip(back["cells"], back["counts"], back["sums"], back["stamps"]):
        w = want[tuple(cell)]
        assert int(n) == w[0] and s.tobytes() == w[1].tobytes() and int(t) == w[2], cell
    # the same within ONE state: combine_cells on arrays that name a cell three times
    rep = np.concatenate([cells[:5], cells[:5], cells[:5]])
    sums = np.random.default_rng(7).normal(size=(15, 9)) * 10.0 ** np.arange(15)[:, None]
    u, n, s, t = pipeline.combine_cells(rep, np.arange(1, 16), sums, np.arange(15))
    order = np.lexsort(cells[:5].T[::-1])
    assert np.array_equal(u, cells[:5][order])
    assert np.array_equal(n, (np.arange(1, 6) + np.arange(6, 11) + np.arange(11, 16))[order])
    assert s.tobytes() == ((sums[:5] + sums[5:10]) + sums[10:])[order].tobytes()
    assert np.array_equal(t, np.arange(10, 15)[order])
    with pytest.raises(OverflowError):
        pipeline.combine_cells(rep[[0, 5]], [0xFFFFFFFF, 1], sums[:2], [0, 0])


def test_take_of_a_box_returns_exactly_the_tiles_that_meet_it_and_leaves_the_rest():
    T = 16
    st = _state(_distinct_cells(3000, -70, 70, 8))
    tiles = np.floor_divide(st["cells"], T)
    for lo, hi in (((-5, 0, 3), (20, 15, 3)), ((-70, -70, -70), (-49, 69, 69)), ((16, 16, 16), (16, 16, 16)), ((200, 0, 0), (300, 5, 5))):
        cache = pipeline.TileCache(tile_cells=T)
        cache.put(st)
        tlo, thi = np.floor_divide(np.array(lo), T), np.floor_divide(np.array(hi), T)
        hit = np.all((tiles >= tlo) & (tiles <= thi), axis=1)
        got = cache.take(lo, hi)
        _same_voxels(got, {k: st[k][hit] for k in ("cells", "counts", "sums", "stamps")})
        assert len(cache) == int((~hit).sum())
        _same_voxels(cache.take_all(), {k: st[k][~hit] for k in ("cells", "counts", "sums", "stamps")})


def test_negative_cells_land_in_the_tile_floor_gives():
    assert np.array_equal(pipeline.tiles_of_cells([[-1, 0, 15], [-16, -17, 16], [-32, 31, -33]], 16),
                          [[-1, 0, 0], [-1, -2, 1], [-2, 1, -3]])
    cache = pipeline.TileCache(tile_cells=16)
    cache.put(_state([[-1, -1, -1], [0, 0, 0], [-16, -16, -16], [-17, 0, 0]]))
    got = cache.take((-16, -16, -16), (-1, -1, -1))  # tile (-1, -1, -1) alone: truncation would have put (-1, -1, -1) into tile 0
    assert sorted(map(tuple, got["cells"])) == [(-16, -16, -16), (-1, -1, -1)]
    assert sorted(map(tuple, cache.take((0, 0, 0), (0, 0, 0))["cells"])) == [(0, 0, 0)]
    assert sorted(map(tuple, cache.take_all()["cells"])) == [(-17, 0, 0)]


def test_a_state_of_another_resolution_is_refused():
    cache = pipeline.TileCache()
    cache.put(_state([[1, 2, 3]], res=0.5))
    with pytest.raises(ValueError):
        cache.put(_state([[4, 5, 6]], res=0.25))
    with pytest.raises(ValueError):
        pipeline.TileCache(tile_cells=0)


def test_load_of_a_file_with_an_unknown_format_version_raises_before_any_store_is_created(tmp_path):
    from nonlinear_optimizer_for_slam_amd import api

    class NoContext:  # any use of it would raise AttributeError, not ValueError
        pass

    st = _state([[1, 2, 3], [4, 5, 6]])
    for name, version in (("future.npz", {"format_version": np.int64(api.VoxelMap.STATE_FORMAT_VERSION + 1)}), ("none.npz", {})):
        path = tmp_path / name
        with open(path, "wb") as f:
            np.savez(f, cells=st["cells"], counts=st["counts"], sums=st["sums"], stamps=st["stamps"], epoch=np.uint64(3),
                     voxel_resolution=np.float64(0.5), search_radius_sq=np.float64(1.0), proper_sqrt_information=np.bool_(True), **version)
        with pytest.raises(ValueError, match="format_version"):
            api.VoxelMap.load(NoContext(), path)
    path = tmp_path / "places.npz"
    with open(path, "wb") as f:
        np.savez(f, format_version=np.int64(99), n_rings=np.int64(2), n_sectors=np.int64(3), max_range=np.float64(80.0),
                 z_floor=np.float64(-2.0), descriptors=np.zeros((1, 2, 3)))
    with pytest.raises(ValueError, match="format_version"):
        api.PlaceDatabase.load(NoContext(), path)
