"""The streamed one-launch solve keeps `stream_lds_chunks` of every workgroup's chunks in LDS after iteration 0
(solve_cluster_kernel, SI > 0).  Every lane still sums its items in the same order, so each setting of the option must
give the same bits as 0 (everything streamed every iteration): poses, cost histories, reports.  Covered: ndt6, ndt3 and
reprojection in fp64 and fp32, just above the resident capacity (few chunks per workgroup, uneven counts) and at a few
million (non-temporal loads for the larger ones), reduced grids (lm_cluster_max_blocks), the abort path, and the
exact-integer datasets of tests/exact_inputs.py, whose first cost must equal the integer sum.
"""
import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import NdtDataset, ReprojDataset, synth
from tests import exact_inputs as X

pytestmark = pytest.mark.gpu

ES = {"f64": 8, "f32": 4}
K = X.library_constants()
EXP = ("exponential", 1.0, 1.0)
HUBER = ("huber", synth.REPROJ_HUBER_THRESHOLD)
R0 = np.array([[np.cos(0.02), -np.sin(0.02), 0.0], [np.sin(0.02), np.cos(0.02), 0.0], [0.0, 0.0, 1.0]])
T0 = np.array([0.05, -0.03, 0.02])


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _resident_plus_one(planes, dtype, cus):
    return K["resident"][(planes, ES[dtype])] * 512 * min(K["cluster_max_blocks"], cus) + 1


def _streamed(ctx):
    g = X.cluster_geometry(ctx.last_kernel())
    assert g["SI"] > 0 and g["RI"] == g["LI"] == 0, ctx.last_kernel()


def _solve(ctx, ds, problem, iters=8):
    if problem == "ndt6":
        R, t, rep = ds.solve6(R0, T0, EXP, max_iterations=iters)
    elif problem == "ndt3":
        R, t, rep = ds.solve3(R0[:2, :2].copy(), T0[:2].copy(), EXP, max_iterations=iters)
    else:
        R, t, rep = ds.solve(R0, T0, synth.REPROJ_INTR4, HUBER, max_iterations=iters)
    return np.concatenate([np.ravel(R), np.ravel(t)]), rep


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _same(ctx, ds, problem, what, settings=(1, 2, 3), launches=1):
    """The solve with every LDS setting equals the solve with everything streamed, bit for bit."""
    with ctx.options(stream_lds_chunks=0):
        pose0, rep0 = _solve(ctx, ds, problem)
    if launches == 1:
        _streamed(ctx)
        assert rep0["launches"] == 1 and len(rep0["cost_history"]) >= 2, (what, rep0)
    for k in settings:
        with ctx.options(stream_lds_chunks=k):
            pose, rep = _solve(ctx, ds, problem)
        assert rep["launches"] == rep0["launches"], (what, k)
        assert np.array_equal(_bits(pose), _bits(pose0)), (what, k, pose - pose0)
        assert np.array_equal(_bits(rep["cost_history"]), _bits(rep0["cost_history"])), (what, k)
        for key in ("iterations", "ok", "printed_cost", "last_cost", "final_lambda", "fallback"):
            assert rep[key] == rep0[key] or (rep[key] != rep[key] and rep0[key] != rep0[key]), (what, k, key)


def test_option_range(ctx):
    assert ctx.get_option("stream_lds_chunks") == 3
    for bad in (-1, 4):
        with pytest.raises(Exception):
            ctx.set_option("stream_lds_chunks", bad)
    assert ctx.get_option("stream_lds_chunks") == 3


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["ndt6", "ndt3"])
def test_ndt_lds_chunks_keep_the_bits(ctx, cus, problem, dtype):
    for n in (_resident_plus_one(15, dtype, cus), 3_000_017):
        ds = NdtDataset.from_planes(ctx, synth.ndt_planes(n, max(1, n // 50)), dtype)
        _same(ctx, ds, problem, "%s %s n=%d" % (problem, dtype, n))
        ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reprojection_lds_chunks_keep_the_bits(ctx, cus, dtype):
    for n in (_resident_plus_one(5, dtype, cus), 8_000_009):
        ds = ReprojDataset.from_planes(ctx, synth.reproj_planes(n), dtype)
        _same(ctx, ds, "reproj", "reproj %s n=%d" % (dtype, n))
        ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reduced_grids_and_abort_keep_the_bits(ctx, cus, dtype):
    """A grid capped below the CU count (ranks sharing a GPU) gives every workgroup more chunks, a grid of one workgroup
    all of them; a launch that gives up at once (debug_cluster_abort) falls back to one launch per iteration."""
    n = _resident_plus_one(15, dtype, cus) + 70_001
    ds = NdtDataset.from_planes(ctx, synth.ndt_planes(n, n // 50), dtype)
    for blocks in (37, 64, 1):
        with ctx.options(lm_cluster_max_blocks=blocks):
            _same(ctx, ds, "ndt6", "%s n=%d blocks=%d" % (dtype, n, blocks), settings=(3,))
    with ctx.options(debug_cluster_abort=1):
        with ctx.options(stream_lds_chunks=3):
            _, rep = _solve(ctx, ds, "ndt6")
        assert rep["fallback"], rep
    with ctx.options(debug_cluster_abort=1):
        _same(ctx, ds, "ndt6", "%s n=%d abort" % (dtype, n), settings=(3,), launches=None)
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exact_datasets(ctx, cus, dtype):
    """Exact-integer datasets: the first cost of the streamed solve is the integer sum, and the whole solve is the same
    with and without LDS chunks."""
    for n in (_resident_plus_one(15, dtype, cus), 2_000_003):
        case = X.ndt_case(n, dtype, cus=cus, seed=n % 1000 + 5)
        ds = NdtDataset.from_planes(ctx, case.planes, dtype)
        hists = []
        for k in (0, 3):
            with ctx.options(stream_lds_chunks=k):
                _, _, rep = ds.solve6(case.R, case.t, None, max_iterations=3)
                _streamed(ctx)
                assert np.asarray(rep["cost_history"])[0] == case.want6[27], (n, k)
                hists.append(rep["cost_history"])
        assert np.array_equal(_bits(hists[0]), _bits(hists[1])), n
        ds.close()
    for n in (_resident_plus_one(5, dtype, cus), 4_000_037):
        case = X.reproj_case(n, dtype, cus=cus, seed=n % 1000 + 9)
        ds = ReprojDataset.from_planes(ctx, case.planes, dtype)
        hists = []
        for k in (0, 3):
            with ctx.options(stream_lds_chunks=k):
                _, _, rep = ds.solve(case.R, case.t, X.REPROJ_INTR, None, X.REPROJ_MIN_DEPTH, max_iterations=3)
                _streamed(ctx)
                assert np.asarray(rep["cost_history"])[0] == case.want[27], (n, k)
                hists.append(rep["cost_history"])
        assert np.array_equal(_bits(hists[0]), _bits(hists[1])), n
        ds.close()
