"""The streamed one-launch solve keeps `stream_reg_rounds` of every workgroup's rounds in vector registers after iteration 0
(solve_cluster_kernel, SI > 0; StreamRegRounds in csrc/assemble_one_launch.hpp), next to the `stream_lds_chunks` it keeps in
LDS.  Every lane still sums its items in the same order, so every setting must give the same bits as 0: poses, cost
histories, reports — crossed with stream_lds_chunks 0 and 3.  Covered: ndt6, ndt3 and reprojection in fp64 and fp32, just
above the resident capacity (few, uneven rounds per workgroup, where the clamp to my_rounds - 1 bites), a few million
(non-temporal loads for the larger ones) and the headline's 10 M for ndt6 fp64, reduced grids (lm_cluster_max_blocks), the
abort path, and the exact-integer datasets of tests/exact_inputs.py, whose first cost must equal the integer sum.
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
REG_MAX = 3  # the option's range; a kernel with fewer slots clamps
LDS_MAX = 3


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _resident_plus_one(planes, dtype, cus):
    return K["resident"][(planes, ES[dtype])] * 512 * min(K["cluster_max_blocks"], cus) + 1


def _streamed(ctx):
    g = X.cluster_geometry(ctx.last_kernel())
    assert g["SI"] > 0 and g["RI"] == g["LI"] == 0, ctx.last_kernel()


def _fewest_rounds(n, dtype, blocks):
    """Rounds of the workgroup of a streamed solve that has the fewest (chunks are dealt grid-stride)."""
    chunk = K["solve_block"] * K["stream_items"][ES[dtype]]
    return -(-n // chunk) // blocks


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


def _same(ctx, ds, problem, what, settings=(1, 2, 3), lds=(0, 3), launches=1, min_iterations=2):
    """The solve with every register setting, at each LDS setting, equals the solve with everything streamed, bit for bit."""
    with ctx.options(stream_reg_rounds=0, stream_lds_chunks=0):
        pose0, rep0 = _solve(ctx, ds, problem)
    if launches == 1:
        _streamed(ctx)
        assert rep0["launches"] == 1 and len(rep0["cost_history"]) >= min_iterations, (what, rep0)
    for l in lds:
        for k in ((0,) if l else ()) + tuple(settings):
            with ctx.options(stream_reg_rounds=k, stream_lds_chunks=l):
                pose, rep = _solve(ctx, ds, problem)
            assert rep["launches"] == rep0["launches"], (what, l, k)
            assert np.array_equal(_bits(pose), _bits(pose0)), (what, l, k, pose - pose0)
            assert np.array_equal(_bits(rep["cost_history"]), _bits(rep0["cost_history"])), (what, l, k)
            for key in ("iterations", "ok", "printed_cost", "last_cost", "final_lambda", "fallback"):
                assert rep[key] == rep0[key] or (rep[key] != rep[key] and rep0[key] != rep0[key]), (what, l, k, key)


def test_option_range(ctx):
    assert ctx.get_option("stream_reg_rounds") == 3
    for bad in (-1, REG_MAX + 1):
        with pytest.raises(Exception):
            ctx.set_option("stream_reg_rounds", bad)
    assert ctx.get_option("stream_reg_rounds") == 3
    for good in range(REG_MAX + 1):
        with ctx.options(stream_reg_rounds=good):
            assert ctx.get_option("stream_reg_rounds") == good


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["ndt6", "ndt3"])
def test_ndt_register_rounds_keep_the_bits(ctx, cus, problem, dtype):
    for n in (_resident_plus_one(15, dtype, cus), 3_000_017):
        ds = NdtDataset.from_planes(ctx, synth.ndt_planes(n, max(1, n // 50)), dtype)
        _same(ctx, ds, problem, "%s %s n=%d" % (problem, dtype, n))
        ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reprojection_register_rounds_keep_the_bits(ctx, cus, dtype):
    for n in (_resident_plus_one(5, dtype, cus), 8_000_009):
        ds = ReprojDataset.from_planes(ctx, synth.reproj_planes(n), dtype)
        _same(ctx, ds, "reproj", "reproj %s n=%d" % (dtype, n))
        ds.close()


def test_headline_size_uses_every_slot(ctx, cus):
    """10 M, ndt6 fp64: every workgroup has far more rounds than register slots + LDS chunks + 1, so from iteration 1 on all
    of them are really read from the chip, and the solve runs at least 3 iterations."""
    n = 10_000_000
    blocks = min(K["cluster_max_blocks"], cus)
    assert _fewest_rounds(n, "f64", blocks) >= REG_MAX + LDS_MAX + 1
    ds = NdtDataset.from_planes(ctx, synth.ndt_planes(n, n // 50), "f64")
    _same(ctx, ds, "ndt6", "headline", min_iterations=3)
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_slot_used_at_a_few_million(ctx, cus, dtype):
    """The few-million cases above give every workgroup at least slots + LDS chunks + 1 rounds (so no clamp hides a slot) and
    run at least 3 iterations.  (The fp32 6-DoF kernel has no register slot — StreamRegRounds — so there the option must
    change nothing at all.)"""
    n = 3_000_017
    blocks = min(K["cluster_max_blocks"], cus)
    assert _fewest_rounds(n, dtype, blocks) >= REG_MAX + LDS_MAX + 1, _fewest_rounds(n, dtype, blocks)
    ds = NdtDataset.from_planes(ctx, synth.ndt_planes(n, n // 50), dtype)
    _same(ctx, ds, "ndt6", "%s n=%d" % (dtype, n), settings=(3,), lds=(3,), min_iterations=3)
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_reduced_grids_and_abort_keep_the_bits(ctx, cus, dtype):
    """A grid capped below the CU count (ranks sharing a GPU) gives every workgroup more rounds, a grid of one workgroup
    all of them; a launch that gives up at once (debug_cluster_abort) falls back to one launch per iteration."""
    n = _resident_plus_one(15, dtype, cus) + 70_001
    ds = NdtDataset.from_planes(ctx, synth.ndt_planes(n, n // 50), dtype)
    for blocks in (37, 64, 1):
        with ctx.options(lm_cluster_max_blocks=blocks):
            _same(ctx, ds, "ndt6", "%s n=%d blocks=%d" % (dtype, n, blocks), settings=(1, 3))
    with ctx.options(debug_cluster_abort=1):
        with ctx.options(stream_reg_rounds=3):
            _, rep = _solve(ctx, ds, "ndt6")
        assert rep["fallback"], rep
    with ctx.options(debug_cluster_abort=1):
        _same(ctx, ds, "ndt6", "%s n=%d abort" % (dtype, n), settings=(3,), launches=None)
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exact_datasets(ctx, cus, dtype):
    """Exact-integer datasets: the first cost of the streamed solve is the integer sum, and the whole solve is the same
    with and without register rounds."""
    for n in (_resident_plus_one(15, dtype, cus), 2_000_003):
        case = X.ndt_case(n, dtype, cus=cus, seed=n % 1000 + 5)
        ds = NdtDataset.from_planes(ctx, case.planes, dtype)
        hists = []
        for l, k in ((0, 0), (0, 3), (3, 0), (3, 3), (3, 1)):
            with ctx.options(stream_reg_rounds=k, stream_lds_chunks=l):
                _, _, rep = ds.solve6(case.R, case.t, None, max_iterations=3)
                _streamed(ctx)
                assert np.asarray(rep["cost_history"])[0] == case.want6[27], (n, l, k)
                hists.append(rep["cost_history"])
        for h in hists[1:]:
            assert np.array_equal(_bits(hists[0]), _bits(h)), n
        ds.close()
    for n in (_resident_plus_one(5, dtype, cus), 4_000_037):
        case = X.reproj_case(n, dtype, cus=cus, seed=n % 1000 + 9)
        ds = ReprojDataset.from_planes(ctx, case.planes, dtype)
        hists = []
        for l, k in ((0, 0), (0, 3), (3, 0), (3, 3), (3, 1)):
            with ctx.options(stream_reg_rounds=k, stream_lds_chunks=l):
                _, _, rep = ds.solve(case.R, case.t, X.REPROJ_INTR, None, X.REPROJ_MIN_DEPTH, max_iterations=3)
                _streamed(ctx)
                assert np.asarray(rep["cost_history"])[0] == case.want[27], (n, l, k)
                hists.append(rep["cost_history"])
        for h in hists[1:]:
            assert np.array_equal(_bits(hists[0]), _bits(h)), n
        ds.close()
