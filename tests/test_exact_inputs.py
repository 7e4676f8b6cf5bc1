"""CPU self-check of tests/exact_inputs.py: the fp64 C oracle and the numpy restatement reproduce the integer sums bit for
bit, so the construction and its magnitude budget are exact in fp64 without a GPU; and the library constants the GPU
tests derive their boundaries from are found in the sources."""
import numpy as np
import pytest

from oracle import oracle_np
from tests import exact_inputs as X


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [0, 1, 2, 65, 1025, 100_000])
def test_oracles_reproduce_the_integer_sums(oracle, n, dtype):
    case = X.ndt_case(n, dtype, seed=n + 5)
    assert np.all(case.want6 == np.round(case.want6)) and np.all(case.want3 == np.round(case.want3))
    for loss in (None, case.huber):
        np.testing.assert_array_equal(oracle.ndt6_accumulate(case.planes, case.R, case.t, loss), case.want6)
        np.testing.assert_array_equal(oracle_np.ndt6_accumulate(case.planes, case.R, case.t, loss), case.want6)
        np.testing.assert_array_equal(oracle.ndt3_accumulate(case.planes, case.R2, case.t2, loss), case.want3)
        np.testing.assert_array_equal(oracle_np.ndt3_accumulate(case.planes, case.R2, case.t2, loss), case.want3)
    rp = X.reproj_case(n, dtype, seed=n + 5)
    for loss in (None, rp.huber):
        args = (rp.planes, rp.R, rp.t, X.REPROJ_INTR, loss, X.REPROJ_MIN_DEPTH)
        np.testing.assert_array_equal(oracle.reproj_accumulate(*args), rp.want)
        np.testing.assert_array_equal(oracle_np.reproj_accumulate(*args), rp.want)
    if n:
        # the all-inlier Huber loss is the identity: w = 1, rho = s, a threshold the element type holds exactly
        assert float(np.float32(case.huber[1])) == case.huber[1] and float(np.float32(rp.huber[1])) == rp.huber[1]


def test_every_item_counts_and_the_budget_holds_at_the_largest_sizes():
    """A dropped item and a duplicated one change the sums (items differ); the budget assertion allows 80 M in fp32."""
    case = X.ndt_case(4096, "f32", seed=3)
    planes = case.planes
    dropped = X.ndt_sums_of_planes(planes[:, 1:], case.R, case.t, case.R2, case.t2, "f32")
    doubled = X.ndt_sums_of_planes(np.concatenate([planes, planes[:, 7:8]], axis=1)[:, 1:], case.R, case.t, case.R2,
                                   case.t2, "f32")
    assert not np.array_equal(dropped[0], case.want6) and not np.array_equal(doubled[0], case.want6)
    np.testing.assert_array_equal(X.ndt_sums_of_planes(planes, case.R, case.t, case.R2, case.t2, "f32")[0], case.want6)
    for dtype in ("f32", "f64"):
        L = X.choose_amplitude(80_000_000, dtype, 256, X._ndt_bound)
        assert L >= 1 and (dtype == "f64" or X._ndt_bound(L) * X.lane_budget(80_000_000, 256) < X.F32_LIMIT)
    with pytest.raises(AssertionError):  # an amplitude beyond the budget is refused, not silently inexact
        X.ndt_case(70_000, "f32", cus=1, amplitude=16)


def test_library_constants_are_found_in_the_sources():
    K = X.library_constants()
    assert K["single_block_max_elements"] % 15 == 0 and K["single_block_max_elements"] % 5 == 0
    assert K["max_partial_rows"] > 0 and K["cluster_max_blocks"] > 0
    assert set(K["resident"]) == {(15, 8), (15, 4), (5, 8), (5, 4)} and min(K["resident"].values()) >= 1
    g64 = X.assemble_geometry("assemble_kernel<nos::Ndt6Problem<double, 1>, double, 1, 512, 3, true, 0>(nos::TiledLayout)")
    g32 = X.assemble_geometry("assemble_kernel<nos::Ndt6Problem<float, 2>, float, 2, 512, 2, false, 0>(nos::TiledLayout)")
    gpp = X.assemble_geometry("assemble_kernel<nos::ReprojProblem<double, 2>, double, 1, 512, 3, false, 3>(nos::T)")
    for g in (g64, g32, gpp):  # every default geometry is in the launch table
        assert X.pass_items_per_lane(10_000_000, g, K, 256) >= 1
    # the per-pass grid rule: min(chunks, bpc · CUs, kMaxPartialRows) workgroups, chunks grid-strided
    assert X.pass_items_per_lane(80_000_000, g32, K, 256) == -(-(-(-80_000_000 // 1024)) // 256) * 2 == 612
    assert X.pass_items_per_lane(10_000_000, g32, K, 256) == 78
    # the solve forms: single workgroup up to the limit (⌈n / 512⌉ per lane), resident to RI + LI, streamed beyond
    single = K["single_block_max_elements"] // 5
    assert X.solve_items_per_lane(single, 5, 4, K, 256) == ("single", -(-single // K["solve_block"]))
    assert X.lane_budget(single, 256, 5, "f32") >= -(-single // K["solve_block"])
    cap = K["resident"][(15, 4)] * K["solve_block"] * 256
    assert X.solve_items_per_lane(cap, 15, 4, K, 256) == ("resident", K["resident"][(15, 4)])
    assert X.solve_items_per_lane(cap + 1, 15, 4, K, 256)[0] == "streamed"
    c = X.cluster_geometry("solve_cluster_kernel<nos::Ndt6Problem<float, 1>, float, 512, 0, 0, 2, false, true>(x)")
    assert (c["RI"], c["LI"], c["SI"]) == (0, 0, 2)


def test_the_poses_survive_the_quaternion_round_trip_of_the_solve(oracle):
    """solve6 / reprojection solve start from R → q → R (LmInit6): the 3-D poses are the tetrahedral group's signed
    permutations, which come back bit for bit."""
    seen = set()
    for seed in range(200):
        R = X.signed_permutation(seed).astype(np.float64)
        seen.add(R.tobytes())
        np.testing.assert_array_equal(oracle.quat_to_matrix(oracle.quat_from_matrix(R.reshape(-1))).reshape(3, 3), R)
    assert len(seen) == 11  # the tetrahedral group without the identity
    quarter = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert not np.array_equal(oracle.quat_to_matrix(oracle.quat_from_matrix(quarter.reshape(-1))).reshape(3, 3), quarter)
