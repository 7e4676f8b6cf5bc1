"""Batched LM solve (nos_ndt6_solve_batch / nos_ndt3_solve_batch / nos_reproj_solve_batch; api.solve6_batch / solve3_batch /
reproj_solve_batch): B independent pose problems, the small ones in ONE launch with one workgroup each.

A problem the batch launch takes runs the very loop of the lone single-workgroup solve (nos::single_block_loop) on the same
data, so every row must equal its lone nos_*_solve BIT FOR BIT: pose, iteration count, costs, λ and cost history.  Larger
problems run as lone solves after the launch.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers
from nonlinear_optimizer_for_slam_amd import _lib, synth
from nonlinear_optimizer_for_slam_amd.api import (Context, NdtDataset, NdtIndexedDataset, ReprojDataset, make_loss,
                                                 reproj_solve_batch, shm_unlink, solve3_batch, solve6_batch)

pytestmark = pytest.mark.gpu

EXP = ("exponential", 1.0, 1.0)
LOSSES = [None, EXP, ("huber", 0.7)]
# 1024 x 15 / 3072 x 5 plane-elements: the single-workgroup cap of the lone solve; 700 / 1000 are no multiples of 512
NDT_SIZES = (1, 37, 700, 1000, 1024)
REPROJ_SIZES = (1, 630, 1000, 3072)
B = 40
INTR = synth.REPROJ_INTR4
SCALARS = ("iterations", "ok", "printed_cost", "last_cost", "final_lambda")


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _assert_row_is_lone(R, t, rep, lone, where):
    Rl, tl, rl = lone
    assert _same(R, Rl) and _same(t, tl), (where, R, Rl, t, tl)
    for k in SCALARS:
        assert _same(rep[k], rl[k]), (where, k, rep[k], rl[k])
    assert _same(rep["cost_history"], rl["cost_history"]), (where, rep["cost_history"], rl["cost_history"])
    assert rep["launches"] == rl["launches"], (where, rep["launches"], rl["launches"])


def _datasets(ctx, problem, dtype, seed=0):
    if problem == "reproj":
        return [ReprojDataset.from_planes(ctx, synth.reproj_planes(n, seed=seed + n), dtype) for n in REPROJ_SIZES]
    return [NdtDataset.from_planes(ctx, synth.ndt_planes(n, max(1, n // 30), seed=seed + n), dtype) for n in NDT_SIZES]


def _poses(problem, count, seed):
    return synth.random_poses(count, seed=seed, planar=problem == "ndt3")


def _batch(problem, datasets, R, t, loss, **kw):
    if problem == "ndt6":
        return solve6_batch(datasets, R, t, loss, **kw)
    if problem == "ndt3":
        return solve3_batch(datasets, R, t, loss, **kw)
    return reproj_solve_batch(datasets, R, t, INTR, loss, **kw)


def _lone(problem, ds, R, t, loss, **kw):
    if problem == "ndt6":
        return ds.solve6(R, t, loss, **kw)
    if problem == "ndt3":
        return ds.solve3(R, t, loss, **kw)
    return ds.solve(R, t, INTR, loss, **kw)


@pytest.mark.parametrize("loss", LOSSES, ids=["none", "exp", "huber"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("problem", ["ndt6", "ndt3", "reproj"])
def test_every_row_equals_its_lone_solve_bit_for_bit(ctx, problem, dtype, loss):
    """B = 40 problems of 1 … cap correspondences from random start poses: each row is its lone solve, bit for bit, and the
    lone solve ran the single-workgroup form (launches == 1)."""
    sets = _datasets(ctx, problem, dtype)
    order = [sets[i % len(sets)] for i in range(B)]
    R0, t0 = _poses(problem, B, seed=17)
    R, t, reps = _batch(problem, order, R0, t0, loss, max_iterations=60)
    assert "solve_batch_kernel<" in ctx.last_kernel()
    assert R.shape == R0.shape and t.shape == t0.shape and len(reps) == B
    for i in range(B):
        lone = _lone(problem, order[i], R0[i], t0[i], loss, max_iterations=60)
        assert lone[2]["launches"] == 1
        _assert_row_is_lone(R[i], t[i], reps[i], lone, (problem, dtype, i, len(order[i])))
    assert sum(r["ok"] for r in reps) >= B // 4  # real solves, not only early failures (n = 1 is rank deficient)
    for ds in sets:
        ds.close()


def test_inputs_are_not_modified_and_the_reference_scene_converges(ctx):
    planes, intr, _, tt = helpers.reference_reprojection_scene()
    ds = ReprojDataset.from_planes(ctx, planes, "f64")
    intr4 = np.array([1.0 / intr[0], 1.0 / intr[1], intr[2], intr[3]])
    R0 = np.tile(np.eye(3), (3, 1, 1))  # [B, 3, 3] is accepted too
    t0 = np.zeros((3, 3))
    R, t, reps = reproj_solve_batch([ds] * 3, R0, t0, intr4, EXP, max_iterations=100)
    assert np.array_equal(R0, np.tile(np.eye(3), (3, 1, 1))) and not t0.any()
    for i in range(3):  # the reference's golden: `COST: 2.33228e-11, iter: 6`
        assert reps[i]["launches"] == 1 and reps[i]["iterations"] == 6 and "%.5g" % reps[i]["printed_cost"] == "2.3323e-11"
    ds.close()


def test_multi_start_one_dataset_many_start_poses(ctx):
    """The reference's 630-point reprojection scene repeated 32 times, each copy from its own start pose."""
    planes, intr, _, _ = helpers.reference_reprojection_scene()
    ds = ReprojDataset.from_planes(ctx, planes, "f64")
    intr4 = np.array([1.0 / intr[0], 1.0 / intr[1], intr[2], intr[3]])
    R0, t0 = synth.random_poses(32, seed=3, max_angle=0.2, max_translation=0.5)
    R, t, reps = reproj_solve_batch([ds] * 32, R0, t0, intr4, EXP, max_iterations=100)
    for i in range(32):
        _assert_row_is_lone(R[i], t[i], reps[i], ds.solve(R0[i], t0[i], intr4, EXP, max_iterations=100), i)
    assert len({R[i].tobytes() for i in range(32)}) > 1  # the rows really are different solves
    ds.close()


def test_problems_above_the_cap_are_solved_in_their_rows(ctx, oracle):
    small = [NdtDataset.from_planes(ctx, synth.ndt_planes(n, max(1, n // 30), seed=n), "f64") for n in (300, 1024)]
    big_planes = synth.ndt_planes(20_000, 1000)
    big = NdtDataset.from_planes(ctx, big_planes, "f64")
    order = [small[0], big, small[1], big, small[0]]
    R0, t0 = synth.random_poses(len(order), seed=11)
    R, t, reps = solve6_batch(order, R0, t0, EXP, max_iterations=60)
    for i, ds in enumerate(order):
        _assert_row_is_lone(R[i], t[i], reps[i], ds.solve6(R0[i], t0[i], EXP, max_iterations=60), i)
    # batch_max_elements raised: the 20 k problem runs in the batch launch too, one workgroup looping over its 40 chunks
    eye, zero = np.tile(np.eye(3).reshape(1, 9), (2, 1)), np.zeros((2, 3))
    with ctx.options(batch_max_elements=20_000 * 15):
        Rb, tb, rb = solve6_batch([small[0], big], eye, zero, EXP, max_iterations=100)
        assert "solve_batch_kernel<nos::Ndt6Problem<double" in ctx.last_kernel()
    assert ctx.get_option("batch_max_elements") == 1024 * 15
    want = oracle.ndt6_solve(big_planes, np.zeros(3), np.eye(3), loss=EXP, max_iterations=100, linear_solver=1)
    assert rb[1]["launches"] == 1 and rb[1]["ok"] and rb[1]["iterations"] == want["iterations"]
    assert rb[1]["printed_cost"] == pytest.approx(want["printed_cost"], rel=1e-9)
    dt, dq = helpers.pose_delta(Rb[1].reshape(3, 3), tb[1], want["R"], want["t"])
    assert dt < 1e-9 and dq < 1e-9, (dt, dq)
    for ds in small + [big]:
        ds.close()


def test_voxel_indexed_datasets_run_as_lone_solves(ctx):
    planes = synth.ndt_planes(600, 20)
    means = planes[3:6].T.copy()
    sq = planes[6:15].T.reshape(-1, 3, 3).copy()
    uniq, inv = np.unique(np.concatenate([means, sq.reshape(-1, 9)], axis=1), axis=0, return_inverse=True)
    idx = NdtIndexedDataset.from_arrays(ctx, planes[0:3].copy(), inv.reshape(1, -1).astype(np.int32), uniq[:, :3].copy(),
                                        uniq[:, 3:].reshape(-1, 3, 3).copy(), "f64")
    flat = NdtDataset.from_planes(ctx, planes, "f64")
    R0, t0 = synth.random_poses(4, seed=5)
    order = [flat, idx, flat, idx]
    R, t, reps = solve6_batch(order, R0, t0, EXP, max_iterations=40)
    for i, ds in enumerate(order):
        _assert_row_is_lone(R[i], t[i], reps[i], ds.solve6(R0[i], t0[i], EXP, max_iterations=40), i)
    idx.close()
    flat.close()


def test_two_thousand_problems_in_one_launch(ctx):
    """Far more workgroups than CUs: nothing in the kernel waits for another workgroup, the extra ones queue."""
    sets = [ReprojDataset.from_planes(ctx, synth.reproj_planes(630, seed=s), "f64") for s in range(8)]
    n = 2048
    order = [sets[i % len(sets)] for i in range(n)]
    R0, t0 = synth.random_poses(n, seed=23)
    R, t, reps = reproj_solve_batch(order, R0, t0, INTR, EXP, max_iterations=30)
    assert all(r["launches"] == 1 for r in reps) and sum(r["ok"] for r in reps) > n // 2
    assert "solve_batch_kernel<nos::ReprojProblem<double" in ctx.last_kernel()
    for i in np.random.default_rng(1).choice(n, 64, replace=False):
        _assert_row_is_lone(R[i], t[i], reps[i], order[i].solve(R0[i], t0[i], INTR, EXP, max_iterations=30), int(i))
    for ds in sets:
        ds.close()


@pytest.mark.parametrize("problem", ["ndt6", "ndt3", "reproj"])
def test_each_problem_follows_its_own_simd_class(ctx, problem):
    plain = _datasets(ctx, problem, "f32", seed=40)
    simd = [ds.set_simd_class(True) for ds in _datasets(ctx, problem, "f32", seed=40)]
    order = [x for pair in zip(plain, simd) for x in pair]
    R0, t0 = _poses(problem, len(order), seed=29)
    R0[1::2], t0[1::2] = R0[0::2], t0[0::2]  # the same start for a dataset with and without the fp32 classes' rules
    R, t, reps = _batch(problem, order, R0, t0, EXP, max_iterations=60)
    for i, ds in enumerate(order):
        _assert_row_is_lone(R[i], t[i], reps[i], _lone(problem, ds, R0[i], t0[i], EXP, max_iterations=60), i)
    if problem != "reproj":  # NDT: λ in float from the first step on, so the rule is visible in the bits
        assert any(not _same(R[2 * k], R[2 * k + 1]) for k in range(len(plain)) if reps[2 * k]["ok"])
    for ds in plain + simd:
        ds.close()


def test_max_iterations_zero_and_empty_batches(ctx):
    ds = NdtDataset.from_planes(ctx, synth.ndt_planes(500, 20), "f64")
    R0, t0 = synth.random_poses(2, seed=2)
    R, t, reps = solve6_batch([ds, ds], R0, t0, EXP, max_iterations=0)
    for i in range(2):
        _assert_row_is_lone(R[i], t[i], reps[i], ds.solve6(R0[i], t0[i], EXP, max_iterations=0), i)
    R, t, reps = solve6_batch([], np.zeros((0, 9)), np.zeros((0, 3)), EXP)
    assert R.shape == (0, 9) and t.shape == (0, 3) and reps == []
    ds.close()


def _raw(lib_fn, handles, n, R, t, *post, opt=True, reports=True):
    o = _lib.NosLmOptions(20, 0, 1e-6, 1e-6, None)
    reps = (_lib.NosLmReport * 4)()
    dp = lambda a: None if a is None else a.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    return lib_fn(handles, n, dp(R), dp(t), *post, ctypes.byref(o) if opt else None, reps if reports else None)


def test_argument_errors_are_reported_before_anything_is_written(ctx):
    lib = _lib.hip_lib()
    planes = synth.ndt_planes(500, 20)
    a = NdtDataset.from_planes(ctx, planes, "f64")
    a32 = NdtDataset.from_planes(ctx, planes, "f32")
    rp = ReprojDataset.from_planes(ctx, synth.reproj_planes(300), "f64")
    other = Context((0,))
    b = NdtDataset.from_planes(other, planes, "f64")
    two = Context((0, 0))
    c2 = NdtDataset.from_planes(two, planes, "f64")
    loss = make_loss(EXP)
    R0, t0 = synth.random_poses(2, seed=8)

    def handles(*ds):
        return (ctypes.c_void_p * len(ds))(*[d._h for d in ds])

    def expect(status, fn, hs, *post, n=2, R=True, t=True, **kw):
        R1, t1 = R0.copy(), t0.copy()
        rc = _raw(fn, hs, n, R1 if R else None, t1 if t else None, *post, **kw)
        assert rc == status, (rc, status, lib.nos_last_error())
        assert np.array_equal(R1, R0) and np.array_equal(t1, t0)  # a rejected call writes nothing

    INV, KIND, UNS = 1, 5, 6
    six = lib.nos_ndt6_solve_batch
    expect(INV, six, None, ctypes.byref(loss))
    expect(INV, six, handles(a, a), ctypes.byref(loss), R=False)
    expect(INV, six, handles(a, a), ctypes.byref(loss), t=False)
    expect(INV, six, handles(a, a), ctypes.byref(loss), opt=False)
    expect(INV, six, handles(a, a), ctypes.byref(loss), reports=False)
    expect(INV, six, handles(a, a), ctypes.byref(loss), n=-1)
    expect(INV, six, handles(a, b), ctypes.byref(loss))        # datasets of different contexts
    expect(INV, six, handles(a, a32), ctypes.byref(loss))      # mixed element types
    expect(KIND, six, handles(a, rp), ctypes.byref(loss))      # a reprojection dataset in an NDT batch
    expect(UNS, six, handles(c2, c2), ctypes.byref(loss))      # two-device context
    intr = np.tile(np.array(INTR), (2, 1))
    expect(INV, lib.nos_reproj_solve_batch, handles(rp, rp), None, ctypes.byref(loss), ctypes.c_double(0.03))
    expect(KIND, lib.nos_reproj_solve_batch, handles(rp, a), intr.ctypes.data_as(_lib.c_double_p), ctypes.byref(loss),
           ctypes.c_double(0.03))
    bad_loss = make_loss(("huber", -1.0))
    expect(INV, six, handles(a, a), ctypes.byref(bad_loss))
    assert _raw(six, None, 0, None, None, ctypes.byref(loss), opt=False, reports=False) == 0  # nothing to do: OK
    with pytest.raises(_lib.NosError) as err:
        solve3_batch([a, rp], np.tile([1.0, 0.0, 0.0, 1.0], (2, 1)), np.zeros((2, 2)), EXP)
    assert err.value.status == KIND
    # batching is process-local: a context with a communicator is refused
    name = "/nos_batch_test_%d" % os.getpid()
    with_comm = Context((0,))
    try:
        with_comm.comm_init_shm(1, 0, name)
        d = NdtDataset.from_planes(with_comm, planes, "f64")
        expect(UNS, six, handles(d, d), ctypes.byref(loss))
        d.close()
    finally:
        with_comm.close()
        shm_unlink(name)
    for ds in (a, a32, rp, b, c2):
        ds.close()
    other.close()
    two.close()
