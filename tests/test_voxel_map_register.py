"""Batched scan-to-map registration against the LIVE voxel store (nos_voxel_map_register6_batch / _register3_batch;
api.register6_batch / register3_batch and pipeline.scan_to_map_batch given an api.VoxelMap; pipeline.odometry(one_launch=True);
DESIGN.md §16).

The truth is the snapshot route on the same store — snapshot() followed by the same batched call on the NdtMap — which
tests/test_register_batch.py pins to the lone scan_to_map: every row must equal it BIT FOR BIT at any scan size (poses by
np.array_equal, reports field by field with the floats compared by their bytes, which is == made safe for a NaN cost).
Both sides run the same rounds on the device, so no stopping threshold can separate them.  Where a row is compared with a
lone pipeline.scan_to_map (whose stopping test is numpy's), the lone runs are checked to keep both stopping quantities off
1e-5 by the margin tests/test_register_batch.py uses.

Stores are small on purpose: a wavy surface of 12 x 12 cell edges, 250 … 450 voxels, built by inserts that force growth
from 16 slots and a prune that removes a far patch (slots renumbered, table rebuilt), at (resolution, radius^2) =
(1, 1), (0.5, 1) — the ball covers 2 r / resolution = 4 edges, so a point visits 5 cells per axis (6 within the guard band
of a face; 2 r / resolution + 2 = 6 is the figure the span limit tests): the second 3 x 3 probe block is partial —, (2, 1)
and (1, 0.25).  _guard_holds asserts the
precondition of the live matcher (every valid mean inside its cell widened by resolution / 1024) for every store compared.

Not reachable from a test: NOS_ERR_HIP for a store an earlier failure left undefined, and the probe-error return (the
table is at most half full); NOS_ERR_UNSUPPORTED for a multi-device context (a store cannot be created on one)."""
import ctypes
import os
import struct

import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import helpers

EXP = ("exponential", 1.0, 1.0)
LOSSES = [None, EXP, ("huber", 0.7)]
GRID = [(1.0, 1.0), (0.5, 1.0), (2.0, 1.0), (1.0, 0.25)]
SIZES = (1, 63, 512, 513, 1500)
GUARD = 1.0 / 1024.0  # of a voxel edge
MARGIN = 1e-4
INVALID, HIP, UNSUPPORTED = 1, 3, 6


def _guard_holds(vm, res):
    st = vm.stats()
    ok = st["valid"]
    if not ok.any():
        return
    lo = st["cells"][ok] * res
    m = st["means"][ok]
    outside = np.maximum(np.maximum(lo - m, m - (lo + res)), 0.0).max()
    assert np.all(m >= lo - GUARD * res) and np.all(m <= lo + res + GUARD * res), outside


def _surface(rng, n, res, shift=(0.0, 0.0)):
    """n points of a wavy sheet over 12 x 12 cell edges (heights within one cell edge), 2 % of an edge of noise"""
    xy = rng.uniform(-6.0, 6.0, size=(n, 2)) * res + np.asarray(shift) * res
    z = res * (0.45 * np.sin(xy[:, 0] / res * 0.9) + 0.35 * np.cos(xy[:, 1] / res * 0.7)) + rng.normal(scale=0.02 * res, size=n)
    return np.column_stack([xy, z])


def _build_store(ctx, res, r2, seed=307):
    """Several inserts, growth from 16 slots, a prune that removes a patch: what a store looks like in use."""
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(seed)
    vm = api.VoxelMap(ctx, res, r2, capacity=0)
    assert vm.memory()["capacity"] == 16
    vm.insert(_surface(rng, 6000, res))
    assert vm.memory()["generation"] >= 1 and vm.memory()["capacity"] > 16  # grown
    vm.insert(_surface(rng, 3000, res, shift=(40.0, 0.0)))  # a far patch, inserted BEFORE part of the near one
    vm.insert(_surface(rng, 6000, res, shift=(1.0, -1.0)))
    before, gen = len(vm), vm.memory()["generation"]
    assert vm.prune(center=(0.0, 0.0, 0.0), half_extent=(8.0 * res, 8.0 * res, 3.0 * res)) > 50  # the far patch goes
    assert len(vm) < before and vm.memory()["generation"] == gen + 1  # slots renumbered, table rebuilt
    vm.insert(_surface(rng, 3000, res))
    assert 150 <= len(vm) <= 600 and vm.n_valid > 100, (len(vm), vm.n_valid)
    return vm


def _make_scans(ctx, res, seed=311):
    """Scans of 1 … 1 500 points of the surface seen from a sensor pose near the identity; the 512-point one is used three
    more times from other start poses (multi-start).  → (Scans to close, batch, R0 [B, 9], t0 [B, 3])"""
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(seed)
    Rt, tt = helpers.rot_xyz(0.01, -0.015, 0.03), np.array([0.08, -0.05, 0.03]) * res
    scans = []
    for n in SIZES:
        world = _surface(rng, n, res) * np.array([0.8, 0.8, 1.0])
        scans.append(api.Scan(ctx, (Rt.T @ (world - tt).T).T))
    batch = list(scans) + [scans[2]] * 3
    R0 = [np.eye(3)] * len(scans) + [helpers.rot_xyz(*rng.uniform(-0.03, 0.03, size=3)) for _ in range(3)]
    t0 = [np.zeros(3)] * len(scans) + [rng.uniform(-0.15, 0.15, size=3) * res for _ in range(3)]
    return scans, batch, np.array([R.reshape(9) for R in R0]), np.array(t0)


@pytest.fixture(scope="module")
def stores(ctx):
    """(resolution, radius^2) → (store, its snapshot, scans, batch, R0, t0): built once, only read by the tests that share it"""
    made = {}

    def get(res, r2):
        if (res, r2) not in made:
            vm = _build_store(ctx, res, r2)
            _guard_holds(vm, res)
            made[(res, r2)] = (vm, vm.snapshot()) + _make_scans(ctx, res)
        return made[(res, r2)]

    yield get
    for vm, snap, scans, _, _, _ in made.values():
        for h in scans + [snap, vm]:
            h.close()


def _bits(x):
    return struct.pack("<d", x) if isinstance(x, float) else x


def _same_reports(got, want, where=None):
    assert len(got) == len(want), where
    for i, (a, b) in enumerate(zip(got, want)):
        assert a["outer_iter"] == b["outer_iter"] and a["ok"] == b["ok"] and len(a["rounds"]) == len(b["rounds"]), (where, i, a, b)
        for ra, rb in zip(a["rounds"], b["rounds"]):
            assert set(ra) == set(rb) == {"matches", "used", "iterations", "ok", "printed_cost", "last_cost"}
            assert {k: _bits(v) for k, v in ra.items()} == {k: _bits(v) for k, v in rb.items()}, (where, i, ra, rb)


def _same_call(a, b, where=None):
    (Ra, ta, ra), (Rb, tb, rb) = a, b
    assert np.array_equal(Ra, Rb) and np.array_equal(ta, tb), (where, np.argwhere(Ra != Rb), np.argwhere(ta != tb))
    _same_reports(ra, rb, where)


def _fn(dof):
    from nonlinear_optimizer_for_slam_amd import api
    return api.register3_batch if dof == 3 else api.register6_batch


# ------------------------------------------------------------------------------ 1. equality with the snapshot route

@pytest.mark.gpu
@pytest.mark.parametrize("res,r2", GRID)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dof", [6, 3])
def test_every_row_equals_the_snapshot_route_bit_for_bit(ctx, stores, dof, dtype, res, r2):
    vm, snap, _, batch, R0, t0 = stores(res, r2)
    assert [len(s) for s in batch[:5]] == list(SIZES)
    n_ok = 0
    for loss in LOSSES:
        for keep in (None, 4):
            want = _fn(dof)(snap, batch, R0, t0, loss, keep_multiple=keep, dtype=dtype)
            assert "register_batch_kernel<" in ctx.last_kernel()
            got = _fn(dof)(vm, batch, R0, t0, loss, keep_multiple=keep, dtype=dtype)
            kernel = ctx.last_kernel()
            assert "register_live_kernel<nos::Ndt%dProblem<%s" % (dof, "double" if dtype == "f64" else "float") in kernel, kernel
            _same_call(got, want, (dof, dtype, res, r2, loss, keep))
            reps = got[2]
            n_ok += sum(r["ok"] for r in reps)
            for r in reps:  # real registrations: matches in every round, the tail drop applied
                for e in r["rounds"]:
                    assert e["used"] == e["matches"] - (e["matches"] % keep if keep else 0)
            assert all(r["rounds"][0]["matches"] >= len(s) // 4 for r, s in zip(reps[1:], batch[1:])), reps
    assert n_ok >= 6 * (len(batch) - 2), n_ok  # the 1-point scan may fail; the others register


# ------------------------------------------------------------------------------ 2. equality with the lone live path

def _quat_vec_norm(R):
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    return float(np.sqrt(max(0.0, (1.0 - c) / 2.0)))


def _lone_margin(ctx, vm, sc, R0, t0, loss, dof, dtype, keep):
    """The lone loop round by round → the smallest |q / 1e-5 - 1| over its stopping quantities (numpy's, as scan_to_map's)."""
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    pose, last, worst = Pose(R0, t0), Pose(R0, t0), np.inf
    for _ in range(10):
        try:
            p, _, _ = pipeline.scan_to_map(ctx, vm, sc, pose, loss, max_outer_iterations=1, dof=dof, dtype=dtype, keep_multiple=keep)
        except RuntimeError:
            break
        dtn, qv = float(np.linalg.norm(p.R.T @ (last.t - p.t))), _quat_vec_norm(p.R.T @ last.R)
        worst = min(worst, abs(dtn / 1e-5 - 1.0), abs(qv / 1e-5 - 1.0))
        if dtn < 1e-5 and qv < 1e-5:
            break
        pose, last = p, Pose(p.R, p.t)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dof", [6, 3])
def test_rows_of_at_most_512_points_equal_the_lone_live_scan_to_map(ctx, stores, dof, dtype):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    vm, _, _, batch, R0, t0 = stores(1.0, 1.0)
    small = [i for i, s in enumerate(batch) if len(s) <= 512]
    assert len(small) == 6
    for loss, keep in ((EXP, 4), (None, None)):
        poses = [Pose(R0[i].reshape(3, 3), t0[i]) for i in range(len(batch))]
        got = pipeline.scan_to_map_batch(ctx, vm, batch, poses, loss, dof=dof, dtype=dtype, keep_multiple=keep)
        n_ok = 0
        for i in small:
            try:
                want = pipeline.scan_to_map(ctx, vm, batch[i], poses[i], loss, dof=dof, dtype=dtype, keep_multiple=keep)
            except RuntimeError:
                want = None
            if want is None:
                assert got[i] is None, i
                continue
            margin = _lone_margin(ctx, vm, batch[i], poses[i].R, poses[i].t, loss, dof, dtype, keep)
            assert margin > MARGIN, ("the input sits on scan_to_map's stopping threshold", i, margin)
            assert got[i] is not None, i
            (pg, rg, og), (pw, rw, ow) = got[i], want
            assert og == ow and np.array_equal(pg.R, pw.R) and np.array_equal(pg.t, pw.t), (dof, dtype, loss, i, og, ow)
            assert len(rg) == len(rw)
            for a, b in zip(rg, rw):
                assert {k: _bits(v) for k, v in a.items()} == {k: _bits(v) for k, v in b.items()}, (i, a, b)
            n_ok += 1
        assert n_ok >= 5


# ------------------------------------------------------------------------------ 3. through the life of a store

@pytest.mark.gpu
@pytest.mark.parametrize("dof", [6, 3])
def test_through_the_life_of_a_store(ctx, dof):
    from nonlinear_optimizer_for_slam_amd import api
    res = 1.0
    rng = np.random.default_rng(313)
    scans, batch, R0, t0 = _make_scans(ctx, res)
    vm = api.VoxelMap(ctx, res, 1.0, capacity=0)

    def compare(expect_all_failed):
        _guard_holds(vm, res)
        snap = vm.snapshot()
        want = _fn(dof)(snap, batch, R0, t0, EXP, keep_multiple=4)
        snap.close()
        got = _fn(dof)(vm, batch, R0, t0, EXP, keep_multiple=4)  # status OK: a failed status raises
        _same_call(got, want)
        if expect_all_failed:  # every problem fails alone in round 0, its pose kept
            assert np.array_equal(got[0], R0) and np.array_equal(got[1], t0)
            for r in got[2]:
                assert not r["ok"] and r["outer_iter"] == 0 and len(r["rounds"]) == 1
                assert r["rounds"][0]["matches"] == 0 and not r["rounds"][0]["ok"]
        elif expect_all_failed is not None:
            assert sum(r["ok"] for r in got[2]) >= len(batch) - 1

    compare(True)  # an empty store is not an error
    vm.insert(_surface(rng, 300, res) * np.array([0.15, 0.15, 1.0]))  # a first insert that fits the 16 slots
    assert vm.memory()["capacity"] == 16 and 0 < len(vm) <= 16
    compare(None)  # a handful of voxels: rows may fail or not, but as the snapshot route's do
    vm.insert(_surface(rng, 8000, res))  # growth
    assert vm.memory()["capacity"] > 16
    compare(False)
    vm.insert(_surface(rng, 3000, res, shift=(40.0, 0.0)))
    assert vm.prune(center=(0.0, 0.0, 0.0), half_extent=(8.0, 8.0, 3.0)) > 0
    compare(False)
    assert vm.prune(center=(1e3, 1e3, 1e3), half_extent=1.0) > 0 and len(vm) == 0  # everything goes
    compare(True)
    vm.insert(_surface(rng, 8000, res))  # and the store lives on
    compare(False)
    for h in scans + [vm]:
        h.close()


def _snapshot_call(vm, dof, batch, R0, t0, loss=EXP, **kwargs):
    snap = vm.snapshot()
    try:
        return _fn(dof)(snap, batch, R0, t0, loss, **kwargs)
    finally:
        snap.close()


# ------------------------------------------------------------------------------ 4. failing problems, degenerate options

@pytest.mark.gpu
@pytest.mark.parametrize("dof", [6, 3])
def test_a_scan_far_from_every_voxel_fails_alone(ctx, stores, dof):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    vm, snap, scans, _, R0, t0 = stores(1.0, 1.0)
    far = api.Scan(ctx, np.random.default_rng(317).uniform(-3, 3, size=(200, 3)) + np.array([500.0, 0.0, 0.0]))
    keep = [1, 2, 4]  # 63, 512 and 1 500 points
    with_far = [scans[1], far, scans[2], scans[4]]
    Rw, tw = np.insert(R0[keep], 1, np.eye(3).reshape(9), axis=0), np.insert(t0[keep], 1, 0.0, axis=0)
    got = _fn(dof)(vm, with_far, Rw, tw, EXP)
    rep = got[2][1]
    assert not rep["ok"] and rep["outer_iter"] == 0 and len(rep["rounds"]) == 1 and rep["rounds"][0]["matches"] == 0
    assert np.array_equal(got[0][1], np.eye(3).reshape(9)) and not got[1][1].any()
    without = _fn(dof)(vm, [scans[i] for i in keep], R0[keep], t0[keep], EXP)
    others = [0, 2, 3]
    assert all(r["ok"] for r in without[2])
    _same_call((got[0][others], got[1][others], [got[2][i] for i in others]), without)
    _same_call(got, _fn(dof)(snap, with_far, Rw, tw, EXP))
    rows = pipeline.scan_to_map_batch(ctx, vm, with_far, [Pose(R.reshape(3, 3), t) for R, t in zip(Rw, tw)], EXP, dof=dof)
    assert rows[1] is None and all(rows[i] is not None for i in others)
    far.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_outer, max_iterations", [(1, 40), (10, 0)])
def test_one_round_and_no_iterations_equal_the_snapshot_route(ctx, stores, max_outer, max_iterations):
    vm, snap, _, batch, R0, t0 = stores(1.0, 1.0)
    for dof in (6, 3):
        for dtype in ("f64", "f32"):
            kw = dict(max_outer_iterations=max_outer, max_iterations=max_iterations, dtype=dtype, keep_multiple=4)
            got = _fn(dof)(vm, batch, R0, t0, EXP, **kw)
            _same_call(got, _fn(dof)(snap, batch, R0, t0, EXP, **kw), (dof, dtype))
            assert all(len(r["rounds"]) <= max_outer for r in got[2])
            if max_iterations == 0:
                assert all(e["iterations"] == 0 for r in got[2] for e in r["rounds"])


# ------------------------------------------------------------------------------ 5. the store is untouched

@pytest.mark.gpu
def test_the_store_is_untouched_and_the_results_are_independent_of_it(ctx):
    vm, twin = _build_store(ctx, 1.0, 1.0), _build_store(ctx, 1.0, 1.0)
    scans, batch, R0, t0 = _make_scans(ctx, 1.0)
    before, mem, info = vm.stats(), vm.memory(), (len(vm), vm.n_valid, vm.n_points)
    got = _fn(6)(vm, batch, R0, t0, EXP, keep_multiple=4)
    assert vm.memory() == mem == twin.memory() and (len(vm), vm.n_valid, vm.n_points) == info  # epoch, generation, bytes
    after = vm.stats()
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    held = (got[0].copy(), got[1].copy(), [dict(r, rounds=[dict(e) for e in r["rounds"]]) for r in got[2]])
    # an insert after a registration gives the store an insert without one gives
    more = _surface(np.random.default_rng(331), 4000, 1.0, shift=(3.0, 2.0))
    assert vm.insert(more) == twin.insert(more)
    a, b = vm.stats(), twin.stats()
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert vm.memory() == twin.memory()
    _same_call(got, held)
    assert vm.prune(center=(0.0, 0.0, 0.0), half_extent=2.0) > 0
    _same_call(got, held)
    vm.close()
    _same_call(got, held)
    for h in scans + [twin]:
        h.close()


# ------------------------------------------------------------------------------ 6. work per call

@pytest.mark.gpu
def test_a_call_is_one_launch_whatever_the_store_holds(ctx):
    """The launch count between profile_begin and profile_end is the library's own tally (as for nos_voxel_map_match):
    nos_voxel_map_register*_batch adds the one launch it issues, so `== 1` documents the call's shape and follows from the
    code — it would NOT notice a second launch, a map-sized memset or an allocation added later without a tally.  The
    guard with teeth here is memory(): capacity, bytes, epoch and generation equal before and after, at ~50 and at ~5 000
    voxels."""
    from nonlinear_optimizer_for_slam_amd import api
    rng = np.random.default_rng(337)
    small, large = api.VoxelMap(ctx, 1.0, 1.0), api.VoxelMap(ctx, 1.0, 1.0)
    small.insert(rng.uniform([-2, -2, -1], [3, 3, 1], size=(3000, 3)))  # 5 x 5 x 2 cells
    large.insert(rng.uniform([-25, -25, -1], [25, 25, 1], size=(150_000, 3)))
    assert 40 <= len(small) <= 60 and 4500 <= len(large) <= 5500, (len(small), len(large))
    scs = [api.Scan(ctx, rng.uniform([-2, -2, -1], [3, 3, 1], size=(n, 3))) for n in (100, 500, 1500)]
    batch = scs * 8
    R0, t0 = np.tile(np.eye(3).reshape(9), (len(batch), 1)), np.zeros((len(batch), 3))
    counts = {}
    for name, vm in (("small", small), ("large", large)):
        for B in (1, len(batch)):
            mem = vm.memory()
            ctx.profile_begin(sample_every=0)
            _, _, reps = _fn(6)(vm, batch[:B], R0[:B], t0[:B], EXP)
            counts[(name, B)] = ctx.profile_end()[0]
            assert "register_live_kernel<" in ctx.last_kernel()
            assert vm.memory() == mem and sum(len(r["rounds"]) for r in reps) >= B  # nothing replaced
    assert set(counts.values()) == {1}, counts
    for h in scs + [small, large]:
        h.close()


# ------------------------------------------------------------------------------ 7. rejections

def _raw_call(vm_h, scs, n=None, ropt_kw=None, opt_kw=None, dof=6, null=None):
    """One nos_voxel_map_register*_batch call on sentinel-filled outputs → (status, everything written as bytes, text)."""
    from nonlinear_optimizer_for_slam_amd import _lib
    from nonlinear_optimizer_for_slam_amd.api import make_loss
    lib = _lib.hip_lib()
    B = len(scs)
    R, t = np.full((B, 9), 7.0), np.full((B, 3), 7.0)
    log = (_lib.NosRegisterRound * (B * 10))()
    ctypes.memset(log, 0x5A, ctypes.sizeof(log))
    kw = dict(max_outer_iterations=10, max_neighbors=2, keep_multiple=0, dtype=_lib.NOS_F64)
    kw.update(ropt_kw or {})
    ropt = _lib.NosRegisterOptions(kw["max_outer_iterations"], kw["max_neighbors"], kw["keep_multiple"], kw["dtype"], log)
    okw = dict(max_iterations=40, cost_history=None)
    okw.update(opt_kw or {})
    opt = _lib.NosLmOptions(okw["max_iterations"], 0, 1e-6, 1e-6, okw["cost_history"])
    reps = (_lib.NosRegisterReport * B)()
    ctypes.memset(reps, 0x5A, ctypes.sizeof(reps))
    handles = (ctypes.c_void_p * B)(*[s._h for s in scs])
    loss = make_loss(EXP)
    args = [vm_h, handles, B if n is None else n, R.ctypes.data_as(_lib.c_double_p), t.ctypes.data_as(_lib.c_double_p),
            ctypes.byref(loss), ctypes.byref(ropt), ctypes.byref(opt), reps]
    if null is not None:
        args[null] = None
    fn = lib.nos_voxel_map_register3_batch if dof == 3 else lib.nos_voxel_map_register6_batch
    st = fn(*args)
    return st, R.tobytes() + t.tobytes() + bytes(reps) + bytes(log), lib.nos_last_error().decode()


@pytest.mark.gpu
def test_rejected_calls_return_their_status_and_write_nothing(ctx, stores):
    from nonlinear_optimizer_for_slam_amd import _lib, api
    from nonlinear_optimizer_for_slam_amd.api import Context, shm_unlink
    vm, _, scans, _, _, _ = stores(1.0, 1.0)
    scs = scans[1:4]
    sentinels = (np.full(3 * 12, 7.0).tobytes() + bytes([0x5A]) * (3 * ctypes.sizeof(_lib.NosRegisterReport)) +
                 bytes([0x5A]) * (3 * 10 * ctypes.sizeof(_lib.NosRegisterRound)))
    mem, before = vm.memory(), vm.stats()
    # everything nos_ndt*_register_batch rejects, with its status
    cases = [dict(null=0), dict(null=1), dict(null=3), dict(null=4), dict(null=6), dict(null=7), dict(null=8), dict(n=-1),
             dict(ropt_kw={"max_outer_iterations": 0}), dict(ropt_kw={"keep_multiple": -1}), dict(ropt_kw={"dtype": 7}),
             dict(opt_kw={"max_iterations": -1}),
             dict(opt_kw={"cost_history": np.zeros(40).ctypes.data_as(ctypes.POINTER(ctypes.c_double))})]
    for case in cases:
        for dof in (6, 3):
            st, written, text = _raw_call(vm._h, scs, dof=dof, **case)
            assert st == INVALID, (case, dof, st, text)
            assert written == sentinels, case
    for k in (0, 3):
        st, written, text = _raw_call(vm._h, scs, ropt_kw={"max_neighbors": k})
        assert st == UNSUPPORTED and "max_neighbors" in text and written == sentinels
    # a scan of another context than the store's: the status nos_ndt*_register_batch and nos_voxel_map_match give it
    other = Context((0,))
    alien = api.Scan(other, np.zeros((4, 3)))
    st, written, text = _raw_call(vm._h, [scs[0], alien, scs[1]])
    assert st == INVALID and "another context" in text and written == sentinels
    alien.close()
    other.close()
    # a context with a communicator
    shm = "/nos_vreg_%d" % os.getpid()
    c2 = Context((0,))
    c2.comm_init_shm(1, 0, shm)
    try:
        v2 = api.VoxelMap(c2, 1.0, 1.0)
        v2.insert(_surface(np.random.default_rng(347), 2000, 1.0))
        s2 = [api.Scan(c2, _surface(np.random.default_rng(349), 50, 1.0)) for _ in range(3)]
        st, written, text = _raw_call(v2._h, s2)
        assert st == UNSUPPORTED and "communicator" in text and written == sentinels
        for h in s2 + [v2]:
            h.close()
    finally:
        c2.close()
        shm_unlink(shm)
    # the 9-cell span limit of the live matcher: 2 r / resolution + 2 > 9
    fine = api.VoxelMap(ctx, 0.25, 1.0)
    fine.insert(_surface(np.random.default_rng(353), 2000, 0.25))
    for dof in (6, 3):
        st, written, text = _raw_call(fine._h, scs, dof=dof)
        assert st == UNSUPPORTED and "9" in text and written == sentinels
    with pytest.raises(_lib.NosError) as err:
        api.register6_batch(fine, scs, np.tile(np.eye(3).reshape(9), (3, 1)), np.zeros((3, 3)), EXP)
    assert err.value.status == UNSUPPORTED
    fine.close()
    # the last admitted span (0.3: 2 / 0.3 + 2 = 8.7) registers, and as its snapshot does
    coarse_enough = _build_store(ctx, 0.3, 1.0)
    _guard_holds(coarse_enough, 0.3)
    R0, t0 = np.tile(np.eye(3).reshape(9), (3, 1)), np.zeros((3, 3))
    _same_call(_fn(6)(coarse_enough, scs, R0, t0, EXP), _snapshot_call(coarse_enough, 6, scs, R0, t0))
    coarse_enough.close()
    # n_problems == 0: nothing to do, nothing written
    st, written, _ = _raw_call(vm._h, scs, n=0)
    assert st == 0 and written == sentinels
    # nothing above touched the store
    assert vm.memory() == mem
    after = vm.stats()
    for key in before:
        assert np.array_equal(before[key], after[key]), key


# ------------------------------------------------------------------------------ 8. pipeline

@pytest.mark.gpu
@pytest.mark.parametrize("dof", [6, 3])
def test_scan_to_map_batch_takes_a_voxel_map(ctx, stores, dof):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    vm, snap, _, batch, R0, t0 = stores(0.5, 1.0)
    poses = [Pose(R.reshape(3, 3), t) for R, t in zip(R0, t0)]
    for kw in (dict(), dict(keep_multiple=4, dtype="f32", loss=("huber", 0.7))):
        got = pipeline.scan_to_map_batch(ctx, vm, batch, poses, dof=dof, **kw)
        assert "register_live_kernel<" in ctx.last_kernel()
        want = pipeline.scan_to_map_batch(ctx, snap, batch, poses, dof=dof, **kw)
        assert len(got) == len(want) == len(batch) and sum(g is not None for g in got) >= len(batch) - 1
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                assert np.array_equal(g[0].R, w[0].R) and np.array_equal(g[0].t, w[0].t) and g[2] == w[2]
                assert [{k: _bits(v) for k, v in e.items()} for e in g[1]] == [{k: _bits(v) for k, v in e.items()} for e in w[1]]
    got = pipeline.scan_to_map_batch(ctx, vm, batch[:2], None, dof=dof)  # identity starts
    want = pipeline.scan_to_map_batch(ctx, snap, batch[:2], None, dof=dof)
    assert [(g is None) for g in got] == [(w is None) for w in want]


@pytest.fixture(scope="module")
def room():
    """tests/test_voxel_map_match.py's 12 frames of the reference's room, each sub-sampled to 500 points"""
    pts = scene.generate_global_points()
    filtered = scene.filter_points(pts, 0.1)
    c, s = np.cos(0.1), np.sin(0.1)
    Rt = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    tt = np.array([-0.2, 0.123, 0.3])  # true pose, MDM/tests/simple_optimization_test.cc:85-88
    rng = np.random.default_rng(359)
    locals_ = []
    for f in range(12):  # a sensor that turns 0.01 rad and moves about 3 cm per frame
        Rf = Rt @ helpers.rot_xyz(0.0, 0.0, 0.01 * f)
        tf = tt + f * np.array([0.02, -0.02, 0.005])
        local = (Rf.T @ (filtered - tf).T).T
        locals_.append(local[np.sort(rng.choice(local.shape[0], size=min(500, local.shape[0]), replace=False))])
    return {"points": pts, "locals": locals_}


def _room_store(ctx, room):
    from nonlinear_optimizer_for_slam_amd import api
    vm = api.VoxelMap(ctx, 1.0, 1.0, proper_sqrt_information=True)
    for b in np.array_split(room["points"], 8):
        vm.insert(b)
    return vm


@pytest.mark.gpu
@pytest.mark.parametrize("kwargs", [{}, {"window_half_extent": (3.0, 2.5, 2.0), "max_voxel_age": 6}, {"filter_voxel_size": 0.3}],
                         ids=["plain", "window", "filter"])
def test_odometry_in_one_launch_per_frame_equals_odometry_with_live_match(ctx, room, kwargs):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    scans = [api.Scan(ctx, p) for p in room["locals"]]
    assert all(len(s) <= 512 for s in scans)
    a, b = _room_store(ctx, room), _room_store(ctx, room)
    want = pipeline.odometry(ctx, a, scans, loss=EXP, live_match=True, keep_multiple=4, **kwargs)
    got = pipeline.odometry(ctx, b, scans, loss=EXP, one_launch=True, keep_multiple=4, **kwargs)
    assert len(got[0]) == len(want[0]) == 12
    for pa, pb in zip(got[0], want[0]):
        assert np.array_equal(pa.R, pb.R) and np.array_equal(pa.t, pb.t)
    assert all(len(r) >= 1 for r in got[1]) and len(got[1]) == len(want[1])
    for ra, rb in zip(got[1], want[1]):
        assert [{k: _bits(v) for k, v in e.items()} for e in ra] == [{k: _bits(v) for k, v in e.items()} for e in rb]
    sa, sb = a.stats(), b.stats()
    for key in sa:
        assert np.array_equal(sa[key], sb[key]), key
    assert a.memory() == b.memory()
    _guard_holds(b, 1.0)
    for h in scans + [a, b]:
        h.close()


@pytest.mark.gpu
def test_a_frame_that_fails_in_one_launch_raises_before_anything_is_inserted(ctx):
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    vm = _build_store(ctx, 1.0, 1.0)
    far = api.Scan(ctx, np.random.default_rng(367).uniform(-3, 3, size=(200, 3)) + np.array([500.0, 0.0, 0.0]))
    mem, info = vm.memory(), (len(vm), vm.n_points)
    with pytest.raises(RuntimeError):
        pipeline.odometry(ctx, vm, [far], one_launch=True)
    assert vm.memory() == mem and (len(vm), vm.n_points) == info
    far.close(), vm.close()


def test_one_launch_refuses_what_it_cannot_do():
    """No GPU: the checks come before the store or a scan is touched."""
    from nonlinear_optimizer_for_slam_amd import pipeline
    for kw in (dict(indexed=True), dict(on_solve=lambda *a: None), dict(device_loop=False), dict(live_match=False)):
        with pytest.raises(ValueError):
            pipeline.odometry(None, None, [], one_launch=True, **kw)
    # what it does take, and the default, reach the (empty) frame loop
    assert pipeline.odometry(None, None, [], one_launch=True, live_match=True, loss=EXP, options=None, max_outer_iterations=3,
                             dof=3, dtype="f32", keep_multiple=4, device_loop=True, indexed=False) == ([], [])
    assert pipeline.odometry(None, None, []) == ([], [])
