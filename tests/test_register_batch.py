"""Batched scan-to-map registration (nos_ndt6_register_batch / nos_ndt3_register_batch; api.register6_batch /
register3_batch; pipeline.scan_to_map_batch): many scans against one map, the reference's outer loop on the device.

Every row must equal its lone pipeline.scan_to_map BIT FOR BIT when the scan has ≤ 512 points: pose, outer_iter and every
round's matches / used / iterations / printed cost.  The batch runs match_kernel's per-point body, the tail drop of
nos_dataset_drop_last_matches and the loop of the single-workgroup solve on the same data the lone calls produce.

Choice of inputs.  scan_to_map stops when |dt| < 1e-5 and |vec(dq)| < 1e-5, computed with numpy; the device computes the
same quantities in the same order, but numpy's BLAS products and np.linalg.norm need not round like the device.  So the
scenes below keep BOTH stopping quantities outside 1e-5 * (1 ± 1e-4) in every round, 50 times the ≈ 2e-6 relative error of
the trace form near the threshold.  test_scenes_keep_the_stopping_quantities_off_the_threshold checks this on the CPU with
the oracle loop (oracle.ndt6_solve / ndt3_solve on the CPU matcher's correspondences) for every fp64 configuration; the
smallest margin it found is min |q / 1e-5 - 1| = 2.5e-02 (random scene) and 3.7e-02 (room scene).  The GPU test checks
the same condition again on the lone runs it compares against (fp32 included), so an input that came too close fails
instead of passing by luck.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle_scene as scene
from tests import helpers

EXP = ("exponential", 1.0, 1.0)
LOSSES = [None, EXP, ("huber", 0.7)]
B_RANDOM = 40
MARGIN = 1e-4


def _quat_vec_norm(R):
    c = (np.trace(R) - 1.0) / 2.0
    c = min(1.0, max(-1.0, c))
    return float(np.sqrt(max(0.0, (1.0 - c) / 2.0)))


def _stop_quantities(R, t, lastR, lastt):
    """scan_to_map's two stopping quantities, computed as it computes them."""
    dR = R.T @ lastR
    dt = R.T @ (lastt - t)
    return float(np.linalg.norm(dt)), _quat_vec_norm(dR)


def _margin(q):
    return abs(q / 1e-5 - 1.0)


# ------------------------------------------------------------------------------------------------ scenes

def _random_scene():
    """A random map in the style of test_gpu_matcher_records_are_bit_exact and 40 scans of 1 … 512 points."""
    rng = np.random.default_rng(2024)
    n_voxels = 500
    means = rng.uniform(-12.0, 12.0, size=(n_voxels, 3)) * np.array([1.0, 1.0, 0.25])
    S = rng.normal(size=(n_voxels, 3, 3))
    valid = rng.uniform(size=n_voxels) >= 0.1
    sizes = np.linspace(1, 512, B_RANDOM).astype(int)
    scans = [rng.uniform(-13.0, 13.0, size=(int(n), 3)) * np.array([1.0, 1.0, 0.25]) for n in sizes]
    poses = []
    for _ in range(B_RANDOM):
        a = rng.uniform(-0.05, 0.05, size=3)
        poses.append((helpers.rot_xyz(*a), rng.uniform(-0.3, 0.3, size=3)))
    return {"means": means, "sqrt_infos": S, "valid": valid}, scans, poses


def _room_scene():
    """The reference's room map and 16 sub-sampled scans (300 … 512 points) of its simple_6dof scan, from identity."""
    pts = scene.generate_global_points()
    ndt = scene.build_ndt_map_eigen(pts, 1.0)
    local, _, _ = scene.captured_run_scan(pts, "simple_6dof")
    rng = np.random.default_rng(11)
    scans = []
    for n in np.linspace(300, 512, 16).astype(int):
        scans.append(local[np.sort(rng.choice(local.shape[0], size=int(n), replace=False))])
    poses = [(np.eye(3), np.zeros(3)) for _ in scans]
    return {"means": ndt["means"], "sqrt_infos": ndt["sqrt_infos"], "valid": ndt["valid"]}, scans, poses


_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        _SCENES[name] = _random_scene() if name == "random" else _room_scene()
    return _SCENES[name]


# ------------------------------------------------------------------------------------------------ CPU: the inputs

def _oracle_loop_margin(oracle, m, local, R, t, dof, loss, keep, max_outer=10):
    """OptimizePoseAnalytic with the CPU matcher and the oracle's solve → smallest stopping-quantity margin seen."""
    lastR, lastt = R.copy(), t.copy()
    worst = np.inf
    stride = keep or 1
    solve = oracle.ndt3_solve if dof == 3 else oracle.ndt6_solve
    for _ in range(max_outer):
        planes, _, idx = scene.match_point_cloud(m["means"], m["sqrt_infos"], m["valid"], local, R, t)
        planes, n_matches = scene.compact_correspondences(planes, idx, stride)
        if planes.shape[1] == 0:
            break  # nothing to solve: the device reports ok = 0 there (checked by the GPU test)
        res = solve(planes, t, R, loss=loss, linear_solver=1)
        R, t = np.asarray(res["R"]).reshape(3, 3), np.asarray(res["t"]).reshape(3)
        if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
            break
        dtn, qv = _stop_quantities(R, t, lastR, lastt)
        worst = min(worst, _margin(dtn), _margin(qv))
        if dtn < 1e-5 and qv < 1e-5:
            break
        lastR, lastt = R.copy(), t.copy()
    return worst


@pytest.mark.parametrize("name", ["random", "room"])
def test_scenes_keep_the_stopping_quantities_off_the_threshold(oracle, name):
    m, scans, poses = _scene(name)
    worst = np.inf
    for dof in (6, 3):
        for loss in LOSSES:
            for keep in (None, 4):
                for local, (R0, t0) in zip(scans, poses):
                    worst = min(worst, _oracle_loop_margin(oracle, m, local, R0, t0, dof, loss, keep))
    print("smallest margin of %s: %.3g" % (name, worst))
    assert worst > MARGIN, (name, worst)


# ------------------------------------------------------------------------------------------------ GPU

def _lone(ctx, gm, sc, R0, t0, loss, dof, dtype, keep, max_outer=10, max_iterations=40):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Options, Pose
    try:
        return pipeline.scan_to_map(ctx, gm, sc, Pose(R0, t0), loss, Options(max_iterations=max_iterations),
                                    max_outer_iterations=max_outer, dof=dof, dtype=dtype, keep_multiple=keep)
    except RuntimeError:
        return None


def _assert_same(got, want, where):
    """A row of scan_to_map_batch against its lone scan_to_map, bit for bit (None: the lone call raised)."""
    if want is None:
        assert got is None, where
        return
    assert got is not None, where
    (pg, rg, og), (pw, rw, ow) = got, want
    assert og == ow, (where, og, ow)
    assert np.array_equal(pg.R, pw.R) and np.array_equal(pg.t, pw.t), (where, pg.R, pw.R, pg.t, pw.t)
    assert len(rg) == len(rw), (where, rg, rw)
    for a, b in zip(rg, rw):
        assert set(a) == set(b) == {"matches", "used", "iterations", "printed_cost"}, (where, a, b)
        for k in ("matches", "used", "iterations"):
            assert a[k] == b[k], (where, k, a, b)
        assert np.array_equal(np.float64(a["printed_cost"]), np.float64(b["printed_cost"])), (where, a, b)


def _maps_and_scans(ctx, name):
    from nonlinear_optimizer_for_slam_amd import api
    m, scans, poses = _scene(name)
    gm = api.NdtMap(ctx, m["means"], m["sqrt_infos"], m["valid"], 1.0)
    scs = [api.Scan(ctx, s) for s in scans]
    return gm, scs, poses


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [None, 4], ids=["all", "keep4"])
@pytest.mark.parametrize("loss", LOSSES, ids=["none", "exp", "huber"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("dof", [6, 3])
@pytest.mark.parametrize("name", ["random", "room"])
def test_every_row_equals_its_lone_scan_to_map_bit_for_bit(ctx, name, dof, dtype, loss, keep):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Options, Pose
    gm, scs, poses = _maps_and_scans(ctx, name)
    got = pipeline.scan_to_map_batch(ctx, gm, scs, [Pose(R, t) for R, t in poses], loss, Options(), dof=dof, dtype=dtype,
                                     keep_multiple=keep)
    assert "register_batch_kernel<" in ctx.last_kernel()
    assert len(got) == len(scs)
    n_ok = 0
    for i, (sc, (R0, t0)) in enumerate(zip(scs, poses)):
        want = _lone(ctx, gm, sc, R0, t0, loss, dof, dtype, keep)
        _assert_same(got[i], want, (name, dof, dtype, loss, keep, i, len(sc)))
        n_ok += want is not None
    assert n_ok >= len(scs) // 2  # real registrations, not only early failures
    for h in scs + [gm]:
        h.close()


@pytest.mark.gpu
def test_rounds_log_and_stopping_quantities(ctx):
    """Round by round, the lone loop's stopping quantities (numpy) stay off the threshold by the margin: the condition on
    the inputs, checked again on the GPU runs themselves, fp32 included (the per-round log itself is compared with the lone
    rounds by the bit-identity tests)."""
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Options, Pose
    for name in ("random", "room"):
        gm, scs, poses = _maps_and_scans(ctx, name)
        for dof in (6, 3):
            for dtype in ("f64", "f32"):
                for loss in LOSSES:
                    for keep in (None, 4):
                        worst = np.inf
                        for sc, (R0, t0) in zip(scs, poses):
                            pose, last = Pose(R0, t0), Pose(R0, t0)
                            for _ in range(10):
                                try:
                                    p, _, _ = pipeline.scan_to_map(ctx, gm, sc, pose, loss, Options(), max_outer_iterations=1,
                                                                   dof=dof, dtype=dtype, keep_multiple=keep)
                                except RuntimeError:
                                    break
                                dtn, qv = _stop_quantities(p.R, p.t, last.R, last.t)
                                worst = min(worst, _margin(dtn), _margin(qv))
                                if dtn < 1e-5 and qv < 1e-5:
                                    break
                                pose, last = p, Pose(p.R, p.t)
                        print("margin %s dof %d %s %s keep %s: %.3g" % (name, dof, dtype, loss, keep, worst))
                        assert worst > MARGIN, (name, dof, dtype, loss, keep, worst)
        for h in scs + [gm]:
            h.close()


@pytest.mark.gpu
def test_multi_start_one_scan_from_64_poses(ctx):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Options, Pose
    gm, scs, _ = _maps_and_scans(ctx, "room")
    sc = scs[-1]
    rng = np.random.default_rng(5)
    poses = [(helpers.rot_xyz(*rng.uniform(-0.04, 0.04, size=3)), rng.uniform(-0.2, 0.2, size=3)) for _ in range(64)]
    got = pipeline.scan_to_map_batch(ctx, gm, [sc] * 64, [Pose(R, t) for R, t in poses], EXP, Options(), keep_multiple=4)
    for i, (R0, t0) in enumerate(poses):
        _assert_same(got[i], _lone(ctx, gm, sc, R0, t0, EXP, 6, "f64", 4), i)
    assert len({got[i][0].t.tobytes() for i in range(64) if got[i] is not None}) > 1
    for h in scs + [gm]:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dof", [6, 3])
def test_a_scan_without_matches_fails_alone(ctx, dof):
    """A scan far from the map: no match at its start pose, the solve fails (ok = 0), the lone call raises; its row keeps
    its start pose and the neighbours are unaffected."""
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    gm, scs, poses = _maps_and_scans(ctx, "room")
    far = api.Scan(ctx, np.asarray(_scene("room")[1][0]) + np.array([500.0, 0.0, 0.0]))
    batch = [scs[0], far, scs[1]]
    starts = [poses[0], (np.eye(3), np.zeros(3)), poses[1]]
    fn = api.register3_batch if dof == 3 else api.register6_batch
    R, t, reps = fn(gm, batch, [p[0] for p in starts], [p[1] for p in starts], EXP)
    assert not reps[1]["ok"] and reps[1]["outer_iter"] == 0 and len(reps[1]["rounds"]) == 1
    assert reps[1]["rounds"][0]["matches"] == 0 and not reps[1]["rounds"][0]["ok"]
    assert np.array_equal(R[1], np.eye(3).reshape(9)) and not t[1].any()
    assert reps[0]["ok"] and reps[2]["ok"]
    with pytest.raises(RuntimeError):
        pipeline.scan_to_map(ctx, gm, far, Pose(), EXP, dof=dof)
    got = pipeline.scan_to_map_batch(ctx, gm, batch, [Pose(*p) for p in starts], EXP, dof=dof)
    assert got[1] is None
    for i in (0, 2):
        _assert_same(got[i], _lone(ctx, gm, batch[i], starts[i][0], starts[i][1], EXP, dof, "f64", None), i)
    for h in scs + [far, gm]:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_outer, max_iterations", [(1, 40), (10, 0)])
def test_one_round_and_no_iterations(ctx, max_outer, max_iterations):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Options, Pose
    gm, scs, poses = _maps_and_scans(ctx, "random")
    for dof in (6, 3):
        got = pipeline.scan_to_map_batch(ctx, gm, scs, [Pose(R, t) for R, t in poses], EXP,
                                         Options(max_iterations=max_iterations), max_outer_iterations=max_outer, dof=dof)
        for i, (sc, (R0, t0)) in enumerate(zip(scs, poses)):
            want = _lone(ctx, gm, sc, R0, t0, EXP, dof, "f64", None, max_outer=max_outer, max_iterations=max_iterations)
            _assert_same(got[i], want, (dof, i))
    for h in scs + [gm]:
        h.close()


@pytest.mark.gpu
def test_2048_problems_in_one_launch(ctx):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Options, Pose
    gm, scs, poses = _maps_and_scans(ctx, "random")
    idx = [i % len(scs) for i in range(2048)]
    got = pipeline.scan_to_map_batch(ctx, gm, [scs[i] for i in idx], [Pose(*poses[i]) for i in idx], EXP, Options())
    assert "register_batch_kernel<" in ctx.last_kernel()
    lone = {i: _lone(ctx, gm, scs[i], poses[i][0], poses[i][1], EXP, 6, "f64", None) for i in range(len(scs))}
    for j, i in enumerate(idx):
        _assert_same(got[j], lone[i], (j, i))
    for h in scs + [gm]:
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dof", [6, 3])
def test_captured_runs_through_the_batch(ctx, oracle, dof):
    """The reference's captured runs (results/*.txt) through one batched call per dof: reference-exact map built on the
    device, keep_multiple = 4, from identity.  Each row prints the captured COST / iter lines, outer_iter and final pose
    (the strings tests/test_reference_ndt_runs.py::_check_run checks)."""
    from nonlinear_optimizer_for_slam_amd import api, pipeline
    from tests.test_reference_ndt_runs import RUNS, _check_run
    pts = scene.generate_global_points_c()
    names = sorted(n for n in RUNS if scene.CAPTURED_RUNS[n][3] == dof)
    assert names
    gm, _ = api.NdtMap.build(ctx, pts, 1.0, 1.0, reference_exact=True)
    scs = [api.Scan(ctx, scene.captured_run_scan(pts, n)[0]) for n in names]
    got = pipeline.scan_to_map_batch(ctx, gm, scs, None, EXP, dof=dof, keep_multiple=4)
    for n, row in zip(names, got):
        pose, rounds, outer = row
        _check_run(oracle, n, pose.R, pose.t, [(r["printed_cost"], r["iterations"], r["matches"]) for r in rounds], outer)
    for h in scs + [gm]:
        h.close()


# ------------------------------------------------------------------------------------------------ rejected calls

def _raw_call(ctx, gm, scs, n=None, R=None, t=None, ropt_kw=None, opt_kw=None, dof=6, null=None):
    """One nos_ndt*_register_batch call on sentinel-filled outputs → (status, R, t, reports bytes, log bytes)."""
    from nonlinear_optimizer_for_slam_amd import _lib
    from nonlinear_optimizer_for_slam_amd.api import make_loss
    lib = _lib.hip_lib()
    B = len(scs)
    R = np.full((B, 9), 7.0) if R is None else R
    t = np.full((B, 3), 7.0) if t is None else t
    log = (_lib.NosRegisterRound * (B * 10))()
    ctypes.memset(log, 0x5A, ctypes.sizeof(log))
    kw = dict(max_outer_iterations=10, max_neighbors=2, keep_multiple=0, dtype=_lib.NOS_F64)
    kw.update(ropt_kw or {})
    ropt = _lib.NosRegisterOptions(kw["max_outer_iterations"], kw["max_neighbors"], kw["keep_multiple"], kw["dtype"], log)
    okw = dict(max_iterations=40, cost_history=None)
    okw.update(opt_kw or {})
    opt = _lib.NosLmOptions(okw["max_iterations"], 0, 1e-6, 1e-6, okw["cost_history"])
    reps = (_lib.NosRegisterReport * max(B, 1))()
    ctypes.memset(reps, 0x5A, ctypes.sizeof(reps))
    handles = (ctypes.c_void_p * max(B, 1))(*[s._h for s in scs])
    loss = make_loss(EXP)
    args = [gm._h, handles, B if n is None else n, R.ctypes.data_as(_lib.c_double_p), t.ctypes.data_as(_lib.c_double_p),
            ctypes.byref(loss), ctypes.byref(ropt), ctypes.byref(opt), reps]
    if null is not None:
        args[null] = None
    fn = lib.nos_ndt3_register_batch if dof == 3 else lib.nos_ndt6_register_batch
    st = fn(*args)
    return st, R, t, bytes(reps), bytes(log)


@pytest.mark.gpu
def test_rejected_calls_write_nothing(ctx):
    from nonlinear_optimizer_for_slam_amd import api
    from nonlinear_optimizer_for_slam_amd.api import Context
    INVALID, UNSUPPORTED = 1, 6  # NOS_ERR_INVALID_ARGUMENT, NOS_ERR_UNSUPPORTED
    gm, all_scans, _ = _maps_and_scans(ctx, "random")
    scs = all_scans[:3]
    from nonlinear_optimizer_for_slam_amd import _lib
    sentinels = (bytes([0x5A]) * (3 * ctypes.sizeof(_lib.NosRegisterReport)),  # what _raw_call fills reports and log with
                 bytes([0x5A]) * (3 * 10 * ctypes.sizeof(_lib.NosRegisterRound)))
    untouched = lambda: sentinels  # noqa: E731
    cases = [
        dict(null=0), dict(null=1), dict(null=3), dict(null=4), dict(null=6), dict(null=7), dict(null=8),
        dict(n=-1),
        dict(ropt_kw={"max_outer_iterations": 0}),
        dict(ropt_kw={"keep_multiple": -1}),
        dict(ropt_kw={"dtype": 7}),
        dict(opt_kw={"max_iterations": -1}),
        dict(opt_kw={"cost_history": np.zeros(40).ctypes.data_as(ctypes.POINTER(ctypes.c_double))}),
    ]
    for case in cases:
        for dof in (6, 3):
            st, R, t, reps, log = _raw_call(ctx, gm, scs, dof=dof, **case)
            assert st == INVALID, (case, dof, st)
            assert (R == 7.0).all() and (t == 7.0).all(), case
            assert (reps, log) == untouched(), case
    st, R, t, reps, log = _raw_call(ctx, gm, scs, ropt_kw={"max_neighbors": 3})
    assert st == UNSUPPORTED and (R == 7.0).all() and (t == 7.0).all() and (reps, log) == untouched()
    # a scan of another context
    other = Context((0,))
    alien = api.Scan(other, np.zeros((4, 3)))
    st, R, t, reps, log = _raw_call(ctx, gm, [scs[0], alien])
    assert st == INVALID and (R == 7.0).all() and (t == 7.0).all()
    alien.close()
    other.close()
    # a context with a communicator
    from nonlinear_optimizer_for_slam_amd.api import shm_unlink
    import os
    shm = "/nos_reg_%d" % os.getpid()
    c2 = Context((0,))
    c2.comm_init_shm(1, 0, shm)
    try:
        m, scans, _ = _scene("random")
        g2 = api.NdtMap(c2, m["means"], m["sqrt_infos"], m["valid"], 1.0)
        s2 = [api.Scan(c2, scans[5])]
        st, R, t, reps, log = _raw_call(c2, g2, s2)
        assert st == UNSUPPORTED and (R == 7.0).all() and (t == 7.0).all()
        g2.close()
        s2[0].close()
    finally:
        c2.close()
        shm_unlink(shm)
    # n_problems == 0: nothing to do
    st, R, t, reps, log = _raw_call(ctx, gm, scs, n=0)
    assert st == 0 and (R == 7.0).all() and (t == 7.0).all()
    for h in all_scans + [gm]:
        h.close()
