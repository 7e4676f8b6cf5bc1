"""GPU sums against the extended-precision reference (oracle/oracle_xp.py) at the inputs where the arithmetic form of a
kernel matters: ill-conditioned sqrt-informations (κ(S) up to 1e4, planar and linear voxels, points on the plane / line),
rank-deficient S with e in its null space, map-frame and pose offsets up to 1e5 m, the Huber and exponential loss edges,
and reprojection depth, sign and pixel-range edges (tests/edge_inputs.py).

Criterion, per case and per quantity (H against sqrt(H_ii H_jj), g against sqrt(H_ii · cost), cost relative):

    error(GPU) ≤ C · error(numpy S form in the kernel's dtype) + FLOOR[dtype],   C = 4,  FLOOR = 16 u

— the kernel may be no worse than the reference's own arithmetic (r = S e, s = rᵀr, J = [S | S M]) in the same precision.
The S form's error is taken as the larger of e = R p + t − mu summed in the reference's order (R p, then t) and in the
kernels' (t inside the fma chain): with the pose and map 1e3-1e5 m from the origin the two differ by up to 40 × in the cost.
fp32 cases are built from fp32-rounded inputs (points, means, S, pose, min_depth), so that the error measured is the
kernel's arithmetic and not the rounding of its inputs.  At κ ≤ 10 the suite's absolute tolerances against the fp64 oracle
(1e-10 / 3e-6 scaled) are asserted as well.

Measured on one MI355X, worst case over every case below, GPU / (numpy S form + 4 u):
  with the stored triangular factor U (S = QU): 1.14 (fp64), 2.1 (fp32)
  with the A = SᵀS form the datasets stored before: planar voxel, points on the plane, cost relative error
  κ = 1e3: fp64 4.7e-13 against 3.7e-17, fp32 2.4e-4 against 9.3e-7; κ = 1e4 fp32: 0.48; rank-deficient S, e in its null
  space: fp64 cost off by 1e9 relative — every one of these fails the criterion.
(profiles/xprec_errors.md holds the table per κ × offset × path × dtype.)
"""
import json
import os

import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import Context, NdtDataset, NdtIndexedDataset, ReprojDataset
from oracle import oracle_xp as xp
from tests import edge_inputs as E
from tests import helpers

pytestmark = pytest.mark.gpu

C = 4.0
FLOOR = {"f64": 16 * 2.0 ** -53, "f32": 16 * 2.0 ** -24}
NP_DTYPE = {"f64": np.float64, "f32": np.float32}
EXP = ("exponential", 1.0, 1.0)
HUBER = ("huber", 0.25)  # exact in fp32: the kernel's threshold is the reference's
LOSSES = [None, EXP, HUBER]
LOG = os.environ.get("NOS_XPREC_LOG")  # optional: one JSON line per comparison (the table of profiles/xprec_errors.md)


def _round(a, dtype):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if dtype == "f32" else a


def _log(**kw):
    if LOG:
        with open(LOG, "a") as f:
            f.write(json.dumps(kw) + "\n")


def check(got, ref, base, dim, dtype, what, cost_only=False):
    """got: the kernel's {upper(H) | g | cost} (or its cost alone); ref: the extended reference; base: the numpy S form
    in the kernel's dtype."""
    names = ("H", "g", "cost")
    if cost_only:
        eg = (0.0, 0.0, abs(float(got) - float(ref[-1])) / max(abs(float(ref[-1])), 1e-300))
    else:
        eg = xp.scaled_errors(got, ref, dim)
    eb = xp.scaled_errors(base[0], ref, dim)
    if len(base) > 1:  # the S form with e summed in either order: the larger error of the two is what that arithmetic admits
        eb = tuple(max(a, b) for a, b in zip(eb, xp.scaled_errors(base[1], ref, dim)))
    _log(what=what, dtype=dtype, gpu=eg, numpy_s_form=eb, cost_only=cost_only)  # eb: the yardstick actually used
    for k in range(3):
        if cost_only and k < 2:
            continue
        bound = C * eb[k] + FLOOR[dtype]
        assert eg[k] <= bound, "%s %s: %s error %.3e > %g x %.3e (numpy S form) + %.1e" % (what, dtype, names[k], eg[k], C,
                                                                                           eb[k], FLOOR[dtype])


def refs6(planes, R, t, loss, dtype):
    """(extended reference, (numpy S form with e = R p + t − mu in the reference's order, and in the kernels' order))"""
    d = NP_DTYPE[dtype]
    return xp.ndt6_accumulate(planes, R, t, loss), (xp.ndt6_accumulate(planes, R, t, loss, dtype=d),
                                                    xp.ndt6_accumulate(planes, R, t, loss, dtype=d, order="fma"))


def refs3(planes, R2, t2, loss, dtype):
    d = NP_DTYPE[dtype]
    return xp.ndt3_accumulate(planes, R2, t2, loss), (xp.ndt3_accumulate(planes, R2, t2, loss, dtype=d),
                                                      xp.ndt3_accumulate(planes, R2, t2, loss, dtype=d, order="fma"))


def _rounded_case(fam, n, dtype, seed=11, three=False):
    planes, (R, t), vox = (E.ndt3_case if three else E.ndt_case)(n, seed=seed, **fam)
    return _round(planes, dtype), _round(R, dtype), _round(t, dtype), vox


FAMILIES = [dict(kappa=k, shape=sh, e_mode=em) for k in E.KAPPAS for sh in ("planar", "linear") for em in ("plane", "iso")]
FAMILIES += [dict(kappa=k, offset=o, offset_in=w) for k in (10.0, 1e3) for o in E.OFFSETS[1:] for w in ("map", "pose")]
FAMILIES += [dict(kappa=1e3, rank_deficient=True, e_mode="null"), dict(kappa=1e4, rank_deficient=True, e_mode="iso")]


def _fid(f):
    return "-".join("%s=%g" % (k, v) if not isinstance(v, str) else "%s=%s" % (k, v) for k, v in f.items())


T_SHIFT = np.array([0.05, -0.03, 0.02])


def _benign(fam):
    """κ ≤ 10, no offset, full rank: where the suite's absolute tolerances against the fp64 oracle apply"""
    return fam["kappa"] <= 10 and not fam.get("offset") and not fam.get("rank_deficient")


def _kernel(ctx, *parts, shard=0):
    name = ctx.last_kernel(shard)
    for p in parts:
        assert p in name, (p, name)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fam", FAMILIES, ids=_fid)
def test_ndt_sums_every_path(ctx, oracle, fam, dtype):
    """20 000 correspondences (5 000 voxels) through the per-pass accumulate (6- and 3-DoF), the resident one-launch solve
    (its first cost), the indexed layout and two shards; 1 000 of them through the single-workgroup solve."""
    T = "double" if dtype == "f64" else "float"
    n = 20_000
    planes, R, t, (pts, vid, means, S) = _rounded_case(fam, n, dtype)
    ds = NdtDataset.from_planes(ctx, planes, dtype)
    refs = {loss: refs6(planes, R, t, loss, dtype) for loss in LOSSES}
    for loss in LOSSES:
        what = "%s %s" % (_fid(fam), loss and loss[0])
        ref, base = refs[loss]
        got = ds.accumulate6(R, t, loss)
        _kernel(ctx, "assemble_kernel<nos::Ndt6Problem<%s" % T)
        check(got, ref, base, 6, dtype, "accumulate6 " + what)
        if _benign(fam):  # away from the generating pose, where g is a sum of n terms, not of n zero-mean ones
            ts = _round(t + T_SHIFT, dtype)
            helpers.assert_normal_equations_close(ds.accumulate6(R, ts, loss), oracle.ndt6_accumulate(planes, R, ts, loss),
                                                  6, 1e-10 if dtype == "f64" else 3e-6)
        _, _, rep = ds.solve6(R, t, loss, max_iterations=1)
        _kernel(ctx, "solve_cluster_kernel<nos::Ndt6Problem<%s" % T, ", 3, 3, 0," if dtype == "f64" else ", 3, 4, 0,")
        check(rep["cost_history"][0], ref, base, 6, dtype, "resident solve6 " + what, cost_only=True)
    # the 3-DoF problem on its own family (offsets in x, y)
    planes3, _, t3, _ = _rounded_case(fam, n, dtype, three=True)
    R2 = _round(E.R2_TEST, dtype)
    ds3 = NdtDataset.from_planes(ctx, planes3, dtype)
    for loss in LOSSES:
        what = "%s %s" % (_fid(fam), loss and loss[0])
        ref, base = refs3(planes3, R2, t3, loss, dtype)
        got = ds3.accumulate3(R2, t3, loss)
        _kernel(ctx, "assemble_kernel<nos::Ndt3Problem<%s" % T)
        check(got, ref, base, 3, dtype, "accumulate3 " + what)
        if _benign(fam):
            ts = _round(t3 + T_SHIFT[:2], dtype)
            helpers.assert_normal_equations_close(ds3.accumulate3(R2, ts, loss),
                                                  oracle.ndt3_accumulate(planes3, R2, ts, loss), 3,
                                                  1e-10 if dtype == "f64" else 3e-6)
        _, _, rep = ds3.solve3(R2, t3, loss, max_iterations=1)
        _kernel(ctx, "solve_cluster_kernel<nos::Ndt3Problem<%s" % T)
        check(rep["cost_history"][0], ref, base, 3, dtype, "resident solve3 " + what, cost_only=True)
    ds3.close()
    ds.close()
    # single-workgroup solve: the first 1000 correspondences
    head = np.ascontiguousarray(planes[:, :1000])
    small = NdtDataset.from_planes(ctx, head, dtype)
    for loss in LOSSES:
        ref, base = refs6(head, R, t, loss, dtype)
        _, _, rep = small.solve6(R, t, loss, max_iterations=1)
        _kernel(ctx, "solve_single_block_kernel<nos::Ndt6Problem<%s" % T)
        check(rep["cost_history"][0], ref, base, 6, dtype, "single-workgroup solve6 %s %s" % (_fid(fam), loss and loss[0]),
              cost_only=True)
    small.close()
    # voxel-indexed layout: the same correspondences as points + voxel ids + a table built from the fp64 S (the reference
    # and the numpy S form take S as the flat planes hold it)
    ids = NdtIndexedDataset.from_arrays(ctx, _round(pts, dtype), vid[None, :], _round(means, dtype), S, dtype)
    for loss in LOSSES:
        ref, base = refs[loss]
        got = ids.accumulate6(R, t, loss)  # assemble_indexed_kernel (not recorded by nos_ctx_last_kernel)
        check(got, ref, base, 6, dtype, "indexed accumulate6 %s %s" % (_fid(fam), loss and loss[0]))
    ids.close()
    # two shards on one device
    c2 = Context((0, 0))
    sh = NdtDataset.from_planes(c2, planes, dtype)
    for loss in LOSSES:
        ref, base = refs[loss]
        got = sh.accumulate6(R, t, loss)
        _kernel(c2, "assemble_kernel<nos::Ndt6Problem<%s" % T, shard=1)
        check(got, ref, base, 6, dtype, "2 shards accumulate6 %s %s" % (_fid(fam), loss and loss[0]))
    sh.close()
    c2.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_streamed_one_launch_solve_at_kappa_1e3(ctx, dtype):
    """1 000 003 correspondences: beyond the resident capacity of either dtype, so the one-launch solve streams them."""
    T = "double" if dtype == "f64" else "float"
    planes, R, t, _ = _rounded_case(dict(kappa=1e3, shape="planar", e_mode="plane"), 1_000_003, dtype, seed=21)
    ds = NdtDataset.from_planes(ctx, planes, dtype)
    ref, base = refs6(planes, R, t, HUBER, dtype)
    got = ds.accumulate6(R, t, HUBER)
    check(got, ref, base, 6, dtype, "1M accumulate6 kappa=1e3 huber")
    _, _, rep = ds.solve6(R, t, HUBER, max_iterations=1)
    _kernel(ctx, "solve_cluster_kernel<nos::Ndt6Problem<%s" % T, ", 0, 0, 1," if dtype == "f64" else ", 0, 0, 2,")
    check(rep["cost_history"][0], ref, base, 6, dtype, "1M streamed solve6 kappa=1e3 huber", cost_only=True)
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_huber_branch_edges(ctx, dtype):
    """s at th², th² ± a few ulps and out to 1e20 th²: the weight is continuous across the branch."""
    th = 1.25
    planes, (R, t) = E.huber_edge_case(20_000, th, seed=4)
    planes, R, t = _round(planes, dtype), _round(R, dtype), _round(t, dtype)
    ds = NdtDataset.from_planes(ctx, planes, dtype)
    ref, base = refs6(planes, R, t, ("huber", th), dtype)
    check(ds.accumulate6(R, t, ("huber", th)), ref, base, 6, dtype, "huber edges")
    ds.close()


def test_fast_rsqrt_holds_to_a_few_ulps_over_the_huber_range(ctx):
    """One correspondence, S = I, e = (a, 0, 0) exactly: s = a², the Huber weight w = th · rsqrt(s) (fast_rsqrt<double>), so
    g₀ = w a = th and cost = 2 th a − th²; a from th to 1e10 th (s to 1e20 th²) and just around th."""
    th = 1.25
    ulp = 2.0 ** -52
    for a in [th * (1 + k * ulp) for k in range(-3, 4)] + list(th * 10.0 ** np.linspace(0.0, 10.0, 41)):
        planes = np.zeros((15, 1))
        planes[3, 0] = -a
        planes[6, 0] = planes[10, 0] = planes[14, 0] = 1.0
        ds = NdtDataset.from_planes(ctx, planes, "f64")
        out = ds.accumulate6(np.eye(3), np.zeros(3), ("huber", th))
        ds.close()
        s = a * a
        if s > th * th:
            assert abs(out[21] - th) <= 4 * ulp * th, (a, out[21])
            want = 2 * th * np.sqrt(np.longdouble(s)) - th * th
            assert abs(np.longdouble(out[27]) - want) <= 4 * ulp * want, (a, out[27], want)
        else:
            assert out[21] == a and out[27] == s, (a, out[21], out[27])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_exponential_loss_to_underflow(ctx, dtype):
    """c2·s from 1e-8 to 2000: the weights run into exp underflow (fp64 past ≈ 745, fp32 past ≈ 104)."""
    loss = ("exponential", 2.0, 0.5)
    planes, (R, t) = E.exponential_edge_case(20_000, 0.5, seed=6)
    planes, R, t = _round(planes, dtype), _round(R, dtype), _round(t, dtype)
    ds = NdtDataset.from_planes(ctx, planes, dtype)
    ref, base = refs6(planes, R, t, loss, dtype)
    check(ds.accumulate6(R, t, loss), ref, base, 6, dtype, "exponential to underflow")
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["mixed", "threshold"])
def test_reprojection_edges(ctx, oracle, kind, dtype):
    """Points in front of and behind the camera, pixels out to ±1e4, and the exact depth-threshold case (identity pose,
    z = min_depth: counted); per-pass, resident and single-workgroup forms."""
    T = "double" if dtype == "f64" else "float"
    min_depth = float(_round(E.MIN_DEPTH, dtype))
    for n in (20_000, 1000):
        planes, (R, t), intr = E.reproj_case(n, kind, seed=8)
        planes, R, t = _round(planes, dtype), _round(R, dtype), _round(t, dtype)
        intr = tuple(float(_round(v, dtype)) for v in intr)
        ds = ReprojDataset.from_planes(ctx, planes, dtype)
        for loss in (None, ("huber", 0.0078125)):  # 2^-7 ≈ 4 px in normalised coordinates
            ref = xp.reproj_accumulate(planes, R, t, intr, loss, min_depth)
            base = (xp.reproj_accumulate(planes, R, t, intr, loss, min_depth, dtype=NP_DTYPE[dtype]),)
            what = "reprojection %s n=%d %s" % (kind, n, loss and loss[0])
            if n > 1024:
                got = ds.accumulate(R, t, intr, loss, min_depth)
                _kernel(ctx, "assemble_kernel<nos::ReprojProblem<%s" % T)
                check(got, ref, base, 6, dtype, "accumulate " + what)
            _, _, rep = ds.solve(R, t, intr, loss, min_depth, max_iterations=1)
            _kernel(ctx, "solve_cluster_kernel<nos::ReprojProblem<%s" % T if n > 1024 else
                    "solve_single_block_kernel<nos::ReprojProblem<%s" % T)
            check(rep["cost_history"][0], ref, base, 6, dtype, "solve " + what, cost_only=True)
        ds.close()
    if kind == "threshold":  # every other point sits exactly at min_depth: counted (!(z < min_depth)), the rest not
        planes, (R, t), intr = E.reproj_case(10, kind)
        ds = ReprojDataset.from_planes(ctx, planes, "f64")
        H, _, _ = helpers.unpack(ds.accumulate(R, t, intr, None, E.MIN_DEPTH), 6)
        assert H[0, 0] == pytest.approx(5 / E.MIN_DEPTH ** 2, rel=1e-15)
        ds.close()


@pytest.mark.parametrize("dtype,offset", [("f64", dict(offset=1e3, offset_in="pose")), ("f32", dict(offset=10.0))],
                         ids=["f64-pose-1e3", "f32-map-10"])
@pytest.mark.parametrize("kappa", [1e2, 1e3])
def test_lm_solve_at_high_kappa_with_an_offset(ctx, oracle, kappa, dtype, offset):
    """The whole LM loop at κ = 1e2 / 1e3 from a start 1 cm / 1 mrad off: the fp64 oracle's loop on the same (fp32-rounded)
    inputs, to the suite's pose tolerances, in as many iterations.  fp64: sensor pose and map 1 km from the origin.  fp32:
    map frame 10 m from the origin — fp32 resolves 1 km to 6e-5 m, which moves e (1e-2 … 1e-1 m) by more than the loop's
    tolerances allow, whatever the arithmetic form (measured: the oracle stops after 38 iterations, fp32 runs to 50)."""
    planes, R_true, t_true, _ = _rounded_case(dict(kappa=kappa, **offset), 50_000, dtype, seed=31)
    R0 = _round(R_true @ helpers.rot_xyz(1e-3, -1e-3, 1e-3), dtype)
    t0 = _round(t_true + np.array([1e-2, -1e-2, 5e-3]), dtype)
    want = oracle.ndt6_solve(planes, t0, R0, loss=None, max_iterations=50, linear_solver=1)
    ds = NdtDataset.from_planes(ctx, planes, dtype)
    R, t, rep = ds.solve6(R0, t0, None, max_iterations=50)
    ds.close()
    assert rep["ok"] and rep["iterations"] == want["iterations"], (rep["iterations"], want["iterations"])
    dt, dq = helpers.pose_delta(R.reshape(3, 3), t, want["R"], want["t"])
    _log(what="lm kappa=%g %s" % (kappa, offset), dtype=dtype, dt=dt, dq=dq, iterations=rep["iterations"])
    if dtype == "f64":
        assert dt < 1e-9 and dq < 1e-9, (dt, dq)
    else:
        assert dt < 2e-7 and dq < 1e-8, (dt, dq)
