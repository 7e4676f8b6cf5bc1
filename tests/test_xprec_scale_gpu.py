"""Full-size sums against the extended-precision reference (oracle/oracle_xp.py) at the sizes the kernels are built for:
10 M and 80 M correspondences per pass, the streamed one-launch solve and the indexed layout at 10 M, reprojection at
BASELINE.json configs[2]'s 2 M and at 10 M.

The datasets tile a prime period of P correspondences (P does not divide any chunk, tile or grid stride), so the
reference of n = K·P + r items is K·S_P + S_r from one longdouble pass over the period (oracle_xp.tiled_sums), with
Σ|term| alike.  Two families, fp32-rounded for fp32 as in tests/test_xprec_gpu.py: benign data (κ(S) = 10), and planar
voxels at κ = 1e3 with points on the plane and the sensor 1 km from the origin; the three losses.

Criterion, per quantity q (H against sqrt(H_ii H_jj), g against sqrt(H_ii · cost), the cost relatively):

    err_q ≤ C · eb_P + FLOOR[dtype] + (k_lane · u_T + ⌈log2 n⌉ · u_64) · ρ_q,     C = 4, FLOOR = 16 u

— test_xprec_gpu's criterion on one period (eb_P: the numpy S form in the kernel's dtype against the reference), plus the
a-priori bound of the kernel's own summation order: k_lane sequential adds in the storage type per lane (u_T), then a
fp64 tree over the lanes and workgroups; ρ_q = Σ|term_q| / scale_q.  k_lane is the busiest lane's item count of the launch
that ran (its template arguments, the grid rule and the CU count: tests/exact_inputs.py; pinned in
tests/test_exact_inputs.py).  At 10 M in fp32 the kernel's error is also held to that of the reference's fp32 ("SIMD")
class's order on the benign family: 8 lanes of n/8 sequential fp32 adds — DESIGN.md §3's claim.  NOS_XPREC_LOG records every comparison
(profiles/xprec_errors.md, "Full size").
"""
import math

import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import NdtDataset, NdtIndexedDataset, ReprojDataset
from oracle import oracle_xp as xp
from tests import edge_inputs as E
from tests import exact_inputs as X
from tests.test_xprec_gpu import C, FLOOR, LOSSES, NP_DTYPE, _log, _round

pytestmark = pytest.mark.gpu

P = 199_999  # prime
U = {"f64": 2.0 ** -53, "f32": 2.0 ** -24}
ES = {"f64": 8, "f32": 4}
T_NAME = {"f64": "double", "f32": "float"}
FAMILIES = {"benign": dict(kappa=10.0, shape="planar", e_mode="iso"),
            "planar-k1e3-pose-1km": dict(kappa=1e3, shape="planar", e_mode="plane", offset=1e3, offset_in="pose")}
K = X.library_constants()
_CACHE = {}


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _period(fam, dtype, three=False):
    key = ("period", fam, dtype, three)
    if key not in _CACHE:
        planes, (R, t), vox = (E.ndt3_case if three else E.ndt_case)(P, seed=17, **FAMILIES[fam])
        if three:
            R = E.R2_TEST
        _CACHE[key] = (_round(planes, dtype), _round(R, dtype), _round(t, dtype), vox)
    return _CACHE[key]


def _reference(kind, fam, dtype, loss):
    """(per-item longdouble terms of the period, eb_P = the numpy S form's (H, g, cost) errors on the period)."""
    key = (kind, fam, dtype, loss)
    if key not in _CACHE:
        d = NP_DTYPE[dtype]
        if kind == "reproj":
            planes, R, t, intr = _reproj_period(dtype)
            args = (R, t, intr, loss, E.MIN_DEPTH)
            fn, dim, orders = xp.reproj_accumulate, 6, ({},)
        else:
            planes, R, t, _ = _period(fam, dtype, three=kind == "ndt3")
            args = (R, t, loss)
            fn, dim = (xp.ndt3_accumulate, 3) if kind == "ndt3" else (xp.ndt6_accumulate, 6)
            orders = ({}, {"order": "fma"})
        terms = fn(planes, *args, terms=True)
        ref = xp.period_sums(terms)[0]
        eb = [xp.scaled_errors(fn(planes, *args, dtype=d, **o), ref, dim) for o in orders]
        _CACHE[key] = (terms, tuple(max(e[k] for e in eb) for k in range(3)))
    return _CACHE[key]


def _reproj_period(dtype):
    key = ("reproj period", dtype)
    if key not in _CACHE:
        planes, (R, t), intr = E.reproj_case(P, "mixed", seed=8)
        _CACHE[key] = (_round(planes, dtype), _round(R, dtype), _round(t, dtype),
                       tuple(float(_round(v, dtype)) for v in intr))
    return _CACHE[key]


def _tile(planes, n):
    reps = -(-n // planes.shape[1])
    return np.ascontiguousarray(np.tile(planes, reps)[:, :n])


def entry_errors(got, ref, mag, dim):
    """Per packed entry: (|got − ref| / scale, Σ|term| / scale, group 0 = H | 1 = g | 2 = cost)."""
    ref = np.asarray(ref, dtype=xp.LD)
    H, _, cost = xp.unpack(ref, dim)
    d = np.sqrt(np.maximum(np.diag(H), xp.LD(0)))
    tri = X.TRI6 if dim == 6 else X.TRI3
    scale = [d[r] * d[c] for r, c in tri] + [d[i] * np.sqrt(abs(cost)) for i in range(dim)] + [abs(cost)]
    scale = np.maximum(np.array(scale, dtype=xp.LD), xp.LD(1e-300))
    err = np.abs(np.asarray(got, dtype=np.float64).astype(xp.LD) - ref) / scale
    group = np.array([0] * len(tri) + [1] * dim + [2])
    return err.astype(np.float64), (np.asarray(mag, dtype=xp.LD) / scale).astype(np.float64), group


def check(got, kind, fam, dtype, loss, n, k_lane, what, cost_only=False):
    """The criterion of the module docstring; returns the worst err / bound."""
    dim = 3 if kind == "ndt3" else 6
    terms, eb = _reference(kind, fam, dtype, loss)
    ref, mag = xp.tiled_sums(terms, n)
    if cost_only:
        got_full = np.asarray(ref, dtype=np.float64).copy()
        got_full[-1] = float(np.asarray(got).reshape(-1)[0])
        got = got_full
    err, rho, group = entry_errors(got, ref, mag, dim)
    bound = C * np.array(eb)[group] + FLOOR[dtype] + (k_lane * U[dtype] + math.ceil(math.log2(n)) * U["f64"]) * rho
    sel = slice(len(err) - 1, None) if cost_only else slice(None)
    ratio = float(np.max(err[sel] / bound[sel]))
    _log(what="full size " + what, dtype=dtype, n=n, k_lane=k_lane, gpu=[float(np.max(err[sel][group[sel] == g], initial=0))
                                                                         for g in range(3)],
         numpy_s_form_period=list(eb), rho_max=float(np.max(rho[sel])), ratio=ratio, cost_only=cost_only)
    worst = int(np.argmax(err[sel] / bound[sel]))
    assert ratio <= 1.0, "%s %s n=%d: entry %d error %.3e > bound %.3e (eb %s, k_lane %d, rho %.3e)" % (
        what, dtype, n, worst, err[sel][worst], bound[sel][worst], eb, k_lane, rho[sel][worst])
    return ratio


def _pass_k(ctx, n, cus):
    return X.pass_items_per_lane(n, X.assemble_geometry(ctx.last_kernel()), K, cus)


def _simd_order_errors(kind, fam, dtype, loss, n):
    """(H, g, cost) errors of the reference fp32 class's order: per-item fp32 terms, 8 lanes of n/8 sequential fp32 adds
    (np.cumsum along each lane), then the 8 lanes added in fp32."""
    planes, R, t, _ = _period(fam, dtype)
    t32 = xp.ndt6_accumulate(planes, R, t, loss, dtype=np.float32, terms=True)
    assert n % 8 == 0
    out = np.zeros(t32.shape[0])
    for q in range(t32.shape[0]):
        lanes = np.cumsum(_tile(t32[q:q + 1], n).reshape(n // 8, 8), axis=0, dtype=np.float32)[-1]
        acc = np.float32(0)
        for v in lanes:
            acc = np.float32(acc + v)
        out[q] = acc
    terms, _ = _reference(kind, fam, dtype, loss)
    return xp.scaled_errors(out, xp.tiled_sums(terms, n)[0], 6)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_ndt_at_ten_million(ctx, cus, fam, dtype):
    """accumulate6 / accumulate3 per pass, the streamed one-launch solve's first cost and the indexed layout at 10 M;
    fp32 per pass also against the reference fp32 class's summation order."""
    n = 10_000_000
    planes, R, t, (pts, vid, means, S) = _period(fam, dtype)
    ds = NdtDataset.from_planes(ctx, _tile(planes, n), dtype)
    for loss in LOSSES:
        got = ds.accumulate6(R, t, loss)
        k = _pass_k(ctx, n, cus)
        check(got, "ndt6", fam, dtype, loss, n, k, "accumulate6 %s %s" % (fam, loss and loss[0]))
        if dtype == "f32" and fam == "benign":  # where the per-item arithmetic is not what dominates the error
            mine = xp.scaled_errors(got, xp.tiled_sums(_reference("ndt6", fam, dtype, loss)[0], n)[0], 6)
            simd = _simd_order_errors("ndt6", fam, dtype, loss, n)
            _log(what="full size simd-order accumulate6 %s %s" % (fam, loss and loss[0]), dtype=dtype, n=n, k_lane=k,
                 gpu=mine, simd_order=simd)
            assert all(a <= b for a, b in zip(mine, simd)), (mine, simd)
        _, _, rep = ds.solve6(R, t, loss, max_iterations=1)
        g = X.cluster_geometry(ctx.last_kernel())
        form, ks = X.solve_items_per_lane(n, 15, ES[dtype], K, cus)
        assert form == "streamed" and g["SI"] == K["stream_items"][ES[dtype]] and g["RI"] == 0, ctx.last_kernel()
        check(rep["cost_history"][:1], "ndt6", fam, dtype, loss, n, ks, "streamed solve6 %s %s" % (fam, loss and loss[0]),
              cost_only=True)
    ds.close()
    # the indexed layout: the period's points and voxel ids tiled over one voxel table
    ids = NdtIndexedDataset.from_arrays(ctx, _tile(_round(pts, dtype), n), _tile(vid[None, :], n), _round(means, dtype),
                                        S, dtype)
    chunks = -(-n // K["indexed_block"][ES[dtype]])  # one item per lane per chunk, grid-strided
    k_idx = -(-chunks // min(chunks, ctx.get_option("indexed_bpc") * cus, K["max_partial_rows"]))
    for loss in LOSSES:
        check(ids.accumulate6(R, t, loss), "ndt6", fam, dtype, loss, n, k_idx, "indexed accumulate6 %s %s" % (fam, loss and loss[0]))
    ids.close()
    planes3, R2, t2, _ = _period(fam, dtype, three=True)
    ds3 = NdtDataset.from_planes(ctx, _tile(planes3, n), dtype)
    for loss in LOSSES:
        got = ds3.accumulate3(R2, t2, loss)
        check(got, "ndt3", fam, dtype, loss, n, _pass_k(ctx, n, cus), "accumulate3 %s %s" % (fam, loss and loss[0]))
    ds3.close()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_ndt_accumulate6_at_eighty_million(ctx, cus, fam, dtype):
    """BASELINE.json configs[3]'s size in one dataset: per-pass accumulate6, ≈ 600 items per fp32 lane."""
    n = 80_000_000
    planes, R, t, _ = _period(fam, dtype)
    ds = NdtDataset.from_planes(ctx, _tile(planes, n), dtype)
    for loss in LOSSES:
        got = ds.accumulate6(R, t, loss)
        check(got, "ndt6", fam, dtype, loss, n, _pass_k(ctx, n, cus), "accumulate6 %s %s" % (fam, loss and loss[0]))
    ds.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [2_000_000, 10_000_000])
def test_reprojection_at_full_size(ctx, cus, n, dtype):
    """Reprojection per pass (ping-pong kernel) and the one-launch solve's first cost (resident at 2 M, streamed at
    10 M): points in front of and behind the camera, pixels to ±1e4."""
    planes, R, t, intr = _reproj_period(dtype)
    ds = ReprojDataset.from_planes(ctx, _tile(planes, n), dtype)
    for loss in (None, ("huber", 0.0078125)):
        got = ds.accumulate(R, t, intr, loss, E.MIN_DEPTH)
        check(got, "reproj", None, dtype, loss, n, _pass_k(ctx, n, cus), "reprojection accumulate %s" % (loss and loss[0]))
        _, _, rep = ds.solve(R, t, intr, loss, E.MIN_DEPTH, max_iterations=1)
        form, ks = X.solve_items_per_lane(n, 5, ES[dtype], K, cus)
        assert ("solve_cluster_kernel<nos::ReprojProblem<%s" % T_NAME[dtype]) in ctx.last_kernel()
        check(rep["cost_history"][:1], "reproj", None, dtype, loss, n, ks, "reprojection %s solve %s" % (form, loss and loss[0]),
              cost_only=True)
    ds.close()
