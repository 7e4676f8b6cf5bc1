"""Pose-graph linearisation and product on exact-integer graphs: every quaternion from {+-1, +-i, +-j, +-k} (rotation
entries 0 and +-1, quaternion products exact), integer positions and offsets in +-8, switch values from {1, 2, 0.5}, free
switches at s = 1 only (prior term exactly 0).  Every term of every sum is a multiple of 1/16 far below 2^53, so float64
adds them without rounding IN ANY ORDER and with or without fused multiply-adds: cost, |gradient|, gradient, the 21
planes of the diagonal blocks and the product must equal the int64 reference bit for bit, under both product forms —
at 256 and 257 poses (a full block; one pose past it), 65 537 (257 workgroups of the linearisation) and 787 493 =
256 * 3076 + 37 poses: 3077 block partials, the fewest at which lanes 0-4 of pgo_sum_rows run the four-accumulator loop
while the other lanes run the left-over loop, with a partly filled last block."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle_pgo as op
from tests import pgo_hard_inputs as hi

Q8 = np.array([[1, 0, 0, 0], [-1, 0, 0, 0], [0, 1, 0, 0], [0, -1, 0, 0],
               [0, 0, 1, 0], [0, 0, -1, 0], [0, 0, 0, 1], [0, 0, 0, -1]], dtype=np.int64)
LIMIT = 2 ** 53


def exact_graph(n, seed=0):
    """→ state dict (layout of pgo_hard_inputs) with integer-valued float64 arrays"""
    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 7))
    walk = np.cumsum(rng.integers(-2, 3, size=(n, 3)), axis=0)
    v = np.mod(walk + 8, 32)                                   # the walk reflected at +-8
    poses[:, :3] = np.where(v <= 16, v, 32 - v) - 8
    poses[:, 3:] = Q8[rng.integers(8, size=n)]
    i = np.arange(n)
    j = i[:, None] + rng.integers(2, 40, size=(n, 2))
    ref = np.concatenate([i[:-1], np.repeat(i, 2)[j.ravel() < n]])
    qry = np.concatenate([i[1:], j.ravel()[j.ravel() < n]])
    m = ref.size
    meas = np.zeros((m, 7))
    meas[:, :3] = rng.integers(-8, 9, size=(m, 3))
    meas[:, 3:] = Q8[rng.integers(8, size=m)]
    sw = np.array([1.0, 2.0, 0.5])[rng.integers(3, size=m)]
    free = ((sw == 1.0) & (rng.integers(3, size=m) == 0)).astype(np.uint8)
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[[0, n // 2]] = 1
    x = rng.integers(-4, 5, size=6 * n + m).astype(np.float64)
    x[6 * n:][free == 0] = 0.0
    for k in range(6):
        x[k * n + np.nonzero(fixed)[0]] = 0.0
    return {"poses": poses, "ref": ref.astype(np.int32), "qry": qry.astype(np.int32), "meas": meas, "sw": sw, "free": free,
            "fixed": fixed, "x": x}


def _i64(a):
    a = np.asarray(a)
    out = a.astype(np.int64)
    assert np.array_equal(out, a)
    return out


def exact_reference(st, lambdas):
    """int64 throughout, values scaled to integers: cost x 4, gradient x 4, diagonal blocks x 4, product x 16 (4 lambda
    must be an integer).  The one float64 piece is the switch curvature |r|^2 + 1e-18 of the switch rows of the product,
    formed as the kernels form it: it equals |r|^2 unless that is 0, and then its row is a chain of products without a sum.
    → dict of float64 arrays, and the largest sum of magnitudes met (to be held against 2^53)"""
    n, m = st["poses"].shape[0], st["ref"].size
    ref, qry = st["ref"].astype(np.int64), st["qry"].astype(np.int64)
    free, fixed = st["free"].astype(bool), st["fixed"].astype(bool)
    r, A, B, C = hi._edge_terms(st, _i64, -1)
    r = np.stack(r, axis=1)
    A, B, C = (np.stack([np.stack(row, axis=1) for row in M], axis=1) for M in (A, B, C))
    s4, s2 = _i64(4 * st["sw"] * st["sw"]), _i64(2 * st["sw"])
    assert np.all(st["sw"][free] == 1.0)
    keep_r, keep_q = ~fixed[ref], ~fixed[qry]
    S_r = sp.csr_matrix((keep_r.astype(np.int64), (ref, np.arange(m))), shape=(n, m))
    S_q = sp.csr_matrix((keep_q.astype(np.int64), (qry, np.arange(m))), shape=(n, m))
    degree = int(np.max(np.bincount(ref, minlength=n) + np.bincount(qry, minlength=n)))
    largest = [0]

    def gather(at_r, at_q):           # [m, k] int64 per end -> [n, k]: the owner's sum over its constraints
        largest[0] = max(largest[0], degree * int(max(np.max(np.abs(at_r)), np.max(np.abs(at_q)))))
        return S_r @ at_r + S_q @ at_q

    def mv(M, v):                     # [m,3,3] [m,3] -> M v
        return (M * v[:, None, :]).sum(2)

    def mtv(M, v):                    # -> M^T v
        return (M * v[:, :, None]).sum(1)

    def mtm(M):                       # -> M^T M
        return (M[:, :, :, None] * M[:, :, None, :]).sum(1)

    # J_r = [-I A; 0 B], J_q = [I 0; 0 C]
    def J_r(u):
        return np.concatenate([mv(A, u[:, 3:]) - u[:, :3], mv(B, u[:, 3:])], axis=1)

    def J_q(u):
        return np.concatenate([u[:, :3], mv(C, u[:, 3:])], axis=1)

    def JT_r(v):
        return np.concatenate([-v[:, :3], mtv(A, v[:, :3]) + mtv(B, v[:, 3:])], axis=1)

    def JT_q(v):
        return np.concatenate([v[:, :3], mtv(C, v[:, 3:])], axis=1)

    rr = np.sum(r * r, axis=1)
    out = {"cost": float(np.sum(s4 * rr)) / 4.0}
    g4 = gather(s4[:, None] * JT_r(r), s4[:, None] * JT_q(r))
    gs = np.where(free, rr, 0)
    sumsq = int(np.sum(g4 * g4)) + 16 * int(np.sum(gs * gs))
    largest[0] = max(largest[0], int(np.sum(s4 * rr)), sumsq)
    out["gnorm"] = float(np.sqrt(np.float64(sumsq) / 16.0))
    out["gradient"] = np.concatenate([g4.T.reshape(-1) / 4.0, gs.astype(np.float64)])
    iu = np.triu_indices(6)
    Hr, Hq = np.zeros((m, 6, 6), dtype=np.int64), np.zeros((m, 6, 6), dtype=np.int64)
    Hr[:, :3, :3], Hr[:, :3, 3:], Hr[:, 3:, 3:] = np.eye(3, dtype=np.int64), -A, mtm(A) + mtm(B)
    Hq[:, :3, :3], Hq[:, 3:, 3:] = np.eye(3, dtype=np.int64), mtm(C)
    h4 = gather(s4[:, None] * Hr[:, iu[0], iu[1]], s4[:, None] * Hq[:, iu[0], iu[1]])
    del Hr, Hq
    diag = [0, 6, 11, 15, 18, 20]
    h4[np.ix_(fixed, diag)] = 4
    out["hdiag"] = (h4.T / 4.0).reshape(-1)
    x = _i64(st["x"])
    X = x[:6 * n].reshape(6, n).T                                # [n, 6]
    xs = np.where(free, x[6 * n:], 0)
    xr, xq = np.where(fixed[ref][:, None], 0, X[ref]), np.where(fixed[qry][:, None], 0, X[qry])
    u = J_r(xr) + J_q(xq)
    v2 = s2[:, None] * u + 2 * r * xs[:, None]
    y4 = gather(s2[:, None] * JT_r(v2), s2[:, None] * JT_q(v2))
    acc = np.sum(r * u, axis=1)                                   # switch rows, free switches only: s = 1
    h_s = rr.astype(np.float64) + op.C_SWITCH * op.C_SWITCH
    out["product"] = {}
    for lam in lambdas:
        lam4 = int(round(4 * lam))
        assert lam4 == 4 * lam
        y16 = 4 * y4 + lam4 * h4[:, diag] * X
        y16[fixed] = (16 + 4 * lam4) * X[fixed]
        largest[0] = max(largest[0], int(np.max(np.abs(y16))))
        ys = np.where(free, acc.astype(np.float64) + h_s * (1.0 + lam) * xs.astype(np.float64), 0.0)
        out["product"][lam] = np.concatenate([y16.T.reshape(-1) / 16.0, ys])
    return out, largest[0]


def test_the_int64_reference_is_the_oracle_on_a_small_exact_graph():
    """CPU: the explicit float64 assembly of oracle_pgo is exact on such a graph too."""
    st = exact_graph(60, seed=3)
    want, largest = exact_reference(st, (0.0, 0.25))
    got = hi.oracle_quantities(st, st["x"], (0.0, 0.25))
    assert largest < LIMIT and np.sum(st["free"]) > 10 and set(st["sw"].tolist()) == {1.0, 2.0, 0.5}
    assert got["cost"] == want["cost"] and want["cost"] > 0
    assert np.array_equal(np.concatenate([got["gradient"], got["switch_gradient"]]), want["gradient"])
    assert np.array_equal(got["hdiag"].reshape(-1), want["hdiag"])
    for lam in (0.0, 0.25):
        assert np.array_equal(np.concatenate([got["product"][lam], got["switch_product"][lam]]), want["product"][lam])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [256, 257, 65_537, 787_493])
def test_exact_integer_graph_bit_for_bit(ctx, n):
    from nonlinear_optimizer_for_slam_amd import pgo
    t0 = time.perf_counter()
    st = exact_graph(n, seed=n)
    lambdas = (0.0, 0.25)
    want, largest = exact_reference(st, lambdas)
    assert largest < LIMIT, largest
    assert (n + 255) // 256 == {256: 1, 257: 2, 65_537: 257, 787_493: 3077}[n]
    t_ref = t1 = time.perf_counter()
    for block in (0, 1):
        with ctx.options(pgo_block=block):
            g = pgo.PoseGraph(ctx, st["poses"], st["ref"], st["qry"], st["meas"], st["sw"], st["free"], st["fixed"])
        t2 = time.perf_counter()
        assert (g.layout_info()["block_poses"] != 0) == (block != 0)
        cost, gnorm = g.linearize()
        assert cost == want["cost"] and gnorm == want["gnorm"], (cost, want["cost"], gnorm, want["gnorm"])
        assert np.array_equal(g.vector("gradient"), want["gradient"])
        assert np.array_equal(g.vector("hdiag"), want["hdiag"])
        for lam in lambdas:
            assert np.array_equal(g.matvec(lam, st["x"]), want["product"][lam]), (block, lam)
        g.close()
        print("  n = %d block = %d: graph creation %.2f s, checks %.2f s" % (n, block, t2 - t1, time.perf_counter() - t2))
        t1 = time.perf_counter()
    print("  n = %d: inputs and int64 reference %.2f s, whole test %.2f s" % (n, t_ref - t0, time.perf_counter() - t0))
