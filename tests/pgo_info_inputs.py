"""Pose graphs whose constraints carry a 6x6 information matrix — TEST INFRASTRUCTURE shared by
test_pgo_information_host.py (CPU), test_pgo_information.py and test_pgo_information_pipeline.py (GPU); DESIGN.md §33.

The rule (include/nos.h, nos_pgo_create_weighted), restated twice:
  * InfoGraph — numpy, on top of oracle_pgo's qrot / qmul / hat / Graph: residual r~ = (R_r^T (p_q - p_r) - t_m, r_R),
    Jacobians [-R_r^T | [u]x ; 0 | B] and [R_r^T | 0 ; 0 | C], Omega' = D Omega D, explicit sparse H, g, cost; the damped
    solve, the retraction and the LM loop are Graph's own.  `mutate` plants the two mistakes the sign-convention test
    must catch ("no_D": Omega used as it stands; "world_rt": the world-frame r_t of the unweighted kernels);
  * reference() — the same formulas over a number type and a sign, as tests/pgo_hard_inputs.py does it for the unweighted
    kernels: mpmath at 50 digits (sign -1) and the first-order error SCALE (float64, every operand replaced by its
    absolute value, every subtraction by an addition).
Error of a float64 result = |got - reference| / scale in units of 2^-52 (pgo_hard_inputs.error_eps).  The yardstick e_np is
InfoGraph's own error in that measure; the device may err up to max(4 e_np, 8) units (the convention of
test_pgo_xprec_gpu.py and DESIGN.md §26).  Nothing in a bound comes from the code under test.

Every case is built once per process and then left unchanged."""
import functools

import mpmath
import numpy as np
import scipy.sparse as sp

from oracle import oracle_pgo as op
from tests import pgo_cases
from tests import pgo_hard_inputs as hi

LAMBDAS = (0.0, 1e-3)
CASES = ("chain13", "two_groups", "two_level")
AGG = {"chain13": 3, "two_groups": 3, "two_level": 3}   # pgo_agg; the coarse level takes part from 4 aggregates on
QUANTITIES = ("cost", "gradient", "switch_gradient", "hdiag", "product", "switch_product")
D = np.diag([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])
UPPER = hi._UPPER
DIAG = hi._DIAG


# ---------------------------------------------------------------- information matrices

def draw_information(m, seed):
    """[m, 6, 6]: Q^T diag(10^U[-2, 4]) Q with a seeded orthogonal Q; every fifth matrix has one eigenvalue exactly 0
    (the direction a corridor does not observe).  Symmetric to the bit."""
    rng = np.random.default_rng(seed)
    out = np.zeros((m, 6, 6))
    for e in range(m):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        lam = 10.0 ** rng.uniform(-2.0, 4.0, size=6)
        if e % 5 == 0:
            lam[int(rng.integers(6))] = 0.0
        A = Q.T @ np.diag(lam) @ Q
        out[e] = 0.5 * (A + A.T)
    return out


def upper21(information):
    a = np.asarray(information, dtype=np.float64).reshape(-1, 6, 6)
    return np.ascontiguousarray(a[:, np.triu_indices(6)[0], np.triu_indices(6)[1]])


# ---------------------------------------------------------------- numpy restatement

def weighted_residual(pr, qr, pq, qq, tm, qm, mutate=()):
    """r~ (6) and e = q_q^* q_r q_m"""
    Rr = op.qrot(qr)
    u = Rr.T @ (pq - pr)
    e = op.qmul(op.qmul(op.qconj(qq), qr), qm)
    rt = (pq - pr) - Rr @ tm if "world_rt" in mutate else u - tm
    return np.concatenate([rt, 2.0 * e[1:]]), e, u


def weighted_jacobians(qr, qm, e, u):
    """(J~_r, J~_q): 6x6 each, w.r.t. (dp, dw) with p <- p + dp, q <- q (x) Exp(dw)."""
    Rt = op.qrot(qr).T
    Jr, Jq = np.zeros((6, 6)), np.zeros((6, 6))
    Jr[:3, :3] = -Rt
    Jr[:3, 3:] = op.hat(u)
    Jr[3:, 3:] = (e[0] * np.eye(3) + op.hat(e[1:])) @ op.qrot(qm).T
    Jq[:3, :3] = Rt
    Jq[3:, 3:] = -e[0] * np.eye(3) + op.hat(e[1:])
    return Jr, Jq


class InfoGraph(op.Graph):
    """oracle_pgo.Graph with one information matrix per constraint: cost and linearize restated, the rest inherited."""

    def __init__(self, poses, ref, qry, meas, information, switch_init=None, switch_free=None, fixed=None, mutate=(),
                 min_norm=False):
        super().__init__(poses, ref, qry, meas, switch_init, switch_free, fixed)
        self.min_norm = min_norm       # solve_step by dense least squares: the minimum-norm step of a singular system
        self.information = np.array(information, dtype=np.float64).reshape(-1, 6, 6)
        assert self.information.shape[0] == self.m
        self.mutate = tuple(mutate)

    def weight(self, e):
        return self.information[e] if "no_D" in self.mutate else D @ self.information[e] @ D

    def solve_step(self, H, g, lam):
        if not self.min_norm:
            return super().solve_step(H, g, lam)
        return np.linalg.lstsq(self.damped(H, lam).toarray(), -g, rcond=1e-13)[0]

    def edge(self, e):
        ir, iq = int(self.ref[e]), int(self.qry[e])
        r, eq, u = weighted_residual(self.poses[ir, :3], self.poses[ir, 3:], self.poses[iq, :3], self.poses[iq, 3:],
                                     self.meas[e, :3], self.meas[e, 3:], self.mutate)
        Jr, Jq = weighted_jacobians(self.poses[ir, 3:], self.meas[e, 3:], eq, u)
        return r, Jr, Jq

    def cost(self):
        c = 0.0
        for e in range(self.m):
            r = self.edge(e)[0]
            s = self.sw[e]
            c += s * s * float(r @ self.weight(e) @ r)
            if self.sw_free[e]:
                c += (1 - s) ** 2 * op.C_SWITCH ** 2
        return c

    def linearize(self):
        n, m = self.n, self.m
        dim = 6 * n + m
        rows, cols, vals = [], [], []
        g = np.zeros(dim)
        cost = 0.0
        for e in range(m):
            ir, iq = int(self.ref[e]), int(self.qry[e])
            r, Jr, Jq = self.edge(e)
            s, free = self.sw[e], bool(self.sw_free[e])
            W = np.zeros((7, 7))
            W[:6, :6] = self.weight(e)
            W[6, 6] = 1.0
            J = np.zeros((7, 13))
            J[:6, :6] = 0.0 if self.fixed[ir] else s * Jr
            J[:6, 6:12] = 0.0 if self.fixed[iq] else s * Jq
            if free:
                J[:6, 12] = r
                J[6, 12] = -op.C_SWITCH
            f = np.concatenate([s * r, [op.C_SWITCH * (1 - s) if free else 0.0]])
            cost += float(f @ W @ f)
            idx = [self._index(ir, k) for k in range(6)] + [self._index(iq, k) for k in range(6)] + [6 * n + e]
            Hl, gl = J.T @ W @ J, J.T @ W @ f
            for a in range(13):
                g[idx[a]] += gl[a]
                for b in range(13):
                    if Hl[a, b] != 0.0:
                        rows.append(idx[a])
                        cols.append(idx[b])
                        vals.append(Hl[a, b])
        H = sp.coo_matrix((vals, (rows, cols)), shape=(dim, dim)).tocsr()
        diag_fix = np.zeros(dim)
        for i in np.nonzero(self.fixed)[0]:
            for k in range(6):
                diag_fix[self._index(int(i), k)] = 1.0
        for e in np.nonzero(~self.sw_free)[0]:
            diag_fix[6 * n + int(e)] = 1.0
        return (H + sp.diags(diag_fix)).tocsr(), g, cost


def info_graph(st, mutate=(), information=None, min_norm=False):
    return InfoGraph(st["poses"], st["ref"], st["qry"], st["meas"], st["information"] if information is None else information,
                     st["sw"], st["free"], st["fixed"], mutate=mutate, min_norm=min_norm)


def restatement_quantities(st, x, lambdas=LAMBDAS):
    """InfoGraph.linearize() and damped() @ x in the layout of reference()"""
    n = st["poses"].shape[0]
    g = info_graph(st)
    H, grad, cost = g.linearize()
    Hd = H.toarray() if n <= 300 else None
    idx = np.arange(n)
    if Hd is not None:
        planes = np.stack([Hd[a * n + idx, b * n + idx] for a, b in UPPER])
    else:
        Hc = H.tocsr()
        planes = np.stack([np.asarray(Hc[a * n + idx, b * n + idx]).ravel() for a, b in UPPER])
    out = {"cost": cost, "gradient": grad[:6 * n], "switch_gradient": grad[6 * n:], "hdiag": planes, "product": {},
           "switch_product": {}}
    for lam in lambdas:
        y = g.damped(H, lam) @ x
        out["product"][lam], out["switch_product"][lam] = y[:6 * n], y[6 * n:]
    return out


# ---------------------------------------------------------------- the formulas once more, over a number type and a sign

def _cross(a, b, sg):
    return [a[1] * b[2] + sg * (a[2] * b[1]), a[2] * b[0] + sg * (a[0] * b[2]), a[0] * b[1] + sg * (a[1] * b[0])]


def _assemble(st, conv, sg, x, lambdas, dpos=None, r_true=None):
    n, m = st["poses"].shape[0], st["ref"].size
    ref, qry = st["ref"].astype(np.int64), st["qry"].astype(np.int64)
    free, fixed = st["free"].astype(bool), st["fixed"].astype(bool)
    P, M = conv(st["poses"]), conv(st["meas"])
    qr, qq, qm, tm = hi._cols(P[ref, 3:]), hi._cols(P[qry, 3:]), hi._cols(M[:, 3:]), hi._cols(M[:, :3])
    Rr, Rm = hi._rot(qr, sg), hi._rot(qm, sg)
    if dpos is None:
        dpos = hi._cols(P[qry, :3] - P[ref, :3])
    Rt = [[Rr[j][i] for j in range(3)] for i in range(3)]
    u = [Rt[i][0] * dpos[0] + Rt[i][1] * dpos[1] + Rt[i][2] * dpos[2] for i in range(3)]
    ew, ex, ey, ez = hi._qmul(hi._qmul((qq[0], sg * qq[1], sg * qq[2], sg * qq[3]), qr, sg), qm, sg)
    r = [u[i] + sg * tm[i] for i in range(3)] + [2 * ex, 2 * ey, 2 * ez]
    Ep = [[ew, sg * ez, ey], [ez, ew, sg * ex], [sg * ey, ex, ew]]
    C = [[sg * ew, sg * ez, ey], [ez, sg * ew, sg * ex], [sg * ey, ex, sg * ew]]
    B = [[Ep[i][0] * Rm[j][0] + Ep[i][1] * Rm[j][1] + Ep[i][2] * Rm[j][2] for j in range(3)] for i in range(3)]
    Wp = conv(np.einsum("ab,ebc,cd->ead", D, st["information"], D))       # sign flips are exact
    W = [[Wp[:, a, b] for b in range(6)] for a in range(6)]
    s = conv(st["sw"])
    zero_m, zero_n = conv(np.zeros(m)), conv(np.zeros(n))
    one_m = zero_m + 1
    c2 = conv(np.array([op.C_SWITCH]))[0] ** 2
    s2 = s * s

    def apply_W(v):
        return [sum(W[a][b] * v[b] for b in range(6)) for a in range(6)]

    def J(role, v):
        if role == 0:
            ux = _cross(u, v[3:], sg)
            return ([ux[i] + sg * (Rt[i][0] * v[0] + Rt[i][1] * v[1] + Rt[i][2] * v[2]) for i in range(3)] +
                    [B[i][0] * v[3] + B[i][1] * v[4] + B[i][2] * v[5] for i in range(3)])
        return ([Rt[i][0] * v[0] + Rt[i][1] * v[1] + Rt[i][2] * v[2] for i in range(3)] +
                [C[i][0] * v[3] + C[i][1] * v[4] + C[i][2] * v[5] for i in range(3)])

    def JT(role, y):
        if role == 0:
            yu = _cross(y[:3], u, sg)
            return ([sg * (Rt[0][j] * y[0] + Rt[1][j] * y[1] + Rt[2][j] * y[2]) for j in range(3)] +
                    [yu[j] + B[0][j] * y[3] + B[1][j] * y[4] + B[2][j] * y[5] for j in range(3)])
        return ([Rt[0][j] * y[0] + Rt[1][j] * y[1] + Rt[2][j] * y[2] for j in range(3)] +
                [C[0][j] * y[3] + C[1][j] * y[4] + C[2][j] * y[5] for j in range(3)])

    keep_r, keep_q = ~fixed[ref], ~fixed[qry]

    def scatter(at_ref, at_qry):
        acc = zero_n.copy()
        np.add.at(acc, ref[keep_r], at_ref[keep_r])
        np.add.at(acc, qry[keep_q], at_qry[keep_q])
        return acc

    wr = apply_W(r)
    rsq = r if r_true is None else r_true
    rr = sum(rsq[k] * wr[k] for k in range(6))
    oms = 1 + sg * s
    out = {"r": r}
    out["cost"] = np.sum(s2 * rr + np.where(free, oms * oms * c2, zero_m))
    out["switch_gradient"] = np.where(free, s * rr + sg * (c2 * oms), zero_m)
    h_s = np.where(free, rr + c2, one_m)
    g_r, g_q = [s2 * v for v in JT(0, wr)], [s2 * v for v in JT(1, wr)]
    out["gradient"] = np.concatenate([scatter(g_r[k], g_q[k]) for k in range(6)])
    cols = []
    for c in range(6):
        ec = [one_m if k == c else zero_m for k in range(6)]
        col_r, col_q = JT(0, apply_W(J(0, ec))), JT(1, apply_W(J(1, ec)))
        cols.append([scatter(s2 * col_r[a], s2 * col_q[a]) for a in range(6)])
    planes = []
    for a, b in UPPER:
        plane = cols[b][a]
        if a == b:
            plane = plane.copy()
            plane[fixed] = 1 + zero_n[fixed]
        planes.append(plane)
    out["hdiag"] = np.stack(planes)
    X = conv(x)
    xk = [X[k * n:(k + 1) * n] for k in range(6)]
    xs_all = X[6 * n:]
    xs = np.where(free, xs_all, zero_m)
    xr = [np.where(fixed[ref], zero_m, xk[k][ref]) for k in range(6)]
    xq = [np.where(fixed[qry], zero_m, xk[k][qry]) for k in range(6)]
    ju = [a + b for a, b in zip(J(0, xr), J(1, xq))]
    wv = apply_W([s * ju[k] + r[k] * xs for k in range(6)])
    y_r, y_q = [s * w for w in JT(0, wv)], [s * w for w in JT(1, wv)]
    hx = []
    for k in range(6):
        rows = scatter(y_r[k], y_q[k])
        rows[fixed] = xk[k][fixed]
        hx.append(rows)
    hs_x = np.where(free, sum(wr[k] * (s * ju[k]) for k in range(6)), zero_m)
    out["product"], out["switch_product"] = {}, {}
    for lam in lambdas:
        lam_c = conv(np.array([lam]))[0]
        out["product"][lam] = np.concatenate([hx[k] + lam_c * (planes[DIAG[k]] * xk[k]) for k in range(6)])
        out["switch_product"][lam] = hs_x + (1 + lam_c) * (h_s * xs_all)
    return out


def reference(st, x, lambdas=LAMBDAS):
    """→ (values at 50 digits: object arrays of mpf, scales: float64 arrays), keyed by QUANTITIES"""
    with mpmath.workdps(hi.DPS):
        xp = _assemble(st, hi.to_mp, -1, x, lambdas)
        r_abs = [np.array([float(abs(v)) for v in col], dtype=np.float64) for col in xp["r"]]
    dpos = hi._cols(np.abs(st["poses"][st["qry"], :3] - st["poses"][st["ref"], :3]))
    scale = _assemble(st, hi._abs, +1, x, lambdas, dpos=dpos, r_true=r_abs)
    return xp, scale


def score(got, ref):
    """→ {quantity: error in units of 2^-52}; the products are the worst over the lambdas of the reference"""
    xp, scale = ref
    out = {}
    for q in QUANTITIES:
        if q.endswith("product"):
            out[q] = max(hi.error_eps(got[q][lam], xp[q][lam], scale[q][lam]) for lam in xp[q])
        else:
            out[q] = hi.error_eps(got[q], xp[q], scale[q])
    return out


def bounds(yardstick):
    return {q: max(4.0 * v, 8.0) for q, v in yardstick.items()}


# ---------------------------------------------------------------- cases

def _state(d, seed, sw=None, free=None):
    m = d["ref"].size
    return {"poses": np.array(d["init"], dtype=np.float64), "ref": np.asarray(d["ref"], dtype=np.int32),
            "qry": np.asarray(d["qry"], dtype=np.int32), "meas": np.array(d["meas"], dtype=np.float64),
            "fixed": np.asarray(d["fixed"], dtype=np.uint8).copy(),
            "sw": np.ones(m) if sw is None else np.array(sw, dtype=np.float64),
            "free": np.zeros(m, dtype=np.uint8) if free is None else np.asarray(free, dtype=np.uint8),
            "information": draw_information(m, seed), "true": d["true"]}


@functools.lru_cache(maxsize=None)
def case(name):
    """→ state dict: poses [n,7], ref, qry, meas [m,7], fixed [n], sw [m], free [m], information [m,6,6].  Read-only."""
    if name == "chain13":
        # 13 poses, 12 + 3 constraints: a chain 0 … 11, pose 12 hanging off pose 0 alone — pose 0 is fixed, so pose 12 has
        # no free neighbour — and three loop constraints.  One of them starts at pose 0: constraint 0 (0 → 1) is one of the
        # semi-definite ones, and as the chain's only tie to the fixed pose it would leave the whole chain free to slide
        # along its null direction (a singular system at lambda = 0)
        d = op.random_graph(12, 0, seed=41)
        true = np.concatenate([d["true"], d["true"][5:6]])
        true[12, :3] += [0.3, -0.4, 0.2]
        init = np.concatenate([d["init"], true[12:13]])
        init[12, :3] += [0.04, 0.03, -0.05]
        init[12, 3:] = op.qmul(init[12, 3:], op.qexp(np.array([0.02, -0.01, 0.015])))
        base = {"true": true, "init": init, "ref": d["ref"], "qry": d["qry"], "meas": d["meas"],
                "fixed": np.concatenate([d["fixed"], [0]]).astype(np.uint8)}
        st = _state(op.with_edges(base, [(0, 12), (0, 6), (3, 10), (4, 11)], seed=42), 43)
        assert st["poses"].shape[0] == 13 and st["ref"].size == 15 and list(np.nonzero(st["fixed"])[0]) == [0]
        return st
    if name == "two_groups":
        # 257 poses (two workgroups of pose rows), 513 constraints (three of switch rows); every third switch free at 0.7;
        # poses 1, 2, 200 fixed; pose 100 has 9 incident constraints.  A constraint with a free switch holds nothing along
        # its own residual (the switch gives way), so where one is a bridge the system at lambda = 0 is singular to the
        # 1e-18 of the switch prior: the head of the chain and its last dozen poses, where the random loop constraints
        # thin out, get extra constraints, most of them with a fixed switch and a full-rank information
        d = op.random_graph(257, 0, seed=44)
        pairs = [(100, 100 + k) for k in (3, 5, 7, 9)] + [(100 - k, 100) for k in (4, 6, 8)]
        pairs = [(0, 3), (0, 4)] + [(k, k + 4) for k in range(244, 253)] + [(253, 256)] + pairs   # constraints 256 … 267
        k = 0
        while len(pairs) < 257:       # loop constraints 2 … 6 poses ahead, spread evenly: every chain constraint is spanned
            a, b = (k * 249) // 238, (k * 249) // 238 + 2 + k % 5
            k += 1
            if 100 not in (a, b) and b < 257:
                pairs.append((a, b))
        d = op.with_edges(d, pairs, seed=46)
        d["fixed"][:] = 0
        d["fixed"][[1, 2, 200]] = 1
        m = d["ref"].size
        free = (np.arange(m) % 3 == 0).astype(np.uint8)
        st = _state(d, 47, sw=np.where(free, 0.7, 1.0), free=free)
        assert st["poses"].shape[0] == 257 and m == 513
        assert int(np.sum(st["ref"] == 100) + np.sum(st["qry"] == 100)) == 9
        return st
    if name == "two_level":
        return _state(pgo_cases._realistic(), 48)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    st = case(name)
    return reference(st, hi.masked_x(st))


@functools.lru_cache(maxsize=None)
def case_yardstick(name):
    """e_np: the float64 restatement's own error against 50 digits, per quantity"""
    st = case(name)
    return score(restatement_quantities(st, hi.masked_x(st)), case_reference(name))


def gpu_graph(ctx, st, information=True, **kwargs):
    from nonlinear_optimizer_for_slam_amd import pgo
    info = st["information"] if information is True else information
    return pgo.PoseGraph(ctx, st["poses"], st["ref"], st["qry"], st["meas"], st["sw"], st["free"], st["fixed"],
                         **({} if info is None else {"information": info}), **kwargs)


# ---------------------------------------------------------------- the corridor

CORRIDOR_NOISE = 0.01     # metres, planted along x in every odometry measurement
CORRIDOR_POSES = 24


@functools.lru_cache(maxsize=None)
def corridor():
    """A straight chain along x (identity rotations, 1 m steps), pose 0 fixed.  Every odometry measurement is off by
    +CORRIDOR_NOISE along x — the direction a corridor registration does not observe — and its information has eigenvalue 0
    there (diag(0, 100, 100, 100, 100, 100)); one full-rank loop constraint 0 → last carries the true relative pose.
    → state dict with "true".  With information the odometry constraints do not resist sliding along x: the loop closure
    alone decides where the chain's end lies along x, and the end lands on it.  Nothing observes the x of the poses in
    between: their rows of the normal matrix and of the gradient are exactly zero (identity rotations keep the zeros
    exact), the minimum-norm step leaves them where dead reckoning put them, and so does a PCG that starts from zero.
    Without information the 0.23 m of accumulated error is spread over all 24 constraints and the end stays 1 cm off."""
    n = CORRIDOR_POSES
    true = np.zeros((n, 7))
    true[:, 0] = np.arange(n)
    true[:, 3] = 1.0
    init = true.copy()
    init[1:, 0] += CORRIDOR_NOISE * np.arange(1, n)          # dead reckoning on the odometry
    ref = np.array(list(range(n - 1)) + [0], dtype=np.int32)
    qry = np.array(list(range(1, n)) + [n - 1], dtype=np.int32)
    meas = np.zeros((n, 7))
    meas[:, 3] = 1.0
    meas[:n - 1, 0] = 1.0 + CORRIDOR_NOISE
    meas[n - 1, 0] = n - 1.0
    info = np.zeros((n, 6, 6))
    info[:n - 1] = np.diag([0.0, 100.0, 100.0, 100.0, 100.0, 100.0])
    info[n - 1] = np.diag([400.0, 400.0, 400.0, 900.0, 900.0, 900.0])
    fixed = np.zeros(n, dtype=np.uint8)
    fixed[0] = 1
    return {"poses": init, "ref": ref, "qry": qry, "meas": meas, "fixed": fixed, "sw": np.ones(n),
            "free": np.zeros(n, dtype=np.uint8), "information": info, "true": true}
