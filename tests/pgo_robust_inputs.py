"""A robust loss on pose-graph constraints with information — TEST INFRASTRUCTURE shared by test_pgo_robust_host.py (CPU),
test_pgo_robust.py and test_pgo_robust_abi.py (GPU); DESIGN.md §34.

The rule (include/nos.h, nos_pgo_set_loss): with q = r~^T Omega' r~ of the measurement-frame residual, rho the loss and
w = rho'(q), every term of the weighted rule (tests/pgo_info_inputs.py) that carries Omega' carries w Omega', the cost is
s^2 rho(q) (+ (1 - s)^2 c^2), and the switch takes g_s = s rho - c^2 (1 - s), h_s = rho + c^2.  Restated twice:
  * RobustGraph — numpy, a subclass of pgo_info_inputs.InfoGraph: cost and linearize restated, the rest inherited.
    `mutate` plants the two mistakes the GPU test must be able to tell from the rule ("w2": w = 2 rho', the NDT kernels'
    convention; "hs_wq": h_s = w q + c^2, g_s = s w q - c^2 (1 - s), the switch treated like a pose);
  * reference() — the formulas of pgo_info_inputs._assemble extended through the loss, over a number type and a sign:
    mpmath at 50 digits, and the first-order error SCALE in float64.  The scale of rho and w carries the scale of q through
    the loss: |rho'(q)| scale(q) + (the magnitudes of the loss's own operations), likewise for w with |rho''(q)|.
Error of a float64 result = |got - reference| / scale in units of 2^-52; the yardstick e_np is RobustGraph's own error in
that measure and the device may err up to max(4 e_np, 8) units.  Nothing in a bound comes from the code
under test.

Per case of pgo_info_inputs.case() the Huber threshold is the median sqrt(q) of the case at its state and the exponential
loss is (1, 1 / median^2), both computed by the restatement: half of the constraints on either side of the threshold.
Every input is built once per process and then left unchanged."""
import functools

import mpmath
import numpy as np
import scipy.sparse as sp

from oracle import oracle_pgo as op
from tests import pgo_hard_inputs as hi
from tests import pgo_info_inputs as pi

LAMBDAS = pi.LAMBDAS
CASES = pi.CASES
KINDS = ("huber", "exponential")
QUANTITIES = pi.QUANTITIES + ("weights",)
UPPER, DIAG = pi.UPPER, pi.DIAG
TINY = float(np.finfo(np.float64).tiny)


# ---------------------------------------------------------------- the loss

def rho_w(loss, q):
    """(rho(q), rho'(q)) in float64; loss: None | ("huber", delta) | ("exponential", c1, c2)"""
    if loss is None:
        return q, 1.0
    if loss[0] == "huber":
        d = float(loss[1])
        if q <= d * d:
            return q, 1.0
        root = np.sqrt(q)
        return 2.0 * d * root - d * d, d / root
    if loss[0] == "exponential":
        c1, c2 = float(loss[1]), float(loss[2])
        ex = np.exp(-c2 * q)
        return c1 - c1 * ex, c1 * c2 * ex
    raise ValueError(loss)


# ---------------------------------------------------------------- numpy restatement

class RobustGraph(pi.InfoGraph):
    """InfoGraph under a robust loss: cost and linearize restated, the rest (damped solve, retraction, LM loop) inherited.
    robust: [m] flags of the constraints the loss applies to, None = all."""

    def __init__(self, poses, ref, qry, meas, information, switch_init=None, switch_free=None, fixed=None, loss=None,
                 robust=None, mutate=()):
        super().__init__(poses, ref, qry, meas, information, switch_init, switch_free, fixed)
        self.loss = loss
        self.robust = np.ones(self.m, dtype=bool) if robust is None else np.asarray(robust, dtype=bool)
        self.robust_mutate = tuple(mutate)

    def edge_loss(self, e, r):
        """→ (q, rho, w) of constraint e at residual r"""
        q = float(r @ self.weight(e) @ r)
        rho, w = rho_w(self.loss if self.robust[e] else None, q)
        if "w2" in self.robust_mutate and self.robust[e] and self.loss is not None:
            w = 2.0 * w
        return q, rho, w

    def weights(self):
        return np.array([self.edge_loss(e, self.edge(e)[0])[2] for e in range(self.m)])

    def q(self):
        return np.array([self.edge_loss(e, self.edge(e)[0])[0] for e in range(self.m)])

    def cost(self):
        c = 0.0
        for e in range(self.m):
            s = self.sw[e]
            c += s * s * self.edge_loss(e, self.edge(e)[0])[1]
            if self.sw_free[e]:
                c += (1 - s) ** 2 * op.C_SWITCH ** 2
        return c

    def linearize(self):
        n, m = self.n, self.m
        dim = 6 * n + m
        rows, cols, vals = [], [], []
        g = np.zeros(dim)
        cost = 0.0
        c2 = op.C_SWITCH ** 2
        for e in range(m):
            ir, iq = int(self.ref[e]), int(self.qry[e])
            r, Jr, Jq = self.edge(e)
            s, free = self.sw[e], bool(self.sw_free[e])
            q, rho, w = self.edge_loss(e, r)
            W = w * self.weight(e)
            J = np.zeros((6, 13))
            J[:, :6] = 0.0 if self.fixed[ir] else s * Jr
            J[:, 6:12] = 0.0 if self.fixed[iq] else s * Jq
            if free:
                J[:, 12] = r
            Hl, gl = J.T @ W @ J, J.T @ W @ (s * r)
            cost += s * s * rho
            if free:                       # the switch: the loss's VALUE, not its weight
                cost += (1 - s) ** 2 * c2
                if "hs_wq" in self.robust_mutate:
                    Hl[12, 12], gl[12] = w * q + c2, s * w * q - c2 * (1 - s)
                else:
                    Hl[12, 12], gl[12] = rho + c2, s * rho - c2 * (1 - s)
            idx = [self._index(ir, k) for k in range(6)] + [self._index(iq, k) for k in range(6)] + [6 * n + e]
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


def robust_graph(st, loss, robust=None, mutate=(), information=None):
    return RobustGraph(st["poses"], st["ref"], st["qry"], st["meas"], st["information"] if information is None else information,
                       st["sw"], st["free"], st["fixed"], loss=loss, robust=robust, mutate=mutate)


def restatement_quantities(st, x, loss, robust=None, mutate=(), lambdas=LAMBDAS):
    """RobustGraph.linearize(), damped() @ x and weights() in the layout of reference()"""
    n = st["poses"].shape[0]
    g = robust_graph(st, loss, robust, mutate)
    H, grad, cost = g.linearize()
    Hc = H.tocsr()
    idx = np.arange(n)
    planes = np.stack([np.asarray(Hc[a * n + idx, b * n + idx]).ravel() for a, b in UPPER])
    out = {"cost": cost, "gradient": grad[:6 * n], "switch_gradient": grad[6 * n:], "hdiag": planes, "product": {},
           "switch_product": {}, "weights": g.weights(), "switch_curvature": H.diagonal()[6 * n:]}
    for lam in lambdas:
        y = g.damped(H, lam) @ x
        out["product"][lam], out["switch_product"][lam] = y[:6 * n], y[6 * n:]
    return out


# ---------------------------------------------------------------- the formulas once more, over a number type and a sign

def _loss_exact(loss, q):
    """(rho, w) of an array of mpf"""
    rho, w = [], []
    for v in q.tolist():
        if loss is None:
            rho.append(v), w.append(mpmath.mpf(1))
        elif loss[0] == "huber":
            d = mpmath.mpf(float(loss[1]))
            if v <= d * d:
                rho.append(v), w.append(mpmath.mpf(1))
            else:
                root = mpmath.sqrt(v)
                rho.append(2 * d * root - d * d), w.append(d / root)
        else:
            c1, c2 = mpmath.mpf(float(loss[1])), mpmath.mpf(float(loss[2]))
            ex = mpmath.exp(-c2 * v)
            rho.append(c1 - c1 * ex), w.append(c1 * c2 * ex)
    return np.array(rho, dtype=object), np.array(w, dtype=object)


def _loss_scale(loss, q_scale, q_true):
    """First-order error scale of (rho, w): q_scale is the scale of q, q_true its magnitude (float64).  Per operation of
    the loss, the magnitude of its result; the error of q enters through |rho'| and |rho''|.  At the Huber threshold both
    branches agree in rho, rho' (and w is continuous), so the branch a rounded q takes does not matter to first order."""
    rho, w = np.empty_like(q_true), np.empty_like(q_true)
    for k, (qs, qt) in enumerate(zip(q_scale.tolist(), q_true.tolist())):
        if loss is None:
            rho[k], w[k] = qs, 0.0
        elif loss[0] == "huber":
            d = float(loss[1])
            if qt <= d * d:
                rho[k], w[k] = qs, 0.0
                if qt + qs * hi.EPS * 64 > d * d:          # within rounding of the threshold: w may come from the other branch
                    w[k] = 1.0 + 0.5 * qs / qt
            else:
                root = np.sqrt(qt)
                rho[k] = d / root * qs + 2 * d * root + d * d
                w[k] = 0.5 * d / (root * qt) * qs + d / root
        else:
            c1, c2 = float(loss[1]), float(loss[2])
            ex = np.exp(-c2 * qt)
            # the argument c2 q carries its own rounding: relative c2 q in exp
            # and a weight that underflows is off by up to the spacing of the subnormals, 2^-52 of the smallest normal number
            rho[k] = c1 * c2 * ex * (qs + qt) + c1 + c1 * ex
            w[k] = c1 * c2 * c2 * ex * (qs + qt) + c1 * c2 * ex + TINY
    return rho, w


def _assemble(st, conv, sg, x, lambdas, loss, robust, dpos=None, r_true=None, q_true=None):
    """pgo_info_inputs._assemble with w Omega' in the place of Omega' and rho in the place of q (the same formulas, the same
    order); q_true: the magnitudes of q for the scale pass."""
    n, m = st["poses"].shape[0], st["ref"].size
    ref, qry = st["ref"].astype(np.int64), st["qry"].astype(np.int64)
    free, fixed = st["free"].astype(bool), st["fixed"].astype(bool)
    flagged = np.ones(m, dtype=bool) if robust is None else np.asarray(robust, dtype=bool)
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
    Wp = conv(np.einsum("ab,ebc,cd->ead", pi.D, st["information"], pi.D))       # sign flips are exact
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
            ux = pi._cross(u, v[3:], sg)
            return ([ux[i] + sg * (Rt[i][0] * v[0] + Rt[i][1] * v[1] + Rt[i][2] * v[2]) for i in range(3)] +
                    [B[i][0] * v[3] + B[i][1] * v[4] + B[i][2] * v[5] for i in range(3)])
        return ([Rt[i][0] * v[0] + Rt[i][1] * v[1] + Rt[i][2] * v[2] for i in range(3)] +
                [C[i][0] * v[3] + C[i][1] * v[4] + C[i][2] * v[5] for i in range(3)])

    def JT(role, y):
        if role == 0:
            yu = pi._cross(y[:3], u, sg)
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
    q = sum(rsq[k] * wr[k] for k in range(6))
    # the loss: exact values (sign -1) or the scale pass (sign +1, q_true given)
    if q_true is None:
        if q.dtype == object:
            rho_l, w_l = _loss_exact(loss, q)
        else:
            rho_l, w_l = (np.array(v) for v in zip(*[rho_w(loss, float(v)) for v in q]))
        rho = np.where(flagged, rho_l, q)
        w = np.where(flagged, w_l, one_m)
        w_out = w
    else:
        rho_l, w_l = _loss_scale(loss, q, q_true)
        rho = np.where(flagged, rho_l, q)
        w_true = np.array([rho_w(loss, float(v))[1] for v in q_true])
        w_out = np.where(flagged, w_l, zero_m)                 # scale of w itself: an unflagged weight is exactly 1
        w = np.where(flagged, np.maximum(w_l, w_true), one_m)  # what multiplies the scales below: |w|, or its scale where larger
    oms = 1 + sg * s
    out = {"r": r, "q": q, "weights": w_out}
    out["cost"] = np.sum(s2 * rho + np.where(free, oms * oms * c2, zero_m))
    out["switch_gradient"] = np.where(free, s * rho + sg * (c2 * oms), zero_m)
    h_s = np.where(free, rho + c2, one_m)
    s2w, sw_ = s2 * w, s * w
    g_r, g_q = [s2w * v for v in JT(0, wr)], [s2w * v for v in JT(1, wr)]
    out["gradient"] = np.concatenate([scatter(g_r[k], g_q[k]) for k in range(6)])
    cols = []
    for c in range(6):
        ec = [one_m if k == c else zero_m for k in range(6)]
        col_r, col_q = JT(0, apply_W(J(0, ec))), JT(1, apply_W(J(1, ec)))
        cols.append([scatter(s2w * col_r[a], s2w * col_q[a]) for a in range(6)])
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
    y_r, y_q = [sw_ * v for v in JT(0, wv)], [sw_ * v for v in JT(1, wv)]
    hx = []
    for k in range(6):
        rows = scatter(y_r[k], y_q[k])
        rows[fixed] = xk[k][fixed]
        hx.append(rows)
    hs_x = np.where(free, sum(wr[k] * (sw_ * ju[k]) for k in range(6)), zero_m)
    out["product"], out["switch_product"] = {}, {}
    for lam in lambdas:
        lam_c = conv(np.array([lam]))[0]
        out["product"][lam] = np.concatenate([hx[k] + lam_c * (planes[DIAG[k]] * xk[k]) for k in range(6)])
        out["switch_product"][lam] = hs_x + (1 + lam_c) * (h_s * xs_all)
    return out


def reference(st, x, loss, robust=None, lambdas=LAMBDAS):
    """→ (values at 50 digits: object arrays of mpf, scales: float64 arrays), keyed by QUANTITIES"""
    with mpmath.workdps(hi.DPS):
        xp = _assemble(st, hi.to_mp, -1, x, lambdas, loss, robust)
        r_abs = [np.array([float(abs(v)) for v in col], dtype=np.float64) for col in xp["r"]]
        q_abs = np.array([float(abs(v)) for v in xp["q"]], dtype=np.float64)
    dpos = hi._cols(np.abs(st["poses"][st["qry"], :3] - st["poses"][st["ref"], :3]))
    scale = _assemble(st, hi._abs, +1, x, lambdas, loss, robust, dpos=dpos, r_true=r_abs, q_true=q_abs)
    return xp, scale


def error_eps(got, xp, scale):
    """pgo_hard_inputs.error_eps, where a zero scale with a value that is exactly the reference's counts as no error (the
    weight of a constraint no loss applies to: scale 0, value 1.0)"""
    got, scale = np.asarray(got, dtype=np.float64).ravel(), np.asarray(scale, dtype=np.float64).ravel()
    xp = np.asarray(xp, dtype=object).ravel()
    assert got.shape == xp.shape == scale.shape, (got.shape, xp.shape, scale.shape)
    worst = 0.0
    with mpmath.workdps(hi.DPS):
        for g, v, sc in zip(got.tolist(), xp.tolist(), scale.tolist()):
            if sc == 0.0:
                if mpmath.mpf(g) != v:
                    return float("inf")
            else:
                worst = max(worst, float(abs(mpmath.mpf(g) - v) / sc))
    return worst / hi.EPS


def score(got, ref, quantities=QUANTITIES):
    """→ {quantity: error in units of 2^-52}; the products are the worst over the lambdas of the reference"""
    xp, scale = ref
    out = {}
    for q in quantities:
        if q.endswith("product"):
            out[q] = max(error_eps(got[q][lam], xp[q][lam], scale[q][lam]) for lam in xp[q])
        else:
            out[q] = error_eps(got[q], xp[q], scale[q])
    return out


def bounds(yardstick):
    return {q: max(4.0 * v, 8.0) for q, v in yardstick.items()}


# ---------------------------------------------------------------- cases

@functools.lru_cache(maxsize=None)
def median_root_q(name):
    """median sqrt(q) of the case at its state, by the restatement"""
    return float(np.median(np.sqrt(robust_graph(pi.case(name), None).q())))


def case_loss(name, kind):
    med = median_root_q(name)
    return ("huber", med) if kind == "huber" else ("exponential", 1.0, 1.0 / (med * med))


def third_flags(name):
    """every third constraint carries the loss"""
    return (np.arange(pi.case(name)["ref"].size) % 3 == 0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case_reference(name, kind, flagged=False):
    st = pi.case(name)
    return reference(st, hi.masked_x(st), case_loss(name, kind), third_flags(name) if flagged else None)


@functools.lru_cache(maxsize=None)
def case_restatement(name, kind, flagged=False, mutate=()):
    st = pi.case(name)
    return restatement_quantities(st, hi.masked_x(st), case_loss(name, kind), third_flags(name) if flagged else None, mutate)


@functools.lru_cache(maxsize=None)
def case_yardstick(name, kind, flagged=False):
    """e_np: the float64 restatement's own error against 50 digits, per quantity"""
    return score(case_restatement(name, kind, flagged), case_reference(name, kind, flagged))


def gpu_graph(ctx, st, loss, robust=None, **kwargs):
    from nonlinear_optimizer_for_slam_amd import pgo
    return pgo.PoseGraph(ctx, st["poses"], st["ref"], st["qry"], st["meas"], st["sw"], st["free"], st["fixed"],
                         information=st["information"], loss=loss, robust=robust, **kwargs)


def gpu_quantities(g, st, x, lambdas=LAMBDAS):
    """linearize() and what follows it, in the layout of reference() → (quantities, |g|)"""
    cost, gnorm = g.linearize()
    got = hi.split_gpu(st["poses"].shape[0], cost, g.vector("gradient"), g.vector("hdiag"),
                       {lam: g.matvec(lam, x) for lam in lambdas})
    got["weights"] = g.edge_weights()
    return got, gnorm


# ---------------------------------------------------------------- the scene

SCENE_LOSS = ("exponential", 0.02, 50.0)
SCENE_OUTLIER = 82
SCENE_LOOPS = (79, 80, 81)
SCENE_VARIANTS = ("identity", "odometry100")


@functools.lru_cache(maxsize=None)
def scene(variant="identity"):
    """oracle_pgo.reference_test_scene(), the reference's own demo (an 80-pose square, 79 odometry constraints, 4 loop
    constraints of which the last is an outlier), with every switch FIXED at 1 — the loss is the only defence — and pose 0
    fixed.  "identity": every information matrix is the identity and the loss applies to every constraint (what the host
    class does with SetLossFunction); "odometry100": the odometry constraints have information 100 I and the loss applies to
    the loop closures alone, the usual choice (on the odometry it would see q = 100 |r|^2 of the noisy start and reject
    the chain).  → state dict with "true" and "robust" (flags or None)."""
    true, noisy, ref, qry, meas, _ = op.reference_test_scene()
    m = ref.size
    fixed = np.zeros(80, dtype=np.uint8)
    fixed[0] = 1
    info = np.broadcast_to(np.eye(6), (m, 6, 6)).copy()
    robust = None
    if variant == "odometry100":
        info[:79] *= 100.0
        robust = (np.arange(m) >= 79).astype(np.uint8)
    return {"poses": noisy, "ref": ref, "qry": qry, "meas": meas, "fixed": fixed, "sw": np.ones(m),
            "free": np.zeros(m, dtype=np.uint8), "information": info, "true": true, "robust": robust}


@functools.lru_cache(maxsize=None)
def scene_restatement(variant="identity", with_loss=True):
    """The restatement's LM loop (optimize() as it stands: 40 iterations, tolerances 1e-6) on the scene
    → (largest position error against the true poses, weights at the end, final poses)"""
    st = scene(variant)
    g = robust_graph(st, SCENE_LOSS if with_loss else None, st["robust"])
    g.optimize()
    return position_error(g.poses, st), g.weights(), g.poses.copy()


def position_error(poses, st):
    return float(np.max(np.linalg.norm(np.asarray(poses)[:, :3] - st["true"][:, :3], axis=1)))
