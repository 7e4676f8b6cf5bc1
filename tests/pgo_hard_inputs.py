"""Hard states of the pose-graph linearisation, its 50-digit reference and the error scale — TEST INFRASTRUCTURE shared
by test_pgo_xprec.py (CPU) and test_pgo_xprec_gpu.py (GPU); DESIGN.md §26.

Quantities: cost, pose gradient, the 21 planes of the diagonal blocks, switch gradient and curvature, and the damped
product y = (H + lambda diag H) x with its pose rows and its switch rows — the formulas in the header of
csrc/pgo_kernels.hpp, restated once (_edge_terms, _assemble) over a number type and a sign:
  * reference: mpmath at DPS digits from the float64 inputs, sign -1;
  * twin:      float64 numpy, sign -1, with the mutations the CPU test plants;
  * SCALE:     float64, every operand replaced by its absolute value and every subtraction by an addition (sign +1):
               rho for the residual, mu for a Jacobian entry, sum s^2 mu^T rho for the gradient, sum s^2 mu^T mu for
               the diagonal blocks, the product formula on mu, rho and |x|.  Two operands keep their true magnitude: the
               position difference p_q - p_r (one exact operation in float64; its operands may be UTM sized), and the
               residual in the squares r_k^2 of the cost and of the switch rows, whose first-order error is |r_k| rho_k.
Error of a float64 result = |got - reference| / scale in units of 2^-52.  The scale is the first-order rounding bound
of the expression, so it stays meaningful where r or J are what a cancellation left; where it is exactly 0 (the
off-diagonal entries of the translation block, the rows of fixed poses) the value must be exactly 0.

Yardstick: oracle_pgo.Graph.linearize() and damped() @ x — float64 scipy assembly — scored in that measure on the same
inputs.  BOUND per state and quantity: max(4 x yardstick, 8) units; the 4 covers fused multiply-adds and another
summation order, the floor of 8 the dozen roundings of a term.  Nothing in it comes from the code under test."""
import functools

import mpmath
import numpy as np

from oracle import oracle_pgo as op

DPS = 50
EPS = 2.0 ** -52
LAMBDAS = (0.0, 1e-3)
N_POSES = 160
BLOCK = 128          # poses per workgroup of the block-local product
FAMILIES = ("baseline", "far", "converged", "half_turn", "long_edges", "non_unit", "switches", "hub")
FAR_OFFSET = np.array([4.5e5, 5.4e6, 300.0])
SWITCH_CYCLE = (0.0, 1e-8, -0.5, 1.0, 3.0, 1e8, 0.7)
QUANTITIES = ("cost", "gradient", "switch_gradient", "hdiag", "switch_curvature", "product", "switch_product")


# ---------------------------------------------------------------- states

def _state(d, sw=None, free=None, **extra):
    m = d["ref"].size
    st = {"poses": np.array(d["init"], dtype=np.float64), "ref": np.asarray(d["ref"], dtype=np.int32),
          "qry": np.asarray(d["qry"], dtype=np.int32), "meas": np.array(d["meas"], dtype=np.float64),
          "fixed": np.asarray(d["fixed"], dtype=np.uint8).copy(),
          "sw": np.ones(m) if sw is None else np.array(sw, dtype=np.float64),
          "free": np.zeros(m, dtype=np.uint8) if free is None else np.asarray(free, dtype=np.uint8)}
    st.update(extra)
    return st


def _unit(v):
    return v / np.linalg.norm(v)


@functools.lru_cache(maxsize=None)
def family(name):
    """→ state dict: poses [n,7], ref, qry, meas [m,7], fixed [n], sw [m], free [m] (+ what the CPU test asserts on).
    Treat as read-only (cached)."""
    n = N_POSES
    if name == "baseline":
        return _state(op.random_graph(n, 3, seed=21))
    if name == "far":
        d = op.random_graph(n, 3, seed=22)
        d["init"] = d["init"].copy()
        d["init"][:, :3] += FAR_OFFSET
        return _state(d)
    if name == "converged":
        return _state(op.random_graph(n, 3, seed=23, noise_t=1e-9, noise_r=1e-9, meas_noise_t=1e-9, meas_noise_r=1e-9))
    if name == "half_turn":
        # rotation noise of 1e-4 rad (not random_graph's 2e-2): the rotation left between a turned and an unturned end is
        # then pi to within 2e-3, i.e. |e_w| < 1e-3
        d = op.random_graph(n, 3, seed=24, noise_r=1e-4, meas_noise_r=1e-4)
        rng = np.random.default_rng(240)
        init, meas = d["init"].copy(), d["meas"].copy()
        for i in range(0, n, 3):
            angle = np.pi + (1e-3 if rng.integers(2) else -1e-3)
            q = op.qmul(init[i, 3:], op.qexp(angle * _unit(rng.normal(size=3))))
            init[i, 3:] = q / np.linalg.norm(q)
        neg_pose = rng.integers(2, size=n).astype(bool)
        neg_meas = rng.integers(2, size=meas.shape[0]).astype(bool)
        init[neg_pose, 3:] *= -1.0
        meas[neg_meas, 3:] *= -1.0
        d["init"], d["meas"] = init, meas
        return _state(d, neg_pose=neg_pose, neg_meas=neg_meas)
    if name == "long_edges":
        d = op.random_graph(n, 3, seed=25)
        true, init = d["true"].copy(), d["init"].copy()
        factor = 8000.0 / np.max(np.linalg.norm(true[1::2, :3], axis=1))
        init[1::2, :3] = true[1::2, :3] * factor + (init[1::2, :3] - true[1::2, :3])
        true[1::2, :3] *= factor
        pairs = list(zip(d["ref"].tolist(), d["qry"].tolist()))
        none = np.zeros(0, dtype=np.int32)
        d = op.with_edges({"true": true, "init": init, "ref": none, "qry": none, "meas": np.zeros((0, 7)),
                           "fixed": d["fixed"]}, pairs, seed=250)       # measurements of the stretched trajectory
        d["init"] = init
        d["fixed"][n // 2 - 3] = 1
        return _state(d)
    if name == "non_unit":
        d = op.random_graph(n, 3, seed=26)
        rng = np.random.default_rng(260)
        d["init"] = d["init"].copy()
        d["meas"] = d["meas"].copy()
        d["init"][:, 3:] *= rng.uniform(1 - 1e-3, 1 + 1e-3, size=(n, 1))
        d["meas"][:, 3:] *= rng.uniform(1 - 1e-3, 1 + 1e-3, size=(d["meas"].shape[0], 1))
        return _state(d)
    if name == "switches":
        d = op.random_graph(n, 3, seed=27)
        m = d["ref"].size
        d["fixed"][n // 2 - 3] = 1
        return _state(d, sw=np.array(SWITCH_CYCLE)[np.arange(m) % len(SWITCH_CYCLE)], free=np.arange(m) % 2)
    if name == "hub":
        d = op.random_graph(280, 0, seed=28)
        pairs = [(5, j) for j in range(7, 207)] + [(j, 6) for j in range(80, 280)]
        return _state(op.with_edges(d, pairs, seed=280))
    raise KeyError(name)


def masked_x(st, seed=0):
    """the vector test_pgo.py multiplies with: normal entries, zero on fixed poses and on switches that are not free"""
    n, m = st["poses"].shape[0], st["ref"].size
    x = np.random.default_rng(seed).normal(size=6 * n + m)
    x[6 * n:][st["free"] == 0] = 0.0
    for i in np.nonzero(st["fixed"])[0]:
        x[[k * n + i for k in range(6)]] = 0.0
    return x


# ---------------------------------------------------------------- the formulas, once, over a number type and a sign

def to_mp(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([mpmath.mpf(float(v)) for v in a.ravel()], dtype=object).reshape(a.shape)


def _cols(a):
    return tuple(a[:, k] for k in range(a.shape[1]))


def _qmul(a, b, sg):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw + sg * (ax * bx) + sg * (ay * by) + sg * (az * bz),
            aw * bx + ax * bw + ay * bz + sg * (az * by),
            aw * by + ay * bw + az * bx + sg * (ax * bz),
            aw * bz + az * bw + ax * by + sg * (ay * bx))


def _rot(q, sg):
    w, x, y, z = q
    return [[1 + sg * (2 * (y * y + z * z)), 2 * (x * y + sg * (w * z)), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 + sg * (2 * (x * x + z * z)), 2 * (y * z + sg * (w * x))],
            [2 * (x * z + sg * (w * y)), 2 * (y * z + w * x), 1 + sg * (2 * (x * x + y * y))]]


def _edge_terms(st, conv, sg, dpos=None, mutate=()):
    """per constraint: r (6 arrays), A = R_r [t_m]x, B = E+ R_m^T, C = E-  (3x3 lists of arrays)"""
    P, M = conv(st["poses"]), conv(st["meas"])
    ref, qry = st["ref"], st["qry"]
    qr, qq, qm, tm = _cols(P[ref, 3:]), _cols(P[qry, 3:]), _cols(M[:, 3:]), _cols(M[:, :3])
    Rr, Rm = _rot(qr, sg), _rot(qm, sg)
    if dpos is None:
        dpos = _cols(P[qry, :3] - P[ref, :3])
    rt = [dpos[i] + sg * (Rr[i][0] * tm[0] + Rr[i][1] * tm[1] + Rr[i][2] * tm[2]) for i in range(3)]
    ew, ex, ey, ez = _qmul(_qmul((qq[0], sg * qq[1], sg * qq[2], sg * qq[3]), qr, sg), qm, sg)
    if "negated_translation_rows" in mutate:       # a negated q_r flips r_R, B and C — and here r_t as well
        rt = [np.where(st["neg_pose"][ref], -v, v) for v in rt]
    r = rt + [2 * ex, 2 * ey, 2 * ez]
    A = [[Rr[i][1] * tm[2] + sg * (Rr[i][2] * tm[1]), Rr[i][2] * tm[0] + sg * (Rr[i][0] * tm[2]),
          Rr[i][0] * tm[1] + sg * (Rr[i][1] * tm[0])] for i in range(3)]
    if "A_sign" in mutate:
        A[0][1] = -A[0][1]
    Ep = [[ew, sg * ez, ey], [ez, ew, sg * ex], [sg * ey, ex, ew]]
    C = [[sg * ew, sg * ez, ey], [ez, sg * ew, sg * ex], [sg * ey, ex, sg * ew]]
    if "B_without_transpose" in mutate:
        B = [[Ep[i][0] * Rm[0][j] + Ep[i][1] * Rm[1][j] + Ep[i][2] * Rm[2][j] for j in range(3)] for i in range(3)]
    else:
        B = [[Ep[i][0] * Rm[j][0] + Ep[i][1] * Rm[j][1] + Ep[i][2] * Rm[j][2] for j in range(3)] for i in range(3)]
    return r, A, B, C


_UPPER = [(a, b) for a in range(6) for b in range(a, 6)]
_DIAG = [0, 6, 11, 15, 18, 20]


def _assemble(st, terms, conv, sg, x, lambdas, r_true=None, skip=None, sw=None):
    """→ dict: cost, gradient [6n], switch_gradient [m], hdiag [21,n], switch_curvature [m],
    product {lambda: [6n]}, switch_product {lambda: [m]}.  r_true: the residual whose magnitude goes into the squares
    (scale mode); skip = (constraint, role): that end's gradient term is left out; sw: other switch values (twin)."""
    n, m = st["poses"].shape[0], st["ref"].size
    ref, qry = st["ref"].astype(np.int64), st["qry"].astype(np.int64)
    free, fixed = st["free"].astype(bool), st["fixed"].astype(bool)
    r, A, B, C = terms
    s = conv(st["sw"] if sw is None else sw)
    zero_m, zero_n = conv(np.zeros(m)), conv(np.zeros(n))
    one_m = zero_m + 1
    c2 = conv(np.array([op.C_SWITCH]))[0] ** 2
    s2 = s * s
    rsq = r if r_true is None else r_true
    rr = sum(rsq[k] * r[k] for k in range(6)) if m else zero_m
    oms = 1 + sg * s
    out = {}
    out["cost"] = np.sum(s2 * rr + np.where(free, oms * oms * c2, zero_m)) if m else zero_m.sum() + 0 * c2
    out["switch_gradient"] = np.where(free, s * rr + sg * (c2 * oms), zero_m)
    h_s = np.where(free, rr + c2, one_m)
    out["switch_curvature"] = h_s
    keep_r, keep_q = ~fixed[ref], ~fixed[qry]

    def scatter(at_ref, at_qry):
        acc = zero_n.copy()
        if at_ref is not None:
            np.add.at(acc, ref[keep_r], at_ref[keep_r])
        if at_qry is not None:
            np.add.at(acc, qry[keep_q], at_qry[keep_q])
        return acc

    def JT(role, v):      # J_role^T v → 6 arrays
        if role == 0:
            return [sg * v[j] for j in range(3)] + [sum(A[i][j] * v[i] + B[i][j] * v[3 + i] for i in range(3)) for j in range(3)]
        return [v[j] for j in range(3)] + [sum(C[i][j] * v[3 + i] for i in range(3)) for j in range(3)]

    def J(role, u):       # J_role u → 6 arrays
        if role == 0:
            return ([sg * u[i] + A[i][0] * u[3] + A[i][1] * u[4] + A[i][2] * u[5] for i in range(3)] +
                    [B[i][0] * u[3] + B[i][1] * u[4] + B[i][2] * u[5] for i in range(3)])
        return [u[i] for i in range(3)] + [C[i][0] * u[3] + C[i][1] * u[4] + C[i][2] * u[5] for i in range(3)]

    # gradient: sum s^2 J^T r
    g_r, g_q = [s2 * v for v in JT(0, r)], [s2 * v for v in JT(1, r)]
    if skip is not None:
        for k in range(6):
            (g_r if skip[1] == 0 else g_q)[k][skip[0]] = zero_m[skip[0]]
    out["gradient"] = np.concatenate([scatter(g_r[k], g_q[k]) for k in range(6)])
    # diagonal blocks: sum s^2 J^T J
    planes = []
    for a, b in _UPPER:
        if b < 3:
            at_r = at_q = s2 if a == b else None
        elif a < 3:
            at_r, at_q = s2 * (sg * A[a][b - 3]), None
        else:
            at_r = s2 * sum(A[i][a - 3] * A[i][b - 3] + B[i][a - 3] * B[i][b - 3] for i in range(3))
            at_q = s2 * sum(C[i][a - 3] * C[i][b - 3] for i in range(3))
        plane = scatter(at_r, at_q)
        if a == b:
            plane[fixed] = 1 + zero_n[fixed]
        planes.append(plane)
    out["hdiag"] = np.stack(planes)
    # product
    X = conv(x)
    xk = [X[k * n:(k + 1) * n] for k in range(6)]
    xs_all = X[6 * n:]
    xs = np.where(free, xs_all, zero_m)
    xr = [np.where(fixed[ref], zero_m, xk[k][ref]) for k in range(6)]
    xq = [np.where(fixed[qry], zero_m, xk[k][qry]) for k in range(6)]
    u = [a + b for a, b in zip(J(0, xr), J(1, xq))]
    v = [s * u[k] + r[k] * xs for k in range(6)]
    y_r, y_q = [s * w for w in JT(0, v)], [s * w for w in JT(1, v)]
    hx = []
    for k in range(6):
        rows = scatter(y_r[k], y_q[k])
        rows[fixed] = xk[k][fixed]
        hx.append(rows)
    hs_x = np.where(free, sum(r[k] * (s * u[k]) for k in range(6)) if m else zero_m, zero_m)
    out["product"], out["switch_product"] = {}, {}
    for lam in lambdas:
        lam_c = conv(np.array([lam]))[0]
        out["product"][lam] = np.concatenate([hx[k] + lam_c * (planes[_DIAG[k]] * xk[k]) for k in range(6)])
        out["switch_product"][lam] = hs_x + (1 + lam_c) * (h_s * xs_all)
    out["r"] = r
    return out


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _abs(a):
    return np.abs(np.asarray(a, dtype=np.float64))


def reference(st, x, lambdas=LAMBDAS):
    """→ (values at DPS digits: object arrays of mpf, scales: float64 arrays), keyed by QUANTITIES"""
    with mpmath.workdps(DPS):
        xp = _assemble(st, _edge_terms(st, to_mp, -1), to_mp, -1, x, lambdas)
        r_abs = [np.array([float(abs(v)) for v in col], dtype=np.float64) for col in xp["r"]]
    dpos = _cols(np.abs(st["poses"][st["qry"], :3] - st["poses"][st["ref"], :3]))
    scale = _assemble(st, _edge_terms(st, _abs, +1, dpos=dpos), _abs, +1, x, lambdas, r_true=r_abs)
    return xp, scale


def twin(st, x, lambdas=LAMBDAS, mutate=(), skip=None, sw=None):
    """the same formulas in float64, with the planted mistakes of test_pgo_xprec.py"""
    return _assemble(st, _edge_terms(st, _f64, -1, mutate=mutate), _f64, -1, x, lambdas, skip=skip, sw=sw)


@functools.lru_cache(maxsize=None)
def family_reference(name):
    st = family(name)
    return reference(st, masked_x(st))


# ---------------------------------------------------------------- the measure

def error_eps(got, xp, scale):
    """max |got - xp| / scale in units of 2^-52; inf where the scale is 0 and the value is not exactly 0"""
    got, scale = np.asarray(got, dtype=np.float64).ravel(), np.asarray(scale, dtype=np.float64).ravel()
    xp = np.asarray(xp, dtype=object).ravel()
    assert got.shape == xp.shape == scale.shape, (got.shape, xp.shape, scale.shape)
    worst = 0.0
    with mpmath.workdps(DPS):
        for g, v, sc in zip(got.tolist(), xp.tolist(), scale.tolist()):
            if sc == 0.0:
                assert v == 0, "a zero scale with a non-zero reference value"
                if g != 0.0:
                    return float("inf")
            else:
                worst = max(worst, float(abs(mpmath.mpf(g) - v) / sc))
    return worst / EPS


def score(got, ref):
    """got: dict like _assemble's (float64); ref = (xp, scale) → {quantity: error in units of 2^-52}; the products are the
    worst over the lambdas of the reference"""
    xp, scale = ref
    out = {}
    for q in QUANTITIES:
        if q in ("product", "switch_product"):
            out[q] = max(error_eps(got[q][lam], xp[q][lam], scale[q][lam]) for lam in xp[q])
        else:
            out[q] = error_eps(got[q], xp[q], scale[q])
    return out


def gnorm_error_eps(gnorm, ref):
    """|gnorm - sqrt(sum g_xp^2)| relative to sqrt(sum scale^2), gradient and switch gradient together"""
    xp, scale = ref
    with mpmath.workdps(DPS):
        want = mpmath.sqrt(sum(v * v for v in xp["gradient"].tolist()) + sum(v * v for v in xp["switch_gradient"].tolist()))
        sc = np.sqrt(np.sum(scale["gradient"] ** 2) + np.sum(scale["switch_gradient"] ** 2))
        return float(abs(mpmath.mpf(float(gnorm)) - want) / sc) / EPS


def oracle_graph(st):
    return op.Graph(st["poses"], st["ref"], st["qry"], st["meas"], st["sw"], st["free"], st["fixed"])


def oracle_quantities(st, x, lambdas=LAMBDAS):
    """oracle_pgo.Graph.linearize() and damped() @ x in the layout of _assemble"""
    n, m = st["poses"].shape[0], st["ref"].size
    g = oracle_graph(st)
    H, grad, cost = g.linearize()
    Hd = H.toarray()
    idx = np.arange(n)
    out = {"cost": cost, "gradient": grad[:6 * n], "switch_gradient": grad[6 * n:],
           "hdiag": np.stack([Hd[a * n + idx, b * n + idx] for a, b in _UPPER]),
           "switch_curvature": Hd[6 * n + np.arange(m), 6 * n + np.arange(m)], "product": {}, "switch_product": {}}
    for lam in lambdas:
        y = g.damped(H, lam) @ x
        out["product"][lam], out["switch_product"][lam] = y[:6 * n], y[6 * n:]
    return out


def split_gpu(n, cost, gradient, hdiag, products):
    """what the library returns, in the layout of _assemble (no switch curvature: it is read through the product)"""
    out = {"cost": cost, "gradient": gradient[:6 * n], "switch_gradient": gradient[6 * n:], "hdiag": hdiag.reshape(21, n),
           "product": {lam: y[:6 * n] for lam, y in products.items()},
           "switch_product": {lam: y[6 * n:] for lam, y in products.items()}}
    return out


def bounds(yardstick):
    return {q: max(4.0 * v, 8.0) for q, v in yardstick.items()}


def yardstick(st, x, ref, lambdas=LAMBDAS):
    return score(oracle_quantities(st, x, lambdas), ref)


@functools.lru_cache(maxsize=None)
def family_yardstick(name):
    st = family(name)
    return yardstick(st, masked_x(st), family_reference(name))


# ---------------------------------------------------------------- retraction

N_PAIRS = 300
RETRACT_LAMBDA = 1e-6


@functools.lru_cache(maxsize=None)
def retraction_graph():
    """300 independent pairs (fixed pose 2k, free pose 2k+1, one constraint 2k → 2k+1; every fourth constraint carries a
    free switch at 0.7), quaternions scaled by 1 +- 1e-3 as in `non_unit`.  The measurement rotation of pair k is off by
    phi_k about a random axis, so the rotation step the solve returns has |dw| ~ phi_k: 260 angles log-spaced over
    1e-12 … 3 rad and 40 at 1e-6 (1 +- d), d in {1e-9, 1e-6, 1e-3, 3e-3} — either side of the retraction's small-angle
    branch.  The 40 sit on pairs without a switch (a free switch shares the residual with the pose step).  → state"""
    rng = np.random.default_rng(31)
    near = [1e-6 * (1 + sgn * d) for d in (1e-9, 1e-6, 1e-3, 3e-3) for sgn in (1, -1)] * 5
    wide = list(np.logspace(-12, np.log10(3.0), N_PAIRS - len(near)))
    slots_near = [k for k in range(N_PAIRS) if k % 4 != 0][3::5][:len(near)]
    assert len(slots_near) == len(near)
    phi = np.zeros(N_PAIRS)
    phi[slots_near] = near
    phi[[k for k in range(N_PAIRS) if k not in set(slots_near)]] = wide
    poses, meas = np.zeros((2 * N_PAIRS, 7)), np.zeros((N_PAIRS, 7))
    for k in range(N_PAIRS):
        qr, qq = op.qexp(rng.normal(scale=0.8, size=3)), op.qexp(rng.normal(scale=0.8, size=3))
        pr = rng.normal(scale=20.0, size=3)
        tm = rng.normal(scale=2.0, size=3)
        poses[2 * k, :3], poses[2 * k, 3:] = pr, qr
        poses[2 * k + 1, :3] = pr + op.qrot(qr) @ tm + rng.normal(scale=0.05, size=3)
        poses[2 * k + 1, 3:] = qq
        meas[k, :3] = tm
        meas[k, 3:] = op.qmul(op.qmul(op.qconj(qr), qq), op.qexp(phi[k] * _unit(rng.normal(size=3))))
    poses[:, 3:] *= rng.uniform(1 - 1e-3, 1 + 1e-3, size=(2 * N_PAIRS, 1))
    meas[:, 3:] *= rng.uniform(1 - 1e-3, 1 + 1e-3, size=(N_PAIRS, 1))
    fixed = np.zeros(2 * N_PAIRS, dtype=np.uint8)
    fixed[0::2] = 1
    free = (np.arange(N_PAIRS) % 4 == 0).astype(np.uint8)
    d = {"init": poses, "ref": 2 * np.arange(N_PAIRS), "qry": 2 * np.arange(N_PAIRS) + 1, "meas": meas, "fixed": fixed}
    return _state(d, sw=np.where(free, 0.7, 1.0), free=free, phi=phi)


def rotation_steps(n, step):
    """[n,3] rotation part of a step vector in plane order"""
    return np.stack([step[k * n:(k + 1) * n] for k in (3, 4, 5)], axis=1)


def branch_counts(dw):
    """(steps with |dw| in [0.997e-6, 1e-6), steps with |dw| in [1e-6, 1.003e-6]) — |dw| as the kernel forms it"""
    th = np.sqrt(dw[:, 0] * dw[:, 0] + dw[:, 1] * dw[:, 1] + dw[:, 2] * dw[:, 2])
    return int(np.sum((th >= 0.997e-6) & (th < 1e-6))), int(np.sum((th >= 1e-6) & (th <= 1.003e-6)))


def retract_xp(q, dw):
    """normalize(q (x) Exp(dw)) at DPS digits: sin, cos and sqrt of mpmath, no small-angle branch → [k,4] object array"""
    out = np.empty((q.shape[0], 4), dtype=object)
    with mpmath.workdps(DPS):
        for i in range(q.shape[0]):
            w = [mpmath.mpf(float(v)) for v in dw[i]]
            a = [mpmath.mpf(float(v)) for v in q[i]]
            th = mpmath.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
            k = mpmath.sin(th / 2) / th if th != 0 else mpmath.mpf(0.5)
            d = (mpmath.cos(th / 2), k * w[0], k * w[1], k * w[2])
            p = _qmul(a, d, -1)
            nrm = mpmath.sqrt(sum(v * v for v in p))
            out[i] = [v / nrm for v in p]
    return out


def quaternion_error_eps(got, xp):
    """largest absolute component error in units of 2^-52"""
    with mpmath.workdps(DPS):
        return float(max(abs(mpmath.mpf(float(g)) - v) for g, v in zip(np.asarray(got).ravel().tolist(), xp.ravel().tolist()))) / EPS


def norm_error_eps(q):
    """largest | |q| - 1 | in units of 2^-52, the norm at DPS digits"""
    with mpmath.workdps(DPS):
        return float(max(abs(mpmath.sqrt(sum(mpmath.mpf(float(v)) ** 2 for v in row)) - 1) for row in np.asarray(q))) / EPS


def oracle_retract(st, step):
    """oracle_pgo.Graph.retract on a copy of the state → (poses, switches)"""
    g = oracle_graph(st)
    g.retract(step)
    return g.poses, g.sw
