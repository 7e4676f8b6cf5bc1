"""Cases, the 50-digit reference and the yardstick of the LM step tests (tests/test_lm_step_xprec.py).  No tests here.

The step is one pass of the loop body after the sums are known (csrc/host/nos_lm.hpp LmAdvance6 / LmAdvance3; on the
device lm_step_lane, csrc/assemble_loop.hpp): damped solve, pose update, the two convergence tests, the λ schedule.

reference_step  the arithmetic of LmAdvance6 / LmAdvance3 from the doubles as given, in mpmath at 60 digits: H from the upper
                triangle with its diagonal times (1 + λ), δ = −H⁻¹ g by LU, t += δ, q ← normalise(q ⊗ Exp(δ_ω)) with the
                un-normalised (1, ω/2) below θ = 1e-6 and cos / sin beyond, R from q; planar: R2 ← R2 · Rot2(δθ).  `ok` is
                the sign of the exact LDLᵀ pivots (a pivot no finite double holds is refused as well), `done` the exact
                norms against the tolerances; the λ schedule is the IEEE statement itself (two roundings, no freedom).
numpy_step      the same statement in plain float64 numpy (np.linalg.solve, np.cos, np.sin, np.sqrt): the yardstick — what a
                straightforward double implementation loses against 60 digits.
layout          sums = {H upper, row-major | g | cost} (28 or 10), settings = {max_iterations, gradient_tolerance,
                parameter_tolerance, float_schedule}, state = {R 9 | t 3 | q wxyz | λ | previous_cost | cost | iteration |
                done | ok} (22): the arguments of nos_debug_lm_step and nos_host_lm_advance.
families        cond_ladder, rank_deficient, must_refuse, angle_ladder, decision_ladder, non_finite_rest, chain — see each
                generator.  Every generator is seeded and asserts, from the 60-digit values, that each of its cases has a
                decision margin: a case without one is an error of the generator, never a skip.
"""
import functools

import numpy as np
from mpmath import mp, mpf

EPS = 2.0 ** -52
DPS = 60
LAMBDAS = (1e-6, 2.5e-4, 1e-3, 0.0061, 1e-2)
MIN_LAMBDA, MAX_LAMBDA = 1e-6, 1e-2
DBL_MAX = float(np.finfo(np.float64).max)
TINY_THETA = 1e-6          # below: the reference's un-normalised small-angle form
SERIES_THETA = 0.125       # the device sums power series below, calls sincos beyond (6-DoF)
SERIES_DTHETA = 0.0625     # the same switch of the planar form
BUDGET = 30
I_LAMBDA, I_PREV, I_COST, I_ITER, I_DONE, I_OK = 16, 17, 18, 19, 20, 21


def tri(n):
    return [(r, c) for r in range(n) for c in range(r, n)]


def pack_sums(H, g, cost):
    n = len(g)
    H = np.asarray(H, dtype=np.float64)
    return np.concatenate([[H[r, c] for r, c in tri(n)], np.asarray(g, dtype=np.float64), [cost]])


def unpack_sums(dof, sums):
    H = np.zeros((dof, dof))
    for k, (r, c) in enumerate(tri(dof)):
        H[r, c] = H[c, r] = sums[k]
    m = dof * (dof + 1) // 2
    return H, np.array(sums[m:m + dof], dtype=np.float64), float(sums[m + dof])


def quat_to_matrix(q, one=1.0, two=2.0):
    """QuatToMatrix of nos_lm.hpp, for floats or mpf."""
    w, x, y, z = q
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
            one - (txx + tyy)]


def quat_from_matrix(R):
    """QuatFromMatrix of nos_lm.hpp restated in numpy float64 (for a signed permutation: square roots of 1, 2 and 4 and
    halvings, all exact)."""
    R = np.asarray(R, dtype=np.float64).reshape(9)
    tr = R[0] + R[4] + R[8]
    if tr > 0.0:
        s = np.sqrt(tr + 1.0)
        f = 0.5 / s
        return np.array([0.5 * s, (R[7] - R[5]) * f, (R[2] - R[6]) * f, (R[3] - R[1]) * f])
    i = 1 if R[4] > R[0] else 0
    if R[8] > R[4 * i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = np.sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0)
    f = 0.5 / s
    v = np.zeros(3)
    v[i] = 0.5 * s
    v[j] = (R[3 * j + i] + R[3 * i + j]) * f
    v[k] = (R[3 * k + i] + R[3 * i + k]) * f
    return np.array([(R[3 * k + j] - R[3 * j + k]) * f, v[0], v[1], v[2]])


def make_state(dof, q=None, angle=0.0, t=(0.0, 0.0, 0.0), lam=1e-3, prev=DBL_MAX, iteration=0):
    st = np.zeros(22)
    if dof == 6:
        q = np.array([1.0, 0.0, 0.0, 0.0]) if q is None else np.asarray(q, dtype=np.float64)
        st[:9] = quat_to_matrix(q)
        st[12:16] = q
    else:
        st[:4] = [np.cos(angle), -np.sin(angle), np.sin(angle), np.cos(angle)]
        st[12] = 1.0
    st[9:12] = t
    st[I_LAMBDA], st[I_PREV], st[I_COST], st[I_ITER], st[I_DONE], st[I_OK] = lam, prev, prev, iteration, 0, 1
    return st


# ---------------------------------------------------------------- the λ schedule: IEEE by construction

def schedule(lam, cost, prev, float_schedule):
    """NextLambda / NextLambdaFloat and the cost bookkeeping of nos_lm.hpp → (λ', previous_cost', up, clamp_lo, clamp_hi)."""
    with np.errstate(all="ignore"):
        up = bool(np.float64(cost) > np.float64(prev))
        factor = np.float64(2.0 if up else 0.6)
        if float_schedule:
            l = np.float32(np.float64(np.float32(lam)) * factor)
            lo, hi = np.float32(1e-6), np.float32(1e-2)
            new_prev = float(np.float64(np.float32(cost)))
        else:
            l = np.float64(lam) * factor
            lo, hi = np.float64(MIN_LAMBDA), np.float64(MAX_LAMBDA)
            new_prev = float(cost)
        clamp_lo, clamp_hi = bool(l < lo), bool(l > hi)
        l = lo if clamp_lo else (hi if clamp_hi else l)
    return float(l), new_prev, up, clamp_lo, clamp_hi


# ---------------------------------------------------------------- the 60-digit reference

def _ldlt_pivots(A, n):
    """Pivots of the unpivoted LDLᵀ, up to and including the first that is not positive."""
    a = [[A[i, k] for k in range(n)] for i in range(n)]
    piv = []
    for j in range(n):
        d = a[j][j]
        piv.append(d)
        if not d > 0:
            break
        for i in range(j + 1, n):
            l = a[i][j] / d
            for k in range(j + 1, i + 1):
                a[i][k] -= l * a[k][j]
    return piv


def _norm(v):
    return mp.sqrt(sum((x * x for x in v), mpf(0)))


def reference_step(dof, sums, settings, state, want_kappa=False):
    """One step from the doubles (or mpf, for a chain) as given → dict:
    ok, done, iteration, lambda, previous_cost, cost: the decisions (floats / ints, exact);
    R, t, q: the pose after the step as mpf lists (the input's values where the solve is refused; None where the step is
    not finite); delta, theta (|δ_ω| or |δθ|), norm_step, norm_g, pivots, kappa (with want_kappa);
    converged, up, down, clamp_lo, clamp_hi, float_applied, budget_end, branch: what the step went through."""
    with mp.workdps(DPS):
        n = dof
        nums = [float(x) for x in sums]
        H_np, g_np, cost = unpack_sums(n, nums)
        lam = float(state[I_LAMBDA])
        out = dict(ok=1, done=int(state[I_DONE]), iteration=int(state[I_ITER]), previous_cost=float(state[I_PREV]),
                   cost=cost, converged=False, up=False, down=False, clamp_lo=False, clamp_hi=False, float_applied=False,
                   budget_end=False, branch=None, kappa=None, delta=None, theta=None, pivots=None, norm_step=None, norm_g=None)
        out["lambda"] = lam
        R0 = [mpf(x) for x in state[:9]]
        t0 = [mpf(x) for x in state[9:12]]
        q0 = [mpf(x) for x in state[12:16]]
        out["R"], out["t"], out["q"] = R0, t0, q0
        refused = not np.all(np.isfinite(H_np))
        if not refused:
            Hd = mp.matrix(n, n)
            for r in range(n):
                for c in range(n):
                    Hd[r, c] = mpf(H_np[r, c]) * (1 + mpf(lam)) if r == c else mpf(H_np[r, c])
            piv = _ldlt_pivots(Hd, n)
            out["pivots"] = piv
            refused = len(piv) < n or not all(0 < d <= mpf(DBL_MAX) for d in piv)
        if refused:
            out["ok"], out["done"], out["branch"] = 0, 1, "refused"
            return out
        if want_kappa:
            ev = [abs(e) for e in mp.eigsy(Hd, eigvals_only=True)]
            out["kappa"] = max(ev) / min(ev)
        g_norm_ok = bool(np.all(np.isfinite(g_np)))
        ptol, gtol = mpf(float(settings[2])), mpf(float(settings[1]))
        if g_norm_ok:
            delta = list(mp.lu_solve(Hd, mp.matrix([-mpf(x) for x in g_np])))
            out["delta"] = delta
            ns, ng = _norm(delta), _norm([mpf(x) for x in g_np])
            out["norm_step"], out["norm_g"] = ns, ng
            out["t"] = [t0[k] + delta[k] if k < (3 if n == 6 else 2) else t0[k] for k in range(3)]
            if n == 6:
                w = delta[3:6]
                th = _norm(w)
                out["theta"] = th
                if th < mpf(TINY_THETA):
                    d = [mpf(1), w[0] / 2, w[1] / 2, w[2] / 2]
                    out["branch"] = "tiny"
                else:
                    k = mp.sin(th / 2) / th
                    d = [mp.cos(th / 2), k * w[0], k * w[1], k * w[2]]
                    out["branch"] = "series" if th < mpf(SERIES_THETA) else "sincos"
                a = q0
                r = [a[0] * d[0] - a[1] * d[1] - a[2] * d[2] - a[3] * d[3],
                     a[0] * d[1] + a[1] * d[0] + a[2] * d[3] - a[3] * d[2],
                     a[0] * d[2] + a[2] * d[0] + a[3] * d[1] - a[1] * d[3],
                     a[0] * d[3] + a[3] * d[0] + a[1] * d[2] - a[2] * d[1]]
                nr = _norm(r)
                q = [x / nr for x in r]
                out["q"] = q
                out["R"] = quat_to_matrix(q, mpf(1), mpf(2))
            else:
                dth = delta[2]
                out["theta"] = abs(dth)
                out["branch"] = "planar_series" if abs(dth) < mpf(SERIES_DTHETA) else "planar_sincos"
                c, s = mp.cos(dth), mp.sin(dth)
                a, b, d_, e = R0[:4]
                out["R"] = [a * c + b * s, b * c - a * s, d_ * c + e * s, e * c - d_ * s] + R0[4:]
            converged = bool(ns < ptol) or bool(ng < gtol)
        else:  # NaN in g: the solve "succeeds", no comparison with a NaN holds
            out["R"] = out["t"] = out["q"] = None
            out["branch"] = "nan_step"
            converged = False
        if converged:
            out["converged"], out["done"] = True, 1
            return out
        fl = int(settings[3]) != 0
        out["lambda"], out["previous_cost"], up, out["clamp_lo"], out["clamp_hi"] = schedule(lam, cost, state[I_PREV], fl)
        out["up"], out["down"] = out["lambda"] > lam, out["lambda"] < lam
        out["float_applied"] = fl
        out["iteration"] += 1
        if out["iteration"] >= int(settings[0]):
            out["done"], out["budget_end"] = 1, True
        return out


def decisions(ref):
    """The reference's decisions in the layout of state[16:22]."""
    return np.array([ref["lambda"], ref["previous_cost"], ref["cost"], ref["iteration"], ref["done"], ref["ok"]],
                    dtype=np.float64)


# ---------------------------------------------------------------- the yardstick

def numpy_step(dof, sums, settings, state):
    """The step in plain float64 numpy → the new state (pose fields; the decisions are the straightforward ones)."""
    n = dof
    H, g, cost = unpack_sums(n, sums)
    st = np.array(state, dtype=np.float64)
    lam = st[I_LAMBDA]
    st[I_COST] = cost
    Hd = H.copy()
    Hd[np.diag_indices(n)] *= 1.0 + lam
    with np.errstate(all="ignore"):
        try:
            np.linalg.cholesky(Hd)
            delta = np.linalg.solve(Hd, -g)
        except np.linalg.LinAlgError:
            st[I_OK], st[I_DONE] = 0, 1
            return st
        if n == 6:
            st[9:12] += delta[:3]
            w = delta[3:]
            th = np.sqrt(np.sum(w * w))
            if th < TINY_THETA:
                d = np.array([1.0, 0.5 * w[0], 0.5 * w[1], 0.5 * w[2]])
            else:
                k = np.sin(0.5 * th) / th
                d = np.array([np.cos(0.5 * th), k * w[0], k * w[1], k * w[2]])
            a = st[12:16]
            r = np.array([a[0] * d[0] - a[1] * d[1] - a[2] * d[2] - a[3] * d[3],
                          a[0] * d[1] + a[1] * d[0] + a[2] * d[3] - a[3] * d[2],
                          a[0] * d[2] + a[2] * d[0] + a[3] * d[1] - a[1] * d[3],
                          a[0] * d[3] + a[3] * d[0] + a[1] * d[2] - a[2] * d[1]])
            q = r / np.sqrt(np.sum(r * r))
            st[12:16] = q
            st[:9] = quat_to_matrix(q)
        else:
            st[9:11] += delta[:2]
            c, s = np.cos(delta[2]), np.sin(delta[2])
            a, b, d_, e = st[:4]
            st[:4] = [a * c + b * s, b * c - a * s, d_ * c + e * s, e * c - d_ * s]
        if np.sqrt(np.sum(delta * delta)) < settings[2] or np.sqrt(np.sum(g * g)) < settings[1]:
            st[I_DONE] = 1
            return st
        st[I_LAMBDA], st[I_PREV] = schedule(lam, cost, st[I_PREV], int(settings[3]) != 0)[:2]
        st[I_ITER] += 1
        if st[I_ITER] >= settings[0]:
            st[I_DONE] = 1
    return st


# ---------------------------------------------------------------- errors, in eps

def solve_error(dof, got, ref):
    """e = ‖δ − δ*‖ / ‖δ*‖ / (eps κ₂) of a solve-family case (identity start rotation, t = 0): δ read back from the pose —
    the translation part is t' itself, the rotation part the logarithm of q' (R2') taken at 60 digits, counted while
    |δ_ω*| ≤ 1 (beyond, only the translation part is counted, still against the whole ‖δ*‖)."""
    with mp.workdps(DPS):
        d = ref["delta"]
        nt = 3 if dof == 6 else 2
        err2 = sum(((mpf(float(got[9 + k])) - d[k]) ** 2 for k in range(nt)), mpf(0))
        if ref["theta"] <= 1:
            if dof == 6:
                w, v = mpf(float(got[12])), [mpf(float(x)) for x in got[13:16]]
                if ref["branch"] == "tiny":
                    rec = [2 * x / w for x in v]  # q' is (1, ω/2) over its norm
                else:
                    nv = _norm(v)
                    rec = [x / nv * 2 * mp.atan2(nv, w) for x in v] if nv > 0 else [mpf(0)] * 3
                err2 += sum(((rec[k] - d[3 + k]) ** 2 for k in range(3)), mpf(0))
            else:
                rec = mp.atan2(-mpf(float(got[1])), mpf(float(got[0])))
                err2 += (rec - d[2]) ** 2
        return float(mp.sqrt(err2) / ref["norm_step"] / (mpf(EPS) * ref["kappa"]))


def pose_errors(dof, got, ref):
    """→ dict of the pose errors in eps: q (max |q − q*|), R (max |R − R*|), t (|t − t*| / (|t*| + |δ*|)), unit (||q| − 1|);
    the planar form has no q."""
    with mp.workdps(DPS):
        nr = 9 if dof == 6 else 4
        out = {"R": float(max(abs(mpf(float(got[k])) - ref["R"][k]) for k in range(nr)) / EPS)}
        nt = 3 if dof == 6 else 2
        dt = _norm([mpf(float(got[9 + k])) - ref["t"][k] for k in range(nt)])
        out["t"] = float(dt / (_norm(ref["t"][:nt]) + _norm(ref["delta"][:nt])) / EPS)
        if dof == 6:
            out["q"] = float(max(abs(mpf(float(got[12 + k])) - ref["q"][k]) for k in range(4)) / EPS)
            out["unit"] = float(abs(_norm([mpf(float(x)) for x in got[12:16]]) - 1) / EPS)
        return out


def drift_errors(dof, got):
    """→ (||q| − 1|, ‖RᵀR − I‖_max) in eps, from the doubles at 60 digits (planar: the 2x2 block, no q)."""
    with mp.workdps(DPS):
        m = 3 if dof == 6 else 2
        R = [[mpf(float(got[m * r + c])) for c in range(m)] for r in range(m)]
        orth = max(abs(sum(R[k][i] * R[k][j] for k in range(m)) - (1 if i == j else 0)) for i in range(m) for j in range(m))
        unit = abs(_norm([mpf(float(x)) for x in got[12:16]]) - 1) if dof == 6 else mpf(0)
        return float(unit / EPS), float(orth / EPS)


# ---------------------------------------------------------------- cases

class Case:
    def __init__(self, family, dof, sums, settings, state, tag, pose=True):
        self.family, self.dof, self.tag = family, dof, tag
        self.sums = np.ascontiguousarray(sums, dtype=np.float64)
        self.settings = np.ascontiguousarray(settings, dtype=np.float64)
        self.state = np.ascontiguousarray(state, dtype=np.float64)
        self.pose = pose  # False: the case pins the decisions only
        self.ref = None

    def __repr__(self):
        return "%s/%d/%s" % (self.family, self.dof, self.tag)


def _bookkeeping(rng, k, dof, cost=None):
    """λ from LAMBDAS, cost above / below the previous cost, iteration 0 / 7 / last of the budget, either schedule."""
    cost = float(10.0 ** rng.uniform(-3, 4)) if cost is None else cost
    lam = LAMBDAS[k % 5]
    prev = cost * (0.5 if (k // 5) % 2 else 2.0)
    fl = (k // 2) % 2
    if fl:
        lam, prev = float(np.float32(lam)), float(np.float32(prev))
    return cost, lam, prev, [0, 7, BUDGET - 1][k % 3], fl


def _exact_norms(dof, H, g, lam):
    """‖δ*‖ and ‖g‖ of a system, at 60 digits."""
    st = make_state(dof, lam=lam)
    ref = reference_step(dof, pack_sums(H, g, 1.0), [BUDGET, 0.0, 0.0, 0], st)
    assert ref["ok"] == 1, ref["pivots"]
    return ref["norm_step"], ref["norm_g"]


def _sided_tolerances(kind, ns, ng):
    """Tolerances a factor 2 away from the exact norms, each on a chosen side → (gtol, ptol, converges)."""
    ns, ng = float(ns), float(ng)
    if kind == 0:
        return 0.0, 2.0 * ns, True      # the step is below its tolerance
    if kind == 1:
        return 0.5 * ng, 0.5 * ns, False  # both above
    if kind == 2:
        return 2.0 * ng, 0.5 * ns, True   # the gradient is below its tolerance
    return 0.0, 0.0, False              # both tests off


def _assert_margin(case, factor):
    """Each armed test lies at least `factor` (relative) away from its tolerance."""
    ref = case.ref
    with mp.workdps(DPS):
        for norm, tol in ((ref["norm_step"], case.settings[2]), (ref["norm_g"], case.settings[1])):
            if tol > 0 and norm is not None:
                assert abs(norm / mpf(float(tol)) - 1) >= factor, (case, float(norm), tol)


def _orthogonal(rng, n, mix=None):
    a = rng.standard_normal((n, n)) if mix is None else np.eye(n) + mix * rng.standard_normal((n, n))
    q, r = np.linalg.qr(a)
    return q * np.sign(np.diag(r))


COND_EXPONENTS = (0, 2, 4, 6, 8, 10, 12, 14, 15)
COND_SCALES = (-200, 0, 200)


def cond_ladder():
    """H = Q diag(10^0 … 10^-k) Qᵀ, g random and scaled (by a power of two) to a step of 2^-1 … 2^-11; three seeds with a
    random orthogonal Q — the multiplicative damping then caps κ₂ of the damped matrix near n / λ — and one with
    Q = I + O(10^(-k/2)), whose damped matrix keeps κ₂ ≈ 10^k.  Each system also times 2^-200 and 2^+200 (H and g alike:
    the same step).  Identity start rotation and t = 0, so that the pose after the step holds δ itself."""
    cases = []
    for dof in (6, 3):
        for ik, k in enumerate(COND_EXPONENTS):
            for seed in range(4):
                rng = np.random.default_rng([20261020, 1, dof, k, seed])
                Q = _orthogonal(rng, dof, None if seed < 3 else 10.0 ** (-k / 2.0))
                H = (Q * 10.0 ** (-k * np.arange(dof) / (dof - 1.0))) @ Q.T
                H = np.triu(H) + np.triu(H, 1).T
                idx = ik * 4 + seed
                cost, lam, prev, it, fl = _bookkeeping(rng, idx, dof)
                g = rng.standard_normal(dof)
                ns, _ = _exact_norms(dof, H, g, lam)
                want = 2.0 ** -int(rng.integers(1, 12))
                g = g * 2.0 ** int(mp.floor(mp.log(want / ns, 2)))
                ns, ng = _exact_norms(dof, H, g, lam)
                gtol, ptol, _ = _sided_tolerances(idx % 4, ns, ng)
                for e in COND_SCALES:
                    sc = 2.0 ** e
                    cases.append(Case("cond_ladder", dof, pack_sums(H * sc, g * sc, cost), [BUDGET, gtol * sc, ptol, fl],
                                      make_state(dof, lam=lam, prev=prev, iteration=it), "k%d_s%d_e%d" % (k, seed, e)))
    return cases


def rank_deficient():
    """H = AᵀA, g = Aᵀb 2^-s with small-integer A of rank 1 … n−1 (a product of two integer factors) and no zero column:
    exactly singular, exactly representable, solvable through the damping alone."""
    cases = []
    for dof in (6, 3):
        for rank in range(1, dof):
            for seed in range(30 if dof == 6 else 35):
                rng = np.random.default_rng([20261020, 2, dof, rank, seed])
                while True:
                    A = rng.integers(-2, 3, size=(dof + 2, rank)) @ rng.integers(-3, 4, size=(rank, dof))
                    if np.linalg.matrix_rank(A) == rank and np.all(np.any(A != 0, axis=0)):
                        break
                b = rng.integers(-4, 5, size=dof + 2)
                if not np.any(A.T @ b):
                    b[0] += 1 if np.any((A.T)[:, 0]) else 0
                H = (A.T @ A).astype(np.float64)
                g = (A.T @ b).astype(np.float64) * 2.0 ** -int(rng.integers(0, 8))
                if not np.any(g):
                    g = H[0].copy()
                idx = rank * 40 + seed
                cost, lam, prev, it, fl = _bookkeeping(rng, idx, dof)
                ns, ng = _exact_norms(dof, H, g, lam)
                gtol, ptol, _ = _sided_tolerances(idx % 4, ns, ng)
                cases.append(Case("rank_deficient", dof, pack_sums(H, g, cost), [BUDGET, gtol, ptol, fl],
                                  make_state(dof, lam=lam, prev=prev, iteration=it), "r%d_s%d" % (rank, seed)))
    return cases


def _spd(rng, n):
    a = rng.standard_normal((n + 2, n))
    return a.T @ a


def must_refuse():
    """Systems the damped solve must refuse: no match at all, an unobserved degree of freedom, −H, an exact LDLᵀ with one
    pivot −1, a diagonal entry whose damped value overflows, NaN / ±Inf in H."""
    cases = []
    kinds = ("zero", "zero_diag", "negated", "ldlt_minus", "inf_pivot", "nan_diag", "nan_off", "inf_diag", "inf_off",
             "minus_inf_off")
    for dof in (6, 3):
        for ki, kind in enumerate(kinds):
            for seed in range(4):
                rng = np.random.default_rng([20261020, 3, dof, ki, seed])
                H = _spd(rng, dof)
                g = rng.standard_normal(dof)
                i = int(rng.integers(dof))
                j = (i + 1 + int(rng.integers(dof - 1))) % dof
                if kind == "zero":
                    H, g = np.zeros((dof, dof)), np.zeros(dof)
                elif kind == "zero_diag":
                    H[i, :] = H[:, i] = 0.0
                elif kind == "negated":
                    H = -H
                elif kind == "ldlt_minus":
                    L = np.tril(rng.integers(-2, 3, size=(dof, dof)), -1) + np.eye(dof)
                    D = np.ones(dof)
                    D[i] = -1.0
                    H = (L * D) @ L.T
                elif kind == "inf_pivot":
                    H[i, i] = DBL_MAX
                elif kind == "nan_diag":
                    H[i, i] = np.nan
                elif kind == "nan_off":
                    H[i, j] = H[j, i] = np.nan
                elif kind == "inf_diag":
                    H[i, i] = np.inf
                elif kind == "inf_off":
                    H[i, j] = H[j, i] = np.inf
                else:
                    H[i, j] = H[j, i] = -np.inf
                idx = ki * 4 + seed
                cost, lam, prev, it, fl = _bookkeeping(rng, idx, dof)
                if kind == "ldlt_minus":
                    lam = LAMBDAS[idx % 3]  # small enough that the damped pivot stays near −1
                    lam = float(np.float32(lam)) if fl else lam
                q = rng.standard_normal(4)
                st = make_state(dof, q=q / np.linalg.norm(q), angle=rng.uniform(-3, 3), t=rng.standard_normal(3), lam=lam,
                                prev=prev, iteration=it)
                cases.append(Case("must_refuse", dof, pack_sums(H, g, cost), [BUDGET, 1e-7, 1e-7, fl], st,
                                  "%s_s%d" % (kind, seed), pose=False))
    return cases


def _assert_refusal_margin(case):
    """The pivots before the refusing one are well positive; the refusing one is exactly zero, well negative, beyond the
    double range, or H is not finite."""
    ref = case.ref
    assert ref["ok"] == 0, case
    if ref["pivots"] is None:
        return
    diag = np.abs(np.diag(unpack_sums(case.dof, case.sums)[0]))
    piv = [float(d) if d <= mpf(DBL_MAX) else np.inf for d in ref["pivots"]]
    j = [k for k, d in enumerate(piv) if not 0 < d < np.inf][0]
    assert all(piv[k] > 1e-3 * diag[k] for k in range(j)), (case, piv)
    assert piv[j] == 0.0 or piv[j] < -1e-3 * max(diag[j], 1.0) or piv[j] == np.inf, (case, piv)


ANGLES6 = (1e-9, 1e-6 * (1 - 2.0 ** -20), 1e-6 * (1 + 2.0 ** -20), 1e-4, 0.125 * (1 - 2.0 ** -20),
           0.125 * (1 + 2.0 ** -20), 0.5, np.pi * (1 - 2.0 ** -20), np.pi * (1 + 2.0 ** -20), 2 * np.pi, 40.0)
ANGLES3 = (0.0625 * (1 - 2.0 ** -20), 0.0625 * (1 + 2.0 ** -20), -0.0625 * (1 - 2.0 ** -20), -0.0625 * (1 + 2.0 ** -20),
           np.pi, -np.pi, 40.0, -40.0, 1e-9, 1e-4, 0.5)


def _start_quaternions(rng):
    out = []
    for _ in range(3):
        q = rng.standard_normal(4)
        out.append(q / np.linalg.norm(q))
    q = rng.standard_normal(4)
    q[0] = -abs(q[0]) - 0.5
    out.append(q / np.linalg.norm(q))             # w < 0
    q = np.array([1e-9, 1.0, -2e-9, 3e-9]) * np.array([rng.uniform(0.5, 1), 1, 1, 1])
    out.append(q / np.linalg.norm(q))             # ≈ (0, 1, 0, 0)
    out.append(np.array([1.0, 0.0, 0.0, 0.0]))
    return out


def angle_ladder():
    """H = h I: g dictates the step.  |δ_ω| on both sides of every switch of the exponential map and at large angles;
    random axes, start orientations including w < 0 and q ≈ (0, 1, 0, 0)."""
    cases = []
    idx = 0
    for dof, angles in ((6, ANGLES6), (3, ANGLES3)):
        for ia, ang in enumerate(angles):
            rng = np.random.default_rng([20261020, 4, dof, ia])
            starts = _start_quaternions(rng)
            for s in range(6):
                idx += 1
                h = float(10.0 ** rng.uniform(-2, 3))
                cost, lam, prev, it, fl = _bookkeeping(rng, idx, dof)
                want = np.zeros(dof)
                if dof == 6:
                    axis = rng.standard_normal(3)
                    want[3:] = ang * axis / np.linalg.norm(axis)
                    want[:3] = rng.standard_normal(3) * 10.0 ** rng.uniform(-3, 0)
                else:
                    want[2] = ang
                    want[:2] = rng.standard_normal(2) * 10.0 ** rng.uniform(-3, 0)
                g = -want * (h * (1.0 + lam))
                st = make_state(dof, q=starts[s], angle=rng.uniform(-np.pi, np.pi), t=rng.standard_normal(3) * 10.0, lam=lam,
                                prev=prev, iteration=it)
                c = Case("angle_ladder", dof, pack_sums(h * np.eye(dof), g, cost), [BUDGET, 0.0, 0.0, fl], st,
                         "a%d_s%d" % (ia, s))
                c.want_theta = abs(ang)
                cases.append(c)
    return cases


def _assert_angle_side(case):
    """The exact angle lies on the side of every switch that its rung names (the 2^-20 offsets dwarf the rounding of g)."""
    th = case.ref["theta"]
    with mp.workdps(DPS):
        assert abs(th / mpf(case.want_theta) - 1) < mpf(2) ** -40, (case, float(th))
        for sw in (TINY_THETA, SERIES_THETA, SERIES_DTHETA):
            assert (th < mpf(sw)) == (case.want_theta < sw), (case, sw)
            assert abs(th / mpf(sw) - 1) > mpf(2) ** -21, (case, sw)


DECISION_RUNGS = (48, 44, 40, 20, 1)


def decision_ladder():
    """H = h I.  The exact |δ| at ptol (1 ± 2^-j), or the exact |g| at gtol (1 ± 2^-j), the other test off; tolerances and
    norms whose squares leave the double range."""
    cases = []
    idx = 0

    def add(dof, rng, h, g, gtol, ptol, tag):
        nonlocal idx
        idx += 1
        cost, lam, prev, it, fl = _bookkeeping(rng, idx, dof)
        q = rng.standard_normal(4)
        st = make_state(dof, q=q / np.linalg.norm(q), angle=rng.uniform(-3, 3), t=rng.standard_normal(3), lam=lam, prev=prev,
                        iteration=it)
        sums = pack_sums(h * np.eye(dof), g, cost)
        if callable(ptol) or callable(gtol):  # placed against the exact norm of this very system
            ref = reference_step(dof, sums, [BUDGET, 0.0, 0.0, fl], st)
            ptol = float(ptol(ref["norm_step"])) if callable(ptol) else ptol
            gtol = float(gtol(ref["norm_g"])) if callable(gtol) else gtol
        cases.append(Case("decision_ladder", dof, sums, [BUDGET, gtol, ptol, fl], st, tag))

    for dof in (6, 3):
        for j in DECISION_RUNGS:
            for sign in (-1, 1):
                for seed in range(2):
                    rng = np.random.default_rng([20261020, 5, dof, j, sign + 1, seed])
                    h = float(10.0 ** rng.uniform(-2, 3))
                    g = rng.standard_normal(dof) * 10.0 ** rng.uniform(-8, -2)
                    place = lambda norm, sign=sign, j=j: norm / (1 + sign * mpf(2) ** -j)  # noqa: E731
                    add(dof, rng, h, g, 0.0, place, "step_j%d_%+d_s%d" % (j, sign, seed))
                    add(dof, rng, h, g, place, 0.0, "grad_j%d_%+d_s%d" % (j, sign, seed))
        rng = np.random.default_rng([20261020, 6, dof])
        for ptol in (1e-170, 1e-160):
            for f in (0.1, 10.0):
                u = rng.standard_normal(dof)
                add(dof, rng, 1.0, u / np.linalg.norm(u) * (ptol * f), 0.0, ptol, "ptol%g_x%g" % (ptol, f))
        for gn, h in ((1e-170, 1.0), (1e200, 2.0 ** 700)):
            for gtol in (1e-160, 1e-6, 1e160):
                u = rng.standard_normal(dof)
                add(dof, rng, h, u / np.linalg.norm(u) * gn, gtol, 0.0, "g%g_gtol%g" % (gn, gtol))
        for gn, gtol in ((1e160, 1e170), (1e180, 1e170), (1e-165, 1e-175)):  # both squares out of range, either side
            u = rng.standard_normal(dof)
            add(dof, rng, 2.0 ** 600 if gn > 1 else 1.0, u / np.linalg.norm(u) * gn, gtol, 0.0, "g%g_gtol%g" % (gn, gtol))
    return cases


def non_finite_rest():
    """NaN in g (the solve "succeeds" with a NaN step: no test may fire, the schedule runs) and a NaN or infinite cost with
    a finite previous cost (NaN counts as "not above").  These pin the decisions only."""
    cases = []
    idx = 0
    for dof in (6, 3):
        for kind, count in (("nan_g", 10), ("nan_cost", 8), ("inf_cost", 8), ("minus_inf_cost", 4)):
            for seed in range(count):
                idx += 1
                rng = np.random.default_rng([20261020, 7, dof, idx])
                H = _spd(rng, dof)
                g = rng.standard_normal(dof) * 0.1
                cost, lam, prev, it, fl = _bookkeeping(rng, idx, dof)
                gtol, ptol = 1e-7, 1e-7
                if kind == "nan_g":
                    g[seed % dof] = np.nan
                else:
                    ns, ng = _exact_norms(dof, H, g, lam)
                    gtol, ptol = 0.5 * float(ng), 0.5 * float(ns)
                    cost = {"nan_cost": np.nan, "inf_cost": np.inf, "minus_inf_cost": -np.inf}[kind]
                q = rng.standard_normal(4)
                st = make_state(dof, q=q / np.linalg.norm(q), angle=rng.uniform(-3, 3), t=rng.standard_normal(3), lam=lam,
                                prev=prev, iteration=it)
                cases.append(Case("non_finite_rest", dof, pack_sums(H, g, cost), [BUDGET, gtol, ptol, fl], st,
                                  "%s_s%d" % (kind, seed), pose=False))
    return cases


CHAIN_STEPS = 256


def chain(dof):
    """256 successive steps with rotation increments of 0.01 – 0.3 rad: (start state, settings, [sums of each step]).  The
    tests are off and the budget is out of reach, so the λ of step k is the schedule's, known beforehand; g = −H_d(λ_k) δ_k
    rounded to double, whatever that makes of δ_k at 60 digits."""
    rng = np.random.default_rng([20261020, 8, dof])
    q = rng.standard_normal(4)
    st = make_state(dof, q=q / np.linalg.norm(q), angle=rng.uniform(-3, 3), t=rng.standard_normal(3), lam=1e-3, prev=1e3)
    settings = np.array([10 * CHAIN_STEPS, 0.0, 0.0, 0.0])
    lam, prev = st[I_LAMBDA], st[I_PREV]
    sums = []
    for _ in range(CHAIN_STEPS):
        H = _spd(rng, dof)
        want = rng.standard_normal(dof) * 0.1
        ang = rng.uniform(0.01, 0.3)
        if dof == 6:
            want[3:] *= ang / np.linalg.norm(want[3:])
        else:
            want[2] = ang * rng.choice([-1.0, 1.0])
        Hd = H.copy()
        Hd[np.diag_indices(dof)] *= 1.0 + lam
        cost = float(10.0 ** rng.uniform(-3, 4))
        sums.append(pack_sums(H, -Hd @ want, cost))
        lam, prev = schedule(lam, cost, prev, False)[:2]
    return st, settings, sums


def reference_chain(dof):
    """The chain at 60 digits, its pose carried in mpf → the references of the 256 steps."""
    st, settings, sums = chain(dof)
    state = list(st)
    refs = []
    for s in sums:
        ref = reference_step(dof, s, settings, state)
        assert ref["ok"] == 1 and ref["done"] == 0
        state = list(ref["R"]) + list(ref["t"]) + list(ref["q"]) + [ref["lambda"], ref["previous_cost"], ref["cost"],
                                                                     ref["iteration"], ref["done"], ref["ok"]]
        refs.append(ref)
    return refs


SOLVE_FAMILIES = ("cond_ladder", "rank_deficient")
FAMILIES = {"cond_ladder": cond_ladder, "rank_deficient": rank_deficient, "must_refuse": must_refuse,
            "angle_ladder": angle_ladder, "decision_ladder": decision_ladder, "non_finite_rest": non_finite_rest}
MIN_CASES = {"cond_ladder": 200, "rank_deficient": 200, "must_refuse": 50, "angle_ladder": 50, "decision_ladder": 50,
             "non_finite_rest": 50}


@functools.lru_cache(maxsize=None)
def cases(family):
    """The cases of one family with their references (computed once per process) and their margins asserted."""
    out = FAMILIES[family]()
    assert len(out) >= MIN_CASES[family] and {c.dof for c in out} == {6, 3}, (family, len(out))
    for c in out:
        c.ref = reference_step(c.dof, c.sums, c.settings, c.state, want_kappa=family in SOLVE_FAMILIES)
        if family in SOLVE_FAMILIES:
            assert c.ref["ok"] == 1 and min(c.ref["pivots"]) > 0, c
            _assert_margin(c, 0.49)
        elif family == "must_refuse":
            _assert_refusal_margin(c)
        elif family == "angle_ladder":
            assert c.ref["ok"] == 1, c
            _assert_angle_side(c)
        elif family == "decision_ladder":
            assert c.ref["ok"] == 1, c
            _assert_margin(c, 2.0 ** -49)  # the 2^-48 rung less the rounding of the tolerance: 8 eps and more
        else:
            assert c.ref["ok"] == 1, c
            _assert_margin(c, 0.49)
    return tuple(out)


def all_cases():
    return [c for f in FAMILIES for c in cases(f)]
