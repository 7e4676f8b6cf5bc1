"""Inputs and yardsticks of the scan deskew tests (tests/test_scan_deskew_host.py, tests/test_scan_deskew.py).  No tests here.

restate  the rule of nos_scan_deskew (include/nos.h) in plain numpy float64, in the form the rule is written:
         phi = tau w, theta = |phi|, p' = p + a phi x p + b phi x (phi x p) + u + b phi x u + c phi x (phi x u).
truth    the same from the doubles as given, in mpmath at 50 digits (more where theta is so small that 1 - cos theta and
         theta - sin theta would otherwise cancel to nothing).
error    max_k |got_k - truth_k| / (max_k |p_k| + |tau| max_k |v_k|) per point, in units of eps = 2^-52.
families 600 points uniform in +-100 m, s uniform in [0, 1], each used at s_ref = 0, 0.5 and 1."""
import mpmath
import numpy as np

from nonlinear_optimizer_for_slam_amd.pipeline import _SERIES_THETA

EPS = 2.0 ** -52
S_REFS = (0.0, 0.5, 1.0)
N_POINTS = 600

_W_THR = 0.5  # three equal components: |w| = 0.866, so theta = |tau| |w| passes 0.25 inside every sweep (|tau| up to 0.5 or 1)

FAMILIES = {  # name: (v, w)
    "typ": ((1.5, -0.2, 0.05), (0.01, -0.02, 0.3)),      # a car
    "fast": ((30.0, 5.0, -2.0), (1.0, -2.0, 3.0)),       # theta up to 3.7
    "tiny": ((1.0, 2.0, 3.0), (1e-9, 2e-9, -1e-9)),      # the small-angle arm
    "thr": ((1.0, 2.0, 3.0), (_W_THR, _W_THR, _W_THR)),  # both arms of c
    "denorm": ((1.0, 0.0, 0.0), (1e-170, 0.0, 0.0)),     # theta^2 underflows to 0
    "big": ((0.0, 0.0, 0.0), (0.0, 0.0, 40.0)),          # argument reduction, theta up to 40
    "pure_t": ((1.0, 2.0, 3.0), (0.0, 0.0, 0.0)),        # w = 0 exactly
}


def twist_of(name):
    v, w = FAMILIES[name]
    return np.array(v + w, dtype=np.float64)


def family(name):
    """→ (points [600,3], times [600], twist [6]); the same points and times for every family."""
    rng = np.random.default_rng(20261020)
    p = rng.uniform(-100.0, 100.0, size=(N_POINTS, 3))
    s = rng.uniform(0.0, 1.0, size=N_POINTS)
    return p, s, twist_of(name)


def thr_straddles(s, s_ref):
    """Does the thr family put points on both sides of the implementation's series threshold at this s_ref?"""
    theta = np.abs(s - s_ref) * np.sqrt(3.0) * _W_THR
    return bool(np.any(theta < _SERIES_THETA) and np.any(theta > _SERIES_THETA))


def restate(p, s, s_ref, twist):
    """The rule in numpy float64.  p [n,3], s [n] → [n,3]."""
    p = np.asarray(p, dtype=np.float64)
    twist = np.asarray(twist, dtype=np.float64)
    v, w = twist[:3], twist[3:]
    tau = (np.asarray(s, dtype=np.float64) - s_ref)[:, None]
    phi, u = tau * w, tau * v
    q = np.sum(phi * phi, axis=1, keepdims=True)
    theta = np.sqrt(q)
    zero = q == 0.0
    small = theta < _SERIES_THETA
    th = np.where(zero, 1.0, theta)
    a = np.where(zero, 1.0, np.sin(th) / th)
    b = np.where(zero, 0.5, 2.0 * np.sin(0.5 * th) ** 2 / (th * th))
    series = 1 / 6 + q * (-1 / 120 + q * (1 / 5040 + q * (-1 / 362880 + q * (1 / 39916800 - q / 6227020800))))
    c = np.where(small, series, (th - np.sin(th)) / (th * th * th))
    pp, pu = np.cross(phi, p), np.cross(phi, u)
    return p + a * pp + b * np.cross(phi, pp) + u + b * pu + c * np.cross(phi, pu)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def truth_point(p, s, s_ref, twist):
    """One point in mpmath from the doubles as given → list of three mpf."""
    mp = mpmath.mp
    with mp.workdps(50):
        tau = mpmath.mpf(float(s)) - mpmath.mpf(float(s_ref))
        w = [mpmath.mpf(float(x)) for x in twist[3:]]
        mag = abs(tau) * max(abs(x) for x in w)
    # theta - sin theta loses three times the digits of theta: carry them
    extra = 0 if mag == 0 else max(0, int(-3 * mpmath.log10(mag))) + 10
    with mp.workdps(50 + extra):
        tau = mpmath.mpf(float(s)) - mpmath.mpf(float(s_ref))
        v = [mpmath.mpf(float(x)) for x in twist[:3]]
        w = [mpmath.mpf(float(x)) for x in twist[3:]]
        p = [mpmath.mpf(float(x)) for x in p]
        phi = [tau * x for x in w]
        u = [tau * x for x in v]
        theta = mpmath.sqrt(sum(x * x for x in phi))
        if theta == 0:
            a, b, c = mpmath.mpf(1), mpmath.mpf(1) / 2, mpmath.mpf(1) / 6
        else:
            a = mpmath.sin(theta) / theta
            b = (1 - mpmath.cos(theta)) / theta ** 2
            c = (theta - mpmath.sin(theta)) / theta ** 3
        pp, pu = _cross(phi, p), _cross(phi, u)
        ppp, ppu = _cross(phi, pp), _cross(phi, pu)
        return [p[k] + a * pp[k] + b * ppp[k] + u[k] + b * pu[k] + c * ppu[k] for k in range(3)]


def truth(p, s, s_ref, twist):
    """→ list of n lists of three mpf."""
    return [truth_point(p[i], s[i], s_ref, twist) for i in range(len(p))]


def errors_eps(got, want, p, s, s_ref, twist):
    """→ [n] the error measure per point, in eps, of float64 rows `got` against mpmath rows `want`."""
    got = np.asarray(got, dtype=np.float64)
    vmax = float(np.max(np.abs(np.asarray(twist, dtype=np.float64)[:3])))
    out = np.zeros(len(want))
    with mpmath.mp.workdps(50):
        for i, row in enumerate(want):
            scale = float(np.max(np.abs(p[i]))) + abs(float(s[i]) - s_ref) * vmax
            worst = max(abs(mpmath.mpf(float(got[i, k])) - row[k]) for k in range(3))
            out[i] = float(worst / scale) / EPS
    return out


_CACHE = {}


def case(name, s_ref):
    """→ dict(p, s, twist, truth, restate, restate_eps) of one family at one s_ref, computed once per process."""
    key = (name, s_ref)
    if key not in _CACHE:
        p, s, twist = family(name)
        want = truth(p, s, s_ref, twist)
        re = restate(p, s, s_ref, twist)
        _CACHE[key] = {"p": p, "s": s, "twist": twist, "truth": want, "restate": re,
                       "restate_eps": float(np.max(errors_eps(re, want, p, s, s_ref, twist)))}
    return _CACHE[key]


# ------------------------------------------------------------------------------ SE(3) exponential in mpmath

def exp_se3(twist):
    """→ (R 3x3, t 3) as nested lists of mpf at 50 digits (more for tiny angles): the SE(3) exponential of a [6] twist."""
    mp = mpmath.mp
    wmax = max(abs(float(x)) for x in twist[3:])
    extra = 0 if wmax == 0 else max(0, int(-3 * np.log10(wmax))) + 10
    with mp.workdps(50 + extra):
        v = [mpmath.mpf(float(x)) for x in twist[:3]]
        w = [mpmath.mpf(float(x)) for x in twist[3:]]
        theta = mpmath.sqrt(sum(x * x for x in w))
        if theta == 0:
            a, b, c = mpmath.mpf(1), mpmath.mpf(1) / 2, mpmath.mpf(1) / 6
        else:
            a = mpmath.sin(theta) / theta
            b = (1 - mpmath.cos(theta)) / theta ** 2
            c = (theta - mpmath.sin(theta)) / theta ** 3
        W = [[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]
        W2 = [[sum(W[i][k] * W[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        R = [[(1 if i == j else 0) + a * W[i][j] + b * W2[i][j] for j in range(3)] for i in range(3)]
        t = [v[i] + sum((b * W[i][j] + c * W2[i][j]) * v[j] for j in range(3)) for i in range(3)]
        return R, t
