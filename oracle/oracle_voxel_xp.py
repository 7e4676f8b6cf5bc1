"""Extended-precision reference of ONE NDT voxel's statistics — TEST INFRASTRUCTURE, next to oracle_xp.py.

The map build and the voxel store finish every voxel with the same small piece of arithmetic (csrc/voxel_finish.hpp):
mean, cov = (Σ d dᵀ + I) / n − m mᵀ, a symmetric 3×3 eigen-decomposition, the validity rules, eigenvalue flooring and
the sqrt-information.  voxel_stats_xp evaluates it in mpmath at 50 digits from the points of the voxel, with nothing
of the kernels' arithmetic in it: no Jacobi sweep, no tie rule, no sign convention.

What it returns for comparison is the INFORMATION MATRIX  Σ_k u_k u_kᵀ / λ_k(floored): a Lipschitz spectral function
of cov, independent of eigenvector signs and of the basis of a tied eigenspace, equal to SᵀS under
NOS_MAP_PROPER_SQRT_INFORMATION.  Under the harness formula S = D^-1/2 V the same matrix is V D^-1 Vᵀ with
D = 1 / diag(S Sᵀ) and V = D^1/2 S (information_from_sqrt below).
"""
import mpmath
import numpy as np

DPS = 50
MIN_POINTS = 5
# the kernels compare and floor with the fp64 constants 0.01: so does the reference
MIN_EIGENVALUE = 0.01
EIG_FLOOR = 0.01
TIE_RULE = 1e-9  # symmetric_eigen3 picks the basis of a pair of eigenvalues whose gap is at most this × the largest


def _to_ld(x):
    """mpf → longdouble (hi + lo: 64 of the 166 bits)"""
    hi = float(x)
    return np.longdouble(hi) + np.longdouble(float(x - mpmath.mpf(hi)))


def voxel_stats_xp(points, cell, resolution):
    """points [n,3] float64, all in the cell `cell` (3 integers) of a grid of edge `resolution` → dict:
      n, valid, mean [3] longdouble, eig [3] and eig_floored [3] (ascending, float64 of the 50-digit values),
      info [3,3] float64 (the information matrix; identity when invalid), gaps (rel. gap λ1−λ0, λ2−λ1 over λ2).
    The corner cell·resolution is subtracted first — exactly, whatever it is, at this precision — and added back to
    the mean; the sums are exact (mpmath.fdot rounds once, at 50 digits, which holds them entirely)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    out = {"n": n, "valid": False, "mean": np.zeros(3, dtype=np.longdouble), "eig": np.zeros(3), "eig_floored": np.zeros(3),
           "info": np.eye(3), "gaps": (np.inf, np.inf)}
    with mpmath.workdps(DPS):
        res = mpmath.mpf(float(resolution))
        corner = [mpmath.mpf(int(c)) * res for c in cell]
        d = [[mpmath.mpf(float(pts[i, k])) - corner[k] for i in range(n)] for k in range(3)]
        if n == 0:
            return out
        m = [mpmath.fsum(d[k]) / n for k in range(3)]
        out["mean"] = np.array([_to_ld(corner[k] + m[k]) for k in range(3)], dtype=np.longdouble)
        cov = mpmath.matrix(3, 3)
        for a in range(3):
            for b in range(a, 3):
                cov[a, b] = cov[b, a] = (mpmath.fdot(d[a], d[b]) + (1 if a == b else 0)) / n - m[a] * m[b]
        w, U = mpmath.eigsy(cov)  # ascending; eigenvectors in the columns of U
        w = [w[k] for k in range(3)]
        out["eig"] = np.array([float(x) for x in w])
        out["gaps"] = (float((w[1] - w[0]) / w[2]), float((w[2] - w[1]) / w[2]))
        if n < MIN_POINTS or w[2] < mpmath.mpf(MIN_EIGENVALUE):
            return out
        floor = w[2] * mpmath.mpf(EIG_FLOOR)
        wf = [max(w[0], floor), max(w[1], floor), w[2]]
        info = mpmath.matrix(3, 3)
        for k in range(3):
            for a in range(3):
                for b in range(3):
                    info[a, b] += U[a, k] * U[b, k] / wf[k]
        out["valid"] = True
        out["eig_floored"] = np.array([float(x) for x in wf])
        out["info"] = np.array([[float(info[a, b]) for b in range(3)] for a in range(3)])
    return out


def merged_gap(stats):
    """The g of the information-matrix bound: the true relative gap of the eigenvalue pairs the tie rule merges (inside
    that rule the code picks the basis by construction, and its matrix is off by the gap), 0 otherwise.  Pairs that are
    both floored are equal afterwards and cost nothing."""
    w, wf = stats["eig"], stats["eig_floored"]
    g = 0.0
    for k, gap in enumerate(stats["gaps"]):
        if gap <= TIE_RULE * (1.0 + 1e-3) and not (wf[k] == wf[k + 1]):  # 1e-3: the code sees the gap to its own rounding
            g += gap
    return g


def voxel_stats_ld(points, cell, resolution):
    """The same statistics in longdouble sums and a float64 eigh: an independent evaluation that ties the 50-digit one
    to ordinary arithmetic → (mean [3], eig_floored [3], info [3,3], valid)."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    corner = np.array([np.longdouble(int(c)) * np.longdouble(float(resolution)) for c in cell], dtype=np.longdouble)
    d = pts.astype(np.longdouble) - corner
    m = d.sum(axis=0) / n
    cov = ((d[:, :, None] * d[:, None, :]).sum(axis=0) + np.eye(3)) / n - np.outer(m, m)
    w, U = np.linalg.eigh(cov.astype(np.float64))
    if n < MIN_POINTS or w[2] < MIN_EIGENVALUE:
        return np.zeros(3), np.zeros(3), np.eye(3), False
    wf = np.array([max(w[0], EIG_FLOOR * w[2]), max(w[1], EIG_FLOOR * w[2]), w[2]])
    return (corner + m), wf, (U / wf) @ U.T, True


def information_from_sqrt(S, proper):
    """sqrt-information S [3,3] as the library returns it → (information matrix, floored eigenvalues 1 / diag(S Sᵀ),
    ‖V Vᵀ − I‖_F of the recovered eigenvector matrix).  proper: S = D^-1/2 Vᵀ, the information is SᵀS;
    harness formula: S = D^-1/2 V, so V = D^1/2 S and the information is V D^-1 Vᵀ."""
    S = np.asarray(S, dtype=np.float64).reshape(3, 3)
    lam = 1.0 / np.einsum("ij,ij->i", S, S)
    V = np.sqrt(lam)[:, None] * S  # proper: Vᵀ
    ortho = float(np.linalg.norm(V @ V.T - np.eye(3)))
    if proper:
        return S.T @ S, lam, ortho
    return (V / lam) @ V.T, lam, ortho
