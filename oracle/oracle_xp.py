"""Extended-precision restatement of the assembly math — TEST INFRASTRUCTURE.

The same sums as oracle_np.py ({upper(H) | g | cost}, same plane order), written from the same reference formulas in the
S form (r = S e, s = rᵀr, J = [S | S M]), but every per-item term and every sum is carried in np.longdouble (x87 80-bit,
u = 2^-64 ≈ 5.4e-20 — eleven more bits than fp64).  The fp64 C oracle works at the precision of the kernels; this one
measures how far a kernel, and a plain evaluation in the kernel's own precision, are from the exact sums.

Inputs are taken as given (float64 arrays; pass fp32-rounded values to measure an fp32 kernel's arithmetic and not the
rounding of its inputs).  Reference lines: MDM/..._analytic.cc:159-185 (6-DoF), MDM/..._analytic_3dof.cc:110-139 (3-DoF),
REM/..._analytic.cc:107-162 (reprojection), NO/loss_function.h:28-33,57-66 (losses).
"""
import numpy as np

LD = np.longdouble
if not np.finfo(LD).eps <= 1.2e-19:  # 2^-63 = 1.08e-19 for the x87 extended format
    raise RuntimeError("oracle_xp needs an 80-bit np.longdouble (eps %.3g); this platform's is not" % np.finfo(LD).eps)

TRI6 = [(r, c) for r in range(6) for c in range(r, 6)]
TRI3 = [(r, c) for r in range(3) for c in range(r, 3)]


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def loss_eval(loss, s):
    """(rho, w) per item, in the precision of s."""
    one = s.dtype.type(1)
    if loss is None or loss[0] == "none":
        return s.copy(), np.ones_like(s)
    if loss[0] == "exponential":
        c1, c2 = s.dtype.type(loss[1]), s.dtype.type(loss[2])
        ex = np.exp(-c2 * s)
        return c1 - c1 * ex, 2 * c1 * c2 * ex
    if loss[0] == "huber":
        th = s.dtype.type(loss[1])
        out = s > th * th
        rr = np.sqrt(np.where(out, s, one))
        return np.where(out, 2 * th * rr - th * th, s), np.where(out, th / rr, one)
    raise ValueError(loss)


def _pack(H, g, cost, tri):
    return np.array([H[r][c] for r, c in tri] + list(g) + [cost], dtype=LD)


def _matvec(S, e):
    """S [3][3][n] (lists of arrays), e [3][n] → [3][n]"""
    return [S[a][0] * e[0] + S[a][1] * e[1] + S[a][2] * e[2] for a in range(3)]


def _matvec_exact(S64, e_parts):
    """r = S e, S [3][3] of fp64 arrays, e as exact_affine parts: the rows of a planar S cancel to 1/κ of their terms
    when e lies in the plane, so r too is summed by exact_affine."""
    return [exact_affine([S64[a][j] for j in range(3) for _ in range(3)], [q for j in range(3) for q in e_parts[j]], ())
            for a in range(3)]


def _sums(w, J, r, rho, dim):
    """H = Σ w JᵀJ, g = Σ w Jᵀr, cost = Σ rho; J [rows][dim][n], r [rows][n]; longdouble sums of longdouble terms."""
    rows = len(J)
    H = [[None] * dim for _ in range(dim)]
    for i in range(dim):
        for j in range(i, dim):
            H[i][j] = np.sum(w * sum(J[k][i] * J[k][j] for k in range(rows)), dtype=r[0].dtype)
    g = [np.sum(w * sum(J[k][i] * r[k] for k in range(rows)), dtype=r[0].dtype) for i in range(dim)]
    return H, g, np.sum(rho, dtype=r[0].dtype)


def _split(a):
    """Veltkamp: a = hi + lo with 26-bit hi, so that products of halves are exact in fp64."""
    c = a * 134217729.0  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def exact_affine(coeffs, xs, addends, parts=False):
    """Σ c_k x_k + Σ addends for fp64 arrays, as a longdouble with about twice the longdouble precision before the final
    rounding: every product is split into four exact fp64 partial products (Veltkamp), the terms are summed by Sum2
    (Ogita, Rump & Oishi 2005) in longdouble.  e = R p + t - mu at |p| = 1e5 then keeps all its digits.  parts=True:
    three fp64 arrays whose sum is that value before its final rounding (input to a second exact_affine: r = S e)."""
    terms = []
    for c, x in zip(coeffs, xs):
        c = np.broadcast_to(np.asarray(c, dtype=np.float64), np.shape(x))
        ch, cl = _split(c)
        xh, xl = _split(np.asarray(x, dtype=np.float64))
        terms += [ch * xh, ch * xl, cl * xh, cl * xl]
    terms += [np.broadcast_to(np.asarray(a, dtype=np.float64), np.shape(xs[0])) for a in addends]
    s = terms[0].astype(LD)
    comp = np.zeros_like(s)
    for tm in terms[1:]:
        s, err = _two_sum(s, tm.astype(LD))
        comp = comp + err
    if not parts:
        return s + comp
    s, comp = _two_sum(s, comp)
    hi = s.astype(np.float64)
    return [hi, (s - hi).astype(np.float64), comp.astype(np.float64)]


def fma(a, b, c):
    """a·b + c rounded once to the dtype of a (fp64: through longdouble; fp32: through fp64, where a·b is exact)."""
    w = LD if np.asarray(a).dtype == np.float64 else np.float64
    return (np.asarray(a).astype(w) * np.asarray(b).astype(w) + np.asarray(c).astype(w)).astype(np.asarray(a).dtype)


def _affine(R_row, x, t, mu, order):
    """e = R_row · x + t − mu in the working dtype; order "ref": R p first, then t (the reference, Eigen); "fma": t innermost
    in a chain of fused multiply-adds (the kernels)."""
    if order == "fma":
        acc = np.full_like(x[0], t)
        for k in reversed(range(len(x))):
            acc = fma(np.full_like(x[0], R_row[k]), x[k], acc)
        return acc - mu
    acc = R_row[0] * x[0]
    for k in range(1, len(x)):
        acc = acc + R_row[k] * x[k]
    return acc + t - mu


def _cast(planes, dtype):
    return [np.asarray(planes[k], dtype=np.float64).astype(dtype) for k in range(planes.shape[0])]


def ndt6_items(planes, R, t, dtype=LD, order="ref"):
    """Per-item r (3 × n) and J (3 × 6 × n) of the S form, every operation in `dtype` (longdouble: e = R p + t - mu
    through exact_affine)."""
    planes = np.asarray(planes, dtype=np.float64)
    R64, t64 = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64)
    x = _cast(planes, dtype)
    R = np.asarray(R, dtype=np.float64).reshape(3, 3).astype(dtype)
    t = np.asarray(t, dtype=np.float64).astype(dtype)
    p, mu = x[0:3], x[3:6]
    S = [[x[6 + 3 * a + b] for b in range(3)] for a in range(3)]
    if dtype == LD:
        e = [exact_affine(R64[i], planes[0:3], (t64[i], -planes[3 + i]), parts=True) for i in range(3)]
        r = _matvec_exact([[planes[6 + 3 * a + b] for b in range(3)] for a in range(3)], e)
    else:
        e = [_affine(R[i], p, t[i], mu[i], order) for i in range(3)]
        r = _matvec(S, e)
    # M = -R [p]x: column b of [p]x is e_b × p … written out: M[i][0] = R[i,2] p1 - R[i,1] p2, etc.
    M = [[R[i, 2] * p[1] - R[i, 1] * p[2], R[i, 0] * p[2] - R[i, 2] * p[0], R[i, 1] * p[0] - R[i, 0] * p[1]]
         for i in range(3)]
    SM = [[S[a][0] * M[0][b] + S[a][1] * M[1][b] + S[a][2] * M[2][b] for b in range(3)] for a in range(3)]
    J = [[S[a][0], S[a][1], S[a][2], SM[a][0], SM[a][1], SM[a][2]] for a in range(3)]
    return r, J


def _terms(w, J, r, rho, dim):
    """Per-item terms of {upper(H) | g | cost}: an [n_out, n] array in the precision of r (their sums are _sums')."""
    rows = len(J)
    out = [w * sum(J[k][i] * J[k][j] for k in range(rows)) for i, j in (TRI6 if dim == 6 else TRI3)]
    out += [w * sum(J[k][i] * r[k] for k in range(rows)) for i in range(dim)]
    return np.array(out + [rho])


def ndt6_accumulate(planes, R, t, loss=None, dtype=LD, order="ref", terms=False):
    """terms=True: the per-item terms ([28, n]) instead of their sums."""
    r, J = ndt6_items(planes, R, t, dtype, order)
    s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    rho, w = loss_eval(loss, s)
    if terms:
        return _terms(w, J, r, rho, 6)
    H, g, cost = _sums(w, J, r, rho, 6)
    return _pack(H, g, cost, TRI6)


def ndt3_items(planes, R2, t2, dtype=LD, order="ref"):
    planes = np.asarray(planes, dtype=np.float64)
    R64, t64 = np.asarray(R2, dtype=np.float64).reshape(2, 2), np.asarray(t2, dtype=np.float64)
    x = _cast(planes, dtype)
    R2 = np.asarray(R2, dtype=np.float64).reshape(2, 2).astype(dtype)
    t2 = np.asarray(t2, dtype=np.float64).astype(dtype)
    p, mu = x[0:3], x[3:6]
    S = [[x[6 + 3 * a + b] for b in range(3)] for a in range(3)]
    if dtype == LD:
        e = [exact_affine(R64[i], planes[0:2], (t64[i], -planes[3 + i]), parts=True) for i in range(2)]
        e.append(exact_affine([1.0], [planes[2]], (-planes[5],), parts=True))
        r = _matvec_exact([[planes[6 + 3 * a + b] for b in range(3)] for a in range(3)], e)
    else:
        e = [_affine(R2[i], p[0:2], t2[i], mu[i], order) for i in range(2)] + [p[2] - mu[2]]
        r = _matvec(S, e)
    d = [R2[0, 1] * p[0] - R2[0, 0] * p[1], R2[1, 1] * p[0] - R2[1, 0] * p[1]]
    J = [[S[a][0], S[a][1], S[a][0] * d[0] + S[a][1] * d[1]] for a in range(3)]
    return r, J


def ndt3_accumulate(planes, R2, t2, loss=None, dtype=LD, order="ref", terms=False):
    r, J = ndt3_items(planes, R2, t2, dtype, order)
    s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    rho, w = loss_eval(loss, s)
    if terms:
        return _terms(w, J, r, rho, 3)
    H, g, cost = _sums(w, J, r, rho, 3)
    return _pack(H, g, cost, TRI3)


def reproj_accumulate(planes, R, t, intr, loss=None, min_depth=0.03, dtype=LD, terms=False):
    """The scalar class's rule: a correspondence with depth z < min_depth contributes nothing."""
    planes = np.asarray(planes, dtype=np.float64)
    R64, t64 = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64)
    x = _cast(planes, dtype)
    R = R64.astype(dtype)
    t = t64.astype(dtype)
    inv_fx, inv_fy, cx, cy = [np.asarray(v, dtype=np.float64).astype(dtype) for v in intr]
    X, px = x[0:3], x[3:5]
    if dtype == LD:
        Xw = [exact_affine(R64[i], planes[0:3], (t64[i],)) for i in range(3)]
    else:
        Xw = [R[i, 0] * X[0] + R[i, 1] * X[1] + R[i, 2] * X[2] + t[i] for i in range(3)]
    ok = ~(Xw[2] < np.asarray(min_depth, dtype=np.float64).astype(dtype))
    one = np.ones_like(Xw[2])
    iz = one / np.where(ok, Xw[2], one)
    r = [Xw[0] * iz - inv_fx * (px[0] - cx), Xw[1] * iz - inv_fy * (px[1] - cy)]
    zero = np.zeros_like(iz)
    dK = [[iz, zero, -Xw[0] * iz * iz], [zero, iz, -Xw[1] * iz * iz]]
    M = [[R[i, 2] * X[1] - R[i, 1] * X[2], R[i, 0] * X[2] - R[i, 2] * X[0], R[i, 1] * X[0] - R[i, 0] * X[1]]
         for i in range(3)]
    J = [[dK[a][0], dK[a][1], dK[a][2]] + [dK[a][0] * M[0][b] + dK[a][1] * M[1][b] + dK[a][2] * M[2][b] for b in range(3)]
         for a in range(2)]
    r = [np.where(ok, v, zero) for v in r]
    J = [[np.where(ok, v, zero) for v in row] for row in J]
    s = r[0] * r[0] + r[1] * r[1]
    rho, w = loss_eval(loss, s)
    if terms:
        return _terms(w, J, r, rho, 6)
    H, g, cost = _sums(w, J, r, rho, 6)
    return _pack(H, g, cost, TRI6)


def period_sums(terms, prefixes=()):
    """Sums of a period's per-item terms (the `terms=True` output of an *_accumulate, in longdouble), for references of
    datasets that tile that period: → (S_P, {r: S_r}, A_P, {r: A_r}) — the period's sums, the sums of its first r items,
    and Σ|term| of both, per quantity."""
    terms = np.asarray(terms, dtype=LD)
    mag = np.abs(terms)
    return (terms.sum(axis=1), {r: terms[:, :r].sum(axis=1) for r in prefixes},
            mag.sum(axis=1), {r: mag[:, :r].sum(axis=1) for r in prefixes})


def tiled_sums(terms, n):
    """Reference sums of the first n items of the period `terms` ([n_out, P]) repeated: n = K·P + r → K·S_P + S_r, and
    Σ|term| likewise (longdouble).  Costs one pass over the period, whatever n is."""
    P = np.asarray(terms).shape[1]
    K, r = divmod(int(n), P)
    SP, Sr, AP, Ar = period_sums(terms, (r,))
    return LD(K) * SP + Sr[r], LD(K) * AP + Ar[r]


def unpack(out, dim):
    """{upper(H) | g | cost} → (H full symmetric, g, cost), in the precision of `out`."""
    tri = TRI6 if dim == 6 else TRI3
    out = np.asarray(out)
    H = np.zeros((dim, dim), dtype=out.dtype)
    for k, (r, c) in enumerate(tri):
        H[r, c] = H[c, r] = out[k]
    return H, out[len(tri):len(tri) + dim].copy(), out[len(tri) + dim]


def scaled_errors_ld(got, want, dim):
    """(H, g, cost) errors of `got` against `want` (both longdouble): H entries against the Cauchy-Schwarz scale
    sqrt(H_ii H_jj), g against sqrt(H_ii · cost), the cost relatively."""
    Hg, gg, cg = unpack(np.asarray(got, dtype=LD), dim)
    Hw, gw, cw = unpack(np.asarray(want, dtype=LD), dim)
    d = np.sqrt(np.maximum(np.diag(Hw), LD(0)))
    tiny = LD(1e-300)
    eH = np.max(np.abs(Hg - Hw) / (np.outer(d, d) + tiny))
    eg = np.max(np.abs(gg - gw) / (d * np.sqrt(max(abs(cw), tiny)) + tiny))
    ec = abs(cg - cw) / max(abs(cw), tiny)
    return float(eH), float(eg), float(ec)


def scaled_errors(got, want, dim):
    """scaled_errors_ld of a float64 result (a kernel's, or a plain evaluation's) against the extended reference."""
    return scaled_errors_ld(np.asarray(got, dtype=np.float64).astype(LD), want, dim)
