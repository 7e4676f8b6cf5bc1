"""Datasets whose every sum the kernels must compute EXACTLY — TEST INFRASTRUCTURE (tests/test_exact_sums_gpu.py).

NDT (6- and 3-DoF): R is a signed permutation (a rotation: det = +1), t, p and mu hold small integers and S is upper
triangular with small integer entries and a positive diagonal.  The factor U of S = QU the datasets store is then S itself
(every Givens rotation of sqrt_info_to_U meets a zero below the diagonal: cos = 1, sin = 0), and every e = R p + t − mu,
r = U e, J = [U | U M] (M = −R [p]x) and every entry of JᵀJ, Jᵀr and rᵀr is a small integer.  With no loss, or a Huber
threshold whose square lies above every s (w = 1, rho = s), each per-item term is an integer and so is every partial sum
— provided it stays below 2^24 in fp32 (the lanes sum in the storage type, assemble_pass.hpp) and below 2^53 in fp64.

Reprojection: fx = fy = 1, cx = cy = 0, integer X, Y and pixels, the depth z = (R X + t)_z a power of two Z0 above
min_depth (or, for one item in eight, 0 or −Z0: such an item must contribute nothing).  Then r = Rn / Z0, J = Jn / Z0², and
H, g, cost are integers over Z0⁴, Z0³, Z0²: exact as long as the numerators stay within the same budgets.  fast_inv
(assemble_items.hpp) has to return 1/Z0 exactly for that: the fp64 form refines the hardware reciprocal by two Newton
steps with fused multiply-adds, which lands on the exact power of two; fp32 divides.

The expected sums are computed here in numpy int64 from the reference's S-form statements (those of oracle_np.py and
oracle_xp.py: e = R p + t − mu, r = S e, J = [S | S M]).  Every item draws its own pseudo-random values (a generator per
chunk of GEN_CHUNK items, seeded with the chunk's index), so a dropped item and a duplicated one do not cancel.

The magnitude budget is asserted by the generators: the largest per-item |term| (every product of an entry summed in
absolute value) times the items a lane may hold must stay below 2^24 for fp32 — assuming no fewer than one wave per CU,
⌈n / (64 · CUs)⌉ items per lane, or the ≤ 4 items of one chunk, or what the solve form that runs at n gives a lane —
and Σ|term| over all items below 2^53.  The amplitude of the integers is chosen as large as the budget allows at the
given n, so that small datasets exercise more bits.
"""
import math
import os
import re

import numpy as np

GEN_CHUNK = 1 << 20
F32_LIMIT = 2 ** 24
F64_LIMIT = 2 ** 53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nonlinear_optimizer_for_slam_amd", "csrc")

TRI6 = [(r, c) for r in range(6) for c in range(r, 6)]
TRI3 = [(r, c) for r in range(3) for c in range(r, 3)]


# ---------------------------------------------------------------- the library's own constants

def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def library_constants():
    """The constants of the launch rules, read from the library's sources (not copied into the tests):
    single_block_max_elements (n × planes below which the single-workgroup solve runs), max_partial_rows (grid cap of the
    per-pass kernel), cluster_max_blocks, resident[(planes, element bytes)] = RI + LI items per lane, and the default
    per-pass launch table bpc[(element bytes, ITEMS, BLOCK, MINW, ping-pong)] = workgroups per CU, the workgroup size of
    the solve kernels (solve_block), the items per lane of one streamed chunk by element bytes (stream_items) and the
    workgroup size of the indexed kernel by element bytes (indexed_block)."""
    one = _read("assemble_one_launch.hpp")
    m = re.search(r"kSingleBlockMaxElements\s*=\s*size_t\((\d+)\)\s*\*\s*(\d+);", one)
    single = int(m.group(1)) * int(m.group(2))
    cmax = int(re.search(r"kClusterMaxBlocks\s*=\s*(\d+);", one).group(1))
    resident = {(int(a), int(b)): int(ri) + int(li) for a, b, ri, li in
                re.findall(r"struct ResidentShape<(\d+), (\d+)> \{ static constexpr int RI = (\d+), LI = (\d+); \};", one)}
    rows = int(re.search(r"kMaxPartialRows\s*=\s*(\d+);", _read("nos_internal.hpp")).group(1))
    core = _read("nos_core.hip")
    solve_block = int(re.search(r"int launch_single\(.*?constexpr int kBlock = (\d+);", core, re.S).group(1))
    si = re.search(r"constexpr int kSI = sizeof\(T\) == 8 \? (\d+) : (\d+);", core)
    ib = re.search(r"constexpr int kBlock = sizeof\(T\) == 8 \? (\d+) : (\d+);", _read("nos_indexed.hip"))
    body = core[core.index("int launch_by_variant("):core.index("#undef NOS_CASE")]
    f64_part, f32_part = body.split("} else {", 1)
    bpc = {}
    for es, part in ((8, f64_part), (4, f32_part)):
        for pp, _idx, items, block, minw, b in re.findall(r"NOS_CASE(_PP)?\((\d+),\s*(\d+),\s*(\d+),\s*([^,]+),\s*(\d+)\)",
                                                           part):
            for w in re.findall(r"\d+", minw):  # "kReproj ? 3 : 2": either
                key = (es, int(items), int(block), int(w), bool(pp))
                assert bpc.get(key, int(b)) == int(b), key  # the geometry names its workgroups per CU unambiguously
                bpc[key] = int(b)
    return dict(single_block_max_elements=single, max_partial_rows=rows, cluster_max_blocks=cmax, resident=resident,
                bpc=bpc, solve_block=solve_block, stream_items={8: int(si.group(1)), 4: int(si.group(2))},
                indexed_block={8: int(ib.group(1)), 4: int(ib.group(2))})


_ASSEMBLE = re.compile(r"assemble_kernel<nos::(\w+)<(\w+), (\d+)>, (\w+), (\d+), (\d+), (\d+), (true|false), (\w+)>")
_CLUSTER = re.compile(r"solve_cluster_kernel<nos::(\w+)<(\w+), (\d+)>, (\w+), (\d+), (\d+), (\d+), (\d+)")


def assemble_geometry(name):
    """Template arguments of a demangled assemble_kernel name → dict(problem, T, ITEMS, BLOCK, MINW, NT, PREFETCH)."""
    m = _ASSEMBLE.search(name)
    assert m, name
    pf = m.group(9)
    return dict(problem=m.group(1), T=m.group(4), ITEMS=int(m.group(5)), BLOCK=int(m.group(6)), MINW=int(m.group(7)),
                NT=m.group(8) == "true", PREFETCH=3 if pf in ("3", "true") else 0)


def cluster_geometry(name):
    """solve_cluster_kernel<Problem, T, BLOCK, RI, LI, SI, …> → dict(problem, T, BLOCK, RI, LI, SI)."""
    m = _CLUSTER.search(name)
    assert m, name
    return dict(problem=m.group(1), T=m.group(4), BLOCK=int(m.group(5)), RI=int(m.group(6)), LI=int(m.group(7)),
                SI=int(m.group(8)))


def pass_items_per_lane(n, geom, consts, cus):
    """Items the busiest lane of the per-pass assemble kernel sums (fp32: in the storage type): the grid rule of
    launch_variant — grid = min(chunks, bpc · CUs, kMaxPartialRows), chunks grid-strided — over the padded layout."""
    chunk = geom["BLOCK"] * geom["ITEMS"]
    es = 8 if geom["T"] == "double" else 4
    bpc = consts["bpc"][(es, geom["ITEMS"], geom["BLOCK"], geom["MINW"], geom["PREFETCH"] == 3)]
    chunks = max(1, -(-n // chunk))  # chunks holding real items (the pads beyond add zeros)
    grid = max(1, min(chunks, bpc * cus, consts["max_partial_rows"]))
    return min(-(-chunks // grid) * geom["ITEMS"], max(n, 1))


def solve_items_per_lane(n, planes, es, consts, cus):
    """(form, items the busiest lane sums in one pass) of nos_*_solve (lm_solve): the single workgroup up to
    kSingleBlockMaxElements plane-elements (chunk c of solve_block items is lane-strided: ⌈n / solve_block⌉ items per
    lane), then the one-launch cluster of min(kClusterMaxBlocks, CUs, ⌈n / solve_block⌉) workgroups — resident while
    ⌈n / (workgroups · solve_block)⌉ fits the shape's RI + LI, streamed beyond (chunks of solve_block · SI items,
    grid-strided)."""
    b = consts["solve_block"]
    if n * planes <= consts["single_block_max_elements"]:
        return "single", max(1, -(-n // b))
    blocks = min(consts["cluster_max_blocks"], cus, -(-n // b))
    per_lane = -(-n // (blocks * b))
    if per_lane <= consts["resident"][(planes, es)]:
        return "resident", per_lane
    si = consts["stream_items"][es]
    return "streamed", -(-(-(-n // (b * si))) // blocks) * si


ITEMS_MAX = 4  # the most items a lane takes from one chunk in any launch geometry (nos_core.hip, NOS_CASE)
_K = None


def lane_budget(n, cus, planes=15, dtype="f32"):
    """Items per lane the magnitude budget assumes: at least one wave per CU for the per-pass kernels (a whole chunk's items
    in one lane at the least), and what the solve form that runs at this n gives its lanes."""
    global _K
    _K = _K or library_constants()
    solve = solve_items_per_lane(n, planes, 8 if dtype == "f64" else 4, _K, cus)[1] if n else 1
    return max(1, -(-n // (64 * cus)), min(n, ITEMS_MAX), solve)


# ---------------------------------------------------------------- poses

def _even(perm):
    return sum(perm[i] > perm[j] for i in range(len(perm)) for j in range(i + 1, len(perm))) % 2 == 0


def signed_permutation(seed, dim=3):
    """A rotation that is a signed permutation matrix (integer entries, det = +1), not the identity.

    3-D: one of the twelve of the tetrahedral group (an even permutation, signs of product +1).  The device loop keeps the
    rotation as a quaternion (LmInit6: R → q → R, as the reference's pose does), and only these survive that round trip
    exactly — their quaternions hold 0, ±1/2 and ±1; a quarter turn's hold √2/2, and the first cost of a solve is then
    taken at a rotation a few ulps away from R (measured: single-workgroup reprojection solve, cost off by 2 ulps)."""
    rng = np.random.default_rng([seed, 7])
    while True:
        perm = rng.permutation(dim)
        R = np.zeros((dim, dim), dtype=np.int64)
        R[np.arange(dim), perm] = rng.choice([-1, 1], size=dim)
        if round(np.linalg.det(R)) == 1 and not np.array_equal(R, np.eye(dim)) and (dim != 3 or _even(perm)):
            return R


# ---------------------------------------------------------------- NDT

def _s_amplitude(L):
    return max(L, 2)  # the diagonal of S takes at least two values, also at the smallest amplitude


def _ndt_bound(L):
    """Largest per-item |term| with |p|, |mu|, |t| ≤ L and |S| ≤ Ls = _s_amplitude(L): |e| ≤ 3L, |r| ≤ 9 L Ls, |M| ≤ 2L,
    |S M| ≤ 6 L Ls: cost ≤ 3 (9 L Ls)² = 243 L² Ls² bounds every entry (H: ≤ 108 L² Ls², g: ≤ 162 L² Ls², 3-DoF less)."""
    return 243 * L ** 2 * _s_amplitude(L) ** 2


def choose_amplitude(n, dtype, cus, bound, cap=64, planes=15):
    """Largest integer amplitude whose worst-case terms keep the sums exact at n items in `dtype`."""
    best = 1
    for L in range(1, cap + 1):
        if dtype == "f32" and bound(L) * lane_budget(n, cus, planes, dtype) >= F32_LIMIT:
            break
        if bound(L) * max(n, 1) >= F64_LIMIT:
            break
        best = L
    return best


def _ndt_chunk(seed, c, m, L):
    rng = np.random.default_rng([seed, c])
    p = rng.integers(-L, L + 1, size=(3, m))
    mu = rng.integers(-L, L + 1, size=(3, m))
    Ls = _s_amplitude(L)
    S = np.zeros((3, 3, m), dtype=np.int64)
    for a in range(3):
        S[a, a] = rng.integers(1, Ls + 1, size=m)
        for b in range(a + 1, 3):
            S[a, b] = rng.integers(-Ls, Ls + 1, size=m)
    return p, mu, S


def _tri_sums(J, r, dim, tri):
    """Σ over the items of {upper(JᵀJ) | Jᵀr | rᵀr} in int64, and the largest per-item Σ|products| of each quantity."""
    Ja = [[np.abs(v) for v in row] for row in J]
    ra = [np.abs(v) for v in r]
    rows = len(J)
    out, mx, tot = [], [], []
    for i, j in tri:
        out.append(int(sum(J[k][i] * J[k][j] for k in range(rows)).sum()))
        a = sum(Ja[k][i] * Ja[k][j] for k in range(rows))
        mx.append(int(a.max(initial=0)))
        tot.append(int(a.sum()))
    for i in range(dim):
        out.append(int(sum(J[k][i] * r[k] for k in range(rows)).sum()))
        a = sum(Ja[k][i] * ra[k] for k in range(rows))
        mx.append(int(a.max(initial=0)))
        tot.append(int(a.sum()))
    s = sum(r[k] * r[k] for k in range(rows))
    out.append(int(s.sum()))
    mx.append(int(s.max(initial=0)))
    tot.append(int(s.sum()))
    return out, mx, tot, int(s.max(initial=0))


def _abs_J(S, M):
    """|J| bound entries: the products of J = [S | S M] summed in absolute value (what an fma chain can hold)."""
    SMa = [[sum(np.abs(S[a][j]) * np.abs(M[j][b]) for j in range(3)) for b in range(3)] for a in range(3)]
    return SMa


def ndt6_int_sums(p, mu, S, R, t):
    """The S form of the reference in int64: e = R p + t − mu, r = S e, M = −R [p]x, J = [S | S M]."""
    e = [R[i, 0] * p[0] + R[i, 1] * p[1] + R[i, 2] * p[2] + t[i] - mu[i] for i in range(3)]
    r = [S[a][0] * e[0] + S[a][1] * e[1] + S[a][2] * e[2] for a in range(3)]
    M = [[R[i, 2] * p[1] - R[i, 1] * p[2], R[i, 0] * p[2] - R[i, 2] * p[0], R[i, 1] * p[0] - R[i, 0] * p[1]]
         for i in range(3)]
    SM = [[S[a][0] * M[0][b] + S[a][1] * M[1][b] + S[a][2] * M[2][b] for b in range(3)] for a in range(3)]
    J = [[S[a][0], S[a][1], S[a][2], SM[a][0], SM[a][1], SM[a][2]] for a in range(3)]
    out, mx, tot, smax = _tri_sums(J, r, 6, TRI6)
    # the |S M| entries themselves (inside the chain that forms C = U M) stay below the term bound: |C| ≤ Σ|S||M|
    mx.append(max((int(v.max(initial=0)) for row in _abs_J(S, M) for v in row), default=0))
    return out, mx, tot, smax


def ndt3_int_sums(p, mu, S, R2, t2):
    e = [R2[i, 0] * p[0] + R2[i, 1] * p[1] + t2[i] - mu[i] for i in range(2)] + [p[2] - mu[2]]
    r = [S[a][0] * e[0] + S[a][1] * e[1] + S[a][2] * e[2] for a in range(3)]
    d = [R2[0, 1] * p[0] - R2[0, 0] * p[1], R2[1, 1] * p[0] - R2[1, 0] * p[1]]
    J = [[S[a][0], S[a][1], S[a][0] * d[0] + S[a][1] * d[1]] for a in range(3)]
    return _tri_sums(J, r, 3, TRI3)


class ExactCase:
    """planes [15 | 5, n] float64; want6 / want3 / want: the exact sums as float64 (every one an exact integer, or an
    integer over a power of two); huber: a loss whose threshold² lies above every s of the dataset (w = 1)."""


def _check_budget(case, n, dtype, cus, mx, tot, planes=15):
    worst = max(mx)
    case.max_term = worst
    case.lane_budget = lane_budget(n, cus, planes, dtype)
    if dtype == "f32":
        assert worst * case.lane_budget < F32_LIMIT, (worst, case.lane_budget)
    assert max(tot, default=0) < F64_LIMIT and worst < F64_LIMIT, (max(tot), worst)


def ndt_case(n, dtype, cus=256, seed=1, three=True, amplitude=None):
    """n NDT correspondences with exact integer sums for the 6-DoF pose (R, t) and, with three=True, the planar pose
    (R2, t2)."""
    case = ExactCase()
    L = amplitude or choose_amplitude(n, dtype, cus, _ndt_bound)
    case.amplitude = L
    R = signed_permutation(seed)
    R2 = signed_permutation(seed + 1, 2)
    rng = np.random.default_rng([seed, 3])
    t = rng.integers(-L, L + 1, size=3)
    t2 = rng.integers(-L, L + 1, size=2)
    planes = np.zeros((15, n))
    s6 = np.zeros(28, dtype=object)
    s3 = np.zeros(10, dtype=object)
    mx6, tot6 = [0] * 29, [0] * 28
    mx3, tot3 = [0] * 10, [0] * 10
    smax = 0
    for c, lo in enumerate(range(0, n, GEN_CHUNK)):
        m = min(GEN_CHUNK, n - lo)
        p, mu, S = _ndt_chunk(seed, c, m, L)
        planes[0:3, lo:lo + m] = p
        planes[3:6, lo:lo + m] = mu
        planes[6:15, lo:lo + m] = S.reshape(9, m)
        out, mx, tot, sm = ndt6_int_sums(p, mu, S, R, t)
        s6 += np.array(out, dtype=object)
        mx6 = [max(a, b) for a, b in zip(mx6, mx)]
        tot6 = [a + b for a, b in zip(tot6, tot)]
        smax = max(smax, sm)
        if three:
            out, mx, tot, sm = ndt3_int_sums(p, mu, S, R2, t2)
            s3 += np.array(out, dtype=object)
            mx3 = [max(a, b) for a, b in zip(mx3, mx)]
            tot3 = [a + b for a, b in zip(tot3, tot)]
            smax = max(smax, sm)
    _check_budget(case, n, dtype, cus, mx6 + mx3, tot6 + tot3)
    case.planes, case.R, case.t, case.R2, case.t2 = planes, R.astype(np.float64), t.astype(np.float64), \
        R2.astype(np.float64), t2.astype(np.float64)
    case.want6 = _as_f64(s6)
    case.want3 = _as_f64(s3) if three else None
    th = math.isqrt(smax) + 1  # th² > every s: every item is a Huber inlier (w = 1, rho = s)
    assert th * th > smax and (dtype == "f64" or th * th < F32_LIMIT)
    case.huber = ("huber", float(th))
    return case


def ndt_sums_of_planes(planes, R, t, R2, t2, dtype, cus=256):
    """Exact sums of any NDT planes holding integers and an upper-triangular S (e.g. the (point, voxel) pairs of an
    indexed dataset) → (want6, want3); the budget is asserted as for ndt_case."""
    n = planes.shape[1]
    s6, s3 = np.zeros(28, dtype=object), np.zeros(10, dtype=object)
    mx_all, tot_all = [0] * 39, [0] * 38
    Ri, ti, R2i, t2i = (np.asarray(v).astype(np.int64) for v in (R, t, R2, t2))
    for lo in range(0, n, GEN_CHUNK):
        q = planes[:, lo:lo + GEN_CHUNK]
        qi = q.astype(np.int64)
        assert np.array_equal(qi, q) and not np.any(qi[[9, 12, 13]]), "integer planes with an upper-triangular S"
        p, mu, S = qi[0:3], qi[3:6], qi[6:15].reshape(3, 3, -1)
        o6, m6, t6, _ = ndt6_int_sums(p, mu, S, Ri, ti)
        o3, m3, t3, _ = ndt3_int_sums(p, mu, S, R2i, t2i)
        s6 += np.array(o6, dtype=object)
        s3 += np.array(o3, dtype=object)
        mx_all = [max(a, b) for a, b in zip(mx_all, m6 + m3)]
        tot_all = [a + b for a, b in zip(tot_all, t6 + t3)]
    _check_budget(ExactCase(), n, dtype, cus, mx_all, tot_all)
    return _as_f64(s6), _as_f64(s3)


def _as_f64(ints, denominators=None):
    out = np.zeros(len(ints))
    for k, v in enumerate(ints):
        v = int(v)
        assert abs(v) < F64_LIMIT, v
        out[k] = float(v) if denominators is None else float(v) / float(denominators[k])  # a power of two: exact
    return out


# ---------------------------------------------------------------- reprojection

REPROJ_INTR = (1.0, 1.0, 0.0, 0.0)  # inv_fx, inv_fy, cx, cy
REPROJ_MIN_DEPTH = 0.5


def _reproj_bound(L, Z0):
    """|X| ≤ 2L (Xw, t ≤ L), |M| ≤ 2 · 2L, |Jn| ≤ Z0·4L + L·4L, |Rn| ≤ L + L·Z0: the largest per-item |term| numerator."""
    j = max(Z0, L, Z0 * 4 * L + 4 * L * L)
    rr = L + L * Z0
    return 2 * max(j * j, j * rr, rr * rr)


def reproj_int_sums(Xw, pix, X, R, Z0, ok):
    """Numerators of the reference's reprojection sums (REM/..._analytic.cc:107-162 with fx = fy = 1, cx = cy = 0, z = Z0):
    Rn = Z0 · r, Jn = Z0² · J — r = Xw/z − pixel, J = [dK | dK M], dK = [[1/z, 0, −x/z²], [0, 1/z, −y/z²]], M = −R [X]x;
    items with z < min_depth (ok == False) contribute nothing."""
    zero = np.zeros_like(Xw[0])
    okz = ok.astype(np.int64)
    M = [[R[i, 2] * X[1] - R[i, 1] * X[2], R[i, 0] * X[2] - R[i, 2] * X[0], R[i, 1] * X[0] - R[i, 0] * X[1]]
         for i in range(3)]
    Rn = [(Xw[0] - pix[0] * Z0) * okz, (Xw[1] - pix[1] * Z0) * okz]
    J = [[zero + Z0, zero, -Xw[0]] + [Z0 * M[0][b] - Xw[0] * M[2][b] for b in range(3)],
         [zero, zero + Z0, -Xw[1]] + [Z0 * M[1][b] - Xw[1] * M[2][b] for b in range(3)]]
    J = [[v * okz for v in row] for row in J]
    return _tri_sums(J, Rn, 6, TRI6)


def reproj_case(n, dtype, cus=256, seed=1, Z0=4, amplitude=None):
    """n reprojection correspondences with exact sums at (R, t), intrinsics REPROJ_INTR and min_depth REPROJ_MIN_DEPTH;
    one item in eight lies at depth 0 or −Z0 and must not count."""
    assert Z0 > REPROJ_MIN_DEPTH and Z0 & (Z0 - 1) == 0
    case = ExactCase()
    L = amplitude or choose_amplitude(n, dtype, cus, lambda a: _reproj_bound(a, Z0), planes=5)
    case.amplitude = L
    R = signed_permutation(seed)
    t = np.random.default_rng([seed, 3]).integers(-L, L + 1, size=3)
    planes = np.zeros((5, n))
    sums = np.zeros(28, dtype=object)
    mx_all, tot_all = [0] * 28, [0] * 28
    smax = 0
    for c, lo in enumerate(range(0, n, GEN_CHUNK)):
        m = min(GEN_CHUNK, n - lo)
        rng = np.random.default_rng([seed, c])
        Xw = rng.integers(-L, L + 1, size=(3, m))
        kind = rng.integers(0, 16, size=m)
        Xw[2] = np.where(kind == 0, 0, np.where(kind == 1, -Z0, Z0))
        ok = Xw[2] >= REPROJ_MIN_DEPTH
        X = R.T @ (Xw - t[:, None])  # R X + t = Xw exactly
        pix = rng.integers(-L, L + 1, size=(2, m))
        planes[0:3, lo:lo + m] = X
        planes[3:5, lo:lo + m] = pix
        out, mx, tot, sm = reproj_int_sums(Xw, pix, X, R, Z0, ok)
        sums += np.array(out, dtype=object)
        mx_all = [max(a, b) for a, b in zip(mx_all, mx)]
        tot_all = [a + b for a, b in zip(tot_all, tot)]
        smax = max(smax, sm)
    _check_budget(case, n, dtype, cus, mx_all, tot_all, planes=5)
    den = [Z0 ** 4] * 21 + [Z0 ** 3] * 6 + [Z0 ** 2]
    case.planes, case.R, case.t = planes, R.astype(np.float64), t.astype(np.float64)
    case.want = _as_f64(sums, den)
    th = math.isqrt(smax) + 1  # in units of 1/Z0: th / Z0 is exact and its square lies above every s
    case.huber = ("huber", th / Z0)
    assert (dtype == "f64" or th * th < F32_LIMIT)
    case.Z0 = Z0
    return case
