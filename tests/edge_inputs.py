"""Input families at the edges of the NDT and reprojection sums (numpy generators shared by test_xprec_oracle.py and
test_xprec_gpu.py).

NDT sqrt-informations are built as the reference builds them, S = D^-1/2 Vᵀ of a covariance V D Vᵀ (not symmetric), with a
chosen condition number κ(S):
  planar voxel: one large singular value of S (the plane's normal), linear voxel: two;
  e = R p + t - mu either in the low-information directions (a point on the plane / line) or isotropic;
  rank-deficient S: one singular value exactly 0 (and a random rotation on the left), e in its null space (exact s = 0).
Offsets put the map frame (p and mu) or the pose (t and mu) at 0, 1e3 or 1e5 m with the same small e of 1e-2 … 1e-1 m.
"""
import numpy as np

from tests import helpers

R_TEST = helpers.rot_xyz(0.01, -0.02, 0.05)
T_TEST = np.array([-0.1, 0.05, 0.2])
C2, S2 = np.cos(0.07), np.sin(0.07)
R2_TEST = np.array([[C2, -S2], [S2, C2]])
T2_TEST = np.array([-0.15, 0.1])

KAPPAS = (1.0, 10.0, 1e2, 1e3, 1e4)
OFFSETS = (0.0, 1e3, 1e5)


def _rotations(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    return q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]


def sqrt_infos(rng, n, kappa, shape="planar", rank_deficient=False):
    """[n, 3, 3] sqrt-informations S = D^-1/2 Vᵀ and [n, 3, 3] V; columns of V ordered so that the LOW-information
    directions of S come first: planar: S's singular values (3, 3, 3κ), linear (3, 3κ, 3κ); rank_deficient: the planar
    values with the first one 0, and S = Q D^-1/2 Vᵀ with a random rotation Q (still SᵀS = V D^-1 Vᵀ)."""
    V = _rotations(rng, n)
    base = 3.0
    if shape == "planar":
        d = np.array([base, base, base * kappa])
    else:
        d = np.array([base, base * kappa, base * kappa])
    if rank_deficient:
        d = d.copy()
        d[0] = 0.0
    S = d[None, :, None] * np.transpose(V, (0, 2, 1))
    if rank_deficient:
        S = np.einsum("nij,njk->nik", _rotations(rng, n), S)
    return S, V


def _e(rng, n, V, mode, shape):
    """residual vectors e [n, 3] of 1e-2 … 1e-1 m"""
    size = 10.0 ** rng.uniform(-2.0, -1.0, size=n)
    if mode == "iso":
        u = rng.normal(size=(n, 3))
    elif mode == "null":  # the null direction of a rank-deficient S
        u = V[:, :, 0]
    else:  # in the low-information directions: the plane (2 of them) / the line (1)
        k = 2 if shape == "planar" else 1
        u = np.einsum("nij,nj->ni", V[:, :, :k], rng.normal(size=(n, k)))
    return u / np.linalg.norm(u, axis=1, keepdims=True) * size[:, None]


def ndt_case(n, kappa=10.0, shape="planar", e_mode="plane", offset=0.0, offset_in="map", rank_deficient=False, seed=0,
             n_voxels=None, R=R_TEST, t=T_TEST, direction=(1.0, 0.5, 0.1), extent=2.0):
    """One input family.  Returns (planes [15, n], pose (R, t), voxels) where voxels = (points [3, n], index [n],
    means [V, 3], sqrt_infos [V, 9]) describes the same correspondences as a voxel-indexed dataset (every item refers to
    voxel index[i]; planes are exactly that expansion).  offset_in = "map": p and mu near `offset`, t as given;
    "pose": t (and so mu) near `offset` × direction, p near 0.  The voxel means spread over ±extent m around that point
    (fp32 rounds e = R p + t - mu to about u·extent: small extents keep that below the arithmetic being measured)."""
    rng = np.random.default_rng(seed)
    nv = n_voxels or max(1, n // 4)
    S, V = sqrt_infos(rng, nv, kappa, shape, rank_deficient)
    vid = rng.integers(0, nv, size=n)
    vid[:nv] = np.arange(min(nv, n))
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).copy()
    direction = np.asarray(direction, dtype=np.float64)
    if offset_in == "pose":
        t = t + offset * direction
        local = rng.uniform(-extent, extent, size=(nv, 3)) * np.array([1.0, 1.0, 0.2])
        means = local + t  # the points sit near the sensor, the map far from the origin
    else:
        means = rng.uniform(-extent, extent, size=(nv, 3)) * np.array([1.0, 1.0, 0.2]) + offset * direction
    e = _e(rng, n, V[vid], e_mode, shape)
    x = means[vid] + e
    p = (x - t) @ R  # Rᵀ (x - t)
    # x = mu + e is itself an fp64 number, and R p + t lands within an ulp of p of it: an evaluation that adds t last
    # would round back onto x and get e = x - mu exactly.  A jitter of a few ulps of |x| moves R p + t off that grid.
    p = p + rng.uniform(-4.0, 4.0, size=p.shape) * np.spacing(np.max(np.abs(x), axis=1, keepdims=True))
    Sm = S[vid].reshape(n, 9)
    planes = np.ascontiguousarray(np.concatenate([p.T, means[vid].T, Sm.T], axis=0))
    voxels = (np.ascontiguousarray(p.T), vid.astype(np.int32), means, S.reshape(nv, 9))
    return planes, (R, t), voxels


def ndt3_case(n, kappa=10.0, shape="planar", e_mode="plane", offset=0.0, offset_in="map", rank_deficient=False, seed=0):
    """As ndt_case, for the 3-DoF problem: the points are generated through (R2, t2) acting on x, y (offsets in x, y only).
    Returns (planes, (R2, t2), voxels)."""
    R3 = np.eye(3)
    R3[:2, :2] = R2_TEST
    planes, (_, t3), vox = ndt_case(n, kappa, shape, e_mode, offset, offset_in, rank_deficient, seed, R=R3,
                                    t=np.array([T2_TEST[0], T2_TEST[1], 0.0]), direction=(1.0, 0.5, 0.0))
    return planes, (R2_TEST, t3[:2].copy()), vox


def huber_edge_case(n, th, seed=0):
    """NDT items whose exact s spreads over the Huber branch: s = th² exactly, th² (1 ± k 2^-52) for k ≤ 8, and out to
    1e20 th² (log-spaced), so that both branches and the switch are exercised; S scaled per item to hit the target."""
    rng = np.random.default_rng(seed)
    planes, pose, _ = ndt_case(n, 10.0, "planar", "iso", seed=seed)
    R, t = pose
    k = np.arange(n)
    near = th * th * (1.0 + (k % 17 - 8) * 2.0 ** -52)
    far = th * th * 10.0 ** rng.uniform(-6.0, 20.0, size=n)
    target = np.where(k % 3 == 0, far, near)
    target[0] = th * th
    p, mu, S = planes[0:3].T, planes[3:6].T, planes[6:15].T.reshape(n, 3, 3)
    e = p @ R.T + t - mu
    r = np.einsum("nij,nj->ni", S, e)
    s = np.einsum("ni,ni->n", r, r)
    S = S * np.sqrt(target / s)[:, None, None]
    planes[6:15] = S.reshape(n, 9).T
    return planes, pose


def exponential_edge_case(n, c2, seed=0):
    """NDT items with c2·s log-spaced from 1e-8 to 2000 (fp64 exp underflows past ≈ 745, fp32 past ≈ 104)."""
    rng = np.random.default_rng(seed)
    planes, pose, _ = ndt_case(n, 10.0, "planar", "iso", seed=seed)
    R, t = pose
    target = 10.0 ** rng.uniform(-8.0, np.log10(2000.0), size=n) / c2
    p, mu, S = planes[0:3].T, planes[3:6].T, planes[6:15].T.reshape(n, 3, 3)
    e = p @ R.T + t - mu
    r = np.einsum("nij,nj->ni", S, e)
    s = np.einsum("ni,ni->n", r, r)
    planes[6:15] = (S * np.sqrt(target / s)[:, None, None]).reshape(n, 9).T
    return planes, pose


REPROJ_INTR = (525.0, 525.0, 320.0, 240.0)  # fx, fy, cx, cy
MIN_DEPTH = 0.03


def reproj_case(n, kind="mixed", seed=0, R=R_TEST, t=T_TEST, pixel_range=1e4):
    """Reprojection correspondences: X in front of and behind the camera (depths -5 … 50 m, kept at least 1e-6 away from
    min_depth), pixels out to ±pixel_range, pixel noise of a few px.  kind = "threshold": identity pose, every depth
    exactly min_depth (the reference counts such a point: its test is !(z < min_depth)) next to points just below it."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = REPROJ_INTR
    if kind == "threshold":
        R, t = np.eye(3), np.zeros(3)
        z = np.full(n, MIN_DEPTH)
        z[1::2] = np.nextafter(MIN_DEPTH, 0.0)
    else:
        z = rng.uniform(-5.0, 50.0, size=n)
        z = np.where(np.abs(z - MIN_DEPTH) < 1e-6, MIN_DEPTH + 1e-3, z)
    uv = rng.uniform(-pixel_range, pixel_range, size=(n, 2))
    zz = np.where(np.abs(z) < 1e-3, 1e-3, z)
    xc = np.stack([(uv[:, 0] - cx) / fx * zz, (uv[:, 1] - cy) / fy * zz, z], axis=1)  # camera frame
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    X = (xc - t) @ R  # world frame: R X + t = xc
    pix = uv + rng.normal(scale=3.0, size=(n, 2))
    if kind == "threshold":
        X = xc
    planes = np.ascontiguousarray(np.concatenate([X.T, pix.T], axis=0))
    intr = (1.0 / fx, 1.0 / fy, cx, cy)
    return planes, (R, np.asarray(t, dtype=np.float64)), intr
