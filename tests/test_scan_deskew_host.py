"""The yardsticks of the scan deskew and the two pose/twist helpers, without a GPU.

1. tests/scan_deskew_inputs.py::restate — the numpy restatement the device test is measured against — is itself held to the
   50-digit truth: 8 eps on typ, fast, tiny, thr, denorm and pure_t, 32 eps on big (where the error grows with theta).  Loose
   caps on the yardstick, from its measured 1.7 / 4.6 / 1.2 / 2.3 / 0.5 / 0.5 and 21 eps: they keep the device test from
   hiding behind a bad restatement.
2. pipeline.twist_pose is the SE(3) exponential (against mpmath) and pipeline.pose_twist its inverse, each within 4 x the
   error the same computation makes when written naively in numpy (measured here; where the naive form gives nothing
   finite it grants nothing), and never asked for less than 4 eps of the largest component."""
import mpmath
import numpy as np
import pytest

from tests import scan_deskew_inputs as di

EPS = di.EPS
CAPS = {"typ": 8.0, "fast": 8.0, "tiny": 8.0, "thr": 8.0, "denorm": 8.0, "pure_t": 8.0, "big": 32.0}


@pytest.mark.parametrize("name", list(di.FAMILIES))
def test_the_numpy_restatement_is_close_to_50_digits(name):
    worst = 0.0
    for s_ref in di.S_REFS:
        c = di.case(name, s_ref)
        worst = max(worst, c["restate_eps"])
        if name == "thr":
            assert di.thr_straddles(c["s"], s_ref), s_ref  # both arms of c are exercised at every s_ref
    print("%s: restate worst %.2f eps (cap %.0f eps)" % (name, worst, CAPS[name]))
    assert worst <= CAPS[name]


def test_restate_leaves_points_alone_where_the_rule_says_so():
    p, s, twist = di.family("typ")
    assert np.array_equal(di.restate(p, np.full_like(s, 0.5), 0.5, twist), p)
    assert np.array_equal(di.restate(p, s, 1.0, np.zeros(6)), p)


# ------------------------------------------------------------------------------ twist_pose, pose_twist

def _naive_exp(twist):
    v, w = twist[:3], twist[3:]
    th = np.sqrt(w @ w)
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    with np.errstate(all="ignore"):
        a, b, c = np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        return np.eye(3) + a * W + b * (W @ W), v + b * (W @ v) + c * (W @ W @ v)


def _naive_log(R, t):
    with np.errstate(all="ignore"):
        th = np.arccos((np.trace(R) - 1.0) / 2.0)
        w = th / (2.0 * np.sin(th)) * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        d = (1.0 - th * np.sin(th) / (2.0 * (1.0 - np.cos(th)))) / th ** 2
        return np.concatenate([t - 0.5 * (W @ t) + d * (W @ W @ t), w])


def _granted(naive_err, largest):
    """4 x the naive computation's error where that is a number, and at least 4 eps of the largest component."""
    floor = 4.0 * EPS * largest
    return max(4.0 * naive_err, floor) if np.isfinite(naive_err) else floor


def _exp_errors(R, t, twist):
    """→ (max |R - R_mp|, max |t - t_mp|) against the mpmath exponential."""
    Rm, tm = di.exp_se3(twist)
    with mpmath.mp.workdps(50):
        eR = max(abs(mpmath.mpf(float(R[i, j])) - Rm[i][j]) for i in range(3) for j in range(3))
        et = max(abs(mpmath.mpf(float(t[i])) - tm[i]) for i in range(3))
    return float(eR), float(et)


@pytest.mark.parametrize("name", list(di.FAMILIES))
def test_twist_pose_is_the_se3_exponential(name):
    from nonlinear_optimizer_for_slam_amd import pipeline
    twist = di.twist_of(name)
    pose = pipeline.twist_pose(twist)
    eR, et = _exp_errors(pose.R, pose.t, twist)
    Rn, tn = _naive_exp(twist)
    nR, nt = _exp_errors(Rn, tn, twist) if np.all(np.isfinite(Rn)) and np.all(np.isfinite(tn)) else (np.nan, np.nan)
    bR, bt = _granted(nR, 1.0), _granted(nt, max(1.0, float(np.max(np.abs(twist[:3])))))
    print("%s: R off by %.2e (naive %.2e, granted %.2e), t off by %.2e (naive %.2e, granted %.2e)" % (name, eR, nR, bR, et, nt, bt))
    assert eR <= bR and et <= bt


@pytest.mark.parametrize("name", ["typ", "tiny", "thr", "denorm", "pure_t"])
def test_pose_twist_inverts_twist_pose(name):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    twist = di.twist_of(name)
    assert np.sqrt(twist[3:] @ twist[3:]) < np.pi
    got = pipeline.pose_twist(Pose(), pipeline.twist_pose(twist))
    err = float(np.max(np.abs(got - twist)))
    naive = _naive_log(*_naive_exp(twist))
    naive_err = float(np.max(np.abs(naive - twist))) if np.all(np.isfinite(naive)) else np.nan
    granted = _granted(naive_err, float(np.max(np.abs(twist))))
    print("%s: round trip off by %.2e (naive %.2e, granted %.2e)" % (name, err, naive_err, granted))
    assert err <= granted
    # from a pose that is not the identity, the same twist: Log(T_a^-1 (T_a Exp(xi)))
    a = pipeline.twist_pose(np.array([0.3, -1.0, 2.0, 0.4, 0.2, -0.7]))
    e = pipeline.twist_pose(twist)
    b = Pose(a.R @ e.R, a.R @ e.t + a.t)
    again = pipeline.pose_twist(a, b)
    assert float(np.max(np.abs(again - twist))) <= 16.0 * EPS * max(3.0, float(np.max(np.abs(twist))))  # + a's own products


def test_pose_twist_of_a_pose_with_itself_is_exactly_zero():
    from nonlinear_optimizer_for_slam_amd import pipeline
    a = pipeline.twist_pose(np.array([0.3, -1.0, 2.0, 0.4, 0.2, -0.7]))
    z = pipeline.pose_twist(a, a)
    assert z.shape == (6,) and np.array_equal(z, np.zeros(6))
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    assert np.array_equal(pipeline.pose_twist(a, Pose(a.R.copy(), a.t.copy())), np.zeros(6))


@pytest.mark.parametrize("theta", [0.0, 1e-300, 1e-9, 1.0, np.pi - 1e-6])
def test_twist_pose_rotation_is_orthonormal_and_inverted_at_every_angle(theta):
    from nonlinear_optimizer_for_slam_amd import pipeline
    from nonlinear_optimizer_for_slam_amd.solvers import Pose
    axis = np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    twist = np.concatenate([[0.5, -0.25, 2.0], theta * axis])
    pose = pipeline.twist_pose(twist)
    off = float(np.max(np.abs(pose.R.T @ pose.R - np.eye(3))))
    print("theta %.17g: |R^T R - I| max %.2e" % (theta, off))
    assert off <= 8.0 * EPS
    assert abs(np.linalg.det(pose.R) - 1.0) <= 8.0 * EPS
    # the logarithm comes back up to pi - 1e-6: near pi the angle is known to eps / sin(theta) only, 2e-10 here
    back = pipeline.pose_twist(Pose(), pose)
    tol = 64.0 * EPS * 2.0 / max(np.sin(theta), 1e-3) if theta > 3.0 else 64.0 * EPS * 2.0
    assert float(np.max(np.abs(back - twist))) <= tol
