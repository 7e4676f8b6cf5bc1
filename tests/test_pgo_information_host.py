"""CPU half of the information-weighted pose graph: the numpy restatement of the rule in include/nos.h
(tests/pgo_info_inputs.py) against central differences, against the unweighted oracle at Omega = I, against 50 digits —
which records the float64 error e_np the GPU bound is built on — and the sign convention with the two mistakes it
must catch."""
import numpy as np
import pytest

from oracle import oracle_pgo as op
from tests import pgo_hard_inputs as hi
from tests import pgo_info_inputs as pi


def test_cases_are_what_they_claim():
    st = pi.case("chain13")
    nbr = set(st["qry"][st["ref"] == 12]) | set(st["ref"][st["qry"] == 12])
    assert nbr == {0} and st["fixed"][0] == 1                    # pose 12: no free neighbour
    st = pi.case("two_groups")
    assert (st["poses"].shape[0] + 255) // 256 == 2 and (st["ref"].size + 255) // 256 == 3
    assert list(np.nonzero(st["fixed"])[0]) == [1, 2, 200]
    assert np.all(st["sw"][st["free"] == 1] == 0.7) and np.array_equal(st["free"], np.arange(513) % 3 == 0)
    st = pi.case("two_level")
    assert st["poses"].shape[0] == 600 and st["poses"].shape[0] >= 4 * pi.AGG["two_level"]
    for name in pi.CASES:
        info = pi.case(name)["information"]
        ev = np.linalg.eigvalsh(info)
        assert np.array_equal(info, np.swapaxes(info, 1, 2))
        assert np.all(np.abs(ev[::5, 0]) <= 1e-12 * ev[::5, -1])             # every fifth: one eigenvalue 0
        assert np.all(ev[np.arange(len(ev)) % 5 != 0, 0] >= 0.99e-2) and np.all(ev[:, -1] <= 1.01e4)


@pytest.mark.parametrize("name", ["chain13", "two_groups"])
def test_jacobians_against_central_differences(name):
    """d r~ / d(dp, dw) of both ends under p += dp, q <- q Exp(dw), by central differences with h = 1e-6: truncation
    h^2 |r'''| / 6 ~ 1e-12 and rounding 1e-16 / h ~ 1e-10 on entries of size <= 10."""
    st = pi.case(name)
    g = pi.info_graph(st)
    h, worst = 1e-6, 0.0
    for e in range(0, st["ref"].size, 7):
        ir, iq = int(st["ref"][e]), int(st["qry"][e])
        _, Jr, Jq = g.edge(e)
        for pose, J in ((ir, Jr), (iq, Jq)):
            num = np.zeros((6, 6))
            for k in range(6):
                r = []
                for sgn in (1.0, -1.0):
                    d = np.zeros(6)
                    d[k] = sgn * h
                    g2 = pi.info_graph(st)
                    g2.poses[pose, :3] += d[:3]
                    g2.poses[pose, 3:] = op.qmul(g2.poses[pose, 3:], op.qexp(d[3:]))
                    r.append(g2.edge(e)[0])
                num[:, k] = (r[0] - r[1]) / (2 * h)
            worst = max(worst, float(np.max(np.abs(num - J))))
    print("  %s: largest |J - central difference| = %.2e" % (name, worst))
    assert worst <= 5e-9, worst


@pytest.mark.parametrize("name", pi.CASES)
def test_identity_information_gives_the_unweighted_cost_and_gradient(name):
    """|r~| = |r| and J~^T r~ = J^T r: with Omega = I cost and gradient are oracle_pgo.Graph's to rounding (1e-12
    relative); the diagonal blocks are not — another residual with the same norm."""
    st = pi.case(name)
    eye = np.broadcast_to(np.eye(6), (st["ref"].size, 6, 6))
    H, g, cost = pi.info_graph(st, information=eye).linearize()
    H0, g0, cost0 = hi.oracle_graph(st).linearize()
    assert abs(cost - cost0) <= 1e-12 * cost0
    assert np.max(np.abs(g - g0)) <= 1e-12 * np.max(np.abs(g0))
    assert abs(H - H0).max() > 1e-3 * abs(H0).max()


@pytest.mark.parametrize("name", pi.CASES)
def test_restatement_against_50_digits(name):
    """Records e_np, the yardstick of tests/test_pgo_information.py.  The cap is a sanity check of the restatement (an
    entry is a sum of a few dozen products: its rounding cannot reach 2^10 units of the first-order scale), not a bound on
    anything else."""
    e_np = pi.case_yardstick(name)
    print("  %s: e_np " % name + "  ".join("%s %.2f" % (q, e_np[q]) for q in pi.QUANTITIES))
    for q in pi.QUANTITIES:
        assert e_np[q] <= 1024.0, (name, q, e_np[q])


def _perturbed_pair(seed, xi, mutate=()):
    """Two poses whose relative pose is (t_true, R_true) exactly consistent; the measurement is (t_m, R_m) with
    t_true = t_m + dt, R_true = R_m Exp(dtheta) → cost of the one constraint"""
    rng = np.random.default_rng(seed)
    qr, qq = op.qexp(rng.normal(scale=0.9, size=3)), op.qexp(rng.normal(scale=0.9, size=3))
    pr = rng.normal(scale=5.0, size=3)
    t_true = rng.normal(scale=2.0, size=3)
    pq = pr + op.qrot(qr) @ t_true
    q_true = op.qmul(op.qconj(qr), qq)
    q_m = op.qmul(q_true, op.qexp(-xi[3:]))
    meas = np.concatenate([t_true - xi[:3], q_m / np.linalg.norm(q_m)])
    omega = pi.draw_information(2, seed + 100)[1]
    g = pi.InfoGraph(np.stack([np.concatenate([pr, qr]), np.concatenate([pq, qq])]), [0], [1], meas[None], omega[None],
                     mutate=mutate)
    return g.cost(), float(xi @ omega @ xi), omega


def test_sign_convention_and_the_mutants_it_catches():
    """Perturb a measurement by xi = (dt, dtheta) as the header defines it: the cost is xi^T Omega xi to second order.
    |xi| = 1e-4: the third-order remainder is ~ |xi| relative, so 1e-3 holds for the rule; Omega with its off-diagonal
    blocks used without D, or the world-frame r_t under a rotated reference, are wrong at first order (relative error of
    order one) — asserted above 1e-2."""
    def worst(mutate):
        errs = []
        for seed in range(12):
            xi = 1e-4 * np.random.default_rng(900 + seed).normal(size=6)
            cost, want, _ = _perturbed_pair(seed, xi, mutate)
            errs.append(abs(cost - want) / want)
        return max(errs)

    errors = {m: worst((m,) if m else ()) for m in ("", "no_D", "world_rt")}
    print("  largest relative |cost - xi^T Omega xi| over 12 pairs: %s" % errors)
    assert errors[""] <= 1e-3, errors
    assert errors["no_D"] > 1e-2 and errors["world_rt"] > 1e-2, errors


def test_information_from_sums_and_packing():
    from nonlinear_optimizer_for_slam_amd import pgo
    sums = np.arange(28, dtype=np.float64) + 1.0
    A = pgo.information_from_sums(sums)
    assert A.shape == (6, 6) and np.array_equal(A, A.T)
    assert np.array_equal(A[np.triu_indices(6)], sums[:21])
    info = pi.case("chain13")["information"]
    assert np.array_equal(pgo.pack_information(info, 15), pi.upper21(info))
    assert np.array_equal(pgo.pack_information(pi.upper21(info), 15), pi.upper21(info))
    with pytest.raises(ValueError):
        pgo.pack_information(info[:14], 15)
    bad = info.copy()
    bad[3, 0, 4] += 1.0
    with pytest.raises(ValueError):
        pgo.pack_information(bad, 15)


def test_quaternion_of_a_rotation_matrix_on_every_branch():
    """pipeline._quat_wxyz (the packing of map_edge): rotations near pi about x, y and z take the three branches in which
    w is not the largest component, small ones the fourth; qrot of the result is the matrix to rounding, |q| = 1, w >= 0."""
    from nonlinear_optimizer_for_slam_amd import pipeline
    rng = np.random.default_rng(77)
    largest = set()
    for axis in (0, 1, 2, None):
        for angle in (np.pi - 1e-3, np.pi - 1e-9, np.pi, 2.5, 0.3, 1e-9, 0.0):
            a = rng.normal(size=3) if axis is None else np.eye(3)[axis] + 1e-3 * rng.normal(size=3)
            a /= np.linalg.norm(a)
            R = op.qrot(op.qexp(angle * a))
            q = pipeline._quat_wxyz(R)
            largest.add(int(np.argmax(np.abs(q))))
            assert abs(np.linalg.norm(q) - 1.0) <= 4e-16 and q[0] >= 0.0
            assert np.max(np.abs(op.qrot(q) - R)) <= 1e-15, (axis, angle)
    assert largest == {0, 1, 2, 3}


def test_corridor_restatement_lands_on_the_loop_closure():
    """The restatement's own answer on the corridor graph: the end of the chain on the loop closure, the unweighted
    oracle 1 cm off, and the two more than ten times the planted noise apart somewhere along the chain."""
    st = pi.corridor()
    w = pi.info_graph(st, min_norm=True)
    w.optimize()
    u = hi.oracle_graph(st)
    u.optimize()
    n = pi.CORRIDOR_POSES
    assert abs(w.poses[n - 1, 0] - st["true"][n - 1, 0]) <= 1e-6
    assert abs(u.poses[n - 1, 0] - st["true"][n - 1, 0]) > 0.5 * pi.CORRIDOR_NOISE
    assert np.max(np.abs(w.poses[:, :3] - u.poses[:, :3])) > 10 * pi.CORRIDOR_NOISE
