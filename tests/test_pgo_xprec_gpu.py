"""The pose-graph kernels against 50 digits on the hard states of pgo_hard_inputs.py: linearisation
(pgo_linearize_kernel, pgo_switch_linearize_kernel), both products (owner-computes and block-local), the retraction
(pgo_retract_kernel) from the step read back, and the state after a retraction (pgo_refresh_entries_kernel).  Bound per
state and quantity: max(4 x the float64 oracle's error, 8) units of 2^-52 in the first-order error scale; nothing in it
comes from the kernels.  test_pgo_xprec.py holds the CPU half: the states, the yardstick, and the measure's teeth."""
import numpy as np
import pytest

from tests import pgo_hard_inputs as hi

pytestmark = pytest.mark.gpu


def _graph(ctx, st, block):
    from nonlinear_optimizer_for_slam_amd import pgo
    with ctx.options(pgo_block=block):
        g = pgo.PoseGraph(ctx, st["poses"], st["ref"], st["qry"], st["meas"], st["sw"], st["free"], st["fixed"])
    assert (g.layout_info()["block_poses"] != 0) == (block != 0)
    return g


def _measure(g, st, x):
    """linearize, read everything back, multiply at every lambda → (quantities in the layout of the reference, gnorm)"""
    cost, gnorm = g.linearize()
    got = hi.split_gpu(st["poses"].shape[0], cost, g.vector("gradient"), g.vector("hdiag"),
                       {lam: g.matvec(lam, x) for lam in hi.LAMBDAS})
    return got, gnorm


def _check(got, gnorm, ref, bound, label):
    quantities = [q for q in hi.QUANTITIES if q != "switch_curvature"]       # read through the switch rows of the product
    xp, scale = ref
    errors = {q: (max(hi.error_eps(got[q][lam], xp[q][lam], scale[q][lam]) for lam in hi.LAMBDAS)
                  if q.endswith("product") else hi.error_eps(got[q], xp[q], scale[q])) for q in quantities}
    errors["gnorm"] = hi.gnorm_error_eps(gnorm, ref)
    print("  %-24s " % label + "  ".join("%s %.2f/%.1f" % (q, errors[q], 8.0 if q == "gnorm" else bound[q]) for q in errors))
    for q in quantities:
        assert errors[q] <= bound[q], (label, q, errors[q], bound[q])
    assert errors["gnorm"] <= 8.0, (label, errors["gnorm"])
    return errors


@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("name", hi.FAMILIES)
def test_linearisation_and_product_within_rounding_of_50_digits(ctx, name, block):
    st = hi.family(name)
    x = hi.masked_x(st)
    g = _graph(ctx, st, block)
    got, gnorm = _measure(g, st, x)
    g.close()
    _check(got, gnorm, hi.family_reference(name), hi.bounds(hi.family_yardstick(name)), "%s block=%d" % (name, block))


@pytest.mark.parametrize("name", ["baseline", "half_turn"])
def test_negated_quaternions_give_the_same_bits(ctx, name):
    """q and -q are the same rotation, a negation is exact, and it flips e, r_R, B and C together: the cost, every gradient
    entry and every entry of the diagonal blocks come back bit for bit."""
    st = hi.family(name)
    flip = np.random.default_rng(5).permutation(st["poses"].shape[0]) < st["poses"].shape[0] // 2
    neg = dict(st, poses=st["poses"].copy())
    neg["poses"][flip, 3:] *= -1.0
    out = []
    for s in (st, neg):
        g = _graph(ctx, s, 1)
        cost, gnorm = g.linearize()
        out.append((cost, gnorm, g.vector("gradient"), g.vector("hdiag")))
        g.close()
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])
    assert np.any(out[0][2] != 0.0)


def test_retraction_against_the_true_exponential(ctx):
    """pgo_retract_kernel from the step that vector("step") reads back, on 300 independent pairs whose rotation steps span
    1e-12 … 3 rad and crowd both sides of the kernel's |dw| < 1e-6 branch."""
    st = hi.retraction_graph()
    n, free_pose, free_sw = st["poses"].shape[0], st["fixed"] == 0, st["free"] == 1
    g = _graph(ctx, st, 1)
    g.linearize()
    g.solve(hi.RETRACT_LAMBDA, 50, 1e-13)
    before, sw_before = g.state()
    step = g.vector("step")
    g.retract()
    after, sw_after = g.state()
    g.close()
    assert np.array_equal(before, st["poses"]) and np.array_equal(sw_before, st["sw"])
    dp = np.stack([step[k * n:(k + 1) * n] for k in range(3)], axis=1)
    dw = hi.rotation_steps(n, step)
    below, above = hi.branch_counts(dw)
    assert below >= 8 and above >= 8, (below, above)
    assert np.array_equal(after[free_pose, :3], before[free_pose, :3] + dp[free_pose])
    assert np.array_equal(sw_after[free_sw], sw_before[free_sw] + step[6 * n:][free_sw])
    assert np.any(step[6 * n:][free_sw] != 0.0) and np.any(dp[free_pose] != 0.0)
    assert np.array_equal(after[~free_pose], before[~free_pose])            # fixed poses: every bit
    assert np.array_equal(sw_after[~free_sw], sw_before[~free_sw])
    xp = hi.retract_xp(before[free_pose, 3:], dw[free_pose])
    oracle_poses, _ = hi.oracle_retract(st, step)
    yard = hi.quaternion_error_eps(oracle_poses[free_pose, 3:], xp)
    err = hi.quaternion_error_eps(after[free_pose, 3:], xp)
    norm = hi.norm_error_eps(after[free_pose, 3:])
    print("  retraction: error %.2f, oracle %.2f, bound %.1f; norm %.2f; |dw| below/above 1e-6: %d/%d"
          % (err, yard, max(4 * yard, 8.0), norm, below, above))
    assert err <= max(4.0 * yard, 8.0), (err, yard)
    assert norm <= 4.0, norm


@pytest.mark.parametrize("block", [0, 1])
@pytest.mark.parametrize("name", ["baseline", "switches"])
def test_the_state_after_a_retraction(ctx, name, block):
    """linearize, solve, retract, then linearize and multiply again — against the 50-digit reference of the state that
    state() returns.  The block-local product keeps its own copy of every switch value: with free switches
    pgo_refresh_entries_kernel must have renewed it (`switches`), without any the refresh is skipped (`baseline`)."""
    st = hi.family(name)
    g = _graph(ctx, st, block)
    g.linearize()
    g.solve(1e-3, 200, 1e-10)
    g.retract()
    poses, sw = g.state()
    new = dict(st, poses=poses, sw=sw)
    assert np.array_equal(sw[st["free"] == 0], st["sw"][st["free"] == 0])
    assert np.all(poses[st["fixed"] == 0, :3] != st["poses"][st["fixed"] == 0, :3])
    if name == "switches":
        assert np.sum(sw != st["sw"]) > 0.9 * np.sum(st["free"])
    x = hi.masked_x(new, seed=1)
    got, gnorm = _measure(g, new, x)
    g.close()
    ref = hi.reference(new, x)
    _check(got, gnorm, ref, hi.bounds(hi.yardstick(new, x, ref)), "%s block=%d after retract" % (name, block))
