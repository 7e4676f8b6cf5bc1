"""The robust loss on pose-graph constraints, CPU half: the shared inputs (tests/pgo_robust_inputs.py) and the rule itself,
checked on the numpy restatement before the GPU is measured against it (tests/test_pgo_robust.py).  No GPU."""
import numpy as np
import pytest

from tests import pgo_hard_inputs as hi
from tests import pgo_info_inputs as pi
from tests import pgo_robust_inputs as ri


@pytest.mark.parametrize("name", ri.CASES)
def test_without_a_loss_the_restatement_is_the_weighted_one(name):
    """cost, gradient and matrix of RobustGraph(loss=None) against InfoGraph: the same numbers up to the rounding of a sum
    taken in another order (the 13 x 13 local blocks are formed from 6 rows here, from 7 there)"""
    st = pi.case(name)
    Hw, gw, cw = pi.info_graph(st).linearize()
    Hr, gr, cr = ri.robust_graph(st, None).linearize()
    assert abs(cr - cw) <= 4 * hi.EPS * abs(cw)
    assert np.max(np.abs(gr - gw)) <= 4 * hi.EPS * np.max(np.abs(gw))
    assert abs(Hr - Hw).max() <= 4 * hi.EPS * abs(Hw).max()
    assert abs(ri.robust_graph(st, None).cost() - pi.info_graph(st).cost()) <= 4 * hi.EPS * abs(cw)
    assert np.array_equal(ri.robust_graph(st, None).weights(), np.ones(st["ref"].size))


def _with_free_switches(st):
    """chain13 and two_level have no free switch: the cost's derivative along a switch is checked on a copy in which every
    third switch is free at 0.7 (two_groups is built that way)"""
    if st["free"].any():
        return st
    out = dict(st)
    out["free"] = (np.arange(st["ref"].size) % 3 == 0).astype(np.uint8)
    out["sw"] = np.where(out["free"], 0.7, 1.0)
    return out


@pytest.mark.parametrize("kind", ri.KINDS)
@pytest.mark.parametrize("name", ri.CASES)
def test_the_gradient_is_the_gradient_of_the_cost(name, kind):
    """Central differences of cost() along 8 pose coordinates and 4 free switches against 2 g (the cost is a sum of
    squares: g is half its gradient), relative difference <= 1e-4.  This is the test w = 2 rho' fails."""
    st = _with_free_switches(pi.case(name))
    loss = ri.case_loss(name, kind)
    n, m = st["poses"].shape[0], st["ref"].size
    g0 = ri.robust_graph(st, loss)
    _, grad, _ = g0.linearize()
    rng = np.random.default_rng(5)
    free_poses = np.nonzero(st["fixed"] == 0)[0]
    coords = [int(k * n + rng.choice(free_poses)) for k in (0, 1, 2, 3, 4, 5, 0, 4)]
    coords += [int(6 * n + e) for e in rng.choice(np.nonzero(st["free"])[0], size=4, replace=False)]
    h = 1e-6
    worst = 0.0
    for c in coords:
        vals = []
        for sign in (1.0, -1.0):
            g = ri.robust_graph(st, loss)
            dx = np.zeros(6 * n + m)
            dx[c] = sign * h
            g.retract(dx)
            vals.append(g.cost())
        fd = (vals[0] - vals[1]) / (2 * h)
        rel = abs(fd - 2.0 * grad[c]) / abs(2.0 * grad[c])
        worst = max(worst, rel)
        assert rel <= 1e-4, (name, kind, c, fd, 2.0 * grad[c])
    print("  %s %s: largest relative difference %.1e" % (name, kind, worst))


@pytest.mark.parametrize("kind", ri.KINDS)
def test_the_matrix_of_two_groups_is_positive_definite(kind):
    """171 free switches at 0.7: with the switch curvature rho + c^2 the smallest eigenvalue stays above 0"""
    H, _, _ = ri.robust_graph(pi.case("two_groups"), ri.case_loss("two_groups", kind)).linearize()
    ev = np.linalg.eigvalsh(H.toarray())
    print("  %s: smallest eigenvalue %.2e, largest %.2e" % (kind, ev[0], ev[-1]))
    assert ev[0] > 0.0


@pytest.mark.parametrize("name", ri.CASES)
def test_either_huber_branch_holds_a_quarter_of_the_constraints(name):
    q = ri.robust_graph(pi.case(name), None).q()
    delta = ri.case_loss(name, "huber")[1]
    inside = float(np.mean(q <= delta * delta))
    print("  %s: sqrt(q) %.2g … %.2g, %.0f %% of the constraints at or below the threshold %.3g" % (
        name, np.sqrt(q.min()), np.sqrt(q.max()), 100 * inside, delta))
    assert 0.25 <= inside <= 0.75


@pytest.mark.parametrize("variant", ri.SCENE_VARIANTS)
def test_the_scene_needs_the_loss(variant):
    """the restatement without a loss ends at least 100 times farther from the true positions than with it"""
    with_loss, weights, _ = ri.scene_restatement(variant, True)
    without, _, _ = ri.scene_restatement(variant, False)
    print("  %s: %.2e m with the loss, %.3f m without (%.0f x); outlier weight %.1e" % (
        variant, with_loss, without, without / with_loss, weights[ri.SCENE_OUTLIER]))
    assert without >= 100.0 * with_loss
    assert weights[ri.SCENE_OUTLIER] < 1e-3 and np.all(weights[list(ri.SCENE_LOOPS)] > 0.99)


@pytest.mark.parametrize("kind", ri.KINDS)
@pytest.mark.parametrize("name", ri.CASES)
def test_the_gpu_bound_tells_the_planted_mistakes_from_the_rule(name, kind):
    """w = 2 rho' moves the restatement's gradient, and h_s = w q + c^2 with g_s = s w q - c^2 (1 - s) moves its switch
    gradient and switch curvature (seen through the switch rows of the product), by more than the bound the GPU test
    allows — so that test fails on either.  The second mistake lives on free switches: two_groups has them."""
    ref = ri.case_reference(name, kind)
    bound = ri.bounds(ri.case_yardstick(name, kind))
    doubled = ri.score(ri.case_restatement(name, kind, mutate=("w2",)), ref)
    assert doubled["gradient"] > bound["gradient"] and doubled["weights"] > bound["weights"], (doubled, bound)
    if pi.case(name)["free"].any():
        wrong = ri.score(ri.case_restatement(name, kind, mutate=("hs_wq",)), ref)
        assert wrong["switch_gradient"] > bound["switch_gradient"], (wrong, bound)
        assert wrong["switch_product"] > bound["switch_product"], (wrong, bound)
        print("  %s %s: w = 2 rho' → gradient %.1e units; h_s = w q + c^2 → switch gradient %.1e, switch rows %.1e (bounds %.0f)"
              % (name, kind, doubled["gradient"], wrong["switch_gradient"], wrong["switch_product"], bound["gradient"]))
