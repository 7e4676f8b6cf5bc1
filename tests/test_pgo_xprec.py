"""The pose-graph linearisation against 50 digits, CPU half: the hard states are where they are meant to
be, the float64 oracle — the yardstick of the GPU bounds — stays within 8 units of 2^-52 of the 50-digit reference on
every one of them, and the measure catches float64 twins with one planted mistake each by more than 100 x their bound.
The GPU half is test_pgo_xprec_gpu.py."""
import numpy as np
import pytest

from oracle import oracle_pgo as op
from tests import pgo_hard_inputs as hi


def _e_w(st):
    return np.array([op.edge_residual(st["poses"][a, :3], st["poses"][a, 3:], st["poses"][b, :3], st["poses"][b, 3:],
                                      st["meas"][e, :3], st["meas"][e, 3:])[1][0]
                     for e, (a, b) in enumerate(zip(st["ref"], st["qry"]))])


def test_the_families_sit_where_they_are_meant_to():
    for name in hi.FAMILIES:
        st = hi.family(name)
        n = st["poses"].shape[0]
        assert n == (280 if name == "hub" else hi.N_POSES) and st["fixed"][0] == 1
        assert np.sum(st["fixed"]) == (2 if name in ("long_edges", "switches") else 1), name
        crossing = (st["ref"] // hi.BLOCK) != (st["qry"] // hi.BLOCK)
        assert np.sum(crossing) >= 10, (name, int(np.sum(crossing)))     # constraints across the block boundary
        assert n > hi.BLOCK and n % hi.BLOCK != 0                          # two blocks, the second partly filled
    far, base = hi.family("far"), op.random_graph(hi.N_POSES, 3, seed=22)
    assert np.array_equal(far["poses"][:, :3], base["init"][:, :3] + hi.FAR_OFFSET)
    assert np.min(np.abs(far["poses"][:, 1])) > 5.3e6
    assert hi.oracle_graph(hi.family("converged")).cost() < 1e-12
    half = hi.family("half_turn")
    assert np.sum(np.abs(_e_w(half)) < 1e-3) >= 40
    assert 60 < np.sum(half["neg_pose"]) < 100 and np.sum(half["neg_meas"]) > 200
    long_edges = hi.family("long_edges")
    span = np.linalg.norm(long_edges["poses"][long_edges["qry"], :3] - long_edges["poses"][long_edges["ref"], :3], axis=1)
    assert 7000.0 < np.max(span) < 8100.0 and np.min(span) < 1.5
    assert np.max(np.linalg.norm(long_edges["meas"][:, :3], axis=1)) > 7000.0
    non_unit = hi.family("non_unit")
    for q in (non_unit["poses"][:, 3:], non_unit["meas"][:, 3:]):
        nrm = np.linalg.norm(q, axis=1)
        assert np.max(np.abs(nrm - 1)) < 1.001e-3 and np.mean(np.abs(nrm - 1) > 1e-4) > 0.8
    sw = hi.family("switches")
    assert set(sw["sw"].tolist()) == set(hi.SWITCH_CYCLE) and np.min(np.abs(sw["sw"][sw["sw"] != 0]) ** 2) > 1e-300
    assert set(sw["sw"][sw["free"] == 1].tolist()) == set(hi.SWITCH_CYCLE)        # every value on a free switch too
    assert np.sum(sw["free"]) == sw["ref"].size // 2
    hub = hi.family("hub")
    assert np.sum(hub["ref"] == 5) == 201 and np.sum(hub["qry"] == 6) == 201
    assert hub["ref"].size == 279 + 400


@pytest.mark.parametrize("name", hi.FAMILIES)
def test_the_yardstick_stays_within_eight_units(name, capsys):
    """A condition on the INPUTS: on every family and quantity the float64 oracle is within 8 x 2^-52 of the 50-digit
    value in the first-order error scale, so the GPU bound max(4 x yardstick, 8) is a statement about roundings."""
    y = hi.family_yardstick(name)
    with capsys.disabled():
        print("\n  %-10s " % name + "  ".join("%s %.2f" % (q, y[q]) for q in hi.QUANTITIES))
    for q in hi.QUANTITIES:
        assert y[q] <= 8.0, (name, q, y[q])
    b = hi.bounds(y)
    assert all(8.0 <= b[q] <= 32.0 for q in hi.QUANTITIES)


def test_the_unmutated_float64_twin_is_as_good_as_the_oracle():
    for name in ("baseline", "switches", "half_turn"):
        st = hi.family(name)
        got = hi.score(hi.twin(st, hi.masked_x(st)), hi.family_reference(name))
        assert all(got[q] <= 8.0 for q in hi.QUANTITIES), (name, got)


def _over_bound(name, got):
    """{quantity: error / bound} of a twin on a family"""
    sc = hi.score(got, hi.family_reference(name))
    b = hi.bounds(hi.family_yardstick(name))
    return {q: sc[q] / b[q] for q in hi.QUANTITIES}


def test_the_measure_bites():
    """Five float64 twins, one planted mistake each; every one is more than 100 x over its bound on the family named for
    it, in the quantities the mistake reaches — and not in those it does not."""
    # one constraint of the hub pose left out of its gradient
    st = hi.family("hub")
    e = int(np.nonzero(st["ref"] == 5)[0][100])
    over = _over_bound("hub", hi.twin(st, hi.masked_x(st), skip=(e, 0)))
    assert over["gradient"] > 100.0 and over["hdiag"] <= 1.0 and over["product"] <= 1.0, over
    # one entry of A = R_r [t_m]x with the wrong sign
    st = hi.family("long_edges")
    over = _over_bound("long_edges", hi.twin(st, hi.masked_x(st), mutate=("A_sign",)))
    assert min(over["gradient"], over["hdiag"], over["product"]) > 100.0 and over["cost"] <= 1.0, over
    # B built with R_m in place of R_m^T
    st = hi.family("half_turn")
    over = _over_bound("half_turn", hi.twin(st, hi.masked_x(st), mutate=("B_without_transpose",)))
    assert min(over["gradient"], over["hdiag"], over["product"]) > 100.0 and over["cost"] <= 1.0, over
    # the translation rows of a negated quaternion's residual negated along with the rotation rows
    over = _over_bound("half_turn", hi.twin(st, hi.masked_x(st), mutate=("negated_translation_rows",)))
    assert over["gradient"] > 100.0 and over["cost"] <= 1.0 and over["hdiag"] <= 1.0, over


def test_a_product_with_the_switch_values_from_before_a_retraction_is_caught():
    """What a block-local product does whose entries were not refreshed: the poses of the new state, the switch values of
    the old one.  Scored against the 50-digit reference of the new state."""
    st = hi.family("switches")
    g = hi.oracle_graph(st)
    H, grad, _ = g.linearize()
    g.retract(g.solve_step(H, grad, 1e-3))
    new = dict(st, poses=g.poses, sw=g.sw)
    assert np.all(new["sw"][st["free"] == 0] == st["sw"][st["free"] == 0])
    assert np.sum(new["sw"] != st["sw"]) > 0.9 * np.sum(st["free"])
    x = hi.masked_x(new)
    ref = hi.reference(new, x)
    b = hi.bounds(hi.yardstick(new, x, ref))
    fresh = hi.score(hi.twin(new, x), ref)
    stale = hi.score(hi.twin(new, x, sw=st["sw"]), ref)
    assert all(fresh[q] <= b[q] for q in hi.QUANTITIES), fresh
    assert stale["product"] > 100.0 * b["product"] and stale["switch_product"] > 100.0 * b["switch_product"], stale


def test_retraction_reference_and_both_sides_of_the_small_angle_branch():
    """normalize(q (x) Exp(dw)) at 50 digits without a small-angle branch, against oracle_pgo.Graph.retract (the yardstick
    of the GPU test) on the step of the direct sparse solve of the retraction graph — and that graph puts at least 8
    rotation steps just below |dw| = 1e-6 and 8 at or just above it."""
    st = hi.retraction_graph()
    n = st["poses"].shape[0]
    g = hi.oracle_graph(st)
    H, grad, _ = g.linearize()
    step = g.solve_step(H, grad, hi.RETRACT_LAMBDA)
    dw = hi.rotation_steps(n, step)
    below, above = hi.branch_counts(dw)
    assert below >= 8 and above >= 8, (below, above)
    th = np.linalg.norm(dw[1::2], axis=1)
    assert np.min(th) < 1e-11 and np.max(th) > 1.0 and np.all(dw[0::2] == 0.0)
    poses, sw = hi.oracle_retract(st, step)
    free = st["fixed"] == 0
    xp = hi.retract_xp(st["poses"][free, 3:], dw[free])
    err = hi.quaternion_error_eps(poses[free, 3:], xp)
    assert err <= 8.0, err                                    # 1.7 on this graph
    assert hi.norm_error_eps(poses[free, 3:]) <= 4.0
    assert np.array_equal(poses[~free], st["poses"][~free])
    # the measure bites: the first-order exponential WITHOUT the renormalisation is far off at |dw| ~ 1
    k = int(np.argmax(th))
    q = st["poses"][2 * k + 1, 3:]
    lazy = op.qmul(q, np.array([1.0, *(0.5 * dw[2 * k + 1])]))
    assert hi.quaternion_error_eps(lazy[None], hi.retract_xp(q[None], dw[2 * k + 1][None])) > 1e10
