"""The LM step — damped solve, pose update, convergence tests, λ schedule — of the host loop (nos_host_lm_advance, CPU) and
of every device loop form (lm_step_lane through the hook nos_debug_lm_step, gpu) against a 60-digit reference, at the sums
and states where such a step goes wrong: condition numbers up to 1e15, exactly singular H saved by the damping alone,
systems that must be refused, angles on both sides of every switch of the exponential map, norms within 2^-48 of their
tolerance and beyond the range of their squares, non-finite sums, and 256 steps in a row.  Cases, reference, yardstick and
the error measures: tests/lm_step_inputs.py.

The bounds are 4 x what the plain numpy float64 statement of the same step (numpy_step) loses on the same family
(this project's convention for a restatement yardstick), the decisions must EQUAL the reference's.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import lm_step_inputs as L

DP = ctypes.POINTER(ctypes.c_double)
SIDES = ["host", pytest.param("device", marks=pytest.mark.gpu)]


@functools.lru_cache(maxsize=None)
def _host_lib():
    from nonlinear_optimizer_for_slam_amd import _lib
    host = ctypes.CDLL(_lib.LIB_HOST)
    host.nos_host_lm_advance.argtypes = [ctypes.c_int, DP, DP, DP]
    return host


@pytest.fixture
def step(request):
    """side → function(dof, sums, settings, state) → the state after one step; the device's needs the session's context."""
    def get(side):
        if side == "host":
            host = _host_lib()

            def run(dof, sums, settings, state):
                out = np.array(state, dtype=np.float64)
                assert host.nos_host_lm_advance(dof, sums.ctypes.data_as(DP), settings.ctypes.data_as(DP), out.ctypes.data_as(DP)) == 0
                return out
            return run
        from nonlinear_optimizer_for_slam_amd import _lib
        ctx = request.getfixturevalue("ctx")
        hip = _lib.hip_lib()

        def run(dof, sums, settings, state):
            out = np.array(state, dtype=np.float64)
            assert hip.nos_debug_lm_step(ctx._h, dof, sums.ctypes.data_as(DP), settings.ctypes.data_as(DP), out.ctypes.data_as(DP)) == 0
            return out
        return run
    return get


_OUT = {}


def outputs(side, family, step):
    """The states after the step of every case of a family, computed once per side."""
    if (side, family) not in _OUT:
        if side == "numpy":
            _OUT[side, family] = [L.numpy_step(c.dof, c.sums, c.settings, c.state) for c in L.cases(family)]
        else:
            run = step(side)
            _OUT[side, family] = [run(c.dof, c.sums, c.settings, c.state) for c in L.cases(family)]
    return _OUT[side, family]


def _pose_cases(pool):
    """The cases whose pose is held to the pose bound: the angle ladder (also alone: its rungs up to half a radian, where
    the angle's own rounding is not yet magnified), and the cond ladder up to κ = 1e4."""
    family = POOLS[pool]
    keep = {"angle_ladder": lambda c: True, "angle_ladder_small": lambda c: c.want_theta <= 0.5,
            "cond_ladder": lambda c: c.ref["kappa"] <= 1e4}[pool]
    return [k for k, c in enumerate(L.cases(family)) if keep(c)]


POOLS = {"angle_ladder": "angle_ladder", "angle_ladder_small": "angle_ladder", "cond_ladder": "cond_ladder"}


def _worst_pose(side, pool, step):
    worst = {}
    got = outputs(side, POOLS[pool], step)
    cs = L.cases(POOLS[pool])
    for k in _pose_cases(pool):
        for name, v in L.pose_errors(cs[k].dof, got[k], cs[k].ref).items():
            if v >= worst.get(name, (-1.0, None))[0]:
                worst[name] = (v, cs[k])
    return worst


# ---------------------------------------------------------------- generators and coverage (CPU)

def test_every_family_has_its_cases_margins_and_branches():
    """The generators' own assertions (sizes, both dof, decision margins, refusal margins, the side of every angle
    switch) hold, and — counted from the reference's values, not hoped for — every branch of the step is taken at least
    ten times."""
    count = dict.fromkeys(("series", "sincos", "tiny", "planar_series", "planar_sincos", "refused", "up", "down", "clamp_lo",
                           "clamp_hi", "float_applied", "budget_end", "converged"), 0)
    lambdas, schedules = set(), set()
    for c in L.all_cases():
        if c.ref["branch"] in count:
            count[c.ref["branch"]] += 1
        for key in ("up", "down", "clamp_lo", "clamp_hi", "float_applied", "budget_end", "converged"):
            count[key] += int(c.ref[key])
        lambdas.add(float(np.float32(c.state[L.I_LAMBDA])))
        schedules.add(int(c.settings[3]))
    assert all(v >= 10 for v in count.values()), count
    assert lambdas == {float(np.float32(v)) for v in L.LAMBDAS} and schedules == {0, 1}
    kappas = [float(c.ref["kappa"]) for c in L.cases("cond_ladder")]
    assert min(kappas) < 1.001 and max(kappas) > 1e14
    kappas = [float(c.ref["kappa"]) for c in L.cases("rank_deficient")]
    assert max(kappas) > 1e7
    assert max(float(c.ref["theta"]) for c in L.cases("angle_ladder")) > 39.0


# ---------------------------------------------------------------- solve accuracy

@pytest.mark.parametrize("family", L.SOLVE_FAMILIES)
@pytest.mark.parametrize("side", SIDES)
def test_damped_solve_stays_within_four_times_the_numpy_solve(step, side, family):
    """e = ‖δ − δ*‖ / ‖δ*‖ / (eps κ₂), δ read back from the pose after the step (identity start, t = 0): the worst e of the
    side is at most 4 x the worst e of np.linalg.solve on the family, and no solve of these families is refused.

    Measured (worst e; cond_ladder / rank_deficient): numpy 0.94 / 0.22, host 0.70 / 0.25, device 1.08 / 0.18."""
    cs = L.cases(family)
    got = outputs(side, family, step)
    assert all(g[L.I_OK] == 1 for g in got), [c for c, g in zip(cs, got) if g[L.I_OK] != 1][:5]
    yard = max(L.solve_error(c.dof, g, c.ref) for c, g in zip(cs, outputs("numpy", family, step)))
    errs = [L.solve_error(c.dof, g, c.ref) for c, g in zip(cs, got)]
    worst = int(np.argmax(errs))
    print("solve accuracy %s %s: worst e = %.3f (%r, kappa %.3g), numpy %.3f" %
          (family, side, errs[worst], cs[worst], float(cs[worst].ref["kappa"]), yard))
    assert errs[worst] <= 4.0 * yard, (cs[worst], errs[worst], yard)


# ---------------------------------------------------------------- pose accuracy

@pytest.mark.parametrize("pool", list(POOLS))
@pytest.mark.parametrize("side", SIDES)
def test_pose_after_the_step_stays_within_four_times_the_numpy_pose(step, side, pool):
    """max |q − q*|, max |R − R*|, |t − t*| / (|t*| + |δ*|) and ||q| − 1|, in eps, over the angle ladder and the κ ≤ 1e4
    part of the cond ladder: each at most 4 x the pool's worst of numpy_step, with a floor of 2 eps.  The angle ladder's worst
    is set by its 40 rad rung, where the last bit of δ itself moves q by 10 eps; its rungs up to 0.5 rad are therefore also
    held to their own, much smaller, yardstick.

    Measured, worst in eps (q / R / t / unit):
      angle ladder           numpy 9.6 / 22.9 / 0.44 / 0.95   host 9.6 / 25.3 / 0.44 / 0.99   device 9.6 / 25.3 / 0.44 / 0.86
      its rungs ≤ 0.5 rad    numpy 0.95 / 2.5 / 0.44 / 0.95   host 0.99 / 3.6 / 0.44 / 0.99   device 0.68 / 2.7 / 0.44 / 0.86
      cond ladder, κ ≤ 1e4   numpy 82 / 170 / 452 / 0.59      host 65 / 156 / 569 / 0.87      device 43 / 88 / 275 / 0.23"""
    yard = _worst_pose("numpy", pool, step)
    got = _worst_pose(side, pool, step)
    print("pose accuracy %s %s: %s | numpy %s" % (pool, side, {k: round(v[0], 3) for k, v in got.items()},
                                                 {k: round(v[0], 3) for k, v in yard.items()}))
    assert len(_pose_cases(pool)) >= 50
    for name, (v, case) in got.items():
        assert v <= max(4.0 * yard[name][0], 2.0), (name, case, v, yard[name][0])


# ---------------------------------------------------------------- decisions

@pytest.mark.parametrize("family", list(L.FAMILIES))
@pytest.mark.parametrize("side", SIDES)
def test_decisions_equal_the_references(step, side, family):
    """λ, previous_cost, cost, iteration, done and ok after the step equal the reference's, case by case; a refused solve
    leaves the pose, λ, the previous cost and the iteration as they were and stores the cost."""
    bad = []
    for c, g in zip(L.cases(family), outputs(side, family, step)):
        if not np.array_equal(g[16:22], L.decisions(c.ref), equal_nan=True):
            bad.append((c, g[16:22].tolist(), L.decisions(c.ref).tolist()))
        if c.ref["ok"] == 0:
            assert g[L.I_OK] == 0 and g[L.I_DONE] == 1, c
            assert g[:18].tobytes() == c.state[:18].tobytes() and g[L.I_ITER] == c.state[L.I_ITER], c
            assert np.array_equal(g[L.I_COST], c.sums[-1], equal_nan=True), c
    assert not bad, (len(bad), bad[:6])
    if family == "must_refuse":
        assert all(c.ref["ok"] == 0 for c in L.cases(family))


# ---------------------------------------------------------------- chain

@functools.lru_cache(maxsize=None)
def _chain_reference(dof):
    return L.reference_chain(dof)


def _run_chain(dof, run):
    """→ (worst ||q| − 1|, worst ‖RᵀR − I‖_max over the 256 steps, final state); the decisions are checked on the way."""
    st, settings, sums = L.chain(dof)
    refs = _chain_reference(dof)
    unit = orth = 0.0
    for s, ref in zip(sums, refs):
        st = run(dof, s, settings, st)
        assert np.array_equal(st[16:22], L.decisions(ref)), (st[16:22], L.decisions(ref))
        u, o = L.drift_errors(dof, st)
        unit, orth = max(unit, u), max(orth, o)
    return unit, orth, st


def _final_error(dof, st, ref):
    e = L.pose_errors(dof, st, ref)
    return max(e["R"], e.get("q", 0.0), e["t"])


@pytest.mark.parametrize("dof", [6, 3])
@pytest.mark.parametrize("side", SIDES)
def test_256_steps_in_a_row_do_not_drift(step, side, dof):
    """Each step's output state feeds the next, rotation increments of 0.01 – 0.3 rad.  After every step ||q| − 1| and
    ‖RᵀR − I‖_max stay within 4 x the worst of the numpy chain (floor 2 eps), and the final pose is within 4 x the numpy
    chain's own distance from the 60-digit chain.

    Measured (eps; unit / orthogonality / final pose): 6-DoF numpy 0.79 / 4.1 / 26.6, host 1.07 / 6.5 / 16.2, device
    0.78 / 3.8 / 21.6; planar (no q) numpy 19.6 / 9.6, host 15.2 / 6.7, device 8.3 / 4.2."""
    final_ref = _chain_reference(dof)[-1]
    yu, yo, yst = _run_chain(dof, L.numpy_step)
    u, o, st = _run_chain(dof, step(side))
    yf, f = _final_error(dof, yst, final_ref), _final_error(dof, st, final_ref)
    print("chain %d-DoF %s: unit %.3f orth %.3f final %.3f | numpy unit %.3f orth %.3f final %.3f" % (dof, side, u, o, f, yu, yo, yf))
    assert u <= max(4.0 * yu, 2.0) and o <= max(4.0 * yo, 2.0), (u, o, yu, yo)
    assert f <= 4.0 * yf, (f, yf)
