"""nos_pgo_set_loss at the C ABI (include/nos.h): what it refuses, that a refused call leaves the graph's loss as it was, and
nos_pgo_get_vector(3) on a graph without information.  Inputs: tests/pgo_robust_inputs.py."""
import ctypes

import numpy as np
import pytest

from tests import pgo_hard_inputs as hi
from tests import pgo_info_inputs as pi
from tests import pgo_robust_inputs as ri

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED = 0, 1, 6
NONE, EXPONENTIAL, HUBER = 0, 1, 2


def _set_loss(ctx, g, kind, a=0.0, b=0.0, flags=None):
    from nonlinear_optimizer_for_slam_amd import _lib
    loss = _lib.NosLoss(kind, 0, a, b)
    return ctx._lib.nos_pgo_set_loss(g._h, ctypes.byref(loss), flags)


REFUSED = [(7, 1.0, 1.0), (-1, 1.0, 1.0), (3, 0.0, 0.0),
           (HUBER, 0.0, 0.0), (HUBER, -1.0, 0.0), (HUBER, float("nan"), 0.0), (HUBER, float("inf"), 0.0),
           (EXPONENTIAL, -1.0, 1.0), (EXPONENTIAL, 1.0, -1.0), (EXPONENTIAL, float("nan"), 1.0),
           (EXPONENTIAL, 1.0, float("nan")), (EXPONENTIAL, float("inf"), 1.0), (EXPONENTIAL, 1.0, float("-inf"))]


@pytest.mark.parametrize("before", (None, "huber", "exponential"))
def test_a_refused_loss_leaves_the_graph_as_it_was(ctx, before):
    """an unknown kind; a Huber threshold that is not finite or <= 0; exponential c1 or c2 not finite or < 0:
    NOS_ERR_INVALID_ARGUMENT, and the next linearisation is bit for bit the one before — with no loss, and with either kind
    set (flags included)"""
    name = "two_groups"
    st = pi.case(name)
    x = hi.masked_x(st)
    flags = ri.third_flags(name)
    g = ri.gpu_graph(ctx, st, None if before is None else ri.case_loss(name, before), robust=None if before is None else flags)
    want, want_gnorm = ri.gpu_quantities(g, st, x)
    for kind, a, b in REFUSED:
        assert _set_loss(ctx, g, kind, a, b) == INVALID, (kind, a, b)
        assert _set_loss(ctx, g, kind, a, b, bytes(st["ref"].size)) == INVALID, (kind, a, b)
    got, gnorm = ri.gpu_quantities(g, st, x)
    g.close()
    assert gnorm == want_gnorm and np.array_equal(got["weights"], want["weights"])
    for q in ("cost", "gradient", "switch_gradient", "hdiag"):
        assert np.array_equal(np.asarray(got[q]), np.asarray(want[q])), q
    for lam in ri.LAMBDAS:
        assert np.array_equal(got["product"][lam], want["product"][lam])
        assert np.array_equal(got["switch_product"][lam], want["switch_product"][lam])
    if before is None:
        assert np.array_equal(got["weights"], np.ones(st["ref"].size))
    else:
        assert np.all(got["weights"][flags == 0] == 1.0) and got["weights"].min() < 1.0


def test_what_is_accepted(ctx):
    """NULL and kind NONE remove the loss; zero c1 or c2 are allowed (the reference's constructor takes them)"""
    st = pi.case("chain13")
    g = pi.gpu_graph(ctx, st)
    assert ctx._lib.nos_pgo_set_loss(g._h, None, None) == OK
    assert _set_loss(ctx, g, NONE, float("nan"), -1.0) == OK          # the parameters of no loss are not read
    assert _set_loss(ctx, g, EXPONENTIAL, 0.0, 0.0) == OK
    assert _set_loss(ctx, g, HUBER, 1e-300) == OK and _set_loss(ctx, g, HUBER, 1e300) == OK
    assert ctx._lib.nos_pgo_set_loss(None, None, None) == INVALID
    g.close()


def test_a_graph_without_information_takes_no_loss(ctx):
    """NOS_ERR_UNSUPPORTED, the message says what to do; removing the loss is fine; the weights are all ones; the graph
    computes what it computed before"""
    from nonlinear_optimizer_for_slam_amd import _lib
    st = pi.case("two_groups")
    g = pi.gpu_graph(ctx, st, information=None)
    before = g.linearize()
    grad = g.vector("gradient")
    for kind, a, b in ((HUBER, 1.0, 0.0), (EXPONENTIAL, 1.0, 1.0)):
        assert _set_loss(ctx, g, kind, a, b) == UNSUPPORTED
        assert "identity" in ctx._lib.nos_last_error().decode()
    assert _set_loss(ctx, g, 7, 1.0, 1.0) == INVALID
    assert _set_loss(ctx, g, NONE) == OK and ctx._lib.nos_pgo_set_loss(g._h, None, None) == OK
    with pytest.raises(_lib.NosError) as err:
        g.set_loss(("huber", 1.0))
    assert err.value.status == UNSUPPORTED
    assert np.array_equal(g.edge_weights(), np.ones(st["ref"].size))
    assert g.linearize() == before and np.array_equal(g.vector("gradient"), grad)
    assert np.array_equal(g.edge_weights(), np.ones(st["ref"].size))
    g.close()


def test_a_loss_without_information_passes_identity_matrices(ctx):
    """PoseGraph(..., loss=...) with information=None is the graph with identity matrices"""
    from nonlinear_optimizer_for_slam_amd import pgo
    st = pi.case("chain13")
    loss = ("huber", 0.05)
    args = (ctx, st["poses"], st["ref"], st["qry"], st["meas"], st["sw"], st["free"], st["fixed"])
    a = pgo.PoseGraph(*args, loss=loss)
    b = pgo.PoseGraph(*args, information=np.broadcast_to(np.eye(6), (15, 6, 6)), loss=loss)
    assert a.linearize() == b.linearize()
    assert np.array_equal(a.vector("gradient"), b.vector("gradient"))
    assert np.array_equal(a.edge_weights(), b.edge_weights()) and a.edge_weights().min() < 1.0
    a.close()
    b.close()
