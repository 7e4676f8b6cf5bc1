"""Every entry point gives the same bits whatever its device memory held before the call (debug_alloc_fill).

The pool hands back parked blocks as they were left, every arena carves a dozen temporaries out of one slab, and many
kernels leave a precondition ("zeroed by the caller", an empty table, tickets at 0, the +0 of an absent slot) to the host: a
missing initialisation passes whenever the block happens to be fresh or to hold harmless leftovers, and which it is
depends on the tests that ran before.  Here every block starts as a chosen word instead.

Each case of tests/alloc_fill_cases.py runs on one context under the fills Z (zeros, twice), A (the word 0x00000001), N
(the word 0x7FC00001: a quiet NaN as a float, and a finite 2^1021 as a double) and D (the word 0x7FF80001: a quiet NaN in
either float width), in this order inside ONE test function: the two zero-filled runs must agree bit for bit, and so must
A, N and D with them.  N and D run only after A has passed — a failing A assertion stops the test — because a leftover
read as an index is harmless under A (it stays inside any array of two elements) and a finding under A is fixed before
that case ever runs under N or D.  Every case also shows, by the context's debug_alloc_filled counter,
that the hook acted on it, and its zero-filled run is held to an independent reference (the CPU oracle, the place rule in
numpy, the voxel store's model, brute-force neighbours, the lone solve of a batch row) with that reference's own
tolerance."""
import time

import pytest

from tests import alloc_fill_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fill_ctx():
    """a context of this module's own: the option never reaches another test's calls"""
    from nonlinear_optimizer_for_slam_amd import Context
    c = Context((0,))
    yield c
    c.close()


def test_the_options_are_range_checked_and_count(fill_ctx):
    """debug_alloc_fill takes -1 … 0x7FFFFFFF, debug_alloc_filled only its reset; off fills nothing, on fills every block
    of a call and is counted; both read back"""
    import numpy as np
    from nonlinear_optimizer_for_slam_amd import _lib
    from nonlinear_optimizer_for_slam_amd.api import Scan
    ctx = fill_ctx
    assert ctx.get_option("debug_alloc_fill") == 0 and ctx.get_option("debug_alloc_filled") == 0
    for key, bad in (("debug_alloc_fill", -2), ("debug_alloc_filled", 1), ("debug_alloc_filled", -1)):
        with pytest.raises(_lib.NosError) as err:
            ctx.set_option(key, bad)
        assert err.value.status == 1, key
    Scan(ctx, np.zeros((5, 3))).close()
    assert ctx.get_option("debug_alloc_filled") == 0  # off
    for word in (cases.FILL_ZERO, cases.FILL_ONE, cases.FILL_NAN, cases.FILL_NAN64, 0x7FFFFFFF):
        with ctx.options(debug_alloc_fill=word):
            assert ctx.get_option("debug_alloc_fill") == word
            ctx.set_option("debug_alloc_filled", 0)
            Scan(ctx, np.zeros((5, 3))).close()
            assert ctx.get_option("debug_alloc_filled") == 2  # the scan's planes and the staging of its upload
    assert ctx.get_option("debug_alloc_fill") == 0
    ctx.set_option("debug_alloc_filled", 0)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_result_does_not_depend_on_what_device_memory_held(fill_ctx, oracle, name):
    started = time.perf_counter()
    values, filled = cases.check_case(fill_ctx, name, oracle)
    print("%s: %d values, %d blocks filled in the last run, %.2f s" % (name, values, filled, time.perf_counter() - started))


def test_every_case_is_listed_once():
    assert not set(cases.NO_DEVICE_ALLOCATION) - set(cases.CASES)
    assert all(isinstance(reason, str) and reason for reason in cases.NO_DEVICE_ALLOCATION.values())
