"""The first LM step of every real loop form on exactly known sums (tests/exact_inputs.py): with max_iterations = 1 and both
tolerances 0 the pose a solve returns must EQUAL, bit for bit, the pose the step hook nos_debug_lm_step gives on the exact
sums from the start state, and so must final_lambda and iterations — whichever form ran the loop: the stand-alone step
kernel, the fused finish of the launch-per-pass loop, the single workgroup, the resident cluster, the streamed one-launch
loop, a row of a batched solve.  tests/test_exact_sums_gpu.py pins the first COST of these forms; tests/test_lm_step_xprec.py
holds the hook's step against 60 digits; this ties the two together, so that the bit-for-bit chains between the forms hang
from an anchored end.

Every size is derived from the library's sources (exact_inputs.library_constants); each case asserts which form ran.
"""
import ctypes

import numpy as np
import pytest

from nonlinear_optimizer_for_slam_amd import NdtDataset, ReprojDataset, _lib
from nonlinear_optimizer_for_slam_amd.api import reproj_solve_batch, solve3_batch, solve6_batch
from tests import exact_inputs as X
from tests import lm_step_inputs as L

pytestmark = pytest.mark.gpu

ES = {"f64": 8, "f32": 4}
K = X.library_constants()
DP = ctypes.POINTER(ctypes.c_double)
ONE_STEP = dict(max_iterations=1, gradient_tolerance=0.0, parameter_tolerance=0.0)


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def hook_step(ctx, dof, sums, R, t):
    """The state LmInit6 / LmInit3 makes of (R, t) — q = QuatFromMatrix(R) restated in numpy: for a signed permutation
    square roots of 1, 2 and 4 and halvings — after one step of the hook on `sums` → (R', t', λ', iterations, ok)."""
    state = L.make_state(dof, q=L.quat_from_matrix(R) if dof == 6 else None)
    if dof == 6:
        assert np.array_equal(state[:9], np.asarray(R, dtype=np.float64).reshape(9))  # R → q → R is exact here
    else:
        state[:4] = np.asarray(R, dtype=np.float64).reshape(4)
    state[9:9 + len(t)] = t
    settings = np.array([1.0, 0.0, 0.0, 0.0])
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    rc = _lib.hip_lib().nos_debug_lm_step(ctx._h, dof, sums.ctypes.data_as(DP), settings.ctypes.data_as(DP), state.ctypes.data_as(DP))
    assert rc == 0
    nr, nt = (9, 3) if dof == 6 else (4, 2)
    return state[:nr].copy(), state[9:9 + nt].copy(), state[L.I_LAMBDA], int(state[L.I_ITER]), bool(state[L.I_OK])


def _same(got, want, what):
    """(R, t, report) of a solve against hook_step's result: the same bits."""
    R, t, rep = got
    wR, wt, wl, wi, wok = want
    assert np.asarray(R).reshape(-1).tobytes() == wR.tobytes(), (what, R, wR)
    assert np.asarray(t).reshape(-1).tobytes() == wt.tobytes(), (what, t, wt)
    assert rep["final_lambda"] == wl and rep["iterations"] == wi and rep["ok"] == wok, (what, rep, want)


class Problem:
    """One exact dataset on the device with its three solves (those its kind has) and the hook's answers."""

    def __init__(self, ctx, kind, n, dtype, cus, seed):
        self.kind, self.n, self.dtype, self.ctx = kind, n, dtype, ctx
        if kind == "ndt":
            self.case = X.ndt_case(n, dtype, cus=cus, seed=seed)
            self.ds = NdtDataset.from_planes(ctx, self.case.planes, dtype)
        else:
            self.case = X.reproj_case(n, dtype, cus=cus, seed=seed)
            self.ds = ReprojDataset.from_planes(ctx, self.case.planes, dtype)

    def solves(self):
        """→ [(name, kernel's problem, planes, solve(), hook's answer)]"""
        c, ds = self.case, self.ds
        if self.kind == "ndt":
            return [("solve6", "Ndt6Problem", 15, lambda: ds.solve6(c.R, c.t, None, **ONE_STEP),
                     hook_step(self.ctx, 6, c.want6, c.R, c.t)),
                    ("solve3", "Ndt3Problem", 15, lambda: ds.solve3(c.R2, c.t2, None, **ONE_STEP),
                     hook_step(self.ctx, 3, c.want3, c.R2, c.t2))]
        return [("reproj", "ReprojProblem", 5,
                 lambda: ds.solve(c.R, c.t, X.REPROJ_INTR, None, X.REPROJ_MIN_DEPTH, **ONE_STEP),
                 hook_step(self.ctx, 6, c.want, c.R, c.t))]

    def close(self):
        self.ds.close()


def _form(ctx, n, planes, dtype, cus):
    """The form the solve that just ran took, read from its kernel's name, checked against the launch rule."""
    name = ctx.last_kernel()
    want = X.solve_items_per_lane(n, planes, ES[dtype], K, cus)[0]
    if "solve_single_block_kernel<" in name:
        got = "single"
    elif "solve_cluster_kernel<" in name:
        got = "streamed" if X.cluster_geometry(name)["SI"] > 0 else "resident"
    else:
        got = "pass"
    return got, want


KINDS = [("ndt", "f64"), ("ndt", "f32"), ("reproj", "f64"), ("reproj", "f32")]


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_first_step_of_the_launch_per_pass_loop_equals_the_hook(ctx, cus, kind, dtype):
    """One launch per pass over several workgroups: the step in the stand-alone one-wave kernel (lm_fused = 0) and in the
    workgroup that finishes the reduction."""
    p = Problem(ctx, kind, 5003, dtype, cus, seed=11)
    for name, _, planes, solve, want in p.solves():
        assert want[4] and want[3] == 1
        for fused in (0, 1):
            with ctx.options(lm_single=0, lm_cluster=0, lm_fused=fused):
                got = solve()
                assert _form(ctx, p.n, planes, dtype, cus)[0] == "pass", ctx.last_kernel()
            _same(got, want, "%s %s lm_fused=%d" % (name, dtype, fused))
    p.close()


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_first_step_of_the_single_workgroup_solve_equals_the_hook(ctx, cus, kind, dtype):
    p = Problem(ctx, kind, 257, dtype, cus, seed=12)
    for name, _, planes, solve, want in p.solves():
        got = solve()
        assert _form(ctx, p.n, planes, dtype, cus) == ("single", "single"), ctx.last_kernel()
        _same(got, want, "%s %s single workgroup" % (name, dtype))
    p.close()


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_first_step_of_the_resident_cluster_solve_equals_the_hook(ctx, cus, kind, dtype):
    """The smallest n beyond the single workgroup: the resident one-launch loop, its all-reduce through the XCD's L2
    (default), through sc1 stores (lm_cluster = 5) and as the resident-only form (lm_cluster = 4)."""
    planes = 15 if kind == "ndt" else 5
    p = Problem(ctx, kind, K["single_block_max_elements"] // planes + 1, dtype, cus, seed=13)
    for name, _, planes, solve, want in p.solves():
        for cluster in (1, 5, 4):
            with ctx.options(lm_cluster=cluster):
                got = solve()
                assert _form(ctx, p.n, planes, dtype, cus) == ("resident", "resident"), ctx.last_kernel()
            assert got[2]["launches"] == 1 and not got[2]["fallback"], got[2]
            _same(got, want, "%s %s lm_cluster=%d" % (name, dtype, cluster))
    p.close()


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_first_step_of_the_streamed_solve_equals_the_hook(ctx, cus, kind, dtype):
    """The smallest n the chip cannot keep resident: the one-launch loop streams it."""
    planes = 15 if kind == "ndt" else 5
    n = K["resident"][(planes, ES[dtype])] * K["solve_block"] * min(K["cluster_max_blocks"], cus) + 1
    p = Problem(ctx, kind, n, dtype, cus, seed=14)
    for name, _, planes, solve, want in p.solves():
        got = solve()
        assert _form(ctx, p.n, planes, dtype, cus) == ("streamed", "streamed"), ctx.last_kernel()
        assert got[2]["launches"] == 1 and not got[2]["fallback"], got[2]
        _same(got, want, "%s %s streamed" % (name, dtype))
    p.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_first_step_of_a_batched_solve_equals_the_hook_row_by_row(ctx, cus, dtype):
    ps = [Problem(ctx, "ndt", n, dtype, cus, seed=20 + n) for n in (257, 65)]
    cs = [p.case for p in ps]
    R, t, reps = solve6_batch([p.ds for p in ps], [c.R for c in cs], [c.t for c in cs], None, **ONE_STEP)
    for i, c in enumerate(cs):
        _same((R[i], t[i], reps[i]), hook_step(ctx, 6, c.want6, c.R, c.t), "solve6_batch row %d %s" % (i, dtype))
    R, t, reps = solve3_batch([p.ds for p in ps], [c.R2 for c in cs], [c.t2 for c in cs], None, **ONE_STEP)
    for i, c in enumerate(cs):
        _same((R[i], t[i], reps[i]), hook_step(ctx, 3, c.want3, c.R2, c.t2), "solve3_batch row %d %s" % (i, dtype))
    for p in ps:
        p.close()
    ps = [Problem(ctx, "reproj", n, dtype, cus, seed=30 + n) for n in (257, 65)]
    cs = [p.case for p in ps]
    R, t, reps = reproj_solve_batch([p.ds for p in ps], [c.R for c in cs], [c.t for c in cs], X.REPROJ_INTR, None,
                                    X.REPROJ_MIN_DEPTH, **ONE_STEP)
    for i, c in enumerate(cs):
        _same((R[i], t[i], reps[i]), hook_step(ctx, 6, c.want, c.R, c.t), "reproj_solve_batch row %d %s" % (i, dtype))
    for p in ps:
        p.close()


# ---------------------------------------------------------------- hand-made datasets of one, two and three items

def _item(p, mu, S):
    return list(p) + list(mu) + [v for row in S for v in row]


TINY = {  # n: items (p, mu, upper-triangular S), integers
    1: [_item((1, 2, -1), (0, 1, 1), ((2, 1, 0), (0, 1, -1), (0, 0, 3)))],
    2: [_item((1, 2, -1), (0, 1, 1), ((2, 1, 0), (0, 1, -1), (0, 0, 3))),       # the same point twice: rank 3 (planar: 2)
        _item((1, 2, -1), (2, 0, -1), ((1, 0, 2), (0, 2, 1), (0, 0, 1)))],
    3: [_item((1, 2, -1), (0, 1, 1), ((2, 1, 0), (0, 1, -1), (0, 0, 3))),       # three points on one line: rank 5
        _item((2, 3, 1), (2, 0, -1), ((1, 0, 2), (0, 2, 1), (0, 0, 1))),
        _item((3, 4, 3), (1, 1, 0), ((3, -1, 1), (0, 1, 0), (0, 0, 2)))],
}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_first_step_on_one_two_and_three_items_equals_the_hook(ctx, cus, dtype):
    """Rank-deficient H saved by the damping alone, through the lone solve and the batch; one item at p = 0 gives a zero
    rotation block: the solve is refused and the pose comes back untouched, lone and batched."""
    R, R2 = X.signed_permutation(5).astype(np.float64), X.signed_permutation(6, 2).astype(np.float64)
    t, t2 = np.array([1.0, -2.0, 1.0]), np.array([-1.0, 2.0])
    sets = []
    for n, items in TINY.items():
        planes = np.array(items, dtype=np.float64).T.copy()
        want6, want3 = X.ndt_sums_of_planes(planes, R, t, R2, t2, dtype, cus)
        H6, H3 = L.unpack_sums(6, want6)[0], L.unpack_sums(3, want3)[0]
        assert np.linalg.matrix_rank(H6) < 6 and np.all(np.diag(H6) > 0) and np.all(np.diag(H3) > 0)
        assert n == 3 or np.linalg.matrix_rank(H3) < 3
        sets.append((NdtDataset.from_planes(ctx, planes, dtype), want6, want3))
    for ds, want6, want3 in sets:
        _same(ds.solve6(R, t, None, **ONE_STEP), hook_step(ctx, 6, want6, R, t), "solve6 n=%d %s" % (len(ds), dtype))
        _same(ds.solve3(R2, t2, None, **ONE_STEP), hook_step(ctx, 3, want3, R2, t2), "solve3 n=%d %s" % (len(ds), dtype))
    B = len(sets)
    Rb, tb, reps = solve6_batch([s[0] for s in sets], [R] * B, [t] * B, None, **ONE_STEP)
    for i, (ds, want6, _) in enumerate(sets):
        _same((Rb[i], tb[i], reps[i]), hook_step(ctx, 6, want6, R, t), "solve6_batch n=%d %s" % (len(ds), dtype))
    Rb, tb, reps = solve3_batch([s[0] for s in sets], [R2] * B, [t2] * B, None, **ONE_STEP)
    for i, (ds, _, want3) in enumerate(sets):
        _same((Rb[i], tb[i], reps[i]), hook_step(ctx, 3, want3, R2, t2), "solve3_batch n=%d %s" % (len(ds), dtype))
    # one item at the origin: no rotation is observed
    planes = np.array([_item((0, 0, 0), (1, -1, 2), ((2, 1, 0), (0, 1, -1), (0, 0, 3)))], dtype=np.float64).T.copy()
    want6, want3 = X.ndt_sums_of_planes(planes, R, t, R2, t2, dtype, cus)
    assert not np.any(L.unpack_sums(6, want6)[0][3:, 3:]) and L.unpack_sums(3, want3)[0][2, 2] == 0
    zero = NdtDataset.from_planes(ctx, planes, dtype)
    lone6, lone3 = zero.solve6(R, t, None, **ONE_STEP), zero.solve3(R2, t2, None, **ONE_STEP)
    Rb, tb, reps = solve6_batch([zero, sets[0][0]], [R, R], [t, t], None, **ONE_STEP)
    Rc, tc, repc = solve3_batch([zero, sets[0][0]], [R2, R2], [t2, t2], None, **ONE_STEP)
    for what, (gR, gt, rep), (wR, wt) in (("solve6", lone6, (R, t)), ("solve3", lone3, (R2, t2)),
                                          ("solve6_batch", (Rb[0], tb[0], reps[0]), (R, t)),
                                          ("solve3_batch", (Rc[0], tc[0], repc[0]), (R2, t2))):
        assert rep["ok"] is False and rep["iterations"] == 0, (what, rep)
        assert np.array_equal(np.asarray(gR).reshape(-1), wR.reshape(-1)) and np.array_equal(np.asarray(gt).reshape(-1), wt), what
    _same((Rb[1], tb[1], reps[1]), hook_step(ctx, 6, sets[0][1], R, t), "solve6_batch beside a refused row " + dtype)
    for ds, _, _ in sets:
        ds.close()
    zero.close()
