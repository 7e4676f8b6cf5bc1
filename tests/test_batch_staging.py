"""The three kinds of batched call — score_batch, register6_batch, solve6_batch — stage their memory through ONE pinned
block per device slot and one piece of code (BatchTrip, csrc/batch_host.hpp).  The block only grows, so a
call may find it smaller than it needs, or larger and still holding another call's descriptors, results or cost history.

One fresh context runs, in this order: a score (B = 1, staging of a few hundred bytes), a registration (B = 4, larger: the
round log), a batched solve (B = 64, max_iterations = 100: the largest, about 50 KB of cost history), one call that fails
validation, then the same calls in reverse order, each now into a block larger than it needs.  The score and the
registration run against an NdtMap and against a VoxelMap.

The calls are deterministic and do not depend on what ran before them, so every repeated call must give its first result
bit for bit — poses, reports, round logs, cost histories, score rows — and the first results must be those of the same
calls on a second, fresh context.  Equality is the condition: there is no tolerance."""
import ctypes

import numpy as np
import pytest

from tests import helpers

pytestmark = pytest.mark.gpu

EXP = ("exponential", 1.0, 1.0)
LO, HI = np.array([-5.0, -5.0, -1.5]), np.array([5.0, 5.0, 1.5])
INVALID = 1


def _freeze(x):
    """A result as something == compares bit for bit (a NaN equals itself, -0.0 differs from 0.0)."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, float):
        return x.hex()
    if isinstance(x, dict):
        return tuple((k, _freeze(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_freeze(v) for v in x)
    return x


class _Scene:
    """Everything the calls need, made on one context from seeds alone."""

    def __init__(self, ctx):
        from nonlinear_optimizer_for_slam_amd import api, synth
        self.api, self.ctx = api, ctx
        rng = np.random.default_rng(2101)
        means = rng.uniform(LO, HI, size=(300, 3))
        S = rng.normal(0.0, 0.3, size=(300, 3, 3)) + np.eye(3) * rng.uniform(0.5, 3.0, size=(300, 3))[:, None, :]
        self.maps = {"ndt": api.NdtMap(ctx, means, S.reshape(300, 9), search_radius_sq=1.0), "voxel": api.VoxelMap(ctx, 1.0, 1.0)}
        for _ in range(2):
            self.maps["voxel"].insert(rng.uniform(LO, HI, size=(30_000, 3)))
        self.scan = api.Scan(ctx, means + rng.normal(0.0, 0.05, size=(300, 3)))  # 300 points, each near a voxel
        self.R4 = np.stack([helpers.rot_xyz(0.01 * k, -0.02, 0.005 * k).reshape(9) for k in range(4)])
        self.t4 = np.array([[0.05 * k, -0.03, 0.02] for k in range(4)])
        self.datasets = [api.NdtDataset.from_planes(ctx, synth.ndt_planes(500, 20, seed=2200 + s), "f64") for s in range(64)]
        self.R64, self.t64 = synth.random_poses(64, seed=2102, planar=False)

    def score(self, kind):
        return _freeze(self.api.score_batch(self.maps[kind], [self.scan], self.R4[:1], self.t4[:1], EXP))

    def register(self, kind):
        return _freeze(self.api.register6_batch(self.maps[kind], [self.scan] * 4, self.R4, self.t4, EXP, max_outer_iterations=10))

    def solve(self):
        R, t, reps = self.api.solve6_batch(self.datasets, self.R64, self.t64, EXP, max_iterations=100)
        assert all(rep["launches"] == 1 and not rep["fallback"] for rep in reps), "every problem runs in the batch launch"
        assert sum(len(rep["cost_history"]) for rep in reps) > 64, "the test needs cost histories"
        return _freeze((R, t, reps))

    def first_results(self):
        """Smallest staging first: (i) scores, (ii) registrations, (iii) the batched solve."""
        out = {("score", k): self.score(k) for k in ("ndt", "voxel")}
        out.update({("register", k): self.register(k) for k in ("ndt", "voxel")})
        out[("solve",)] = self.solve()
        return out

    def close(self):
        for d in self.datasets:
            d.close()
        self.scan.close()
        for m in self.maps.values():
            m.close()


def test_batched_calls_of_every_kind_share_one_pinned_block_and_repeat_bit_for_bit():
    from nonlinear_optimizer_for_slam_amd import Context, _lib
    ctx_a, ctx_b = Context((0,)), Context((0,))
    a, b = _Scene(ctx_a), _Scene(ctx_b)
    first = a.first_results()
    for key, value in first.items():
        print(key, "frozen result of", len(repr(value)), "characters")

    # (iv) a call that fails validation, between the calls that stage: a scan of another context
    rows = np.zeros(2, dtype=a.api.SCORE_DTYPE)
    rows["matches"], rows["matched_points"], rows["cost"], rows["reserved"] = 11, 12, 13.5, 14.5
    untouched = rows.tobytes()
    handles = (ctypes.c_void_p * 2)(a.scan._h, b.scan._h)
    loss = _lib.NosLoss(_lib.NOS_LOSS_EXPONENTIAL, 0, 1.0, 1.0)
    dp = lambda x: x.ctypes.data_as(_lib.c_double_p)  # noqa: E731
    status = _lib.hip_lib().nos_ndt_score_batch(a.maps["ndt"]._h, handles, 2, dp(a.R4), dp(a.t4), ctypes.byref(loss), 2,
                                                rows.ctypes.data_as(ctypes.POINTER(_lib.NosPoseScore)))
    assert status == INVALID
    assert rows.tobytes() == untouched
    with pytest.raises(_lib.NosError) as err:
        a.api.register6_batch(a.maps["voxel"], [a.scan, b.scan], a.R4[:2], a.t4[:2], EXP)
    assert err.value.status == INVALID

    # (v) in reverse order, each into a block larger than it needs and full of another call's bytes
    assert a.solve() == first[("solve",)]
    for kind in ("voxel", "ndt"):
        assert a.register(kind) == first[("register", kind)], kind
    for kind in ("voxel", "ndt"):
        assert a.score(kind) == first[("score", kind)], kind

    # the first results are those of a context whose block these calls grew on their own
    second = b.first_results()
    for key in first:
        assert second[key] == first[key], key
    a.close()
    b.close()
    ctx_a.close()
    ctx_b.close()
