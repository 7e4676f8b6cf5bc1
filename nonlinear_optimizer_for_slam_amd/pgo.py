"""Pose-graph optimisation handles over the C ABI (nos_pgo_*, include/nos.h) and a Python view of the
C++ drop-in class PoseGraphOptimizerHip (csrc/host/nos_pgo_solver.hpp)."""
import ctypes
import sys

import numpy as np

from . import _lib
from ._lib import c_double_p, check


def _dp(a):
    return a.ctypes.data_as(c_double_p)


_UPPER = np.triu_indices(6)


def information_from_sums(sums):
    """The 6x6 information matrix of a pose-graph edge from an accumulate6 / map_to_map result (its 21 numbers H, upper
    triangle row-major, in front of b and the cost): sums [>= 21] → [6, 6] symmetric.  At the pose a registration returns,
    target = reference and source = query, H is the information of that relative pose in the convention of
    PoseGraph(information=...) as it stands (include/nos.h, nos_pgo_create_weighted)."""
    h = np.asarray(sums, dtype=np.float64).reshape(-1)[:21]
    if h.size != 21:
        raise ValueError("sums holds fewer than 21 numbers")
    out = np.zeros((6, 6))
    out[_UPPER] = h
    return out + np.triu(out, 1).T


def pack_information(information, m):
    """[m, 6, 6] (symmetric; the upper triangle is read) or [m, 21] → contiguous [m, 21], upper triangle row-major."""
    a = np.asarray(information, dtype=np.float64)
    if a.shape == (m, 6, 6):
        if not np.array_equal(a, np.swapaxes(a, 1, 2)):
            raise ValueError("information matrices must be symmetric")
        a = a[:, _UPPER[0], _UPPER[1]]
    elif a.shape != (m, 21):
        raise ValueError("information must be [m, 6, 6] or [m, 21] for m = %d constraints, got %r" % (m, a.shape))
    return np.ascontiguousarray(a)


class PoseGraph:
    """Device-resident pose graph (nos_pose_graph).  poses [n,7] = px py pz qw qx qy qz, meas [m,7] likewise.
    information: [m, 6, 6] or [m, 21] (upper triangle row-major) — one information matrix per constraint over the error
    (dt, dtheta) of its measurement, t_true = t_m + dt, R_true = R_m Exp(dtheta) (nos_pgo_create_weighted in
    include/nos.h states the rule); None: every constraint weighs |r|^2 (nos_pgo_create).
    loss: None | ("huber", delta) | ("exponential", c1, c2) — a robust loss on q = r~^T Omega' r~ (set_loss; the rule is
    stated at nos_pgo_set_loss in include/nos.h); robust: [m] flags of the constraints it applies to, None = all.  A loss
    lives on graphs with information: with information=None every constraint takes the identity."""

    def __init__(self, ctx, poses, ref, qry, meas, switch_init=None, switch_free=None, fixed=None, information=None,
                 loss=None, robust=None):
        self._ctx = ctx
        self._lib = ctx._lib
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        meas = np.ascontiguousarray(meas, dtype=np.float64).reshape(-1, 7)
        ref = np.ascontiguousarray(ref, dtype=np.int32)
        qry = np.ascontiguousarray(qry, dtype=np.int32)
        self.n_poses, self.n_edges = poses.shape[0], ref.size
        ip = ctypes.POINTER(ctypes.c_int32)
        sw = None if switch_init is None else np.ascontiguousarray(switch_init, dtype=np.float64)
        swf = None if switch_free is None else np.ascontiguousarray(switch_free, dtype=np.uint8).tobytes()
        fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.uint8).tobytes()
        h = ctypes.c_void_p()
        if information is None and loss is not None and self.n_edges > 0:
            information = np.broadcast_to(np.eye(6), (self.n_edges, 6, 6))
        if information is None:
            check(self._lib.nos_pgo_create(ctx.handle, self.n_poses, _dp(poses), self.n_edges, ref.ctypes.data_as(ip),
                                           qry.ctypes.data_as(ip), _dp(meas), None if sw is None else _dp(sw), swf, fx,
                                           ctypes.byref(h)), "nos_pgo_create")
        else:
            info = pack_information(information, self.n_edges)
            check(self._lib.nos_pgo_create_weighted(ctx.handle, self.n_poses, _dp(poses), self.n_edges,
                                                    ref.ctypes.data_as(ip), qry.ctypes.data_as(ip), _dp(meas),
                                                    None if sw is None else _dp(sw), swf, fx, _dp(info), ctypes.byref(h)),
                  "nos_pgo_create_weighted")
        self._h = h
        ctx._adopt(self)
        if loss is not None:
            self.set_loss(loss, robust)

    def set_loss(self, loss, robust=None):
        """The robust loss from the NEXT linearize() on (nos_pgo_set_loss): None | ("huber", delta) |
        ("exponential", c1, c2); robust: [m] flags of the constraints it applies to (usually the loop closures), None = all.
        Products and solves before the next linearize() keep the weights of the last one, so an annealed schedule is a loop
        of set_loss / linearize / solve / retract."""
        from .api import make_loss
        l = make_loss(loss)
        flags = None
        if robust is not None:
            flags = np.ascontiguousarray(robust, dtype=np.uint8).reshape(-1)
            if flags.size != self.n_edges:
                raise ValueError("robust must hold one flag per constraint (%d), got %d" % (self.n_edges, flags.size))
            flags = flags.tobytes() if flags.size else b"\0"
        check(self._lib.nos_pgo_set_loss(self._h, ctypes.byref(l), flags), "nos_pgo_set_loss")

    def edge_weights(self):
        """[m]: the weight w = rho'(q) every constraint had at the last linearize() — 1.0 where no loss applies, near 0 for
        a constraint the loss has rejected."""
        out = np.ones(max(self.n_edges, 1))
        check(self._lib.nos_pgo_get_vector(self._h, 3, _dp(out)), "nos_pgo_get_vector")
        return out[:self.n_edges]

    @property
    def n_unknowns(self):
        return int(self._lib.nos_pgo_num_unknowns(self._h))

    def linearize(self):
        """→ (cost, |gradient|)."""
        c, g = ctypes.c_double(), ctypes.c_double()
        check(self._lib.nos_pgo_linearize(self._h, ctypes.byref(c), ctypes.byref(g)), "nos_pgo_linearize")
        return c.value, g.value

    def solve(self, lam, max_iterations=500, rel_tolerance=1e-10):
        """→ (pcg iterations, relative residual, |step|)."""
        it, res, sn = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        check(self._lib.nos_pgo_solve(self._h, ctypes.c_double(lam), max_iterations, ctypes.c_double(rel_tolerance),
                                      ctypes.byref(it), ctypes.byref(res), ctypes.byref(sn)), "nos_pgo_solve")
        return it.value, res.value, sn.value

    def retract(self):
        check(self._lib.nos_pgo_retract(self._h), "nos_pgo_retract")

    def state(self):
        poses = np.zeros((self.n_poses, 7))
        sw = np.zeros(max(self.n_edges, 1))
        check(self._lib.nos_pgo_get_state(self._h, _dp(poses), _dp(sw)), "nos_pgo_get_state")
        return poses, sw[:self.n_edges]

    def vector(self, which):
        """which: "gradient" | "step" | "hdiag"."""
        idx = {"gradient": 0, "step": 1, "hdiag": 2}[which]
        out = np.zeros(21 * self.n_poses if idx == 2 else self.n_unknowns)
        check(self._lib.nos_pgo_get_vector(self._h, idx, _dp(out)), "nos_pgo_get_vector")
        return out

    def matvec(self, lam, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.zeros_like(x)
        check(self._lib.nos_pgo_matvec(self._h, ctypes.c_double(lam), _dp(x), _dp(y)), "nos_pgo_matvec")
        return y

    def precondition(self, lam, r):
        """z = M^-1 r (nos_pgo_precondition): the preconditioner solve() would use at this lambda, for a host vector in the
        order of matvec().  Follows linearize(); honours the context options pgo_precond, pgo_agg and pgo_coarse_probe."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        check(self._lib.nos_pgo_precondition(self._h, ctypes.c_double(lam), _dp(r), _dp(z)), "nos_pgo_precondition")
        return z

    def layout_info(self):
        """What the sweeps touch (nos_pgo_layout_info): poses, constraints, entries / block size / blocks / halo poses of
        the block-local product (0 when the owner-computes product runs), aggregates and PCR levels of the coarse level."""
        info = (ctypes.c_ulonglong * 8)()
        check(self._lib.nos_pgo_layout_info(self._h, info), "nos_pgo_layout_info")
        keys = ("poses", "constraints", "entries", "block_poses", "blocks", "halo_poses", "aggregates", "pcr_levels")
        return dict(zip(keys, (int(v) for v in info)))

    def time_sweep(self, which, lam=1e-3, repeats=20):
        """ms per device-resident sweep (nos_pgo_time_sweep): which = "matvec" (the product of a PCG iteration) or
        "linearize" (the linearisation kernels, without the host's scalar readbacks)."""
        ms = ctypes.c_double()
        check(self._lib.nos_pgo_time_sweep(self._h, {"matvec": 0, "linearize": 1}[which], ctypes.c_double(lam), int(repeats),
                                           ctypes.byref(ms)), "nos_pgo_time_sweep")
        return ms.value

    def optimize(self, max_iterations=40, gradient_tolerance=1e-6, parameter_tolerance=1e-6, pcg_iterations=500,
                 pcg_tolerance=1e-10):
        """The reference's LM loop shape (always step; lambda x2 / x0.6 on the cost, clamp [1e-6, 1e-2]) driven
        from Python — the C++ class PoseGraphOptimizerHip runs the same loop natively."""
        lam, prev = 1e-3, np.finfo(np.float64).max
        hist = []
        it = 0
        for it in range(max_iterations):
            cost, gnorm = self.linearize()
            pcg_it, res, step = self.solve(lam, pcg_iterations, pcg_tolerance)
            self.retract()
            hist.append((cost, gnorm, step, pcg_it, res))
            if step < parameter_tolerance or gnorm < gradient_tolerance:
                break
            lam = min(max(lam * (2.0 if cost > prev else 0.6), 1e-6), 1e-2)
            prev = cost
        return it, hist

    def close(self):
        if self._h:
            self._lib.nos_pgo_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class PoseGraphOptimizerHip:
    """Python view of the C++ drop-in class (csrc/host/nos_pgo_solver.hpp) with the reference's surface:
    SetPose(index, pose7) / SetConstraint(ref, qry, rel_pose7, is_loop) / SetPoseConstant(index) / SetLossFunction(loss) /
    Solve(options).
    pose7 = px py pz qw qx qy qz.  After a successful Solve the registered pose arrays hold the optimum."""

    def __init__(self, pcg_max_iterations=2000, pcg_tolerance=1e-10):
        self._poses = {}
        self._constraints = []
        self._fixed = []
        self.pcg_max_iterations = pcg_max_iterations
        self.pcg_tolerance = pcg_tolerance
        self.report = None
        self.switch_parameters = None
        self._loss = None

    def SetLossFunction(self, loss):
        """loss: None | ("exponential", c1, c2) | ("huber", threshold), applied to every constraint.  Any other tuple stands
        for a LossFunction subclass the library has no device form of: Solve then returns False."""
        self._loss = loss

    def SetPose(self, pose_index, pose7):
        self._poses[int(pose_index)] = pose7  # kept by reference, overwritten on success

    def SetConstraint(self, reference_pose_index, query_pose_index, relative_pose7, is_loop=False, information=None):
        """information: 6 x 6 (SetConstraintInformation of the C++ class; the rule of PoseGraph(information=...))."""
        info = None if information is None else np.array(information, dtype=np.float64).reshape(36)
        self._constraints.append((int(reference_pose_index), int(query_pose_index),
                                  np.asarray(relative_pose7, dtype=np.float64).reshape(7), bool(is_loop), info))

    def SetPoseConstant(self, pose_index):
        self._fixed.append(int(pose_index))

    def Solve(self, options):
        from .synth import host_lib
        idx = np.array(sorted(self._poses), dtype=np.int32)
        poses = np.ascontiguousarray(np.stack([np.asarray(self._poses[i], dtype=np.float64) for i in idx]))
        m = len(self._constraints)
        ref = np.array([c[0] for c in self._constraints], dtype=np.int32)
        qry = np.array([c[1] for c in self._constraints], dtype=np.int32)
        meas = np.ascontiguousarray(np.stack([c[2] for c in self._constraints])) if m else np.zeros((1, 7))
        loop = np.array([c[3] for c in self._constraints], dtype=np.uint8).tobytes() if m else b"\0"
        fixed = np.array(self._fixed, dtype=np.int32)
        sw = np.ones(max(m, 1))
        rep = np.zeros(6)
        ip = ctypes.POINTER(ctypes.c_int)
        head = (ctypes.c_size_t(idx.size), idx.ctypes.data_as(ip), _dp(poses), ctypes.c_size_t(m), ref.ctypes.data_as(ip),
                qry.ctypes.data_as(ip), _dp(meas), loop, ctypes.c_size_t(fixed.size), fixed.ctypes.data_as(ip),
                ctypes.c_int(options.max_iterations), ctypes.c_double(options.gradient_tolerance),
                ctypes.c_double(options.parameter_tolerance), ctypes.c_int(self.pcg_max_iterations),
                ctypes.c_double(self.pcg_tolerance))
        has = np.array([c[4] is not None for c in self._constraints], dtype=np.uint8)
        info = None
        if has.any():
            info = np.ascontiguousarray(np.stack([np.zeros(36) if c[4] is None else c[4] for c in self._constraints]))
        if self._loss is not None:
            from .api import make_loss
            try:
                l = make_loss(self._loss)
                kind, a, b = l.kind, l.a, l.b
            except ValueError:
                kind, a, b = -1, 0.0, 0.0
            ok = host_lib().nos_host_pgo_solve_robust(*head, None if info is None else _dp(info), has.tobytes() if m else b"\0",
                                                      ctypes.c_int(kind), ctypes.c_double(a), ctypes.c_double(b), _dp(sw),
                                                      _dp(rep))
        elif info is not None:
            ok = host_lib().nos_host_pgo_solve_weighted(*head, _dp(info), has.tobytes(), _dp(sw), _dp(rep))
        else:
            ok = host_lib().nos_host_pgo_solve(*head, _dp(sw), _dp(rep))
        self.report = {"iterations": int(rep[0]), "initial_cost": rep[1], "final_cost": rep[2],
                       "final_gradient_norm": rep[3], "total_pcg_iterations": int(rep[4]), "status": int(rep[5])}
        if ok:
            for k, i in enumerate(idx):
                self._poses[int(i)][:] = poses[k]
            self.switch_parameters = sw[:m].copy()
        return bool(ok)
