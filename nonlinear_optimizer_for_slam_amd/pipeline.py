"""GPU-resident scan-to-map registration: match → solve → re-match, nothing returns to the host
between matching and solving except the pose.

Mirrors the outer loop of the reference's test drivers (OptimizePoseAnalytic,
nonlinear_optimizer/mahalanobis_distance_minimizer/tests/simple_optimization_test.cc:474-503):
up to 10 rounds of {MatchPointCloud at the current pose, Solve()}, stopping when the pose changed by
less than 1e-5 in translation and in the quaternion vector part.
"""
import math

import numpy as np

from .api import NdtMap, Scan, VoxelMap, register3_batch, register6_batch, score_batch
from .solvers import MahalanobisDistanceMinimizerHip, MahalanobisDistanceMinimizerHip3DOF, Options, Pose


def _quat_vec_norm(R):
    """|vec(q)| of the rotation matrix R = sin(angle / 2)."""
    c = (np.trace(R) - 1.0) / 2.0
    c = min(1.0, max(-1.0, c))
    return float(np.sqrt(max(0.0, (1.0 - c) / 2.0)))


_SERIES_THETA = 0.25  # below it (theta - sin theta) / theta^3 and its kin come from their series (kDeskewSeriesTheta)


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def twist_pose(twist):
    """twist [6] = (v, w), translation first → Pose = Exp(twist), the SE(3) exponential (the rule of nos_scan_deskew,
    DESIGN.md §24): R = I + a [w]x + b [w]x², t = (I + b [w]x + c [w]x²) v with a = sin θ / θ, b = (1 − cos θ) / θ²,
    c = (θ − sin θ) / θ³ at θ = |w|.  1 − cos θ is 2 sin²(θ/2), c comes from its series below θ = 0.25, and θ < 1e-8 (θ = 0,
    θ² underflowing) gives the limits 1, 1/2, 1/6."""
    twist = np.asarray(twist, dtype=np.float64).reshape(6)
    v, w = twist[:3], twist[3:]
    theta = math.hypot(w[0], w[1], w[2])  # scaled: 1e-170 stays 1e-170
    q = theta * theta
    if theta < 1e-8:  # the limits are exact to the last digit here (1 − θ²/6, …), and θ² may underflow
        a, b, c = 1.0, 0.5, 1.0 / 6.0
    else:
        a = np.sin(theta) / theta
        b = 2.0 * np.sin(0.5 * theta) ** 2 / q
        if theta < _SERIES_THETA:
            c = 1 / 6 + q * (-1 / 120 + q * (1 / 5040 + q * (-1 / 362880 + q * (1 / 39916800 - q / 6227020800))))
        else:
            c = (theta - np.sin(theta)) / (q * theta)
    W = _hat(w)
    W2 = W @ W
    return Pose(np.eye(3) + a * W + b * W2, v + b * (W @ v) + c * (W2 @ v))


def pose_twist(pose_a, pose_b):
    """→ twist [6] = Log(T_a⁻¹ T_b), translation first: the constant body-frame twist that carries pose_a to pose_b in
    one unit of time (twist_pose's inverse).  Rotation angles up to π − 1e-6; at π itself the axis' sign is not defined
    and the result is one of the two logarithms, with no promise which.
    The angle is atan2(|vec|, (tr − 1) / 2) with vec the antisymmetric part of R, so it is as accurate near 0 as near π/2;
    beyond 3π/4 the axis comes from the symmetric part, where vec loses its digits.  The translation is V⁻¹ t,
    V⁻¹ = I − ½ [w]x + d [w]x², d = (1 − (θ/2) cot(θ/2)) / θ², from its series below θ = 0.25."""
    if np.array_equal(pose_a.R, pose_b.R) and np.array_equal(pose_a.t, pose_b.t):
        return np.zeros(6)  # exactly, whatever the rounding of Rᵀ R
    R = pose_a.R.T @ pose_b.R
    t = pose_a.R.T @ (pose_b.t - pose_a.t)
    vec = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])  # sin θ · axis
    s = math.hypot(vec[0], vec[1], vec[2])
    cth = 0.5 * (np.trace(R) - 1.0)
    theta = float(np.arctan2(s, cth))
    if s == 0.0:
        w = vec.copy()  # θ = 0 (θ = π exactly is not supported)
    elif cth > -0.7:
        w = vec * (theta / s)
    else:  # R + Rᵀ = 2 cos θ I + 2 (1 − cos θ) k kᵀ: the largest k_i from the diagonal, the others from its row
        S = 0.5 * (R + R.T)
        i = int(np.argmax(np.diag(S)))
        ki = np.sqrt(max(0.0, (S[i, i] - cth) / (1.0 - cth)))
        axis = S[i] / ((1.0 - cth) * ki)
        axis[i] = ki
        if vec[i] < 0.0:
            axis = -axis
        w = axis * (theta / np.sqrt(axis @ axis))
    q = theta * theta
    if theta < _SERIES_THETA:
        d = 1 / 12 + q * (1 / 720 + q * (1 / 30240 + q * (1 / 1209600 + q * (1 / 47900160 + q * (
            691 / 1307674368000 + q * (1 / 74724249600 + q * (3617 / 10670622842880000)))))))
    else:
        half = 0.5 * theta
        d = (1.0 - half * np.cos(half) / np.sin(half)) / q
    W = _hat(w)
    return np.concatenate([t - 0.5 * (W @ t) + d * (W @ (W @ t)), w])


def scan_to_map(ctx, ndt_map, scan, initial_pose=None, loss=("exponential", 1.0, 1.0), options=None,
                max_outer_iterations=10, dof=6, dtype="f64", on_solve=None, indexed=False, keep_multiple=None,
                device_loop=True, live_indexed=False):
    """ndt_map: api.NdtMap, or an api.VoxelMap — every round then matches against the live store (VoxelMap.match, no
    snapshot) and gives the pose, rounds and outer_iter of scan_to_map on its snapshot(), bit for bit; scan: api.Scan.
    → (Pose, list of per-round dicts, outer_iter) — outer_iter as the reference prints it (index of the round that met
    the stopping test, or max_outer_iterations).

    indexed=True: the matcher emits voxel ids instead of 120-byte records (nos_ndt_match_indexed) and the solver runs on
    the voxel-indexed layout — 2-3x less memory traffic per LM iteration for large scans (sort the scan by cell first:
    api.Scan(..., sort_cell=...)); same sums, same pose.

    live_indexed=True (an api.VoxelMap only): every round matches through VoxelMap.match_indexed(..., sort_by_voxel=False)
    — the voxel-indexed layout against the live store, with a voxel table of just the voxels the round matched
    (nos_voxel_map_match_indexed).  Pose, rounds and outer_iter are bit for bit those of
    scan_to_map(ctx, voxel_map.snapshot(), scan, indexed=True).  Its own keyword because indexed=True with a VoxelMap
    raises ValueError and keeps doing so; an NdtMap, keep_multiple or indexed=True next to it raise ValueError.

    keep_multiple=k: every round uses only the first floor(N/k)*k of its N matches, as the reference's classes do on their
    correspondence vector (k = 4: scalar 3-DoF class, MDM/..._analytic_3dof.cc:33-36, and the revision of the 6-DoF class
    behind results/*.txt; k = 8: the SIMD classes) — done on the device (nos_dataset_drop_last_matches).

    on_solve(round, report, n_matches) is called after every inner Solve (e.g. to print the
    reference's `COST: ..., iter: ...` lines)."""
    if indexed and keep_multiple:
        raise ValueError("keep_multiple (the tail drop of the reference's classes) is implemented for the flat layout only: "
                         "a voxel-indexed dataset has no per-match records to clear (nos_dataset_drop_last_matches)")
    if live_indexed:
        if indexed:
            raise ValueError("live_indexed=True and indexed=True are two routes: pick one (indexed=True needs an NdtMap)")
        if keep_multiple:
            raise ValueError("keep_multiple is implemented for the flat layout only: live_indexed=True builds a "
                             "voxel-indexed dataset")
        if not isinstance(ndt_map, VoxelMap):
            raise ValueError("live_indexed=True matches against a live VoxelMap: with an NdtMap use indexed=True")
    if indexed and isinstance(ndt_map, VoxelMap):
        raise ValueError("indexed=True needs an NdtMap: there is no live voxel-indexed match against a VoxelMap "
                         "(take a snapshot() first)")
    pose = Pose() if initial_pose is None else Pose(initial_pose.R, initial_pose.t)
    last = Pose(pose.R, pose.t)
    options = options or Options()
    solver = (MahalanobisDistanceMinimizerHip3DOF if dof == 3 else MahalanobisDistanceMinimizerHip)(
        device_ids=ctx.device_ids, dtype=dtype, device_loop=device_loop)
    solver.SetLossFunction(loss)
    rounds = []
    outer = 0
    for outer in range(max_outer_iterations):
        n_used = None
        if indexed or live_indexed:
            dataset, n_matches = ndt_map.match_indexed(scan, pose.R, pose.t, 2, dtype, sort_by_voxel=False)
        else:
            dataset, n_matches = ndt_map.match(scan, pose.R, pose.t, 2, dtype)
            if keep_multiple:
                n_used = n_matches - n_matches % int(keep_multiple)
                dataset.drop_last_matches(n_matches - n_used)
        try:
            if not solver.SolveDataset(options, dataset, pose):
                raise RuntimeError("SolveDataset failed (status %d)" % solver.report.status)
        finally:
            dataset.close()
        rounds.append({"matches": n_matches, "used": n_matches if n_used is None else n_used,  # matched / summed by the solve
                       "iterations": solver.report.iterations, "printed_cost": solver.report.printed_cost})
        if on_solve is not None:
            on_solve(outer, solver.report, n_matches)
        dR = pose.R.T @ last.R                  # optimized_pose.inverse() * last_optimized_pose
        dt = pose.R.T @ (last.t - pose.t)
        if np.linalg.norm(dt) < 1e-5 and _quat_vec_norm(dR) < 1e-5:
            break
        last = Pose(pose.R, pose.t)
    else:
        outer = max_outer_iterations  # never met the stopping test: the reference's loop variable ends at the bound
    return pose, rounds, outer


def map_to_map(ctx, target, source, initial_pose=None, loss=("exponential", 1.0, 1.0), options=None,
               max_outer_iterations=10, max_neighbors=2, dtype="f64", levels=None, on_solve=None):
    """The pose of one api.VoxelMap in the frame of another, from their voxels alone (distribution-to-distribution NDT,
    DESIGN.md §23): scan_to_map's outer loop with target.match_map(source, ...) as the matcher — up to
    max_outer_iterations rounds of {match_map at the current pose, 6-DoF SolveDataset}, the same stopping test, the same
    `rounds` dicts, RuntimeError when a round's solve fails.  A round's information matrices are those of its match and
    stay fixed during its solve; the next round re-evaluates them with the correspondences.  Neither store is modified.
    levels: None, or factors such as (4, 2, 1) — coarse to fine: for a factor f != 1 target.coarsened(f) is registered
    against the source coarsened ON THE SAME GRID: the source's voxels merged, under the previous level's pose, into a
    fresh store with the coarse target's resolution and radius (VoxelMap.merge, the source's flags), so both coarse maps
    cut space along the same planes and summarise the same pieces of it when the pose is right.  (source.coarsened(f)
    cuts along the source's own axes, which the pose turns and shifts against the target's; two partitions half a cell
    apart give means that differ by up to half a coarse cell at the true pose.)  That level solves for the correction on
    top of its start pose and the two are composed.  Both temporaries are closed, also before an exception leaves;
    factor 1 uses the stores themselves and has to be the last one (ValueError otherwise: a coarse level's normal
    equations describe its correction, not the pose returned).  Every level runs up to max_outer_iterations rounds;
    `rounds` is the concatenation, each dict with a "level" key, and outer_iter is the last level's.
    → (Pose, rounds, outer_iter, info).  info["sums"]: NdtDataset.accumulate6 (21 H | 6 g | cost, under `loss`) of ONE
    MORE match_map of the stores themselves at the returned pose — so correspondences, information matrices and
    linearisation point all belong to that pose; its 6 x 6 block is what a caller turns into the information of a
    pose-graph edge.  info["matches"]: that match's count."""
    pose = Pose() if initial_pose is None else Pose(initial_pose.R, initial_pose.t)
    options = options or Options()
    solver = MahalanobisDistanceMinimizerHip(device_ids=ctx.device_ids, dtype=dtype)
    solver.SetLossFunction(loss)
    rounds, outer, info = [], 0, {}
    factors = (1,) if levels is None else tuple(levels)
    if not factors:
        raise ValueError("levels needs at least one factor")
    if factors[-1] != 1:
        raise ValueError("the last factor of levels has to be 1: info[\"sums\"] and the returned pose belong to the stores "
                         "themselves, a coarse level only prepares the start of the next (got %r)" % (factors,))
    for li, factor in enumerate(factors):
        made = []
        base = None
        try:
            if factor == 1:
                tgt, src = target, source
            else:
                tgt = target.coarsened(factor)
                made.append(tgt)
                src = VoxelMap(ctx, tgt.voxel_resolution, tgt.search_radius_sq, flags=source._flags)
                made.append(src)
                base = pose
                src.merge(source, base.R, base.t)
                pose = Pose()  # the correction on top of `base`: src is already in the target's frame as base has it
            last = Pose(pose.R, pose.t)
            for outer in range(max_outer_iterations):
                dataset, n_matches = tgt.match_map(src, pose.R, pose.t, max_neighbors, dtype)
                try:
                    if not solver.SolveDataset(options, dataset, pose):
                        raise RuntimeError("SolveDataset failed (status %d)" % solver.report.status)
                finally:
                    dataset.close()
                row = {"matches": n_matches, "used": n_matches, "iterations": solver.report.iterations,
                       "printed_cost": solver.report.printed_cost}
                if levels is not None:
                    row["level"] = factor
                rounds.append(row)
                if on_solve is not None:
                    on_solve(outer, solver.report, n_matches)
                dR = pose.R.T @ last.R
                dt = pose.R.T @ (last.t - pose.t)
                if np.linalg.norm(dt) < 1e-5 and _quat_vec_norm(dR) < 1e-5:
                    break
                last = Pose(pose.R, pose.t)
            else:
                outer = max_outer_iterations
            if li == len(factors) - 1:
                dataset, n_matches = tgt.match_map(src, pose.R, pose.t, max_neighbors, dtype)
                try:
                    info = {"sums": dataset.accumulate6(pose.R, pose.t, loss), "matches": n_matches}
                finally:
                    dataset.close()
            if base is not None:
                pose = Pose(pose.R @ base.R, pose.R @ base.t + pose.t)
        finally:
            for vm in made:
                vm.close()
    return pose, rounds, outer, info


def _quat_wxyz(R):
    """Unit quaternion (w x y z, w >= 0) of a rotation matrix: the largest of the four components from the diagonal, the
    other three from the off-diagonal sums and differences."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    d = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2],
                  R[2, 2] - R[0, 0] - R[1, 1]])
    k = int(np.argmax(d))
    q = np.zeros(4)
    q[k] = 0.5 * np.sqrt(1.0 + d[k])
    f = 0.25 / q[k]
    if k == 0:
        q[1:] = (R[2, 1] - R[1, 2]) * f, (R[0, 2] - R[2, 0]) * f, (R[1, 0] - R[0, 1]) * f
    else:
        i, j, l = k - 1, k % 3, (k + 1) % 3
        q[0] = (R[l, j] - R[j, l]) * f
        q[1 + j] = (R[j, i] + R[i, j]) * f
        q[1 + l] = (R[l, i] + R[i, l]) * f
    q /= np.linalg.norm(q)
    return -q if q[0] < 0.0 else q


def map_edge(ctx, target, source, guess=None, **map_to_map_kwargs):
    """A pose-graph edge between two submaps: map_to_map(ctx, target, source, guess, **map_to_map_kwargs) and the packing
    pgo.PoseGraph takes.  → {"meas": pose7 = px py pz qw qx qy qz of the source (query) in the frame of the target
    (reference), "information": 6 x 6 = pgo.information_from_sums(info["sums"]) — the normal matrix of the registration
    at that pose, which is the information of the measurement in PoseGraph's convention as it stands (include/nos.h),
    "matches": info["matches"], "rounds": map_to_map's rounds}."""
    from .pgo import information_from_sums
    pose, rounds, _, info = map_to_map(ctx, target, source, guess, **map_to_map_kwargs)
    meas = np.concatenate([np.asarray(pose.t, dtype=np.float64).reshape(3), _quat_wxyz(pose.R)])
    return {"meas": meas, "information": information_from_sums(info["sums"]), "matches": info["matches"], "rounds": rounds}


def scan_to_map_batch(ctx, ndt_map, scans, initial_poses=None, loss=("exponential", 1.0, 1.0), options=None,
                      max_outer_iterations=10, dof=6, dtype="f64", keep_multiple=None):
    """scan_to_map for many scans against one map in ONE launch (api.register6_batch / register3_batch): the outer loop
    runs on the device, one workgroup per scan.  scans: list of api.Scan (the same one may repeat); initial_poses: None
    (identity for all) or a list of Poses.  → list of (Pose, rounds, outer_iter) shaped exactly as scan_to_map returns
    them, or None where scan_to_map would raise RuntimeError (a round's solve failed; the other rows are unaffected).
    Bit for bit scan_to_map's result for scans of ≤ 512 points, to rounding above.
    ndt_map: api.NdtMap, or an api.VoxelMap — the rounds then match against the live store inside the launch (no
    snapshot); every row is bit for bit the row of the call on its snapshot(), at any scan size."""
    scans = list(scans)
    B = len(scans)
    if initial_poses is None:
        initial_poses = [Pose() for _ in range(B)]
    if len(initial_poses) != B:
        raise ValueError("%d scans but %d initial poses" % (B, len(initial_poses)))
    options = options or Options()
    R0 = np.array([p.R.reshape(9) for p in initial_poses]).reshape(B, 9)
    t0 = np.array([p.t.reshape(3) for p in initial_poses]).reshape(B, 3)
    fn = register3_batch if dof == 3 else register6_batch
    R, t, reports = fn(ndt_map, scans, R0, t0, loss, max_outer_iterations=max_outer_iterations,
                       keep_multiple=keep_multiple, dtype=dtype, max_iterations=options.max_iterations,
                       gradient_tolerance=options.gradient_tolerance, parameter_tolerance=options.parameter_tolerance)
    out = []
    for i, rep in enumerate(reports):
        if not rep["ok"]:
            out.append(None)
            continue
        rounds = [{"matches": r["matches"], "used": r["used"], "iterations": r["iterations"],
                   "printed_cost": r["printed_cost"]} for r in rep["rounds"]]
        out.append((Pose(R[i].reshape(3, 3), t[i]), rounds, rep["outer_iter"]))
    return out


def _ndt_fitness(scores, loss):
    """The NDT fitness a · matches − cost of score_batch rows under the exponential loss (a, b): a Σ exp(−b s) over the
    correspondences, higher is better."""
    return float(loss[1]) * scores["matches"].astype(np.float64) - scores["cost"]


def relocalize(ctx, ndt_map, scan, candidates, loss=("exponential", 1.0, 1.0), top_k=8, score_scan=None, key=None,
               **scan_to_map_batch_kwargs):
    """Which of many candidate poses is the scan at?  Score them all in one call, register the best few, score again.
    ndt_map: api.NdtMap or api.VoxelMap (the live store); scan: api.Scan; candidates: list of Poses.
    1. every candidate is scored with score_scan (default: scan; a coarser scan.filtered(...) is the intended use) by
       api.score_batch — one launch, one number per pose;
    2. they are ranked by key(scores) → [len(candidates)] floats, higher is better, ties by lower candidate index.  The
       default key is the NDT fitness a · matches − cost (_ndt_fitness), which needs the exponential loss: another loss
       without a key raises ValueError;
    3. scan_to_map_batch registers the full scan from the top_k candidates (scan_to_map_batch_kwargs go to it unchanged);
    4. the final poses of the registrations that did not fail are scored with the full scan in one more score_batch call;
    5. → (Pose, info) of the best final key, ties by lower candidate index.  info: scores and fitness (stage 1, per
       candidate), chosen (candidate indices registered, best first), registrations (scan_to_map_batch's rows for them),
       final_scores and final_fitness (per chosen candidate; a failed registration: a zero row and -inf), winner (the
       candidate index the returned pose started from).
    If every registration failed, RuntimeError, as scan_to_map raises."""
    candidates = list(candidates)
    if key is None:
        if loss is None or loss[0] != "exponential":
            raise ValueError("the default key is the NDT fitness a * matches - cost of the exponential loss: "
                             "pass key= with loss %r" % (loss,))
        key = lambda scores: _ndt_fitness(scores, loss)  # noqa: E731
    if not candidates:
        raise ValueError("relocalize needs at least one candidate pose")
    n = len(candidates)
    R = np.array([p.R.reshape(9) for p in candidates]).reshape(n, 9)
    t = np.array([p.t.reshape(3) for p in candidates]).reshape(n, 3)
    scores = score_batch(ndt_map, [scan if score_scan is None else score_scan] * n, R, t, loss)
    fitness = np.asarray(key(scores), dtype=np.float64).reshape(n)
    chosen = sorted(range(n), key=lambda i: (-fitness[i], i))[:max(int(top_k), 1)]
    rows = scan_to_map_batch(ctx, ndt_map, [scan] * len(chosen), [candidates[i] for i in chosen], loss=loss,
                             **scan_to_map_batch_kwargs)
    alive = [k for k, row in enumerate(rows) if row is not None]
    if not alive:
        raise RuntimeError("SolveDataset failed for every candidate (each registration returned ok = 0)")
    Rf = np.array([rows[k][0].R.reshape(9) for k in alive]).reshape(len(alive), 9)
    tf = np.array([rows[k][0].t.reshape(3) for k in alive]).reshape(len(alive), 3)
    alive_scores = score_batch(ndt_map, [scan] * len(alive), Rf, tf, loss)
    final_scores = np.zeros(len(chosen), dtype=alive_scores.dtype)
    final_fitness = np.full(len(chosen), -np.inf)
    final_scores[alive] = alive_scores
    final_fitness[alive] = np.asarray(key(alive_scores), dtype=np.float64).reshape(len(alive))
    best = min(alive, key=lambda k: (-final_fitness[k], chosen[k]))
    info = {"scores": scores, "fitness": fitness, "chosen": list(chosen), "registrations": rows,
            "final_scores": final_scores, "final_fitness": final_fitness, "winner": chosen[best]}
    return rows[best][0], info


def loop_candidates(db, query, top_k=5, max_distance=None, exclude_last=0):
    """Have I been here before, and roughly which way was I facing?  One exhaustive search of an api.PlaceDatabase
    (every stored place at every yaw) → the best places as a list of (index, distance, yaw), sorted by
    distance, then index; at most top_k of them (None: all), only those with distance <= max_distance when that is given.
    query: an api.Scan (its descriptor never leaves the device) or one host descriptor [n_rings, n_sectors].
    yaw = 2π · shift / n_sectors wrapped to (−π, π]: the yaw of the query's sensor relative to the stored scan's, so the
    rough pose of the query is T_stored ∘ Rz(yaw) (candidate_poses).
    exclude_last: the newest entries are left out (the search window is narrowed, they are not even read) — a place does
    not match the frames just before it."""
    count = max(len(db) - max(int(exclude_last), 0), 0)
    if count == 0:
        return []
    distance, shift = db.search(query, 0, count)
    distance, shift = np.asarray(distance).reshape(-1, count), np.asarray(shift).reshape(-1, count)
    if distance.shape[0] != 1:
        raise ValueError("loop_candidates takes one query")
    distance, shift = distance[0], shift[0]
    order = sorted(range(count), key=lambda i: (distance[i], i))
    if max_distance is not None:
        order = [i for i in order if distance[i] <= max_distance]
    if top_k is not None:
        order = order[:max(int(top_k), 0)]
    out = []
    for i in order:
        yaw = 2.0 * math.pi * int(shift[i]) / db.n_sectors
        if yaw > math.pi:
            yaw -= 2.0 * math.pi
        out.append((i, float(distance[i]), yaw))
    return out


def candidate_poses(candidates, stored_poses):
    """loop_candidates' rows → the rough poses of the query as relocalize takes them: for (index, distance, yaw) the Pose
    R = R_stored · Rz(yaw), t = t_stored, with (R_stored, t_stored) = stored_poses[index] (a Pose or an (R, t) pair)."""
    out = []
    for index, _, yaw in candidates:
        stored = stored_poses[index]
        R, t = (stored.R, stored.t) if hasattr(stored, "R") else stored
        c, s = math.cos(yaw), math.sin(yaw)
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        out.append(Pose(np.asarray(R, dtype=np.float64).reshape(3, 3) @ Rz, np.asarray(t, dtype=np.float64).reshape(3)))
    return out


def map_places(ctx, vmap, poses, pattern, db=None, max_range=None, n_rings=20, n_sectors=60, descriptor_max_range=80.0,
               z_floor=-2.0, reserve=0, **raycast_kwargs):
    """Places from a map nobody scanned: for every pose the store is ray-cast along `pattern` and the hit
    points, a scan in that pose's sensor frame, go into a PlaceDatabase — ray cast → db.add(scan), nothing visits the
    host but the counts.  → (db, hits_per_pose).  The database is indexed like `poses`, so loop_candidates →
    candidate_poses(found, poses) → relocalize work on a map that was merged, coarsened, paged in or built elsewhere.
    vmap: api.VoxelMap; poses: Poses or (R, t) pairs; pattern: an api.Scan of beam directions (api.ray_pattern uploaded)
    or the [n, 3] array itself; max_range: the ray cast's (required).  db: an api.PlaceDatabase to append to (it must be
    empty for its indices to be those of `poses`); None: a new one with n_rings, n_sectors, descriptor_max_range and
    z_floor (with `reserve` or len(poses) places reserved).  raycast_kwargs (min_range, max_mahalanobis_sq, min_points,
    origin) go to VoxelMap.raycast unchanged."""
    from .api import PlaceDatabase
    if max_range is None:
        raise ValueError("map_places needs the ray cast's max_range")
    rc = {"min_range": 0.0, "max_mahalanobis_sq": 1.0, "min_points": 0, "origin": (0, 0, 0)}  # VoxelMap.raycast's defaults
    unknown = set(raycast_kwargs) - set(rc)
    if unknown:
        raise TypeError("map_places: unknown ray cast parameters %s" % sorted(unknown))
    rc.update(raycast_kwargs)
    poses = list(poses)
    own_pattern = not isinstance(pattern, Scan)
    rays = Scan(ctx, pattern) if own_pattern else pattern
    own_db = db is None
    if own_db:
        db = PlaceDatabase(ctx, n_rings, n_sectors, descriptor_max_range, z_floor, reserve=max(int(reserve), len(poses)))
    hits = []
    try:
        for pose in poses:
            R, t = (pose.R, pose.t) if hasattr(pose, "R") else pose
            _, _, info = vmap._raycast(rays, R, t, max_range, rc["min_range"], rc["max_mahalanobis_sq"], rc["min_points"], rc["origin"],
                                       True, False)  # the hit points stay on the device, the per-ray arrays are not fetched
            try:
                db.add(info["scan"])
            finally:
                info["scan"].close()
            hits.append(info["hits"])
    except Exception:
        if own_db:
            db.close()
        raise
    finally:
        if own_pattern:
            rays.close()
    return db, hits


def combine_cells(cells, counts, sums, stamps):
    """Voxels of one grid that may name a cell more than once → one voxel per cell, in ascending cell order: counts added,
    sums added in ARRIVAL order (left to right, as they stand in the arrays), stamp the last one's.  A plain function over
    arrays: cells [n,3] int64, counts [n], sums [n,9], stamps [n] → the same four.  A cell whose count passes 2^32 − 1
    raises OverflowError."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
    counts = np.asarray(counts, dtype=np.uint32).reshape(-1)
    sums = np.asarray(sums, dtype=np.float64).reshape(-1, 9)
    stamps = np.asarray(stamps, dtype=np.uint32).reshape(-1)
    uniq, inverse = np.unique(cells, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    if uniq.shape[0] == cells.shape[0]:  # nothing came twice: only the order changes
        order = np.argsort(inverse, kind="stable")
        return uniq, counts[order], sums[order], stamps[order]
    total = np.zeros(uniq.shape[0], dtype=np.uint64)
    np.add.at(total, inverse, counts.astype(np.uint64))
    if total.size and int(total.max()) > 0xFFFFFFFF:
        raise OverflowError("a cached voxel would hold more than 2^32 - 1 points")
    out = np.zeros((uniq.shape[0], 9))
    np.add.at(out, inverse, sums)  # unbuffered: one addition per row, in the order of the rows
    last = np.zeros(uniq.shape[0], dtype=np.uint32)
    last[inverse] = stamps  # a repeated index keeps the last assignment
    return uniq, total.astype(np.uint32), out, last


def tiles_of_cells(cells, tile_cells):
    """→ the tile floor(cell / tile_cells) of every cell, [n,3] int64 (floor, so negative cells land in negative tiles)."""
    return np.floor_divide(np.asarray(cells, dtype=np.int64).reshape(-1, 3), np.int64(tile_cells))


class TileCache:
    """Host-side cache of voxels paged out of an api.VoxelMap, keyed by tile = floor(cell / tile_cells) per
    axis: the sliding window of odometry() as a cache over a larger map.  put() takes a state (VoxelMap.export), take()
    gives one back (for VoxelMap.add) and forgets it.  All voxels belong to one grid: a state of another
    voxel_resolution raises ValueError.  Nothing here touches a device."""

    def __init__(self, tile_cells=16):
        if int(tile_cells) < 1:
            raise ValueError("tile_cells must be >= 1")
        self.tile_cells = int(tile_cells)
        self._tiles = {}  # (tx, ty, tz) → (cells, counts, sums, stamps), one voxel per cell, ascending cell
        self._meta = None  # voxel_resolution, search_radius_sq, proper_sqrt_information of the first state
        self._epoch = 0
        self._n = 0

    def __len__(self):
        """Number of cached voxels."""
        return self._n

    def put(self, state):
        """The voxels of a state, grouped by tile.  A cell that is cached already (or comes twice) is combined in arrival
        order: counts added, sums added, stamp the later one (combine_cells).  → number of voxels the state held."""
        counts = np.asarray(state["counts"], dtype=np.uint32).reshape(-1)
        n = counts.size
        if n == 0:
            return 0
        meta = (float(state["voxel_resolution"]), float(state["search_radius_sq"]), bool(state["proper_sqrt_information"]))
        if self._meta is None:
            self._meta = meta
        elif meta[0] != self._meta[0]:
            raise ValueError("the cache holds voxels of resolution %r, the state has %r" % (self._meta[0], meta[0]))
        self._epoch = max(self._epoch, int(state.get("epoch", 0)))
        cells = np.asarray(state["cells"], dtype=np.int64).reshape(-1, 3)
        sums = np.asarray(state["sums"], dtype=np.float64).reshape(-1, 9)
        stamps = state.get("stamps")
        stamps = np.zeros(n, dtype=np.uint32) if stamps is None else np.asarray(stamps, dtype=np.uint32).reshape(-1)
        tiles = tiles_of_cells(cells, self.tile_cells)
        uniq, inverse = np.unique(tiles, axis=0, return_inverse=True)
        order = np.argsort(inverse.reshape(-1), kind="stable")  # by tile, arrival order within a tile
        bounds = np.searchsorted(inverse.reshape(-1)[order], np.arange(uniq.shape[0] + 1))
        for k in range(uniq.shape[0]):
            rows = order[bounds[k]:bounds[k + 1]]
            key = tuple(int(x) for x in uniq[k])
            new = (cells[rows], counts[rows], sums[rows], stamps[rows])
            old = self._tiles.get(key)
            if old is not None:
                self._n -= old[1].size
                new = tuple(np.concatenate([a, b]) for a, b in zip(old, new))
            self._tiles[key] = combine_cells(*new)
            self._n += self._tiles[key][1].size
        return n

    def take(self, lo_cell, hi_cell):
        """Removes and returns, as ONE state, every cached tile that meets the closed cell box lo_cell … hi_cell ([3] each,
        inclusive): whole tiles, so voxels outside the box come along.  Tiles in ascending order, cells ascending within
        a tile.  The state's epoch is the largest one put() has seen."""
        lo = tiles_of_cells(np.asarray(lo_cell, dtype=np.int64), self.tile_cells)[0]
        hi = tiles_of_cells(np.asarray(hi_cell, dtype=np.int64), self.tile_cells)[0]
        hit = sorted(key for key in self._tiles if all(lo[k] <= key[k] <= hi[k] for k in range(3)))
        parts = [self._tiles.pop(key) for key in hit]
        res, radius, proper = self._meta if self._meta is not None else (None, None, None)
        if parts:
            cells, counts, sums, stamps = (np.concatenate(a) for a in zip(*parts))
        else:
            cells, counts = np.zeros((0, 3), dtype=np.int64), np.zeros(0, dtype=np.uint32)
            sums, stamps = np.zeros((0, 9)), np.zeros(0, dtype=np.uint32)
        self._n -= counts.size
        return {"cells": cells, "counts": counts, "sums": sums, "stamps": stamps, "epoch": self._epoch,
                "voxel_resolution": res, "search_radius_sq": radius, "proper_sqrt_information": proper}

    def take_all(self):
        """take() of everything."""
        lim = 1 << 40
        return self.take((-lim,) * 3, (lim,) * 3)


_ONE_LAUNCH_KWARGS = ("loss", "options", "max_outer_iterations", "dof", "dtype", "keep_multiple")


def odometry(ctx, voxel_map, scans, initial_pose=None, window_half_extent=None, max_voxel_age=None, filter_voxel_size=None,
             insert_filtered=False, live_match=None, one_launch=False, live_indexed=False, sweep_times=None, sweep_reference=1.0,
             carve=None, place_db=None, tiles=None, **scan_to_map_kwargs):
    """Scan-to-map odometry over a growing map (api.VoxelMap): for each scan, snapshot the store → scan_to_map from the
    previous scan's pose → insert the scan at the pose found (VoxelMap.insert_scan, warped on the device).  The harness's
    sequence UpdateNdtMap → OptimizePose → UpdateNdtMap (MDM/tests/simple_optimization_test.cc:236-281, 474-503) with the
    map kept on the device between frames.  scans: iterable of api.Scan; scan_to_map_kwargs go to scan_to_map unchanged.
    window_half_extent ([3] or a scalar, metres) and / or max_voxel_age (inserts): a sliding window — after each insert
    the store is pruned (VoxelMap.prune) to the box pose.t ± window_half_extent and / or to the voxels touched within the
    last max_voxel_age inserts; with both None nothing is pruned.
    filter_voxel_size: each frame's scan is voxel-filtered on the device (Scan.filtered, the harness's FilterPoints, :91)
    and the filtered scan is registered, while the FULL scan is inserted — the harness builds its map from all points and
    registers the filtered ones (:81, :91-92); insert_filtered=True inserts the filtered scan instead.  The filtered scan
    is closed after the frame.  None: the scans are registered and inserted as they are.
    live_match=True: no snapshot is taken; every round matches against the store itself (VoxelMap.match), so no step
    of a frame passes over the whole map.  Same poses and rounds, bit for bit.
    one_launch=True: each frame's registration is ONE batched call of one problem against the live store
    (scan_to_map_batch on the VoxelMap): all rounds in one launch with one host wait, instead of a match and a solve
    launch and their waits per round — what a frame of a small (filtered) scan is made of.  Implies live_match.  Takes
    loss, options, max_outer_iterations, dof, dtype and keep_multiple; indexed, on_solve, device_loop=False and an explicit
    live_match=False raise ValueError.  A frame whose registration fails raises RuntimeError as scan_to_map does, before
    anything is inserted.  Same poses and rounds as live_match=True, bit for bit, for scans of ≤ 512 points; to rounding
    above, where the lone path is also the faster one.
    live_indexed=True: every round matches through VoxelMap.match_indexed (scan_to_map's live_indexed: the voxel-indexed
    layout with a compact table, no snapshot).  Implies live_match; an explicit live_match=False raises ValueError.  Same
    poses and rounds, bit for bit, as odometry(indexed=True) on the snapshot route.  Not a keyword of one_launch=True.
    sweep_times: a sequence of one time array per scan (indexed like the scan's `order`): every frame is first motion-
    compensated on the device (Scan.deskewed) and the deskewed scan takes the raw scan's place for the
    filter, the registration and the insert; it is closed after the frame, also when an exception leaves.  Convention:
    times are in units of one sweep period; a frame's pose is the sensor pose at its reference instant, the time
    sweep_reference of its own array (1.0: the end of the sweep); consecutive reference instants are 1.0 apart.  Frame k
    is deskewed with the constant-velocity twist pose_twist(poses[k-2], poses[k-1]), frames 0 and 1 with zero.  The
    start pose of a frame's registration stays the previous pose.  None: nothing is deskewed.
    carve: a dict of VoxelMap.carve keywords (may be empty) — every frame, after the registration and before the insert,
    the store is carved along the rays of the scan about to be inserted, at the pose found (line of sight):
    what stood in front of the sensor for a few frames (a car, a person, a door) goes once the sensor sees through it.
    The inserted scan is the carving scan, so every cell the insert will touch is protected by its own hits.  Caveats.
    Deskewed frames: the ray origin is the sensor at the frame's reference instant, while the true origins differ by the
    motion within the sweep — end_margin has to cover that.  Grazing rays skim the cells of the surface they end on:
    min_crossings and the hit protection are the guards.  None: nothing is carved, bit for bit.
    place_db: an api.PlaceDatabase — the Scan Context descriptor of every frame that was registered is appended to it (on
    the device), built from the scan the frame registers, after the deskew and before the filter, and added once the
    registration has succeeded: an empty database's index of a frame is then its index in the returned poses, ready for
    loop_candidates.  None: nothing is added, bit for bit.
    tiles: a TileCache, only together with window_half_extent — the window becomes a cache over a larger map (DESIGN.md
    §31).  After each pose the voxels the prune is about to remove are paged out (tiles.put(VoxelMap.export(...,
    removed=True))), the prune runs as it always did, and every cached tile that meets the new window is paged back in
    (VoxelMap.add(tiles.take(...)), the window's cells by the prune's own bounds): when the vehicle returns to a place the
    map there is what it was, count and sums bit for bit, instead of empty.  Whole tiles come back, so voxels of a tile
    that reach beyond the window travel in and out until the window has passed; what is paged in is stamped as touched.
    None: nothing is exported or added, bit for bit.
    → (list of Poses, list of per-scan round lists)."""
    if tiles is not None and window_half_extent is None:
        raise ValueError("tiles pages voxels in and out of the window: it needs window_half_extent")
    if live_indexed:
        if live_match is not None and not live_match:
            raise ValueError("live_indexed=True matches against the live store: live_match=False contradicts it")
        scan_to_map_kwargs["live_indexed"] = True  # with one_launch=True: its unknown-keyword TypeError below
        live_match = True
    if one_launch:
        if live_match is not None and not live_match:
            raise ValueError("one_launch=True registers against the live store: live_match=False contradicts it")
        if scan_to_map_kwargs.get("indexed"):
            raise ValueError("one_launch=True: there is no voxel-indexed match against a VoxelMap")
        if scan_to_map_kwargs.get("on_solve") is not None:
            raise ValueError("one_launch=True: the rounds run inside one launch, on_solve cannot be called between them")
        if not scan_to_map_kwargs.get("device_loop", True):
            raise ValueError("one_launch=True: the LM loop runs on the device, device_loop=False contradicts it")
        unknown = sorted(set(scan_to_map_kwargs) - set(_ONE_LAUNCH_KWARGS) - {"indexed", "on_solve", "device_loop"})
        if unknown:
            raise TypeError("one_launch=True does not take %s" % ", ".join(unknown))
        batch_kwargs = {k: v for k, v in scan_to_map_kwargs.items() if k in _ONE_LAUNCH_KWARGS}
    live_match = bool(live_match) or one_launch
    pose = Pose() if initial_pose is None else Pose(initial_pose.R, initial_pose.t)
    windowed = window_half_extent is not None or max_voxel_age is not None
    poses, all_rounds = [], []
    for k, scan in enumerate(scans):
        raw = scan
        if sweep_times is not None:  # constant velocity: the last frame-to-frame motion goes on through this sweep
            twist = pose_twist(poses[k - 2], poses[k - 1]) if k >= 2 else np.zeros(6)
            scan = raw.deskewed(sweep_times[k], twist, sweep_reference)
        registered = scan
        try:
            if filter_voxel_size is not None:
                registered = scan.filtered(filter_voxel_size)
            ndt_map = voxel_map if live_match else voxel_map.snapshot()
            try:
                if one_launch:
                    row = scan_to_map_batch(ctx, voxel_map, [registered], [pose], **batch_kwargs)[0]
                    if row is None:
                        raise RuntimeError("SolveDataset failed (a round of the one-launch registration returned ok = 0)")
                    pose, rounds, _ = row
                else:
                    pose, rounds, _ = scan_to_map(ctx, ndt_map, registered, initial_pose=pose, **scan_to_map_kwargs)
            finally:
                if not live_match:
                    ndt_map.close()
            inserted = registered if insert_filtered else scan
            if carve is not None:
                voxel_map.carve(inserted, pose.R, pose.t, **carve)
            voxel_map.insert_scan(inserted, pose.R, pose.t)
            if place_db is not None:
                place_db.add(scan)
        finally:
            if registered is not scan:
                registered.close()
            if scan is not raw:
                scan.close()
        if windowed:
            box = window_half_extent is not None
            if tiles is not None:
                tiles.put(voxel_map.export(center=pose.t, half_extent=window_half_extent, max_age=max_voxel_age, removed=True))
            voxel_map.prune(center=pose.t if box else None, half_extent=window_half_extent if box else None,
                            max_age=max_voxel_age)
            if tiles is not None and len(tiles):
                # the window in cells, as the prune bounds it: floor((center -+ half_extent) * (1 / resolution))
                c, h = np.asarray(pose.t, dtype=np.float64).reshape(3), np.asarray(window_half_extent, dtype=np.float64)
                inv_res = 1.0 / voxel_map.voxel_resolution
                paged = tiles.take(np.floor((c - h) * inv_res), np.floor((c + h) * inv_res))
                if paged["counts"].size:
                    voxel_map.add(paged)
        poses.append(Pose(pose.R, pose.t))
        all_rounds.append(rounds)
    return poses, all_rounds


def compose_map(ctx, submaps, poses, voxel_resolution=None, search_radius_sq=None, proper_sqrt_information=True, capacity=0):
    """The global map from submaps at their current pose estimates — e.g. rebuilt after PoseGraph.optimize has corrected
    the trajectory, without the raw scans: every api.VoxelMap of `submaps` is merged under its pose (VoxelMap.merge, map
    point = R p + t), in list order, into a fresh VoxelMap.  poses: one Pose (or (R, t) pair) per submap.  voxel_resolution
    and search_radius_sq default to the first submap's.  → the new VoxelMap, the caller's to close; on an error it is
    closed before the exception leaves.  The submaps are not modified."""
    submaps, poses = list(submaps), list(poses)
    if len(submaps) != len(poses):
        raise ValueError("%d submaps but %d poses" % (len(submaps), len(poses)))
    if not submaps and (voxel_resolution is None or search_radius_sq is None):
        raise ValueError("without submaps, voxel_resolution and search_radius_sq have to be given")
    res = submaps[0].voxel_resolution if voxel_resolution is None else voxel_resolution
    radius = submaps[0].search_radius_sq if search_radius_sq is None else search_radius_sq
    out = VoxelMap(ctx, res, radius, proper_sqrt_information=proper_sqrt_information, capacity=capacity)
    try:
        for sub, pose in zip(submaps, poses):
            R, t = (pose.R, pose.t) if hasattr(pose, "R") else pose
            out.merge(sub, R, t)
    except Exception:
        out.close()
        raise
    return out
