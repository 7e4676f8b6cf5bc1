"""Thin Python handles over the C ABI (include/nos.h): Context, NdtDataset, ReprojDataset.

numpy arrays go in and out; torch is optional (import it BEFORE creating the first Context if it is going to be
used in the same process: torch bundles its own HIP runtime with the system runtime's soname, and the first one
loaded serves the whole process) and only used for device-resident planes
(`from_device_planes`) and for device-resident results (`*_async`), i.e. as plumbing for
device memory, streams and torch.distributed — all arithmetic happens in libnos_hip.so.
"""
import ctypes
import sys
import weakref

import numpy as np

from . import _lib
from ._lib import (NOS_F32, NOS_F64, NOS_LOSS_EXPONENTIAL, NOS_LOSS_HUBER, NOS_LOSS_NONE,
                   NosLoss, c_double_p, c_void_pp, check, hip_lib)

_DTYPES = {"f64": NOS_F64, "f32": NOS_F32, NOS_F64: NOS_F64, NOS_F32: NOS_F32}


def make_loss(loss):
    """None | ("none",) | ("exponential", c1, c2) | ("huber", threshold) → NosLoss.

    Mirrors the constructors of the reference's loss_function.h (ExponentialLossFunction(c1, c2),
    HuberLossFunction(threshold)); argument validation happens inside the C ABI.
    """
    if loss is None or loss[0] == "none":
        return NosLoss(NOS_LOSS_NONE, 0, 0.0, 0.0)
    if loss[0] == "exponential":
        return NosLoss(NOS_LOSS_EXPONENTIAL, 0, float(loss[1]), float(loss[2]))
    if loss[0] == "huber":
        return NosLoss(NOS_LOSS_HUBER, 0, float(loss[1]), 0.0)
    raise ValueError("unknown loss %r" % (loss,))


def _dvec(x, n):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
    if a.size != n:
        raise ValueError("expected %d doubles, got %d" % (n, a.size))
    return a


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def runtime_info():
    """Where the HIP runtime and librccl mapped into this process come from (nos_runtime_info) → dict."""
    import json
    buf = ctypes.create_string_buffer(4096)
    check(hip_lib().nos_runtime_info(buf, 4096), "nos_runtime_info")
    return json.loads(buf.value.decode())


def new_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, all ranks pass it to Context.comm_init)."""
    buf = ctypes.create_string_buffer(128)
    check(hip_lib().nos_comm_get_unique_id(buf), "nos_comm_get_unique_id")
    return buf.raw


def shm_unlink(name):
    check(hip_lib().nos_comm_shm_unlink(name.encode()), "nos_comm_shm_unlink")


class Context:
    """nos_ctx: one HIP stream + workspace per listed device (include/nos.h)."""

    def __init__(self, device_ids=(0,)):
        self._lib = hip_lib()
        ids = (ctypes.c_int * len(device_ids))(*device_ids)
        h = ctypes.c_void_p()
        check(self._lib.nos_ctx_create(ids, len(device_ids), ctypes.byref(h)), "nos_ctx_create")
        self._h = h
        self.device_ids = tuple(device_ids)
        self._children = weakref.WeakSet()  # datasets / maps / scans living on this context

    def _adopt(self, child):
        self._children.add(child)

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_ptr, shard=0):
        check(self._lib.nos_ctx_set_stream(self._h, shard, ctypes.c_void_p(stream_ptr)), "nos_ctx_set_stream")

    def use_torch_stream(self, shard=0):
        import torch
        self.set_stream(torch.cuda.current_stream().cuda_stream, shard)

    def set_launch(self, blocks_per_cu=0, variant=0):
        check(self._lib.nos_ctx_set_launch(self._h, blocks_per_cu, variant), "nos_ctx_set_launch")

    def set_option(self, key, value):
        """Experiment knob of the context (include/nos.h, "experiment knobs"): e.g. set_option("lm_cluster", 0)."""
        check(self._lib.nos_ctx_set_option(self._h, key.encode(), int(value)), "nos_ctx_set_option")

    def get_option(self, key):
        v = ctypes.c_int()
        check(self._lib.nos_ctx_get_option(self._h, key.encode(), ctypes.byref(v)), "nos_ctx_get_option")
        return v.value

    def options(self, **kv):
        """with ctx.options(lm_cluster=0, lm_single=0): ... — set for the block, restored afterwards."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {k: self.get_option(k) for k in kv}
            try:
                for k, v in kv.items():
                    self.set_option(k, v)
                yield self
            finally:
                for k, v in old.items():
                    self.set_option(k, v)
        return scope()

    @property
    def comm_rccl_count(self):
        """Ranks RCCL reports for this context's communicator (ncclCommCount); 0 without an RCCL communicator."""
        v = ctypes.c_int()
        check(self._lib.nos_ctx_comm_rccl_count(self._h, ctypes.byref(v)), "nos_ctx_comm_rccl_count")
        return v.value

    def comm_init(self, n_ranks, rank, unique_id):
        """Collective: join the RCCL communicator identified by the 128-byte unique_id."""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        check(self._lib.nos_ctx_comm_init(self._h, n_ranks, rank, buf), "nos_ctx_comm_init")

    def comm_init_from_torch(self, group=None):
        """Bootstrap the native RCCL communicator through an initialised torch.distributed group:
        rank 0 creates the unique id, broadcasts it, every rank joins."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        payload = [new_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(payload, src=0, group=group)
        self.comm_init(world, rank, payload[0])

    def comm_init_shm(self, n_ranks, rank, name, device_memory=False):
        """Collective (ranks of one node): join the mailbox communicator `name` ('/...'); the sums are then exchanged
        inside the launch.  device_memory=False: slots in the POSIX shared-memory segment (nos_ctx_comm_init_shm);
        True: slots in fine-grained device memory of every rank, shared through HIP IPC handles — peers write into each
        other's buffers device to device (nos_ctx_comm_init_shm_device)."""
        if device_memory:
            check(self._lib.nos_ctx_comm_init_shm_device(self._h, n_ranks, rank, name.encode()), "nos_ctx_comm_init_shm_device")
        else:
            check(self._lib.nos_ctx_comm_init_shm(self._h, n_ranks, rank, name.encode()), "nos_ctx_comm_init_shm")

    def comm_init_shm_from_torch(self, group=None, device_memory=False):
        """Bootstrap the mailbox communicator through an initialised torch.distributed group: rank 0 picks a fresh
        name, every rank attaches, rank 0 unlinks the name once all are in (the mapping stays alive)."""
        import torch.distributed as dist
        import uuid
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        payload = ["/nos_%s" % uuid.uuid4().hex if rank == 0 else None]
        dist.broadcast_object_list(payload, src=0, group=group)
        try:
            self.comm_init_shm(world, rank, payload[0], device_memory=device_memory)
        finally:
            dist.barrier(group=group)
            if rank == 0:
                shm_unlink(payload[0])

    def comm_destroy(self):
        check(self._lib.nos_ctx_comm_destroy(self._h), "nos_ctx_comm_destroy")

    @property
    def comm_size(self):
        return int(self._lib.nos_ctx_comm_size(self._h))

    def comm_allreduce(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(self._lib.nos_ctx_comm_allreduce(self._h, _dp(v), v.size), "nos_ctx_comm_allreduce")
        return v

    def last_kernel(self, shard=0):
        """Demangled symbol of the hot-path kernel launched last on this context (nos_ctx_last_kernel)."""
        buf = ctypes.create_string_buffer(1024)
        check(self._lib.nos_ctx_last_kernel(self._h, shard, buf, len(buf)), "nos_ctx_last_kernel")
        return buf.value.decode()

    def profile_begin(self, max_launches=4096, sample_every=1):
        check(self._lib.nos_ctx_profile_begin(self._h, max_launches, sample_every), "nos_ctx_profile_begin")

    def profile_end(self):
        """→ (n_launches, mean_ms, min_ms, max_ms) of the assemble kernels launched since profile_begin."""
        n = ctypes.c_int()
        mean = ctypes.c_double()
        lo = ctypes.c_double()
        hi = ctypes.c_double()
        check(self._lib.nos_ctx_profile_end(self._h, ctypes.byref(n), ctypes.byref(mean), ctypes.byref(lo),
                                            ctypes.byref(hi)), "nos_ctx_profile_end")
        return n.value, mean.value, lo.value, hi.value

    def synchronize(self):
        check(self._lib.nos_ctx_synchronize(self._h), "nos_ctx_synchronize")

    def close(self):
        if self._h:
            for child in list(self._children):  # device objects must not outlive their context
                child.close()
            self._lib.nos_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def _lm_call(fn, where, pre_args, post_args, R, t, max_iterations, gradient_tolerance, parameter_tolerance,
             launches_in_flight):
    """Shared body of the device-resident solve methods: returns (R, t, report dict)."""
    from ._lib import NosLmOptions, NosLmReport
    hist = np.full(max(int(max_iterations), 1), np.nan)
    opt = NosLmOptions(int(max_iterations), int(launches_in_flight), float(gradient_tolerance),
                       float(parameter_tolerance), _dp(hist))
    rep = NosLmReport()
    check(fn(*pre_args, _dp(R), _dp(t), *post_args, ctypes.byref(opt), ctypes.byref(rep)), where)
    return R, t, _lm_report(rep, hist[:max(int(max_iterations), 0)])


def _lm_report(rep, hist_row):
    """The report dict of one solve: a NosLmReport and its row of the cost history (NaN where no iteration ran)."""
    executed = int(np.count_nonzero(~np.isnan(hist_row)))
    return {"iterations": rep.iterations, "ok": bool(rep.ok), "launches": rep.launches, "fallback": bool(rep.fallback),
            "printed_cost": rep.printed_cost, "last_cost": rep.last_cost, "final_lambda": rep.final_lambda,
            "cost_history": hist_row[:executed].copy()}


def _poses(R, t, B, nR, nt, copy):
    """The poses of a batched call as contiguous R [B, nR] and t [B, nt]; copy: the call writes them, the inputs stay."""
    R = np.array(R, dtype=np.float64) if copy else np.asarray(R, dtype=np.float64)
    t = np.array(t, dtype=np.float64) if copy else np.asarray(t, dtype=np.float64)
    if R.size != B * nR or t.size != B * nt:
        got = "%s and %s" % (R.shape, t.shape) if copy else "%d and %d values" % (R.size, t.size)
        raise ValueError("expected R [%d, %d] and t [%d, %d], got %s" % (B, nR, B, nt, got))
    return np.ascontiguousarray(R.reshape(B, nR)), np.ascontiguousarray(t.reshape(B, nt))


def _handles(objs):
    """The handle array a batched entry point takes (never of length 0)."""
    return (ctypes.c_void_p * max(len(objs), 1))(*[o._h for o in objs])


def _batch_call(fn, where, datasets, R, t, nR, nt, post_args, max_iterations, gradient_tolerance, parameter_tolerance):
    """Shared body of the batched solves: returns (R [B, nR], t [B, nt], [B report dicts shaped like _lm_call's])."""
    from ._lib import NosLmOptions, NosLmReport
    datasets = list(datasets)
    B = len(datasets)
    R, t = _poses(R, t, B, nR, nt, copy=True)
    m = max(int(max_iterations), 1)
    hist = np.full((B, m), np.nan)  # row i starts at i * max_iterations
    opt = NosLmOptions(int(max_iterations), 0, float(gradient_tolerance), float(parameter_tolerance), _dp(hist))
    reps = (NosLmReport * max(B, 1))()
    check(fn(_handles(datasets), B, _dp(R), _dp(t), *post_args, ctypes.byref(opt), reps), where)
    return R, t, [_lm_report(reps[i], hist[i, :max(int(max_iterations), 0)]) for i in range(B)]


def solve6_batch(datasets, R, t, loss=None, max_iterations=100, gradient_tolerance=1e-6, parameter_tolerance=1e-6):
    """B independent 6-DoF NDT solves, the small ones in one launch (nos_ndt6_solve_batch).  datasets: B NdtDatasets of one
    context and element type (the same one may repeat); R [B, 9] or [B, 3, 3], t [B, 3].  Row i equals
    datasets[i].solve6(R[i], t[i], ...).  Returns (R [B, 9], t [B, 3], [B reports])."""
    l = make_loss(loss)
    return _batch_call(hip_lib().nos_ndt6_solve_batch, "nos_ndt6_solve_batch", datasets, R, t, 9, 3, (ctypes.byref(l),),
                       max_iterations, gradient_tolerance, parameter_tolerance)


def solve3_batch(datasets, R2, t2, loss=None, max_iterations=100, gradient_tolerance=1e-6, parameter_tolerance=1e-6):
    """B independent planar NDT solves (nos_ndt3_solve_batch): R2 [B, 4] or [B, 2, 2], t2 [B, 2].
    Returns (R2 [B, 4], t2 [B, 2], [B reports])."""
    l = make_loss(loss)
    return _batch_call(hip_lib().nos_ndt3_solve_batch, "nos_ndt3_solve_batch", datasets, R2, t2, 4, 2, (ctypes.byref(l),),
                       max_iterations, gradient_tolerance, parameter_tolerance)


def reproj_solve_batch(datasets, R, t, intr, loss=None, min_depth=0.03, max_iterations=100, gradient_tolerance=1e-6,
                       parameter_tolerance=1e-6):
    """B independent reprojection solves (nos_reproj_solve_batch): R [B, 9] or [B, 3, 3], t [B, 3]; intr [B, 4], or [4] for
    every problem.  Returns (R [B, 9], t [B, 3], [B reports])."""
    B = len(datasets)
    intr = np.asarray(intr, dtype=np.float64)
    intr = np.ascontiguousarray(np.broadcast_to(intr, (B, 4)) if intr.shape == (4,) else intr.reshape(B, 4))
    l = make_loss(loss)
    return _batch_call(hip_lib().nos_reproj_solve_batch, "nos_reproj_solve_batch", datasets, R, t, 9, 3,
                       (_dp(intr), ctypes.byref(l), ctypes.c_double(min_depth)), max_iterations, gradient_tolerance,
                       parameter_tolerance)


def _register_call(fn, where, ndt_map, scans, R, t, loss, max_outer_iterations, keep_multiple, max_neighbors, dtype,
                   max_iterations, gradient_tolerance, parameter_tolerance):
    """Shared body of the batched registrations: returns (R [B, 9], t [B, 3], [B report dicts])."""
    from ._lib import NosLmOptions, NosRegisterOptions, NosRegisterReport, NosRegisterRound
    scans = list(scans)
    B = len(scans)
    R, t = _poses(R, t, B, 9, 3, copy=True)
    m = max(int(max_outer_iterations), 1)
    log = (NosRegisterRound * (max(B, 1) * m))()  # row i starts at i * max_outer_iterations
    ropt = NosRegisterOptions(int(max_outer_iterations), int(max_neighbors), int(keep_multiple or 0), _DTYPES[dtype], log)
    opt = NosLmOptions(int(max_iterations), 0, float(gradient_tolerance), float(parameter_tolerance), None)
    reps = (NosRegisterReport * max(B, 1))()
    l = make_loss(loss)
    check(fn(ndt_map._h, _handles(scans), B, _dp(R), _dp(t), ctypes.byref(l), ctypes.byref(ropt), ctypes.byref(opt), reps), where)
    out = []
    for i in range(B):
        rep = reps[i]
        rounds = [{"matches": int(e.matches), "used": int(e.used), "iterations": int(e.iterations), "ok": bool(e.ok),
                   "printed_cost": float(e.printed_cost), "last_cost": float(e.last_cost)}
                  for e in log[i * m:i * m + rep.rounds]]
        out.append({"outer_iter": rep.outer_iter, "rounds": rounds, "ok": bool(rep.ok)})
    return R, t, out


def _register_entry(ndt_map, dof):
    """The C entry point of a batched registration by the kind of map: an NdtMap, or a VoxelMap (the live store)."""
    name = ("nos_voxel_map_register%d_batch" if isinstance(ndt_map, VoxelMap) else "nos_ndt%d_register_batch") % dof
    return getattr(hip_lib(), name), name  # a library without the symbol: AttributeError, no other route is tried


def register6_batch(ndt_map, scans, R, t, loss, max_outer_iterations=10, keep_multiple=None, max_neighbors=2, dtype="f64",
                    max_iterations=40, gradient_tolerance=1e-6, parameter_tolerance=1e-6):
    """B scan-to-map registrations against one map in one launch (nos_ndt6_register_batch): every round's matching, tail
    drop (keep_multiple), LM solve and stopping test run on the device.  scans: B Scans of the map's context (the same one
    may repeat: multi-start); R [B, 9] or [B, 3, 3], t [B, 3] start poses.  Row i equals pipeline.scan_to_map from
    (R[i], t[i]).  Returns (R [B, 9], t [B, 3], [B reports {outer_iter, rounds: [per-round dicts], ok}]).
    ndt_map: an NdtMap, or a VoxelMap — every round is then matched against the live store inside the same launch
    (nos_voxel_map_register6_batch): no snapshot, and row i is bit for bit the row of the call on its snapshot()."""
    fn, name = _register_entry(ndt_map, 6)
    return _register_call(fn, name, ndt_map, scans, R, t, loss, max_outer_iterations, keep_multiple, max_neighbors, dtype,
                          max_iterations, gradient_tolerance, parameter_tolerance)


def register3_batch(ndt_map, scans, R, t, loss, max_outer_iterations=10, keep_multiple=None, max_neighbors=2, dtype="f64",
                    max_iterations=40, gradient_tolerance=1e-6, parameter_tolerance=1e-6):
    """Planar form (nos_ndt3_register_batch; for a VoxelMap nos_voxel_map_register3_batch): R [B, 9], t [B, 3] are full
    3-D poses; every round solves for the top-left 2x2 and (x, y) and writes only those back, as the 3-DoF drop-in class
    does."""
    fn, name = _register_entry(ndt_map, 3)
    return _register_call(fn, name, ndt_map, scans, R, t, loss, max_outer_iterations, keep_multiple, max_neighbors, dtype,
                          max_iterations, gradient_tolerance, parameter_tolerance)


SCORE_CHUNK_POINTS = 1024  # kScoreChunkPoints of csrc/score_kernels.hpp: points per workgroup of a score call
SCORE_DTYPE = np.dtype([("matches", np.uint64), ("matched_points", np.uint64), ("cost", np.float64),
                        ("reserved", np.float64)])  # nos_pose_score


def _score_entry(ndt_map):
    """The C entry point of a score call by the kind of map, as _register_entry."""
    name = "nos_voxel_map_score_batch" if isinstance(ndt_map, VoxelMap) else "nos_ndt_score_batch"
    return getattr(hip_lib(), name), name  # a library without the symbol: AttributeError, no other route is tried


def score_batch(ndt_map, scans, R, t, loss, max_neighbors=2):
    """How well scans[b] fits the map at (R[b], t[b]), for B problems in one call (nos_ndt_score_batch; for a VoxelMap
    nos_voxel_map_score_batch, against the live store).  scans: B Scans of the map's context (the same one may repeat:
    one scan, many poses); R [B, 9] or [B, 3, 3], t [B, 3].  → structured array [B] with fields matches (what
    match(...) counts), matched_points (points with at least one match) and cost (Σ ρ, the [27] of match(..., "f64")
    + accumulate6: the same terms bit for bit, summed in a fixed order that depends on the scan's size alone).  A row does
    not depend on B, on its position or on the other rows."""
    scans = list(scans)
    B = len(scans)
    R, t = _poses(R, t, B, 9, 3, copy=False)
    out = np.zeros(max(B, 1), dtype=SCORE_DTYPE)
    fn, name = _score_entry(ndt_map)
    l = make_loss(loss)
    check(fn(ndt_map._h, _handles(scans), B, _dp(R), _dp(t), ctypes.byref(l), int(max_neighbors),
             out.ctypes.data_as(ctypes.POINTER(_lib.NosPoseScore))), name)
    rows = np.zeros(B, dtype=[(f, SCORE_DTYPE[f]) for f in ("matches", "matched_points", "cost")])  # packed: 24 bytes
    for field in rows.dtype.names:
        rows[field] = out[field][:B]
    return rows


class _Dataset:
    _n_planes = 0
    _create = _create_dev = _create_rec = None

    def __init__(self, ctx, handle):
        self._ctx = ctx
        self._lib = ctx._lib
        self._h = handle
        ctx._adopt(self)

    @classmethod
    def from_planes(cls, ctx, planes, dtype="f64"):
        """planes: [n_planes, n] float64 host array (plane order of include/nos.h)."""
        planes = np.ascontiguousarray(planes, dtype=np.float64)
        if planes.ndim != 2 or planes.shape[0] != cls._n_planes:
            raise ValueError("planes must be [%d, n]" % cls._n_planes)
        arr = (c_double_p * cls._n_planes)(*[planes[k].ctypes.data_as(c_double_p) for k in range(cls._n_planes)])
        h = ctypes.c_void_p()
        fn = getattr(ctx._lib, cls._create)
        check(fn(ctx.handle, planes.shape[1], arr, _DTYPES[dtype], ctypes.byref(h)), cls._create)
        return cls(ctx, h)

    @classmethod
    def from_device_planes(cls, ctx, planes, dtype="f64"):
        """planes: torch CUDA tensor [n_planes, n], float64 or float32, contiguous."""
        import torch
        if not planes.is_cuda or planes.dim() != 2 or planes.shape[0] != cls._n_planes or not planes.is_contiguous():
            raise ValueError("planes must be a contiguous CUDA tensor [%d, n]" % cls._n_planes)
        src = NOS_F64 if planes.dtype == torch.float64 else NOS_F32
        if planes.dtype not in (torch.float64, torch.float32):
            raise ValueError("planes must be float64 or float32")
        n = planes.shape[1]
        step = planes.element_size() * n
        arr = (ctypes.c_void_p * cls._n_planes)(*[planes.data_ptr() + k * step for k in range(cls._n_planes)])
        h = ctypes.c_void_p()
        torch.cuda.current_stream().synchronize()
        fn = getattr(ctx._lib, cls._create_dev)
        check(fn(ctx.handle, n, arr, src, _DTYPES[dtype], ctypes.byref(h)), cls._create_dev)
        return cls(ctx, h)

    @classmethod
    def from_records(cls, ctx, records, stride_bytes, field_offsets, dtype="f64"):
        """records: host bytes-like / uint8 array of n*stride_bytes; field_offsets: byte offsets
        of the n_planes doubles inside a record (AoS ingestion, include/nos.h)."""
        rec = np.ascontiguousarray(np.frombuffer(records, dtype=np.uint8) if not isinstance(records, np.ndarray)
                                   else records.view(np.uint8).reshape(-1))
        if rec.size % stride_bytes != 0:
            raise ValueError("records size is not a multiple of stride_bytes")
        n = rec.size // stride_bytes
        offs = (ctypes.c_size_t * cls._n_planes)(*[int(o) for o in field_offsets])
        h = ctypes.c_void_p()
        fn = getattr(ctx._lib, cls._create_rec)
        check(fn(ctx.handle, n, rec.ctypes.data_as(ctypes.c_void_p), stride_bytes, offs, _DTYPES[dtype],
                 ctypes.byref(h)), cls._create_rec)
        return cls(ctx, h)

    def __len__(self):
        return int(self._lib.nos_dataset_size(self._h))

    @property
    def stream_bytes(self):
        return int(self._lib.nos_dataset_stream_bytes(self._h))

    def set_simd_class(self, on=True):
        """Semantics of the reference's fp32 ("SIMD") solver classes for this dataset (nos_dataset_set_simd_class): NDT —
        float lambda / previous_cost in the LM loop; reprojection — depth > 0 mask on the weight only.  The tail drop
        (first floor(N/8)*8 correspondences) is the caller's: create the dataset from that prefix."""
        check(self._lib.nos_dataset_set_simd_class(self._h, int(bool(on))), "nos_dataset_set_simd_class")
        return self

    @property
    def dtype(self):
        return "f32" if self._lib.nos_dataset_dtype(self._h) == NOS_F32 else "f64"

    def close(self):
        if self._h:
            self._lib.nos_dataset_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class NdtDataset(_Dataset):
    """Device-resident NDT correspondences (point, mean, sqrt-information)."""
    _n_planes = 15
    _create = "nos_ndt_dataset_create"
    _create_dev = "nos_ndt_dataset_create_from_device"
    _create_rec = "nos_ndt_dataset_create_from_records"

    def drop_last_matches(self, n_drop):
        """Clear the last n_drop non-empty records (slot order) of a matcher-written dataset: the tail drop of the
        reference's solver classes, e.g. n_matches % 4 for the scalar 3-DoF class (nos_dataset_drop_last_matches)."""
        check(self._lib.nos_dataset_drop_last_matches(self._h, int(n_drop)), "nos_dataset_drop_last_matches")

    def accumulate6(self, R, t, loss=None):
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        out = np.zeros(28)
        l = make_loss(loss)
        check(self._lib.nos_ndt6_accumulate(self._h, _dp(R), _dp(t), ctypes.byref(l), _dp(out)), "nos_ndt6_accumulate")
        return out

    def solve6(self, R, t, loss=None, max_iterations=100, gradient_tolerance=1e-6, parameter_tolerance=1e-6,
               launches_in_flight=0):
        """Whole LM loop on the device (nos_ndt6_solve).  Returns (R[9], t[3], report)."""
        R = _dvec(R, 9).copy()
        t = _dvec(t, 3).copy()
        l = make_loss(loss)
        return _lm_call(self._lib.nos_ndt6_solve, "nos_ndt6_solve", (self._h,), (ctypes.byref(l),), R, t,
                        max_iterations, gradient_tolerance, parameter_tolerance, launches_in_flight)

    def solve3(self, R2, t2, loss=None, max_iterations=100, gradient_tolerance=1e-6, parameter_tolerance=1e-6,
               launches_in_flight=0):
        """Planar LM loop on the device (nos_ndt3_solve).  Returns (R2[4], t2[2], report)."""
        R2 = _dvec(R2, 4).copy()
        t2 = _dvec(t2, 2).copy()
        l = make_loss(loss)
        return _lm_call(self._lib.nos_ndt3_solve, "nos_ndt3_solve", (self._h,), (ctypes.byref(l),), R2, t2,
                        max_iterations, gradient_tolerance, parameter_tolerance, launches_in_flight)

    def accumulate6_async(self, R, t, loss, out_tensor):
        """Enqueue on the context stream; result lands in the CUDA float64 tensor out_tensor[28]."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        l = make_loss(loss)
        check(self._lib.nos_ndt6_accumulate_async(self._h, _dp(R), _dp(t), ctypes.byref(l),
                                                  ctypes.c_void_p(out_tensor.data_ptr())), "nos_ndt6_accumulate_async")

    def accumulate3(self, R2, t2, loss=None):
        R2 = _dvec(R2, 4)
        t2 = _dvec(t2, 2)
        out = np.zeros(10)
        l = make_loss(loss)
        check(self._lib.nos_ndt3_accumulate(self._h, _dp(R2), _dp(t2), ctypes.byref(l), _dp(out)), "nos_ndt3_accumulate")
        return out

    def accumulate3_async(self, R2, t2, loss, out_tensor):
        R2 = _dvec(R2, 4)
        t2 = _dvec(t2, 2)
        l = make_loss(loss)
        check(self._lib.nos_ndt3_accumulate_async(self._h, _dp(R2), _dp(t2), ctypes.byref(l),
                                                  ctypes.c_void_p(out_tensor.data_ptr())), "nos_ndt3_accumulate_async")

    def time_kernel6(self, R, t, loss=None, repeats=20):
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        l = make_loss(loss)
        k = ctypes.c_double()
        tot = ctypes.c_double()
        check(self._lib.nos_ndt6_time_kernel(self._h, _dp(R), _dp(t), ctypes.byref(l), repeats, ctypes.byref(k),
                                             ctypes.byref(tot)), "nos_ndt6_time_kernel")
        return k.value, tot.value

    def time_kernel3(self, R2, t2, loss=None, repeats=20):
        R2 = _dvec(R2, 4)
        t2 = _dvec(t2, 2)
        l = make_loss(loss)
        k = ctypes.c_double()
        tot = ctypes.c_double()
        check(self._lib.nos_ndt3_time_kernel(self._h, _dp(R2), _dp(t2), ctypes.byref(l), repeats, ctypes.byref(k),
                                             ctypes.byref(tot)), "nos_ndt3_time_kernel")
        return k.value, tot.value


class NdtIndexedDataset(NdtDataset):
    """Voxel-indexed NDT correspondences: points [3,n] + voxel ids [K,n] (-1 = none) + a voxel table
    (means [V,3], sqrt-informations [V,3,3]).  Same accumulate6 / accumulate3 interface and the same sums as
    the flat NdtDataset, at 24 B + 4 B·K per point instead of 120 B per correspondence (include/nos.h)."""
    _n_planes = 3  # what nos_dataset_download returns for this kind: the (voxel-sorted) point planes

    @classmethod
    def from_arrays(cls, ctx, points, index, means, sqrt_infos, dtype="f64", sort_by_voxel=True):
        points = np.ascontiguousarray(points, dtype=np.float64)
        index = np.ascontiguousarray(np.atleast_2d(index), dtype=np.int32)
        means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1, 3)
        S = np.ascontiguousarray(sqrt_infos, dtype=np.float64).reshape(-1, 9)
        if points.ndim != 2 or points.shape[0] != 3 or index.shape[1] != points.shape[1]:
            raise ValueError("points must be [3, n] and index [K, n]")
        K, n = index.shape
        pp = (c_double_p * 3)(*[points[k].ctypes.data_as(c_double_p) for k in range(3)])
        ip_t = ctypes.POINTER(ctypes.c_int32)
        ip = (ip_t * K)(*[index[k].ctypes.data_as(ip_t) for k in range(K)])
        h = ctypes.c_void_p()
        check(ctx._lib.nos_ndt_indexed_dataset_create(ctx.handle, n, pp, K, ip, means.shape[0], _dp(means), _dp(S),
                                                      _DTYPES[dtype], int(bool(sort_by_voxel)), ctypes.byref(h)),
              "nos_ndt_indexed_dataset_create")
        return cls(ctx, h)

    def _indexed_info(self):
        k, v = ctypes.c_int(), ctypes.c_size_t()
        check(self._lib.nos_indexed_dataset_info(self._h, ctypes.byref(k), ctypes.byref(v)), "nos_indexed_dataset_info")
        return int(k.value), int(v.value)

    @property
    def n_slots(self):
        """id planes per point (1 or 2)"""
        return self._indexed_info()[0]

    @property
    def n_voxels(self):
        """rows of the voxel table"""
        return self._indexed_info()[1]

    def ids(self):
        """→ [n_slots, n] int32: the voxel ids (table rows, -1 = none) in stored order (nos_indexed_dataset_download)."""
        K, _ = self._indexed_info()
        out = np.zeros((K, len(self)), dtype=np.int32)
        ip_t = ctypes.POINTER(ctypes.c_int32)
        planes = (ip_t * K)(*[out[k].ctypes.data_as(ip_t) for k in range(K)])
        check(self._lib.nos_indexed_dataset_download(self._h, planes, None), "nos_indexed_dataset_download")
        return out

    def table(self):
        """→ [n_voxels, 16] float64: the voxel table {mean(3), U(6) of S = QU, pads}, widened from the element type."""
        _, V = self._indexed_info()
        out = np.zeros((V, 16))
        check(self._lib.nos_indexed_dataset_download(self._h, None, _dp(out)), "nos_indexed_dataset_download")
        return out


class ReprojDataset(_Dataset):
    """Device-resident 3D↔2D correspondences (X, Y, Z, u, v)."""
    _n_planes = 5
    _create = "nos_reproj_dataset_create"
    _create_dev = "nos_reproj_dataset_create_from_device"
    _create_rec = "nos_reproj_dataset_create_from_records"

    def accumulate(self, R, t, intr, loss=None, min_depth=0.03):
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        intr = _dvec(intr, 4)
        out = np.zeros(28)
        l = make_loss(loss)
        check(self._lib.nos_reproj_accumulate(self._h, _dp(R), _dp(t), _dp(intr), ctypes.byref(l),
                                              ctypes.c_double(min_depth), _dp(out)), "nos_reproj_accumulate")
        return out

    def solve(self, R, t, intr, loss=None, min_depth=0.03, max_iterations=100, gradient_tolerance=1e-6,
              parameter_tolerance=1e-6, launches_in_flight=0):
        """Whole LM loop on the device (nos_reproj_solve).  Returns (R[9], t[3], report)."""
        R = _dvec(R, 9).copy()
        t = _dvec(t, 3).copy()
        intr = _dvec(intr, 4)
        l = make_loss(loss)
        return _lm_call(self._lib.nos_reproj_solve, "nos_reproj_solve", (self._h,),
                        (_dp(intr), ctypes.byref(l), ctypes.c_double(min_depth)), R, t,
                        max_iterations, gradient_tolerance, parameter_tolerance, launches_in_flight)

    def accumulate_async(self, R, t, intr, loss, out_tensor, min_depth=0.03):
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        intr = _dvec(intr, 4)
        l = make_loss(loss)
        check(self._lib.nos_reproj_accumulate_async(self._h, _dp(R), _dp(t), _dp(intr), ctypes.byref(l),
                                                    ctypes.c_double(min_depth),
                                                    ctypes.c_void_p(out_tensor.data_ptr())),
              "nos_reproj_accumulate_async")

    def time_kernel(self, R, t, intr, loss=None, min_depth=0.03, repeats=20):
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        intr = _dvec(intr, 4)
        l = make_loss(loss)
        k = ctypes.c_double()
        tot = ctypes.c_double()
        check(self._lib.nos_reproj_time_kernel(self._h, _dp(R), _dp(t), _dp(intr), ctypes.byref(l),
                                               ctypes.c_double(min_depth), repeats, ctypes.byref(k),
                                               ctypes.byref(tot)), "nos_reproj_time_kernel")
        return k.value, tot.value


class NdtMap:
    """Device-resident NDT voxel map for matching (nos_ndt_map): means [V,3], sqrt-information
    [V,3,3] row-major, optional validity mask; search_radius_sq is the FLANN `radius` of the
    reference's MatchPointCloud (squared distance, 1.0 there)."""

    def __init__(self, ctx, means, sqrt_infos, valid=None, search_radius_sq=1.0):
        self._ctx = ctx
        self._lib = ctx._lib
        means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1, 3)
        S = np.ascontiguousarray(sqrt_infos, dtype=np.float64).reshape(-1, 9)
        if means.shape[0] != S.shape[0]:
            raise ValueError("means and sqrt_infos disagree on the voxel count")
        vbuf = None
        if valid is not None:
            vbuf = np.ascontiguousarray(valid, dtype=np.uint8).tobytes()
        h = ctypes.c_void_p()
        check(self._lib.nos_ndt_map_create(ctx.handle, means.shape[0], _dp(means), _dp(S), vbuf,
                                           ctypes.c_double(search_radius_sq), ctypes.byref(h)), "nos_ndt_map_create")
        self._h = h
        ctx._adopt(self)

    @classmethod
    def build(cls, ctx, points, voxel_resolution=1.0, search_radius_sq=1.0, proper_sqrt_information=True,
              reference_exact=False, return_stats=True):
        """Construct the map from raw points [n,3] on the GPU (nos_ndt_map_build, the reference's
        UpdateNdtMap).  → (NdtMap, stats dict with means, sqrt_infos, valid, counts, cells).

        proper_sqrt_information=True (default) stores D^-1/2 V^T, the true square root of the inverse
        covariance; False reproduces the harness formula D^-1/2 V, which is only meaningful when V happens
        to be symmetric (include/nos.h).

        reference_exact=True (NOS_MAP_REFERENCE_EXACT): the harness formula with the reference binary's rounding —
        sequential per-voxel accumulation, Eigen's SelfAdjointEigenSolver restated, the reference build's fused
        multiply-adds; voxels in first-seen order; the stats dict also carries eigvals / eigvecs.

        return_stats=False: out_stats = NULL — the voxel statistics never leave the device (the matcher's tables are
        built there); → (NdtMap, None)."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        h = ctypes.c_void_p()
        hs = ctypes.c_void_p()
        lib = ctx._lib
        flags = 2 if reference_exact else int(bool(proper_sqrt_information))
        check(lib.nos_ndt_map_build(ctx.handle, pts.shape[0], _dp(pts), ctypes.c_double(voxel_resolution),
                                    ctypes.c_double(search_radius_sq), flags,
                                    ctypes.byref(h), ctypes.byref(hs) if return_stats else None),
              "nos_ndt_map_build")
        if not return_stats:
            self = cls.__new__(cls)
            self._ctx = ctx
            self._lib = lib
            self._h = h
            ctx._adopt(self)
            return self, None
        V = int(lib.nos_map_stats_size(hs))
        means = np.zeros((V, 3))
        S = np.zeros((V, 9))
        valid = np.zeros(V, dtype=np.uint8)
        counts = np.zeros(V, dtype=np.uint32)
        cells = np.zeros((V, 3), dtype=np.int64)
        check(lib.nos_map_stats_get(hs, _dp(means), _dp(S), valid.ctypes.data_as(ctypes.c_char_p),
                                    counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                    cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), "nos_map_stats_get")
        stats = {"means": means, "sqrt_infos": S.reshape(V, 3, 3), "valid": valid.astype(bool),
                 "counts": counts, "cells": cells}
        if reference_exact:
            evals = np.zeros((V, 3))
            evecs = np.zeros((V, 9))
            check(lib.nos_map_stats_get_eigen(hs, _dp(evals), _dp(evecs)), "nos_map_stats_get_eigen")
            stats["eigvals"] = evals
            stats["eigvecs"] = evecs.reshape(V, 3, 3)
        lib.nos_map_stats_destroy(hs)
        self = cls.__new__(cls)
        self._ctx = ctx
        self._lib = lib
        self._h = h
        ctx._adopt(self)
        return self, stats

    def __len__(self):
        return int(self._lib.nos_ndt_map_size(self._h))

    def match(self, scan, R, t, max_neighbors=2, dtype="f64"):
        """→ (NdtDataset with 2 slots per scan point, number of real matches)."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        h = ctypes.c_void_p()
        n = ctypes.c_size_t()
        check(self._lib.nos_ndt_match(self._h, scan._h, _dp(R), _dp(t), max_neighbors, _DTYPES[dtype],
                                      ctypes.byref(h), ctypes.byref(n)), "nos_ndt_match")
        return NdtDataset(self._ctx, h), int(n.value)

    def match_indexed(self, scan, R, t, max_neighbors=2, dtype="f64", sort_by_voxel=True):
        """→ (NdtIndexedDataset with max_neighbors voxel slots per scan point, number of real matches)."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        h = ctypes.c_void_p()
        n = ctypes.c_size_t()
        check(self._lib.nos_ndt_match_indexed(self._h, scan._h, _dp(R), _dp(t), max_neighbors, _DTYPES[dtype],
                                              int(bool(sort_by_voxel)), ctypes.byref(h), ctypes.byref(n)),
              "nos_ndt_match_indexed")
        return NdtIndexedDataset(self._ctx, h), int(n.value)

    def score(self, scan, R, t, loss, max_neighbors=2):
        """score_batch for one pose → (matches, matched_points, cost)."""
        row = score_batch(self, [scan], _dvec(R, 9), _dvec(t, 3), loss, max_neighbors)[0]
        return int(row["matches"]), int(row["matched_points"]), float(row["cost"])

    def close(self):
        if self._h:
            self._lib.nos_ndt_map_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def _read_map_stats(lib, hs):
    """nos_map_stats handle → dict with means, sqrt_infos, valid, counts, cells (the handle stays the caller's)."""
    V = int(lib.nos_map_stats_size(hs))
    means = np.zeros((V, 3))
    S = np.zeros((V, 9))
    valid = np.zeros(V, dtype=np.uint8)
    counts = np.zeros(V, dtype=np.uint32)
    cells = np.zeros((V, 3), dtype=np.int64)
    check(lib.nos_map_stats_get(hs, _dp(means), _dp(S), valid.ctypes.data_as(ctypes.c_char_p),
                                counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), "nos_map_stats_get")
    return {"means": means, "sqrt_infos": S.reshape(V, 3, 3), "valid": valid.astype(bool), "counts": counts, "cells": cells}


class VoxelMap:
    """Incremental NDT voxel map (nos_voxel_map): a device-resident store that grows scan by scan — the reference's
    UpdateNdtMap used as the update it is.  insert() / insert_scan() add a batch to the voxels it falls into and
    re-derive the statistics of those voxels only; snapshot() gives an ordinary, independent NdtMap to match against,
    match() matches a scan against the store itself.

    Voxel ids (the order of stats(), the matcher's tie-break) follow the sequence of batches: batch of first appearance,
    then ascending cell.  proper_sqrt_information as in NdtMap.build; capacity (voxels) only avoids early growth.
    prune() removes voxels by a box and / or by age (a sliding window) and renumbers the survivors by their rank;
    carve() removes, the same way, the voxels a scan's rays pass through (line of sight).
    raycast() tells what a sensor at a pose would see: the first voxel every beam hits, and its range.
    export() copies the state — cells, counts, the nine sums, stamps — to the host, whole or by a prune's rule; restore()
    makes an empty store that state again, bit for bit, add() takes it as one more batch; save() / load() keep it in a file."""

    def __init__(self, ctx, voxel_resolution=1.0, search_radius_sq=1.0, proper_sqrt_information=True, capacity=0,
                 flags=None):
        self._ctx = ctx
        self._lib = ctx._lib
        self._h = None
        h = ctypes.c_void_p()
        flags = int(bool(proper_sqrt_information)) if flags is None else int(flags)
        self.voxel_resolution, self.search_radius_sq, self._flags = float(voxel_resolution), float(search_radius_sq), flags
        check(self._lib.nos_voxel_map_create(ctx.handle, ctypes.c_double(voxel_resolution), ctypes.c_double(search_radius_sq),
                                             flags, int(capacity), ctypes.byref(h)), "nos_voxel_map_create")
        self._h = h
        ctx._adopt(self)

    def insert(self, points):
        """points [n,3] in the map frame (host) → number of voxels the batch fell into."""
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_insert(self._h, pts.shape[0], _dp(pts), ctypes.byref(n)), "nos_voxel_map_insert")
        return int(n.value)

    def insert_scan(self, scan, R, t):
        """The points of an api.Scan warped by R p + t on the device → number of voxels touched."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        n = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_insert_scan(self._h, scan._h, _dp(R), _dp(t), ctypes.byref(n)),
              "nos_voxel_map_insert_scan")
        return int(n.value)

    def merge(self, other, R=None, t=None):
        """Every voxel of another VoxelMap moved by R p + t (default: the identity) and added to the voxels of this one
        (nos_voxel_map_merge) → number of voxels of this store the merge touched.  Only `other`'s counts and sums are read:
        the cost follows its voxels, not its points, and it may differ in resolution, search radius and flags.  A source
        voxel goes, whole, to the cell its transformed mean falls into.  `other` is not modified."""
        R = _dvec(np.eye(3) if R is None else R, 9)
        t = _dvec(np.zeros(3) if t is None else t, 3)
        n = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_merge(self._h, other._h, _dp(R), _dp(t), ctypes.byref(n)), "nos_voxel_map_merge")
        return int(n.value)

    def coarsened(self, factor, search_radius_sq=None):
        """→ a new VoxelMap at voxel_resolution · factor filled by merge(self): one level of a multi-resolution map, built
        from this store's voxels without the points.  search_radius_sq defaults to this store's · factor²; the flags are
        this store's.  The new store is closed before an exception leaves."""
        factor = float(factor)
        radius = self.search_radius_sq * factor * factor if search_radius_sq is None else search_radius_sq
        out = VoxelMap(self._ctx, self.voxel_resolution * factor, radius, flags=self._flags)
        try:
            out.merge(self)
        except Exception:
            out.close()
            raise
        return out

    def snapshot(self):
        """→ NdtMap of the store as it is now; it stays valid after later inserts and after close()."""
        h = ctypes.c_void_p()
        check(self._lib.nos_voxel_map_snapshot(self._h, ctypes.byref(h)), "nos_voxel_map_snapshot")
        m = NdtMap.__new__(NdtMap)
        m._ctx = self._ctx
        m._lib = self._lib
        m._h = h
        self._ctx._adopt(m)
        return m

    def match(self, scan, R, t, max_neighbors=2, dtype="f64"):
        """NdtMap.match against the store as it is now, without a snapshot (nos_voxel_map_match) → (NdtDataset with
        2 slots per scan point, number of real matches): bit for bit what snapshot().match(...) returns, at the cost of
        the scan alone.  The dataset is independent of the store; the store is not modified."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        h = ctypes.c_void_p()
        n = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_match(self._h, scan._h, _dp(R), _dp(t), max_neighbors, _DTYPES[dtype],
                                            ctypes.byref(h), ctypes.byref(n)), "nos_voxel_map_match")
        return NdtDataset(self._ctx, h), int(n.value)

    def match_indexed(self, scan, R, t, max_neighbors=2, dtype="f64", sort_by_voxel=True):
        """NdtMap.match_indexed against the store as it is now, without a snapshot (nos_voxel_map_match_indexed) →
        (NdtIndexedDataset, number of real matches).  The voxel table is COMPACT: one row per distinct voxel this scan
        matched, in ascending slot order (n_voxels ≤ max_neighbors · len(scan)), so it is sized by the scan, not by the
        map.  With sort_by_voxel=False every sum and solve is bit for bit that of snapshot().match_indexed(...,
        sort_by_voxel=False); with True, equal to rounding.  The dataset is independent of the store; the store is not
        modified."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        h = ctypes.c_void_p()
        n = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_match_indexed(self._h, scan._h, _dp(R), _dp(t), max_neighbors, _DTYPES[dtype],
                                                    int(bool(sort_by_voxel)), ctypes.byref(h), ctypes.byref(n)),
              "nos_voxel_map_match_indexed")
        return NdtIndexedDataset(self._ctx, h), int(n.value)

    def match_map(self, source, R, t, max_neighbors=2, dtype="f64"):
        """Another VoxelMap matched against this one, voxel against voxel (distribution-to-distribution NDT,
        nos_voxel_map_match_map) → (NdtDataset with 2 slots per voxel of `source`, number of real matches).  Every valid
        voxel mean of `source` is warped by R p + t and searched on this store exactly as match() searches a point; a
        match is an ordinary record p = source mean, mu = this store's mean, and a sqrt-information S with
        SᵀS = (Σ_this + R Σ_source Rᵀ)⁻¹, evaluated at this pose and fixed in the dataset.  Slots 2v and 2v + 1 belong to
        source voxel v; an invalid voxel and a missing neighbour are all-zero records.  Neither store is modified;
        source may be this store, and may differ in resolution, search radius and flags."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        h = ctypes.c_void_p()
        n = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_match_map(self._h, source._h, _dp(R), _dp(t), max_neighbors, _DTYPES[dtype],
                                                ctypes.byref(h), ctypes.byref(n)), "nos_voxel_map_match_map")
        return NdtDataset(self._ctx, h), int(n.value)

    def score(self, scan, R, t, loss, max_neighbors=2):
        """score_batch for one pose → (matches, matched_points, cost)."""
        row = score_batch(self, [scan], _dvec(R, 9), _dvec(t, 3), loss, max_neighbors)[0]
        return int(row["matches"]), int(row["matched_points"]), float(row["cost"])

    def stats(self):
        """→ dict with means, sqrt_infos, valid, counts, cells in voxel-id order (the keys NdtMap.build returns)."""
        hs = ctypes.c_void_p()
        check(self._lib.nos_voxel_map_stats(self._h, ctypes.byref(hs)), "nos_voxel_map_stats")
        try:
            return _read_map_stats(self._lib, hs)
        finally:
            self._lib.nos_map_stats_destroy(hs)

    @staticmethod
    def _keep_rule(who, center, half_extent, max_age):
        """→ the nos_voxel_prune that prune() and export() hand down: a box, an age, or both."""
        if (center is None) != (half_extent is None):
            raise ValueError("center and half_extent go together")
        if center is None and max_age is None:
            raise ValueError("%s needs a box (center, half_extent), max_age, or both" % who)
        rule = _lib.NosVoxelPrune()
        rule.struct_size = ctypes.sizeof(_lib.NosVoxelPrune)
        if center is not None:
            rule.what |= _lib.NOS_PRUNE_BOX
            c = _dvec(center, 3)
            h = np.asarray(half_extent, dtype=np.float64)
            h = np.full(3, float(h)) if h.ndim == 0 else _dvec(h, 3)
            for k in range(3):
                rule.center[k], rule.half_extent[k] = c[k], h[k]
        if max_age is not None:
            if int(max_age) < 0:
                raise ValueError("max_age must be >= 0")
            rule.what |= _lib.NOS_PRUNE_AGE
            rule.max_age = int(max_age)
        return rule

    def prune(self, center=None, half_extent=None, max_age=None):
        """Sliding window (nos_voxel_map_prune) → number of voxels removed.  center [3] with half_extent ([3], or a scalar
        for a cube): keep the voxels whose cell meets the closed box center ± half_extent.  max_age: keep the voxels an
        insert touched within the last max_age inserts (0 = the last insert only).  Both: a voxel must pass both.  The
        survivors keep their order and are renumbered by rank; the store may shrink."""
        rule = self._keep_rule("prune", center, half_extent, max_age)
        n = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_prune(self._h, ctypes.byref(rule), ctypes.byref(n)), "nos_voxel_map_prune")
        return int(n.value)

    def export(self, center=None, half_extent=None, max_age=None, removed=False):
        """The store's state on the host (nos_voxel_map_export) → dict with cells [n,3] int64, counts [n]
        uint32, sums [n,9] (about the cell corner, the store's own numbers), stamps [n] uint32 in voxel-id order, and epoch,
        voxel_resolution, search_radius_sq, proper_sqrt_information.  Without a rule: every voxel.  center / half_extent /
        max_age are prune()'s, read exactly as prune() reads them: the voxels that prune would KEEP, or with removed=True
        the ones it would remove — what a caller pages out before pruning.  The store is not modified."""
        rule = None
        if center is not None or half_extent is not None or max_age is not None:
            rule = self._keep_rule("export", center, half_extent, max_age)
        elif removed:
            raise ValueError("removed=True needs a box (center, half_extent), max_age, or both")
        hs = ctypes.c_void_p()
        check(self._lib.nos_voxel_map_export(self._h, ctypes.byref(rule) if rule is not None else None,
                                             _lib.NOS_STATE_REMOVED if removed else _lib.NOS_STATE_KEPT, ctypes.byref(hs)),
              "nos_voxel_map_export")
        try:
            n = int(self._lib.nos_voxel_state_size(hs))
            cells = np.zeros((n, 3), dtype=np.int64)
            counts, stamps = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
            sums = np.zeros((n, 9))
            res, radius = ctypes.c_double(), ctypes.c_double()
            flags, epoch = ctypes.c_int(), ctypes.c_ulonglong()
            check(self._lib.nos_voxel_state_info(hs, ctypes.byref(res), ctypes.byref(radius), ctypes.byref(flags),
                                                 ctypes.byref(epoch), None), "nos_voxel_state_info")
            u32p = ctypes.POINTER(ctypes.c_uint32)
            check(self._lib.nos_voxel_state_get(hs, cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), counts.ctypes.data_as(u32p),
                                                _dp(sums), stamps.ctypes.data_as(u32p)), "nos_voxel_state_get")
        finally:
            self._lib.nos_voxel_state_destroy(hs)
        return {"cells": cells, "counts": counts, "sums": sums, "stamps": stamps, "epoch": int(epoch.value),
                "voxel_resolution": float(res.value), "search_radius_sq": float(radius.value),
                "proper_sqrt_information": bool(flags.value & 1)}

    def _import(self, mode, state):
        cells = np.ascontiguousarray(state["cells"], dtype=np.int64).reshape(-1, 3)
        counts = np.ascontiguousarray(state["counts"], dtype=np.uint32).reshape(-1)
        sums = np.ascontiguousarray(state["sums"], dtype=np.float64).reshape(-1, 9)
        stamps = state.get("stamps")
        if stamps is not None:
            stamps = np.ascontiguousarray(stamps, dtype=np.uint32).reshape(-1)
        n = counts.size
        if cells.shape[0] != n or sums.shape[0] != n or (stamps is not None and stamps.size != n):
            raise ValueError("cells, counts, sums and stamps of a state have one entry per voxel")
        res = state.get("voxel_resolution")
        u32p = ctypes.POINTER(ctypes.c_uint32)
        touched = ctypes.c_size_t()
        check(self._lib.nos_voxel_map_import(self._h, mode, ctypes.c_double(self.voxel_resolution if res is None else res), n,
                                             cells.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), counts.ctypes.data_as(u32p),
                                             _dp(sums), stamps.ctypes.data_as(u32p) if stamps is not None else None,
                                             int(state.get("epoch", 0)), ctypes.byref(touched)), "nos_voxel_map_import")
        return int(touched.value)

    def restore(self, state):
        """A state (the dict export() returns) into this store, which must hold no voxel (nos_voxel_map_import,
        NOS_IMPORT_RESTORE): voxel i of the state becomes voxel id i with its count, sums and stamp as given, the epoch
        becomes the state's, and the statistics are re-derived with THIS store's flags.  Restored from export() of a store
        with the same resolution and flags, this store cannot be told from that one by anything but memory()'s capacity
        and generation.  Without "stamps" every voxel is stamped with the epoch.  → number of voxels."""
        return self._import(_lib.NOS_IMPORT_RESTORE, state)

    def add(self, state):
        """A state added to this store as ONE batch (nos_voxel_map_import, NOS_IMPORT_ADD) → number of voxels touched.
        Cells the store holds get count += n and sums += s; the others are appended in ascending cell order; the epoch
        advances by one.  The state's stamps and epoch are ignored.  A voxel that was exported, pruned and added back
        where its cell is absent has the count, sums, mean, sqrt-information and validity it had, bit for bit."""
        return self._import(_lib.NOS_IMPORT_ADD, state)

    @classmethod
    def from_state(cls, ctx, state, capacity=0):
        """→ a new VoxelMap with the state's resolution, search radius and flags, restored from it.  The new store is closed
        before an exception leaves."""
        out = cls(ctx, state["voxel_resolution"], state["search_radius_sq"],
                  proper_sqrt_information=bool(state["proper_sqrt_information"]), capacity=capacity)
        try:
            out.restore(state)
        except Exception:
            out.close()
            raise
        return out

    STATE_FORMAT_VERSION = 1

    def save(self, path):
        """export() written as one .npz (np.savez; a path is written as it is given) that load() reads back."""
        state = self.export()
        with open(path, "wb") as f:
            np.savez(f, format_version=np.int64(self.STATE_FORMAT_VERSION), cells=state["cells"], counts=state["counts"],
                     sums=state["sums"], stamps=state["stamps"], epoch=np.uint64(state["epoch"]),
                     voxel_resolution=np.float64(state["voxel_resolution"]), search_radius_sq=np.float64(state["search_radius_sq"]),
                     proper_sqrt_information=np.bool_(state["proper_sqrt_information"]))

    @classmethod
    def load(cls, ctx, path, capacity=0):
        """→ the VoxelMap that save() wrote, as from_state gives it.  A file of an unknown format_version raises ValueError
        before any store is created."""
        with np.load(path, allow_pickle=False) as z:
            version = int(z["format_version"]) if "format_version" in z.files else None
            if version != cls.STATE_FORMAT_VERSION:
                raise ValueError("%s: format_version %r of a voxel map file is not known (this build reads %d)"
                                 % (path, version, cls.STATE_FORMAT_VERSION))
            state = {"cells": z["cells"], "counts": z["counts"], "sums": z["sums"], "stamps": z["stamps"],
                     "epoch": int(z["epoch"]), "voxel_resolution": float(z["voxel_resolution"]),
                     "search_radius_sq": float(z["search_radius_sq"]),
                     "proper_sqrt_information": bool(z["proper_sqrt_information"])}
        return cls.from_state(ctx, state, capacity)

    def carve(self, scan, R, t, min_crossings=2, min_hits=1, end_margin=None, min_range=0.0, max_range=None, origin=(0, 0, 0),
              dry_run=False, counts=False):
        """Line-of-sight carving (nos_voxel_map_carve) → (number of voxels removed, info).  Every point of
        the api.Scan is a ray from the sensor `origin` (scan frame), warped by R p + t and walked cell by cell through the
        grid: a voxel that at least min_crossings rays pass through and in whose cell fewer than min_hits rays of this
        scan end is free space and goes, as prune() removes voxels (survivors keep their order, renumbered by rank).
        end_margin (default 1.5 · voxel_resolution): metres cut off each ray before its endpoint, so that the surface a
        ray ends on is not carved by it.  Rays no longer than min_range are skipped; rays longer than max_range (default
        1024 · voxel_resolution) are walked up to max_range.  dry_run=True removes nothing and returns the number of voxels
        that would go.  info: {"skipped": rays skipped} and, with counts=True, "crossings" and "hits" — uint32 arrays in
        voxel-id order as it was BEFORE the call, for callers who accumulate evidence over several scans themselves."""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        o = _dvec(origin, 3)
        what = _lib.NosVoxelCarve()
        what.struct_size = ctypes.sizeof(_lib.NosVoxelCarve)
        for k in range(3):
            what.origin[k] = o[k]
        what.end_margin = 1.5 * self.voxel_resolution if end_margin is None else float(end_margin)
        what.min_range = float(min_range)
        what.max_range = 1024.0 * self.voxel_resolution if max_range is None else float(max_range)
        if int(min_crossings) < 0 or int(min_hits) < 0:
            raise ValueError("min_crossings and min_hits must be >= 1")
        what.min_crossings, what.min_hits, what.dry_run = int(min_crossings), int(min_hits), int(bool(dry_run))
        removed, skipped = ctypes.c_size_t(), ctypes.c_size_t()
        crossings = hits = None
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if counts:
            n = len(self)
            crossings, hits = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        check(self._lib.nos_voxel_map_carve(self._h, scan._h, _dp(R), _dp(t), ctypes.byref(what), ctypes.byref(removed),
                                            ctypes.byref(skipped), crossings.ctypes.data_as(u32p) if counts else None,
                                            hits.ctypes.data_as(u32p) if counts else None), "nos_voxel_map_carve")
        info = {"skipped": int(skipped.value)}
        if counts:
            info["crossings"], info["hits"] = crossings, hits
        return int(removed.value), info

    def raycast(self, rays, R, t, max_range, min_range=0.0, max_mahalanobis_sq=1.0, min_points=0, origin=(0, 0, 0),
                points=False):
        """Ray casting (nos_voxel_map_raycast) → (voxels int32 [n], ranges float64 [n], info): what would a
        sensor at the pose (R, t) see?  Every point p of the api.Scan `rays` is a beam from `origin` (rays' frame) through
        p, warped by R p + t and walked cell by cell up to max_range; it ends at the first voxel — valid, with at least
        min_points points — whose Gaussian comes within max_mahalanobis_sq of the beam inside its cell, no nearer than
        min_range.  voxels[i] is that voxel's id (-1: none) and ranges[i] the range along the beam (0.0: none), indexed
        like the scan's stored positions.  A measured scan gives the predicted range of every measured beam, a
        ray_pattern renders a view.  info: {"hits": rays that hit, "skipped": rays with a non-finite point, of zero
        length or leaving the addressable grid}; with points=True also "scan": the resident Scan of the hit points in the
        rays' frame, in stored order, whose `order` names each hit's ray — descriptor(), PlaceDatabase.add, filtered,
        match and insert_scan take it as any scan.  The store is only read."""
        return self._raycast(rays, R, t, max_range, min_range, max_mahalanobis_sq, min_points, origin, points, True)

    def _raycast(self, rays, R, t, max_range, min_range, max_mahalanobis_sq, min_points, origin, points, results):
        """raycast(); results=False: the per-ray arrays are not brought to the host (→ None, None, info)"""
        R = _dvec(R, 9)
        t = _dvec(t, 3)
        o = _dvec(origin, 3)
        what = _lib.NosVoxelRaycast()
        what.struct_size = ctypes.sizeof(_lib.NosVoxelRaycast)
        for k in range(3):
            what.origin[k] = o[k]
        what.min_range, what.max_range = float(min_range), float(max_range)
        what.max_mahalanobis_sq = float(max_mahalanobis_sq)
        if not 0 <= int(min_points) <= 0xFFFFFFFF:
            raise ValueError("min_points must be in 0 … 2^32 - 1")
        what.min_points = int(min_points)
        voxels = ranges = None
        if results:
            n = len(rays)
            voxels, ranges = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.float64)
        hits, skipped = ctypes.c_size_t(), ctypes.c_size_t()
        h = ctypes.c_void_p()
        check(self._lib.nos_voxel_map_raycast(self._h, rays._h, _dp(R), _dp(t), ctypes.byref(what),
                                              voxels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if results else None,
                                              _dp(ranges) if results else None, ctypes.byref(h) if points else None,
                                              ctypes.byref(hits), ctypes.byref(skipped)), "nos_voxel_map_raycast")
        info = {"hits": int(hits.value), "skipped": int(skipped.value)}
        if points:
            info["scan"] = Scan._adopted(self._ctx, h)
        return voxels, ranges, info

    def memory(self):
        """→ dict: capacity (slots), bytes (device memory held), epoch (successful non-empty inserts so far), generation
        (times the device block was replaced: growth, a prune that removed something)."""
        cap, nbytes = ctypes.c_size_t(), ctypes.c_size_t()
        epoch, gen = ctypes.c_ulonglong(), ctypes.c_ulonglong()
        check(self._lib.nos_voxel_map_memory(self._h, ctypes.byref(cap), ctypes.byref(nbytes), ctypes.byref(epoch),
                                             ctypes.byref(gen)), "nos_voxel_map_memory")
        return {"capacity": int(cap.value), "bytes": int(nbytes.value), "epoch": int(epoch.value), "generation": int(gen.value)}

    def _info(self):
        v, ok, n = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_ulonglong()
        check(self._lib.nos_voxel_map_info(self._h, ctypes.byref(v), ctypes.byref(ok), ctypes.byref(n)), "nos_voxel_map_info")
        return int(v.value), int(ok.value), int(n.value)

    def __len__(self):
        return self._info()[0]

    @property
    def n_valid(self):
        return self._info()[1]

    @property
    def n_points(self):
        return self._info()[2]

    def close(self):
        if self._h:
            self._lib.nos_voxel_map_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class Scan:
    """Device-resident scan points in the sensor's local frame (nos_scan): points [n,3]."""

    def __init__(self, ctx, points, sort_cell=None, filter_voxel=None):
        """sort_cell: if set, reorder the points by grid cell of that edge (nos_scan_sort_by_cell) — faster matching
        for scans whose points do not arrive in spatial order; `order` then maps positions to input indices.
        filter_voxel: if set, keep the first point of every voxel of that edge (nos_scan_filter, on the device) before
        sorting; the raw device copy is released and `order` maps positions to indices of `points`."""
        self._ctx = ctx
        self._lib = ctx._lib
        self._h = None
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        h = ctypes.c_void_p()
        check(self._lib.nos_scan_create(ctx.handle, pts.shape[0], _dp(pts), ctypes.byref(h)), "nos_scan_create")
        self._h = h
        ctx._adopt(self)
        if filter_voxel is not None:
            kept = self.filtered(filter_voxel)
            self._lib.nos_scan_destroy(self._h)
            self._h, kept._h = kept._h, None
        if sort_cell is not None:
            self.sort_by_cell(sort_cell)

    @classmethod
    def _adopted(cls, ctx, handle):
        """a Scan around a handle the library returned"""
        out = cls.__new__(cls)
        out._ctx = ctx
        out._lib = ctx._lib
        out._h = handle
        ctx._adopt(out)
        return out

    def filtered(self, voxel_size):
        """→ a new Scan with the first point (smallest input index) of every voxel of edge voxel_size, in this scan's
        stored order (nos_scan_filter: FilterPoints of the reference's harness, on the device).  Its `order` gives every
        kept point's index in the array this scan was made from.  This scan is unchanged."""
        h = ctypes.c_void_p()
        check(self._lib.nos_scan_filter(self._h, ctypes.c_double(voxel_size), ctypes.byref(h)), "nos_scan_filter")
        out = Scan.__new__(Scan)
        out._ctx = self._ctx
        out._lib = self._lib
        out._h = h
        self._ctx._adopt(out)
        return out

    def deskewed(self, times, twist, reference_time=1.0):
        """→ a new Scan, motion-compensated under a constant twist (nos_scan_deskew, on the device): the point measured at
        times[i] becomes Exp((times[i] - reference_time) * twist) p, its coordinates in the sensor frame at reference_time.
        times: one time stamp per point of the array this scan was made from (indexed like `order`, so a sorted or filtered
        scan takes the source array's stamps); twist: [6] = (v, w), body frame, per unit of `times` (pipeline.pose_twist
        gives one from two poses).  Same length, same stored order, same `order`.  This scan is unchanged."""
        times = np.ascontiguousarray(times, dtype=np.float64).reshape(-1)
        twist = np.ascontiguousarray(twist, dtype=np.float64).reshape(-1)
        if twist.size != 6:
            raise ValueError("twist must have 6 components (v, w)")
        h = ctypes.c_void_p()
        check(self._lib.nos_scan_deskew(self._h, _dp(times), times.size, ctypes.c_double(reference_time), _dp(twist),
                                        ctypes.byref(h)), "nos_scan_deskew")
        out = Scan.__new__(Scan)
        out._ctx = self._ctx
        out._lib = self._lib
        out._h = h
        self._ctx._adopt(out)
        return out

    def descriptor(self, n_rings=20, n_sectors=60, max_range=80.0, z_floor=-2.0):
        """→ (desc [n_rings, n_sectors], n_used): the Scan Context descriptor of this scan in its own sensor frame
        (nos_scan_descriptor, on the device; the rule: include/nos.h) — max(z) − z_floor per ring and sector
        of the points with finite coordinates, z ≥ z_floor and horizontal range < max_range; n_used counts them."""
        params = _lib.NosPlaceParams(int(n_rings), int(n_sectors), float(max_range), float(z_floor))
        in_limits = 1 <= params.n_rings <= 64 and 1 <= params.n_sectors <= 128  # otherwise the call rejects and writes nothing
        desc = np.zeros((params.n_rings, params.n_sectors) if in_limits else (1, 1), dtype=np.float64)
        used = ctypes.c_size_t(0)
        check(self._lib.nos_scan_descriptor(self._h, ctypes.byref(params), _dp(desc), ctypes.byref(used)),
              "nos_scan_descriptor")
        return desc, int(used.value)

    def points(self):
        """→ the points [n,3] in stored order (nos_scan_points; diagnostics and tests)."""
        out = np.zeros((len(self), 3), dtype=np.float64)
        check(self._lib.nos_scan_points(self._h, _dp(out)), "nos_scan_points")
        return out

    def sort_by_cell(self, cell_edge):
        check(self._lib.nos_scan_sort_by_cell(self._h, ctypes.c_double(cell_edge)), "nos_scan_sort_by_cell")

    @property
    def order(self):
        """order[j] = index (in the array given to the constructor) of the point stored at position j."""
        out = np.zeros(len(self), dtype=np.uint32)
        check(self._lib.nos_scan_order(self._h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))), "nos_scan_order")
        return out

    def __len__(self):
        return int(self._lib.nos_scan_size(self._h))

    def close(self):
        if self._h:
            self._lib.nos_scan_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


class PlaceDatabase:
    """Device-resident database of Scan Context descriptors of one parameter set (nos_place_db; the rule: include/nos.h,
    DESIGN.md §27): add places as the trajectory grows, search every stored place at every yaw in one launch."""

    def __init__(self, ctx, n_rings=20, n_sectors=60, max_range=80.0, z_floor=-2.0, reserve=0):
        self._ctx = ctx
        self._lib = ctx._lib
        self._h = None
        params = _lib.NosPlaceParams(int(n_rings), int(n_sectors), float(max_range), float(z_floor))
        h = ctypes.c_void_p()
        check(self._lib.nos_place_db_create(ctx.handle, ctypes.byref(params), int(reserve), ctypes.byref(h)),
              "nos_place_db_create")
        self._h = h
        self.n_rings, self.n_sectors = params.n_rings, params.n_sectors
        self.max_range, self.z_floor = params.max_range, params.z_floor
        ctx._adopt(self)

    def _host_descriptors(self, desc):
        a = np.ascontiguousarray(desc, dtype=np.float64)
        if a.ndim < 2 or a.shape[-2:] != (self.n_rings, self.n_sectors):
            raise ValueError("expected descriptors of shape [..., %d, %d], got %r" % (self.n_rings, self.n_sectors, a.shape))
        return a

    def add(self, desc_or_scan):
        """Append a place: a host descriptor [n_rings, n_sectors] (nos_place_db_add) or an api.Scan, whose descriptor is
        built on the device and never leaves it (nos_place_db_add_scan).  → its index."""
        index = ctypes.c_size_t(0)
        if isinstance(desc_or_scan, Scan):
            check(self._lib.nos_place_db_add_scan(self._h, desc_or_scan._h, ctypes.byref(index), None), "nos_place_db_add_scan")
        else:
            a = self._host_descriptors(desc_or_scan)
            if a.ndim != 2:
                raise ValueError("add takes one descriptor")
            check(self._lib.nos_place_db_add(self._h, _dp(a), ctypes.byref(index)), "nos_place_db_add")
        return int(index.value)

    def __len__(self):
        return int(self._lib.nos_place_db_size(self._h))

    def get(self, index):
        """→ stored descriptor `index`, [n_rings, n_sectors] (nos_place_db_get)."""
        out = np.zeros((self.n_rings, self.n_sectors), dtype=np.float64)
        check(self._lib.nos_place_db_get(self._h, int(index), _dp(out)), "nos_place_db_get")
        return out

    def search(self, queries_or_scan, first=0, count=None):
        """Distance and best shift of every query against the stored places first … first + count − 1 (count=None: to the
        end).  queries_or_scan: descriptors [Q, n_rings, n_sectors], one descriptor [n_rings, n_sectors], or an api.Scan
        (its descriptor is built and searched on the device).  → (distance, shift), float64 / int32 of shape [Q, count], or
        [count] for a single query.  The query sensor is yawed by about 2π · shift / n_sectors relative to the stored one."""
        first = int(first)
        count = max(len(self) - first, 0) if count is None else int(count)
        i32p = ctypes.POINTER(ctypes.c_int32)
        if isinstance(queries_or_scan, Scan):
            dist = np.zeros(count, dtype=np.float64)
            shift = np.zeros(count, dtype=np.int32)
            check(self._lib.nos_place_db_search_scan(self._h, queries_or_scan._h, first, count, _dp(dist),
                                                     shift.ctypes.data_as(i32p), None), "nos_place_db_search_scan")
            return dist, shift
        a = self._host_descriptors(queries_or_scan)
        single = a.ndim == 2
        q = a.reshape(-1, self.n_rings, self.n_sectors)
        dist = np.zeros((q.shape[0], count), dtype=np.float64)
        shift = np.zeros((q.shape[0], count), dtype=np.int32)
        check(self._lib.nos_place_db_search(self._h, _dp(q), q.shape[0], first, count, _dp(dist), shift.ctypes.data_as(i32p)),
              "nos_place_db_search")
        return (dist[0], shift[0]) if single else (dist, shift)

    FILE_FORMAT_VERSION = 1

    def save(self, path):
        """The parameters and every stored descriptor (get) written as one .npz that load() reads back."""
        desc = np.zeros((len(self), self.n_rings, self.n_sectors), dtype=np.float64)
        for k in range(desc.shape[0]):
            desc[k] = self.get(k)
        with open(path, "wb") as f:
            np.savez(f, format_version=np.int64(self.FILE_FORMAT_VERSION), n_rings=np.int64(self.n_rings),
                     n_sectors=np.int64(self.n_sectors), max_range=np.float64(self.max_range), z_floor=np.float64(self.z_floor),
                     descriptors=desc)

    @classmethod
    def load(cls, ctx, path):
        """→ the PlaceDatabase that save() wrote: same parameters, the descriptors added (add) in their order.  A file of
        an unknown format_version raises ValueError before any database is created."""
        with np.load(path, allow_pickle=False) as z:
            version = int(z["format_version"]) if "format_version" in z.files else None
            if version != cls.FILE_FORMAT_VERSION:
                raise ValueError("%s: format_version %r of a place database file is not known (this build reads %d)"
                                 % (path, version, cls.FILE_FORMAT_VERSION))
            params = (int(z["n_rings"]), int(z["n_sectors"]), float(z["max_range"]), float(z["z_floor"]))
            desc = z["descriptors"]
        out = cls(ctx, *params, reserve=desc.shape[0])
        try:
            for d in desc:
                out.add(d)
        except Exception:
            out.close()
            raise
        return out

    def close(self):
        if self._h:
            self._lib.nos_place_db_destroy(self._h)
            self._h = None

    def __del__(self):
        # at interpreter shutdown the HIP runtime may already be gone: leave the handle to the OS
        if sys is None or sys.is_finalizing():
            return
        try:
            self.close()
        except Exception:
            pass


def ray_pattern(n_azimuth, elevations):
    """→ [len(elevations) * n_azimuth, 3] unit directions of a spinning sensor, elevation-major: for every elevation
    (radians above the horizon) n_azimuth beams at azimuth 2π (k + ½) / n_azimuth, k = 0 … n_azimuth − 1, as
    (cos el cos az, cos el sin az, sin el).  The beams sit in the MIDDLE of their azimuth cells: where n_azimuth is a
    multiple of a descriptor's n_sectors no beam lies on a sector border, so the last bit of an arctangent cannot move a
    rendered point to the neighbouring sector.  A host helper: upload it as an api.Scan and hand it to VoxelMap.raycast."""
    n_azimuth = int(n_azimuth)
    if n_azimuth < 1:
        raise ValueError("n_azimuth must be >= 1")
    el = np.asarray(elevations, dtype=np.float64).reshape(-1, 1)
    az = (2.0 * np.pi / n_azimuth) * (np.arange(n_azimuth, dtype=np.float64) + 0.5).reshape(1, -1)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1)
    return np.ascontiguousarray(d.reshape(-1, 3))


def download(dataset):
    """Dataset → host planes [n_planes, n] (diagnostics / tests)."""
    n = len(dataset)
    planes = np.zeros((dataset._n_planes, n))
    arr = (c_double_p * dataset._n_planes)(*[planes[k].ctypes.data_as(c_double_p) for k in range(dataset._n_planes)])
    check(dataset._lib.nos_dataset_download(dataset._h, arr), "nos_dataset_download")
    return planes
