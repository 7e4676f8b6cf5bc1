"""ctypes binding of libnos_hip.so (the C ABI in include/nos.h).

The library is the product; this module only loads it.  If the shared object is missing or a
HIP device is not usable, every call raises — there is no CPU fallback anywhere in the package.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# NOS_HIP_LIB: an alternative build of the same library (e.g. the -DNOS_LM_TIMING probe build of tools/); default in-tree
LIB_HIP = os.environ.get("NOS_HIP_LIB") or os.path.join(CSRC, "libnos_hip.so")
LIB_HOST = os.path.join(CSRC, "libnos_host.so")

c_double_p = ctypes.POINTER(ctypes.c_double)
c_void_pp = ctypes.POINTER(ctypes.c_void_p)

NOS_OK = 0
NOS_F64 = 0
NOS_F32 = 1
NOS_LOSS_NONE = 0
NOS_LOSS_EXPONENTIAL = 1
NOS_LOSS_HUBER = 2

# every symbol include/nos.h declares; tests check the library exports all of them
C_ABI_SYMBOLS = (
    "nos_ctx_create", "nos_ctx_destroy", "nos_ctx_num_devices", "nos_ctx_set_stream",
    "nos_ctx_synchronize", "nos_comm_get_unique_id", "nos_ctx_comm_init", "nos_ctx_comm_size", "nos_ctx_comm_init_shm", "nos_ctx_comm_init_shm_device", "nos_comm_shm_unlink", "nos_ctx_comm_destroy",
    "nos_ctx_comm_allreduce", "nos_ndt_dataset_create", "nos_reproj_dataset_create",
    "nos_ndt_dataset_create_from_device", "nos_reproj_dataset_create_from_device",
    "nos_ndt_dataset_create_from_records", "nos_reproj_dataset_create_from_records",
    "nos_dataset_download", "nos_ndt_map_create", "nos_ndt_map_destroy", "nos_ndt_map_size", "nos_scan_create",
    "nos_scan_destroy", "nos_scan_size", "nos_scan_sort_by_cell", "nos_scan_order", "nos_scan_filter", "nos_scan_points", "nos_scan_deskew", "nos_scan_descriptor", "nos_place_db_create", "nos_place_db_destroy", "nos_place_db_size", "nos_place_db_add", "nos_place_db_add_scan", "nos_place_db_get", "nos_place_db_search", "nos_place_db_search_scan", "nos_ndt_match", "nos_ndt_indexed_dataset_create", "nos_ndt_match_indexed", "nos_indexed_dataset_info", "nos_indexed_dataset_download", "nos_ndt_map_build", "nos_map_stats_size",
    "nos_map_stats_get", "nos_map_stats_get_eigen", "nos_map_stats_destroy",
    "nos_voxel_map_create", "nos_voxel_map_insert", "nos_voxel_map_insert_scan", "nos_voxel_map_info", "nos_voxel_map_snapshot",
    "nos_voxel_map_stats", "nos_voxel_map_match", "nos_voxel_map_match_indexed", "nos_voxel_map_prune", "nos_voxel_map_carve", "nos_voxel_map_raycast", "nos_voxel_map_memory", "nos_voxel_map_merge", "nos_voxel_map_match_map", "nos_voxel_map_export", "nos_voxel_state_size", "nos_voxel_state_info", "nos_voxel_state_get", "nos_voxel_state_destroy", "nos_voxel_map_import", "nos_voxel_map_destroy", "nos_dataset_drop_last_matches", "nos_pgo_create", "nos_pgo_create_weighted", "nos_pgo_set_loss", "nos_pgo_destroy", "nos_pgo_num_unknowns",
    "nos_pgo_linearize", "nos_pgo_solve", "nos_pgo_retract", "nos_pgo_get_state", "nos_pgo_get_vector",
    "nos_pgo_matvec", "nos_pgo_precondition", "nos_pgo_time_sweep", "nos_pgo_layout_info", "nos_debug_lm_step", "nos_debug_voxel_finish", "nos_debug_voxel_moments", "nos_debug_voxel_pair_information", "nos_dataset_destroy", "nos_dataset_size", "nos_dataset_dtype", "nos_dataset_stream_bytes",
    "nos_dataset_set_simd_class",
    "nos_ndt6_accumulate", "nos_ndt3_accumulate", "nos_reproj_accumulate",
    "nos_ndt6_accumulate_async", "nos_ndt3_accumulate_async", "nos_reproj_accumulate_async",
    "nos_ndt6_solve", "nos_ndt3_solve", "nos_reproj_solve",
    "nos_ndt6_solve_batch", "nos_ndt3_solve_batch", "nos_reproj_solve_batch",
    "nos_ndt6_register_batch", "nos_ndt3_register_batch", "nos_voxel_map_register6_batch", "nos_voxel_map_register3_batch",
    "nos_ndt_score_batch", "nos_voxel_map_score_batch",
    "nos_ctx_set_launch", "nos_ctx_set_option", "nos_ctx_get_option", "nos_runtime_info", "nos_ctx_comm_rccl_count",
    "nos_ctx_last_kernel", "nos_ctx_profile_begin", "nos_ctx_profile_end", "nos_ndt6_time_kernel", "nos_reproj_time_kernel",
    "nos_ndt3_time_kernel", "nos_status_string", "nos_last_error", "nos_version",
)


class NosLoss(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("a", ctypes.c_double), ("b", ctypes.c_double)]


class NosLmOptions(ctypes.Structure):
    _fields_ = [("max_iterations", ctypes.c_int32), ("launches_in_flight", ctypes.c_int32),
                ("gradient_tolerance", ctypes.c_double), ("parameter_tolerance", ctypes.c_double),
                ("cost_history", ctypes.POINTER(ctypes.c_double))]


class NosLmReport(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("ok", ctypes.c_int32), ("launches", ctypes.c_int32),
                ("fallback", ctypes.c_int32), ("printed_cost", ctypes.c_double), ("last_cost", ctypes.c_double),
                ("final_lambda", ctypes.c_double)]


class NosRegisterRound(ctypes.Structure):
    _fields_ = [("matches", ctypes.c_uint64), ("used", ctypes.c_uint64), ("iterations", ctypes.c_int32),
                ("ok", ctypes.c_int32), ("printed_cost", ctypes.c_double), ("last_cost", ctypes.c_double)]


class NosRegisterOptions(ctypes.Structure):
    _fields_ = [("max_outer_iterations", ctypes.c_int32), ("max_neighbors", ctypes.c_int32),
                ("keep_multiple", ctypes.c_int32), ("dtype", ctypes.c_int32),
                ("round_log", ctypes.POINTER(NosRegisterRound))]


class NosRegisterReport(ctypes.Structure):
    _fields_ = [("outer_iter", ctypes.c_int32), ("rounds", ctypes.c_int32), ("ok", ctypes.c_int32), ("pad", ctypes.c_int32)]


class NosPoseScore(ctypes.Structure):
    _fields_ = [("matches", ctypes.c_uint64), ("matched_points", ctypes.c_uint64), ("cost", ctypes.c_double),
                ("reserved", ctypes.c_double)]


NOS_PRUNE_BOX = 1
NOS_PRUNE_AGE = 2


class NosVoxelPrune(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("what", ctypes.c_int), ("center", ctypes.c_double * 3),
                ("half_extent", ctypes.c_double * 3), ("max_age", ctypes.c_ulonglong)]


NOS_CARVE_MAX_CELLS = 4096
NOS_STATE_KEPT = 0
NOS_STATE_REMOVED = 1
NOS_IMPORT_RESTORE = 0
NOS_IMPORT_ADD = 1


class NosVoxelCarve(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("origin", ctypes.c_double * 3), ("end_margin", ctypes.c_double),
                ("min_range", ctypes.c_double), ("max_range", ctypes.c_double), ("min_crossings", ctypes.c_uint32),
                ("min_hits", ctypes.c_uint32), ("dry_run", ctypes.c_int)]


class NosVoxelRaycast(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_size_t), ("origin", ctypes.c_double * 3), ("min_range", ctypes.c_double),
                ("max_range", ctypes.c_double), ("max_mahalanobis_sq", ctypes.c_double), ("min_points", ctypes.c_uint32)]


class NosPlaceParams(ctypes.Structure):
    _fields_ = [("n_rings", ctypes.c_int32), ("n_sectors", ctypes.c_int32), ("max_range", ctypes.c_double),
                ("z_floor", ctypes.c_double)]


class NosError(RuntimeError):
    def __init__(self, status, where, detail):
        super().__init__("%s failed: status %d (%s)" % (where, status, detail))
        self.status = status


_hip = None


def hip_lib():
    """Load libnos_hip.so; raises if it has not been built (no fallback)."""
    global _hip
    if _hip is None:
        if not os.path.exists(LIB_HIP):
            raise ImportError(
                "libnos_hip.so is missing at %s — build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950); this package has no CPU fallback." % LIB_HIP)
        lib = ctypes.CDLL(LIB_HIP)
        _declare(lib)
        _hip = lib
    return _hip


def _declare(lib):
    vp = ctypes.c_void_p
    sz = ctypes.c_size_t
    i = ctypes.c_int
    dp = c_double_p
    lp = ctypes.POINTER(NosLoss)
    lib.nos_ctx_create.argtypes = [ctypes.POINTER(ctypes.c_int), i, c_void_pp]
    lib.nos_ctx_destroy.argtypes = [vp]
    lib.nos_ctx_num_devices.argtypes = [vp]
    lib.nos_ctx_set_stream.argtypes = [vp, i, vp]
    lib.nos_ctx_synchronize.argtypes = [vp]
    lib.nos_ctx_set_launch.argtypes = [vp, i, i]
    lib.nos_ctx_set_option.argtypes = [vp, ctypes.c_char_p, i]
    lib.nos_ctx_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i)]
    lib.nos_runtime_info.argtypes = [ctypes.c_char_p, sz]
    lib.nos_ctx_comm_rccl_count.argtypes = [vp, ctypes.POINTER(i)]
    lib.nos_comm_get_unique_id.argtypes = [ctypes.c_char_p]
    lib.nos_ctx_comm_init.argtypes = [vp, i, i, ctypes.c_char_p]
    lib.nos_ctx_comm_init_shm.argtypes = [vp, i, i, ctypes.c_char_p]
    if hasattr(lib, "nos_ctx_comm_init_shm_device"):
        lib.nos_ctx_comm_init_shm_device.argtypes = [vp, i, i, ctypes.c_char_p]
    lib.nos_comm_shm_unlink.argtypes = [ctypes.c_char_p]
    lib.nos_ctx_comm_destroy.argtypes = [vp]
    lib.nos_ctx_comm_size.argtypes = [vp]
    lib.nos_ctx_comm_allreduce.argtypes = [vp, dp, i]
    if hasattr(lib, "nos_ctx_last_kernel"):  # absent from older builds loaded through NOS_HIP_LIB (tools/ab_resident.sh)
        lib.nos_ctx_last_kernel.argtypes = [vp, i, ctypes.c_char_p, sz]
    lib.nos_ctx_profile_begin.argtypes = [vp, i, i]
    lib.nos_ctx_profile_end.argtypes = [vp, ctypes.POINTER(i), dp, dp, dp]
    lib.nos_ndt_dataset_create.argtypes = [vp, sz, ctypes.POINTER(dp), i, c_void_pp]
    lib.nos_reproj_dataset_create.argtypes = [vp, sz, ctypes.POINTER(dp), i, c_void_pp]
    lib.nos_ndt_dataset_create_from_device.argtypes = [vp, sz, c_void_pp, i, i, c_void_pp]
    lib.nos_reproj_dataset_create_from_device.argtypes = [vp, sz, c_void_pp, i, i, c_void_pp]
    lib.nos_ndt_dataset_create_from_records.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), i, c_void_pp]
    lib.nos_reproj_dataset_create_from_records.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), i, c_void_pp]
    lib.nos_dataset_download.argtypes = [vp, ctypes.POINTER(dp)]
    lib.nos_ndt_map_create.argtypes = [vp, sz, dp, dp, ctypes.c_char_p, ctypes.c_double, c_void_pp]
    lib.nos_ndt_map_destroy.argtypes = [vp]
    lib.nos_ndt_map_size.argtypes = [vp]
    lib.nos_ndt_map_size.restype = sz
    lib.nos_scan_create.argtypes = [vp, sz, dp, c_void_pp]
    lib.nos_scan_destroy.argtypes = [vp]
    lib.nos_scan_size.argtypes = [vp]
    lib.nos_scan_size.restype = sz
    lib.nos_scan_sort_by_cell.argtypes = [vp, ctypes.c_double]
    lib.nos_scan_order.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    lib.nos_scan_filter.argtypes = [vp, ctypes.c_double, c_void_pp]
    lib.nos_scan_points.argtypes = [vp, dp]
    lib.nos_scan_deskew.argtypes = [vp, dp, sz, ctypes.c_double, dp, c_void_pp]
    if hasattr(lib, "nos_scan_descriptor"):  # place recognition: absent from older builds loaded through NOS_HIP_LIB
        pp, szp, i32p = ctypes.POINTER(NosPlaceParams), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_int32)
        lib.nos_scan_descriptor.argtypes = [vp, pp, dp, szp]
        lib.nos_place_db_create.argtypes = [vp, pp, sz, c_void_pp]
        lib.nos_place_db_destroy.argtypes = [vp]
        lib.nos_place_db_size.argtypes = [vp]
        lib.nos_place_db_size.restype = sz
        lib.nos_place_db_add.argtypes = [vp, dp, szp]
        lib.nos_place_db_add_scan.argtypes = [vp, vp, szp, szp]
        lib.nos_place_db_get.argtypes = [vp, sz, dp]
        lib.nos_place_db_search.argtypes = [vp, dp, ctypes.c_int32, sz, sz, dp, i32p]
        lib.nos_place_db_search_scan.argtypes = [vp, vp, sz, sz, dp, i32p, szp]
    lib.nos_ndt_match.argtypes = [vp, vp, dp, dp, i, i, c_void_pp, ctypes.POINTER(sz)]
    lib.nos_ndt_indexed_dataset_create.argtypes = [vp, sz, ctypes.POINTER(dp), i, ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)),
                                                   sz, dp, dp, i, i, c_void_pp]
    lib.nos_ndt_match_indexed.argtypes = [vp, vp, dp, dp, i, i, i, c_void_pp, ctypes.POINTER(sz)]
    lib.nos_ndt_map_build.argtypes = [vp, sz, dp, ctypes.c_double, ctypes.c_double, i, c_void_pp, c_void_pp]
    lib.nos_map_stats_size.argtypes = [vp]
    lib.nos_map_stats_size.restype = sz
    lib.nos_map_stats_get.argtypes = [vp, dp, dp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_int64)]
    if hasattr(lib, "nos_map_stats_get_eigen"):
        lib.nos_map_stats_get_eigen.argtypes = [vp, dp, dp]
    lib.nos_map_stats_destroy.argtypes = [vp]
    if hasattr(lib, "nos_voxel_map_create"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_voxel_map_create.argtypes = [vp, ctypes.c_double, ctypes.c_double, i, sz, c_void_pp]
        lib.nos_voxel_map_insert.argtypes = [vp, sz, dp, ctypes.POINTER(sz)]
        lib.nos_voxel_map_insert_scan.argtypes = [vp, vp, dp, dp, ctypes.POINTER(sz)]
        lib.nos_voxel_map_info.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_ulonglong)]
        lib.nos_voxel_map_snapshot.argtypes = [vp, c_void_pp]
        lib.nos_voxel_map_stats.argtypes = [vp, c_void_pp]
        lib.nos_voxel_map_destroy.argtypes = [vp]
        if hasattr(lib, "nos_voxel_map_prune"):  # the sliding window: absent from builds older still
            ull_p = ctypes.POINTER(ctypes.c_ulonglong)
            lib.nos_voxel_map_prune.argtypes = [vp, ctypes.POINTER(NosVoxelPrune), ctypes.POINTER(sz)]
            lib.nos_voxel_map_memory.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(sz), ull_p, ull_p]
        if hasattr(lib, "nos_voxel_map_carve"):  # line-of-sight carving: absent from builds older still
            u32p = ctypes.POINTER(ctypes.c_uint32)
            lib.nos_voxel_map_carve.argtypes = [vp, vp, dp, dp, ctypes.POINTER(NosVoxelCarve), ctypes.POINTER(sz),
                                                ctypes.POINTER(sz), u32p, u32p]
        if hasattr(lib, "nos_voxel_map_raycast"):  # ray casting: absent from builds older still
            lib.nos_voxel_map_raycast.argtypes = [vp, vp, dp, dp, ctypes.POINTER(NosVoxelRaycast), ctypes.POINTER(ctypes.c_int32), dp,
                                                  c_void_pp, ctypes.POINTER(sz), ctypes.POINTER(sz)]
        if hasattr(lib, "nos_voxel_map_merge"):  # one store merged into another under a pose: absent from builds older still
            lib.nos_voxel_map_merge.argtypes = [vp, vp, dp, dp, ctypes.POINTER(sz)]
        if hasattr(lib, "nos_voxel_map_match_map"):  # one store matched against another: absent from builds older still
            lib.nos_voxel_map_match_map.argtypes = [vp, vp, dp, dp, i, i, c_void_pp, ctypes.POINTER(sz)]
        if hasattr(lib, "nos_voxel_map_export"):  # a store's state out and in: absent from builds older still
            ull, u32p, i64p = ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int64)
            lib.nos_voxel_map_export.argtypes = [vp, ctypes.POINTER(NosVoxelPrune), i, c_void_pp]
            lib.nos_voxel_state_size.argtypes = [vp]
            lib.nos_voxel_state_size.restype = sz
            lib.nos_voxel_state_info.argtypes = [vp, dp, dp, ctypes.POINTER(i), ctypes.POINTER(ull), ctypes.POINTER(ull)]
            lib.nos_voxel_state_get.argtypes = [vp, i64p, u32p, dp, u32p]
            lib.nos_voxel_state_destroy.argtypes = [vp]
            lib.nos_voxel_map_import.argtypes = [vp, i, ctypes.c_double, sz, i64p, u32p, dp, u32p, ull, ctypes.POINTER(sz)]
        if hasattr(lib, "nos_voxel_map_match"):  # matching against the live store: absent from builds older still
            lib.nos_voxel_map_match.argtypes = [vp, vp, dp, dp, i, i, c_void_pp, ctypes.POINTER(sz)]
        if hasattr(lib, "nos_voxel_map_match_indexed"):  # the voxel-indexed form of it: absent from builds older still
            lib.nos_voxel_map_match_indexed.argtypes = [vp, vp, dp, dp, i, i, i, c_void_pp, ctypes.POINTER(sz)]
            lib.nos_indexed_dataset_info.argtypes = [vp, ctypes.POINTER(i), ctypes.POINTER(sz)]
            lib.nos_indexed_dataset_download.argtypes = [vp, ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)), dp]
    if hasattr(lib, "nos_dataset_drop_last_matches"):
        lib.nos_dataset_drop_last_matches.argtypes = [vp, sz]
    ip = ctypes.POINTER(ctypes.c_int32)
    lib.nos_pgo_create.argtypes = [vp, sz, dp, sz, ip, ip, dp, dp, ctypes.c_char_p, ctypes.c_char_p, c_void_pp]
    if hasattr(lib, "nos_pgo_create_weighted"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_pgo_create_weighted.argtypes = [vp, sz, dp, sz, ip, ip, dp, dp, ctypes.c_char_p, ctypes.c_char_p, dp, c_void_pp]
    if hasattr(lib, "nos_pgo_set_loss"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_pgo_set_loss.argtypes = [vp, ctypes.POINTER(NosLoss), ctypes.c_char_p]
    lib.nos_pgo_destroy.argtypes = [vp]
    lib.nos_pgo_num_unknowns.argtypes = [vp]
    lib.nos_pgo_num_unknowns.restype = sz
    lib.nos_pgo_linearize.argtypes = [vp, dp, dp]
    lib.nos_pgo_solve.argtypes = [vp, ctypes.c_double, i, ctypes.c_double, ctypes.POINTER(i), dp, dp]
    lib.nos_pgo_retract.argtypes = [vp]
    lib.nos_pgo_get_state.argtypes = [vp, dp, dp]
    lib.nos_pgo_get_vector.argtypes = [vp, i, dp]
    lib.nos_pgo_matvec.argtypes = [vp, ctypes.c_double, dp, dp]
    if hasattr(lib, "nos_pgo_precondition"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_pgo_precondition.argtypes = [vp, ctypes.c_double, dp, dp]
    if hasattr(lib, "nos_pgo_layout_info"):
        lib.nos_pgo_layout_info.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
    if hasattr(lib, "nos_debug_lm_step"):
        lib.nos_debug_lm_step.argtypes = [vp, i, dp, dp, dp]
    if hasattr(lib, "nos_debug_voxel_finish"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_debug_voxel_finish.argtypes = [ctypes.c_uint32, dp, ctypes.POINTER(ctypes.c_int64), ctypes.c_double, dp, i, dp, dp,
                                               ctypes.POINTER(ctypes.c_ubyte)]
    if hasattr(lib, "nos_debug_voxel_moments"):  # absent from older builds loaded through NOS_HIP_LIB
        i64p = ctypes.POINTER(ctypes.c_int64)
        lib.nos_debug_voxel_moments.argtypes = [ctypes.c_uint32, dp, i64p, ctypes.c_double, dp, dp, ctypes.c_double, i64p, dp]
    if hasattr(lib, "nos_debug_voxel_pair_information"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_debug_voxel_pair_information.argtypes = [dp, dp, dp, dp, ctypes.POINTER(ctypes.c_ubyte)]
    if hasattr(lib, "nos_pgo_time_sweep"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_pgo_time_sweep.argtypes = [vp, i, ctypes.c_double, i, dp]
    lib.nos_dataset_destroy.argtypes = [vp]
    lib.nos_dataset_set_simd_class.argtypes = [vp, ctypes.c_int]
    lib.nos_dataset_set_simd_class.restype = ctypes.c_int
    lib.nos_dataset_size.argtypes = [vp]
    lib.nos_dataset_size.restype = sz
    lib.nos_dataset_dtype.argtypes = [vp]
    lib.nos_dataset_stream_bytes.argtypes = [vp]
    lib.nos_dataset_stream_bytes.restype = sz
    lib.nos_ndt6_accumulate.argtypes = [vp, dp, dp, lp, dp]
    lib.nos_ndt3_accumulate.argtypes = [vp, dp, dp, lp, dp]
    lib.nos_reproj_accumulate.argtypes = [vp, dp, dp, dp, lp, ctypes.c_double, dp]
    lib.nos_ndt6_accumulate_async.argtypes = [vp, dp, dp, lp, vp]
    lib.nos_ndt3_accumulate_async.argtypes = [vp, dp, dp, lp, vp]
    lib.nos_reproj_accumulate_async.argtypes = [vp, dp, dp, dp, lp, ctypes.c_double, vp]
    lmo, lmr = ctypes.POINTER(NosLmOptions), ctypes.POINTER(NosLmReport)
    lib.nos_ndt6_solve.argtypes = [vp, dp, dp, lp, lmo, lmr]
    lib.nos_ndt3_solve.argtypes = [vp, dp, dp, lp, lmo, lmr]
    lib.nos_reproj_solve.argtypes = [vp, dp, dp, dp, lp, ctypes.c_double, lmo, lmr]
    if hasattr(lib, "nos_ndt6_solve_batch"):  # absent from older builds loaded through NOS_HIP_LIB
        lib.nos_ndt6_solve_batch.argtypes = [c_void_pp, ctypes.c_int32, dp, dp, lp, lmo, lmr]
        lib.nos_ndt3_solve_batch.argtypes = [c_void_pp, ctypes.c_int32, dp, dp, lp, lmo, lmr]
        lib.nos_reproj_solve_batch.argtypes = [c_void_pp, ctypes.c_int32, dp, dp, dp, lp, ctypes.c_double, lmo, lmr]
    if hasattr(lib, "nos_ndt6_register_batch"):  # absent from older builds loaded through NOS_HIP_LIB
        ro, rr = ctypes.POINTER(NosRegisterOptions), ctypes.POINTER(NosRegisterReport)
        lib.nos_ndt6_register_batch.argtypes = [vp, c_void_pp, ctypes.c_int32, dp, dp, lp, ro, lmo, rr]
        lib.nos_ndt3_register_batch.argtypes = [vp, c_void_pp, ctypes.c_int32, dp, dp, lp, ro, lmo, rr]
        if hasattr(lib, "nos_voxel_map_register6_batch"):  # against the live voxel store: absent from builds older still
            lib.nos_voxel_map_register6_batch.argtypes = [vp, c_void_pp, ctypes.c_int32, dp, dp, lp, ro, lmo, rr]
            lib.nos_voxel_map_register3_batch.argtypes = [vp, c_void_pp, ctypes.c_int32, dp, dp, lp, ro, lmo, rr]
    if hasattr(lib, "nos_ndt_score_batch"):  # pose scoring: absent from older builds loaded through NOS_HIP_LIB
        sp = ctypes.POINTER(NosPoseScore)
        lib.nos_ndt_score_batch.argtypes = [vp, c_void_pp, ctypes.c_int32, dp, dp, lp, i, sp]
        lib.nos_voxel_map_score_batch.argtypes = [vp, c_void_pp, ctypes.c_int32, dp, dp, lp, i, sp]
    lib.nos_ndt6_time_kernel.argtypes = [vp, dp, dp, lp, i, dp, dp]
    lib.nos_ndt3_time_kernel.argtypes = [vp, dp, dp, lp, i, dp, dp]
    lib.nos_reproj_time_kernel.argtypes = [vp, dp, dp, dp, lp, ctypes.c_double, i, dp, dp]
    lib.nos_status_string.argtypes = [i]
    lib.nos_status_string.restype = ctypes.c_char_p
    lib.nos_last_error.restype = ctypes.c_char_p
    lib.nos_version.restype = ctypes.c_char_p


def check(status, where):
    if status != NOS_OK:
        lib = hip_lib()
        detail = "%s: %s" % (lib.nos_status_string(status).decode(), lib.nos_last_error().decode())
        raise NosError(status, where, detail)
