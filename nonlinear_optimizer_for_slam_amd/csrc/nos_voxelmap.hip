// nos_voxelmap.hip — the entry points of the incremental NDT voxel store, a device-resident map that grows scan by scan
// (DESIGN.md §13), and its two debug hooks: argument checks in the order include/nos.h documents, then the host code of
// voxel_store_host.hpp (the store and what writes it: a batch grouped by voxel through group_host.hpp, §19; prune, §13;
// carve, §25) or of voxel_query_host.hpp (what reads it: matches through match_host.hpp, §18; ray cast, §32; export, §31).
#define NOS_WITH_VOXEL_INDEX_KERNELS  // voxelmatch_kernels.hpp: this unit compiles (and launches) the two index kernels
#include "voxel_query_host.hpp"  // voxel_store_host.hpp with it

using namespace nosd;

extern "C" {

int nos_voxel_map_create(nos_ctx* ctx, double voxel_resolution, double search_radius_sq, int flags, size_t capacity_hint,
                         nos_voxel_map** out) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || !out) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx / out is NULL");
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "a voxel store needs a single-device context");
  if (flags & NOS_MAP_REFERENCE_EXACT)
    return fail(NOS_ERR_UNSUPPORTED, "NOS_MAP_REFERENCE_EXACT accumulates sequentially in point order: one-shot builds only");
  if (flags & ~NOS_MAP_PROPER_SQRT_INFORMATION) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown flags");
  if (!(voxel_resolution > 0.0) || !std::isfinite(voxel_resolution)) return fail(NOS_ERR_INVALID_ARGUMENT, "bad voxel resolution");
  if (!(search_radius_sq > 0.0) || !std::isfinite(search_radius_sq)) return fail(NOS_ERR_INVALID_ARGUMENT, "bad search radius");
  if (capacity_hint > (size_t(1) << 30)) return fail(NOS_ERR_UNSUPPORTED, "too many voxels for one store");
  std::unique_ptr<nos_voxel_map> vm(new (std::nothrow) nos_voxel_map());
  if (!vm) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  vm->ctx = ctx;
  vm->voxel_resolution = voxel_resolution;
  vm->search_radius_sq = search_radius_sq;
  vm->flags = flags;
  vm->capacity = 16;
  while (vm->capacity < capacity_hint) vm->capacity *= 2;
  vm->min_capacity = vm->capacity;
  DeviceSlot& slot = ctx->slots[0];
  hipError_t e = hipSetDevice(slot.device);
  if (e == hipSuccess) e = device_alloc(slot, &vm->d_info, nos::kInfoWords * sizeof(unsigned int));
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info, 0, nos::kInfoWords * sizeof(unsigned int), slot.stream);
  if (e == hipSuccess) e = store_alloc(slot, vm->capacity, &vm->d_block, &vm->block_bytes, &vm->view);
  if (e == hipSuccess) e = hipStreamSynchronize(slot.stream);
  if (e != hipSuccess) {
    if (vm->d_info) (void)hipFree(vm->d_info);
    if (vm->d_block) (void)hipFree(vm->d_block);
    return hip_fail(e, "voxel store create");
  }
  *out = vm.release();
  return NOS_OK;
}

int nos_voxel_map_insert(nos_voxel_map* vm, size_t n_points, const double* points_xyz, size_t* n_touched) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map is NULL");
  if (!points_xyz && n_points > 0) return fail(NOS_ERR_INVALID_ARGUMENT, "points is NULL");
  const nos::PosePod identity{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
  return store_insert(vm, n_points, points_xyz, nullptr, nullptr, identity, n_touched);
}

int nos_voxel_map_insert_scan(nos_voxel_map* vm, nos_scan* scan, const double R[9], const double t[3], size_t* n_touched) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm || !scan || !R || !t) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (vm->ctx != scan->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map and scan belong to different contexts");
  return store_insert(vm, scan->n, nullptr, scan->d_planes, scan->d_order, make_pose(R, t), n_touched);
}

int nos_voxel_map_merge(nos_voxel_map* dst, const nos_voxel_map* src, const double R[9], const double t[3], size_t* n_touched) {
  if (!dst || !src || !R || !t) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (dst == src) return fail(NOS_ERR_INVALID_ARGUMENT, "a voxel map cannot be merged into itself");
  nosd::CtxGuard guard_(dst->ctx);  // one solve / accumulate / create at a time per context
  if (dst->ctx != src->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "the two voxel maps belong to different contexts");
  if (const int rc = check_pose_finite(R, t); rc != NOS_OK) return rc;
  return store_merge(dst, src, make_pose(R, t), n_touched);
}

// Test hook: the moment transform on the HOST — voxel_moments as the kernel compiles it, no GPU call.
int nos_debug_voxel_moments(uint32_t count, const double sums[9], const int64_t cell[3], double src_resolution,
                            const double R[9], const double t[3], double dst_resolution, int64_t cell_out[3],
                            double sums_out[9]) {
  if (!sums || !cell || !R || !t || !cell_out || !sums_out) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (count == 0) return fail(NOS_ERR_INVALID_ARGUMENT, "a voxel holds at least one point");
  if (!(src_resolution > 0.0) || !std::isfinite(src_resolution) || !(dst_resolution > 0.0) || !std::isfinite(dst_resolution))
    return fail(NOS_ERR_INVALID_ARGUMENT, "bad voxel resolution");
  double acc[9], Rm[9], tv[3], cf[3], out[9];
  for (int k = 0; k < 9; ++k) acc[k] = sums[k], Rm[k] = R[k];
  for (int k = 0; k < 3; ++k) tv[k] = t[k];
  const int64_t c[3] = {cell[0], cell[1], cell[2]};
  nos::voxel_moments(count, acc, c, src_resolution, Rm, tv, dst_resolution, 1.0 / dst_resolution, cf, out);
  for (int k = 0; k < 3; ++k)
    if (!(cf[k] >= -9.0e18 && cf[k] <= 9.0e18)) return fail(NOS_ERR_UNSUPPORTED, "the destination cell is not representable");
  for (int k = 0; k < 3; ++k) cell_out[k] = int64_t(cf[k]);
  for (int k = 0; k < 9; ++k) sums_out[k] = out[k];
  return NOS_OK;
}

int nos_voxel_map_info(const nos_voxel_map* vm, size_t* n_voxels, size_t* n_valid, unsigned long long* n_points) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map is NULL");
  if (n_voxels) *n_voxels = vm->n_voxels;
  if (n_valid) *n_valid = vm->n_valid;
  if (n_points) *n_points = vm->n_points;
  return NOS_OK;
}

int nos_voxel_map_prune(nos_voxel_map* vm, const nos_voxel_prune* what, size_t* n_removed) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm || !what) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  nos::VoxelKeepRule rule{};
  int rc = keep_rule(vm, what, &rule);
  if (rc == NOS_OK) rc = check_usable(vm->broken);
  return rc != NOS_OK ? rc : store_prune(vm, rule, n_removed);
}

int nos_voxel_map_carve(nos_voxel_map* vm, nos_scan* scan, const double R[9], const double t[3], const nos_voxel_carve* what,
                        size_t* n_removed, size_t* n_skipped, uint32_t* crossings_out, uint32_t* hits_out) {
  // the NULL, struct and value checks come before any device (and any handle's content) is touched
  if (!vm || !scan || !R || !t || !what) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (what->struct_size < sizeof(nos_voxel_carve)) return fail(NOS_ERR_INVALID_ARGUMENT, "struct_size is smaller than nos_voxel_carve");
  if (const int rc = check_pose_finite(R, t, what->origin); rc != NOS_OK) return rc;
  if (!std::isfinite(what->end_margin) || what->end_margin < 0.0 || !std::isfinite(what->min_range) || what->min_range < 0.0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "end_margin and min_range must be finite and >= 0");
  if (!std::isfinite(what->max_range) || !(what->max_range > 0.0)) return fail(NOS_ERR_INVALID_ARGUMENT, "max_range must be finite and > 0");
  if (what->min_crossings == 0 || what->min_hits == 0) return fail(NOS_ERR_INVALID_ARGUMENT, "min_crossings and min_hits must be >= 1");
  if (vm->ctx != scan->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map and scan belong to different contexts");
  nosd::CtxGuard guard_(vm->ctx);  // one solve / accumulate / create at a time per context
  if (vm->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "carving a voxel store needs a single-device context");
  if (const int rc = check_ray_reach(what->max_range, vm->voxel_resolution); rc != NOS_OK) return rc;
  if (const int rc = check_usable(vm->broken); rc != NOS_OK) return rc;
  nos::VoxelCarveParams prm{};
  for (int k = 0; k < 3; ++k) prm.origin[k] = what->origin[k];
  prm.end_margin = what->end_margin, prm.min_range = what->min_range, prm.max_range = what->max_range;
  prm.res = vm->voxel_resolution;
  prm.inv_res = 1.0 / vm->voxel_resolution;  // what voxel_points_kernel is handed
  prm.max_cells = NOS_CARVE_MAX_CELLS;
  return store_carve(vm, scan, make_pose(R, t), prm, what->min_crossings, what->min_hits, what->dry_run != 0, n_removed, n_skipped,
                     crossings_out, hits_out);
}

int nos_voxel_map_raycast(nos_voxel_map* vm, nos_scan* rays, const double R[9], const double t[3], const nos_voxel_raycast* what,
                          int32_t* voxel_out, double* range_out, nos_scan** out_scan, size_t* n_hit, size_t* n_skipped) {
  // the NULL, struct and value checks come before any device (and any handle's content) is touched
  if (!vm || !rays || !R || !t || !what) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (what->struct_size < sizeof(nos_voxel_raycast)) return fail(NOS_ERR_INVALID_ARGUMENT, "struct_size is smaller than nos_voxel_raycast");
  if (const int rc = check_pose_finite(R, t, what->origin); rc != NOS_OK) return rc;
  if (!std::isfinite(what->max_range) || !(what->max_range > 0.0)) return fail(NOS_ERR_INVALID_ARGUMENT, "max_range must be finite and > 0");
  if (!std::isfinite(what->min_range) || what->min_range < 0.0 || !std::isfinite(what->max_mahalanobis_sq) || what->max_mahalanobis_sq < 0.0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "min_range and max_mahalanobis_sq must be finite and >= 0");
  if (vm->ctx != rays->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map and scan belong to different contexts");
  nosd::CtxGuard guard_(vm->ctx);  // one solve / accumulate / create at a time per context
  if (vm->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "ray casting a voxel store needs a single-device context");
  if (const int rc = check_ray_reach(what->max_range, vm->voxel_resolution); rc != NOS_OK) return rc;
  if (const int rc = check_usable(vm->broken); rc != NOS_OK) return rc;
  nos::VoxelRaycastParams prm{};
  for (int k = 0; k < 3; ++k) prm.origin[k] = what->origin[k];
  prm.min_range = what->min_range, prm.max_range = what->max_range, prm.max_mahalanobis_sq = what->max_mahalanobis_sq;
  prm.res = vm->voxel_resolution;
  prm.inv_res = 1.0 / vm->voxel_resolution;  // what voxel_points_kernel is handed
  prm.min_points = what->min_points;
  prm.max_cells = NOS_CARVE_MAX_CELLS;
  return store_raycast(vm, rays, make_pose(R, t), prm, voxel_out, range_out, out_scan, n_hit, n_skipped);
}

int nos_voxel_map_memory(const nos_voxel_map* vm, size_t* capacity, size_t* bytes, unsigned long long* epoch,
                         unsigned long long* generation) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map is NULL");
  if (capacity) *capacity = vm->capacity;
  if (bytes) *bytes = vm->block_bytes + nos::kInfoWords * sizeof(unsigned int);
  if (epoch) *epoch = vm->epoch;
  if (generation) *generation = vm->generation;
  return NOS_OK;
}

int nos_voxel_map_snapshot(nos_voxel_map* vm, nos_ndt_map** out_map) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm || !out_map) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (const int rc = check_usable(vm->broken); rc != NOS_OK) return rc;
  *out_map = nullptr;
  // the matcher's tables straight from the store's device-resident statistics; the map copies what it keeps
  return map_create_device(vm->ctx, vm->n_voxels, vm->view.mean, vm->view.sqrt_info, vm->view.valid, vm->search_radius_sq,
                           out_map);
}

int nos_voxel_map_match(nos_voxel_map* vm, nos_scan* scan, const double R[9], const double t[3], int max_neighbors, int dtype,
                        nos_dataset** out_ds, size_t* n_matches) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  int rc = check_store_match(vm, scan, R, t, out_ds, max_neighbors, dtype);
  if (rc != NOS_OK) return rc;
  nos_dataset* ds = nullptr;  // *out_ds is written on success only
  rc = run_match(StoreSource{live_store(vm)}, nos::voxel_match_kernel<double>, nos::voxel_match_kernel<float>, vm->ctx, scan,
                 make_pose(R, t), max_neighbors, dtype, &ds, n_matches);
  if (rc == NOS_OK) *out_ds = ds;
  return rc;
}

int nos_voxel_map_match_map(nos_voxel_map* target, nos_voxel_map* source, const double R[9], const double t[3], int max_neighbors,
                            int dtype, nos_dataset** out_ds, size_t* n_matches) {
  nosd::CtxGuard guard_(target ? target->ctx : nullptr);  // one solve / accumulate / create at a time per context
  // nos_voxel_map_match's rejections in its order, with the source store where it has the scan
  if (!target || !source || !R || !t || !out_ds) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (target->ctx != source->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "the two voxel maps belong to different contexts");
  if (dtype != NOS_F64 && dtype != NOS_F32) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown dtype %d", dtype);
  if (max_neighbors < 1 || max_neighbors > 2) return fail(NOS_ERR_UNSUPPORTED, "max_neighbors must be 1 or 2");
  if (target->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "matching against a voxel store needs a single-device context");
  int rc = check_live_store(live_store(target));
  if (rc != NOS_OK) return rc;
  if (source->broken) return fail(NOS_ERR_HIP, "the source voxel store was left undefined by an earlier failure");
  nos_dataset* ds = nullptr;  // *out_ds is written on success only
  const nos::PosePod pose = make_pose(R, t);
  rc = run_match_over(StoreSource{live_store(target)}, nos::voxel_match_map_kernel<double>, nos::voxel_match_map_kernel<float>,
                      target->ctx, StoreVoxels(source, pose), pose, max_neighbors, dtype, &ds, n_matches);
  if (rc == NOS_OK) *out_ds = ds;
  return rc;
}

// Test hook: the combined information on the HOST — voxel_pair_information as the kernel compiles it, no GPU call.
int nos_debug_voxel_pair_information(const double S_target[9], const double S_source[9], const double R[9], double S_out[9],
                                     unsigned char* ok) {
  if (!S_target || !S_source || !R || !S_out || !ok) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  double St[9], Ss[9], Rm[9], out[9];
  for (int k = 0; k < 9; ++k) St[k] = S_target[k], Ss[k] = S_source[k], Rm[k] = R[k];
  *ok = nos::voxel_pair_information(St, Ss, Rm, out);
  for (int k = 0; k < 9; ++k) S_out[k] = out[k];
  return NOS_OK;
}

int nos_voxel_map_match_indexed(nos_voxel_map* vm, nos_scan* scan, const double R[9], const double t[3], int max_neighbors,
                                int dtype, int sort_by_voxel, nos_dataset** out_ds, size_t* n_matches) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  int rc = check_store_match(vm, scan, R, t, out_ds, max_neighbors, dtype);
  if (rc != NOS_OK) return rc;
  const StoreSource src{live_store(vm)};
  const size_t n = scan->n;
  if (n >= (size_t(1) << 31)) return fail(NOS_ERR_UNSUPPORTED, "too many points for one indexed dataset");
  nos_ctx* ctx = vm->ctx;
  DeviceSlot& slot = ctx->slots[0];
  const size_t n_keys = n * size_t(max_neighbors);
  DeviceBuffers buf(&slot);  // the id planes, their sorted copy, the distinct list and rocPRIM's temporaries
  buf.reserve(2 * n * sizeof(int32_t) + 2 * n_keys * sizeof(uint32_t) + (size_t(1) << 20));
  int32_t* d_idx = nullptr;
  uint32_t *rows = nullptr, n_rows = 0;
  size_t count = 0;
  // 1. the search: store slots (or -1) per point and slot plane; 2. the compact table behind it, before the wait (1 of 2)
  rc = run_match_ids(src, voxel_match_index_kernel, ctx, buf, scan, make_pose(R, t), max_neighbors, &d_idx, &count,
                     [&](int32_t* ids) { return compact_ids(vm->capacity, slot, buf, ids, n_keys, &rows, &n_rows); });
  if (rc != NOS_OK) return rc;
  // the list ends with the key of -1 exactly when some id is absent, i.e. when fewer than n_keys ids matched
  const size_t n_voxels = n_rows - ((n_rows > 0 && count < n_keys) ? 1u : 0u);
  // 3. points, ids and the gathered table rows into one dataset (wait 2 of 2 inside); the sources are the store's own arrays
  rc = indexed_from_device(ctx, n, scan->d_planes, max_neighbors, d_idx, n_voxels, src.view.mean, src.view.sqrt_info, rows, dtype,
                           sort_by_voxel, out_ds);
  if (rc != NOS_OK) return rc;
  if (n_matches) *n_matches = count;
  return NOS_OK;
}

int nos_voxel_map_register6_batch(nos_voxel_map* vm, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                                  const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                                  nos_register_report* reports) {
  return voxel_map_register(6, vm, scans, n_problems, R, t, loss, ropt, options, reports);
}

int nos_voxel_map_register3_batch(nos_voxel_map* vm, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                                  const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                                  nos_register_report* reports) {
  return voxel_map_register(3, vm, scans, n_problems, R, t, loss, ropt, options, reports);
}

int nos_voxel_map_score_batch(nos_voxel_map* vm, nos_scan* const* scans, int32_t n_problems, const double* R, const double* t,
                              const nos_loss* loss, int max_neighbors, nos_pose_score* scores) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm) return score_live(nullptr, scans, n_problems, R, t, loss, max_neighbors, scores);
  const LiveStore store = live_store(vm);
  return score_live(&store, scans, n_problems, R, t, loss, max_neighbors, scores);
}

int nos_voxel_map_stats(nos_voxel_map* vm, nos_map_stats** out_stats) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm || !out_stats) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (const int rc = check_usable(vm->broken); rc != NOS_OK) return rc;
  *out_stats = nullptr;
  std::unique_ptr<nos_map_stats> stats(new (std::nothrow) nos_map_stats());
  if (!stats) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  std::vector<uint64_t> h_keys;
  DeviceSlot& slot = vm->ctx->slots[0];
  const nos::VoxelStoreView& v = vm->view;
  hipError_t e = vm->n_voxels > 0 ? hipSetDevice(slot.device) : hipSuccess;
  if (e == hipSuccess) e = download_stats(vm->n_voxels, v.mean, v.sqrt_info, v.valid, v.count, v.key, slot.stream, stats.get(), &h_keys);
  if (e == hipSuccess && vm->n_voxels > 0) e = hipStreamSynchronize(slot.stream);
  if (e != hipSuccess) return hip_fail(e, "voxel store download");
  cells_from_packed_keys(h_keys, stats.get());
  *out_stats = stats.release();
  return NOS_OK;
}

int nos_voxel_map_export(nos_voxel_map* vm, const nos_voxel_prune* select, int side, nos_voxel_state** out_state) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm || !out_state) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (side != NOS_STATE_KEPT && side != NOS_STATE_REMOVED) return fail(NOS_ERR_INVALID_ARGUMENT, "side must be NOS_STATE_KEPT or NOS_STATE_REMOVED");
  nos::VoxelKeepRule rule{};
  if (select) {
    const int rc = keep_rule(vm, select, &rule);
    if (rc != NOS_OK) return rc;
  }
  if (vm->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "exporting a voxel store needs a single-device context");
  if (const int rc = check_usable(vm->broken); rc != NOS_OK) return rc;
  std::unique_ptr<nos_voxel_state> state(new (std::nothrow) nos_voxel_state());
  if (!state) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  const int rc = store_export(vm, select ? &rule : nullptr, side, state.get());
  if (rc != NOS_OK) return rc;
  *out_state = state.release();
  return NOS_OK;
}

size_t nos_voxel_state_size(const nos_voxel_state* state) { return state ? state->counts.size() : 0; }

int nos_voxel_state_info(const nos_voxel_state* state, double* voxel_resolution, double* search_radius_sq, int* flags,
                         unsigned long long* epoch, unsigned long long* n_points) {
  if (!state) return fail(NOS_ERR_INVALID_ARGUMENT, "state is NULL");
  if (voxel_resolution) *voxel_resolution = state->voxel_resolution;
  if (search_radius_sq) *search_radius_sq = state->search_radius_sq;
  if (flags) *flags = state->flags;
  if (epoch) *epoch = state->epoch;
  if (n_points) *n_points = state->n_points;
  return NOS_OK;
}

int nos_voxel_state_get(const nos_voxel_state* state, int64_t* cells_xyz, uint32_t* counts, double* sums, uint32_t* stamps) {
  if (!state) return fail(NOS_ERR_INVALID_ARGUMENT, "state is NULL");
  const size_t n = state->counts.size();
  if (cells_xyz && n > 0) std::memcpy(cells_xyz, state->cells.data(), n * 3 * sizeof(int64_t));
  if (counts && n > 0) std::memcpy(counts, state->counts.data(), n * sizeof(uint32_t));
  if (sums && n > 0) std::memcpy(sums, state->sums.data(), n * 9 * sizeof(double));
  if (stamps && n > 0) std::memcpy(stamps, state->stamps.data(), n * sizeof(uint32_t));
  return NOS_OK;
}

int nos_voxel_state_destroy(nos_voxel_state* state) {
  delete state;
  return NOS_OK;
}

int nos_voxel_map_import(nos_voxel_map* vm, int mode, double voxel_resolution, size_t n, const int64_t* cells_xyz,
                         const uint32_t* counts, const double* sums, const uint32_t* stamps, unsigned long long epoch,
                         size_t* n_touched) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  // the checks that need no device, the NOS_ERR_INVALID_ARGUMENT ones that read nothing of the store first
  if (!vm) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map is NULL");
  if (mode != NOS_IMPORT_RESTORE && mode != NOS_IMPORT_ADD) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown import mode %d", mode);
  if (n > 0 && (!cells_xyz || !counts || !sums)) return fail(NOS_ERR_INVALID_ARGUMENT, "cells / counts / sums is NULL");
  if (std::memcmp(&voxel_resolution, &vm->voxel_resolution, sizeof(double)) != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "the state's voxel resolution is not the store's: its sums are about the corners of another grid");
  if (vm->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "importing into a voxel store needs a single-device context");
  if (n > (size_t(1) << 30)) return fail(NOS_ERR_UNSUPPORTED, "too many voxels for one store");
  for (size_t i = 0; i < n; ++i) {
    if (counts[i] == 0) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel %zu has a count of 0: a voxel holds at least one point", i);
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(sums[9 * i + k])) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel %zu has a non-finite sum", i);
  }
  const int64_t lim = int64_t(1) << 20;
  std::vector<uint64_t> keys(n);
  for (size_t i = 0; i < n; ++i) {
    const int64_t* c = cells_xyz + 3 * i;
    for (int k = 0; k < 3; ++k)
      if (c[k] < -lim || c[k] >= lim)
        return fail(NOS_ERR_UNSUPPORTED, "voxel %zu lies outside the addressable grid (+-2^20 cells per axis)", i);
    keys[i] = nos::pack_cell(c[0], c[1], c[2]);
  }
  if (mode == NOS_IMPORT_RESTORE && vm->n_voxels != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "NOS_IMPORT_RESTORE needs a store that holds no voxel (this one holds %u)", vm->n_voxels);
  if (const int rc = check_usable(vm->broken); rc != NOS_OK) return rc;
  if (mode == NOS_IMPORT_RESTORE) return store_restore(vm, n, keys, cells_xyz, counts, sums, stamps, epoch, n_touched);
  return store_add(vm, n, keys, cells_xyz, counts, sums, n_touched);
}

int nos_voxel_map_destroy(nos_voxel_map* vm) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm) return NOS_OK;
  (void)hipSetDevice(vm->ctx->slots[0].device);
  if (vm->d_block) (void)hipFree(vm->d_block);
  if (vm->d_info) (void)hipFree(vm->d_info);
  delete vm;
  return NOS_OK;
}

}  // extern "C"
