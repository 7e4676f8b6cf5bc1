// voxel_query_host.hpp — everything that only reads the voxel store of voxel_store_host.hpp: the ray cast,
// the export of its state (§31), and what a match against it is handed (§14, §17, §23: live_store, the compact table of an
// indexed match, a second store's voxels as the items of a map-to-map match).  Part of nos_voxelmap.hip, the one unit that
// includes it.
#pragma once

#include "voxel_store_host.hpp"
#include "match_host.hpp"

#include "voxelmatch_kernels.hpp"
#include "voxeld2d_kernels.hpp"
#include "voxelraycast_kernels.hpp"

#include <optional>

namespace nosd {

// One ray cast: every point of `rays` under `pose` is a beam walked through the grid until the first
// voxel it hits.  The store is only read — its info block too: the three counters are the cast's own, in arena memory.
// Waits: the one that brings the counters, the hit count of the select and the per-ray results; a second one behind the
// gather when the caller wants the hit points and there are any.  The outputs are written once nothing can fail any more.
inline int store_raycast(nos_voxel_map* vm, const nos_scan* rays, const nos::PosePod& pose, const nos::VoxelRaycastParams& prm,
                         int32_t* voxel_out, double* range_out, nos_scan** out_scan, size_t* n_hit, size_t* n_skipped) {
  const size_t n = rays->n;
  if (n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points for one ray cast");
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  hipError_t e = hipSetDevice(slot.device);
  if (e != hipSuccess) return hip_fail(e, "voxel store ray cast");
  std::optional<NewScan> hits;  // the hit points, made only for a caller who wants them
  if (out_scan && !hits.emplace(vm->ctx)) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  if (n == 0 || vm->n_voxels == 0) {  // nothing to cast, or nothing to hit
    if (out_scan) {
      e = hits->alloc(0, false);
      if (e != hipSuccess) return hip_fail(e, "voxel store ray cast (empty scan)");
      *out_scan = hits->release();
    }
    for (size_t i = 0; i < n; ++i) {
      if (voxel_out) voxel_out[i] = -1;
      if (range_out) range_out[i] = 0.0;
    }
    if (n_hit) *n_hit = 0;
    if (n_skipped) *n_skipped = 0;
    return NOS_OK;
  }
  std::vector<int32_t> h_voxel;
  std::vector<double> h_range;
  try {
    if (voxel_out) h_voxel.resize(n);
    if (range_out) h_range.resize(n);
  } catch (const std::bad_alloc&) {
    return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  }
  unsigned int h_cnt[nos::kRaycastWords] = {};
  uint32_t n_kept = 0;
  {
    DeviceBuffers buf(&slot);  // arena for the temporaries; goes back when this block ends
    buf.reserve(n * (sizeof(int32_t) + 2 * sizeof(double) + sizeof(uint32_t)) + (size_t(8) << 20));
    int32_t* d_voxel = nullptr;
    double *d_range = nullptr, *d_scale = nullptr;
    uint32_t *kept = nullptr, *d_count = nullptr;
    unsigned int* cnt = nullptr;
    PrimTmp t_select;
    e = buf.alloc(&d_voxel, n);
    if (e == hipSuccess) e = buf.alloc(&d_range, n);
    if (e == hipSuccess) e = buf.alloc(&cnt, size_t(nos::kRaycastWords));
    if (e == hipSuccess && out_scan) e = buf.alloc(&d_scale, n);
    if (e == hipSuccess && out_scan) e = buf.alloc(&kept, n);
    if (e == hipSuccess && out_scan) e = buf.alloc(&d_count, 1);
    const nos::RaycastHit is_hit{d_voxel};
    const rocprim::counting_iterator<uint32_t> positions(0u);
    const auto select = [&](void* tmp, size_t& bytes) { return rocprim::select(tmp, bytes, positions, kept, d_count, n, is_hit, st); };
    if (e == hipSuccess && out_scan) e = prim_plan(buf, select, t_select);
    if (e == hipSuccess) e = hipMemsetAsync(cnt, 0, sizeof h_cnt, st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::voxel_raycast_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, vm->view, rays->d_planes,
                         uint64_t(n), pose, prm, d_voxel, d_range, d_scale, cnt);
      e = hipGetLastError();
    }
    if (e == hipSuccess && out_scan) e = prim_run(select, t_select);
    if (e == hipSuccess && out_scan) e = hipMemcpyAsync(&n_kept, d_count, sizeof n_kept, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && voxel_out) e = hipMemcpyAsync(h_voxel.data(), d_voxel, n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && range_out) e = hipMemcpyAsync(h_range.data(), d_range, n * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the first wait: counters, results, and what sizes the new scan
    if (e != hipSuccess) return hip_fail(e, "voxel store ray cast");
    if (h_cnt[nos::kRaycastProbeError] != 0)
      return fail(NOS_ERR_HIP, "voxel store ray cast failed: a table probe or a ray's walk ran past its bound");
    if (out_scan && n_kept != h_cnt[nos::kRaycastHits])
      return fail(NOS_ERR_HIP, "voxel store ray cast: inconsistent hit count (%u selected, %u counted)", n_kept, h_cnt[nos::kRaycastHits]);
    if (out_scan && n_kept == 0) {
      e = hits->alloc(0, false);
      if (e != hipSuccess) return hip_fail(e, "voxel store ray cast (empty scan)");
    } else if (out_scan) {
      e = hits->alloc(n_kept, true);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(nos::voxel_raycast_gather_kernel, dim3((n_kept + 255) / 256), dim3(256), 0, st, rays->d_planes, uint32_t(n),
                           rays->d_order, kept, n_kept, d_scale, prm.origin[0], prm.origin[1], prm.origin[2], hits->scan->d_planes,
                           hits->scan->d_order);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipStreamSynchronize(st);  // the second wait: the gather has read the arena's arrays
      if (e != hipSuccess) return hip_fail(e, "voxel store ray cast (hit points)");
    }
  }
  if (voxel_out) std::memcpy(voxel_out, h_voxel.data(), n * sizeof(int32_t));
  if (range_out) std::memcpy(range_out, h_range.data(), n * sizeof(double));
  if (out_scan) *out_scan = hits->release();
  if (n_hit) *n_hit = h_cnt[nos::kRaycastHits];
  if (n_skipped) *n_skipped = h_cnt[nos::kRaycastSkipped];
  return NOS_OK;
}

// One export.  rule == nullptr: the first n_voxels entries of key, count, acc and stamp as they are, one
// wait.  Otherwise a prune's keep flags and their scan (KeepPass), the wait that tells how many slots are selected, the
// gather of those slots into arena arrays, the wait for the data.  Nothing of the store is written; `out` is written
// once nothing can fail any more.
inline int store_export(nos_voxel_map* vm, const nos::VoxelKeepRule* rule, int side, nos_voxel_state* out) {
  const size_t V = vm->n_voxels;
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  DeviceBuffers buf(&slot);
  const nos::VoxelStoreView& v = vm->view;
  const uint64_t* d_key = v.key;
  const uint32_t *d_count = v.count, *d_stamp = v.stamp;
  const double* d_acc = v.acc;
  size_t m = V;
  hipError_t e = V > 0 ? hipSetDevice(slot.device) : hipSuccess;
  if (e != hipSuccess) return hip_fail(e, "voxel store export");
  if (rule && V > 0) {
    KeepPass pass(vm);
    buf.reserve(V * 2 * sizeof(uint32_t) + (size_t(1) << 20));
    e = pass.plan(buf);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::voxel_keep_kernel, pass.grid, dim3(256), 0, st, v, *rule, pass.keep, vm->d_info);
      e = hipGetLastError();
    }
    if (e != hipSuccess) return hip_fail(e, "voxel store export (keep)");
    unsigned int h_info[nos::kInfoWords] = {};
    const int rc = pass.wait(h_info, nos::kInfoRemoved, 4);  // wait 1 of 2: how many slots go out
    if (rc != NOS_OK) return rc;
    m = side == NOS_STATE_REMOVED ? size_t(pass.totals[0]) : V - size_t(pass.totals[0]);
    if (m > 0) {
      uint64_t* g_key = nullptr;
      uint32_t *g_count = nullptr, *g_stamp = nullptr;
      double* g_acc = nullptr;
      buf.reserve(m * (sizeof(uint64_t) + 2 * sizeof(uint32_t) + 9 * sizeof(double)) + (size_t(1) << 20));
      e = buf.alloc(&g_key, m);
      if (e == hipSuccess) e = buf.alloc(&g_count, m);
      if (e == hipSuccess) e = buf.alloc(&g_acc, m * 9);
      if (e == hipSuccess) e = buf.alloc(&g_stamp, m);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(nos::voxel_state_gather_kernel, pass.grid, dim3(256), 0, st, v, pass.keep, pass.new_slot,
                           side == NOS_STATE_REMOVED ? 0u : 1u, g_key, g_count, g_acc, g_stamp);
        e = hipGetLastError();
      }
      if (e != hipSuccess) return hip_fail(e, "voxel store export (gather)");
      d_key = g_key, d_count = g_count, d_acc = g_acc, d_stamp = g_stamp;
    }
  }
  std::vector<uint64_t> h_keys(m);
  std::vector<int64_t> cells(m * 3);
  std::vector<uint32_t> counts(m), stamps(m);
  std::vector<double> sums(m * 9);
  if (m > 0) {
    e = hipMemcpyAsync(h_keys.data(), d_key, m * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(counts.data(), d_count, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(sums.data(), d_acc, m * 9 * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(stamps.data(), d_stamp, m * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the wait for the data
    if (e != hipSuccess) return hip_fail(e, "voxel store export (download)");
  }
  unsigned long long points = 0;
  for (size_t i = 0; i < m; ++i) {
    int32_t c[3];
    nos::unpack_cell(h_keys[i], c);
    for (int k = 0; k < 3; ++k) cells[3 * i + k] = c[k];
    points += counts[i];
  }
  out->voxel_resolution = vm->voxel_resolution, out->search_radius_sq = vm->search_radius_sq, out->flags = vm->flags;
  out->epoch = vm->epoch, out->n_points = points;
  out->cells.swap(cells), out->counts.swap(counts), out->sums.swap(sums), out->stamps.swap(stamps);
  return NOS_OK;
}

// The store as whatever matches against it is handed it: the view the live matcher reads (nothing of it is written), the
// two words of d_info a match may write, the cells the search ball spans per axis.
inline LiveStore live_store(const nos_voxel_map* vm) {
  const nos::VoxelStoreView& v = vm->view;
  nos::VoxelMatchView view{};
  view.table_key = v.table_key;
  view.table_slot = v.table_slot;
  view.mean = v.mean;
  view.sqrt_info = v.sqrt_info;
  view.valid = v.valid;
  view.table_mask = v.table_mask;
  view.inv_res = 1.0 / vm->voxel_resolution;  // what voxel_points_kernel is handed
  view.reach = std::sqrt(vm->search_radius_sq) + nos::kVoxelMatchGuard * vm->voxel_resolution;
  view.radius_sq = vm->search_radius_sq;
  static_assert(nos::kInfoMatches % 2 == 0 && nos::kInfoMatches + 2 <= nos::kInfoWords, "info layout");
  return LiveStore{vm->ctx, view, reinterpret_cast<unsigned long long*>(vm->d_info + nos::kInfoMatches),
                   vm->d_info + nos::kInfoProbeError, 2.0 * std::sqrt(vm->search_radius_sq) / vm->voxel_resolution + 2.0,
                   vm->broken};
}

// What both matches against the store reject: check_match_call's list (the dtype in it, ahead of max_neighbors), then
// what only a store adds.
inline int check_store_match(const nos_voxel_map* vm, const nos_scan* scan, const double* R, const double* t, nos_dataset** out_ds,
                             int max_neighbors, int dtype) {
  const int rc = check_match_call(vm ? vm->ctx : nullptr, scan, R, t, out_ds, max_neighbors, dtype);
  if (rc != NOS_OK) return rc;
  if (vm->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "matching against a voxel store needs a single-device context");
  return check_live_store(live_store(vm));
}

// The compact table of an indexed match, queued behind the search that wrote `ids` — n_keys store slots
// or -1 (plane 1, all -1 when max_neighbors = 1, is left out): *rows = the distinct ids, ascending (radix sort over the
// bits a slot can have, then unique; 0xFFFFFFFF, the key of -1, last when some id is absent), every id replaced by its
// rank among them, their number in *n_rows after the caller's wait.  All memory is the arena's, which the caller's
// buf.reserve sized by the scan: nothing here allocates or waits while the search is in flight.
inline hipError_t compact_ids(size_t capacity, DeviceSlot& slot, DeviceBuffers& buf, int32_t* ids, size_t n_keys, uint32_t** rows,
                              uint32_t* n_rows) {
  hipStream_t st = slot.stream;
  int key_bits = 1;  // a slot is < capacity = 2^c, and -1 has bit c set: c + 1 bits order both
  while ((size_t(1) << (key_bits - 1)) < capacity) ++key_bits;
  uint32_t *sorted = nullptr, *d_n_rows = nullptr;
  PrimTmp t_sort, t_unique;
  uint32_t* keys = reinterpret_cast<uint32_t*>(ids);  // -1 reads as 0xFFFFFFFF: after every slot
  const auto sort = [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, keys, sorted, n_keys, 0, key_bits, st); };
  const auto unique = [&](void* t, size_t& b) { return rocprim::unique(t, b, sorted, *rows, d_n_rows, n_keys, rocprim::equal_to<uint32_t>(), st); };
  hipError_t e = buf.alloc(&sorted, n_keys);
  if (e == hipSuccess) e = buf.alloc(rows, n_keys);
  if (e == hipSuccess) e = buf.alloc(&d_n_rows, 1);
  if (e == hipSuccess && n_keys > 0) e = prim_size(sort, t_sort);
  if (e == hipSuccess && n_keys > 0) e = prim_size(unique, t_unique);
  if (e == hipSuccess) e = prim_share(buf, {&t_sort, &t_unique});
  if (e == hipSuccess) e = hipMemsetAsync(d_n_rows, 0, sizeof(uint32_t), st);
  if (e == hipSuccess && n_keys > 0) {
    e = prim_run(sort, t_sort);
    if (e == hipSuccess) e = prim_run(unique, t_unique);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(voxel_rank_ids_kernel, dim3(unsigned((n_keys + 255) / 256)), dim3(256), 0, st, ids, uint64_t(n_keys),
                         *rows, d_n_rows);
      e = hipGetLastError();
    }
    // bracket profiling, SELF-REPORTED like start_match's launch: the kernel above and one per rocPRIM call (whose own
    // launches depend on the number of keys and key bits)
    if (slot.prof_on && slot.prof_every == 0) slot.prof_launches += 3;
  }
  if (e == hipSuccess) e = hipMemcpyAsync(n_rows, d_n_rows, sizeof *n_rows, hipMemcpyDeviceToHost, st);
  return e;
}

// The items of the map-to-map match (match_host.hpp's run_match_over): a store's voxels where every other match has a
// scan's points — one lane per slot of `source`, two dataset slots each; nothing of the store is written.  rot: the
// pose's rotation once more, for the kernel's algebra (voxeld2d_kernels.hpp).
struct StoreVoxels {
  const nos_voxel_map* source;
  nos::RotPod rot;
  static constexpr const char* kForm = "map-to-map ";
  StoreVoxels(const nos_voxel_map* s, const nos::PosePod& pose) : source(s) {
    for (int k = 0; k < 9; ++k) rot.R[k] = pose.R[k];
  }
  size_t n() const { return source->n_voxels; }
  template <typename F>
  void lead(F f) const {
    const nos::VoxelStoreView& sv = source->view;
    f(static_cast<const unsigned char*>(sv.valid), static_cast<const double*>(sv.mean), static_cast<const double*>(sv.sqrt_info),
      rot);
  }
};

// The two batched registrations against the store, which differ in `dof` only.
inline int voxel_map_register(int dof, nos_voxel_map* vm, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                              const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                              nos_register_report* reports) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm) return register_live(dof, nullptr, scans, n_problems, R, t, loss, ropt, options, reports);
  const LiveStore store = live_store(vm);
  return register_live(dof, &store, scans, n_problems, R, t, loss, ropt, options, reports);
}

}  // namespace nosd
