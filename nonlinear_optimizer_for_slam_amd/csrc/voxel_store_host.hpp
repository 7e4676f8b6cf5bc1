// voxel_store_host.hpp — the incremental NDT voxel store and everything that writes it: its memory (one
// block per capacity, adopt_block), the mutators — insert, merge (§22), prune, carve (§25), restore and add (§31) — and the
// two passes they are made of (GroupPass: a batch grouped by cell, §19; KeepPass: keep flags and the compaction behind
// them).  What only reads the store is in voxel_query_host.hpp; both are part of nos_voxelmap.hip, the one unit that
// includes them, which holds the entry points.
#pragma once

#include "group_host.hpp"

#include "voxelmap_kernels.hpp"
#include "voxelmerge_kernels.hpp"
#include "voxelcarve_kernels.hpp"
#include "voxelstate_kernels.hpp"

struct nos_voxel_map {
  nos_ctx* ctx = nullptr;
  double voxel_resolution = 1.0;
  double search_radius_sq = 1.0;
  int flags = 0;
  size_t capacity = 0;            // slots the arrays have room for (a power of two); the table has 2 * capacity entries
  size_t min_capacity = 0;        // the capacity the store was created with: a prune never shrinks below it
  uint32_t n_voxels = 0;          // slots in use
  size_t n_valid = 0;
  unsigned long long n_points = 0;
  unsigned long long epoch = 0;   // inserts that merged at least one point; a slot's stamp is the epoch of its last touch
  unsigned long long generation = 0;  // times d_block was replaced (growth, a prune that removed something)
  void* d_block = nullptr;        // the ONE allocation behind the arrays and the table of `view`
  size_t block_bytes = 0;
  unsigned int* d_info = nullptr; // [nos::kInfoWords]
  bool broken = false;            // a merge reported a probe error: the store's content is undefined
  nos::VoxelStoreView view{};
};

// A store's state on the host, whole or in part: what nos_voxel_map_export returns.
struct nos_voxel_state {
  double voxel_resolution = 1.0;
  double search_radius_sq = 1.0;
  int flags = 0;
  unsigned long long epoch = 0;     // the store's at the export
  unsigned long long n_points = 0;  // the counts below, added up
  std::vector<int64_t> cells;       // [n][3]
  std::vector<uint32_t> counts;     // [n]
  std::vector<double> sums;         // [n][9] about the cell corner, the store's own
  std::vector<uint32_t> stamps;     // [n]
};

namespace nosd {

// What a merge, a carve and a ray cast reject of their pose.  origin: the sensor's, which the last two check along with t.
inline int check_pose_finite(const double R[9], const double t[3], const double* origin = nullptr) {
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(R[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "R has a non-finite entry");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t[k]) || (origin && !std::isfinite(origin[k])))
      return fail(NOS_ERR_INVALID_ARGUMENT, "%s has a non-finite entry", origin ? "t or origin" : "t");
  return NOS_OK;
}

// A ray's trip count, which a carve and a ray cast bound: at most ceil(max_range / res) + 1 steps per axis.
inline int check_ray_reach(double max_range, double res) {
  if (3.0 * (std::ceil(max_range / res) + 1.0) > double(NOS_CARVE_MAX_CELLS))
    return fail(NOS_ERR_UNSUPPORTED, "max_range spans more than NOS_CARVE_MAX_CELLS cells: 3 (ceil(max_range / resolution) + 1) > %d",
                NOS_CARVE_MAX_CELLS);
  return NOS_OK;
}

// What the finish of a voxel (voxel_finish.hpp) runs with in this store, whichever kernel calls it.
inline nos::MapBuildParams finish_params(const nos_voxel_map* vm) {
  return nos::MapBuildParams{5, 0.01, 0.01, (vm->flags & NOS_MAP_PROPER_SQRT_INFORMATION) ? 1 : 0, vm->voxel_resolution};
}

// Arrays and table for `capacity` slots in one allocation; the table's keys start empty (queued on the slot's stream).
inline hipError_t store_alloc(DeviceSlot& slot, size_t capacity, void** block, size_t* block_bytes, nos::VoxelStoreView* v) {
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t table = 2 * capacity;
  const size_t b_key = up(capacity * sizeof(uint64_t)), b_count = up(capacity * sizeof(uint32_t));
  const size_t b_acc = up(capacity * 9 * sizeof(double)), b_mean = up(capacity * 3 * sizeof(double));
  const size_t b_S = up(capacity * 9 * sizeof(double)), b_valid = up(capacity), b_stamp = up(capacity * sizeof(uint32_t));
  const size_t b_tkey = up(table * sizeof(unsigned long long)), b_tslot = up(table * sizeof(uint32_t));
  char* base = nullptr;
  const size_t bytes = b_key + b_count + b_acc + b_mean + b_S + b_valid + b_stamp + b_tkey + b_tslot;
  hipError_t e = device_alloc(slot, &base, bytes);
  if (e != hipSuccess) return e;
  char* p = base;
  v->key = reinterpret_cast<uint64_t*>(p), p += b_key;
  v->count = reinterpret_cast<uint32_t*>(p), p += b_count;
  v->acc = reinterpret_cast<double*>(p), p += b_acc;
  v->mean = reinterpret_cast<double*>(p), p += b_mean;
  v->sqrt_info = reinterpret_cast<double*>(p), p += b_S;
  v->valid = reinterpret_cast<unsigned char*>(p), p += b_valid;
  v->stamp = reinterpret_cast<uint32_t*>(p), p += b_stamp;
  v->table_key = reinterpret_cast<unsigned long long*>(p), p += b_tkey;
  v->table_slot = reinterpret_cast<uint32_t*>(p);
  v->table_mask = uint32_t(table - 1);
  e = hipMemsetAsync(v->table_key, 0xFF, table * sizeof(unsigned long long), slot.stream);
  if (e != hipSuccess) {
    (void)hipFree(base);
    return e;
  }
  *block = base;
  *block_bytes = bytes;
  return hipSuccess;
}

// How store_reserve, a keep pass's compaction and a restore end (e, probe_error: what filling the new block gave, after the
// wait that lets the old one go): a failure frees the new block and leaves the store untouched; else the store's arrays
// and table are the new ones.  counter_what != nullptr: the fill left the block's valid count in kInfoKeptValid, and when
// nothing failed the device-side valid counter follows first (in stream order before any later merge), a failure of that
// copy going by this name; nullptr: the caller has no counter to move.
inline int adopt_block(nos_voxel_map* vm, hipError_t e, unsigned int probe_error, const char* what, const char* counter_what,
                       const char* overflow, void* block, size_t block_bytes, const nos::VoxelStoreView& view, size_t capacity) {
  if (e == hipSuccess && probe_error == 0 && counter_what) {
    e = hipMemcpyAsync(vm->d_info + nos::kInfoValid, vm->d_info + nos::kInfoKeptValid, sizeof(unsigned int), hipMemcpyDeviceToDevice,
                       vm->ctx->slots[0].stream);
    what = counter_what;
  }
  if (e != hipSuccess || probe_error != 0) {
    (void)hipFree(block);
    if (e != hipSuccess) return hip_fail(e, what);
    return fail(NOS_ERR_HIP, "%s", overflow);
  }
  (void)hipFree(vm->d_block);
  vm->d_block = block;
  vm->block_bytes = block_bytes;
  vm->view = view;
  vm->capacity = capacity;
  ++vm->generation;
  return NOS_OK;
}

// Room for `need` slots: arrays and table double (new allocation, device copies, every key hashed into the new table)
// until they hold them.  The store is untouched when this fails.
inline int store_reserve(nos_voxel_map* vm, size_t need) {
  if (need <= vm->capacity) return NOS_OK;
  if (need > (size_t(1) << 30)) return fail(NOS_ERR_UNSUPPORTED, "too many voxels for one store");
  size_t capacity = vm->capacity;
  while (capacity < need) capacity *= 2;
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  void* block = nullptr;
  size_t block_bytes = 0;
  nos::VoxelStoreView nv{};
  hipError_t e = store_alloc(slot, capacity, &block, &block_bytes, &nv);
  if (e != hipSuccess) return hip_fail(e, "growing the voxel store");
  const size_t V = vm->n_voxels;
  nv.n_voxels = vm->n_voxels;
  unsigned int err = 0;
  if (V > 0) {
    const nos::VoxelStoreView& ov = vm->view;
    e = hipMemcpyAsync(nv.key, ov.key, V * sizeof(uint64_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nv.count, ov.count, V * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nv.acc, ov.acc, V * 9 * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nv.mean, ov.mean, V * 3 * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nv.sqrt_info, ov.sqrt_info, V * 9 * sizeof(double), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nv.valid, ov.valid, V, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(nv.stamp, ov.stamp, V * sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(vm->d_info + nos::kInfoProbeError, 0, sizeof(unsigned int), st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::voxel_rehash_kernel, dim3(unsigned((V + 255) / 256)), dim3(256), 0, st, nv, vm->d_info);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&err, vm->d_info + nos::kInfoProbeError, sizeof err, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the old block is freed by adopt_block
  // the three texts: what failed, the counter's copy (none: a copy of the slots in use keeps their valid flags), overflow
  return adopt_block(vm, e, err, "growing the voxel store", nullptr, "growing the voxel store failed: the new table overflowed",
                     block, block_bytes, nv, capacity);
}

// The back half of an insert and of a merge, ONE copy: U runs (keys ascending and unique, their counts, their nine sums
// about the corner of the key's cell) go into the store — room for them, lookup, rank of the misses, voxel_merge_kernel
// (count += n, acc += seg, the finish, stamp = epoch + 1), the closing wait and the bookkeeping.  Nothing of the store is
// written before the merge kernel; `buf` is the caller's arena, `points` what the runs hold together.  A run that would
// take its voxel past 2^32 − 1 points is flagged by the lookup, the merge kernel then writes nothing, and the closing
// wait brings the flag with the words it reads anyway: the call is rejected with the store as it was (its capacity
// aside), naming `member` (e.g. "point") number names.member_idx[...] of that run.
inline int store_merge_runs(nos_voxel_map* vm, DeviceBuffers& buf, const uint64_t* run_key, const uint32_t* run_count,
                            const double* seg_acc, uint32_t U, unsigned long long points, const nos::VoxelRunNames& names,
                            const char* member, const char* what, size_t* n_touched) {
  hipStream_t st = vm->ctx->slots[0].stream;
  unsigned int h_info[nos::kInfoWords] = {};
  uint32_t *run_slot = nullptr, *miss = nullptr, *rank = nullptr;
  int rc = store_reserve(vm, size_t(vm->n_voxels) + U);  // load factor <= 1/2 whatever the number of new voxels
  if (rc != NOS_OK) return rc;
  PrimTmp t_rank;
  const auto rank_misses = [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, miss, rank, 0u, size_t(U), rocprim::plus<uint32_t>(), st); };
  hipError_t e = buf.alloc(&run_slot, U);
  if (e == hipSuccess) e = buf.alloc(&miss, U);
  if (e == hipSuccess) e = buf.alloc(&rank, U);
  if (e == hipSuccess) e = prim_plan(buf, rank_misses, t_rank);
  if (e != hipSuccess) return hip_fail(e, what);
  const dim3 ugrid(unsigned((size_t(U) + 255) / 256));
  hipLaunchKernelGGL(nos::voxel_lookup_kernel, ugrid, dim3(256), 0, st, vm->view, run_key, run_count, names, U, run_slot, miss,
                     vm->d_info);
  e = hipGetLastError();
  if (e == hipSuccess) e = prim_run(rank_misses, t_rank);
  if (e != hipSuccess) return hip_fail(e, what);  // still nothing written
  hipLaunchKernelGGL(nos::voxel_merge_kernel, ugrid, dim3(256), 0, st, vm->view, run_key, run_count, seg_acc, run_slot, rank, U,
                     finish_params(vm), uint32_t(vm->epoch + 1), vm->d_info);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(h_info, vm->d_info, 5 * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the wait at the end
  if (e != hipSuccess || h_info[nos::kInfoProbeError] != 0) {
    vm->broken = true;
    if (e != hipSuccess) return hip_fail(e, what);
    return fail(NOS_ERR_HIP, "%s failed: a table probe found no free entry", what);
  }
  if (h_info[nos::kInfoFarPoint] != 0)  // the merge kernel wrote nothing: the store is as it was
    return fail(NOS_ERR_UNSUPPORTED, "%s %u takes its destination voxel past 2^32 - 1 points", member, h_info[nos::kInfoFarPoint] - 1u);
  vm->n_voxels += h_info[nos::kInfoNew];
  vm->view.n_voxels = vm->n_voxels;
  vm->n_valid = size_t(int(h_info[nos::kInfoValid]));
  vm->n_points += points;
  ++vm->epoch;  // what the merge stamped the touched slots with
  if (n_touched) *n_touched = U;
  return NOS_OK;
}

// The front half of an insert, of a merge and of an add, ONE copy: a batch of n keyed items is grouped by
// cell.  open: the device and the size of the arena, from which the caller then takes its own arrays.  plan: the groups'
// arrays and all rocPRIM planning, then the four info words (bad, far, probe error, new) zeroed — all ahead of the
// caller's first kernel, which writes g.keys, g.idx and the flags.  The caller queues the grouping (g.queue) among its own
// kernels.  wait: the first n_words info words into h_info and the ONE wait in the middle, which also brings the run
// count g.queue asked for.  Nothing of the store is written before it; what the flags reject, and in which words, is the
// caller's.  `buf` goes on to store_merge_runs.
struct GroupPass {
  nos_voxel_map* vm;
  DeviceSlot& slot;
  hipStream_t st;
  DeviceBuffers buf;      // arena: every temporary comes from the slot's buffer pool — no hipMalloc / hipFree per call
  KeyGroups<uint64_t> g;  // a run = the items of one cell, in item order
  explicit GroupPass(nos_voxel_map* m) : vm(m), slot(m->ctx->slots[0]), st(slot.stream), buf(&slot) {}
  hipError_t open(size_t arena_bytes) {
    const hipError_t e = hipSetDevice(slot.device);
    buf.reserve(arena_bytes);
    return e;
  }
  hipError_t plan(size_t n) {
    hipError_t e = g.arrays(buf, st, n);
    if (e == hipSuccess) e = g.temporaries(buf, 63);
    if (e == hipSuccess) e = hipMemsetAsync(vm->d_info, 0, 4 * sizeof(unsigned int), st);
    return e;
  }
  hipError_t wait(unsigned int* h_info, int n_words) {
    hipError_t e = hipMemcpyAsync(h_info, vm->d_info, size_t(n_words) * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
  }
};

// One insert.  host_xyz != nullptr: [n][3] in the map frame; otherwise d_planes = 3 planes of n doubles in a local frame,
// warped by `pose` on the device, `order` the scan's original indices when it was sorted by cell (else nullptr).
inline int store_insert(nos_voxel_map* vm, size_t n, const double* host_xyz, const double* d_planes, const uint32_t* order,
                        const nos::PosePod& pose, size_t* n_touched) {
  if (const int rc = check_usable(vm->broken); rc != NOS_OK) return rc;
  if (n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points for one insert");
  if (n == 0) {
    if (n_touched) *n_touched = 0;
    return NOS_OK;
  }
  GroupPass pass(vm);  // the batch grouped by voxel: a run = the points of one voxel, in point order
  KeyGroups<uint64_t>& g = pass.g;
  hipStream_t st = pass.st;
  double *rec = nullptr, *staged = nullptr, *seg_acc = nullptr;
  hipError_t e = pass.open(n * (7 * sizeof(double) + 3 * sizeof(uint64_t) + 4 * sizeof(uint32_t)) + (size_t(16) << 20));
  if (e == hipSuccess) e = pass.buf.alloc(&rec, n * 4);
  if (e == hipSuccess && host_xyz) e = pass.buf.alloc(&staged, n * 3);
  if (e == hipSuccess) e = pass.plan(n);
  // step 1: records, keys, the finite / in-range check
  unsigned int h_info[nos::kInfoWords] = {};
  uint32_t U = 0;
  if (e == hipSuccess && host_xyz) e = hipMemcpyAsync(staged, host_xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    const dim3 grid(unsigned((n + 255) / 256));
    const double inv_res = 1.0 / vm->voxel_resolution;
    if (host_xyz)
      hipLaunchKernelGGL((nos::voxel_points_kernel<false>), grid, dim3(256), 0, st, staged, uint64_t(n), pose, inv_res, rec, g.keys,
                         g.idx, vm->d_info);
    else
      hipLaunchKernelGGL((nos::voxel_points_kernel<true>), grid, dim3(256), 0, st, d_planes, uint64_t(n), pose, inv_res, rec, g.keys,
                         g.idx, vm->d_info);
    e = hipGetLastError();
  }
  // step 2: stable sort of (packed key, index), run-length encode.  The packed key orders cells exactly as the build's
  // compact in-box key does, so a run's points are summed in the order the build sums them.
  if (e == hipSuccess) e = g.queue(&U);
  if (e == hipSuccess) e = pass.wait(h_info, 2);  // the one wait in the middle: run count and flags
  if (e != hipSuccess) return hip_fail(e, "voxel store insert (sort)");
  // nothing of the store has been written so far: a rejected batch leaves it as it was
  if (h_info[nos::kInfoBadPoint] != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "point %u has a non-finite coordinate", h_info[nos::kInfoBadPoint] - 1u);
  if (h_info[nos::kInfoFarPoint] != 0)
    return fail(NOS_ERR_UNSUPPORTED, "point %u lies outside the addressable grid (+-2^20 cells per axis)",
                h_info[nos::kInfoFarPoint] - 1u);
  // step 3: the build's sums kernel on the batch; step 4 (store_merge_runs): lookup, rank of the misses, merge + finish
  pass.buf.reserve(size_t(U) * (9 * sizeof(double) + 3 * sizeof(uint32_t)) + (size_t(1) << 20));
  e = pass.buf.alloc(&seg_acc, size_t(U) * 9);
  if (e == hipSuccess) e = g.queue_offsets(U);
  if (e != hipSuccess) return hip_fail(e, "voxel store insert (segments)");
  e = launch_voxel_sums(rec, g.idx_sorted, g.offsets, g.counts, U, 1.0 / vm->voxel_resolution, vm->voxel_resolution, seg_acc, st);
  if (e != hipSuccess) return hip_fail(e, "voxel store insert (sums)");
  return store_merge_runs(vm, pass.buf, g.uniq, g.counts, seg_acc, U, n, nos::VoxelRunNames{g.idx_sorted, g.offsets, order}, "point",
                          "voxel store insert", n_touched);
}

// One merge of `src` into `dst` under `pose`: the source's slots become moment records about destination
// cells, grouped by destination cell and added up per cell; the wait in the middle reads the run count and the flags, and
// nothing of the destination is written before it.  The source is only read.
inline int store_merge(nos_voxel_map* dst, const nos_voxel_map* src, const nos::PosePod& pose, size_t* n_touched) {
  if (const int rc = check_usable(dst->broken || src->broken); rc != NOS_OK) return rc;
  const size_t n = src->n_voxels;
  if (n == 0) {
    if (n_touched) *n_touched = 0;
    return NOS_OK;
  }
  GroupPass pass(dst);  // the source's slots grouped by destination cell: a run = the voxels that land in one cell, in slot order
  KeyGroups<uint64_t>& g = pass.g;
  hipStream_t st = pass.st;
  double *mom = nullptr, *seg_acc = nullptr;
  uint32_t *mom_count = nullptr, *seg_count = nullptr;
  hipError_t e = pass.open(n * (18 * sizeof(double) + 3 * sizeof(uint64_t) + 9 * sizeof(uint32_t)) + (size_t(16) << 20));
  if (e == hipSuccess) e = pass.buf.alloc(&mom, n * 9);
  if (e == hipSuccess) e = pass.buf.alloc(&mom_count, n);
  if (e == hipSuccess) e = pass.buf.alloc(&seg_acc, n * 9);
  if (e == hipSuccess) e = pass.buf.alloc(&seg_count, n);
  if (e == hipSuccess) e = pass.plan(n);
  unsigned int h_info[nos::kInfoWords] = {};
  uint32_t U = 0;
  const dim3 grid(unsigned((n + 255) / 256));
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_moments_kernel, grid, dim3(256), 0, st, src->view, src->voxel_resolution, pose,
                       dst->voxel_resolution, 1.0 / dst->voxel_resolution, mom, mom_count, g.keys, g.idx, dst->d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = g.queue(&U);
  if (e == hipSuccess) e = g.queue_offsets(uint32_t(n));  // over the most runs there can be: their number is still on its way
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_moment_sums_kernel, grid, dim3(256), 0, st, mom, mom_count, g.idx_sorted, g.offsets,
                       g.counts, g.n_runs, seg_acc, seg_count, dst->d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = pass.wait(h_info, 2);  // the one wait in the middle: run count and flags
  if (e != hipSuccess) return hip_fail(e, "voxel store merge (sums)");
  // nothing of the destination has been written so far: a rejected merge leaves it as it was
  if (h_info[nos::kInfoBadPoint] != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "source voxel %u has non-finite moments under this pose", h_info[nos::kInfoBadPoint] - 1u);
  if (h_info[nos::kInfoFarPoint] != 0)
    return fail(NOS_ERR_UNSUPPORTED,
                "source voxel %u lands outside the addressable grid (+-2^20 cells per axis), or the source voxels of its "
                "destination cell hold more than 2^32 - 1 points together", h_info[nos::kInfoFarPoint] - 1u);
  return store_merge_runs(dst, pass.buf, g.uniq, seg_count, seg_acc, U, src->n_points,
                          nos::VoxelRunNames{g.idx_sorted, g.offsets, nullptr}, "source voxel", "voxel store merge", n_touched);
}

// The keep flags of a prune or of a carve and everything behind them, ONE copy.  plan: arena memory
// for the flags and their ranks, the scan's plan, the totals zeroed — all ahead of the caller's keep kernel, which writes
// keep[] and the totals.  wait: the exclusive scan of the flags, then the ONE wait, which brings `n_words` words of d_info
// from `first_word` on (the totals among them) into h_info.  compact: nothing to remove → nothing written, nothing
// allocated; else the survivors move to a fresh block in their old order and the table is rebuilt there, with the
// closing wait.  A failure at any point leaves the store as it was.
struct KeepPass {
  nos_voxel_map* vm;
  size_t V;
  hipStream_t st;
  dim3 grid;
  uint32_t *keep = nullptr, *new_slot = nullptr;
  PrimTmp t_slots;
  // removed voxels, their points (two words), valid voxels kept: words kInfoRemoved … kInfoKeptValid
  unsigned int totals[4] = {0, 0, 0, 0};
  explicit KeepPass(nos_voxel_map* m)
      : vm(m), V(m->n_voxels), st(m->ctx->slots[0].stream), grid(unsigned((size_t(m->n_voxels) + 255) / 256)) {}
  hipError_t scan(void* t, size_t& b) const { return rocprim::exclusive_scan(t, b, keep, new_slot, 0u, V, rocprim::plus<uint32_t>(), st); }
  hipError_t plan(DeviceBuffers& buf) {
    const auto new_slots = [&](void* t, size_t& b) { return scan(t, b); };
    hipError_t e = buf.alloc(&keep, V);
    if (e == hipSuccess) e = buf.alloc(&new_slot, V);
    if (e == hipSuccess) e = prim_plan(buf, new_slots, t_slots);
    static_assert(nos::kInfoKeptValid == nos::kInfoRemoved + 3 && nos::kInfoRemovedPoints == nos::kInfoRemoved + 1, "info layout");
    if (e == hipSuccess) e = hipMemsetAsync(vm->d_info + nos::kInfoRemoved, 0, sizeof totals, st);
    return e;
  }
  int wait(unsigned int* h_info, int first_word, int n_words) {
    const auto new_slots = [&](void* t, size_t& b) { return scan(t, b); };
    hipError_t e = prim_run(new_slots, t_slots);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h_info + first_word, vm->d_info + first_word, size_t(n_words) * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait: what goes?
    if (e != hipSuccess) return hip_fail(e, "voxel store prune (keep)");
    for (int k = 0; k < 4; ++k) totals[k] = h_info[nos::kInfoRemoved + k];
    return NOS_OK;
  }
  int compact(size_t* n_removed) {
    const size_t removed = totals[0];
    if (removed == 0) {  // the common per-frame case: nothing written, nothing allocated
      if (n_removed) *n_removed = 0;
      return NOS_OK;
    }
    const unsigned long long removed_points = (unsigned long long)totals[1] | ((unsigned long long)totals[2] << 32);
    const size_t kept = V - removed;
    size_t capacity = vm->capacity;
    if (kept <= vm->capacity / 4) {
      capacity = 16;
      while (capacity < 2 * kept) capacity *= 2;
      capacity = std::max(capacity, vm->min_capacity);
    }
    void* block = nullptr;
    size_t block_bytes = 0;
    nos::VoxelStoreView nv{};
    hipError_t e = store_alloc(vm->ctx->slots[0], capacity, &block, &block_bytes, &nv);
    if (e != hipSuccess) return hip_fail(e, "voxel store prune (new block)");
    nv.n_voxels = uint32_t(kept);
    unsigned int err = 0;
    e = hipMemsetAsync(vm->d_info + nos::kInfoProbeError, 0, sizeof(unsigned int), st);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(nos::voxel_compact_kernel, grid, dim3(256), 0, st, vm->view, nv, keep, new_slot, vm->d_info);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&err, vm->d_info + nos::kInfoProbeError, sizeof err, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // the closing wait: the old block is freed by adopt_block
    // the three texts: what failed, the counter's copy, overflow
    const int rc = adopt_block(vm, e, err, "voxel store prune (compact)", "voxel store prune (counter)",
                               "voxel store prune failed: the new table overflowed", block, block_bytes, nv, capacity);
    if (rc != NOS_OK) return rc;
    vm->n_voxels = uint32_t(kept);
    vm->n_valid = totals[3];
    vm->n_points -= removed_points;
    if (n_removed) *n_removed = removed;
    return NOS_OK;
  }
};

// What a prune and an export by selection read a nos_voxel_prune with, ONE copy: its validation in the header's order, the
// box bounds in cells, the age test's two words.  `what` is not NULL.
inline int keep_rule(const nos_voxel_map* vm, const nos_voxel_prune* what, nos::VoxelKeepRule* rule) {
  *rule = nos::VoxelKeepRule{};
  if (what->struct_size < sizeof(nos_voxel_prune)) return fail(NOS_ERR_INVALID_ARGUMENT, "struct_size is smaller than nos_voxel_prune");
  if (what->what == 0 || (what->what & ~(NOS_PRUNE_BOX | NOS_PRUNE_AGE)))
    return fail(NOS_ERR_INVALID_ARGUMENT, "what must be NOS_PRUNE_BOX, NOS_PRUNE_AGE or both");
  rule->use_box = (what->what & NOS_PRUNE_BOX) ? 1 : 0;
  rule->use_age = (what->what & NOS_PRUNE_AGE) ? 1 : 0;
  if (rule->use_box) {
    const double inv_res = 1.0 / vm->voxel_resolution;  // what voxel_points_kernel is handed
    const double lim = double(1 << 20);
    for (int k = 0; k < 3; ++k) {
      const double c = what->center[k], h = what->half_extent[k];
      if (!std::isfinite(c) || !std::isfinite(h) || h < 0.0)
        return fail(NOS_ERR_INVALID_ARGUMENT, "the box needs a finite center and a finite, non-negative half extent");
      // a cell survives iff it intersects the closed box; a box beyond the addressable grid keeps nothing
      const double lo = std::floor((c - h) * inv_res), hi = std::floor((c + h) * inv_res);
      rule->lo[k] = int32_t(std::min(std::max(lo, -lim), lim));
      rule->hi[k] = int32_t(std::min(std::max(hi, -lim - 1.0), lim - 1.0));
    }
  }
  rule->epoch = uint32_t(vm->epoch);
  rule->max_age = what->max_age > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(what->max_age);
  return NOS_OK;
}

// One prune: keep flags and totals by box and / or age, then KeepPass.
inline int store_prune(nos_voxel_map* vm, const nos::VoxelKeepRule& rule, size_t* n_removed) {
  if (vm->n_voxels == 0) {
    if (n_removed) *n_removed = 0;
    return NOS_OK;
  }
  DeviceSlot& slot = vm->ctx->slots[0];
  DeviceBuffers buf(&slot);
  KeepPass pass(vm);
  hipError_t e = hipSetDevice(slot.device);
  buf.reserve(pass.V * 2 * sizeof(uint32_t) + (size_t(1) << 20));
  if (e == hipSuccess) e = pass.plan(buf);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_keep_kernel, pass.grid, dim3(256), 0, pass.st, vm->view, rule, pass.keep, vm->d_info);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return hip_fail(e, "voxel store prune (keep)");
  unsigned int h_info[nos::kInfoWords] = {};
  const int rc = pass.wait(h_info, nos::kInfoRemoved, 4);
  return rc != NOS_OK ? rc : pass.compact(n_removed);
}

// One carve: the rays of `scan` under `pose` are walked through the grid (crossings and hits per slot,
// zeroed per call), the keep flags follow from the two counters, then KeepPass.  Waits: the one that reads totals, flags
// and the skipped count (it also brings the counters when the caller asked for them); the closing one of the compaction
// when something goes.  The outputs are written once nothing can fail any more.
inline int store_carve(nos_voxel_map* vm, const nos_scan* scan, const nos::PosePod& pose, const nos::VoxelCarveParams& prm,
                       uint32_t min_crossings, uint32_t min_hits, bool dry_run, size_t* n_removed, size_t* n_skipped,
                       uint32_t* crossings_out, uint32_t* hits_out) {
  const size_t n = scan->n;
  if (n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points for one carve");
  if (n == 0 || vm->n_voxels == 0) {  // nothing to walk, or nothing to find: every ray would count nothing
    if (n_removed) *n_removed = 0;
    if (n_skipped) *n_skipped = 0;
    if (crossings_out) std::memset(crossings_out, 0, size_t(vm->n_voxels) * sizeof(uint32_t));
    if (hits_out) std::memset(hits_out, 0, size_t(vm->n_voxels) * sizeof(uint32_t));
    return NOS_OK;
  }
  DeviceSlot& slot = vm->ctx->slots[0];
  DeviceBuffers buf(&slot);
  KeepPass pass(vm);
  const size_t V = pass.V;
  hipStream_t st = pass.st;
  uint32_t* counters = nullptr;  // crossings [V], then hits [V]
  std::vector<uint32_t> h_counters;
  const bool want_counts = crossings_out || hits_out;
  if (want_counts) h_counters.resize(2 * V);
  hipError_t e = hipSetDevice(slot.device);
  buf.reserve(V * 4 * sizeof(uint32_t) + (size_t(1) << 20));
  if (e == hipSuccess) e = buf.alloc(&counters, 2 * V);
  if (e == hipSuccess) e = pass.plan(buf);
  if (e == hipSuccess) e = hipMemsetAsync(counters, 0, 2 * V * sizeof(uint32_t), st);
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info + nos::kInfoProbeError, 0, sizeof(unsigned int), st);
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info + nos::kInfoSkipped, 0, sizeof(unsigned int), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_carve_walk_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, vm->view, scan->d_planes,
                       uint64_t(n), pose, prm, counters, counters + V, vm->d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_carve_keep_kernel, pass.grid, dim3(256), 0, st, vm->view, counters, counters + V, min_crossings,
                       min_hits, pass.keep, vm->d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess && want_counts)
    e = hipMemcpyAsync(h_counters.data(), counters, 2 * V * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return hip_fail(e, "voxel store carve (walk)");
  unsigned int h_info[nos::kInfoWords] = {};
  static_assert(nos::kInfoProbeError < nos::kInfoRemoved && nos::kInfoSkipped == nos::kInfoKeptValid + 1, "info layout");
  int rc = pass.wait(h_info, nos::kInfoProbeError, nos::kInfoSkipped - nos::kInfoProbeError + 1);
  if (rc != NOS_OK) return rc;
  if (h_info[nos::kInfoProbeError] != 0)  // the store was only read: it is as it was
    return fail(NOS_ERR_HIP, "voxel store carve failed: a table probe or a ray's walk ran past its bound");
  if (dry_run) {  // what would go; nothing of the store is written
    if (n_removed) *n_removed = h_info[nos::kInfoRemoved];
  } else {
    rc = pass.compact(n_removed);
    if (rc != NOS_OK) return rc;
  }
  if (n_skipped) *n_skipped = h_info[nos::kInfoSkipped];
  if (crossings_out) std::memcpy(crossings_out, h_counters.data(), V * sizeof(uint32_t));
  if (hits_out) std::memcpy(hits_out, h_counters.data() + V, V * sizeof(uint32_t));
  return NOS_OK;
}

// What a restore and an add say of a state that names cell `i` of cells_xyz more than once.
inline int fail_repeated_cell(const int64_t* cells_xyz, size_t i) {
  const int64_t* c = cells_xyz + 3 * i;
  return fail(NOS_ERR_INVALID_ARGUMENT, "cell (%lld, %lld, %lld) comes twice", (long long)c[0], (long long)c[1], (long long)c[2]);
}

// NOS_IMPORT_RESTORE into a store that holds no voxel: the n voxels as given become slots 0 … n − 1 of
// a FRESH block — keys, counts, sums and stamps copied in, voxel_restore_kernel for the rest — which adopt_block makes
// the store's only when nothing failed, a repeated cell included.  keys: the cells packed, on the host.
inline int store_restore(nos_voxel_map* vm, size_t n, const std::vector<uint64_t>& keys, const int64_t* cells_xyz,
                         const uint32_t* counts, const double* sums, const uint32_t* stamps, unsigned long long epoch,
                         size_t* n_touched) {
  if (n == 0) {
    vm->epoch = epoch;
    if (n_touched) *n_touched = 0;
    return NOS_OK;
  }
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  size_t capacity = vm->capacity;
  while (capacity < n) capacity *= 2;
  void* block = nullptr;
  size_t block_bytes = 0;
  nos::VoxelStoreView nv{};
  hipError_t e = hipSetDevice(slot.device);
  if (e == hipSuccess) e = store_alloc(slot, capacity, &block, &block_bytes, &nv);
  if (e != hipSuccess) return hip_fail(e, "voxel store restore (new block)");
  nv.n_voxels = uint32_t(n);
  unsigned int h_info[nos::kInfoWords] = {};
  e = hipMemcpyAsync(nv.key, keys.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(nv.count, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(nv.acc, sums, n * 9 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && stamps) e = hipMemcpyAsync(nv.stamp, stamps, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info, 0, 3 * sizeof(unsigned int), st);  // bad, far, probe error
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info + nos::kInfoRemoved, 0, 4 * sizeof(unsigned int), st);  // a keep pass's totals
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_restore_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, nv, uint32_t(n), stamps ? 1 : 0,
                       uint32_t(epoch), finish_params(vm), vm->d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_info, vm->d_info, nos::kInfoWords * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait; the old block is freed by adopt_block
  if (e == hipSuccess && h_info[nos::kInfoBadPoint] != 0) {
    (void)hipFree(block);
    return fail_repeated_cell(cells_xyz, h_info[nos::kInfoBadPoint] - 1u);
  }
  // the three texts: what failed, the counter's copy, overflow
  const int rc = adopt_block(vm, e, h_info[nos::kInfoProbeError], "voxel store restore", "voxel store restore (counter)",
                             "voxel store restore failed: the new table overflowed", block, block_bytes, nv, capacity);
  if (rc != NOS_OK) return rc;
  vm->n_voxels = uint32_t(n);
  vm->n_valid = h_info[nos::kInfoKeptValid];
  vm->n_points = (unsigned long long)h_info[nos::kInfoRemovedPoints] | ((unsigned long long)h_info[nos::kInfoRemovedPoints + 1] << 32);
  vm->epoch = epoch;
  if (n_touched) *n_touched = n;
  return NOS_OK;
}

// NOS_IMPORT_ADD: the state as ONE batch of an insert whose runs are given — its keys grouped by cell,
// counts and sums brought into that order (a repeated cell and a voxel taken past 2^32 − 1 points flagged on the way), the
// wait that reads the flags, then store_merge_runs.  Nothing of the store is written before that.
inline int store_add(nos_voxel_map* vm, size_t n, const std::vector<uint64_t>& keys, const int64_t* cells_xyz, const uint32_t* counts,
                     const double* sums, size_t* n_touched) {
  if (n == 0) {
    if (n_touched) *n_touched = 0;
    return NOS_OK;
  }
  GroupPass pass(vm);  // the state's voxels grouped by cell: every run has ONE member, or the state is rejected
  KeyGroups<uint64_t>& g = pass.g;
  hipStream_t st = pass.st;
  uint32_t *d_count = nullptr, *run_count = nullptr;
  double *d_acc = nullptr, *run_acc = nullptr;
  std::vector<uint32_t> iota(n);
  unsigned long long points = 0;
  for (size_t i = 0; i < n; ++i) iota[i] = uint32_t(i), points += counts[i];
  hipError_t e = pass.open(n * (18 * sizeof(double) + 3 * sizeof(uint64_t) + 9 * sizeof(uint32_t)) + (size_t(16) << 20));
  if (e == hipSuccess) e = pass.buf.alloc(&d_count, n);
  if (e == hipSuccess) e = pass.buf.alloc(&run_count, n);
  if (e == hipSuccess) e = pass.buf.alloc(&d_acc, n * 9);
  if (e == hipSuccess) e = pass.buf.alloc(&run_acc, n * 9);
  if (e == hipSuccess) e = pass.plan(n);
  unsigned int h_info[nos::kInfoWords] = {};
  uint32_t U = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(g.keys, keys.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(g.idx, iota.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_count, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_acc, sums, n * 9 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = g.queue(&U);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_state_runs_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, vm->view, g.keys_sorted,
                       g.idx_sorted, uint32_t(n), d_count, d_acc, run_count, run_acc, vm->d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = pass.wait(h_info, 3);  // the one wait in the middle: the flags
  if (e != hipSuccess) return hip_fail(e, "voxel store add (sort)");
  // nothing of the store has been written so far: a rejected state leaves it as it was
  if (h_info[nos::kInfoBadPoint] != 0) return fail_repeated_cell(cells_xyz, h_info[nos::kInfoBadPoint] - 1u);
  if (h_info[nos::kInfoFarPoint] != 0)
    return fail(NOS_ERR_UNSUPPORTED, "voxel %u of the state takes its destination voxel past 2^32 - 1 points", h_info[nos::kInfoFarPoint] - 1u);
  if (h_info[nos::kInfoProbeError] != 0) return fail(NOS_ERR_HIP, "voxel store add failed: a table probe found no free entry");
  // without a repeated cell the sorted keys ARE the runs' keys (U == n)
  return store_merge_runs(vm, pass.buf, g.keys_sorted, run_count, run_acc, uint32_t(n), points,
                          nos::VoxelRunNames{g.idx_sorted, nullptr, nullptr}, "voxel", "voxel store add", n_touched);
}

}  // namespace nosd
