// nos_voxelmap.hip — incremental NDT voxel store: a device-resident map that grows scan by scan; a batch
// is grouped by voxel through group_host.hpp (§19), matched against through match_host.hpp (§18); it forgets by box and age
// (prune, §13) and by line of sight (carve, §25); it answers what a sensor at a pose would see (ray cast, §32).
#define NOS_WITH_VOXEL_INDEX_KERNELS  // voxelmatch_kernels.hpp: this unit compiles (and launches) the two index kernels
#include "group_host.hpp"
#include "match_host.hpp"

#include "voxelmap_kernels.hpp"
#include "voxelmatch_kernels.hpp"
#include "voxelmerge_kernels.hpp"
#include "voxeld2d_kernels.hpp"
#include "voxelcarve_kernels.hpp"
#include "voxelraycast_kernels.hpp"
#include "voxelstate_kernels.hpp"

using namespace nosd;

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

namespace {

// Arrays and table for `capacity` slots in one allocation; the table's keys start empty.
hipError_t store_alloc(size_t capacity, hipStream_t st, void** block, size_t* block_bytes, nos::VoxelStoreView* v) {
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t table = 2 * capacity;
  const size_t b_key = up(capacity * sizeof(uint64_t)), b_count = up(capacity * sizeof(uint32_t));
  const size_t b_acc = up(capacity * 9 * sizeof(double)), b_mean = up(capacity * 3 * sizeof(double));
  const size_t b_S = up(capacity * 9 * sizeof(double)), b_valid = up(capacity), b_stamp = up(capacity * sizeof(uint32_t));
  const size_t b_tkey = up(table * sizeof(unsigned long long)), b_tslot = up(table * sizeof(uint32_t));
  char* base = nullptr;
  const size_t bytes = b_key + b_count + b_acc + b_mean + b_S + b_valid + b_stamp + b_tkey + b_tslot;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&base), bytes);
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
  e = hipMemsetAsync(v->table_key, 0xFF, table * sizeof(unsigned long long), st);
  if (e != hipSuccess) {
    (void)hipFree(base);
    return e;
  }
  *block = base;
  *block_bytes = bytes;
  return hipSuccess;
}

// How store_reserve and store_prune end (e, probe_error: what filling the new block gave, after the wait that lets the old
// one go): a failure frees the new block and leaves the store untouched; else the store's arrays and table are the new ones.
int adopt_block(nos_voxel_map* vm, hipError_t e, unsigned int probe_error, const char* what, const char* overflow, void* block,
                size_t block_bytes, const nos::VoxelStoreView& view, size_t capacity) {
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
int store_reserve(nos_voxel_map* vm, size_t need) {
  if (need <= vm->capacity) return NOS_OK;
  if (need > (size_t(1) << 30)) return fail(NOS_ERR_UNSUPPORTED, "too many voxels for one store");
  size_t capacity = vm->capacity;
  while (capacity < need) capacity *= 2;
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  void* block = nullptr;
  size_t block_bytes = 0;
  nos::VoxelStoreView nv{};
  hipError_t e = store_alloc(capacity, st, &block, &block_bytes, &nv);
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
  return adopt_block(vm, e, err, "growing the voxel store", "growing the voxel store failed: the new table overflowed", block,
                     block_bytes, nv, capacity);
}

// The back half of an insert and of a merge, ONE copy: U runs (keys ascending and unique, their counts, their nine sums
// about the corner of the key's cell) go into the store — room for them, lookup, rank of the misses, voxel_merge_kernel
// (count += n, acc += seg, the finish, stamp = epoch + 1), the closing wait and the bookkeeping.  Nothing of the store is
// written before the merge kernel; `buf` is the caller's arena, `points` what the runs hold together.  A run that would
// take its voxel past 2^32 − 1 points is flagged by the lookup, the merge kernel then writes nothing, and the closing
// wait brings the flag with the words it reads anyway: the call is rejected with the store as it was (its capacity
// aside), naming `member` (e.g. "point") number names.member_idx[...] of that run.
int store_merge_runs(nos_voxel_map* vm, DeviceBuffers& buf, const uint64_t* run_key, const uint32_t* run_count,
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
  const nos::MapBuildParams prm{5, 0.01, 0.01, (vm->flags & NOS_MAP_PROPER_SQRT_INFORMATION) ? 1 : 0, vm->voxel_resolution};
  const dim3 ugrid(unsigned((size_t(U) + 255) / 256));
  hipLaunchKernelGGL(nos::voxel_lookup_kernel, ugrid, dim3(256), 0, st, vm->view, run_key, run_count, names, U, run_slot, miss,
                     vm->d_info);
  e = hipGetLastError();
  if (e == hipSuccess) e = prim_run(rank_misses, t_rank);
  if (e != hipSuccess) return hip_fail(e, what);  // still nothing written
  hipLaunchKernelGGL(nos::voxel_merge_kernel, ugrid, dim3(256), 0, st, vm->view, run_key, run_count, seg_acc, run_slot, rank, U, prm,
                     uint32_t(vm->epoch + 1), vm->d_info);
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

// One insert.  host_xyz != nullptr: [n][3] in the map frame; otherwise d_planes = 3 planes of n doubles in a local frame,
// warped by `pose` on the device, `order` the scan's original indices when it was sorted by cell (else nullptr).
int store_insert(nos_voxel_map* vm, size_t n, const double* host_xyz, const double* d_planes, const uint32_t* order,
                 const nos::PosePod& pose, size_t* n_touched) {
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
  if (n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points for one insert");
  if (n == 0) {
    if (n_touched) *n_touched = 0;
    return NOS_OK;
  }
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  DeviceBuffers buf(&slot);  // arena: every temporary comes from the slot's buffer pool — no hipMalloc / hipFree per insert
  double *rec = nullptr, *staged = nullptr, *seg_acc = nullptr;
  KeyGroups<uint64_t> g;  // the batch grouped by voxel: a run = the points of one voxel, in point order
  hipError_t e = hipSetDevice(slot.device);
  buf.reserve(n * (7 * sizeof(double) + 3 * sizeof(uint64_t) + 4 * sizeof(uint32_t)) + (size_t(16) << 20));
  if (e == hipSuccess) e = buf.alloc(&rec, n * 4);
  if (e == hipSuccess && host_xyz) e = buf.alloc(&staged, n * 3);
  if (e == hipSuccess) e = g.arrays(buf, st, n);
  if (e == hipSuccess) e = g.temporaries(buf, 63);  // all planning ahead of the first kernel
  // step 1: records, keys, the finite / in-range check
  unsigned int h_info[nos::kInfoWords] = {};
  uint32_t U = 0;
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info, 0, 4 * sizeof(unsigned int), st);  // bad, far, probe error, new
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
  if (e == hipSuccess) e = hipMemcpyAsync(h_info, vm->d_info, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait in the middle: run count and flags
  if (e != hipSuccess) return hip_fail(e, "voxel store insert (sort)");
  // nothing of the store has been written so far: a rejected batch leaves it as it was
  if (h_info[nos::kInfoBadPoint] != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "point %u has a non-finite coordinate", h_info[nos::kInfoBadPoint] - 1u);
  if (h_info[nos::kInfoFarPoint] != 0)
    return fail(NOS_ERR_UNSUPPORTED, "point %u lies outside the addressable grid (+-2^20 cells per axis)",
                h_info[nos::kInfoFarPoint] - 1u);
  // step 3: the build's sums kernel on the batch; step 4 (store_merge_runs): lookup, rank of the misses, merge + finish
  buf.reserve(size_t(U) * (9 * sizeof(double) + 3 * sizeof(uint32_t)) + (size_t(1) << 20));
  e = buf.alloc(&seg_acc, size_t(U) * 9);
  if (e == hipSuccess) e = g.queue_offsets(U);
  if (e != hipSuccess) return hip_fail(e, "voxel store insert (segments)");
  e = launch_voxel_sums(rec, g.idx_sorted, g.offsets, g.counts, U, 1.0 / vm->voxel_resolution, vm->voxel_resolution, seg_acc, st);
  if (e != hipSuccess) return hip_fail(e, "voxel store insert (sums)");
  return store_merge_runs(vm, buf, g.uniq, g.counts, seg_acc, U, n, nos::VoxelRunNames{g.idx_sorted, g.offsets, order}, "point",
                          "voxel store insert", n_touched);
}

// One merge of `src` into `dst` under `pose`: the source's slots become moment records about destination
// cells, grouped by destination cell and added up per cell; the wait in the middle reads the run count and the flags, and
// nothing of the destination is written before it.  The source is only read.
int store_merge(nos_voxel_map* dst, const nos_voxel_map* src, const nos::PosePod& pose, size_t* n_touched) {
  if (dst->broken || src->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
  const size_t n = src->n_voxels;
  if (n == 0) {
    if (n_touched) *n_touched = 0;
    return NOS_OK;
  }
  DeviceSlot& slot = dst->ctx->slots[0];
  hipStream_t st = slot.stream;
  DeviceBuffers buf(&slot);  // arena: every temporary comes from the slot's buffer pool
  double *mom = nullptr, *seg_acc = nullptr;
  uint32_t *mom_count = nullptr, *seg_count = nullptr;
  KeyGroups<uint64_t> g;  // the source's slots grouped by destination cell: a run = the voxels that land in one cell, in slot order
  hipError_t e = hipSetDevice(slot.device);
  buf.reserve(n * (18 * sizeof(double) + 3 * sizeof(uint64_t) + 9 * sizeof(uint32_t)) + (size_t(16) << 20));
  if (e == hipSuccess) e = buf.alloc(&mom, n * 9);
  if (e == hipSuccess) e = buf.alloc(&mom_count, n);
  if (e == hipSuccess) e = buf.alloc(&seg_acc, n * 9);
  if (e == hipSuccess) e = buf.alloc(&seg_count, n);
  if (e == hipSuccess) e = g.arrays(buf, st, n);
  if (e == hipSuccess) e = g.temporaries(buf, 63);  // all planning ahead of the first kernel
  unsigned int h_info[nos::kInfoWords] = {};
  uint32_t U = 0;
  const dim3 grid(unsigned((n + 255) / 256));
  if (e == hipSuccess) e = hipMemsetAsync(dst->d_info, 0, 4 * sizeof(unsigned int), st);  // bad, far, probe error, new
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
  if (e == hipSuccess) e = hipMemcpyAsync(h_info, dst->d_info, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait in the middle: run count and flags
  if (e != hipSuccess) return hip_fail(e, "voxel store merge (sums)");
  // nothing of the destination has been written so far: a rejected merge leaves it as it was
  if (h_info[nos::kInfoBadPoint] != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "source voxel %u has non-finite moments under this pose", h_info[nos::kInfoBadPoint] - 1u);
  if (h_info[nos::kInfoFarPoint] != 0)
    return fail(NOS_ERR_UNSUPPORTED,
                "source voxel %u lands outside the addressable grid (+-2^20 cells per axis), or the source voxels of its "
                "destination cell hold more than 2^32 - 1 points together", h_info[nos::kInfoFarPoint] - 1u);
  return store_merge_runs(dst, buf, g.uniq, seg_count, seg_acc, U, src->n_points, nos::VoxelRunNames{g.idx_sorted, g.offsets, nullptr},
                          "source voxel", "voxel store merge", n_touched);
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
    hipError_t e = store_alloc(capacity, st, &block, &block_bytes, &nv);
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
    const char* what = "voxel store prune (compact)";
    if (e == hipSuccess && err == 0) {
      // the device-side valid counter follows (in stream order before any later merge)
      e = hipMemcpyAsync(vm->d_info + nos::kInfoValid, vm->d_info + nos::kInfoKeptValid, sizeof(unsigned int),
                         hipMemcpyDeviceToDevice, st);
      what = "voxel store prune (counter)";
    }
    const int rc = adopt_block(vm, e, err, what, "voxel store prune failed: the new table overflowed", block, block_bytes, nv, capacity);
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
int keep_rule(const nos_voxel_map* vm, const nos_voxel_prune* what, nos::VoxelKeepRule* rule) {
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
int store_prune(nos_voxel_map* vm, const nos::VoxelKeepRule& rule, size_t* n_removed) {
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
int store_carve(nos_voxel_map* vm, const nos_scan* scan, const nos::PosePod& pose, const nos::VoxelCarveParams& prm,
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

// An empty scan in nos_scan_create's form of one.
int empty_scan(nos_ctx* ctx, nos_scan** out) {
  std::unique_ptr<nos_scan> s(new (std::nothrow) nos_scan());
  if (!s) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  s->ctx = ctx;
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&s->d_planes), 3 * sizeof(double));
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return hip_fail(e, "voxel store ray cast (empty scan)");
  }
  *out = s.release();
  return NOS_OK;
}

// One ray cast: every point of `rays` under `pose` is a beam walked through the grid until the first
// voxel it hits.  The store is only read — its info block too: the three counters are the cast's own, in arena memory.
// Waits: the one that brings the counters, the hit count of the select and the per-ray results; a second one behind the
// gather when the caller wants the hit points and there are any.  The outputs are written once nothing can fail any more.
int store_raycast(nos_voxel_map* vm, const nos_scan* rays, const nos::PosePod& pose, const nos::VoxelRaycastParams& prm,
                  int32_t* voxel_out, double* range_out, nos_scan** out_scan, size_t* n_hit, size_t* n_skipped) {
  const size_t n = rays->n;
  if (n >= 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "too many points for one ray cast");
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  hipError_t e = hipSetDevice(slot.device);
  if (e != hipSuccess) return hip_fail(e, "voxel store ray cast");
  nos_scan* hits_scan = nullptr;
  if (n == 0 || vm->n_voxels == 0) {  // nothing to cast, or nothing to hit
    if (out_scan) {
      const int rc = empty_scan(vm->ctx, &hits_scan);
      if (rc != NOS_OK) return rc;
      *out_scan = hits_scan;
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
  double* out_planes = nullptr;
  uint32_t* out_order = nullptr;
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
      const int rc = empty_scan(vm->ctx, &hits_scan);
      if (rc != NOS_OK) return rc;
    } else if (out_scan) {
      e = hipMalloc(reinterpret_cast<void**>(&out_planes), size_t(n_kept) * 3 * sizeof(double));
      if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&out_order), size_t(n_kept) * sizeof(uint32_t));
      if (e == hipSuccess) {
        hipLaunchKernelGGL(nos::voxel_raycast_gather_kernel, dim3((n_kept + 255) / 256), dim3(256), 0, st, rays->d_planes, uint32_t(n),
                           rays->d_order, kept, n_kept, d_scale, prm.origin[0], prm.origin[1], prm.origin[2], out_planes, out_order);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipStreamSynchronize(st);  // the second wait: the gather has read the arena's arrays
      if (e == hipSuccess) {
        hits_scan = new (std::nothrow) nos_scan();
        if (!hits_scan) e = hipErrorOutOfMemory;
      }
      if (e != hipSuccess) {
        (void)hipGetLastError();  // a failed allocation must not surface as the next call's launch error
        if (out_planes) (void)hipFree(out_planes);
        if (out_order) (void)hipFree(out_order);
        return hip_fail(e, "voxel store ray cast (hit points)");
      }
      hits_scan->ctx = vm->ctx;
      hits_scan->n = n_kept;
      hits_scan->d_planes = out_planes;
      hits_scan->d_order = out_order;
    }
  }
  if (voxel_out) std::memcpy(voxel_out, h_voxel.data(), n * sizeof(int32_t));
  if (range_out) std::memcpy(range_out, h_range.data(), n * sizeof(double));
  if (out_scan) *out_scan = hits_scan;
  if (n_hit) *n_hit = h_cnt[nos::kRaycastHits];
  if (n_skipped) *n_skipped = h_cnt[nos::kRaycastSkipped];
  return NOS_OK;
}

// One export.  rule == nullptr: the first n_voxels entries of key, count, acc and stamp as they are, one
// wait.  Otherwise a prune's keep flags and their scan (KeepPass), the wait that tells how many slots are selected, the
// gather of those slots into arena arrays, the wait for the data.  Nothing of the store is written; `out` is written
// once nothing can fail any more.
int store_export(nos_voxel_map* vm, const nos::VoxelKeepRule* rule, int side, nos_voxel_state* out) {
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

// NOS_IMPORT_RESTORE into a store that holds no voxel: the n voxels as given become slots 0 … n − 1 of
// a FRESH block — keys, counts, sums and stamps copied in, voxel_restore_kernel for the rest — which adopt_block makes
// the store's only when nothing failed, a repeated cell included.  keys: the cells packed, on the host.
int store_restore(nos_voxel_map* vm, size_t n, const std::vector<uint64_t>& keys, const int64_t* cells_xyz, const uint32_t* counts,
                  const double* sums, const uint32_t* stamps, unsigned long long epoch, size_t* n_touched) {
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
  if (e == hipSuccess) e = store_alloc(capacity, st, &block, &block_bytes, &nv);
  if (e != hipSuccess) return hip_fail(e, "voxel store restore (new block)");
  nv.n_voxels = uint32_t(n);
  const nos::MapBuildParams prm{5, 0.01, 0.01, (vm->flags & NOS_MAP_PROPER_SQRT_INFORMATION) ? 1 : 0, vm->voxel_resolution};
  unsigned int h_info[nos::kInfoWords] = {};
  e = hipMemcpyAsync(nv.key, keys.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(nv.count, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(nv.acc, sums, n * 9 * sizeof(double), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && stamps) e = hipMemcpyAsync(nv.stamp, stamps, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info, 0, 3 * sizeof(unsigned int), st);  // bad, far, probe error
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info + nos::kInfoRemoved, 0, 4 * sizeof(unsigned int), st);  // a keep pass's totals
  if (e == hipSuccess) {
    hipLaunchKernelGGL(nos::voxel_restore_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, st, nv, uint32_t(n), stamps ? 1 : 0,
                       uint32_t(epoch), prm, vm->d_info);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(h_info, vm->d_info, nos::kInfoWords * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait; the old block is freed by adopt_block
  if (e == hipSuccess && h_info[nos::kInfoBadPoint] != 0) {
    (void)hipFree(block);
    const int64_t* c = cells_xyz + 3 * size_t(h_info[nos::kInfoBadPoint] - 1u);
    return fail(NOS_ERR_INVALID_ARGUMENT, "cell (%lld, %lld, %lld) comes twice", (long long)c[0], (long long)c[1], (long long)c[2]);
  }
  const char* what = "voxel store restore";
  if (e == hipSuccess && h_info[nos::kInfoProbeError] == 0) {
    // the device-side valid counter follows (in stream order before any later merge)
    e = hipMemcpyAsync(vm->d_info + nos::kInfoValid, vm->d_info + nos::kInfoKeptValid, sizeof(unsigned int), hipMemcpyDeviceToDevice, st);
    what = "voxel store restore (counter)";
  }
  const int rc = adopt_block(vm, e, h_info[nos::kInfoProbeError], what, "voxel store restore failed: the new table overflowed", block,
                             block_bytes, nv, capacity);
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
int store_add(nos_voxel_map* vm, size_t n, const std::vector<uint64_t>& keys, const int64_t* cells_xyz, const uint32_t* counts,
              const double* sums, size_t* n_touched) {
  if (n == 0) {
    if (n_touched) *n_touched = 0;
    return NOS_OK;
  }
  DeviceSlot& slot = vm->ctx->slots[0];
  hipStream_t st = slot.stream;
  DeviceBuffers buf(&slot);  // arena: every temporary comes from the slot's buffer pool
  uint32_t *d_count = nullptr, *run_count = nullptr;
  double *d_acc = nullptr, *run_acc = nullptr;
  KeyGroups<uint64_t> g;  // the state's voxels grouped by cell: every run has ONE member, or the state is rejected
  std::vector<uint32_t> iota(n);
  unsigned long long points = 0;
  for (size_t i = 0; i < n; ++i) iota[i] = uint32_t(i), points += counts[i];
  hipError_t e = hipSetDevice(slot.device);
  buf.reserve(n * (18 * sizeof(double) + 3 * sizeof(uint64_t) + 9 * sizeof(uint32_t)) + (size_t(16) << 20));
  if (e == hipSuccess) e = buf.alloc(&d_count, n);
  if (e == hipSuccess) e = buf.alloc(&run_count, n);
  if (e == hipSuccess) e = buf.alloc(&d_acc, n * 9);
  if (e == hipSuccess) e = buf.alloc(&run_acc, n * 9);
  if (e == hipSuccess) e = g.arrays(buf, st, n);
  if (e == hipSuccess) e = g.temporaries(buf, 63);  // all planning ahead of the first kernel
  unsigned int h_info[nos::kInfoWords] = {};
  uint32_t U = 0;
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info, 0, 4 * sizeof(unsigned int), st);  // bad, far, probe error, new
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
  if (e == hipSuccess) e = hipMemcpyAsync(h_info, vm->d_info, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // the one wait in the middle: the flags
  if (e != hipSuccess) return hip_fail(e, "voxel store add (sort)");
  // nothing of the store has been written so far: a rejected state leaves it as it was
  if (h_info[nos::kInfoBadPoint] != 0) {
    const int64_t* c = cells_xyz + 3 * size_t(h_info[nos::kInfoBadPoint] - 1u);
    return fail(NOS_ERR_INVALID_ARGUMENT, "cell (%lld, %lld, %lld) comes twice", (long long)c[0], (long long)c[1], (long long)c[2]);
  }
  if (h_info[nos::kInfoFarPoint] != 0)
    return fail(NOS_ERR_UNSUPPORTED, "voxel %u of the state takes its destination voxel past 2^32 - 1 points", h_info[nos::kInfoFarPoint] - 1u);
  if (h_info[nos::kInfoProbeError] != 0) return fail(NOS_ERR_HIP, "voxel store add failed: a table probe found no free entry");
  // without a repeated cell the sorted keys ARE the runs' keys (U == n)
  return store_merge_runs(vm, buf, g.keys_sorted, run_count, run_acc, uint32_t(n), points,
                          nos::VoxelRunNames{g.idx_sorted, nullptr, nullptr}, "voxel", "voxel store add", n_touched);
}

// The store as whatever matches against it is handed it: the view the live matcher reads (nothing of it is written), the
// two words of d_info a match may write, the cells the search ball spans per axis.
LiveStore live_store(const nos_voxel_map* vm) {
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
int check_store_match(const nos_voxel_map* vm, const nos_scan* scan, const double* R, const double* t, nos_dataset** out_ds,
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
hipError_t compact_ids(size_t capacity, DeviceSlot& slot, DeviceBuffers& buf, int32_t* ids, size_t n_keys, uint32_t** rows,
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

int voxel_map_register(int dof, nos_voxel_map* vm, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                       const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                       nos_register_report* reports) {
  nosd::CtxGuard guard_(vm ? vm->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!vm) return register_live(dof, nullptr, scans, n_problems, R, t, loss, ropt, options, reports);
  const LiveStore store = live_store(vm);
  return register_live(dof, &store, scans, n_problems, R, t, loss, ropt, options, reports);
}

}  // namespace

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
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&vm->d_info), nos::kInfoWords * sizeof(unsigned int));
  if (e == hipSuccess) e = hipMemsetAsync(vm->d_info, 0, nos::kInfoWords * sizeof(unsigned int), slot.stream);
  if (e == hipSuccess) e = store_alloc(vm->capacity, slot.stream, &vm->d_block, &vm->block_bytes, &vm->view);
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
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(R[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "R has a non-finite entry");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "t has a non-finite entry");
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
  const int rc = keep_rule(vm, what, &rule);
  if (rc != NOS_OK) return rc;
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
  return store_prune(vm, rule, n_removed);
}

int nos_voxel_map_carve(nos_voxel_map* vm, nos_scan* scan, const double R[9], const double t[3], const nos_voxel_carve* what,
                        size_t* n_removed, size_t* n_skipped, uint32_t* crossings_out, uint32_t* hits_out) {
  // the NULL, struct and value checks come before any device (and any handle's content) is touched
  if (!vm || !scan || !R || !t || !what) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  if (what->struct_size < sizeof(nos_voxel_carve)) return fail(NOS_ERR_INVALID_ARGUMENT, "struct_size is smaller than nos_voxel_carve");
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(R[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "R has a non-finite entry");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t[k]) || !std::isfinite(what->origin[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "t or origin has a non-finite entry");
  if (!std::isfinite(what->end_margin) || what->end_margin < 0.0 || !std::isfinite(what->min_range) || what->min_range < 0.0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "end_margin and min_range must be finite and >= 0");
  if (!std::isfinite(what->max_range) || !(what->max_range > 0.0)) return fail(NOS_ERR_INVALID_ARGUMENT, "max_range must be finite and > 0");
  if (what->min_crossings == 0 || what->min_hits == 0) return fail(NOS_ERR_INVALID_ARGUMENT, "min_crossings and min_hits must be >= 1");
  if (vm->ctx != scan->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map and scan belong to different contexts");
  nosd::CtxGuard guard_(vm->ctx);  // one solve / accumulate / create at a time per context
  if (vm->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "carving a voxel store needs a single-device context");
  // a ray's trip count: at most ceil(max_range / res) + 1 steps per axis
  if (3.0 * (std::ceil(what->max_range / vm->voxel_resolution) + 1.0) > double(NOS_CARVE_MAX_CELLS))
    return fail(NOS_ERR_UNSUPPORTED, "max_range spans more than NOS_CARVE_MAX_CELLS cells: 3 (ceil(max_range / resolution) + 1) > %d",
                NOS_CARVE_MAX_CELLS);
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
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
  for (int k = 0; k < 9; ++k)
    if (!std::isfinite(R[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "R has a non-finite entry");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t[k]) || !std::isfinite(what->origin[k])) return fail(NOS_ERR_INVALID_ARGUMENT, "t or origin has a non-finite entry");
  if (!std::isfinite(what->max_range) || !(what->max_range > 0.0)) return fail(NOS_ERR_INVALID_ARGUMENT, "max_range must be finite and > 0");
  if (!std::isfinite(what->min_range) || what->min_range < 0.0 || !std::isfinite(what->max_mahalanobis_sq) || what->max_mahalanobis_sq < 0.0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "min_range and max_mahalanobis_sq must be finite and >= 0");
  if (vm->ctx != rays->ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "voxel map and scan belong to different contexts");
  nosd::CtxGuard guard_(vm->ctx);  // one solve / accumulate / create at a time per context
  if (vm->ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "ray casting a voxel store needs a single-device context");
  // a ray's trip count: at most ceil(max_range / res) + 1 steps per axis
  if (3.0 * (std::ceil(what->max_range / vm->voxel_resolution) + 1.0) > double(NOS_CARVE_MAX_CELLS))
    return fail(NOS_ERR_UNSUPPORTED, "max_range spans more than NOS_CARVE_MAX_CELLS cells: 3 (ceil(max_range / resolution) + 1) > %d",
                NOS_CARVE_MAX_CELLS);
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
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
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
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
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
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
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
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
  if (vm->broken) return fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure");
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
