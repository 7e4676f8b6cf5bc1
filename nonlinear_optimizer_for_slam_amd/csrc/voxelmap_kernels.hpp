// voxelmap_kernels.hpp — incremental NDT voxel store on the GPU: a map that grows scan by scan.
//
// Restates UpdateNdtMap of the reference's test harness AS AN UPDATE
// (nonlinear_optimizer/mahalanobis_distance_minimizer/tests/simple_optimization_test.cc:236-281): a batch of points is
// added to the count / sum / moment of the voxels it falls into, in a map that already exists (:240-252), and mean,
// covariance, eigen-decomposition and sqrt-information are re-derived for the touched voxels only
// (`updated_voxel_key_set`, :254-280).  mapbuild_kernels.hpp is the one-shot form of the same function.
//
// One insert = keys and 32-byte point records (voxel_points_kernel) → stable radix sort of (packed key, index) →
// run-length encode → voxel_sums_kernel as the build runs it (nine per-segment sums, fixed order) →
// voxel_lookup_kernel (which touched voxels does the store hold?) → exclusive scan of the misses →
// voxel_merge_kernel (new slots, table inserts, count += n, acc += seg, the per-voxel finish).
//
// Keys are unique after the run-length encode, so one lane owns one voxel: no two lanes update the same slot and there
// are no floating-point atomics anywhere.  Every hand-off between the steps is a kernel boundary on one stream: the table
// is only READ by the lookup and only WRITTEN by the merge, and a merge lane reads nothing another merge lane writes.
//
// Slot numbers (= voxel ids, the matcher's tie-break) are a function of the sequence of batches alone: batch of first
// appearance, then ascending cell — a missing voxel gets V_old + (its rank among the batch's misses in sorted-key order),
// never a counter bumped with atomicAdd.
//
// One prune = voxel_keep_kernel (a 0/1 flag per slot by box and / or age, and the totals of what goes) → exclusive scan
// of the flags → voxel_compact_kernel (every kept slot moves to its rank among the kept ones in a FRESH block and enters
// that block's empty table).  Out of place, because a parallel in-place stable compaction races: a lane's destination is
// another lane's unread source.  A carve (voxelcarve_kernels.hpp) writes its own keep flags and shares everything behind them.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hpp"
#include "voxel_finish.hpp"

namespace nos {

constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// words of the store's device-side info block
enum VoxelInfoWord {
  kInfoBadPoint = 0,    // 1 + index of a point with a non-finite coordinate (atomicMax; 0 = none)
  kInfoFarPoint = 1,    // 1 + index of a point whose cell lies outside +-2^20 (atomicMax; 0 = none); behind the wait that
                        // reads that, 1 + a member of a run that takes its voxel past 2^32 - 1 points (voxel_lookup_kernel)
  kInfoProbeError = 2,  // a probe loop ran through the whole table (cannot happen at load factor <= 1/2)
  kInfoNew = 3,         // voxels the last merge created
  kInfoValid = 4,       // valid voxels in the store (kept across inserts; int)
  kInfoRemoved = 5,     // voxels the last keep pass marked for removal
  kInfoRemovedPoints = 6,  // their points: one 64-bit counter in words 6 and 7
  kInfoKeptValid = 8,   // valid voxels among those the last keep pass kept
  kInfoSkipped = 9,     // rays the last carve skipped (voxelcarve_kernels.hpp); a carve also raises bit 1 of
                        // kInfoProbeError when a ray's trip count ran past its bound
  kInfoMatches = 10,    // real matches of the last nos_voxel_map_match(_indexed): one 64-bit counter in words 10 and 11.  That call
                        // writes these two words and clears kInfoProbeError before its launch; "the store is not modified"
                        // holds for the info block by convention only: no call reads words 10-11, and every call that
                        // reads kInfoProbeError (insert, growth, prune) clears it itself before the kernels that raise it
  kInfoWords = 12
};

// The store as the kernels see it.  Arrays have room for `capacity` slots, the first n_voxels are in use; the table has
// table_mask + 1 >= 2 * capacity entries (a power of two), kEmptyCell = free.
struct VoxelStoreView {
  uint64_t* key;          // [capacity] packed cell key (pack_cell)
  uint32_t* count;        // [capacity]
  double* acc;            // [capacity][9] sx sy sz | mxx mxy mxz myy myz mzz about the cell corner (voxel_sums_kernel's)
  double* mean;           // [capacity][3]
  double* sqrt_info;      // [capacity][9]
  unsigned char* valid;   // [capacity]
  uint32_t* stamp;        // [capacity] the store's insert counter (low 32 bits) at the last insert that touched the slot
  unsigned long long* table_key;  // [table_mask + 1]
  uint32_t* table_slot;           // [table_mask + 1]
  uint32_t table_mask;
  uint32_t n_voxels;
};

// Step 1.  Point i of a batch → its 32-byte record {x, y, z, 0} (what voxel_sums_kernel gathers), its packed key and its
// index; a non-finite coordinate or a cell outside the addressable grid raises a flag instead (the host reads the flags
// before anything is merged).  WARP = false: points as the caller's [n][3] array, already in the map frame.  WARP = true:
// three planes in the scan's local frame, warped by the pose with the operation order of the matcher (match_point,
// match_kernels.hpp) — the point lands in the map exactly where the matcher saw it.
template <bool WARP>
__global__ __launch_bounds__(256) void voxel_points_kernel(const double* __restrict__ src, uint64_t n, PosePod pose,
                                                           double inv_res, double* __restrict__ rec /* [n][4] */,
                                                           uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                           unsigned int* __restrict__ info) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  double qx, qy, qz;
  if (WARP) {
    const double x = src[i], y = src[n + i], z = src[2 * n + i];
    qx = __builtin_fma(pose.R[2], z, __builtin_fma(pose.R[0], x, pose.R[1] * y)) + pose.t[0];
    qy = __builtin_fma(pose.R[5], z, __builtin_fma(pose.R[3], x, pose.R[4] * y)) + pose.t[1];
    qz = __builtin_fma(pose.R[8], z, __builtin_fma(pose.R[6], x, pose.R[7] * y)) + pose.t[2];
  } else {
    qx = src[3 * i], qy = src[3 * i + 1], qz = src[3 * i + 2];
  }
  using V2 = double __attribute__((ext_vector_type(2)));
  V2* out = reinterpret_cast<V2*>(rec) + 2 * i;
  out[0] = V2{qx, qy};
  out[1] = V2{qz, 0.0};
  const double c[3] = {floor(qx * inv_res), floor(qy * inv_res), floor(qz * inv_res)};
  const double lim = double(1 << 20);
  bool finite = true, inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    finite = finite && (c[k] >= -9.0e18 && c[k] <= 9.0e18);  // a NaN fails both tests
    inside = inside && (c[k] >= -lim && c[k] < lim);
  }
  const uint32_t tag = uint32_t(i) + 1u;
  // qx * inv_res can overflow for a finite qx: the point itself decides "non-finite"
  const bool bad = !(fabs(qx) <= 1.79e308 && fabs(qy) <= 1.79e308 && fabs(qz) <= 1.79e308);
  if (bad) atomicMax(&info[kInfoBadPoint], tag);
  else if (!finite || !inside) atomicMax(&info[kInfoFarPoint], tag);
  keys[i] = (finite && inside) ? pack_cell(int64_t(c[0]), int64_t(c[1]), int64_t(c[2])) : 0ull;
  idx[i] = uint32_t(i);
}

// The slot that holds `key`, or kNoSlot.  Bounded by the table size; *error is raised instead of spinning.
__device__ __forceinline__ uint32_t voxel_table_find(const VoxelStoreView& s, uint64_t key, unsigned int* error) {
  uint32_t h = hash_cell(key) & s.table_mask;
  for (uint32_t probe = 0; probe <= s.table_mask; ++probe) {
    const unsigned long long k = s.table_key[h];
    if (k == key) return s.table_slot[h];
    if (k == kEmptyCell) return kNoSlot;
    h = (h + 1) & s.table_mask;
  }
  atomicOr(error, 1u);
  return kNoSlot;
}

// Claims a free entry for `key` (which no other lane inserts and the table does not hold) and points it at `slot`.
__device__ __forceinline__ void voxel_table_insert(const VoxelStoreView& s, uint64_t key, uint32_t slot, unsigned int* error) {
  uint32_t h = hash_cell(key) & s.table_mask;
  for (uint32_t probe = 0; probe <= s.table_mask; ++probe) {
    if (atomicCAS(&s.table_key[h], (unsigned long long)kEmptyCell, (unsigned long long)key) == kEmptyCell) {
      s.table_slot[h] = slot;  // read by later launches only
      return;
    }
    h = (h + 1) & s.table_mask;
  }
  atomicOr(error, 1u);
}

// Who a run is named by when it would take its voxel past 2^32 − 1 points: member_idx[first[u]] (first == nullptr: run u
// has one member, at position u) is a member of run u — a point of the batch, a voxel of the source or of the state —
// and `order`, when not nullptr, maps it to the caller's numbering (a cell-sorted scan's original indices).
struct VoxelRunNames {
  const uint32_t* member_idx;
  const uint32_t* first;
  const uint32_t* order;
};

// Step 4a.  One lane per touched voxel u (run u of the sorted batch): the store's slot for its key, or kNoSlot and
// miss[u] = 1.  A run that would take the voxel it found past 2^32 − 1 points raises kInfoFarPoint with 1 + the name of
// one of its members (atomicMax; the host has read and found the word 0 before this launch).  The table is read-only here.
__global__ __launch_bounds__(256) void voxel_lookup_kernel(VoxelStoreView s, const uint64_t* __restrict__ run_key,
                                                           const uint32_t* __restrict__ run_count, VoxelRunNames names,
                                                           uint32_t n_runs, uint32_t* __restrict__ run_slot,
                                                           uint32_t* __restrict__ miss, unsigned int* __restrict__ info) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= n_runs) return;
  const uint32_t slot = voxel_table_find(s, run_key[u], &info[kInfoProbeError]);
  run_slot[u] = slot;
  miss[u] = slot == kNoSlot ? 1u : 0u;
  if (slot != kNoSlot && (unsigned long long)s.count[slot] + run_count[u] > 0xFFFFFFFFull) {
    uint32_t who = names.member_idx[names.first ? names.first[u] : u];
    if (names.order) who = names.order[who];
    atomicMax(&info[kInfoFarPoint], who + 1u);
  }
}

// Step 4b.  One lane per touched voxel: a miss takes slot n_voxels + rank (rank = exclusive scan of `miss`, i.e. its
// place among the batch's new voxels in ascending cell order) and enters the table; then count += n and
// acc[k] = acc[k] + seg[k] with plain loads and stores (a new voxel's sums ARE the segment's: the bits of a one-shot
// build), the finish for this slot only, and stamp = this insert's number.  Store and segment both hold their sums about the
// corner of the slot's cell (voxel_finish.hpp), a function of the key alone, so they add as they are; the finish gets the
// cell from unpack_cell of the key.  The valid-voxel counter moves by an integer atomic per wave.
__global__ __launch_bounds__(256) void voxel_merge_kernel(VoxelStoreView s, const uint64_t* __restrict__ run_key,
                                                          const uint32_t* __restrict__ run_count,
                                                          const double* __restrict__ seg_acc /* [n_runs][9] */,
                                                          const uint32_t* __restrict__ run_slot,
                                                          const uint32_t* __restrict__ rank, uint32_t n_runs,
                                                          MapBuildParams prm, uint32_t epoch,
                                                          unsigned int* __restrict__ info) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  // the lookup found a run that takes its voxel past 2^32 − 1 points: the whole call is rejected, nothing is written.
  // The word is final here (the lookup is an earlier launch on this stream) and no lane of this kernel writes it.
  if (info[kInfoFarPoint] != 0) return;
  int delta = 0;
  if (u < n_runs) {
    const uint64_t key = run_key[u];
    uint32_t slot = run_slot[u];
    const bool fresh = slot == kNoSlot;
    uint32_t count = run_count[u];
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = seg_acc[9 * size_t(u) + k];
    unsigned char was_valid = 0;
    if (fresh) {
      slot = s.n_voxels + rank[u];
      voxel_table_insert(s, key, slot, &info[kInfoProbeError]);
      s.key[slot] = key;
      if (u == n_runs - 1) info[kInfoNew] = rank[u] + 1u;
    } else {
      count += s.count[slot];
#pragma unroll
      for (int k = 0; k < 9; ++k) acc[k] = s.acc[9 * size_t(slot) + k] + acc[k];
      was_valid = s.valid[slot];
      if (u == n_runs - 1) info[kInfoNew] = rank[u];
    }
    s.count[slot] = count;
#pragma unroll
    for (int k = 0; k < 9; ++k) s.acc[9 * size_t(slot) + k] = acc[k];
    int32_t c[3];
    unpack_cell(key, c);
    const int64_t cell[3] = {c[0], c[1], c[2]};
    double S[9], mean[3];
    const unsigned char ok = voxel_finish(acc, count, cell, prm, mean, S);
    for (int k = 0; k < 3; ++k) s.mean[3 * size_t(slot) + k] = mean[k];
    for (int k = 0; k < 9; ++k) s.sqrt_info[9 * size_t(slot) + k] = S[k];
    s.valid[slot] = ok;
    s.stamp[slot] = epoch;
    delta = int(ok) - int(was_valid);
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) delta += __shfl_xor(delta, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && delta != 0) atomicAdd(reinterpret_cast<int*>(&info[kInfoValid]), delta);
}

// Growth: every slot of the store enters the (new, empty, twice as large) table again.
__global__ __launch_bounds__(256) void voxel_rehash_kernel(VoxelStoreView s, unsigned int* __restrict__ info) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= s.n_voxels) return;
  voxel_table_insert(s, s.key[v], v, &info[kInfoProbeError]);
}

// What a prune keeps.  Box: cell c is kept iff lo[k] <= c[k] <= hi[k] on every axis (bounds computed on the host in
// double, see nos_voxel_map_prune).  Age: kept iff epoch - stamp <= max_age, in 32-bit wrap-around arithmetic.
struct VoxelKeepRule {
  int32_t lo[3], hi[3];
  uint32_t epoch, max_age;
  int use_box, use_age;
};

// What every keep kernel ends with (every lane of the block calls it): the totals of what goes — voxels removed, their
// points, valid voxels kept — summed over the wave and added by one integer atomic per wave each.
__device__ __forceinline__ void voxel_keep_totals(unsigned int removed, unsigned long long removed_points, unsigned int kept_valid,
                                                  unsigned int* __restrict__ info) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    removed += __shfl_xor(removed, o, kWave);
    kept_valid += __shfl_xor(kept_valid, o, kWave);
    removed_points += __shfl_xor(removed_points, o, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (removed != 0) {
      atomicAdd(&info[kInfoRemoved], removed);
      atomicAdd(reinterpret_cast<unsigned long long*>(&info[kInfoRemovedPoints]), removed_points);
    }
    if (kept_valid != 0) atomicAdd(&info[kInfoKeptValid], kept_valid);
  }
}

// Prune, step 1.  One lane per slot in use: keep[v] = 1 iff the voxel passes every test the rule asks for.  The totals
// (voxels removed, their points, valid voxels kept) move by one integer atomic per wave each.  Nothing of the store is written.
__global__ __launch_bounds__(256) void voxel_keep_kernel(VoxelStoreView s, VoxelKeepRule rule, uint32_t* __restrict__ keep,
                                                         unsigned int* __restrict__ info) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  unsigned int removed = 0, kept_valid = 0;
  unsigned long long removed_points = 0;
  if (v < s.n_voxels) {
    bool ok = true;
    if (rule.use_box) {
      int32_t c[3];
      unpack_cell(s.key[v], c);
#pragma unroll
      for (int k = 0; k < 3; ++k) ok = ok && c[k] >= rule.lo[k] && c[k] <= rule.hi[k];
    }
    if (rule.use_age) ok = ok && uint32_t(rule.epoch - s.stamp[v]) <= rule.max_age;
    keep[v] = ok ? 1u : 0u;
    if (ok) {
      kept_valid = s.valid[v] ? 1u : 0u;
    } else {
      removed = 1u;
      removed_points = s.count[v];
    }
  }
  voxel_keep_totals(removed, removed_points, kept_valid, info);
}

// Prune, step 2.  One lane per slot of the old block: a kept slot moves, with everything it holds, to
// new_slot[v] (= its rank among the kept slots, so the order of the survivors is theirs) in the new block `d`, and its
// key enters d's table, which starts empty.  Keys are unique, so the CAS insert of the merge is all it takes.
__global__ __launch_bounds__(256) void voxel_compact_kernel(VoxelStoreView s, VoxelStoreView d,
                                                            const uint32_t* __restrict__ keep,
                                                            const uint32_t* __restrict__ new_slot,
                                                            unsigned int* __restrict__ info) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= s.n_voxels || keep[v] == 0) return;
  const uint32_t w = new_slot[v];
  const uint64_t key = s.key[v];
  d.key[w] = key;
  d.count[w] = s.count[v];
#pragma unroll
  for (int k = 0; k < 9; ++k) d.acc[9 * size_t(w) + k] = s.acc[9 * size_t(v) + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) d.mean[3 * size_t(w) + k] = s.mean[3 * size_t(v) + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) d.sqrt_info[9 * size_t(w) + k] = s.sqrt_info[9 * size_t(v) + k];
  d.valid[w] = s.valid[v];
  d.stamp[w] = s.stamp[v];
  voxel_table_insert(d, key, w, &info[kInfoProbeError]);
}

}  // namespace nos
