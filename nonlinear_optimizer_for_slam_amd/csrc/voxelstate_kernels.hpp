// voxelstate_kernels.hpp — a voxel store's STATE leaves the device and comes back: a voxel is its cell,
// count, nine sums about the cell corner and stamp; mean, sqrt-information and validity are voxel_finish of those, so
// nothing else is ever carried.
//
// Export of a selection = voxel_keep_kernel and the scan of a prune (voxelmap_kernels.hpp) → voxel_state_gather_kernel
// (the selected slots, in slot order, into contiguous arrays).  The flags are a prune's; `want` says which half of the
// partition goes out, and a slot's place follows from the ONE scan: its rank among the kept slots, or its slot minus that.
//
// Restore = the caller's arrays copied into a FRESH block → voxel_restore_kernel (stamp, finish, table insert, totals);
// the block becomes the store's only when nothing failed.
//
// Add = the state's keys grouped by cell (group_host.hpp) → voxel_state_runs_kernel (counts and sums in sorted order, a
// repeated cell and a count past 2^32 − 1 flagged; the store is only read) → the back half of an insert as it is.
//
// One lane per voxel everywhere, plain loads and stores, no floating-point arithmetic but the finish.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxelmap_kernels.hpp"

namespace nos {

// Export.  One lane per slot v in use with keep[v] == want: everything that makes up the voxel goes to position
// kept_rank[v] (want = 1: the kept slots) or v - kept_rank[v] (want = 0: the others) of the output arrays — the slot's
// rank among the selected ones, so they come out in slot order.  Nothing of the store is written.
__global__ __launch_bounds__(256) void voxel_state_gather_kernel(VoxelStoreView s, const uint32_t* __restrict__ keep,
                                                                 const uint32_t* __restrict__ kept_rank, uint32_t want,
                                                                 uint64_t* __restrict__ key_out, uint32_t* __restrict__ count_out,
                                                                 double* __restrict__ acc_out /* [m][9] */,
                                                                 uint32_t* __restrict__ stamp_out) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= s.n_voxels || keep[v] != want) return;
  const uint32_t w = want ? kept_rank[v] : v - kept_rank[v];
  key_out[w] = s.key[v];
  count_out[w] = s.count[v];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc_out[9 * size_t(w) + k] = s.acc[9 * size_t(v) + k];
  stamp_out[w] = s.stamp[v];
}

// voxel_table_insert for keys nobody vouches for: an entry that already holds `key` means the key came twice.
// → false for such a key (nothing is written for it).
__device__ __forceinline__ bool voxel_table_insert_unique(const VoxelStoreView& s, uint64_t key, uint32_t slot, unsigned int* error) {
  uint32_t h = hash_cell(key) & s.table_mask;
  for (uint32_t probe = 0; probe <= s.table_mask; ++probe) {
    const unsigned long long seen = atomicCAS(&s.table_key[h], (unsigned long long)kEmptyCell, (unsigned long long)key);
    if (seen == kEmptyCell) {
      s.table_slot[h] = slot;  // read by later launches only
      return true;
    }
    if (seen == key) return false;
    h = (h + 1) & s.table_mask;
  }
  atomicOr(error, 1u);
  return true;
}

// Restore.  `d` is a fresh block (empty table) whose key, count and acc arrays — and stamp, when has_stamps — hold the
// caller's n voxels as they were given.  One lane per voxel: the stamp when there is none, the finish from (acc, count,
// cell of the key), the table insert.  A key that is already in the table raises kInfoBadPoint with 1 + the voxel
// (atomicMax, voxel_points_kernel's convention).  Totals, one integer atomic per wave each, in the words a keep pass uses
// for the block IT fills: valid voxels in kInfoKeptValid, points in the 64-bit counter of words 6 and 7.
__global__ __launch_bounds__(256) void voxel_restore_kernel(VoxelStoreView d, uint32_t n, int has_stamps, uint32_t stamp,
                                                            MapBuildParams prm, unsigned int* __restrict__ info) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  unsigned int valid = 0;
  unsigned long long points = 0;
  if (v < n) {
    const uint64_t key = d.key[v];
    const uint32_t count = d.count[v];
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = d.acc[9 * size_t(v) + k];
    int32_t c[3];
    unpack_cell(key, c);
    const int64_t cell[3] = {c[0], c[1], c[2]};
    double S[9], mean[3];
    const unsigned char ok = voxel_finish(acc, count, cell, prm, mean, S);
    for (int k = 0; k < 3; ++k) d.mean[3 * size_t(v) + k] = mean[k];
    for (int k = 0; k < 9; ++k) d.sqrt_info[9 * size_t(v) + k] = S[k];
    d.valid[v] = ok;
    if (!has_stamps) d.stamp[v] = stamp;
    if (!voxel_table_insert_unique(d, key, v, &info[kInfoProbeError])) atomicMax(&info[kInfoBadPoint], v + 1u);
    valid = ok ? 1u : 0u;
    points = count;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    valid += __shfl_xor(valid, o, kWave);
    points += __shfl_xor(points, o, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (valid != 0) atomicAdd(&info[kInfoKeptValid], valid);
    if (points != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&info[kInfoRemovedPoints]), points);
  }
}

// Add.  One lane per position i of the state's keys in sorted order (sorted_idx[i] = the voxel of the state at that
// position): run_count[i] and run_acc[i][9], the operands of voxel_merge_kernel, are that voxel's count and sums as they
// are.  A key equal to its left neighbour raises kInfoBadPoint, a count that would take the store's voxel past 2^32 − 1
// points kInfoFarPoint, both with 1 + the voxel of the state (atomicMax); the host reads the flags before anything is
// merged.  The store is only read.
__global__ __launch_bounds__(256) void voxel_state_runs_kernel(VoxelStoreView s, const uint64_t* __restrict__ sorted_key,
                                                               const uint32_t* __restrict__ sorted_idx, uint32_t n,
                                                               const uint32_t* __restrict__ count /* [n] as given */,
                                                               const double* __restrict__ acc /* [n][9] as given */,
                                                               uint32_t* __restrict__ run_count,
                                                               double* __restrict__ run_acc /* [n][9] */,
                                                               unsigned int* __restrict__ info) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = sorted_idx[i];
  const uint64_t key = sorted_key[i];
  const uint32_t c = count[j];
  run_count[i] = c;
#pragma unroll
  for (int k = 0; k < 9; ++k) run_acc[9 * size_t(i) + k] = acc[9 * size_t(j) + k];
  if (i > 0 && sorted_key[i - 1] == key) atomicMax(&info[kInfoBadPoint], j + 1u);
  const uint32_t slot = voxel_table_find(s, key, &info[kInfoProbeError]);
  if (slot != kNoSlot && (unsigned long long)s.count[slot] + c > 0xFFFFFFFFull) atomicMax(&info[kInfoFarPoint], j + 1u);
}

}  // namespace nos
