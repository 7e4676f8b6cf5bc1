// voxelmerge_kernels.hpp — the front half of merging one voxel store into another under a pose: where
// an insert turns POINTS into per-voxel sums (voxel_points_kernel, sort, voxel_sums_kernel), a merge turns the source's
// VOXELS into them.
//
// One merge = voxel_moments_kernel (every source slot → its destination key and its nine sums about the destination
// cell's corner, voxel_moments.hpp) → stable radix sort of (packed key, source slot) → run-length encode → exclusive scan
// → voxel_moment_sums_kernel (the records of one destination cell added up) → the back half of an insert as it is:
// voxel_lookup_kernel, rank of the misses, voxel_merge_kernel (voxelmap_kernels.hpp).
//
// One lane owns one source slot, then one run: no floating-point atomics, and no order that depends on arrival — a run's
// members are in ascending source slot after the stable sort, and they are added left to right.  Only the source's key,
// count and acc arrays are read; nothing of either store is written here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_moments.hpp"
#include "voxelmap_kernels.hpp"

namespace nos {

// Step 1.  One lane per source slot v in use: mom[v][9] = the slot's sums moved by `pose` into the destination grid,
// mom_count[v] = its count, keys[v] = the packed destination cell, idx[v] = v.  A non-finite result or a destination cell
// outside +-2^20 raises kInfoBadPoint / kInfoFarPoint with v + 1 (voxel_points_kernel's words and convention) and leaves
// key 0; the host reads the flags before anything is merged.
__global__ __launch_bounds__(256) void voxel_moments_kernel(VoxelStoreView src, double res_src, PosePod pose, double res_dst,
                                                            double inv_res_dst, double* __restrict__ mom /* [n_voxels][9] */,
                                                            uint32_t* __restrict__ mom_count, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ idx, unsigned int* __restrict__ info) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= src.n_voxels) return;
  int32_t c[3];
  unpack_cell(src.key[v], c);
  const int64_t cell[3] = {c[0], c[1], c[2]};
  double acc[9], out[9], cf[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = src.acc[9 * size_t(v) + k];
  const uint32_t count = src.count[v];
  voxel_moments(count, acc, cell, res_src, pose.R, pose.t, res_dst, inv_res_dst, cf, out);
  const double lim = double(1 << 20);
  bool finite = true, inside = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) finite = finite && fabs(out[k]) <= 1.79e308;  // a NaN fails the test
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    finite = finite && (cf[k] >= -9.0e18 && cf[k] <= 9.0e18);
    inside = inside && (cf[k] >= -lim && cf[k] < lim);
  }
  const uint32_t tag = v + 1u;
  if (!finite) atomicMax(&info[kInfoBadPoint], tag);
  else if (!inside) atomicMax(&info[kInfoFarPoint], tag);
#pragma unroll
  for (int k = 0; k < 9; ++k) mom[9 * size_t(v) + k] = out[k];
  mom_count[v] = count;
  keys[v] = (finite && inside) ? pack_cell(int64_t(cf[0]), int64_t(cf[1]), int64_t(cf[2])) : 0ull;
  idx[v] = v;
}

// Step 3.  One lane per run u of the sorted keys (*n_runs of them, known on the device only: the launch covers the most
// there can be): seg_acc[u][9] and seg_count[u], the operands of voxel_merge_kernel, = the run's records and counts added
// in ascending source slot, left to right, with plain adds; a run of one member is copied as it is.  The count is summed
// in 64 bits: a total above 2^32 − 1 raises kInfoFarPoint with 1 + the source slot that crossed it.  Only the SOURCE
// voxels of one cell are added here; what the destination voxel already holds is added to the run's count by
// voxel_lookup_kernel, which raises the same word when run + destination pass 2^32 − 1.
__global__ __launch_bounds__(256) void voxel_moment_sums_kernel(const double* __restrict__ mom /* [n][9] */,
                                                                const uint32_t* __restrict__ mom_count,
                                                                const uint32_t* __restrict__ sorted_idx,
                                                                const uint32_t* __restrict__ run_offset,
                                                                const uint32_t* __restrict__ run_length,
                                                                const uint32_t* __restrict__ n_runs,
                                                                double* __restrict__ seg_acc /* [n_runs][9] */,
                                                                uint32_t* __restrict__ seg_count,
                                                                unsigned int* __restrict__ info) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= *n_runs) return;
  const uint32_t begin = run_offset[u], len = run_length[u];
  uint32_t i = sorted_idx[begin];
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = mom[9 * size_t(i) + k];
  unsigned long long total = mom_count[i];
  for (uint32_t m = 1; m < len; ++m) {
    i = sorted_idx[begin + m];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = acc[k] + mom[9 * size_t(i) + k];
    const unsigned long long before = total;
    total += mom_count[i];
    if (before <= 0xFFFFFFFFull && total > 0xFFFFFFFFull) atomicMax(&info[kInfoFarPoint], i + 1u);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) seg_acc[9 * size_t(u) + k] = acc[k];
  seg_count[u] = uint32_t(total);
}

}  // namespace nos
