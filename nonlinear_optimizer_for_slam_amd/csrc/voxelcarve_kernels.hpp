// voxelcarve_kernels.hpp — line-of-sight carving of the voxel store: the third prune rule.
//
// A ray that ends beyond a voxel has passed through it, so that voxel is free space.  One carve =
// voxel_carve_walk_kernel (one lane per scan point: the ray from the sensor origin to the point is walked cell by cell
// through the grid; every visited cell the store holds gets crossings[slot] += 1, the cell of the endpoint hits[slot] += 1)
// → voxel_carve_keep_kernel (keep[v] = 0 iff crossings[v] >= min_crossings and hits[v] < min_hits, and a prune's totals)
// → the tail of a prune as it is (exclusive scan of the flags, out-of-place stable compaction).
//
// The counters are integers and the adds are integer atomics, so the counts do not depend on the order in which the lanes
// arrive: the determinism argument of the scan filter's atomicMin.  The table is only READ by the walk; the counters are
// read by the keep kernel in a later launch.  Kernel boundaries on one stream are the only hand-offs.
//
// The walk is stated operation by operation in include/nos.h (nos_voxel_map_carve) and restated in numpy by
// tests/voxel_carve_inputs.py.  Where the contract names an unfused operation the code below stands under
// `fp contract(off)`: hipcc would otherwise fuse a * b + c.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxelmap_kernels.hpp"

namespace nos {

// What the walk is handed.  origin is in the SCAN's frame; res / inv_res are the pair an insert uses.
struct VoxelCarveParams {
  double origin[3];
  double end_margin, min_range, max_range;
  double res, inv_res;
  uint32_t max_cells;  // NOS_CARVE_MAX_CELLS: the bound on a ray's trip count
};

// p → R p + t with the multiply-adds of voxel_points_kernel<true> (the matcher's warp, match_point).
__device__ __forceinline__ void carve_warp(const PosePod& pose, double x, double y, double z, double q[3]) {
  q[0] = __builtin_fma(pose.R[2], z, __builtin_fma(pose.R[0], x, pose.R[1] * y)) + pose.t[0];
  q[1] = __builtin_fma(pose.R[5], z, __builtin_fma(pose.R[3], x, pose.R[4] * y)) + pose.t[1];
  q[2] = __builtin_fma(pose.R[8], z, __builtin_fma(pose.R[6], x, pose.R[7] * y)) + pose.t[2];
}

// floor(v * inv_res) per axis → c; false when a cell lies outside the addressable +-2^20 (a NaN fails both tests).
__device__ __forceinline__ bool carve_cell(const double v[3], double inv_res, int32_t c[3]) {
  const double lim = double(1 << 20);
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = floor(v[k] * inv_res);
    inside = inside && (f >= -lim && f < lim);
    c[k] = inside ? int32_t(f) : 0;
  }
  return inside;
}

// Parameter of the j-th face an axis crosses (j >= 1), from j and never accumulated: the face lies at g = (ca + j) res
// going up, (ca - j + 1) res going down; tau = (g - a) / den with den = b - a formed once per axis.
__device__ __forceinline__ double carve_tau(int32_t ca, int32_t j, bool up, double a, double den, double res) {
#pragma clang fp contract(off)
  const double g = double(up ? ca + j : ca - j + 1) * res;
  return (g - a) / den;
}

__device__ __forceinline__ void carve_visit(const VoxelStoreView& s, int32_t cx, int32_t cy, int32_t cz,
                                            uint32_t* __restrict__ counter, unsigned int* __restrict__ info) {
  const uint32_t slot = voxel_table_find(s, pack_cell(cx, cy, cz), &info[kInfoProbeError]);
  if (slot != kNoSlot) atomicAdd(&counter[slot], 1u);  // result unused: a no-return integer atomic
}

// The ray of one scan point.  false = skipped (nothing counted).
__device__ __forceinline__ bool carve_ray(const VoxelStoreView& s, const PosePod& pose, const VoxelCarveParams& prm, double x,
                                          double y, double z, uint32_t* __restrict__ crossings,
                                          uint32_t* __restrict__ hits, unsigned int* __restrict__ info) {
#pragma clang fp contract(off)
  double a[3], e[3], b[3], den[3];
  carve_warp(pose, prm.origin[0], prm.origin[1], prm.origin[2], a);
  carve_warp(pose, x, y, z, e);
  if (!(fabs(e[0]) <= 1.79e308 && fabs(e[1]) <= 1.79e308 && fabs(e[2]) <= 1.79e308)) return false;
  const double dx = e[0] - a[0], dy = e[1] - a[1], dz = e[2] - a[2];
  const double len = sqrt((dx * dx + dy * dy) + dz * dz);
  if (!(len > prm.min_range) || !(len > prm.end_margin)) return false;  // a NaN length is skipped too
  const double sc = len <= prm.max_range ? (len - prm.end_margin) / len : prm.max_range / len;
  b[0] = a[0] + sc * dx, b[1] = a[1] + sc * dy, b[2] = a[2] + sc * dz;
  int32_t ca[3], cb[3], ce[3];
  // all three cells are formed before any is judged: no short-circuit
  const bool in_a = carve_cell(a, prm.inv_res, ca), in_b = carve_cell(b, prm.inv_res, cb), in_e = carve_cell(e, prm.inv_res, ce);
  if (!(in_a && in_b && in_e)) return false;
  carve_visit(s, ce[0], ce[1], ce[2], hits, info);

  int32_t n[3], j[3] = {1, 1, 1};
  bool up[3];
  double tau[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    up[k] = cb[k] >= ca[k];
    n[k] = up[k] ? cb[k] - ca[k] : ca[k] - cb[k];
    den[k] = b[k] - a[k];
    if (n[k] > 0) tau[k] = carve_tau(ca[k], 1, up[k], a[k], den[k], prm.res);  // an axis that does not step divides nothing
  }
  uint32_t steps = uint32_t(n[0]) + uint32_t(n[1]) + uint32_t(n[2]);
  if (steps + 1u > prm.max_cells) {  // the host's max_range check rules this out; bounded all the same
    atomicOr(&info[kInfoProbeError], 2u);
    steps = prm.max_cells - 1u;
  }
  int32_t cx = ca[0], cy = ca[1], cz = ca[2];
  carve_visit(s, cx, cy, cz, crossings, info);
  for (uint32_t it = 0; it < steps; ++it) {
    // the pending crossing with the smallest tau; equal tau go to x before y before z
    int k = -1;
    double best = 0.0;
    if (j[0] <= n[0]) k = 0, best = tau[0];
    if (j[1] <= n[1] && (k < 0 || tau[1] < best)) k = 1, best = tau[1];
    if (j[2] <= n[2] && (k < 0 || tau[2] < best)) k = 2, best = tau[2];
    if (k < 0) break;  // cannot happen while it < n_x + n_y + n_z
    // one copy of the step, selected by k (no indexed register arrays)
    const int32_t jk = (k == 0 ? j[0] : k == 1 ? j[1] : j[2]) + 1;
    const int32_t nk = k == 0 ? n[0] : k == 1 ? n[1] : n[2];
    const bool upk = k == 0 ? up[0] : k == 1 ? up[1] : up[2];
    double tk = 0.0;
    if (jk <= nk)
      tk = carve_tau(k == 0 ? ca[0] : k == 1 ? ca[1] : ca[2], jk, upk, k == 0 ? a[0] : k == 1 ? a[1] : a[2],
                     k == 0 ? den[0] : k == 1 ? den[1] : den[2], prm.res);
    const int32_t step = upk ? 1 : -1;
    if (k == 0) cx += step, j[0] = jk, tau[0] = tk;
    else if (k == 1) cy += step, j[1] = jk, tau[1] = tk;
    else cz += step, j[2] = jk, tau[2] = tk;
    carve_visit(s, cx, cy, cz, crossings, info);
  }
  return true;
}

// Carve, step 1.  One lane per scan point (three planes in the scan's local frame, as voxel_points_kernel<true> reads
// them).  The skipped rays are counted by one integer atomic per wave.  Nothing of the store is written.
__global__ __launch_bounds__(256) void voxel_carve_walk_kernel(VoxelStoreView s, const double* __restrict__ src, uint64_t n,
                                                               PosePod pose, VoxelCarveParams prm,
                                                               uint32_t* __restrict__ crossings, uint32_t* __restrict__ hits,
                                                               unsigned int* __restrict__ info) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  unsigned int skipped = 0;
  if (i < n) skipped = carve_ray(s, pose, prm, src[i], src[n + i], src[2 * n + i], crossings, hits, info) ? 0u : 1u;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) skipped += __shfl_xor(skipped, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && skipped != 0) atomicAdd(&info[kInfoSkipped], skipped);
}

// Carve, step 2.  One lane per slot in use: keep[v] = 0 iff crossings[v] >= min_crossings and hits[v] < min_hits, and the
// totals voxel_keep_kernel forms.  Nothing of the store is written.
__global__ __launch_bounds__(256) void voxel_carve_keep_kernel(VoxelStoreView s, const uint32_t* __restrict__ crossings,
                                                               const uint32_t* __restrict__ hits, uint32_t min_crossings,
                                                               uint32_t min_hits, uint32_t* __restrict__ keep,
                                                               unsigned int* __restrict__ info) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  unsigned int removed = 0, kept_valid = 0;
  unsigned long long removed_points = 0;
  if (v < s.n_voxels) {
    const bool ok = !(crossings[v] >= min_crossings && hits[v] < min_hits);
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

}  // namespace nos
