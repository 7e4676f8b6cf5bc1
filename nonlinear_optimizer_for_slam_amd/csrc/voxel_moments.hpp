// voxel_moments.hpp — one NDT voxel's count / sum / moment moved by a rigid pose into another grid: the
// destination cell and the nine sums about THAT cell's corner.  A host / device function only, no kernels, next to
// voxel_finish.hpp: shared by the store's merge (voxel_moments_kernel, voxelmerge_kernels.hpp) and the host test hook
// nos_debug_voxel_moments.
//
// With n = count, s = Σd, M = Σ d dᵀ about the corner o of the source cell, a point p = o + d goes to
// p' = R p + t = o' + d' with d' = R d + b, b = (R o + t) − o', so
//   s' = R s + n b,    M' = R M Rᵀ + (R s) bᵀ + b (R s)ᵀ + n b bᵀ.
// The covariance M'/n − (s'/n)(s'/n)ᵀ = R (M/n − (s/n)(s/n)ᵀ) Rᵀ does not depend on b: b is formed ONCE and that value
// is used in every term, so its rounding error moves the mean and nothing else.
//
// The destination cell is the cell of the transformed MEAN, floor((R mu + t) · inv_res) with the multiply-adds of the
// matcher's warp (warp_point, match_kernels.hpp): the cell an insert_scan would put a point at the source voxel's mean into.
// The whole voxel goes there.  The mean comes from the sums, never from the store's mean array (zero below min_points).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxel_finish.hpp"

namespace nos {

// acc = sx sy sz | mxx mxy mxz myy myz mzz about the corner of `cell` in a grid of edge res_src, count >= 1;
// R row-major, not checked for orthonormality; inv_res_dst = 1.0 / res_dst, the value an insert hands voxel_points_kernel.
// → cell_out: the destination cell per axis as floor() returned it (integer-valued, or non-finite when the pose
// overflows: the caller checks the range before it converts), out: the nine sums about cell_origin(cell_out, res_dst).
// Nothing is fused except the three multiply-adds of the warp, which are spelled out: host and device round alike.
__host__ __device__ inline void voxel_moments(uint32_t count, const double (&acc)[9], const int64_t (&cell)[3], double res_src,
                                              const double (&R)[9], const double (&t)[3], double res_dst, double inv_res_dst,
                                              double (&cell_out)[3], double (&out)[9]) {
#pragma clang fp contract(off)
  const double n = double(count);
  double o[3], mu[3];
  for (int k = 0; k < 3; ++k) {
    o[k] = cell_origin(double(cell[k]), res_src);
    mu[k] = o[k] + acc[k] / n;
  }
  double b[3], Rs[3];
  for (int i = 0; i < 3; ++i) {
    const double* r = R + 3 * i;
    const double q = __builtin_fma(r[2], mu[2], __builtin_fma(r[0], mu[0], r[1] * mu[1])) + t[i];  // the warp of the mean
    cell_out[i] = floor(q * inv_res_dst);
    const double Ro = __builtin_fma(r[2], o[2], __builtin_fma(r[0], o[0], r[1] * o[1])) + t[i];    // the warp of the corner
    b[i] = Ro - cell_origin(cell_out[i], res_dst);
    Rs[i] = r[0] * acc[0] + r[1] * acc[1] + r[2] * acc[2];
    out[i] = Rs[i] + n * b[i];
  }
  const double M[9] = {acc[3], acc[4], acc[5], acc[4], acc[6], acc[7], acc[5], acc[7], acc[8]};
  double RM[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) RM[3 * i + j] = R[3 * i] * M[j] + R[3 * i + 1] * M[3 + j] + R[3 * i + 2] * M[6 + j];
  int e = 3;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      const double rmr = RM[3 * i] * R[3 * j] + RM[3 * i + 1] * R[3 * j + 1] + RM[3 * i + 2] * R[3 * j + 2];
      out[e++] = ((rmr + Rs[i] * b[j]) + b[i] * Rs[j]) + (n * b[i]) * b[j];
    }
}

}  // namespace nos
