// voxeld2d_kernels.hpp — one live voxel store matched against another: distribution-to-distribution NDT (Stoyanov et
// al. 2012).  Every valid voxel of a SOURCE store is warped by the pose, looked up on a TARGET store with the
// point matcher's own search (warp_point, find_two_nearest on the VoxelMatchView: same radius test, guard band and
// (distance, slot) order), and each match becomes one ordinary flat NDT record
//   p = mean_s (source frame),  mu = mean_j,  S with SᵀS = A = (Σ_j + R Σ_s Rᵀ)⁻¹,  U = sqrt_info_to_U(S),
// Σ_x = (S_xᵀ S_x)⁻¹ being the covariance the store's sqrt-information stands for (eigenvalue floor included).  A is
// evaluated at the pose of the match and held fixed by the solve that follows, as the correspondences are.  Source slot v
// owns dataset slots 2v and 2v + 1, so the result has write_match_records' form and every solver path runs on it.
//
// voxel_pair_information holds all the arithmetic that is new; the kernel and the host test hook
// nos_debug_voxel_pair_information both call it, as voxel_finish and voxel_moments are shared.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxelmatch_kernels.hpp"

namespace nos {

// B = S⁻¹ (row-major) by the adjugate → false when the determinant is zero (a NaN passes here and fails the pivots of
// the caller's Cholesky).
__host__ __device__ __forceinline__ bool voxel_inverse3(const double (&S)[9], double (&B)[9]) {
#pragma clang fp contract(off)
  double adj[9];
  adj[0] = S[4] * S[8] - S[5] * S[7];
  adj[1] = S[2] * S[7] - S[1] * S[8];
  adj[2] = S[1] * S[5] - S[2] * S[4];
  adj[3] = S[5] * S[6] - S[3] * S[8];
  adj[4] = S[0] * S[8] - S[2] * S[6];
  adj[5] = S[2] * S[3] - S[0] * S[5];
  adj[6] = S[3] * S[7] - S[4] * S[6];
  adj[7] = S[1] * S[6] - S[0] * S[7];
  adj[8] = S[0] * S[4] - S[1] * S[3];
  const double det = S[0] * adj[0] + S[1] * adj[3] + S[2] * adj[6];
#pragma unroll
  for (int k = 0; k < 9; ++k) B[k] = adj[k] / det;
  return det != 0.0;
}

// S_out (row-major, lower triangular) with S_outᵀ S_out = (Σ_t + R Σ_s Rᵀ)⁻¹, where Σ_x = (S_xᵀ S_x)⁻¹ = S_x⁻¹ S_x⁻ᵀ.
// → 1, or 0 (S_out all zero) when an input is not finite or singular, or the combined covariance is not finite or not
// positive definite.  R row-major, not checked for orthonormality.
//   1. B_x = S_x⁻¹ by the adjugate: the condition of S_x, not of S_xᵀ S_x, enters;
//   2. C = B_t B_tᵀ + (R B_s)(R B_s)ᵀ, the six entries of the lower triangle;
//   3. C = L Lᵀ (Cholesky) and S_out = L⁻¹ by forward substitution: A = L⁻ᵀ L⁻¹.
// Plain fp64 with division and sqrt, nothing fused: host and device round alike.
__host__ __device__ __forceinline__ unsigned char voxel_pair_information(const double (&St)[9], const double (&Ss)[9],
                                                                         const double (&R)[9], double (&S_out)[9]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int k = 0; k < 9; ++k) S_out[k] = 0.0;
  double Bt[9], Bs[9], RB[9];  // S_t⁻¹, S_s⁻¹, R S_s⁻¹
  bool ok = voxel_inverse3(St, Bt);
  ok = voxel_inverse3(Ss, Bs) && ok;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) RB[3 * i + j] = R[3 * i] * Bs[j] + R[3 * i + 1] * Bs[3 + j] + R[3 * i + 2] * Bs[6 + j];
  double C[3][3];  // lower triangle of the combined covariance
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j > i) continue;
      const double ct = Bt[3 * i] * Bt[3 * j] + Bt[3 * i + 1] * Bt[3 * j + 1] + Bt[3 * i + 2] * Bt[3 * j + 2];
      const double cs = RB[3 * i] * RB[3 * j] + RB[3 * i + 1] * RB[3 * j + 1] + RB[3 * i + 2] * RB[3 * j + 2];
      C[i][j] = ct + cs;
    }
  // Cholesky, row by row; a pivot that is not a positive finite number (NaN included) ends it
  const double big = 1.0e300;
  const double p0 = C[0][0];
  ok = ok && p0 > 0.0 && p0 < big;
  const double l00 = sqrt(p0);
  const double l10 = C[1][0] / l00, l20 = C[2][0] / l00;
  const double p1 = C[1][1] - l10 * l10;
  ok = ok && p1 > 0.0 && p1 < big;
  const double l11 = sqrt(p1);
  const double l21 = (C[2][1] - l20 * l10) / l11;
  const double p2 = C[2][2] - l20 * l20 - l21 * l21;
  ok = ok && p2 > 0.0 && p2 < big;
  const double l22 = sqrt(p2);
  // L⁻¹, lower triangular
  const double s00 = 1.0 / l00, s11 = 1.0 / l11, s22 = 1.0 / l22;
  const double s10 = -(l10 * s00) / l11;
  const double s21 = -(l21 * s11) / l22;
  const double s20 = -(l20 * s00 + l21 * s10) / l22;
  const double out[9] = {s00, 0.0, 0.0, s10, s11, 0.0, s20, s21, s22};
#pragma unroll
  for (int k = 0; k < 9; ++k) ok = ok && out[k] - out[k] == 0.0;  // finite
  if (!ok) return 0;
#pragma unroll
  for (int k = 0; k < 9; ++k) S_out[k] = out[k];
  return 1;
}

// One lane per source slot v < n_src: slots 2v and 2v + 1 of the dataset (nearest, second nearest).  An invalid source
// voxel, a missing neighbour, the second slot when max_neighbors = 1 and a pair voxel_pair_information refuses write
// all-zero records and are not counted.  The search runs first and the 3 x 3 algebra afterwards, neighbour by neighbour,
// so the nine-probe state and the matrix temporaries are not live together.  Both stores are read, neither is written
// (src_* may be the target's own arrays); error: the TARGET's kInfoProbeError word.  rot: pose.R once more, as a kernel
// argument of its own: the copy the algebra reads is fetched after the search instead of being held in scalar registers
// across it, where the search's own uniform state leaves no room for it (with one copy the kernel reserves scratch for
// scalar spills).  That is the register allocation of one compiler: the second copy can go, and the algebra read
// pose.R, as soon as that form builds without scratch — the resource test (tests/test_voxel_map_match_map_abi.py) says.
// The arguments ahead of n_src are what the host's StoreVoxels hands over (match_host.hpp's Items).
struct RotPod {
  double R[9];
};

template <typename DST>
__global__ __launch_bounds__(256) void voxel_match_map_kernel(VoxelMatchView map, const unsigned char* __restrict__ src_valid,
                                                              const double* __restrict__ src_mean,
                                                              const double* __restrict__ src_sqrt_info, RotPod rot,
                                                              uint64_t n_src, PosePod pose, int max_neighbors, TiledLayout L,
                                                              DST* __restrict__ dst, unsigned long long* __restrict__ n_matches,
                                                              unsigned int* __restrict__ error) {
  const uint64_t v = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  int found = 0;
  if (v < n_src) {
    double p[3] = {0.0, 0.0, 0.0};
    uint32_t j[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
    if (src_valid[v] != 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = src_mean[3 * size_t(v) + k];
      double q[3];
      warp_point(pose, p[0], p[1], p[2], q[0], q[1], q[2]);
      TwoNearest best;
      find_two_nearest(map, q, best, error);
      j[0] = best.j[0];
      j[1] = max_neighbors > 1 ? best.j[1] : 0xFFFFFFFFu;
    }
    double mu[2][3], S[2][9];
    bool ok[2];
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      ok[n] = false;
#pragma unroll
      for (int k = 0; k < 3; ++k) mu[n][k] = 0.0;
#pragma unroll
      for (int k = 0; k < 9; ++k) S[n][k] = 0.0;
      if (j[n] != 0xFFFFFFFFu) {
        double St[9], Ss[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          St[k] = map.sqrt_info[9 * size_t(j[n]) + k];
          Ss[k] = src_sqrt_info[9 * size_t(v) + k];
        }
        ok[n] = voxel_pair_information(St, Ss, rot.R, S[n]) != 0;
        if (ok[n]) {
#pragma unroll
          for (int k = 0; k < 3; ++k) mu[n][k] = map.mean[3 * size_t(j[n]) + k];
        }
      }
    }
    // the record writer of write_match_records: two consecutive slots → one 2-wide store per stored plane
    using V2 = DST __attribute__((ext_vector_type(2)));
    const uint64_t i0 = 2 * v;
    auto put = [&](int plane, DST v0, DST v1) {
      V2 w;
      w[0] = v0;
      w[1] = v1;
      *reinterpret_cast<V2*>(dst + plane_offset(L, i0, plane)) = w;
    };
#pragma unroll
    for (int f = 0; f < 3; ++f) put(f, ok[0] ? DST(p[f]) : DST(0), ok[1] ? DST(p[f]) : DST(0));
#pragma unroll
    for (int f = 0; f < 3; ++f) put(3 + f, DST(mu[0][f]), DST(mu[1][f]));
    DST S0[9], S1[9], U0[6], U1[6];
#pragma unroll
    for (int f = 0; f < 9; ++f) {
      S0[f] = DST(S[0][f]);
      S1[f] = DST(S[1][f]);
      put(ndt_stored_plane(6 + f), S0[f], S1[f]);
    }
    sqrt_info_to_U<DST>(S0, U0);
    sqrt_info_to_U<DST>(S1, U1);
#pragma unroll
    for (int k = 0; k < 6; ++k) put(6 + k, U0[k], U1[k]);
    found = int(ok[0]) + int(ok[1]);
  }
  add_match_count(found, n_matches);
}

}  // namespace nos
