// voxelraycast_kernels.hpp — ray casting through the voxel store: what would a sensor at this pose see?
//
// One cast = voxel_raycast_kernel (one lane per ray: the segment from the warped sensor origin to max_range along the
// beam is walked cell by cell by the carve's walk — raycast_walk, a copy of its loop that can stop; at every visited cell
// the store holds, that is valid and has enough points, the maximum-likelihood point of the voxel's Gaussian along the ray is taken inside the cell —
// tau clamped to [tau_in, tau_out] — and the first cell where its Mahalanobis distance passes the threshold ends the
// walk) → when the caller wants the hit points: one rocPRIM select of the hit positions and voxel_raycast_gather_kernel.
//
// The store is only READ.  A ray's result depends on that ray, the pose and the store alone: no lane reads what another
// wrote, and the only atomics are the two integer counters (hits, skipped), one add per wave each.
//
// The ray and the walk are stated operation by operation in include/nos.h (nos_voxel_map_raycast) and restated in numpy
// by tests/voxel_raycast_inputs.py; they stand under `fp contract(off)` like the carve's.  The hit test is NOT
// bit-defined: the compiler may fuse and reorder it (raycast_test stands outside the pragma).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "voxelcarve_kernels.hpp"

namespace nos {

// What the cast is handed.  origin is in the RAYS' frame; res / inv_res are the pair an insert uses.
struct VoxelRaycastParams {
  double origin[3];
  double min_range, max_range, max_mahalanobis_sq;
  double res, inv_res;
  uint32_t min_points;
  uint32_t max_cells;  // NOS_CARVE_MAX_CELLS: the bound on a ray's trip count
};

// The carve's walk from a (cell ca) to b (cell cb) with a visitor that may stop it — the ray cast's OWN copy of the loop
// of carve_ray (voxelcarve_kernels.hpp): with one loop shared by both kernels the carve ran 44 - 76 % longer (DESIGN.md
// §32), so the carve keeps its loop as it is.  Same crossings (carve_tau), same order, same bound.
// visit(cx, cy, cz, tau_in, tau_out) is called for the 1 + n_x + n_y + n_z cells in walk order, at the top of the loop so
// that the leaving crossing is known, and may end the walk by returning true.  tau_in is the parameter of the crossing that entered the cell (0 for the first), tau_out that of the
// crossing that leaves it (1 for the last).  *error gets bit 1 when the trip count ran past max_cells.
template <typename Visit>
__device__ __forceinline__ void raycast_walk(const double a[3], const double b[3], const int32_t ca[3], const int32_t cb[3],
                                             double res, uint32_t max_cells, unsigned int* error, Visit visit) {
#pragma clang fp contract(off)
  // the per-axis state in named scalars, read from the arrays once: nothing below indexes memory by the stepping axis
  const double a0 = a[0], a1 = a[1], a2 = a[2];
  const int32_t c0 = ca[0], c1 = ca[1], c2 = ca[2];
  const bool up0 = cb[0] >= c0, up1 = cb[1] >= c1, up2 = cb[2] >= c2;
  const int32_t n0 = up0 ? cb[0] - c0 : c0 - cb[0], n1 = up1 ? cb[1] - c1 : c1 - cb[1], n2 = up2 ? cb[2] - c2 : c2 - cb[2];
  const double den0 = b[0] - a0, den1 = b[1] - a1, den2 = b[2] - a2;
  // an axis that does not step divides nothing
  double tau0 = 0.0, tau1 = 0.0, tau2 = 0.0;
  if (n0 > 0) tau0 = carve_tau(c0, 1, up0, a0, den0, res);
  if (n1 > 0) tau1 = carve_tau(c1, 1, up1, a1, den1, res);
  if (n2 > 0) tau2 = carve_tau(c2, 1, up2, a2, den2, res);
  int32_t j0 = 1, j1 = 1, j2 = 1;
  uint32_t steps = uint32_t(n0) + uint32_t(n1) + uint32_t(n2);
  if (steps + 1u > max_cells) {  // the host's max_range check rules this out; bounded all the same
    atomicOr(error, 2u);
    steps = max_cells - 1u;
  }
  int32_t cx = c0, cy = c1, cz = c2;
  double tau_in = 0.0;
  for (uint32_t it = 0;; ++it) {
    // the pending crossing with the smallest tau; equal tau go to x before y before z
    int k = -1;
    double best = 1.0;
    if (it < steps) {  // k stays -1 past the last crossing: cannot happen while it < n_x + n_y + n_z
      if (j0 <= n0) k = 0, best = tau0;
      if (j1 <= n1 && (k < 0 || tau1 < best)) k = 1, best = tau1;
      if (j2 <= n2 && (k < 0 || tau2 < best)) k = 2, best = tau2;
    }
    if (visit(cx, cy, cz, tau_in, best) || k < 0) break;  // best is 1 for the last cell
    // one copy of the step, selected by k
    const int32_t jk = (k == 0 ? j0 : k == 1 ? j1 : j2) + 1;
    const int32_t nk = k == 0 ? n0 : k == 1 ? n1 : n2;
    const bool upk = k == 0 ? up0 : k == 1 ? up1 : up2;
    double tk = 0.0;
    if (jk <= nk)
      tk = carve_tau(k == 0 ? c0 : k == 1 ? c1 : c2, jk, upk, k == 0 ? a0 : k == 1 ? a1 : a2, k == 0 ? den0 : k == 1 ? den1 : den2, res);
    const int32_t step = upk ? 1 : -1;
    if (k == 0) cx += step, j0 = jk, tau0 = tk;
    else if (k == 1) cy += step, j1 = jk, tau1 = tk;
    else cz += step, j2 = jk, tau2 = tk;
    tau_in = best;
  }
}

// words of the cast's own counter block (arena memory, zeroed per call: the store's info block is not touched)
enum VoxelRaycastWord { kRaycastHits = 0, kRaycastSkipped = 1, kRaycastProbeError = 2, kRaycastWords = 4 };

// The test of one voxel: the maximum-likelihood point of N(mean, (SᵀS)⁻¹) along a + tau w, tau clamped to the cell's
// stretch of the ray.  true = hit, *tau_hit = the clamped parameter.  A NaN anywhere compares false: no hit.
__device__ __forceinline__ bool raycast_test(const VoxelStoreView& s, uint32_t v, const double a[3], const double w[3],
                                             double tau_in, double tau_out, const VoxelRaycastParams& prm, double* tau_hit) {
  const double* __restrict__ mean = s.mean + 3 * size_t(v);
  const double* __restrict__ S = s.sqrt_info + 9 * size_t(v);
  const double m0 = mean[0] - a[0], m1 = mean[1] - a[1], m2 = mean[2] - a[2];
  const double S0 = S[0], S1 = S[1], S2 = S[2], S3 = S[3], S4 = S[4], S5 = S[5], S6 = S[6], S7 = S[7], S8 = S[8];
  const double w0 = S0 * w[0] + S1 * w[1] + S2 * w[2], w1 = S3 * w[0] + S4 * w[1] + S5 * w[2], w2 = S6 * w[0] + S7 * w[1] + S8 * w[2];
  const double q0 = S0 * m0 + S1 * m1 + S2 * m2, q1 = S3 * m0 + S4 * m1 + S5 * m2, q2 = S6 * m0 + S7 * m1 + S8 * m2;
  const double den = w0 * w0 + w1 * w1 + w2 * w2;
  if (!(den > 0.0)) return false;
  const double tau_star = (w0 * q0 + w1 * q1 + w2 * q2) / den;
  if (!(tau_star == tau_star)) return false;  // fmax would drop the NaN
  const double tau_c = fmin(fmax(tau_star, tau_in), tau_out);
  const double u0 = tau_c * w[0] - m0, u1 = tau_c * w[1] - m1, u2 = tau_c * w[2] - m2;
  const double r0 = S0 * u0 + S1 * u1 + S2 * u2, r1 = S3 * u0 + S4 * u1 + S5 * u2, r2 = S6 * u0 + S7 * u1 + S8 * u2;
  const double dist = r0 * r0 + r1 * r1 + r2 * r2;
  *tau_hit = tau_c;
  return dist <= prm.max_mahalanobis_sq && tau_c * prm.max_range >= prm.min_range;
}

// The ray of one scan point.  false = skipped.  *voxel = the first voxel hit or -1; *range = its range or 0.0;
// *scale = range / len, the factor that takes p - origin to the hit point in the rays' frame (0.0 without a hit).
__device__ __forceinline__ bool raycast_ray(const VoxelStoreView& s, const PosePod& pose, const VoxelRaycastParams& prm, double x,
                                            double y, double z, int32_t* voxel, double* range, double* scale,
                                            unsigned int* __restrict__ counters) {
#pragma clang fp contract(off)
  *voxel = -1, *range = 0.0, *scale = 0.0;
  double a[3], e[3], b[3], w[3];
  carve_warp(pose, prm.origin[0], prm.origin[1], prm.origin[2], a);
  carve_warp(pose, x, y, z, e);
  if (!(fabs(e[0]) <= 1.79e308 && fabs(e[1]) <= 1.79e308 && fabs(e[2]) <= 1.79e308)) return false;
  const double dx = e[0] - a[0], dy = e[1] - a[1], dz = e[2] - a[2];
  const double len = sqrt((dx * dx + dy * dy) + dz * dz);
  if (!(len > 0.0)) return false;  // a NaN length is skipped too
  const double sc = prm.max_range / len;
  b[0] = a[0] + sc * dx, b[1] = a[1] + sc * dy, b[2] = a[2] + sc * dz;
  w[0] = b[0] - a[0], w[1] = b[1] - a[1], w[2] = b[2] - a[2];
  int32_t ca[3], cb[3];
  const bool in_a = carve_cell(a, prm.inv_res, ca), in_b = carve_cell(b, prm.inv_res, cb);  // both formed, then judged
  if (!(in_a && in_b)) return false;
  int32_t hit = -1;
  double tau_hit = 0.0;
  raycast_walk(a, b, ca, cb, prm.res, prm.max_cells, &counters[kRaycastProbeError],
             [&](int32_t cx, int32_t cy, int32_t cz, double tau_in, double tau_out) {
               const uint32_t v = voxel_table_find(s, pack_cell(cx, cy, cz), &counters[kRaycastProbeError]);
               if (v == kNoSlot) return false;
               // mean and S (12 doubles) are loaded only for a cell the store holds, that is valid and has the points
               if (s.valid[v] == 0 || s.count[v] < prm.min_points) return false;
               if (!raycast_test(s, v, a, w, tau_in, tau_out, prm, &tau_hit)) return false;
               hit = int32_t(v);
               return true;
             });
  if (hit >= 0) {
    const double r = tau_hit * prm.max_range;
    *voxel = hit, *range = r, *scale = r / len;
  }
  return true;
}

// The cast.  One lane per stored position of the scan (three planes in the rays' frame).  voxel_out / range_out are
// written for every position (coalesced), scale_out (may be nullptr) too.  Hits and skipped rays are counted by one
// integer atomic per wave each.  Nothing of the store is written.
__global__ __launch_bounds__(256) void voxel_raycast_kernel(VoxelStoreView s, const double* __restrict__ src, uint64_t n,
                                                            PosePod pose, VoxelRaycastParams prm, int32_t* __restrict__ voxel_out,
                                                            double* __restrict__ range_out, double* __restrict__ scale_out,
                                                            unsigned int* __restrict__ counters) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  unsigned int skipped = 0, hits = 0;
  if (i < n) {
    int32_t voxel;
    double range, scale;
    skipped = raycast_ray(s, pose, prm, src[i], src[n + i], src[2 * n + i], &voxel, &range, &scale, counters) ? 0u : 1u;
    hits = voxel >= 0 ? 1u : 0u;
    voxel_out[i] = voxel;
    range_out[i] = range;
    if (scale_out != nullptr) scale_out[i] = scale;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    skipped += __shfl_xor(skipped, o, kWave);
    hits += __shfl_xor(hits, o, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if (skipped != 0) atomicAdd(&counters[kRaycastSkipped], skipped);
    if (hits != 0) atomicAdd(&counters[kRaycastHits], hits);
  }
}

// keep[pos] for rocPRIM's select over the positions 0 .. n-1: the rays that hit
struct RaycastHit {
  const int32_t* voxel;
  __device__ __forceinline__ bool operator()(const uint32_t& pos) const { return voxel[pos] >= 0; }
};

// The scan of hit points: for the j-th hit in stored order, origin + scale (p - origin) per component (product rounded,
// then the sum) and the original index of its ray.
__global__ __launch_bounds__(256) void voxel_raycast_gather_kernel(const double* __restrict__ planes, uint32_t n,
                                                                   const uint32_t* __restrict__ order,
                                                                   const uint32_t* __restrict__ kept, uint32_t n_kept,
                                                                   const double* __restrict__ scale, double ox, double oy, double oz,
                                                                   double* __restrict__ out_planes, uint32_t* __restrict__ out_order) {
#pragma clang fp contract(off)
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_kept) return;
  const uint32_t pos = kept[j];
  const double q = scale[pos];
  out_planes[j] = ox + q * (planes[pos] - ox);
  out_planes[size_t(n_kept) + j] = oy + q * (planes[size_t(n) + pos] - oy);
  out_planes[2 * size_t(n_kept) + j] = oz + q * (planes[2 * size_t(n) + pos] - oz);
  out_order[j] = order != nullptr ? order[pos] : pos;
}

}  // namespace nos
