// mapbuild_kernels.hpp — NDT map construction on the GPU.
//
// Restates UpdateNdtMap of the reference's test harness
// (nonlinear_optimizer/mahalanobis_distance_minimizer/tests/simple_optimization_test.cc:236-281):
//   per point:  voxel key, ++count, sum += p, moment += p pᵀ   (moment starts at IDENTITY, MDM/types.h:14)
//   per voxel:  count < 5 → invalid;  mean = sum / count;  cov = moment / count − mean meanᵀ;
//               (here with d = p − the cell's corner in place of p, and mean = corner + sum / count: the same covariance
//               without the cancellation of eps |p|² far from the origin, voxel_finish.hpp)
//               eigen-decomposition (ascending);  largest eigenvalue < 0.01 → invalid;
//               the two smaller eigenvalues are floored at 0.01 × largest (:268-273);
//               sqrt_information = diag(eigvals^-1/2) · eigenvectors (:275-276)
// GPU form: voxel keys → stable radix sort of (key, point id) → run-length encode → one wave per
// voxel sums its points in a fixed order (lane-strided, then butterfly), so the statistics are
// deterministic, and finishes the 3×3 symmetric eigenproblem with cyclic Jacobi rotations.
// Eigenvector sign convention (the reference inherits Eigen's, which is not reproducible here):
// the first component of each eigenvector whose magnitude is within 1e-6 of its largest is positive.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hpp"
#include "voxel_finish.hpp"

namespace nos {

__global__ __launch_bounds__(256) void voxel_key_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                        const double* __restrict__ pz, uint64_t n, double inv_res,
                                                        uint64_t* __restrict__ keys, uint32_t* __restrict__ idx) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  keys[i] = pack_cell(int64_t(floor(px[i] * inv_res)), int64_t(floor(py[i] * inv_res)), int64_t(floor(pz[i] * inv_res)));
  idx[i] = uint32_t(i);
}

// Compact keys (round 4).  The packed key above spends 63 bits whatever the scene's extent, and a radix sort pays for every
// one of them: 8 passes over 10 M (key, index) pairs = 0.75 of the map build's 6.8 ms.  With the cells' bounding box known,
// key = ((x - x0) NY + (y - y0)) NZ + (z - z0) orders the cells exactly as the packed key does — lexicographically in
// (x, y, z) — in ceil(log2(NX NY NZ)) bits: 18 for a 100 x 100 x 10 m scene at 1 m, i.e. 3 passes.
//   box[0..2] = min cell, box[3..5] = max cell, initialised to INT64_MAX / INT64_MIN; grid-stride so that the whole grid
//   sends a few thousand atomics, not one per wave.
__global__ __launch_bounds__(256) void voxel_box_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                        const double* __restrict__ pz, uint64_t n, double inv_res,
                                                        long long* __restrict__ box) {
  long long lo[3] = {0x7FFFFFFFFFFFFFFFll, 0x7FFFFFFFFFFFFFFFll, 0x7FFFFFFFFFFFFFFFll};
  long long hi[3] = {-0x7FFFFFFFFFFFFFFFll - 1, -0x7FFFFFFFFFFFFFFFll - 1, -0x7FFFFFFFFFFFFFFFll - 1};
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.x) * 256) {
    const double c[3] = {floor(px[i] * inv_res), floor(py[i] * inv_res), floor(pz[i] * inv_res)};
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (c[k] >= -9.0e18 && c[k] <= 9.0e18) {  // finite and representable (a NaN fails both tests)
        const long long v = (long long)c[k];
        lo[k] = v < lo[k] ? v : lo[k];
        hi[k] = v > hi[k] ? v : hi[k];
      }
  }
  __shared__ long long s_lo[3][256], s_hi[3][256];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s_lo[k][threadIdx.x] = lo[k];
    s_hi[k][threadIdx.x] = hi[k];
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (int(threadIdx.x) < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const long long a = s_lo[k][threadIdx.x + o], b = s_hi[k][threadIdx.x + o];
        if (a < s_lo[k][threadIdx.x]) s_lo[k][threadIdx.x] = a;
        if (b > s_hi[k][threadIdx.x]) s_hi[k][threadIdx.x] = b;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) {
    atomicMin(&box[threadIdx.x], s_lo[threadIdx.x][0]);
    atomicMax(&box[3 + threadIdx.x], s_hi[threadIdx.x][0]);
  }
}

// origin = min cell, dims = NX, NY, NZ (their product < 2^62); coordinates outside the box (non-finite points) are clamped in
__global__ __launch_bounds__(256) void voxel_compact_key_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                                const double* __restrict__ pz, uint64_t n, double inv_res,
                                                                long long x0, long long y0, long long z0, long long nx,
                                                                long long ny, long long nz, uint64_t* __restrict__ keys,
                                                                uint32_t* __restrict__ idx) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  auto rel = [](double c, long long origin, long long dim) -> long long {
    if (!(c >= -9.0e18 && c <= 9.0e18)) return 0;
    const long long v = (long long)c - origin;
    return v < 0 ? 0 : (v >= dim ? dim - 1 : v);
  };
  const long long x = rel(floor(px[i] * inv_res), x0, nx), y = rel(floor(py[i] * inv_res), y0, ny),
                  z = rel(floor(pz[i] * inv_res), z0, nz);
  keys[i] = uint64_t((x * ny + y) * nz + z);
  idx[i] = uint32_t(i);
}

// Two kernels since round 4.  In the one-kernel form lane 0 of every wave ran the 3x3 eigen-decomposition while 63 lanes
// idled: at 796 k voxels of ≈ 12 points that was 3.0 of the build's 12 ms (profiles/r04_mapbuild_summary.json: issue stalls
// 46 %, one launch 3 041 µs).  Same additions in the same order, same eigen routine.
//
// The points once more as 32-byte records {x, y, z, 0}: the sums kernel GATHERS points by sorted index, and a gather of three
// 8-byte values from three planes touches three 64-byte sectors per point (1.9 GB of HBM traffic for 10 M points, 0.9 ms:
// profiles/r04_mapbuild_summary.json), one aligned 32-byte record one.
__global__ __launch_bounds__(256) void points_to_records_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                                const double* __restrict__ pz, uint64_t n,
                                                                double* __restrict__ rec /* [n][4] */) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  using V2 = double __attribute__((ext_vector_type(2)));
  V2* out = reinterpret_cast<V2*>(rec) + 2 * i;
  out[0] = V2{px[i], py[i]};
  out[1] = V2{pz[i], 0.0};
}

// (1) One wave per voxel: count / sum / moment in a fixed order.  seg_offset[v] .. + seg_count[v] index into sorted_idx.
//     acc_out: [n_voxels][9] = sx sy sz | mxx mxy mxz myy myz mzz of d = p − corner of p's cell, which every lane forms from
//     its own point (the expressions of the key kernels and of voxel_finish: floor(x inv_res), cell_origin).
//     rec != nullptr: the points as records (above).
__global__ __launch_bounds__(256) void voxel_sums_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                         const double* __restrict__ pz, const double* __restrict__ rec,
                                                         const uint32_t* __restrict__ sorted_idx,
                                                         const uint32_t* __restrict__ seg_offset,
                                                         const uint32_t* __restrict__ seg_count, uint32_t n_voxels,
                                                         double inv_res, double res, double* __restrict__ acc_out) {
  const uint32_t v = (blockIdx.x * 256 + threadIdx.x) / kWave;
  const int lane = threadIdx.x & (kWave - 1);
  if (v >= n_voxels) return;  // wave-uniform
  const uint32_t begin = seg_offset[v], count = seg_count[v];
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t k = lane; k < count; k += kWave) {
    const uint32_t i = sorted_idx[begin + k];
    double x, y, z;
    if (rec != nullptr) {  // kernel-uniform
      using V2 = double __attribute__((ext_vector_type(2)));
      const V2* r2 = reinterpret_cast<const V2*>(rec) + 2 * size_t(i);
      const V2 a = r2[0], b = r2[1];
      x = a[0], y = a[1], z = b[0];
    } else {
      x = px[i], y = py[i], z = pz[i];
    }
    x -= cell_origin(floor(x * inv_res), res);
    y -= cell_origin(floor(y * inv_res), res);
    z -= cell_origin(floor(z * inv_res), res);
    acc[0] += x;
    acc[1] += y;
    acc[2] += z;
    acc[3] = fma(x, x, acc[3]);
    acc[4] = fma(x, y, acc[4]);
    acc[5] = fma(x, z, acc[5]);
    acc[6] = fma(y, y, acc[6]);
    acc[7] = fma(y, z, acc[7]);
    acc[8] = fma(z, z, acc[8]);
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = wave_sum(acc[k]);
  if (lane < 9) {  // lane k stores sum k (every lane holds all nine after the butterfly)
    double mine = acc[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mine = lane == k ? acc[k] : mine;
    acc_out[9 * size_t(v) + lane] = mine;
  }
}

// How voxel_eigen_kernel reads a voxel's cell out of its sort key: the packed key (pack_cell), or the compact key
// ((x − x0) ny + (y − y0)) nz + (z − z0) of voxel_compact_key_kernel.
struct CellKeyForm {
  long long x0, y0, z0;
  unsigned long long ny, nz;
  int compact;
};

// (2) One LANE per voxel: the finish (voxel_finish.hpp), with the voxel's cell decoded from its key.
__global__ __launch_bounds__(256) void voxel_eigen_kernel(const double* __restrict__ acc_in,
                                                          const uint32_t* __restrict__ seg_count,
                                                          const uint64_t* __restrict__ seg_key, CellKeyForm form,
                                                          uint32_t n_voxels, MapBuildParams prm, double* __restrict__ mean_out,
                                                          double* __restrict__ sqrt_info_out,
                                                          unsigned char* __restrict__ valid_out) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_voxels) return;
  const uint32_t count = seg_count[v];
  double acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = acc_in[9 * size_t(v) + k];
  int64_t cell[3];
  const uint64_t key = seg_key[v];
  if (form.compact) {
    const uint64_t nyz = form.ny * form.nz;
    cell[0] = int64_t(key / nyz) + form.x0;
    cell[1] = int64_t((key % nyz) / form.nz) + form.y0;
    cell[2] = int64_t(key % form.nz) + form.z0;
  } else {
    int32_t c[3];
    unpack_cell(key, c);
    for (int k = 0; k < 3; ++k) cell[k] = c[k];
  }
  double S[9], mean[3];
  const unsigned char ok = voxel_finish(acc, count, cell, prm, mean, S);
  for (int k = 0; k < 3; ++k) mean_out[3 * size_t(v) + k] = mean[k];
  for (int k = 0; k < 9; ++k) sqrt_info_out[9 * size_t(v) + k] = S[k];
  valid_out[v] = ok;
}

}  // namespace nos
