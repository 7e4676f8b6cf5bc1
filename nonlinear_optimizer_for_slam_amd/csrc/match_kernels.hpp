// match_kernels.hpp — GPU correspondence matcher for NDT scan-to-map.
//
// Restates MatchPointCloud of the reference's test harness
// (nonlinear_optimizer/mahalanobis_distance_minimizer/tests/simple_optimization_test.cc:296-342):
// every scan point is warped by the current pose and matched to its (up to) two nearest valid NDT
// voxel means within the search radius (FLANN radiusSearch on L2_Simple, i.e. SQUARED distance
// < radius, max_neighbors = 2, sorted); each match becomes one correspondence
// {local point, mean, sqrt-information}.  The k-d tree is replaced by a uniform grid with cell
// edge = sqrt(radius) (1 + 2^-30): all candidates of a point lie in its 27-cell neighbourhood — the
// slack covers the rounding of x * inv_cell, see map_create_device.  The voxel records are stored
// in cell order so one cell's candidates are contiguous.
//
// Output goes straight into the tiled-SoA dataset the assemble kernels read: two slots per point
// (slot 2i + k = k-th nearest), an absent neighbour is an all-zero record, which contributes
// exactly nothing to H, g and cost — so no compaction pass and no host round trip are needed
// between matching and solving.  HBM-bound integer/pointer work: coalesced point reads, 16-byte
// coalesced record writes, candidate reads served from L2 (the map is small).
//
// One matcher for both kinds of map.  find_two_nearest has an overload per view — MapView here,
// VoxelMatchView (the live voxel store) in voxelmatch_kernels.hpp — and everything around the search exists once:
//   match_point<DST>     = warp_point, find_two_nearest, write_match_records   → records: match_kernel, voxel_match_kernel
//                          (that call for the thread's point, then add_match_count) and the registrations (register_problem)
//   match_point_ids      = warp_point, find_two_nearest, -1 for an absent slot → ids: match_index_kernel, voxel_match_index_kernel
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "assemble_kernels.hpp"

namespace nos {

constexpr uint64_t kEmptyCell = ~0ull;

struct MapView {
  const double* mean;        // [V][3] in cell order
  const double* sqrt_info;   // [V][9] row-major, cell order
  const uint32_t* orig_id;   // [V] original voxel index (tie-break, diagnostics)
  const uint64_t* cell_key;  // open-addressing table, kEmptyCell = free
  const uint32_t* cell_start;
  const uint32_t* cell_count;
  uint32_t table_mask;       // table size - 1 (power of two)
  double inv_cell;           // 1 / cell edge; the edge is sqrt(radius_sq) (1 + 2^-30), set by map_create_device alone
  double radius_sq;
  // Dense form of the same grid (set when the map's bounding box is small enough, which it is for every
  // scene the reference handles): cells in lexicographic (x, y, z) order — the order the voxel records are
  // stored in — with `dense_begin[c]` = number of records in cells before c.  The three z-neighbours of a
  // column are consecutive cells, so their records are ONE contiguous run [begin[c-1], begin[c+2]): a point
  // inspects 9 runs (2 loads each) instead of probing a hash table 27 times.
  const uint32_t* dense_begin;  // [nx*ny*nz + 1], null = hash table only
  const double* record;         // [V][4] = mean x, y, z, original id (bit pattern) — one 32-byte candidate record
  int64_t ox, oy, oz;           // cell coordinates of dense cell (0,0,0)
  int32_t nx, ny, nz;
};

__host__ __device__ __forceinline__ uint64_t pack_cell(int64_t ix, int64_t iy, int64_t iz) {
  const uint64_t bias = 1ull << 20;
  return ((uint64_t(ix + int64_t(bias)) & 0x1FFFFFull) << 42) | ((uint64_t(iy + int64_t(bias)) & 0x1FFFFFull) << 21) |
         (uint64_t(iz + int64_t(bias)) & 0x1FFFFFull);
}

__host__ __device__ __forceinline__ void unpack_cell(uint64_t key, int32_t c[3]) {
  const int32_t bias = 1 << 20;
  c[0] = int32_t((key >> 42) & 0x1FFFFFull) - bias;
  c[1] = int32_t((key >> 21) & 0x1FFFFFull) - bias;
  c[2] = int32_t(key & 0x1FFFFFull) - bias;
}

__host__ __device__ __forceinline__ uint32_t hash_cell(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return uint32_t(k);
}

struct PosePod {
  double R[9];
  double t[3];
};

struct TwoNearest {
  double d[2];
  uint32_t j[2];   // position in the map's cell-ordered arrays, 0xFFFFFFFF = none
  uint32_t id[2];  // original voxel id (tie-break)
  __device__ __forceinline__ void init() {
    d[0] = d[1] = 1e300;
    j[0] = j[1] = id[0] = id[1] = 0xFFFFFFFFu;
  }
  // keep the two smallest (distance, original id) pairs, nearest first
  __device__ __forceinline__ void offer(double dist, uint32_t pos, uint32_t orig) {
    if (dist < d[0] || (dist == d[0] && orig < id[0])) {
      d[1] = d[0];
      j[1] = j[0];
      id[1] = id[0];
      d[0] = dist;
      j[0] = pos;
      id[0] = orig;
    } else if (dist < d[1] || (dist == d[1] && orig < id[1])) {
      d[1] = dist;
      j[1] = pos;
      id[1] = orig;
    }
  }
};

// Squared distance, one fixed evaluation order for every form of the search (left to the compiler, "ex ex + ey ey + ez ez"
// fuses a different product in different surroundings: an ulp apart, enough to move a point across the radius test).
__device__ __forceinline__ double match_dist(double ex, double ey, double ez) {
  return __builtin_fma(ez, ez, __builtin_fma(ey, ey, ex * ex));
}

// The (up to) two nearest valid voxel means within the radius of the world point q — FLANN radiusSearch with
// max_neighbors = 2 on squared distances, ties broken by original voxel id.  Same result from both grid forms.
// One overload per map view (the live store's: voxelmatch_kernels.hpp), one signature: the warped point, the result in
// best.j (a position in view.mean / view.sqrt_info, or 0xFFFFFFFF), the probe-error word (unused: no probe here can fail).
__device__ __forceinline__ void find_two_nearest(const MapView& map, const double (&q)[3], TwoNearest& best, unsigned int*) {
  const double qx = q[0], qy = q[1], qz = q[2];
  best.init();
  const int64_t cx = int64_t(floor(qx * map.inv_cell));
  const int64_t cy = int64_t(floor(qy * map.inv_cell));
  const int64_t cz = int64_t(floor(qz * map.inv_cell));
  if (map.dense_begin != nullptr) {
    const int64_t rx = cx - map.ox, ry = cy - map.oy, rz = cz - map.oz;
    const int64_t z0 = rz - 1 < 0 ? 0 : rz - 1;
    const int64_t z1 = rz + 1 > map.nz - 1 ? map.nz - 1 : rz + 1;
    if (z0 > z1) return;
    using V2 = double __attribute__((ext_vector_type(2)));
    const V2* rec = reinterpret_cast<const V2*>(map.record);
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int64_t xx = rx + dx;
      if (xx < 0 || xx >= map.nx) continue;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int64_t yy = ry + dy;
        if (yy < 0 || yy >= map.ny) continue;
        const int64_t col = (xx * map.ny + yy) * map.nz;
        const uint32_t b = map.dense_begin[col + z0];
        const uint32_t e = map.dense_begin[col + z1 + 1];
        for (uint32_t j = b; j < e; ++j) {
          const V2 m01 = rec[2 * size_t(j)];
          const V2 m23 = rec[2 * size_t(j) + 1];
          const double dist = match_dist(qx - m01[0], qy - m01[1], qz - m23[0]);
          if (dist < map.radius_sq) best.offer(dist, j, uint32_t(__double_as_longlong(m23[1])));
        }
      }
    }
    return;
  }
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const uint64_t key = pack_cell(cx + dx, cy + dy, cz + dz);
        uint32_t h = hash_cell(key) & map.table_mask;
        uint32_t start = 0, count = 0;
        for (uint32_t probe = 0; probe <= map.table_mask; ++probe) {  // bounded: table is never full
          const uint64_t k = map.cell_key[h];
          if (k == key) {
            start = map.cell_start[h];
            count = map.cell_count[h];
            break;
          }
          if (k == kEmptyCell) break;
          h = (h + 1) & map.table_mask;
        }
        for (uint32_t j = start; j < start + count; ++j) {
          const double ex = qx - map.mean[3 * size_t(j)];
          const double ey = qy - map.mean[3 * size_t(j) + 1];
          const double ez = qz - map.mean[3 * size_t(j) + 2];
          const double dist = match_dist(ex, ey, ez);
          if (dist < map.radius_sq) best.offer(dist, j, map.orig_id[j]);
        }
      }
}

// The local point (x, y, z) warped by `pose`.  The multiply-adds are spelled out, in the form the compiler chose for
// match_kernel when it was written as `R0 x + R1 y + R2 z + t0`: left to the compiler, a different surrounding kernel
// could fuse another product.  match_point and match_point_ids, the only callers, warp every point of every matcher; the
// voxel store's insert (voxel_points_kernel) spells the same form.
__device__ __forceinline__ void warp_point(const PosePod& pose, double x, double y, double z, double& qx, double& qy,
                                           double& qz) {
  qx = __builtin_fma(pose.R[2], z, __builtin_fma(pose.R[0], x, pose.R[1] * y)) + pose.t[0];
  qy = __builtin_fma(pose.R[5], z, __builtin_fma(pose.R[3], x, pose.R[4] * y)) + pose.t[1];
  qz = __builtin_fma(pose.R[8], z, __builtin_fma(pose.R[6], x, pose.R[7] * y)) + pose.t[2];
}

// Slots 2i and 2i + 1 of the dataset for scan point i = (x, y, z): record k holds the local point, mean[best_j[k]] and
// sqrt_info[best_j[k]] (and its triangular factor U), or all zeros when best_j[k] is 0xFFFFFFFF (or k = 1 and
// max_neighbors = 1).  → the number of real records (0-2).  `mean` [V][3] and `sqrt_info` [V][9] are whatever arrays the
// search indexed: the snapshot's cell-ordered copies or the voxel store's own — one record writer, so the two routes
// store the same bits for the same voxel.
template <typename DST>
__device__ __forceinline__ int write_match_records(const double* __restrict__ mean, const double* __restrict__ sqrt_info,
                                                   const uint32_t (&best_j)[2], double x, double y, double z, uint64_t i,
                                                   int max_neighbors, const TiledLayout& L, DST* __restrict__ dst) {
  // two consecutive slots 2i, 2i+1 → one 2-wide store per field
  const uint64_t i0 = 2 * i;
  using V2 = DST __attribute__((ext_vector_type(2)));
  const bool ok0 = best_j[0] != 0xFFFFFFFFu;
  const bool ok1 = best_j[1] != 0xFFFFFFFFu && max_neighbors > 1;
  const double pl[3] = {x, y, z};
  auto put = [&](int plane, DST v0, DST v1) {  // slots 2i, 2i + 1 of one stored plane
    V2 v;
    v[0] = v0;
    v[1] = v1;
    *reinterpret_cast<V2*>(dst + plane_offset(L, i0, plane)) = v;
  };
#pragma unroll
  for (int f = 0; f < 3; ++f) put(f, ok0 ? DST(pl[f]) : DST(0), ok1 ? DST(pl[f]) : DST(0));
#pragma unroll
  for (int f = 0; f < 3; ++f)
    put(3 + f, ok0 ? DST(mean[3 * size_t(best_j[0]) + f]) : DST(0), ok1 ? DST(mean[3 * size_t(best_j[1]) + f]) : DST(0));
  DST S0[9], S1[9], U0[6], U1[6];
#pragma unroll
  for (int f = 0; f < 9; ++f) {
    S0[f] = ok0 ? DST(sqrt_info[9 * size_t(best_j[0]) + f]) : DST(0);
    S1[f] = ok1 ? DST(sqrt_info[9 * size_t(best_j[1]) + f]) : DST(0);
    put(ndt_stored_plane(6 + f), S0[f], S1[f]);
  }
  sqrt_info_to_U<DST>(S0, U0);
  sqrt_info_to_U<DST>(S1, U1);
#pragma unroll
  for (int k = 0; k < 6; ++k) put(6 + k, U0[k], U1[k]);
  return int(ok0) + int(ok1);
}

// The number of real matches of a launch: wave sum of the per-lane counts → one atomic per wave (integer, order
// independent).  Every lane of the block calls this (lanes without a point with found = 0).
__device__ __forceinline__ void add_match_count(int found, unsigned long long* __restrict__ n_matches) {
  int s = found;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && s > 0) atomicAdd(n_matches, (unsigned long long)s);
}

// Scan point i (i < n_points) warped by `pose` and matched against `map` (a MapView or a VoxelMatchView): writes slots
// 2i and 2i + 1 of the dataset and returns the number of real matches among them (0-2).  error: the probe-error word
// find_two_nearest is handed.  The one-thread-per-point kernels and the batched registrations (register_problem: the
// lanes of one workgroup striding over a scan) all call this, so a registration round's records are a lone match's bits.
template <typename DST, typename View>
__device__ __forceinline__ int match_point(const View& map, const double* __restrict__ px, const double* __restrict__ py,
                                           const double* __restrict__ pz, uint64_t i, const PosePod& pose,
                                           int max_neighbors, const TiledLayout& L, DST* __restrict__ dst,
                                           unsigned int* __restrict__ error) {
  const double x = px[i], y = py[i], z = pz[i];
  double q[3];
  warp_point(pose, x, y, z, q[0], q[1], q[2]);
  TwoNearest best;
  find_two_nearest(map, q, best, error);
  return write_match_records<DST>(map.mean, map.sqrt_info, best.j, x, y, z, i, max_neighbors, L, dst);
}

// match_point naming the voxels instead of writing their records: idx0[i] / idx1[i] = best.j of the nearest / second
// nearest voxel, or -1 (idx1 also when max_neighbors = 1).  → the number of ids that are not -1.  The same warp and the
// same search, so the indexed form names exactly the voxels whose records the flat form writes.
// kSecondFirst: the order of the two terms of that number, which moves the last ten instructions of an index kernel: each
// kernel names the order that keeps the body it had before it called this function (tools/compare_kernel_asm.py).  It
// pins the source to one compiler's choice: delete it as soon as identical code objects are no longer asked for.
template <bool kSecondFirst, typename View>
__device__ __forceinline__ int match_point_ids(const View& map, const double* __restrict__ px, const double* __restrict__ py,
                                               const double* __restrict__ pz, uint64_t i, const PosePod& pose,
                                               int max_neighbors, int32_t* __restrict__ idx0, int32_t* __restrict__ idx1,
                                               unsigned int* __restrict__ error) {
  double q[3];
  warp_point(pose, px[i], py[i], pz[i], q[0], q[1], q[2]);
  TwoNearest best;
  find_two_nearest(map, q, best, error);
  const bool ok0 = best.j[0] != 0xFFFFFFFFu, ok1 = best.j[1] != 0xFFFFFFFFu && max_neighbors > 1;
  idx0[i] = ok0 ? int32_t(best.j[0]) : -1;  // a position is < 2^31 (nos_ndt_map_create, store_reserve)
  idx1[i] = ok1 ? int32_t(best.j[1]) : -1;
  if constexpr (kSecondFirst) return int(ok1) + int(ok0);
  return int(ok0) + int(ok1);
}

// One thread per scan point.  points: 3 planes of n doubles (local frame).
template <typename DST>
__global__ __launch_bounds__(256) void match_kernel(MapView map, const double* __restrict__ px,
                                                    const double* __restrict__ py,
                                                    const double* __restrict__ pz, uint64_t n_points,
                                                    PosePod pose, int max_neighbors, TiledLayout L,
                                                    DST* __restrict__ dst,
                                                    unsigned long long* __restrict__ n_matches) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  const int found = i < n_points ? match_point<DST>(map, px, py, pz, i, pose, max_neighbors, L, dst, nullptr) : 0;
  add_match_count(found, n_matches);
}

// Clears the last n_drop NON-EMPTY records of a matcher-written NDT dataset, in slot order: what dropping the tail of
// the reference's compacted correspondence vector does (floor(N/4)*4 of the scalar 3-DoF class,
// MDM/mahalanobis_distance_minimizer_analytic_3dof.cc:33-36).  A record is empty when its sqrt-information is all zero.
// One wave walks backwards from the end, 64 slots at a time; n_drop is small (< 8), so it touches the tail only.
// drop_last_records is that wave's work (lane = 0 … 63), also run by the first wave of register_batch_kernel.
template <typename T>
__device__ __forceinline__ void drop_last_records(T* __restrict__ data, const TiledLayout& L, uint64_t n_drop, int lane) {
  uint64_t remaining = n_drop;
  for (uint64_t pos = L.n; remaining > 0 && pos > 0; pos = pos > 64 ? pos - 64 : 0) {
    const bool in_range = pos > uint64_t(lane);
    const uint64_t i = in_range ? pos - 1 - uint64_t(lane) : 0;
    bool nonempty = false;
    if (in_range)
      for (int f = 6; f < 15; ++f) nonempty = nonempty || data[plane_offset(L, i, ndt_stored_plane(f))] != T(0);
    const unsigned long long mask = __ballot(nonempty);
    const uint64_t before = uint64_t(__popcll(mask & ((1ull << lane) - 1ull)));  // non-empty slots nearer to the end
    if (nonempty && before < remaining)  // all 21 stored planes (U as well): the cleared record contributes nothing
      for (int f = 0; f < kNdtStored; ++f) data[plane_offset(L, i, f)] = T(0);
    const uint64_t found = uint64_t(__popcll(mask));
    remaining -= found < remaining ? found : remaining;
  }
}

template <typename T>
__global__ __launch_bounds__(64) void drop_last_matches_kernel(T* __restrict__ data, TiledLayout L, uint64_t n_drop) {
  drop_last_records<T>(data, L, n_drop, int(threadIdx.x));
}

// tiled dataset → planar host-order planes (diagnostics / tests); flat NDT (ndt != 0): the 15 planes of nos.h (p, mu, S)
template <typename SRC>
__global__ __launch_bounds__(256) void untile_kernel(const SRC* __restrict__ src, int n_fields, int ndt, TiledLayout L,
                                                     double* __restrict__ dst /* [n_fields][L.n] */) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  const int f = blockIdx.y;
  if (i >= L.n || f >= n_fields) return;
  const uint64_t off = plane_offset(L, i, ndt != 0 ? ndt_stored_plane(f) : f);
  dst[uint64_t(f) * L.n + i] = double(src[off]);
}

}  // namespace nos

// match_kernel emitting voxel ids (positions in the map's cell-ordered arrays) instead of records.  Not a template, so
// every unit that sees the definition compiles a copy: nos_indexed.hip, the one unit that launches it, asks for it.
#ifdef NOS_WITH_MATCH_INDEX_KERNEL
namespace {
__global__ __launch_bounds__(256) void match_index_kernel(nos::MapView map, const double* __restrict__ px,
                                                          const double* __restrict__ py, const double* __restrict__ pz,
                                                          uint64_t n_points, nos::PosePod pose, int max_neighbors,
                                                          int32_t* __restrict__ idx0, int32_t* __restrict__ idx1,
                                                          unsigned long long* __restrict__ n_matches) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  const int found = i < n_points ? nos::match_point_ids<true>(map, px, py, pz, i, pose, max_neighbors, idx0, idx1, nullptr) : 0;
  nos::add_match_count(found, n_matches);
}
}  // namespace
#endif
