// voxelmatch_kernels.hpp — the correspondence matcher on the LIVE voxel store: no snapshot per frame.
//
// MatchPointCloud of the reference's test harness
// (nonlinear_optimizer/mahalanobis_distance_minimizer/tests/simple_optimization_test.cc:296-342), as match_kernels.hpp
// restates it, with the k-d tree replaced by the table the store's insert already maintains: a voxel cell holds at most
// ONE voxel, so the candidates of a warped point are the cells its search ball touches, each looked up by key
// (voxel_table_find's probe sequence) in VoxelStoreView::table_key / table_slot.  Nothing is sorted, gathered or built
// per frame: the work of a match follows the scan, not the size of the map.
//
// The result is, bit for bit, what match_kernel gives on a snapshot of the same store: this header adds one overload of
// find_two_nearest and nothing else of the matcher (match_point and match_point_ids of match_kernels.hpp, instantiated for
// this view), with the same distance (match_dist), the same strict radius test and the same (distance, voxel id) order
// in TwoNearest — the slot number IS the id a snapshot carries for the voxel, view.mean / view.sqrt_info the values it
// copies.  TwoNearest::offer keeps the two smallest (distance, id) pairs of whatever it is offered, in any order, so only
// the SET of candidates matters: the visited cells must hold every valid voxel whose mean can pass the radius test.  That
// is the guard band `g` (kVoxelMatchGuard of a cell edge; the argument is in DESIGN.md §15): a mean lies in its own cell
// only up to the rounding of the sums and of the cell assignment.
//
// Memory side: per (x, 3 x 3 block of y, z) step a lane issues NINE independent probes — key and slot of the first
// table entry of every cell are loaded together, then valid flag and mean of every hit — so a 27-cell search is three
// rounds of dependent loads, not 27; a collision (the table is at most half full) is resolved by a bounded loop
// afterwards.  Consecutive z cells differ in the lowest key bits only, but the hash scatters them: what makes the lanes of
// a wave share table lines is a cell-sorted scan (nos_scan_sort_by_cell).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hpp"

namespace nos {

constexpr double kVoxelMatchGuard = 1.0 / 1024.0;  // guard band g as a fraction of the voxel edge
constexpr int kVoxelMatchMaxSpan = 9;              // cells a search ball may span per axis (nos_voxel_map_match rejects more)

// The store as the matcher reads it (nothing of it is written).
struct VoxelMatchView {
  const unsigned long long* table_key;  // [table_mask + 1], kEmptyCell = free
  const uint32_t* table_slot;           // [table_mask + 1]
  const double* mean;                   // [capacity][3]
  const double* sqrt_info;              // [capacity][9]
  const unsigned char* valid;           // [capacity]
  uint32_t table_mask;
  double inv_res;    // 1.0 / voxel_resolution: the factor the insert assigns cells with
  double reach;      // sqrt(radius_sq) + g
  double radius_sq;
};

// find_two_nearest on the live store: the cells the ball around the warped point q touches, and the nine-probe rounds
// into `best` — best.j[k] is the store slot of the k-th nearest valid voxel mean within the radius (ties by slot), or
// 0xFFFFFFFF.  error: the store's kInfoProbeError word, raised when a probe runs through the whole table.
__device__ __forceinline__ void find_two_nearest(const VoxelMatchView& map, const double (&q)[3], TwoNearest& best,
                                                 unsigned int* __restrict__ error) {
  constexpr int kProbes = 9;  // the 3 x 3 block of (y, z) cells probed together per step
  // cells floor((q - r - g) inv_res) … floor((q + r + g) inv_res) per axis, clamped to the addressable grid
  // [-2^20, 2^20) that voxel_points_kernel admits — no voxel lives outside it, and pack_cell would fold a cell beyond
  // it onto a real key.  A point that is not finite, or whose range misses the grid altogether, visits no cell.
  int64_t c0[3];
  int span[3];
  bool reachable = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lim = double(1 << 20);
    const double lo = fmax(floor((q[k] - map.reach) * map.inv_res), -lim);
    const double hi = fmin(floor((q[k] + map.reach) * map.inv_res), lim - 1.0);
    reachable = reachable && (lo <= hi);  // a NaN fails (fmax / fmin would drop it: test the point itself too)
    reachable = reachable && (q[k] == q[k]);
    c0[k] = reachable ? int64_t(lo) : 0;
    const int n = reachable ? int(hi - lo) + 1 : 0;
    span[k] = n < kVoxelMatchMaxSpan ? n : kVoxelMatchMaxSpan;
  }
  if (!reachable) span[0] = 0;
  best.init();
  for (int ix = 0; ix < span[0]; ++ix)
    for (int by = 0; by < span[1]; by += 3)
      for (int bz = 0; bz < span[2]; bz += 3) {
        uint64_t key[kProbes];
        uint32_t h[kProbes], slot[kProbes];
        unsigned long long seen[kProbes];
        bool on[kProbes];
        // round 1: the first table entry of every cell of the block — key and slot loaded together, nothing depends on
        // a compare
#pragma unroll
        for (int u = 0; u < kProbes; ++u) {
          const int dy = by + u / 3, dz = bz + u % 3;
          on[u] = dy < span[1] && dz < span[2];
          key[u] = pack_cell(c0[0] + ix, c0[1] + dy, c0[2] + dz);
          h[u] = hash_cell(key[u]) & map.table_mask;
        }
#pragma unroll
        for (int u = 0; u < kProbes; ++u) {
          seen[u] = map.table_key[h[u]];
          slot[u] = map.table_slot[h[u]];
        }
        // collisions: voxel_table_find's probe sequence from the second entry on, bounded by the table size
#pragma unroll
        for (int u = 0; u < kProbes; ++u) {
          bool hit = on[u] && seen[u] == key[u];
          if (on[u] && !hit && seen[u] != kEmptyCell) {
            uint32_t hh = h[u];
            bool ended = false;
            for (uint32_t probe = 1; probe <= map.table_mask; ++probe) {
              hh = (hh + 1) & map.table_mask;
              const unsigned long long k = map.table_key[hh];
              if (k == key[u]) {
                slot[u] = map.table_slot[hh];
                hit = ended = true;
                break;
              }
              if (k == kEmptyCell) {
                ended = true;
                break;
              }
            }
            if (!ended) atomicOr(error, 1u);
          }
          on[u] = hit;
          slot[u] = hit ? slot[u] : 0u;  // slot 0 exists in every store (capacity >= 16): a miss reads it and drops it
        }
        // round 2: valid flag and mean of every hit, again independent loads
        unsigned char ok[kProbes];
        double m[kProbes][3];
#pragma unroll
        for (int u = 0; u < kProbes; ++u) {
          ok[u] = map.valid[slot[u]];
#pragma unroll
          for (int k = 0; k < 3; ++k) m[u][k] = map.mean[3 * size_t(slot[u]) + k];
        }
#pragma unroll
        for (int u = 0; u < kProbes; ++u) {
          const double dist = match_dist(q[0] - m[u][0], q[1] - m[u][1], q[2] - m[u][2]);
          if (on[u] && ok[u] != 0 && dist < map.radius_sq) best.offer(dist, slot[u], slot[u]);
        }
      }
}

// One thread per scan point.  points: 3 planes of n doubles (local frame).  error: the store's kInfoProbeError word.
template <typename DST>
__global__ __launch_bounds__(256) void voxel_match_kernel(VoxelMatchView map, const double* __restrict__ px,
                                                          const double* __restrict__ py, const double* __restrict__ pz,
                                                          uint64_t n_points, PosePod pose, int max_neighbors, TiledLayout L,
                                                          DST* __restrict__ dst, unsigned long long* __restrict__ n_matches,
                                                          unsigned int* __restrict__ error) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  const int found = i < n_points ? match_point<DST>(map, px, py, pz, i, pose, max_neighbors, L, dst, error) : 0;
  add_match_count(found, n_matches);
}

}  // namespace nos

// The two kernels of the voxel-indexed match against the store.  Not templates, so every unit that sees
// the definitions compiles a copy: nos_voxelmap.hip, the one unit that launches them, asks for them.
#ifdef NOS_WITH_VOXEL_INDEX_KERNELS
namespace {
// voxel_match_kernel emitting store slots instead of records: what match_index_kernel is to match_kernel.
__global__ __launch_bounds__(256) void voxel_match_index_kernel(nos::VoxelMatchView map, const double* __restrict__ px,
                                                                const double* __restrict__ py, const double* __restrict__ pz,
                                                                uint64_t n_points, nos::PosePod pose, int max_neighbors,
                                                                int32_t* __restrict__ idx0, int32_t* __restrict__ idx1,
                                                                unsigned long long* __restrict__ n_matches,
                                                                unsigned int* __restrict__ error) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  const int found = i < n_points ? nos::match_point_ids<false>(map, px, py, pz, i, pose, max_neighbors, idx0, idx1, error) : 0;
  nos::add_match_count(found, n_matches);
}

// ids[i] (a store slot, or -1 which stays) → its rank in `rows`, the ascending list of the *n_rows distinct values of
// ids (0xFFFFFFFF, the key of -1, last when present): a binary search in a list the size of the scan's footprint, which
// stays in L2.  Every id is in the list.
__global__ __launch_bounds__(256) void voxel_rank_ids_kernel(int32_t* __restrict__ ids, uint64_t n_ids,
                                                             const uint32_t* __restrict__ rows,
                                                             const uint32_t* __restrict__ n_rows) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n_ids) return;
  const int32_t id = ids[i];
  if (id < 0) return;
  uint32_t lo = 0, hi = *n_rows;  // first position with rows[pos] >= id
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (rows[mid] < uint32_t(id)) lo = mid + 1;
    else hi = mid;
  }
  ids[i] = int32_t(lo);
}
}  // namespace
#endif
