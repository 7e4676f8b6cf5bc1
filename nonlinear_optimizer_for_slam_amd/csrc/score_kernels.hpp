// score_kernels.hpp — how well does a scan fit the map at a pose: many (scan, pose) problems scored in one launch
// (nos_ndt_score_batch / nos_voxel_map_score_batch).
//
// From (map, scan, pose) straight to three numbers, nothing written in between: what nos_ndt_match / nos_voxel_map_match
// with dtype = NOS_F64 followed by nos_ndt6_accumulate gives — n_matches, the points with a match and the cost Σ ρ —
// without the 120-byte records, the 27 other sums and the two host waits.  Everything a term is made of exists once in
// the tree and is called here: warp_point and find_two_nearest (the search, for either view), sqrt_info_to_U (what the
// record writer stores next to S) and Ndt6Problem<double, LOSS>::item_U (e from the LOCAL point by the item's own
// multiply-add chain, r = U e, s, the loss).  A term is therefore the value the existing route adds to its acc[27], bit
// for bit; only the order of the sum is this file's own.
//
// The sum, fixed by the scan's point count alone: the points are cut into chunks of kScoreChunkPoints; one workgroup of
// kScoreBlock lanes takes one (problem, chunk) pair; lane l adds its points l, l + 256, … of the chunk in ascending order,
// slot 0 before slot 1; the wave butterfly and then waves 0 … 3 give the chunk's partial; score_finish_kernel adds a
// problem's partials in ascending chunk order.  No atomics on a double, no dependence on the batch around the problem.
#pragma once

#include "voxelmatch_kernels.hpp"

namespace nos {

constexpr int kScoreBlock = 256;
constexpr int kScoreChunkPoints = 1024;  // C: points per workgroup, four per lane

// One problem.  Workgroup first_block + c takes its chunk c and leaves partials[first_block + c].
struct ScoreDesc {
  const double* points;  // the scan: 3 planes of n_points doubles (nos_scan::d_planes)
  uint64_t n_points;
  double R[9], t[3];
  uint32_t first_block;
  uint32_t n_chunks;     // (n_points + C - 1) / C; 0 for an empty scan
};

struct ScoreLoss {
  double la, lb, lc;  // as Ndt6Params
};

// What one workgroup leaves behind (plain stores by one lane).
struct alignas(16) ScorePartial {
  double cost;
  uint32_t matches;
  uint32_t matched_points;
};

// The layout of nos_pose_score (include/nos.h).  Row 0 of a call's result block is a header: its `matches` carries the
// live store's probe-error word (0 for a snapshot); problem b is row 1 + b.
struct ScoreRow {
  uint64_t matches;
  uint64_t matched_points;
  double cost;
  double reserved;
};

// The term of one correspondence (local point p, voxel j of the view's arrays) added to acc[27]: the inputs the record
// writer stores for dtype f64 — mean[j], U = sqrt_info_to_U<double>(sqrt_info[j]) — through the item itself.  The other
// 27 sums of item_U are never read: the compiler drops them.
template <int LOSS>
__device__ __forceinline__ void score_term(const double* __restrict__ mean, const double* __restrict__ sqrt_info, uint32_t j,
                                           const double (&p)[3], const Ndt6Params<double>& P, double (&acc)[28]) {
  double mu[3], S[9], U[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) mu[k] = mean[3 * size_t(j) + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) S[k] = sqrt_info[9 * size_t(j) + k];
  sqrt_info_to_U<double>(S, U);
  Ndt6Problem<double, LOSS>::template item_U<double>(p, mu, U, P, acc);
}

// blocks: .x = problem, .y = chunk of the workgroup.  error: the live store's kInfoProbeError word (null for a snapshot).
template <typename View, int LOSS>
__global__ __launch_bounds__(kScoreBlock, 4) void score_batch_kernel(View map, unsigned int* __restrict__ error,
                                                                  const ScoreDesc* __restrict__ descs,
                                                                  const uint2* __restrict__ blocks, ScoreLoss loss,
                                                                  int max_neighbors, ScorePartial* __restrict__ partials) {
  constexpr int kWaves = kScoreBlock / kWave;
  __shared__ double s_cost[kWaves];
  __shared__ uint32_t s_matches[kWaves], s_points[kWaves];
  __shared__ uint32_t s_j[2][kScoreChunkPoints];  // the chunk's voxels, written and read back by the same lane
  const uint2 where = blocks[blockIdx.x];
  const ScoreDesc& d = descs[where.x];
  const uint64_t n = d.n_points;
  const double* const px = d.points;
  const double* const py = px + n;
  const double* const pz = py + n;
  const uint64_t begin = uint64_t(where.y) * kScoreChunkPoints;
  const uint32_t count = uint32_t(begin + kScoreChunkPoints < n ? kScoreChunkPoints : n - begin);
  // 1. the search, with voxel_match_kernel's registers: nothing of the cost is live across it
  {
    PosePod pose;
#pragma unroll
    for (int k = 0; k < 9; ++k) pose.R[k] = d.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pose.t[k] = d.t[k];
    for (uint32_t li = threadIdx.x; li < count; li += kScoreBlock) {
      const uint64_t i = begin + li;
      double q[3];
      warp_point(pose, px[i], py[i], pz[i], q[0], q[1], q[2]);
      TwoNearest best;
      find_two_nearest(map, q, best, error);
      s_j[0][li] = best.j[0];
      s_j[1][li] = max_neighbors > 1 ? best.j[1] : 0xFFFFFFFFu;
    }
  }
  // 2. the terms: this lane's points in ascending order, slot 0 before slot 1
  Ndt6Params<double> P;
#pragma unroll
  for (int k = 0; k < 9; ++k) P.R[k] = d.R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) P.t[k] = d.t[k];
  P.la = loss.la;
  P.lb = loss.lb;
  P.lc = loss.lc;
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  uint32_t matches = 0, points = 0;
  for (uint32_t li = threadIdx.x; li < count; li += kScoreBlock) {
    const uint64_t i = begin + li;
    const uint32_t j0 = s_j[0][li], j1 = s_j[1][li];
    const bool ok0 = j0 != 0xFFFFFFFFu, ok1 = j1 != 0xFFFFFFFFu;
    const double p[3] = {px[i], py[i], pz[i]};
    if (ok0) score_term<LOSS>(map.mean, map.sqrt_info, j0, p, P, acc);
    if (ok1) score_term<LOSS>(map.mean, map.sqrt_info, j1, p, P, acc);
    matches += uint32_t(ok0) + uint32_t(ok1);
    points += uint32_t(ok0);
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const double cost = wave_sum(acc[27]);
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    matches += __shfl_xor(matches, o, kWave);
    points += __shfl_xor(points, o, kWave);
  }
  if (lane == 0) {
    s_cost[wave] = cost;
    s_matches[wave] = matches;
    s_points[wave] = points;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScorePartial out;
    out.cost = 0.0;
    out.matches = out.matched_points = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      out.cost += s_cost[w];
      out.matches += s_matches[w];
      out.matched_points += s_points[w];
    }
    partials[blockIdx.x] = out;
  }
}

// One lane per problem: its chunk partials in ascending chunk order → row 1 + b; lane 0 of the grid also writes the header.
// Runs behind score_batch_kernel on the same stream, so every partial and the probe-error word are final.
__global__ __launch_bounds__(kScoreBlock) void score_finish_kernel(const ScoreDesc* __restrict__ descs, uint32_t n_problems,
                                                                   const ScorePartial* __restrict__ partials,
                                                                   const unsigned int* __restrict__ error,
                                                                   ScoreRow* __restrict__ rows) {
  const uint32_t b = blockIdx.x * kScoreBlock + threadIdx.x;
  if (b == 0) {
    ScoreRow h;
    h.matches = error != nullptr ? uint64_t(*error) : 0ull;
    h.matched_points = 0;
    h.cost = h.reserved = 0.0;
    rows[0] = h;
  }
  if (b >= n_problems) return;
  const uint32_t first = descs[b].first_block, n_chunks = descs[b].n_chunks;
  ScoreRow r;
  r.matches = r.matched_points = 0;
  r.cost = r.reserved = 0.0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const ScorePartial part = partials[first + c];
    r.cost += part.cost;
    r.matches += part.matches;
    r.matched_points += part.matched_points;
  }
  rows[1 + size_t(b)] = r;
}

}  // namespace nos
