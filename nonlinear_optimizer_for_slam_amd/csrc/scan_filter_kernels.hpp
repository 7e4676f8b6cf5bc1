// scan_filter_kernels.hpp — voxel-grid filter of a device-resident scan: the first point of every cell, in stored order.
//
// Restates FilterPoints of the reference's test harness
// (nonlinear_optimizer/mahalanobis_distance_minimizer/tests/simple_optimization_test.cc:206-223): walk the points in
// index order, keep a point iff its voxel has not been seen yet.  "First occurrence per key" needs no sort:
//
//   claim   one lane per stored position: cell = floor(p * inv_res) (voxel_key_kernel's expression), packed with
//           pack_cell; the cell's entry in an open-addressing table of 64-bit keys is claimed by compare-and-swap and the
//           point's ORIGINAL index goes into that entry's `first` word by atomicMin.  The entry is remembered per
//           position (4 B) so nothing probes twice.  Lanes of a wave that hold the same cell in consecutive positions —
//           the usual case: neighbours in a scan are neighbours in space — combine their indices on chip first and send
//           one atomic per run.
//   select  keep[pos] = (first[entry[pos]] == original index of pos), compacted by one rocPRIM select (ScanFilterKeep).
//   gather  the kept positions' coordinates and original indices go to the new scan.
//
// Deterministic although the table is filled concurrently: which ENTRY a cell gets depends on arrival order, but no
// output depends on the entry — `first` is an integer minimum (order-independent), and the kept positions leave the
// select in ascending position order.  There are no floating-point atomics.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.hpp"

namespace nos {

constexpr uint32_t kFilterNoEntry = 0xFFFFFFFFu;

// words of the filter's device-side error block
enum ScanFilterWord {
  kFilterBadPoint = 0,    // 1 + original index of a point with a non-finite coordinate (atomicMax; 0 = none)
  kFilterFarPoint = 1,    // 1 + original index of a point whose cell lies outside +-2^20 (atomicMax; 0 = none)
  kFilterProbeError = 2,  // a probe loop ran through the whole table (cannot happen at load factor <= 1/2)
  kFilterWords = 4
};

// The entry of `key`, claimed if it is free.  Keys only ever go from kEmptyCell to a cell and stay: a plain load that sees
// the cell (however stale) is final, one that sees kEmptyCell is settled by the compare-and-swap.
__device__ __forceinline__ uint32_t scan_filter_claim(unsigned long long* __restrict__ tab_key, uint32_t table_mask, uint64_t key,
                                                      unsigned int* __restrict__ info) {
  uint32_t h = hash_cell(key) & table_mask;
  for (uint32_t probe = 0; probe <= table_mask; ++probe) {
    unsigned long long seen = tab_key[h];
    if (seen == kEmptyCell) seen = atomicCAS(&tab_key[h], (unsigned long long)kEmptyCell, (unsigned long long)key);
    if (seen == kEmptyCell || seen == key) return h;
    h = (h + 1) & table_mask;
  }
  atomicOr(&info[kFilterProbeError], 1u);
  return kFilterNoEntry;
}

// order == nullptr: the scan was never sorted nor filtered, a point's original index is its position.
__global__ __launch_bounds__(256) void scan_filter_claim_kernel(const double* __restrict__ px, const double* __restrict__ py,
                                                                const double* __restrict__ pz,
                                                                const uint32_t* __restrict__ order, uint32_t n, double inv_res,
                                                                unsigned long long* __restrict__ tab_key,
                                                                uint32_t* __restrict__ tab_first, uint32_t table_mask,
                                                                uint32_t* __restrict__ entry, unsigned int* __restrict__ info) {
  const uint32_t pos = blockIdx.x * 256 + threadIdx.x;  // n < 2^32 - 1 and the grid covers n: no wrap
  const bool live = pos < n;
  uint64_t key = kEmptyCell;  // lanes without a cell: beyond n, or a point that raises an error word
  uint32_t orig = 0xFFFFFFFFu;
  if (live) {
    const double x = px[pos], y = py[pos], z = pz[pos];
    orig = order != nullptr ? order[pos] : pos;
    const double c[3] = {floor(x * inv_res), floor(y * inv_res), floor(z * inv_res)};
    const double lim = double(1 << 20);
    bool inside = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) inside = inside && (c[k] >= -lim && c[k] < lim);  // a NaN fails both tests
    // x * inv_res can overflow for a finite x: the point itself decides "non-finite"
    const bool bad = !(fabs(x) <= 1.79e308 && fabs(y) <= 1.79e308 && fabs(z) <= 1.79e308);
    if (bad) atomicMax(&info[kFilterBadPoint], orig + 1u);
    else if (!inside) atomicMax(&info[kFilterFarPoint], orig + 1u);
    else key = pack_cell(int64_t(c[0]), int64_t(c[1]), int64_t(c[2]));
  }
  // runs of equal keys in consecutive lanes: a run's head is a lane whose left neighbour holds another key
  const int lane = int(threadIdx.x) & (kWave - 1);
  const uint32_t key_lo = uint32_t(key), key_hi = uint32_t(key >> 32);
  const uint32_t left_lo = uint32_t(__shfl_up(int(key_lo), 1, kWave)), left_hi = uint32_t(__shfl_up(int(key_hi), 1, kWave));
  const bool head = lane == 0 || left_lo != key_lo || left_hi != key_hi;
  const unsigned long long heads = __ballot(head);  // bit 0 is always set
  const int start = 63 - __builtin_clzll(heads & (~0ull >> (63 - lane)));                 // my run's first lane
  const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
  const int tail = after != 0ull ? lane + __builtin_ctzll(after) : kWave - 1;            // my run's last lane
  // inclusive min-scan inside the run: afterwards the tail holds the run's smallest original index
  uint32_t lowest = orig;
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t other = uint32_t(__shfl_up(int(lowest), d, kWave));
    if (lane - d >= start) lowest = min(lowest, other);
  }
  uint32_t mine = kFilterNoEntry;
  if (lane == tail && key != kEmptyCell) {
    mine = scan_filter_claim(tab_key, table_mask, key, info);
    if (mine != kFilterNoEntry) atomicMin(&tab_first[mine], lowest);
  }
  const uint32_t e = uint32_t(__shfl(int(mine), tail, kWave));
  if (live) entry[pos] = e;
}

// keep[pos] for rocPRIM's select over the positions 0 .. n-1
struct ScanFilterKeep {
  const uint32_t* tab_first;
  const uint32_t* entry;
  const uint32_t* order;  // or nullptr
  __device__ __forceinline__ bool operator()(const uint32_t& pos) const {
    const uint32_t e = entry[pos];
    return e != kFilterNoEntry && tab_first[e] == (order != nullptr ? order[pos] : pos);
  }
};

// the new scan: three planes of n_kept and, for every kept point, its original index
__global__ __launch_bounds__(256) void scan_filter_gather_kernel(const double* __restrict__ planes, uint32_t n,
                                                                 const uint32_t* __restrict__ order,
                                                                 const uint32_t* __restrict__ kept, uint32_t n_kept,
                                                                 double* __restrict__ out_planes, uint32_t* __restrict__ out_order) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n_kept) return;
  const uint32_t pos = kept[j];
  out_planes[j] = planes[pos];
  out_planes[size_t(n_kept) + j] = planes[size_t(n) + pos];
  out_planes[2 * size_t(n_kept) + j] = planes[2 * size_t(n) + pos];
  out_order[j] = order != nullptr ? order[pos] : pos;
}

}  // namespace nos
