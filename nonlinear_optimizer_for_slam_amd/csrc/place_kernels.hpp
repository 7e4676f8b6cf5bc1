// place_kernels.hpp — place recognition: the Scan Context descriptor of a device-resident scan and the exhaustive search
// of a database of stored descriptors, every stored place at every yaw.
//
// The rule (include/nos.h).  Descriptor: R rings x S sectors about the sensor; a point (x, y, z) counts
// when its coordinates are finite, z >= z_floor and r = sqrt(x x + y y) < max_range; ring i = min(floor(r (R /
// max_range)), R - 1); sector j = floor(a (S / 2 pi)) mod S with a = atan2(y, x) (+ 2 pi when negative), sector 0 for
// x == y == 0; a bin holds max(z) - z_floor, an empty bin 0.  Distance: with column norms |a_j| = sqrt(sum_i a[i][j]^2)
// and, per shift s, d_s = (1 / m) sum_j (1 - <q_j, c_(j+s)> / (|q_j| |c_(j+s)|)) over the m columns j (ascending) where
// both norms are > 0 (d_s = 1 when m == 0), the result is min_s d_s and the smallest s that attains it.
//
// How it is evaluated.
//   place_descriptor_kernel  one point per lane, grid-stride.  The maximum is taken on an ORDER-PRESERVING INTEGER KEY of
//       z (place_key: for finite doubles a < b <=> key(a) < key(b), key 0 = "no point"), first in the workgroup's LDS bins,
//       then — non-empty bins only — in a global key array, both with an integer atomic max.  An integer max does not
//       depend on arrival order, so the bits are the same from run to run and for every launch geometry (the argument
//       scan_filter_kernels.hpp makes for its atomicMin).  n_used is an integer sum.  No floating-point atomic anywhere.
//   place_finish_kernel      decodes the keys, subtracts z_floor ONCE per bin (the value is one rounding of a double the
//       scan contains), and writes a SLOT: the descriptor column by column (slot[j R + i], what the search reads
//       contiguously) followed by the S column norms, summed over the rings ascending.  The same kernel turns a host
//       descriptor (ring-major doubles) into a slot, so stored places and queries have one format and one set of norms.
//   place_search_kernel      one wave per workgroup, one candidate at a time in LDS (ring-major there: lane s reads
//       c[i][(j + s) mod S], consecutive lanes consecutive doubles, no bank conflict), kept across all queries.  Lane s
//       owns shift s (and s + 64 when S > 64): it walks j ascending and forms <q_j, c_(j+s)> over i ascending — every
//       entry of the S x S table of column dot products exactly once, S^2 R multiply-adds per pair, the table never
//       stored — so d_s is summed in the stated order by one lane.  A query column sits in one register across the wave and
//       ring i reaches every lane through v_readlane (no memory access in the inner loop but the LDS read);
//       four queries at a time share each read of the candidate (place_search_tile), the rest go one by one.
//       The minimum over the lanes is a butterfly on (d, s), ties to the smaller s.  A pair's bits depend on the two
//       slots alone: not on the query count, the window, the grid or the database's capacity.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nos {

constexpr int kPlaceMaxRings = 64;
constexpr int kPlaceMaxSectors = 128;
constexpr int kPlaceSmallBins = 2048;                              // 16 KB of LDS: covers the default 20 x 60
constexpr int kPlaceMaxBins = kPlaceMaxRings * kPlaceMaxSectors;   // 64 KB of LDS
constexpr int kPlacePointsPerBlock = 4096;                         // a workgroup zeroes and flushes its bins once per this many points at least

// everything that is the same for all points; by value, so it lives in scalar registers
struct PlaceDev {
  int32_t n_rings, n_sectors;
  double max_range, z_floor;
  double ring_scale;    // n_rings / max_range
  double sector_scale;  // n_sectors / (2 pi)
  double two_pi;
};

// doubles of a slot: the descriptor column-major, then the column norms
__host__ __device__ inline size_t place_slot_doubles(int n_rings, int n_sectors) { return size_t(n_rings + 1) * size_t(n_sectors); }

// Order-preserving key of a finite double; 0 is no finite double's key (it would be the key of an all-ones NaN).
__device__ inline unsigned long long place_key(double z) {
  const unsigned long long u = static_cast<unsigned long long>(__double_as_longlong(z));
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline double place_unkey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double(static_cast<long long>(u));
}

__device__ inline bool place_finite(double v) { return fabs(v) < __builtin_huge_val(); }  // a NaN fails the test

// planes: [3][n] (stored order; the descriptor does not depend on it).  keys: [n_rings * n_sectors], zeroed by the caller.
template <int kBins>
__global__ __launch_bounds__(256) void place_descriptor_kernel(const double* __restrict__ planes, size_t n, PlaceDev P,
                                                               unsigned long long* __restrict__ keys,
                                                               unsigned long long* __restrict__ n_used) {
  __shared__ unsigned long long bins[kBins];
  const int n_bins = P.n_rings * P.n_sectors;  // <= kBins: the host picks the instantiation
  for (int b = threadIdx.x; b < n_bins; b += 256) bins[b] = 0ull;
  __syncthreads();
  unsigned int used = 0;
  const size_t step = size_t(gridDim.x) * 256;
  for (size_t p = size_t(blockIdx.x) * 256 + threadIdx.x; p < n; p += step) {
    const double x = planes[p], y = planes[n + p], z = planes[2 * n + p];
    if (!(place_finite(x) && place_finite(y) && place_finite(z))) continue;
    if (!(z >= P.z_floor)) continue;
    const double r = sqrt(x * x + y * y);
    if (!(r < P.max_range)) continue;
    int i = int(floor(r * P.ring_scale));
    i = i < P.n_rings - 1 ? i : P.n_rings - 1;
    int j = 0;
    if (!(x == 0.0 && y == 0.0)) {
      double a = atan2(y, x);
      if (a < 0.0) a += P.two_pi;
      j = int(floor(a * P.sector_scale));
      if (j >= P.n_sectors) j -= P.n_sectors;  // a rounded up to 2 pi
    }
    atomicMax(&bins[i * P.n_sectors + j], place_key(z));
    ++used;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < n_bins; b += 256) {
    const unsigned long long k = bins[b];
    if (k != 0ull) atomicMax(&keys[b], k);
  }
  for (int off = 32; off > 0; off >>= 1) used += __shfl_down(used, off, 64);
  if ((threadIdx.x & 63) == 0 && used != 0) atomicAdd(n_used, static_cast<unsigned long long>(used));
}

// Workgroup b builds slot b: from the keys (keys != nullptr; one descriptor) or from ring-major doubles src + b R S.
// One lane per column, rings ascending.
__global__ __launch_bounds__(128) void place_finish_kernel(const unsigned long long* __restrict__ keys,
                                                           const double* __restrict__ src, int n_rings, int n_sectors,
                                                           double z_floor, double* __restrict__ slots) {
  const int j = threadIdx.x;
  if (j >= n_sectors) return;
  const size_t cells = size_t(n_rings) * n_sectors;
  double* slot = slots + size_t(blockIdx.x) * place_slot_doubles(n_rings, n_sectors);
  double acc = 0.0;
  for (int i = 0; i < n_rings; ++i) {
    double v;
    if (keys != nullptr) {
      const unsigned long long k = keys[i * n_sectors + j];
      v = k != 0ull ? place_unkey(k) - z_floor : 0.0;
    } else {
      v = src[size_t(blockIdx.x) * cells + size_t(i) * n_sectors + j];
    }
    slot[size_t(j) * n_rings + i] = v;
    acc += v * v;
  }
  slot[cells + j] = sqrt(acc);
}

// Slot → ring-major doubles (what the public interface shows).
__global__ __launch_bounds__(128) void place_unslot_kernel(const double* __restrict__ slot, int n_rings, int n_sectors,
                                                           double* __restrict__ desc) {
  const int j = threadIdx.x;
  if (j >= n_sectors) return;
  for (int i = 0; i < n_rings; ++i) desc[size_t(i) * n_sectors + j] = slot[size_t(j) * n_rings + i];
}

constexpr int kPlaceQueryTile = 4;  // queries that share one pass over the candidate in LDS

// The double that lane `src` (wave-uniform, 0 … 63) holds in v, in every lane: two v_readlane_b32 into scalar registers.
__device__ inline double place_readlane(double v, int src) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
  const unsigned int lo = static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(b & 0xffffffffull), src));
  const unsigned int hi = static_cast<unsigned int>(__builtin_amdgcn_readlane(static_cast<int>(b >> 32), src));
  return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
}

// kQ queries (slots qs[0 … kQ-1]) against the candidate in c_lds (norms cn), every shift: lane s walks j ascending, i
// ascending.  A pair's arithmetic is the same sequence of operations for every kQ, so its bits do not depend on the tile.
template <int kShifts, int kQ>
__device__ inline void place_search_tile(const double* __restrict__ qs0, size_t stride, const double* c_lds,
                                         const double* __restrict__ cn, int R, int S, int lane, const int (&s)[kShifts],
                                         const bool (&live)[kShifts], double* __restrict__ distance_out,
                                         int32_t* __restrict__ shift_out, size_t out_stride) {
  // A query's column j lives in one register across the wave (lane i holds ring i; n_rings <= 64), loaded one column
  // ahead with one coalesced read; ring i's value reaches every lane through a scalar register (place_readlane).  The
  // query's column norms live the same way (lane l holds columns l and l + 64), the candidate's norm of the next column is
  // fetched one column ahead.  Nothing in the inner loop waits for memory but the LDS read of the candidate.
  const int cells = R * S;
  double sum[kQ][kShifts];
  int m[kQ][kShifts];
  int k[kShifts];
  double qn[kQ][kShifts];
  double qcol[kQ];
  double nc[kShifts];
#pragma unroll
  for (int h = 0; h < kShifts; ++h) {
    k[h] = s[h];  // (j + s) mod S at j = 0
    nc[h] = cn[k[h]];
#pragma unroll
    for (int t = 0; t < kQ; ++t) {
      sum[t][h] = 0.0;
      m[t][h] = 0;
      qn[t][h] = lane + 64 * h < S ? qs0[size_t(t) * stride + cells + lane + 64 * h] : 0.0;
    }
  }
#pragma unroll
  for (int t = 0; t < kQ; ++t) qcol[t] = lane < R ? qs0[size_t(t) * stride + lane] : 0.0;
  for (int j = 0; j < S; ++j) {
    // the next column's operands (the last column fetches column 0 again: in bounds, unused)
    const int jn = j + 1 == S ? 0 : j + 1;
    int kn[kShifts];
    double nc_next[kShifts], qcol_next[kQ];
#pragma unroll
    for (int h = 0; h < kShifts; ++h) {
      kn[h] = k[h] + 1 == S ? 0 : k[h] + 1;
      nc_next[h] = cn[kn[h]];
    }
#pragma unroll
    for (int t = 0; t < kQ; ++t) qcol_next[t] = lane < R ? qs0[size_t(t) * stride + size_t(jn) * R + lane] : 0.0;
    double dot[kQ][kShifts];
#pragma unroll
    for (int t = 0; t < kQ; ++t)
#pragma unroll
      for (int h = 0; h < kShifts; ++h) dot[t][h] = 0.0;
    for (int i = 0; i < R; ++i) {
      double cv[kShifts];
#pragma unroll
      for (int h = 0; h < kShifts; ++h) cv[h] = c_lds[i * S + k[h]];
#pragma unroll
      for (int t = 0; t < kQ; ++t) {
        const double qv = place_readlane(qcol[t], i);
#pragma unroll
        for (int h = 0; h < kShifts; ++h) dot[t][h] = fma(qv, cv[h], dot[t][h]);
      }
    }
#pragma unroll
    for (int t = 0; t < kQ; ++t) {
      const double nq = place_readlane(kShifts > 1 && j >= 64 ? qn[t][kShifts - 1] : qn[t][0], j & 63);
#pragma unroll
      for (int h = 0; h < kShifts; ++h) {
        if (nq > 0.0 && nc[h] > 0.0) {
          sum[t][h] += 1.0 - dot[t][h] / (nq * nc[h]);
          ++m[t][h];
        }
      }
      qcol[t] = qcol_next[t];
    }
#pragma unroll
    for (int h = 0; h < kShifts; ++h) {
      k[h] = kn[h];
      nc[h] = nc_next[h];
    }
  }
#pragma unroll
  for (int t = 0; t < kQ; ++t) {
    double best = __builtin_huge_val();
    int best_s = lane == 0 ? 0 : 0x7fffffff;  // lane 0 owns shift 0: a NaN distance still leaves a shift in range
#pragma unroll
    for (int h = 0; h < kShifts; ++h) {
      const double d = m[t][h] > 0 ? sum[t][h] / double(m[t][h]) : 1.0;
      if (live[h] && (d < best || (d == best && s[h] < best_s))) {
        best = d;
        best_s = s[h];
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(best, off, 64);
      const int os = __shfl_xor(best_s, off, 64);
      if (od < best || (od == best && os < best_s)) {
        best = od;
        best_s = os;
      }
    }
    if (lane == 0) {
      distance_out[size_t(t) * out_stride] = best;
      shift_out[size_t(t) * out_stride] = best_s;
    }
  }
}

// qslots: [n_queries] slots; slots: the database; candidates first … first + count - 1.  Dynamic LDS: n_rings * n_sectors
// doubles.  kShifts = 1 (n_sectors <= 64) or 2.  distance / shift: [n_queries][count].
template <int kShifts>
__global__ __launch_bounds__(64) void place_search_kernel(const double* __restrict__ qslots, int n_queries,
                                                          const double* __restrict__ slots, size_t first, size_t count,
                                                          int n_rings, int n_sectors, double* __restrict__ distance,
                                                          int32_t* __restrict__ shift) {
  extern __shared__ double c_lds[];  // [n_rings][n_sectors]
  const int lane = threadIdx.x;
  const int R = n_rings, S = n_sectors;
  const int cells = R * S;
  const size_t stride = place_slot_doubles(R, S);
  int s[kShifts];
  bool live[kShifts];
#pragma unroll
  for (int h = 0; h < kShifts; ++h) {
    live[h] = lane + 64 * h < S;
    s[h] = live[h] ? lane + 64 * h : 0;  // an idle lane computes shift 0 again and drops it
  }
  for (size_t ci = blockIdx.x; ci < count; ci += gridDim.x) {
    const double* __restrict__ c = slots + (first + ci) * stride;
    const double* __restrict__ cn = c + cells;
    __syncthreads();  // the previous candidate has been read
    for (int g = lane; g < cells; g += 64) {
      const int k = g / R, i = g - k * R;
      c_lds[i * S + k] = c[g];
    }
    __syncthreads();
    int q = 0;
    for (; q + kPlaceQueryTile <= n_queries; q += kPlaceQueryTile)
      place_search_tile<kShifts, kPlaceQueryTile>(qslots + size_t(q) * stride, stride, c_lds, cn, R, S, lane, s, live,
                                                  distance + size_t(q) * count + ci, shift + size_t(q) * count + ci, count);
    for (; q < n_queries; ++q)
      place_search_tile<kShifts, 1>(qslots + size_t(q) * stride, stride, c_lds, cn, R, S, lane, s, live,
                                    distance + size_t(q) * count + ci, shift + size_t(q) * count + ci, count);
  }
}

}  // namespace nos
