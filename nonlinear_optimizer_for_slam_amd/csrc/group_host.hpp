// group_host.hpp — host side of grouping by key, as match_host.hpp is for matching: what the map build and
// the scan sort (nos_mapbuild.hip), the voxel store (voxel_store_host.hpp), the matcher's tables (nos_match.hip), the indexed
// dataset (nos_indexed.hip) and the scan filter (nos_scanfilter.hip) share.  No kernel lives here.
#pragma once

#include "nos_internal.hpp"

#include <rocprim/rocprim.hpp>

namespace nosd {

// A rocPRIM call is written ONCE, as a callable (void* tmp, size_t& bytes) → hipError_t, and its temporary kept here.
// Planning (prim_size, then prim_share or prim_plan: neither queues nor waits) is apart from queuing (prim_run).
struct PrimTmp {
  void* ptr = nullptr;
  size_t bytes = 0;
};
template <typename Call>
hipError_t prim_size(Call&& call, PrimTmp& t) {  // rocPRIM's size query: a null temporary
  return call(nullptr, t.bytes);
}
// one temporary from the arena for calls that run one after another on one stream: the largest of their sizes
inline hipError_t prim_share(DeviceBuffers& buf, std::initializer_list<PrimTmp*> ts) {
  size_t bytes = 16;
  for (const PrimTmp* t : ts) bytes = std::max(bytes, t->bytes);
  void* ptr = nullptr;
  const hipError_t e = buf.alloc_bytes(&ptr, bytes);
  for (PrimTmp* t : ts) t->ptr = ptr;
  return e;
}
template <typename Call>
hipError_t prim_plan(DeviceBuffers& buf, Call&& call, PrimTmp& t) {
  const hipError_t e = prim_size(call, t);
  return e == hipSuccess ? prim_share(buf, {&t}) : e;
}
template <typename Call>
hipError_t prim_run(Call&& call, PrimTmp t) {
  return call(t.ptr, t.bytes);
}

// n (key, index) pairs grouped by key.  arrays + temporaries plan (arena only; apart, because the build learns its key bits
// after a wait of its own); the caller fills keys[i], idx[i]; queue: stable radix sort over `bits` key bits (equal keys keep
// their index order), run-length encoding, the run count on its way to *h_runs.  It does NOT wait: the caller's wait also
// brings the caller's own words (the insert's bad / far flags, the tables' flags).  queue_offsets, after that wait: the
// exclusive scan of the counts over the runs there are.  A template so that only a unit that groups compiles its kernels.
template <typename Key>
struct KeyGroups {
  size_t n = 0;
  unsigned bits = 64;
  hipStream_t st = nullptr;
  Key *keys = nullptr, *keys_sorted = nullptr, *uniq = nullptr;       // as given, sorted, one per run
  uint32_t *idx = nullptr, *idx_sorted = nullptr;                     // as given, in key order
  uint32_t *counts = nullptr, *offsets = nullptr, *n_runs = nullptr;  // per run: length, first position; their number
  PrimTmp t_sort, t_rle, t_scan;

  // the three rocPRIM calls, each written once: size query with tmp = nullptr, queued otherwise
  hipError_t sort(void* tmp, size_t& b) { return rocprim::radix_sort_pairs(tmp, b, keys, keys_sorted, idx, idx_sorted, n, 0, bits, st); }
  hipError_t encode(void* tmp, size_t& b) { return rocprim::run_length_encode(tmp, b, keys_sorted, n, uniq, counts, n_runs, st); }
  hipError_t scan(void* tmp, size_t& b, size_t runs) {
    return rocprim::exclusive_scan(tmp, b, counts, offsets, 0u, runs, rocprim::plus<uint32_t>(), st);
  }
  // sorted_idx: where the indices in key order go when the caller keeps them (the map's d_orig_id); else the arena's
  hipError_t arrays(DeviceBuffers& buf, hipStream_t stream, size_t n_pairs, uint32_t* sorted_idx = nullptr) {
    n = n_pairs, st = stream, idx_sorted = sorted_idx;
    hipError_t e = buf.alloc(&keys, n);
    if (e == hipSuccess) e = buf.alloc(&keys_sorted, n);
    if (e == hipSuccess) e = buf.alloc(&uniq, n);
    if (e == hipSuccess) e = buf.alloc(&idx, n);
    if (e == hipSuccess && !idx_sorted) e = buf.alloc(&idx_sorted, n);
    if (e == hipSuccess) e = buf.alloc(&counts, n);
    if (e == hipSuccess) e = buf.alloc(&offsets, n);
    if (e == hipSuccess) e = buf.alloc(&n_runs, 1);
    return e;
  }
  hipError_t temporaries(DeviceBuffers& buf, unsigned key_bits) {
    bits = key_bits;
    if (n == 0) return hipSuccess;
    hipError_t e = sort(nullptr, t_sort.bytes);
    if (e == hipSuccess) e = encode(nullptr, t_rle.bytes);
    if (e == hipSuccess) e = scan(nullptr, t_scan.bytes, n);  // sized for the most runs there can be
    return e == hipSuccess ? prim_share(buf, {&t_sort, &t_rle, &t_scan}) : e;
  }
  hipError_t queue(uint32_t* h_runs) {
    hipError_t e = sort(t_sort.ptr, t_sort.bytes);
    if (e == hipSuccess) e = encode(t_rle.ptr, t_rle.bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(h_runs, n_runs, sizeof *h_runs, hipMemcpyDeviceToHost, st);
    return e;
  }
  hipError_t queue_offsets(uint32_t runs) { return runs > 0 ? scan(t_scan.ptr, t_scan.bytes, runs) : hipSuccess; }
};

// Voxel statistics from device arrays, queued on st: V means, sqrt-informations, valid flags and counts into `stats` (sized
// here, its cells too), V keys into h_keys.  The caller waits, then decodes the keys.
inline hipError_t download_stats(size_t V, const double* d_mean, const double* d_S, const unsigned char* d_valid,
                                 const uint32_t* d_count, const uint64_t* d_key, hipStream_t st, nos_map_stats* stats,
                                 std::vector<uint64_t>* h_keys) {
  h_keys->resize(V), stats->means.resize(V * 3), stats->sqrt_infos.resize(V * 9);
  stats->valid.resize(V), stats->counts.resize(V), stats->cells.resize(V * 3);
  if (V == 0) return hipSuccess;
  hipError_t e = hipMemcpyAsync(stats->means.data(), d_mean, V * 3 * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(stats->sqrt_infos.data(), d_S, V * 9 * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(stats->valid.data(), d_valid, V, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(stats->counts.data(), d_count, V * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(h_keys->data(), d_key, V * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
  return e;
}

// stats->cells from packed keys (pack_cell's form), after the wait that brought them
inline void cells_from_packed_keys(const std::vector<uint64_t>& h_keys, nos_map_stats* stats) {
  for (size_t v = 0; v < h_keys.size(); ++v) {
    int32_t c[3];
    nos::unpack_cell(h_keys[v], c);
    for (int k = 0; k < 3; ++k) stats->cells[3 * v + k] = c[k];
  }
}

}  // namespace nosd
