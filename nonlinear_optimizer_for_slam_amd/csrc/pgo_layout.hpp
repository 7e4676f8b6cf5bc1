// pgo_layout.hpp — the layout of a pose graph as the device code reads it, built on the host.  Pure host code: no HIP header,
// compiles with a plain C++17 compiler (tests/host/pgo_layout_dump.cpp), so the list building can be tested and run under a
// sanitizer without a GPU.  nos_pgo_create uploads what build_pgo_layout makes (pgo_host.hpp); the kernels that read it are in
// pgo_kernels.hpp (PgoView, PgoBlockView).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

namespace nos {

// Block-local product: blocks of kPgoBlockPoses consecutive poses.  kPgoSlotLimit / kPgoHaloLimit are PACKING limits (16-bit
// slot and local-index fields of an entry), not the LDS budget: at both limits the product would ask for
// (128 + 512) x 112 B + 2304 x 48 B = 182 272 B, more than a CU has (160 KiB).  What a workgroup may have is asked of the
// device (pgo_product_lds against the budget, pgo_host.hpp); a trajectory graph needs ≈ 70 KB.
constexpr uint32_t kPgoBlockPoses = 128, kPgoSlotLimit = 2304, kPgoHaloLimit = 512;
constexpr uint32_t kPgoNoSlot = 0xFFFFu;  // slot field of an entry's end that lies outside the block

// What one host thread produced for its contiguous range of blocks [first_block, …): a contiguous piece of every list.
struct PgoLayoutPiece {
  uint32_t first_block = 0;
  std::vector<double> ent;           // [entries][10]
  std::vector<uint32_t> edge, halo;  // constraint of every entry; halo pose ids, block after block
};

struct PgoLayout {
  uint32_t n_poses = 0, n_edges = 0, n_free_switches = 0;
  size_t bad_constraint = 0;  // the first constraint with an invalid pose index, when build_pgo_layout returns false
  // gathered data as 64-byte records
  std::vector<double> pose_rec;  // [n_poses][8]: px py pz qw qx qy qz, fixed flag
  std::vector<double> edge_rec;  // [n_edges][8]: t_m (3), q_m wxyz (4), switch value
  std::vector<uint8_t> sw_free, fixed;
  // adjacency: constraints incident to pose i are adj[adj_off[i] .. adj_off[i+1]) in constraint order; entry = 2 * constraint
  // + role (0: the pose is the reference end, 1: the query end); adj_nbr holds the pose at the other end
  std::vector<uint32_t> adj_off, adj, adj_nbr;
  // block lists (blocks_fit only; empty otherwise).  The pieces stay pieces: they go to the device end to end, piece p at
  // entry_off[first_block] / halo_off[first_block] — at 1 M poses the entries are ≈ 370 MB, not worth a second host copy
  uint32_t n_blocks = 0;
  uint32_t largest_slots = 0;  // adjacency entries of the largest block (0 when no block lists were asked for)
  uint32_t largest_halo = 0;   // halo poses of the largest block (blocks_fit only)
  bool blocks_fit = false;     // block lists asked for, and every block within the packing limits
  std::vector<uint32_t> entry_off, halo_off;  // [n_blocks + 1]
  std::vector<PgoLayoutPiece> pieces;
};

// Host threads of the list building: min(16, hardware threads, blocks / 64), at least 1; max_threads != 0 replaces the first
// two terms.  The layout does not depend on the count.
inline unsigned pgo_layout_threads(uint32_t n_blocks, unsigned max_threads) {
  const unsigned cap = max_threads != 0 ? max_threads : std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  return std::min<unsigned>(cap, std::max(1u, n_blocks / 64u));
}

// Per block of kPgoBlockPoses consecutive poses, the constraints that touch it, in constraint order, each with the adjacency
// slots (positions relative to the block's first adjacency entry) of its ends inside the block and with its two poses as
// indices LOCAL to the block: < kPgoBlockPoses = own pose, else kPgoBlockPoses + position in the block's halo list (the other
// blocks' poses its constraints refer to, ascending).  ONE pass over the blocks, spread over a few host threads (blocks are
// independent; a thread takes a contiguous range of blocks, so what it produces is a contiguous piece of every list).
// Stops early, with blocks_fit = false, when a block exceeds the halo limit.
inline void pgo_build_block_lists(const int32_t* ref, const int32_t* qry, unsigned n_threads, PgoLayout* L) {
  const uint32_t N = L->n_poses, n_blocks = L->n_blocks;
  const std::vector<uint32_t>&adj_off = L->adj_off, &adj = L->adj, &adj_nbr = L->adj_nbr;
  const std::vector<double>& edge_rec = L->edge_rec;
  std::vector<uint32_t>&bent_off = L->entry_off, &bhalo_off = L->halo_off;
  std::vector<PgoLayoutPiece>& pieces = L->pieces;
  struct Ent {
    uint32_t e, slot_r, slot_q;
  };
  const uint32_t per = (n_blocks + n_threads - 1) / n_threads;
  pieces.resize(n_threads);
  std::atomic<bool> too_large{false};
  {
    std::vector<std::thread> pool;
    for (unsigned w = 0; w < n_threads; ++w)
      pool.emplace_back([&, w]() {
        const uint32_t b0 = std::min(n_blocks, w * per), b1 = std::min(n_blocks, b0 + per);
        PgoLayoutPiece& out = pieces[w];
        out.first_block = b0;
        std::vector<Ent> ents;
        std::vector<uint32_t> halo;
        for (uint32_t b = b0; b < b1 && !too_large.load(std::memory_order_relaxed); ++b) {
          const uint32_t lo = b * kPgoBlockPoses, hi = std::min(N, lo + kPgoBlockPoses), a0 = adj_off[lo];
          ents.clear();
          halo.clear();
          for (uint32_t a = a0; a < adj_off[hi]; ++a) {
            const uint32_t e = adj[a] >> 1, role = adj[a] & 1u;
            ents.push_back({e, role == 0 ? a - a0 : kPgoNoSlot, role == 0 ? kPgoNoSlot : a - a0});
            const uint32_t other = adj_nbr[a];
            if (other < lo || other >= hi) halo.push_back(other);
          }
          // constraint order; the two adjacency positions of a constraint with both ends in the block become one entry
          std::sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) { return x.e < y.e; });
          size_t n_out = 0;
          for (size_t k = 0; k < ents.size(); ++k) {
            if (n_out > 0 && ents[n_out - 1].e == ents[k].e) {
              if (ents[k].slot_r != kPgoNoSlot) ents[n_out - 1].slot_r = ents[k].slot_r;
              if (ents[k].slot_q != kPgoNoSlot) ents[n_out - 1].slot_q = ents[k].slot_q;
            } else {
              ents[n_out++] = ents[k];
            }
          }
          ents.resize(n_out);
          std::sort(halo.begin(), halo.end());
          halo.erase(std::unique(halo.begin(), halo.end()), halo.end());
          bent_off[b + 1] = uint32_t(ents.size());
          bhalo_off[b + 1] = uint32_t(halo.size());
          if (halo.size() > kPgoHaloLimit) too_large.store(true);
          auto local = [&](uint32_t pose) -> uint32_t {
            if (pose >= lo && pose < hi) return pose - lo;
            return kPgoBlockPoses + uint32_t(std::lower_bound(halo.begin(), halo.end(), pose) - halo.begin());
          };
          size_t k = out.edge.size();
          out.ent.resize(size_t(10) * (k + ents.size()));
          out.edge.resize(k + ents.size());
          for (const Ent& en : ents) {
            double* rec = out.ent.data() + size_t(10) * k;
            for (int q = 0; q < 8; ++q) rec[q] = edge_rec[size_t(8) * en.e + q];
            const unsigned long long w8 = (unsigned long long)en.e | ((unsigned long long)local(uint32_t(ref[en.e])) << 32) |
                                          ((unsigned long long)local(uint32_t(qry[en.e])) << 48);
            const unsigned long long w9 = (unsigned long long)en.slot_r | ((unsigned long long)en.slot_q << 16);
            memcpy(&rec[8], &w8, sizeof w8);
            memcpy(&rec[9], &w9, sizeof w9);
            out.edge[k++] = en.e;
          }
          out.halo.insert(out.halo.end(), halo.begin(), halo.end());
        }
      });
    for (std::thread& th : pool) th.join();
  }
  L->blocks_fit = !too_large.load();
}

// The layout of a graph from the arguments of nos_pgo_create (switch_init / switch_free / fixed may be NULL).  want_blocks:
// build the block lists of the block-local product (option pgo_block, and the graph has a constraint).  → false, with
// bad_constraint set, when a constraint names a pose that does not exist or the same pose twice.
inline bool build_pgo_layout(size_t n_poses, const double* poses, size_t n_edges, const int32_t* ref, const int32_t* qry,
                             const double* meas, const double* switch_init, const unsigned char* switch_free,
                             const unsigned char* fixed, bool want_blocks, PgoLayout* L, unsigned max_threads = 0) {
  *L = PgoLayout();
  for (size_t e = 0; e < n_edges; ++e)
    if (ref[e] < 0 || qry[e] < 0 || size_t(ref[e]) >= n_poses || size_t(qry[e]) >= n_poses || ref[e] == qry[e]) {
      L->bad_constraint = e;
      return false;
    }
  const uint32_t N = L->n_poses = uint32_t(n_poses), M = L->n_edges = uint32_t(n_edges);
  // 64-byte records + adjacency (once per graph)
  L->pose_rec.assign(size_t(8) * N, 0.0);
  L->edge_rec.assign(size_t(8) * std::max<uint32_t>(M, 1), 0.0);
  for (uint32_t i = 0; i < N; ++i) {
    for (int k = 0; k < 7; ++k) L->pose_rec[size_t(8) * i + k] = poses[size_t(7) * i + k];
    L->pose_rec[size_t(8) * i + 7] = (fixed && fixed[i]) ? 1.0 : 0.0;  // element 7 = "fixed" flag (block-local product)
  }
  L->sw_free.assign(std::max<uint32_t>(M, 1), 0);
  L->fixed.assign(N, 0);
  for (uint32_t e = 0; e < M; ++e) {
    for (int k = 0; k < 7; ++k) L->edge_rec[size_t(8) * e + k] = meas[size_t(7) * e + k];
    L->edge_rec[size_t(8) * e + 7] = switch_init ? switch_init[e] : 1.0;
    if (switch_free && switch_free[e]) {
      L->sw_free[e] = 1;
      ++L->n_free_switches;
    }
  }
  if (fixed)
    for (uint32_t i = 0; i < N; ++i) L->fixed[i] = fixed[i] ? 1 : 0;
  std::vector<uint32_t>&adj_off = L->adj_off, &adj = L->adj, &adj_nbr = L->adj_nbr;
  adj_off.assign(size_t(N) + 1, 0);
  adj.resize(std::max<size_t>(size_t(2) * M, 1));
  adj_nbr.resize(std::max<size_t>(size_t(2) * M, 1));
  for (uint32_t e = 0; e < M; ++e) {
    ++adj_off[size_t(ref[e]) + 1];
    ++adj_off[size_t(qry[e]) + 1];
  }
  for (uint32_t i = 0; i < N; ++i) adj_off[i + 1] += adj_off[i];
  {
    std::vector<uint32_t> cursor(adj_off.begin(), adj_off.end() - 1);
    for (uint32_t e = 0; e < M; ++e) {  // constraint order → deterministic accumulation order per pose
      adj_nbr[cursor[ref[e]]] = uint32_t(qry[e]);
      adj[cursor[ref[e]]++] = 2 * e;
      adj_nbr[cursor[qry[e]]] = uint32_t(ref[e]);
      adj[cursor[qry[e]]++] = 2 * e + 1;
    }
  }
  const uint32_t n_blocks = L->n_blocks = (N + kPgoBlockPoses - 1) / kPgoBlockPoses;
  if (!want_blocks) return true;
  for (uint32_t b = 0; b < n_blocks; ++b) {
    const uint32_t lo = b * kPgoBlockPoses, hi = std::min(N, lo + kPgoBlockPoses);
    L->largest_slots = std::max(L->largest_slots, adj_off[hi] - adj_off[lo]);
  }
  if (L->largest_slots > kPgoSlotLimit) return true;
  L->entry_off.assign(size_t(n_blocks) + 1, 0);
  L->halo_off.assign(size_t(n_blocks) + 1, 0);
  pgo_build_block_lists(ref, qry, pgo_layout_threads(n_blocks, max_threads), L);
  if (!L->blocks_fit) {  // how far each thread came before it saw the stop depends on timing: leave nothing of it behind
    L->entry_off.clear();
    L->halo_off.clear();
    L->pieces.clear();
    return true;
  }
  for (uint32_t b = 0; b < n_blocks; ++b) {
    L->largest_halo = std::max(L->largest_halo, L->halo_off[b + 1]);
    L->entry_off[b + 1] += L->entry_off[b];
    L->halo_off[b + 1] += L->halo_off[b];
  }
  return true;
}

}  // namespace nos
