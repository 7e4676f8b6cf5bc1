// pgo_host.hpp — host side of the pose-graph solver below its entry points (nos_pgo.hip): the graph's device state and its
// upload, one helper per launch sequence, the coarse level and the PCG loops.  Layout builder: pgo_layout.hpp (no HIP);
// kernels: pgo_kernels.hpp, pgo_coarse_kernels.hpp.
#pragma once

#include "nos_internal.hpp"

#include "pgo_kernels.hpp"
#include "pgo_coarse_kernels.hpp"

struct nos_pose_graph {
  nos_ctx* ctx = nullptr;
  uint32_t n_poses = 0, n_edges = 0;
  size_t n_unknowns = 0;  // 6 n_poses + n_edges
  uint32_t n_free_switches = 0;
  // every device and pinned allocation of the graph, recorded by pgo_alloc; nos_pgo_destroy frees this list and nothing else
  struct Owned {
    void* ptr;
    bool pinned;
  };
  std::vector<Owned> owned;
  // graph (gathered data as 64-byte records, see pgo_kernels.hpp)
  double* d_pose = nullptr;       // [n_poses][8]: px py pz qw qx qy qz pad
  int32_t *d_ref = nullptr, *d_qry = nullptr;
  double* d_edge = nullptr;       // [n_edges][8]: t_m (3) q_m wxyz (4) switch (1)
  double* d_info = nullptr;       // [n_edges][24]: Omega' = D Omega D, 21 upper entries + 3 pads (nos_pgo_create_weighted); NULL: unweighted
  // robust loss (nos_pgo_set_loss): `loss` is what the NEXT linearisation will apply; `lin_robust` says whether the last one
  // applied one, that is, whether entries 21 / 22 of the Omega' records hold its w / rho and the robust sweeps are to run
  nos_loss loss{NOS_LOSS_NONE, 0, 0.0, 0.0};
  uint8_t* d_robust = nullptr;    // [n_edges] flags of the constraints the loss applies to (allocated at the first call with flags)
  bool robust_flags = false;      // d_robust is in force (false: the loss applies to every constraint)
  bool lin_robust = false;
  uint8_t *d_sw_free = nullptr, *d_fixed = nullptr;
  uint32_t *d_adj_off = nullptr, *d_adj = nullptr, *d_adj_nbr = nullptr;
  // linear system
  double *d_hdiag = nullptr, *d_minv = nullptr;  // 21 planes each
  double* d_hs = nullptr;                         // switch curvature
  double *d_grad = nullptr, *d_x = nullptr, *d_r = nullptr, *d_z = nullptr, *d_p = nullptr, *d_ap = nullptr;
  double* d_p2 = nullptr;  // second direction buffer: the block-local product writes p_new = z + beta p while it reads p
  double *d_partials = nullptr, *d_scalars = nullptr;
  unsigned int* d_tickets = nullptr;  // [2] arrival counters of the in-launch tails (product, preconditioner); zero between launches
  double* h_scalars = nullptr;  // pinned [8]
  uint32_t partial_blocks = 0;
  nos::PgoView view{};
  // block-local product (pgo_matvec_block_kernel): per-block entry lists; block_poses = 0 → owner-computes kernels
  double* d_bent = nullptr;        // [n_entries][10]
  uint32_t* d_bent_off = nullptr;  // [n_blocks + 1]
  uint32_t* d_bent_edge = nullptr; // [n_entries] constraint of every entry (switch refresh after a retract)
  uint32_t* d_bhalo = nullptr;     // halo pose ids, block after block
  uint32_t* d_bhalo_off = nullptr; // [n_blocks + 1]
  uint32_t block_poses = 0, n_blocks = 0, n_entries = 0;
  size_t n_halo = 0;               // halo poses over all blocks
  int product_grid = 0;            // workgroups of the block-local product (what is resident), decided at the first launch
  nos::PgoBlockView bview{};
  // coarse level of the two-level preconditioner (pgo_coarse_kernels.hpp), allocated on first use
  uint32_t agg = 0, n_agg = 0, pcr_levels = 0;
  size_t pcr_pitch = 0;  // elements between two planes of the PCR factors (see PcrLevelLayout)
  double* d_coarse = nullptr;  // one allocation: L/D/U x 2, Dinv, alpha/gamma per level, rhs x 2
  double *c_L[2] = {nullptr, nullptr}, *c_D[2] = {nullptr, nullptr}, *c_U[2] = {nullptr, nullptr};
  double *c_Dinv = nullptr, *c_alpha = nullptr, *c_gamma = nullptr, *c_b[2] = {nullptr, nullptr};
};

namespace nosd {

constexpr uint32_t kPgoDotBlocks = 1024;

// ---- ownership and upload

// `count` elements (at least one) of device or pinned memory, owned by the graph.
template <class T>
hipError_t pgo_alloc(nos_pose_graph* pg, T** out, size_t count, bool pinned = false) {
  const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  void* p = nullptr;
  const hipError_t e = pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : device_alloc(pg->ctx->slots[0], &p, bytes);
  if (e != hipSuccess) return e;
  pg->owned.push_back({p, pinned});
  *out = static_cast<T*>(p);
  return hipSuccess;
}

inline void pgo_free_one(const nos_pose_graph::Owned& o) { (void)(o.pinned ? hipHostFree(o.ptr) : hipFree(o.ptr)); }

// Gives one buffer back before the graph goes (the coarse level when the aggregate size changes).
inline void pgo_release(nos_pose_graph* pg, void* ptr) {
  for (size_t k = 0; k < pg->owned.size(); ++k)
    if (pg->owned[k].ptr == ptr) {
      pgo_free_one(pg->owned[k]);
      pg->owned.erase(pg->owned.begin() + k);
      return;
    }
}

template <class T>
hipError_t pgo_upload(nos_pose_graph* pg, T** out, const T* host, size_t count) {
  const hipError_t e = pgo_alloc(pg, out, count);
  if (e != hipSuccess || count == 0) return e;
  return hipMemcpy(*out, host, count * sizeof(T), hipMemcpyHostToDevice);
}
template <class T>
hipError_t pgo_upload(nos_pose_graph* pg, T** out, const std::vector<T>& host) {
  return pgo_upload(pg, out, host.data(), host.size());
}

// ---- information matrices (nos_pgo_create_weighted)

// Eigenvalues of a symmetric 6x6 by cyclic Jacobi rotations (host; a dozen sweeps reach float64 rounding).  The matrix is
// divided by its largest |entry| first and the eigenvalues scaled back: the convergence test squares entries, and those of
// a finite matrix above 1e154 would overflow it (the loop would leave at once and hand back the diagonal).
inline void pgo_sym6_eigenvalues(const double A_in[36], double ev[6]) {
  double A[6][6], top = 0.0;
  for (int k = 0; k < 36; ++k) top = std::max(top, std::fabs(A_in[k]));
  if (!(top > 0.0)) {
    for (int a = 0; a < 6; ++a) ev[a] = 0.0;
    return;
  }
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) A[a][b] = A_in[6 * a + b] / top;
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) (a == b ? diag : off) += A[a][b] * A[a][b];
    if (!(off > 1e-40 * diag)) break;
    for (int p = 0; p < 5; ++p)
      for (int q = p + 1; q < 6; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 6; ++k) {  // columns p, q
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {  // rows p, q
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
      }
  }
  for (int a = 0; a < 6; ++a) ev[a] = A[a][a] * top;
}

// information: [n_edges][21] upper triangles, row-major.  → -1 when every matrix is finite, not zero and positive
// semi-definite (smallest eigenvalue >= -1e-12 x the largest), else the index of the first constraint that is not;
// packed: [n_edges][24] records of Omega' = D Omega D, D = diag(I, -I) (pgo_kernels.hpp), pads zero.
inline long long pgo_pack_information(size_t n_edges, const double* information, std::vector<double>* packed) {
  packed->assign(n_edges * 24, 0.0);
  for (size_t e = 0; e < n_edges; ++e) {
    const double* u = information + 21 * e;
    double A[36], ev[6];
    bool finite = true, zero = true;
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b, ++k) {
        finite = finite && std::isfinite(u[k]);
        zero = zero && u[k] == 0.0;
        A[6 * a + b] = A[6 * b + a] = u[k];
        (*packed)[24 * e + k] = (a < 3 && b >= 3) ? -u[k] : u[k];
      }
    if (!finite || zero) return (long long)e;
    pgo_sym6_eigenvalues(A, ev);
    const double lo = *std::min_element(ev, ev + 6), hi = *std::max_element(ev, ev + 6);
    if (!(hi > 0.0) || lo < -1e-12 * hi) return (long long)e;
  }
  return -1;
}

// LDS of the block-local product (pgo_matvec_block_kernel<128, 256>): 14 doubles per own and halo pose, 6 per slot.
// halo_cap / slot_cap are the capacities the kernel is launched with: the largest halo rounded up to 8, the largest slot
// count but at least 256 (the tail's sum re-uses the slots: >= 1024 doubles).
constexpr size_t kPgoLdsCap = size_t(160) * 1024;  // LDS of one CU: no workgroup gets more, whatever the runtime reports
constexpr uint32_t pgo_halo_cap(uint32_t largest_halo) { return (largest_halo + 7u) & ~7u; }
constexpr uint32_t pgo_slot_cap(uint32_t largest_slots) { return largest_slots > 256u ? largest_slots : 256u; }
constexpr size_t pgo_product_lds(uint32_t halo_cap, uint32_t slot_cap) {
  return ((size_t(128) + halo_cap) * 14 + size_t(slot_cap) * 6) * sizeof(double);
}

// The one place that names the instantiations of the block-local product.
using PgoProductKernel = decltype(&nos::pgo_matvec_block_kernel<128, 256, false>);
inline PgoProductKernel pgo_product_kernel(bool switch_rows) {
  return switch_rows ? nos::pgo_matvec_block_kernel<128, 256, true> : nos::pgo_matvec_block_kernel<128, 256, false>;
}

// The product keeps a block's poses, halo and slots in LDS: a graph that needs more than a workgroup may have goes to the
// owner-computes kernels like one beyond the packing limits.
inline bool pgo_blocks_fit_lds(const nos_ctx* ctx, const nos::PgoLayout& L) {
  int lds_max = 0;
  if (hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->slots[0].device) != hipSuccess)
    lds_max = 64 * 1024;
  const size_t budget = std::min<size_t>(size_t(std::max(lds_max, 0)), kPgoLdsCap);
  hipFuncAttributes fa{};  // the kernel's own static LDS (the tail's flag) counts against the same budget
  const void* kernel = reinterpret_cast<const void*>(pgo_product_kernel(L.n_free_switches > 0));
  const size_t fixed_lds = hipFuncGetAttributes(&fa, kernel) == hipSuccess ? fa.sharedSizeBytes : size_t(64);
  return pgo_product_lds(pgo_halo_cap(L.largest_halo), pgo_slot_cap(L.largest_slots)) + fixed_lds <= budget;
}

// The block lists of the layout: the pieces go to the device end to end (no host-side concatenation); one spare element
// behind the entry and halo lists: the product kernel's unconditional (clamped) loads of a block without entries or without
// a halo then stay inside the allocation.
inline hipError_t pgo_upload_blocks(nos_pose_graph* pg, const nos::PgoLayout& L) {
  const size_t n_ent = L.entry_off[L.n_blocks], n_halo = L.halo_off[L.n_blocks];
  hipError_t e = pgo_alloc(pg, &pg->d_bent, (n_ent + 1) * 10);
  if (e == hipSuccess) e = pgo_alloc(pg, &pg->d_bent_edge, n_ent);
  if (e == hipSuccess) e = pgo_alloc(pg, &pg->d_bhalo, n_halo + 1);
  if (e == hipSuccess) e = hipMemset(pg->d_bent + n_ent * 10, 0, 10 * sizeof(double));
  if (e == hipSuccess) e = hipMemset(pg->d_bhalo + n_halo, 0, sizeof(uint32_t));
  for (const nos::PgoLayoutPiece& pc : L.pieces) {
    const size_t eo = L.entry_off[pc.first_block], ho = L.halo_off[pc.first_block];
    if (e == hipSuccess && !pc.edge.empty()) {
      e = hipMemcpy(pg->d_bent + eo * 10, pc.ent.data(), pc.ent.size() * sizeof(double), hipMemcpyHostToDevice);
      if (e == hipSuccess)
        e = hipMemcpy(pg->d_bent_edge + eo, pc.edge.data(), pc.edge.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !pc.halo.empty())
      e = hipMemcpy(pg->d_bhalo + ho, pc.halo.data(), pc.halo.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_bent_off, L.entry_off);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_bhalo_off, L.halo_off);
  pg->block_poses = nos::kPgoBlockPoses;
  pg->n_blocks = L.n_blocks;
  pg->n_entries = uint32_t(n_ent);
  pg->n_halo = n_halo;
  return e;
}

// Everything a graph holds on the device, from its layout; `blocks`: with the lists of the block-local product.  Separate
// allocations in a fixed order: the kernels' speed has been measured with these addresses, not with an arena's.
inline hipError_t pgo_upload_graph(nos_pose_graph* pg, const nos::PgoLayout& L, const int32_t* ref, const int32_t* qry,
                                   bool blocks, const std::vector<double>* information = nullptr) {
  const uint32_t N = L.n_poses, M = L.n_edges;
  hipError_t e = hipSetDevice(pg->ctx->slots[0].device);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_pose, L.pose_rec);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_edge, L.edge_rec);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_adj_nbr, L.adj_nbr);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_sw_free, L.sw_free);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_fixed, L.fixed);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_adj_off, L.adj_off);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_adj, L.adj);
  if (e == hipSuccess && blocks) e = pgo_upload_blocks(pg, L);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_ref, ref, M);
  if (e == hipSuccess) e = pgo_upload(pg, &pg->d_qry, qry, M);
  if (e == hipSuccess && information != nullptr) e = pgo_upload(pg, &pg->d_info, *information);  // behind the unweighted graph's buffers
  auto zeroed = [&](double** p, size_t count) {
    if (e == hipSuccess) e = pgo_alloc(pg, p, count);
    if (e == hipSuccess) e = hipMemset(*p, 0, std::max<size_t>(count, 1) * sizeof(double));
  };
  zeroed(&pg->d_hdiag, size_t(21) * N);
  zeroed(&pg->d_minv, size_t(21) * N);
  zeroed(&pg->d_hs, M);
  for (double** v : {&pg->d_grad, &pg->d_x, &pg->d_r, &pg->d_z, &pg->d_p, &pg->d_ap, &pg->d_p2}) zeroed(v, pg->n_unknowns);
  zeroed(&pg->d_partials, size_t(2) * pg->partial_blocks);
  zeroed(&pg->d_scalars, 8);
  if (e == hipSuccess) e = pgo_alloc(pg, &pg->d_tickets, 4);
  if (e == hipSuccess) e = hipMemset(pg->d_tickets, 0, 16);
  if (e == hipSuccess) e = pgo_alloc(pg, &pg->h_scalars, 8, /*pinned=*/true);
  if (e != hipSuccess) return e;
  pg->view = nos::PgoView{pg->d_pose, pg->d_edge, pg->d_ref, pg->d_qry, pg->d_sw_free, pg->d_adj_off, pg->d_adj, pg->d_adj_nbr,
                          pg->d_fixed, N, M};
  pg->bview = nos::PgoBlockView{pg->d_bent, pg->d_bent_off, pg->d_bhalo, pg->d_bhalo_off, pg->n_blocks,
                                pgo_halo_cap(L.largest_halo), pgo_slot_cap(L.largest_slots)};
  return hipSuccess;
}

// ---- host vector order: the documented host order is 6 planes of n_poses then the switch rows; the device holds
// [n_poses][6] records then the switch rows

inline void to_records(const nos_pose_graph* pg, const double* planes, double* rec) {
  const size_t N = pg->n_poses;
  for (size_t i = 0; i < N; ++i)
    for (int k = 0; k < 6; ++k) rec[6 * i + k] = planes[size_t(k) * N + i];
  for (size_t e = 0; e < pg->n_edges; ++e) rec[6 * N + e] = planes[6 * N + e];
}
// switch_rows = false: the caller fills the switch rows (the device vector's took no part in what was computed)
inline void to_planes(const nos_pose_graph* pg, const double* rec, double* planes, bool switch_rows = true) {
  const size_t N = pg->n_poses;
  for (size_t i = 0; i < N; ++i)
    for (int k = 0; k < 6; ++k) planes[size_t(k) * N + i] = rec[6 * i + k];
  for (size_t e = 0; switch_rows && e < pg->n_edges; ++e) planes[6 * N + e] = rec[6 * N + e];
}

// ---- launch helpers

inline int pgo_read_scalars(nos_pose_graph* pg, int count, double* out) {
  DeviceSlot& slot = pg->ctx->slots[0];
  NOS_HIP_CHECK(hipMemcpyAsync(pg->h_scalars, pg->d_scalars, sizeof(double) * count, hipMemcpyDeviceToHost, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  for (int k = 0; k < count; ++k) out[k] = pg->h_scalars[k];
  return NOS_OK;
}

inline void pgo_launch_sum_partials(nos_pose_graph* pg, uint32_t rows, int width) {
  hipLaunchKernelGGL(nos::pgo_sum_partials_kernel, dim3(1), dim3(1024), 0, pg->ctx->slots[0].stream, pg->d_partials, rows,
                     width, pg->d_scalars);
}

inline int pgo_dot(nos_pose_graph* pg, const double* a, const double* b, double* out) {
  DeviceSlot& slot = pg->ctx->slots[0];
  const uint32_t blocks = uint32_t(std::min<size_t>(kPgoDotBlocks, (pg->n_unknowns + 255) / 256));
  hipLaunchKernelGGL(nos::pgo_dot_kernel, dim3(blocks), dim3(256), 0, slot.stream, a, b, pg->n_unknowns, pg->d_partials);
  pgo_launch_sum_partials(pg, blocks, 1);
  NOS_HIP_CHECK(hipGetLastError());
  return pgo_read_scalars(pg, 1, out);
}

// Diagonal blocks, gradient, switch curvature and the block partials of the cost (one row per workgroup of the first launch).
inline void pgo_launch_linearize(nos_pose_graph* pg) {
  DeviceSlot& slot = pg->ctx->slots[0];
  if (pg->d_info != nullptr && pg->loss.kind != NOS_LOSS_NONE) {  // … under a robust loss: rho and w once, then the robust siblings
    pg->lin_robust = true;
    if (pg->n_edges > 0)
      hipLaunchKernelGGL(nos::pgo_robust_weights_kernel, dim3((pg->n_edges + 255) / 256), dim3(256), 0, slot.stream, pg->view,
                         pg->d_info, pg->loss, pg->robust_flags ? pg->d_robust : static_cast<const uint8_t*>(nullptr));
    hipLaunchKernelGGL(nos::pgo_linearize_robust_kernel, dim3((pg->n_poses + 255) / 256), dim3(256), 0, slot.stream, pg->view,
                       pg->d_info, pg->d_hdiag, pg->d_grad, pg->d_partials);
    if (pg->n_edges > 0)
      hipLaunchKernelGGL(nos::pgo_switch_linearize_robust_kernel, dim3((pg->n_edges + 255) / 256), dim3(256), 0, slot.stream,
                         pg->view, pg->d_info, pg->d_grad + size_t(6) * pg->n_poses, pg->d_hs);
    return;
  }
  pg->lin_robust = false;
  if (pg->d_info != nullptr) {  // constraints with information: the weighted siblings
    hipLaunchKernelGGL(nos::pgo_linearize_weighted_kernel, dim3((pg->n_poses + 255) / 256), dim3(256), 0, slot.stream, pg->view,
                       pg->d_info, pg->d_hdiag, pg->d_grad, pg->d_partials);
    if (pg->n_edges > 0)
      hipLaunchKernelGGL(nos::pgo_switch_linearize_weighted_kernel, dim3((pg->n_edges + 255) / 256), dim3(256), 0, slot.stream,
                         pg->view, pg->d_info, pg->d_grad + size_t(6) * pg->n_poses, pg->d_hs);
    return;
  }
  hipLaunchKernelGGL(nos::pgo_linearize_kernel, dim3((pg->n_poses + 255) / 256), dim3(256), 0, slot.stream, pg->view,
                     pg->d_hdiag, pg->d_grad, pg->d_partials);
  if (pg->n_edges > 0)
    hipLaunchKernelGGL(nos::pgo_switch_linearize_kernel, dim3((pg->n_edges + 255) / 256), dim3(256), 0, slot.stream,
                       pg->view, pg->d_grad + size_t(6) * pg->n_poses, pg->d_hs);
}

// The product of a PCG iteration with its in-launch tail (p.Ap, alpha): block-local form when the graph has its entry lists.
// z / x_new (block-local form only): the vector multiplied is x_new = z + beta x, formed in the same launch (see the kernel).
inline int pgo_launch_product(nos_pose_graph* pg, double lambda, const double* x, double* y, const double* z = nullptr,
                              double* x_new = nullptr) {
  DeviceSlot& slot = pg->ctx->slots[0];
  const nos::PgoTail tail{pg->d_partials, pg->d_tickets, pg->d_scalars};
  const int switch_rows = pg->n_free_switches > 0 ? 1 : 0;
  if (pg->block_poses != 0) {
    constexpr int kT = 256;
    const size_t lds = pgo_product_lds(pg->bview.halo_cap, pg->bview.slot_cap);
    const PgoProductKernel kernel = pgo_product_kernel(switch_rows != 0);
    // Per launch, not once at create: the attribute belongs to the KERNEL, not to the graph.  Two graphs alive at once need
    // different amounts, and set once at create the smaller graph's value would be in force when the larger one launches.
    if (lds > size_t(48) * 1024) {
      const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
      if (ea != hipSuccess) return fail(NOS_ERR_HIP, "pose-graph product: %zu bytes of LDS refused: %s", lds, hipGetErrorString(ea));
    }
    if (pg->product_grid == 0) {  // persistent workgroups: as many as are resident together
      int per_cu = 0;
      const hipError_t eo = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), kT, lds);
      if (eo != hipSuccess || per_cu < 1) per_cu = 1;
      pg->product_grid = int(std::min<size_t>(pg->n_blocks, size_t(per_cu) * size_t(slot.num_cus)));
    }
    hipLaunchKernelGGL(kernel, dim3(unsigned(pg->product_grid)), dim3(kT), lds, slot.stream, pg->view, pg->bview, pg->d_hdiag,
                       pg->d_hs, lambda, x, y, tail, z, x_new);
  } else {
    const uint32_t pose_blocks = (pg->n_poses + 255) / 256;
    const uint32_t mv_blocks = pose_blocks + (switch_rows ? (pg->n_edges + 255) / 256 : 0u);
    if (pg->d_info != nullptr && pg->lin_robust)  // the weights of the last linearisation, whatever nos_pgo_set_loss said since
      hipLaunchKernelGGL(nos::pgo_matvec_cg_robust_kernel, dim3(mv_blocks), dim3(256), 0, slot.stream, pg->view, pg->d_info,
                         pg->d_hdiag, pg->d_hs, lambda, x, y, pose_blocks, tail);
    else if (pg->d_info != nullptr)
      hipLaunchKernelGGL(nos::pgo_matvec_cg_weighted_kernel, dim3(mv_blocks), dim3(256), 0, slot.stream, pg->view, pg->d_info,
                         pg->d_hdiag, pg->d_hs, lambda, x, y, pose_blocks, tail);
    else
      hipLaunchKernelGGL(nos::pgo_matvec_cg_kernel, dim3(mv_blocks), dim3(256), 0, slot.stream, pg->view, pg->d_hdiag, pg->d_hs,
                       lambda, x, y, pose_blocks, tail);
  }
  NOS_HIP_CHECK(hipGetLastError());
  return NOS_OK;
}

// ---- coarse level (pgo_coarse_kernels.hpp)

// Rows of the largest residue class of PCR level `level`.
inline uint32_t pcr_rows(uint32_t n_agg, uint32_t level) { return uint32_t((uint64_t(n_agg) + (1ull << level) - 1) >> level); }

// The PCR levels run in spans of up to kPcrSpanLevels levels per launch (pgo_pcr_span_kernel); a span whose residue classes
// fit one workgroup takes all remaining levels.  → first level of the span that contains level l.
constexpr uint32_t kPcrSpanLevels = 4, kPcrSpanThreads = 128;
inline uint32_t pcr_span_start(uint32_t n_agg, uint32_t levels, uint32_t l) {
  uint32_t s = 0;
  for (;;) {
    if (pcr_rows(n_agg, s) <= kPcrSpanThreads) return s;  // the last span: levels [s, levels)
    const uint32_t k = std::min(kPcrSpanLevels, levels - s);
    if (l < s + k) return s;
    s += k;
  }
}
inline nos::PcrLevelLayout pcr_layout(uint32_t n_agg, uint32_t levels, uint32_t l) {
  const uint32_t shift = pcr_span_start(n_agg, levels, l);
  return nos::PcrLevelLayout{shift, pcr_rows(n_agg, shift)};
}

inline int pgo_coarse_alloc(nos_pose_graph* pg, uint32_t agg) {
  if (pg->d_coarse != nullptr && pg->agg == agg) return NOS_OK;
  if (pg->d_coarse != nullptr) {
    pgo_release(pg, pg->d_coarse);
    pg->d_coarse = nullptr;
  }
  pg->agg = agg;
  pg->n_agg = (pg->n_poses + agg - 1) / agg;
  pg->pcr_levels = 0;
  while ((1u << pg->pcr_levels) < pg->n_agg) ++pg->pcr_levels;
  const size_t blk = size_t(36) * pg->n_agg, vec = size_t(6) * pg->n_agg;
  pg->pcr_pitch = pg->n_agg;
  for (uint32_t l = 0; l < pg->pcr_levels; ++l) {
    const nos::PcrLevelLayout lay = pcr_layout(pg->n_agg, pg->pcr_levels, l);
    pg->pcr_pitch = std::max(pg->pcr_pitch, (size_t(1) << lay.shift) * lay.rows);
  }
  const size_t fac = size_t(std::max<uint32_t>(pg->pcr_levels, 1)) * 36 * pg->pcr_pitch;  // all levels' alpha (or gamma) planes
  NOS_HIP_CHECK(pgo_alloc(pg, &pg->d_coarse, 6 * blk + blk + 2 * fac + 2 * vec));
  double* p = pg->d_coarse;
  auto take = [&p](size_t count) {
    double* at = p;
    p += count;
    return at;
  };
  for (int k = 0; k < 2; ++k) {
    pg->c_L[k] = take(blk);
    pg->c_D[k] = take(blk);
    pg->c_U[k] = take(blk);
  }
  pg->c_Dinv = take(blk);
  pg->c_alpha = take(fac);
  pg->c_gamma = take(fac);
  pg->c_b[0] = take(vec);
  pg->c_b[1] = take(vec);
  return NOS_OK;
}

// A_c = P^T H' P (assembled directly; option pgo_coarse_probe: probed with 18 masked products), then the PCR elimination.
// The probing form uses d_p / d_ap as scratch: call before the CG vectors are initialised.
inline int pgo_coarse_setup(nos_pose_graph* pg, double lambda, uint32_t agg) {
  int rc = pgo_coarse_alloc(pg, agg);
  if (rc != NOS_OK) return rc;
  DeviceSlot& slot = pg->ctx->slots[0];
  const uint32_t N = pg->n_poses, C = pg->n_agg;
  const uint32_t pose_blocks = (N + 255) / 256, cblocks = (C + 127) / 128;
  const size_t N6 = size_t(6) * N;
  if (pg->ctx->settings.pgo_coarse_probe == 0 && pg->d_info == nullptr) {
    // the three block diagonals of A_c = P^T H' P, assembled directly: one sweep over the constraints each
    const dim3 grid((C + 3) / 4);
    hipLaunchKernelGGL(nos::pgo_coarse_assemble_kernel<0>, grid, dim3(256), 0, slot.stream, pg->view, pg->d_hdiag, lambda, agg, C,
                       pg->c_D[0]);
    hipLaunchKernelGGL(nos::pgo_coarse_assemble_kernel<1>, grid, dim3(256), 0, slot.stream, pg->view, pg->d_hdiag, lambda, agg, C,
                       pg->c_L[0]);
    hipLaunchKernelGGL(nos::pgo_coarse_assemble_kernel<2>, grid, dim3(256), 0, slot.stream, pg->view, pg->d_hdiag, lambda, agg, C,
                       pg->c_U[0]);
  } else {
    // round 2's way, kept for comparison (option pgo_coarse_probe) and the way of every graph with information (the
    // sigma / P / Q structure of the direct assembly does not survive a general Omega): A_c probed with 18 masked
    // matrix-free products
    NOS_HIP_CHECK(hipMemsetAsync(pg->c_L[0], 0, size_t(3) * 36 * C * sizeof(double), slot.stream));  // L, D, U of buffer 0
    NOS_HIP_CHECK(hipMemsetAsync(pg->d_p + N6, 0, size_t(pg->n_edges) * sizeof(double), slot.stream));  // switch part of the probe
    for (int colour = 0; colour < 3; ++colour)
      for (int dof = 0; dof < 6; ++dof) {
        hipLaunchKernelGGL(nos::pgo_coarse_probe_kernel, dim3(pose_blocks), dim3(256), 0, slot.stream, pg->view, agg, colour, dof,
                           pg->d_p);
        if (pg->d_info != nullptr && pg->lin_robust)  // the operator the solve multiplies by, or the preconditioner is another matrix's
          hipLaunchKernelGGL(nos::pgo_matvec_pose_robust_kernel, dim3(pose_blocks), dim3(256), 0, slot.stream, pg->view,
                             pg->d_info, pg->d_hdiag, lambda, pg->d_p, pg->d_p + N6, pg->d_ap, pg->d_partials, agg);
        else if (pg->d_info != nullptr)
          hipLaunchKernelGGL(nos::pgo_matvec_pose_weighted_kernel, dim3(pose_blocks), dim3(256), 0, slot.stream, pg->view,
                             pg->d_info, pg->d_hdiag, lambda, pg->d_p, pg->d_p + N6, pg->d_ap, pg->d_partials, agg);
        else
          hipLaunchKernelGGL(nos::pgo_matvec_pose_kernel, dim3(pose_blocks), dim3(256), 0, slot.stream, pg->view, pg->d_hdiag,
                             lambda, pg->d_p, pg->d_p + N6, pg->d_ap, pg->d_partials, agg);
        hipLaunchKernelGGL(nos::pgo_coarse_restrict_kernel, dim3((C + 3) / 4), dim3(256), 0, slot.stream, pg->view, agg, C,
                           pg->d_ap, pg->c_b[0]);
        hipLaunchKernelGGL(nos::pgo_coarse_scatter_kernel, dim3(cblocks), dim3(128), 0, slot.stream, C, colour, dof, pg->c_b[0],
                           pg->c_L[0], pg->c_D[0], pg->c_U[0]);
      }
  }
  hipLaunchKernelGGL(nos::pgo_coarse_symmetrize_kernel, dim3(cblocks), dim3(128), 0, slot.stream, C, pg->c_L[0], pg->c_D[0],
                     pg->c_U[0]);
  int cur = 0;
  for (uint32_t lvl = 0; lvl < pg->pcr_levels; ++lvl) {
    hipLaunchKernelGGL(nos::pgo_pcr_setup_kernel, dim3(cblocks), dim3(128), 0, slot.stream, C, 1u << lvl, pg->c_L[cur],
                       pg->c_D[cur], pg->c_U[cur], pg->c_L[1 - cur], pg->c_D[1 - cur], pg->c_U[1 - cur],
                       pg->c_alpha + size_t(lvl) * 36 * pg->pcr_pitch, pg->c_gamma + size_t(lvl) * 36 * pg->pcr_pitch,
                       pcr_layout(C, pg->pcr_levels, lvl), pg->pcr_pitch);
    cur = 1 - cur;
  }
  hipLaunchKernelGGL(nos::pgo_pcr_finish_kernel, dim3(cblocks), dim3(128), 0, slot.stream, C, pg->c_D[cur], pg->c_Dinv);
  NOS_HIP_CHECK(hipGetLastError());
  return NOS_OK;
}

// Right-hand side in c_b[0] → xc = A_c^-1 rhs; returns the buffer holding xc.  The ⌈log2 n_agg⌉ PCR levels run in
// spans (pcr_span_start): at 1 M poses / 20 834 aggregates three launches — levels 0-3 and 4-7 with halos (213 and 224
// workgroups of 128 rows), then levels 8-14 and the block solves inside one workgroup per residue class (256) — instead of 16.
inline int pgo_pcr_rhs(nos_pose_graph* pg, const double** xc) {
  DeviceSlot& slot = pg->ctx->slots[0];
  const uint32_t C = pg->n_agg, L = pg->pcr_levels;
  constexpr uint32_t kT = kPcrSpanThreads;
  int cur = 0;
  uint32_t l = 0;
  for (;;) {
    const uint32_t rows = pcr_rows(C, l);
    const double* a = pg->c_alpha;
    const double* g = pg->c_gamma;
    const nos::PcrLevelLayout lay{l, rows};
    if (rows <= kT) {  // the rest of the levels and the block solves, one workgroup per class
      hipLaunchKernelGGL(nos::pgo_pcr_span_kernel<kT>, dim3(1u << l), dim3(kT), 0, slot.stream, C, l, L, 0u, a, g,
                         pg->pcr_pitch, lay, pg->c_Dinv, pg->c_b[cur], pg->c_b[1 - cur]);
      cur = 1 - cur;
      break;
    }
    const uint32_t k = std::min(kPcrSpanLevels, L - l), halo = (1u << k) - 1u, per = kT - 2 * halo;
    const uint32_t chunks = (rows + per - 1) / per;
    hipLaunchKernelGGL(nos::pgo_pcr_span_kernel<kT>, dim3(chunks << l), dim3(kT), 0, slot.stream, C, l, l + k, halo, a, g,
                       pg->pcr_pitch, lay, static_cast<const double*>(nullptr), pg->c_b[cur], pg->c_b[1 - cur]);
    cur = 1 - cur;
    l += k;
  }
  NOS_HIP_CHECK(hipGetLastError());
  *xc = pg->c_b[cur];
  return NOS_OK;
}

// xc = A_c^-1 P^T r  →  returns the buffer holding xc.
inline int pgo_coarse_apply(nos_pose_graph* pg, const double* r, const double** xc) {
  DeviceSlot& slot = pg->ctx->slots[0];
  const uint32_t C = pg->n_agg;
  hipLaunchKernelGGL(nos::pgo_coarse_restrict_kernel, dim3((C + 3) / 4), dim3(256), 0, slot.stream, pg->view, pg->agg, C, r,
                     pg->c_b[0]);
  return pgo_pcr_rhs(pg, xc);
}

// ---- preconditioner

// The preconditioner of one solve at one lambda: what nos_pgo_solve and nos_pgo_precondition share.
struct PgoPrecond {
  uint32_t agg = 0;           // poses per aggregate of the coarse level
  bool two_level = false;     // coarse correction on top of block-Jacobi
  uint32_t active_edges = 0;  // switch rows that take part (0: no free switch, the rows stay identically zero)
  uint32_t pblocks = 0;       // workgroups of pgo_apply_precond_kernel = rows of its partials
};

// Block-Jacobi inverses and, from a few aggregates on, the coarse operator and its PCR factors.  The probing form of the
// coarse set-up uses d_p / d_ap as scratch: call before the CG vectors (or a test's r) are put in place.
inline int pgo_precond_setup(nos_pose_graph* pg, double lambda, PgoPrecond* pc) {
  DeviceSlot& slot = pg->ctx->slots[0];
  pc->active_edges = pg->n_free_switches > 0 ? pg->n_edges : 0;
  pc->pblocks = (pg->n_poses + pc->active_edges + 255) / 256;
  hipLaunchKernelGGL(nos::pgo_precond_kernel, dim3((pg->n_poses + 255) / 256), dim3(256), 0, slot.stream, pg->d_hdiag,
                     lambda, pg->n_poses, pg->d_minv);
  // two-level preconditioner: rigid-motion coarse space over aggregates of consecutive poses (pgo_coarse_kernels.hpp);
  // worth its set-up (18 products) from a few aggregates on
  pc->agg = uint32_t(std::max(2, pg->ctx->settings.pgo_agg));
  pc->two_level = pg->ctx->settings.pgo_precond != 0 && pg->n_poses >= 4 * pc->agg;
  if (pc->two_level) return pgo_coarse_setup(pg, lambda, pc->agg);
  return NOS_OK;
}

// d_z = M^-1 d_r (+ the coarse correction B xc), the block partials of r.z and r.r to d_partials; with a tail, the workgroup
// that finishes last sums them and computes beta.
inline void pgo_launch_precond(nos_pose_graph* pg, double lambda, const PgoPrecond& pc, const double* xc,
                               nos::PgoTail tail = nos::PgoTail{nullptr, nullptr, nullptr}) {
  const size_t N6 = size_t(6) * pg->n_poses;
  hipLaunchKernelGGL(nos::pgo_apply_precond_kernel, dim3(pc.pblocks), dim3(256), 0, pg->ctx->slots[0].stream, pg->d_minv,
                     pg->d_hs, lambda, pg->n_poses, pc.active_edges, pg->d_r, pg->d_r + N6, pg->d_z, pg->d_z + N6,
                     pg->d_partials, pg->d_pose, pg->d_fixed, xc, pc.agg, tail);
}

// d_z = M^-1 d_r, with the block partials of r.z and r.r in d_partials (host-read form: no in-launch tail).
inline int pgo_precond_apply(nos_pose_graph* pg, double lambda, const PgoPrecond& pc) {
  const double* xc = nullptr;
  if (pc.two_level) {
    const int rca = pgo_coarse_apply(pg, pg->d_r, &xc);
    if (rca != NOS_OK) return rca;
  }
  pgo_launch_precond(pg, lambda, pc, xc);
  return NOS_OK;
}

// ---- PCG: (H with its diagonal scaled by 1 + lambda) x = -gradient

struct PgoCg {
  nos_pose_graph* pg;
  double lambda;
  PgoPrecond pc;
  size_t n = 0;          // rows that take part: without free switches the switch rows of every CG vector stay zero
  unsigned vblocks = 0;  // workgroups of the vector kernels
  double rz = 0.0, rr = 0.0, b_norm = 0.0, res = 0.0;
  int it = 0;
};

// z = M^-1 r, then r.z and r.r to the host.
inline int pgo_cg_precond(PgoCg& s) {
  nos_pose_graph* pg = s.pg;
  int rc = pgo_precond_apply(pg, s.lambda, s.pc);
  if (rc != NOS_OK) return rc;
  pgo_launch_sum_partials(pg, s.pc.pblocks, 2);
  NOS_HIP_CHECK(hipGetLastError());
  double v[2];
  rc = pgo_read_scalars(pg, 2, v);
  s.rz = v[0];
  s.rr = v[1];
  return rc;
}

// Preconditioner set-up, x = 0, r = -g, z = M^-1 r, p = z.
inline int pgo_cg_start(PgoCg& s) {
  nos_pose_graph* pg = s.pg;
  DeviceSlot& slot = pg->ctx->slots[0];
  int rc = pgo_precond_setup(pg, s.lambda, &s.pc);
  if (rc != NOS_OK) return rc;
  s.n = size_t(6) * pg->n_poses + s.pc.active_edges;
  s.vblocks = unsigned((s.n + 255) / 256);
  NOS_HIP_CHECK(hipMemsetAsync(pg->d_x, 0, s.n * sizeof(double), slot.stream));
  NOS_HIP_CHECK(hipMemsetAsync(pg->d_r, 0, s.n * sizeof(double), slot.stream));
  hipLaunchKernelGGL(nos::pgo_cg_update_kernel, dim3(s.vblocks), dim3(256), 0, slot.stream, s.n, 1.0, pg->d_x, pg->d_grad,
                     pg->d_p /*scratch x: untouched since alpha*p with p = d_x = 0*/, pg->d_r);
  rc = pgo_cg_precond(s);
  if (rc != NOS_OK) return rc;
  s.res = s.b_norm = std::sqrt(s.rr);
  NOS_HIP_CHECK(hipMemcpyAsync(pg->d_p, pg->d_z, s.n * sizeof(double), hipMemcpyDeviceToDevice, slot.stream));
  return NOS_OK;
}

// CG scalars stay on the device (in-launch tails: pgo_cg_alpha / pgo_cg_beta); the host looks at |r| only every kCheck
// iterations, so up to kCheck - 1 iterations more than strictly needed may run (they only improve the step).
// One PCG iteration = 6 launches with the block-local product (direction update inside the product: p ping-pongs between two
// buffers), 7 with the owner-computes product, 4 / 5 without the coarse level: product (+ p.Ap, alpha) · update +
// restriction · PCR spans (2 at 1 M poses) · preconditioner (+ r.z, r.r, beta) [· direction].
inline int pgo_cg_device_scalars(PgoCg& s, int max_iterations, double rel_tolerance) {
  nos_pose_graph* pg = s.pg;
  DeviceSlot& slot = pg->ctx->slots[0];
  constexpr int kCheck = 8;
  const bool fuse_direction = pg->block_poses != 0;
  bool dir_flip = false;
  if (fuse_direction)  // the first product forms p = z + 0 * p_old: p_old must be finite
    NOS_HIP_CHECK(hipMemsetAsync(pg->d_p, 0, pg->n_unknowns * sizeof(double), slot.stream));
  const double init[8] = {0.0, 0.0, 0.0, s.rr, s.rz, 0.0, 0.0, 0.0};
  NOS_HIP_CHECK(hipMemcpyAsync(pg->d_scalars, init, sizeof init, hipMemcpyHostToDevice, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));  // `init` is a stack array
  const double stop = rel_tolerance * s.b_norm;
  const nos::PgoTail pc_tail{pg->d_partials, pg->d_tickets + 1, pg->d_scalars};
  while (s.it < max_iterations) {
    const int batch = std::min(kCheck, max_iterations - s.it);
    for (int k = 0; k < batch; ++k) {
      double* p_cur = pg->d_p;
      int rc;
      if (fuse_direction) {  // p_new = z + beta p_old (beta = 0 and p_old = 0 before the first product: p = z)
        double* p_old = dir_flip ? pg->d_p2 : pg->d_p;
        p_cur = dir_flip ? pg->d_p : pg->d_p2;
        rc = pgo_launch_product(pg, s.lambda, p_old, pg->d_ap, pg->d_z, p_cur);
        dir_flip = !dir_flip;
      } else {
        rc = pgo_launch_product(pg, s.lambda, pg->d_p, pg->d_ap);
      }
      if (rc != NOS_OK) return rc;
      const double* xc = nullptr;
      if (s.pc.two_level) {
        const uint32_t ur_blocks = (pg->n_agg + 3) / 4 + (s.pc.active_edges + 255) / 256;
        hipLaunchKernelGGL(nos::pgo_update_restrict_kernel, dim3(ur_blocks), dim3(256), 0, slot.stream, pg->view, s.pc.agg,
                           pg->n_agg, s.n, pg->d_scalars, p_cur, pg->d_ap, pg->d_x, pg->d_r, pg->c_b[0]);
        rc = pgo_pcr_rhs(pg, &xc);
        if (rc != NOS_OK) return rc;
      } else {
        hipLaunchKernelGGL(nos::pgo_cg_update_dev_kernel, dim3(s.vblocks), dim3(256), 0, slot.stream, s.n, pg->d_scalars,
                           p_cur, pg->d_ap, pg->d_x, pg->d_r);
      }
      pgo_launch_precond(pg, s.lambda, s.pc, xc, pc_tail);
      if (!fuse_direction)
        hipLaunchKernelGGL(nos::pgo_cg_direction_dev_kernel, dim3(s.vblocks), dim3(256), 0, slot.stream, s.n, pg->d_scalars,
                           pg->d_z, pg->d_p);
      NOS_HIP_CHECK(hipGetLastError());
    }
    s.it += batch;
    double sc[8];
    const int rc = pgo_read_scalars(pg, 8, sc);
    if (rc != NOS_OK) return rc;
    s.res = std::sqrt(sc[3]);
    if (sc[7] != 0.0 || !(s.res > stop)) break;  // breakdown, or converged (NaN also ends the loop)
  }
  return NOS_OK;
}

// CG scalars read by the host every iteration (option pgo_host_scalars): the same product kernel and the same in-launch sum
// as the device-resident form, p.Ap read back from the scalar block.
inline int pgo_cg_host_scalars(PgoCg& s, int max_iterations, double rel_tolerance) {
  nos_pose_graph* pg = s.pg;
  DeviceSlot& slot = pg->ctx->slots[0];
  for (; s.it < max_iterations; ++s.it) {
    double pap = 0.0;
    int rc = pgo_launch_product(pg, s.lambda, pg->d_p, pg->d_ap);
    if (rc == NOS_OK) rc = pgo_read_scalars(pg, 1, &pap);
    if (rc != NOS_OK) return rc;
    if (!(pap > 0.0) || !std::isfinite(pap)) break;  // breakdown: keep the current iterate
    const double alpha = s.rz / pap, rz_old = s.rz;
    hipLaunchKernelGGL(nos::pgo_cg_update_kernel, dim3(s.vblocks), dim3(256), 0, slot.stream, s.n, alpha, pg->d_p, pg->d_ap,
                       pg->d_x, pg->d_r);
    rc = pgo_cg_precond(s);
    if (rc != NOS_OK) return rc;
    s.res = std::sqrt(s.rr);
    if (s.res <= rel_tolerance * s.b_norm) {
      ++s.it;
      break;
    }
    const double beta = s.rz / rz_old;
    hipLaunchKernelGGL(nos::pgo_cg_direction_kernel, dim3(s.vblocks), dim3(256), 0, slot.stream, s.n, beta, pg->d_z, pg->d_p);
  }
  return NOS_OK;
}

}  // namespace nosd
