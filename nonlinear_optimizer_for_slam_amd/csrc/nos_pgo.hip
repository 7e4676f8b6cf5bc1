// nos_pgo.hip — the pose-graph entry points.  Layout builder: pgo_layout.hpp; device state, launch
// helpers, coarse level and PCG: pgo_host.hpp; kernels: pgo_kernels.hpp, pgo_coarse_kernels.hpp.
#include "pgo_host.hpp"

using namespace nosd;

extern "C" {

int nos_pgo_destroy(nos_pose_graph* pg) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg) return NOS_OK;
  for (const nos_pose_graph::Owned& o : pg->owned) pgo_free_one(o);
  delete pg;
  return NOS_OK;
}

// poses: [n_poses][7] = px py pz qw qx qy qz (PoseParameter, pose_graph_optimizer.h:16-19);
// meas:  [n_edges][7] = relative_pose_from_reference_to_query as t (3) + quaternion wxyz (types.h:13-19);
// switch_init / switch_free / fixed may be NULL (1.0 / none free / none fixed).
// Three steps: build the layout on the host, decide the product's form, upload.
int nos_pgo_create(nos_ctx* ctx, size_t n_poses, const double* poses, size_t n_edges, const int32_t* ref,
                   const int32_t* qry, const double* meas, const double* switch_init,
                   const unsigned char* switch_free, const unsigned char* fixed, nos_pose_graph** out_pg) {
  return nos_pgo_create_weighted(ctx, n_poses, poses, n_edges, ref, qry, meas, switch_init, switch_free, fixed, nullptr, out_pg);
}

// information: [n_edges][21], the upper triangle (row-major) of every constraint's 6x6 information matrix in the
// measurement frame (include/nos.h); NULL = nos_pgo_create.  A graph with information takes the two general paths: the
// owner-computes product (no block lists) and the probed coarse operator.  A matrix that is not finite, zero or not
// positive semi-definite is refused before any device work, with *out_pg as the caller left it.
int nos_pgo_create_weighted(nos_ctx* ctx, size_t n_poses, const double* poses, size_t n_edges, const int32_t* ref,
                            const int32_t* qry, const double* meas, const double* switch_init,
                            const unsigned char* switch_free, const unsigned char* fixed, const double* information,
                            nos_pose_graph** out_pg) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || !out_pg) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx / out_pg is NULL");
  const bool weighted = information != nullptr && n_edges > 0;
  std::vector<double> packed;
  if (weighted) {
    if (n_edges > 0x7FFFFFFFull) return fail(NOS_ERR_INVALID_ARGUMENT, "bad graph size");
    const long long bad = pgo_pack_information(n_edges, information, &packed);
    if (bad >= 0)
      return fail(NOS_ERR_INVALID_ARGUMENT, "the information matrix of constraint %lld is not finite, zero or not positive semi-definite", bad);
  }
  *out_pg = nullptr;
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "pose-graph optimisation needs a single-device context");
  if (n_poses == 0 || n_poses > 0x7FFFFFFFull || n_edges > 0x7FFFFFFFull) return fail(NOS_ERR_INVALID_ARGUMENT, "bad graph size");
  if (!poses || (n_edges > 0 && (!ref || !qry || !meas))) return fail(NOS_ERR_INVALID_ARGUMENT, "graph arrays are NULL");
  nos::PgoLayout L;
  const bool want_blocks = ctx->settings.pgo_block != 0 && n_edges > 0 && !weighted;
  if (!nos::build_pgo_layout(n_poses, poses, n_edges, ref, qry, meas, switch_init, switch_free, fixed, want_blocks, &L))
    return fail(NOS_ERR_INVALID_ARGUMENT, "constraint %zu has an invalid pose index", L.bad_constraint);  // "Constraint is invalid."
  // block-local product where the lists fit their packing and a workgroup's LDS; owner-computes kernels otherwise
  const bool blocks = !weighted && L.blocks_fit && pgo_blocks_fit_lds(ctx, L);
  nos_pose_graph* pg = new (std::nothrow) nos_pose_graph();
  if (!pg) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  pg->ctx = ctx;
  pg->n_poses = L.n_poses;
  pg->n_edges = L.n_edges;
  pg->n_unknowns = size_t(6) * L.n_poses + L.n_edges;
  pg->n_free_switches = L.n_free_switches;
  pg->partial_blocks = std::max<uint32_t>(kPgoDotBlocks, (L.n_poses + 255) / 256 + (L.n_edges + 255) / 256 + 2);
  const hipError_t e = pgo_upload_graph(pg, L, ref, qry, blocks, weighted ? &packed : nullptr);
  if (e != hipSuccess) {
    nos_pgo_destroy(pg);
    return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "pose-graph upload failed: %s", hipGetErrorString(e));
  }
  *out_pg = pg;
  return NOS_OK;
}

size_t nos_pgo_num_unknowns(const nos_pose_graph* pg) { return pg ? pg->n_unknowns : 0; }

// The robust loss the NEXT nos_pgo_linearize applies (include/nos.h states the rule).  Nothing is launched here: products,
// solves and preconditioner applications until then keep the weights of the last linearisation.  A refused call leaves
// the loss and the flags as they were.
int nos_pgo_set_loss(nos_pose_graph* pg, const nos_loss* loss, const unsigned char* robust) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg) return fail(NOS_ERR_INVALID_ARGUMENT, "pg is NULL");
  nos_loss want{NOS_LOSS_NONE, 0, 0.0, 0.0};
  if (loss != nullptr) {
    if (loss->kind == NOS_LOSS_HUBER) {
      if (!std::isfinite(loss->a) || !(loss->a > 0.0))
        return fail(NOS_ERR_INVALID_ARGUMENT, "pose-graph loss: the Huber threshold must be finite and > 0, got %g", loss->a);
      want = nos_loss{NOS_LOSS_HUBER, 0, loss->a, 0.0};
    } else if (loss->kind == NOS_LOSS_EXPONENTIAL) {
      if (!std::isfinite(loss->a) || !std::isfinite(loss->b) || loss->a < 0.0 || loss->b < 0.0)
        return fail(NOS_ERR_INVALID_ARGUMENT, "pose-graph loss: exponential c1, c2 must be finite and >= 0, got %g, %g", loss->a,
                    loss->b);
      want = nos_loss{NOS_LOSS_EXPONENTIAL, 0, loss->a, loss->b};
    } else if (loss->kind != NOS_LOSS_NONE) {
      return fail(NOS_ERR_INVALID_ARGUMENT, "pose-graph loss: unknown kind %d", int(loss->kind));
    }
  }
  if (want.kind == NOS_LOSS_NONE) {  // removing the loss is fine on any graph
    pg->loss = want;
    pg->robust_flags = false;
    return NOS_OK;
  }
  if (pg->d_info == nullptr)
    return fail(NOS_ERR_UNSUPPORTED,
                "a robust loss needs a pose graph with information: pass identity matrices to nos_pgo_create_weighted");
  if (robust != nullptr) {
    DeviceSlot& slot = pg->ctx->slots[0];
    NOS_HIP_CHECK(hipSetDevice(slot.device));
    if (pg->d_robust == nullptr) {
      const hipError_t e = pgo_alloc(pg, &pg->d_robust, pg->n_edges);
      if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "pose-graph loss flags: %s", hipGetErrorString(e));
    }
    NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));  // no weights kernel is reading the old flags
    NOS_HIP_CHECK(hipMemcpy(pg->d_robust, robust, pg->n_edges, hipMemcpyHostToDevice));
  }
  pg->robust_flags = robust != nullptr;
  pg->loss = want;
  return NOS_OK;
}

// Linearise at the current estimate: diagonal blocks, gradient, cost = sum of squared residuals,
// |gradient|_2.  Must precede nos_pgo_solve / nos_pgo_matvec.
int nos_pgo_linearize(nos_pose_graph* pg, double* cost, double* gradient_norm) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg) return fail(NOS_ERR_INVALID_ARGUMENT, "pg is NULL");
  NOS_HIP_CHECK(hipSetDevice(pg->ctx->slots[0].device));
  pgo_launch_linearize(pg);
  pgo_launch_sum_partials(pg, (pg->n_poses + 255) / 256, 1);
  NOS_HIP_CHECK(hipGetLastError());
  double c = 0.0, gg = 0.0;
  int rc = pgo_read_scalars(pg, 1, &c);
  if (rc != NOS_OK) return rc;
  rc = pgo_dot(pg, pg->d_grad, pg->d_grad, &gg);
  if (rc != NOS_OK) return rc;
  if (cost) *cost = c;
  if (gradient_norm) *gradient_norm = std::sqrt(gg);
  return NOS_OK;
}

// Solve (H with its diagonal scaled by 1 + lambda) step = -gradient by preconditioned CG (block-Jacobi, two-level from a few
// aggregates on).  Stops at |residual| <= rel_tolerance |gradient| or after max_iterations.
int nos_pgo_solve(nos_pose_graph* pg, double lambda, int max_iterations, double rel_tolerance, int* iterations,
                  double* rel_residual, double* step_norm) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg) return fail(NOS_ERR_INVALID_ARGUMENT, "pg is NULL");
  NOS_HIP_CHECK(hipSetDevice(pg->ctx->slots[0].device));
  PgoCg cg{pg, lambda};
  int rc = pgo_cg_start(cg);
  if (rc == NOS_OK && cg.b_norm > 0.0)
    rc = pg->ctx->settings.pgo_host_scalars == 0 ? pgo_cg_device_scalars(cg, max_iterations, rel_tolerance)
                                                 : pgo_cg_host_scalars(cg, max_iterations, rel_tolerance);
  if (rc != NOS_OK) return rc;
  double xx = 0.0;
  rc = pgo_dot(pg, pg->d_x, pg->d_x, &xx);
  if (rc != NOS_OK) return rc;
  if (iterations) *iterations = cg.it;
  if (rel_residual) *rel_residual = cg.b_norm > 0.0 ? cg.res / cg.b_norm : 0.0;
  if (step_norm) *step_norm = std::sqrt(xx);
  return NOS_OK;
}

// Apply the last computed step: p += dp, q = normalize(q (x) Exp(dw)), s += ds.
int nos_pgo_retract(nos_pose_graph* pg) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg) return fail(NOS_ERR_INVALID_ARGUMENT, "pg is NULL");
  DeviceSlot& slot = pg->ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  const uint32_t N = pg->n_poses;
  hipLaunchKernelGGL(nos::pgo_retract_kernel, dim3((N + pg->n_edges + 255) / 256), dim3(256), 0, slot.stream, N, pg->n_edges,
                     pg->d_fixed, pg->d_sw_free, pg->d_x, pg->d_x + size_t(6) * N, pg->d_pose, pg->d_edge);
  if (pg->block_poses != 0 && pg->n_free_switches > 0)  // the block entries carry their own copy of the constraint records
    hipLaunchKernelGGL(nos::pgo_refresh_entries_kernel, dim3((pg->n_entries + 255) / 256), dim3(256), 0, slot.stream,
                       pg->n_entries, pg->d_bent_edge, pg->d_edge, pg->d_bent);
  NOS_HIP_CHECK(hipGetLastError());
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  return NOS_OK;
}

int nos_pgo_get_state(nos_pose_graph* pg, double* poses, double* switches) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg) return fail(NOS_ERR_INVALID_ARGUMENT, "pg is NULL");
  const uint32_t N = pg->n_poses, M = pg->n_edges;
  NOS_HIP_CHECK(hipSetDevice(pg->ctx->slots[0].device));
  NOS_HIP_CHECK(hipStreamSynchronize(pg->ctx->slots[0].stream));
  if (poses) {
    std::vector<double> rec(size_t(8) * N);
    NOS_HIP_CHECK(hipMemcpy(rec.data(), pg->d_pose, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < N; ++i)
      for (int k = 0; k < 7; ++k) poses[size_t(7) * i + k] = rec[size_t(8) * i + k];
  }
  if (switches && M > 0) {
    std::vector<double> rec(size_t(8) * M);
    NOS_HIP_CHECK(hipMemcpy(rec.data(), pg->d_edge, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (uint32_t e = 0; e < M; ++e) switches[e] = rec[size_t(8) * e + 7];
  }
  return NOS_OK;
}

// Diagnostics for the parity tests: which = 0 gradient, 1 last step, 2 diagonal blocks (21 planes), 3 the robust weight
// of every constraint at the last linearisation (n_edges values; 1.0 where no loss applied).
int nos_pgo_get_vector(nos_pose_graph* pg, int which, double* out) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg || !out) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  NOS_HIP_CHECK(hipSetDevice(pg->ctx->slots[0].device));
  NOS_HIP_CHECK(hipStreamSynchronize(pg->ctx->slots[0].stream));
  if (which == 3) {
    const size_t M = pg->n_edges;
    if (pg->d_info == nullptr || !pg->lin_robust) {
      for (size_t e = 0; e < M; ++e) out[e] = 1.0;
      return NOS_OK;
    }
    // entry 21 of every 24-double record, a slab of records at a time
    constexpr size_t kSlab = 65536;
    std::vector<double> rec(std::min(M, kSlab) * 24);
    for (size_t e0 = 0; e0 < M; e0 += kSlab) {
      const size_t count = std::min(kSlab, M - e0);
      NOS_HIP_CHECK(hipMemcpy(rec.data(), pg->d_info + 24 * e0, count * 24 * sizeof(double), hipMemcpyDeviceToHost));
      for (size_t k = 0; k < count; ++k) out[e0 + k] = rec[24 * k + 21];
    }
    return NOS_OK;
  }
  const double* src = which == 0 ? pg->d_grad : which == 1 ? pg->d_x : pg->d_hdiag;
  if (which == 2) {
    NOS_HIP_CHECK(hipMemcpy(out, src, size_t(21) * pg->n_poses * sizeof(double), hipMemcpyDeviceToHost));
    return NOS_OK;
  }
  std::vector<double> rec(pg->n_unknowns);
  NOS_HIP_CHECK(hipMemcpy(rec.data(), src, rec.size() * sizeof(double), hipMemcpyDeviceToHost));
  to_planes(pg, rec.data(), out);
  return NOS_OK;
}

int nos_pgo_layout_info(const nos_pose_graph* pg, unsigned long long info[8]) {
  if (!pg || !info) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  const bool block = pg->block_poses != 0;
  info[0] = pg->n_poses, info[1] = pg->n_edges, info[2] = block ? pg->n_entries : 0, info[3] = block ? pg->block_poses : 0;
  info[4] = block ? pg->n_blocks : 0, info[5] = block ? pg->n_halo : 0, info[6] = pg->n_agg, info[7] = pg->pcr_levels;
  return NOS_OK;
}

// Timing aid: `repeats` sweeps back to back between one pair of events (bench.py; nothing else uses it).
int nos_pgo_time_sweep(nos_pose_graph* pg, int which, double lambda, int repeats, double* ms_per_sweep) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg || !ms_per_sweep || repeats < 1 || which < 0 || which > 1) return fail(NOS_ERR_INVALID_ARGUMENT, "bad argument");
  DeviceSlot& slot = pg->ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  if (which == 0) {  // x = gradient (its switch rows included); CG scalars zeroed: beta = 0, no breakdown flag
    NOS_HIP_CHECK(hipMemcpyAsync(pg->d_p, pg->d_grad, pg->n_unknowns * sizeof(double), hipMemcpyDeviceToDevice, slot.stream));
    NOS_HIP_CHECK(hipMemsetAsync(pg->d_scalars, 0, 8 * sizeof(double), slot.stream));
  }
  auto sweep = [&]() {
    if (which == 1) {
      pgo_launch_linearize(pg);
    } else if (pg->block_poses != 0) {  // as the PCG iteration launches it: with the direction update in its staging
      (void)pgo_launch_product(pg, lambda, pg->d_p, pg->d_ap, pg->d_grad, pg->d_p2);
    } else {
      (void)pgo_launch_product(pg, lambda, pg->d_p, pg->d_ap);
    }
  };
  sweep();  // warm
  NOS_HIP_CHECK(hipEventRecord(slot.ev0, slot.stream));
  for (int k = 0; k < repeats; ++k) sweep();
  NOS_HIP_CHECK(hipEventRecord(slot.ev1, slot.stream));
  NOS_HIP_CHECK(hipGetLastError());
  NOS_HIP_CHECK(hipEventSynchronize(slot.ev1));
  float ms = 0.f;
  NOS_HIP_CHECK(hipEventElapsedTime(&ms, slot.ev0, slot.ev1));
  *ms_per_sweep = double(ms) / repeats;
  return NOS_OK;
}

// y = (H with damped diagonal) x for a host vector (tests).
int nos_pgo_matvec(nos_pose_graph* pg, double lambda, const double* x, double* y) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg || !x || !y) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  DeviceSlot& slot = pg->ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  const size_t N6 = size_t(6) * pg->n_poses, n = pg->n_unknowns;
  std::vector<double> rec(n);
  to_records(pg, x, rec.data());
  NOS_HIP_CHECK(hipMemcpyAsync(pg->d_p, rec.data(), n * sizeof(double), hipMemcpyHostToDevice, slot.stream));
  NOS_HIP_CHECK(hipMemsetAsync(pg->d_ap, 0, n * sizeof(double), slot.stream));
  int rc = pgo_launch_product(pg, lambda, pg->d_p, pg->d_ap);  // the product the PCG iteration makes
  if (rc != NOS_OK) return rc;
  NOS_HIP_CHECK(hipMemcpyAsync(rec.data(), pg->d_ap, n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  to_planes(pg, rec.data(), y, pg->n_free_switches > 0);
  if (pg->n_free_switches == 0)  // the switch rows took no part: their diagonal alone
    for (size_t e = 0; e < pg->n_edges; ++e) y[N6 + e] = (1.0 + lambda) * x[N6 + e];
  return NOS_OK;
}

// z = M^-1 r for a host vector (tests): the preconditioner nos_pgo_solve would use at this lambda.
int nos_pgo_precondition(nos_pose_graph* pg, double lambda, const double* r, double* z) {
  nosd::CtxGuard guard_(pg ? pg->ctx : nullptr);  // one solve / accumulate / create at a time per context
  if (!pg || !r || !z) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL argument");
  DeviceSlot& slot = pg->ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  PgoPrecond pc;
  int rc = pgo_precond_setup(pg, lambda, &pc);  // before r goes up: the probing form uses d_p / d_ap as scratch
  if (rc != NOS_OK) return rc;
  const size_t N6 = size_t(6) * pg->n_poses, n = pg->n_unknowns;
  std::vector<double> rec(n);
  to_records(pg, r, rec.data());
  NOS_HIP_CHECK(hipMemcpyAsync(pg->d_r, rec.data(), n * sizeof(double), hipMemcpyHostToDevice, slot.stream));
  rc = pgo_precond_apply(pg, lambda, pc);
  if (rc != NOS_OK) return rc;
  NOS_HIP_CHECK(hipGetLastError());
  NOS_HIP_CHECK(hipMemcpyAsync(rec.data(), pg->d_z, n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  to_planes(pg, rec.data(), z, pc.active_edges > 0);
  if (pc.active_edges == 0)  // the switch rows took no part: their diagonal alone
    for (size_t e = 0; e < pg->n_edges; ++e) z[N6 + e] = r[N6 + e] / (1.0 + lambda);
  return NOS_OK;
}

}  // extern "C"
