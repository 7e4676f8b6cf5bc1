// register_host.hpp — host side of a batched registration, shared by nos_register.hip (against a snapshot: nos_ndt_map)
// and nos_voxelregister.hip (against the live voxel store): validation, descriptors, pooled scratch, the launch through
// the caller's Launcher, the copy back.  One copy of each step; the two units differ in the map view and the kernel only.
#pragma once

#include "batch_host.hpp"
#include "assemble_register.hpp"

namespace nosd {

constexpr int kRegisterBlock = 512;  // the single-workgroup solve's block: same chunks, same reduction order

struct RegisterCall {
  int dof;
  nos_ctx* ctx;  // the map's context; NULL: the map argument was NULL
  nos_scan* const* scans;
  int n;
  double* R;  // [n][9], in-out
  double* t;  // [n][3], in-out
  const nos_loss* loss;
  const nos_register_options* ropt;
  const nos_lm_options* opt;
  nos_register_report* reports;
};

// Not the shared fill_params: a registration has a 3x3 start pose and a loss, no Request and no dataset to take them from.
template <typename T>
inline void fill_loss_params(nos::Ndt6Params<T>& P, const double R[9], const double t[3], const nos_loss* loss) {
  for (int k = 0; k < 9; ++k) P.R[k] = T(R[k]);
  for (int k = 0; k < 3; ++k) P.t[k] = T(t[k]);
  fill_loss(loss, P.la, P.lb, P.lc);
}
template <typename T>
inline void fill_loss_params(nos::Ndt3Params<T>& P, const double R[9], const double t[3], const nos_loss* loss) {
  const double R2[4] = {R[0], R[1], R[3], R[4]};
  for (int k = 0; k < 4; ++k) P.R2[k] = T(R2[k]);
  for (int k = 0; k < 2; ++k) P.t2[k] = T(t[k]);
  fill_loss(loss, P.la, P.lb, P.lc);
}

// Descriptors up through pinned memory, one pooled device block for descriptors, results, round log and every problem's
// scratch dataset, one launch, results and log down in one copy, one synchronisation (BatchTrip), then the caller's arrays.
// Launcher: the map and its kernel (SnapshotLauncher of nos_register.hip, LiveLauncher of nos_voxelregister.hip):
//   static constexpr bool kTallyLaunch               whether the launch is added to the bracket profiler's tally
//   hipError_t prepare(stream)                        what must be on the stream before the launch
//   const void* launch<Problem, T>(n_blocks, descs, results, log, ropt, stream)   the launch → the kernel's host address
template <template <typename, int> class ProblemT, typename T, typename Launcher>
int run_register(const RegisterCall& c, int loss_kind, const Launcher& launcher) {
  using Desc = nos::RegisterDesc<typename ProblemT<T, nos::kLossNone>::Params>;
  nos_ctx* ctx = c.ctx;
  DeviceSlot& slot = ctx->slots[0];
  hipStream_t stream = slot.stream;
  const size_t B = size_t(c.n);
  const int max_outer = c.ropt->max_outer_iterations;
  // scratch datasets: the layout nos_ndt_match gives a dataset of 2n slots of this element type
  const int tile_log2 = dataset_tile_log2(ctx, c.ropt->dtype);
  if (tile_log2 != 0 && (tile_log2 < 10 || tile_log2 > 24)) return fail(NOS_ERR_INVALID_ARGUMENT, "tile_log2 out of range");
  BatchTrip trip(slot);
  const auto descs = trip.section(BatchTrip::kUp, B * sizeof(Desc));
  const auto results = trip.section(BatchTrip::kDown, B * sizeof(nos::RegisterResult));
  const auto log = trip.section(BatchTrip::kDown, B * size_t(max_outer) * sizeof(nos::RegisterRound));
  std::vector<nos::TiledLayout> layouts(B);
  std::vector<BatchTrip::Section> scratch(B);
  for (size_t i = 0; i < B; ++i) {
    layouts[i] = make_layout(2 * c.scans[i]->n, nos::kNdtStored, tile_log2, ctx->settings.plane_skew);
    scratch[i] = trip.section(BatchTrip::kDeviceOnly, layout_elems(layouts[i], nos::kNdtStored) * sizeof(T));
  }
  const int rc = trip.open();
  if (rc != NOS_OK) return rc;
  for (size_t i = 0; i < B; ++i) {
    const nos_scan* scan = c.scans[i];
    Desc& d = *new (trip.host<Desc>(descs) + i) Desc{};
    d.L = layouts[i];
    d.L.base = trip.dev<unsigned char>(scratch[i]);
    fill_loss_params(d.P, c.R + 9 * i, c.t + 3 * i, c.loss);
    d.points = scan->d_planes;
    d.n_points = scan->n;
    d.n_chunks = uint32_t((std::max<uint64_t>(d.L.n, 1) + kRegisterBlock - 1) / kRegisterBlock);
    d.dof = c.dof;
    set_pose(d, c.R + 9 * i, c.t + 3 * i);
    d.settings = make_lm_settings(c.opt, 0, kKindNdt);  // as lm_solve; a matcher-written dataset has simd_class 0
  }
  if (trip.send() && trip.check(launcher.prepare(stream))) {
    const void* const kernel = with_loss(loss_kind, [&](auto loss) {  // one loss for the whole call
      return launcher.template launch<ProblemT<T, decltype(loss)::value>, T>(
          uint32_t(B), trip.dev<const Desc>(descs), trip.dev<nos::RegisterResult>(results), trip.dev<nos::RegisterRound>(log),
          c.ropt, stream);
    });
    if (trip.launched()) {
      slot.last_kernel = kernel;
      // bracket profiling (nos_ctx_profile_begin with sample_every = 0): the call's one launch, SELF-REPORTED, for the
      // launchers that ask for it (the snapshot's never reported its launch and still does not)
      if (Launcher::kTallyLaunch && slot.prof_on && slot.prof_every == 0) ++slot.prof_launches;
      trip.fetch();
    }
  }
  const int status = trip.close("batched registration");
  if (status != NOS_OK) return status;

  static_assert(sizeof(nos::RegisterRound) == sizeof(nos_register_round), "round log entry layout");
  for (size_t i = 0; i < B; ++i)  // live store only; before anything of the caller's is written
    if (trip.host<const nos::RegisterResult>(results)[i].probe_error != 0)
      return fail(NOS_ERR_HIP, "batched registration against the voxel store failed: a table probe ran through the whole table");
  for (size_t i = 0; i < B; ++i) {
    const nos::RegisterResult& r = trip.host<const nos::RegisterResult>(results)[i];
    for (int k = 0; k < 9; ++k) c.R[9 * i + k] = r.R[k];
    for (int k = 0; k < 3; ++k) c.t[3 * i + k] = r.t[k];
    nos_register_report& rep = c.reports[i];
    rep.outer_iter = r.outer_iter;
    rep.rounds = r.rounds;
    rep.ok = r.ok;
    rep.pad = 0;
    if (c.ropt->round_log != nullptr) {
      nos_register_round* row = c.ropt->round_log + i * size_t(max_outer);
      for (int k = 0; k < max_outer; ++k) {
        nos_register_round& o = row[k];
        if (k < r.rounds) {
          const nos::RegisterRound& g = trip.host<const nos::RegisterRound>(log)[i * size_t(max_outer) + size_t(k)];
          o.matches = g.matches;
          o.used = g.used;
          o.iterations = g.iterations;
          o.ok = g.ok;
          o.printed_cost = g.printed_cost;
          o.last_cost = g.last_cost;
        } else {
          memset(&o, 0, sizeof o);
        }
      }
    }
  }
  return NOS_OK;
}

// Validation first (nothing is launched and nothing written before every check has passed), then the launch.
// more_checks(): what the kind of map rejects beyond the common list, after it (→ a status).
template <typename Checks, typename Launcher>
int register_batch(const RegisterCall& c, const Checks& more_checks, const Launcher& launcher) {
  if (c.n < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "n_problems < 0");
  if (c.n == 0) return NOS_OK;
  if (!c.ctx || !c.scans || !c.R || !c.t || !c.ropt || !c.opt || !c.reports) return fail(NOS_ERR_INVALID_ARGUMENT, "NULL array");
  nos_ctx* ctx = c.ctx;
  CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  const int rc_scans = check_scans(ctx, c.scans, c.n);
  if (rc_scans != NOS_OK) return rc_scans;
  const nos_register_options& ro = *c.ropt;
  if (ro.max_outer_iterations < 1) return fail(NOS_ERR_INVALID_ARGUMENT, "max_outer_iterations < 1");
  if (ro.keep_multiple < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "keep_multiple < 0");
  if (ro.dtype != NOS_F64 && ro.dtype != NOS_F32) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown dtype %d", ro.dtype);
  if (c.opt->max_iterations < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "max_iterations < 0");
  if (c.opt->cost_history != nullptr)
    return fail(NOS_ERR_INVALID_ARGUMENT, "cost_history is not supported by batched registration (rounds: round_log)");
  int loss_kind = 0;
  const int rc = check_loss(c.loss, &loss_kind);
  if (rc != NOS_OK) return rc;
  if (ro.max_neighbors < 1 || ro.max_neighbors > 2) return fail(NOS_ERR_UNSUPPORTED, "max_neighbors must be 1 or 2");
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "batched registration needs a single-device context");
  if (ctx->comm != nullptr || ctx->shm_dev != nullptr)
    return fail(NOS_ERR_UNSUPPORTED, "batched registration is process-local: the context has a communicator");
  const int rc_more = more_checks();
  if (rc_more != NOS_OK) return rc_more;
  const bool f64 = ro.dtype == NOS_F64;
  if (c.dof == 6)
    return f64 ? run_register<nos::Ndt6Problem, double>(c, loss_kind, launcher)
               : run_register<nos::Ndt6Problem, float>(c, loss_kind, launcher);
  return f64 ? run_register<nos::Ndt3Problem, double>(c, loss_kind, launcher)
             : run_register<nos::Ndt3Problem, float>(c, loss_kind, launcher);
}

}  // namespace nosd
