// nos_batch.hip — nos_ndt6_solve_batch / nos_ndt3_solve_batch / nos_reproj_solve_batch (C ABI of include/nos.h).
//
// B independent pose problems: the small flat ones in ONE launch, one workgroup each (nos::solve_batch_kernel, the loop of
// the lone single-workgroup solve), the others one at a time through the lone solve (lm_solve) after it.  Every problem ends
// with what nos_*_solve would give it.
#include "batch_host.hpp"

namespace nosd {
namespace {

constexpr int kBatchBlock = 512;  // the single-workgroup solve's block: same chunks, same reduction order

// Arguments of one batched call, the same for the three problems (6, 3, or 2 = reprojection).
struct BatchCall {
  int problem;
  nos_dataset* const* ds;
  int n;
  double* R;  // [n][nR], in-out
  int nR;
  double* t;  // [n][nt], in-out
  int nt;
  const double* intr;  // [n][4]: reprojection only
  double min_depth;
  const nos_loss* loss;
  const nos_lm_options* opt;
  nos_lm_report* reports;
};

// The batch launch over the problems listed in `members`: descriptors up through pinned memory, one launch, results and
// cost histories down in one copy, one synchronisation (BatchTrip), then the caller's arrays.
template <template <typename, int> class ProblemT, typename T>
int run_batch(const BatchCall& c, const std::vector<Request>& rq, const std::vector<int>& members) {
  using Desc = nos::BatchDesc<typename ProblemT<T, nos::kLossNone>::Params>;
  DeviceSlot& slot = c.ds[0]->ctx->slots[0];
  const size_t B = members.size();
  const int max_it = c.opt->max_iterations;
  const bool with_history = c.opt->cost_history != nullptr;
  BatchTrip trip(slot);
  const auto descs = trip.section(BatchTrip::kUp, B * sizeof(Desc));
  const auto results = trip.section(BatchTrip::kDown, B * sizeof(nos::BatchResult));
  const auto history = trip.section(BatchTrip::kDown, with_history ? B * size_t(max_it) * sizeof(double) : 0);
  const int rc = trip.open();
  if (rc != NOS_OK) return rc;
  for (size_t j = 0; j < B; ++j) {
    const int i = members[j];
    const nos_dataset* ds = c.ds[i];
    Desc& d = *new (trip.host<Desc>(descs) + j) Desc{};
    d.L = ds->shards[0].layout;
    fill_params(d.P, rq[size_t(i)], ds);
    d.n_chunks = uint32_t((std::max<uint64_t>(d.L.n, 1) + kBatchBlock - 1) / kBatchBlock);
    d.init = make_lm_init(ds, rq[size_t(i)], c.opt, c.R + size_t(i) * c.nR, c.nR, c.t + size_t(i) * c.nt, c.nt);  // as lm_solve
  }
  if (trip.send()) {
    const void* const kernel = with_loss(rq[size_t(members[0])].loss_kind, [&](auto loss) {  // one loss for the whole call
      const auto k = nos::solve_batch_kernel<ProblemT<T, decltype(loss)::value>, T, kBatchBlock>;
      hipLaunchKernelGGL(k, dim3(uint32_t(B)), dim3(kBatchBlock), 0, slot.stream, trip.dev<const Desc>(descs),
                         trip.dev<nos::BatchResult>(results), with_history ? trip.dev<double>(history) : nullptr, max_it);
      return reinterpret_cast<const void*>(k);
    });
    if (trip.launched()) {
      slot.last_kernel = kernel;
      trip.fetch();
    }
  }
  const int status = trip.close("batched solve");
  if (status != NOS_OK) return status;

  for (size_t j = 0; j < B; ++j) {
    const int i = members[j];
    const nos::BatchResult& r = trip.host<const nos::BatchResult>(results)[j];
    for (int k = 0; k < c.nR; ++k) c.R[size_t(i) * c.nR + k] = r.st.R[k];
    for (int k = 0; k < c.nt; ++k) c.t[size_t(i) * c.nt + k] = r.st.t[k];
    if (with_history)
      for (int k = 0; k < r.executed && k < max_it; ++k)
        c.opt->cost_history[size_t(i) * size_t(max_it) + k] = trip.host<const double>(history)[j * size_t(max_it) + k];
    nos_lm_report& rep = c.reports[i];
    rep.iterations = r.st.iteration;
    rep.ok = r.st.ok;
    rep.launches = 1;
    rep.fallback = 0;
    rep.printed_cost = r.st.previous_cost;
    rep.last_cost = r.st.cost;
    rep.final_lambda = r.st.lambda;
  }
  return NOS_OK;
}

// Validation first (nothing is launched and nothing written before every check has passed), then the batch launch, then
// the lone solves.
int solve_batch(const BatchCall& c) {
  if (c.n < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "n_problems < 0");
  if (c.n == 0) return NOS_OK;
  if (!c.ds || !c.R || !c.t || !c.opt || !c.reports || (c.problem == 2 && !c.intr))
    return fail(NOS_ERR_INVALID_ARGUMENT, "NULL array");
  for (int i = 0; i < c.n; ++i)
    if (c.ds[i] == nullptr) return fail(NOS_ERR_INVALID_ARGUMENT, "dataset %d is NULL", i);
  nos_ctx* ctx = c.ds[0]->ctx;
  CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (c.opt->max_iterations < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "max_iterations < 0");
  std::vector<Request> rq(size_t(c.n));
  for (int i = 0; i < c.n; ++i) {
    const nos_dataset* ds = c.ds[i];
    if (ds->ctx != ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "dataset %d belongs to another context", i);
    if (ds->dtype != c.ds[0]->dtype) return fail(NOS_ERR_INVALID_ARGUMENT, "dataset %d has another element type", i);
    const int rc = build_request(c.problem, ds, c.R + size_t(i) * c.nR, c.nR, c.t + size_t(i) * c.nt, c.nt,
                                 c.intr ? c.intr + size_t(i) * 4 : nullptr, c.min_depth, c.loss, &rq[size_t(i)]);
    if (rc != NOS_OK) return rc;
  }
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "batched solves need a single-device context");
  if (ctx->comm != nullptr || ctx->shm_dev != nullptr)
    return fail(NOS_ERR_UNSUPPORTED, "batched solves are process-local: the context has a communicator");

  // the batch launch takes flat datasets up to batch_max_elements plane-elements, when there is a loop to run
  std::vector<int> members, lone;
  for (int i = 0; i < c.n; ++i) {
    const nos_dataset* ds = c.ds[i];
    const bool in_batch = ds->kind != kKindNdtIndexed && c.opt->max_iterations > 0 &&
                          ds->n * size_t(ds->n_fields) <= size_t(ctx->settings.batch_max_elements);
    (in_batch ? members : lone).push_back(i);
  }
  if (!members.empty()) {
    const bool f64 = c.ds[0]->dtype == NOS_F64;
    int rc;
    if (c.problem == 6)
      rc = f64 ? run_batch<nos::Ndt6Problem, double>(c, rq, members) : run_batch<nos::Ndt6Problem, float>(c, rq, members);
    else if (c.problem == 3)
      rc = f64 ? run_batch<nos::Ndt3Problem, double>(c, rq, members) : run_batch<nos::Ndt3Problem, float>(c, rq, members);
    else
      rc = f64 ? run_batch<nos::ReprojProblem, double>(c, rq, members) : run_batch<nos::ReprojProblem, float>(c, rq, members);
    if (rc != NOS_OK) return rc;
  }
  // the others exactly as nos_*_solve runs them; row i of the cost history starts at i * max_iterations
  for (const int i : lone) {
    nos_lm_options opt = *c.opt;
    if (opt.cost_history != nullptr) opt.cost_history += size_t(i) * size_t(opt.max_iterations);
    const int rc = lm_solve(c.ds[i], rq[size_t(i)], &opt, c.R + size_t(i) * c.nR, c.nR, c.t + size_t(i) * c.nt, c.nt,
                            &c.reports[i]);
    if (rc != NOS_OK) return rc;
  }
  return NOS_OK;
}

}  // namespace
}  // namespace nosd

extern "C" {

int nos_ndt6_solve_batch(nos_dataset* const* ds, int32_t n_problems, double* R, double* t, const nos_loss* loss,
                         const nos_lm_options* options, nos_lm_report* reports) {
  return nosd::solve_batch({6, ds, n_problems, R, 9, t, 3, nullptr, 0.0, loss, options, reports});
}

int nos_ndt3_solve_batch(nos_dataset* const* ds, int32_t n_problems, double* R2, double* t2, const nos_loss* loss,
                         const nos_lm_options* options, nos_lm_report* reports) {
  return nosd::solve_batch({3, ds, n_problems, R2, 4, t2, 2, nullptr, 0.0, loss, options, reports});
}

int nos_reproj_solve_batch(nos_dataset* const* ds, int32_t n_problems, double* R, double* t, const double* intr,
                           const nos_loss* loss, double min_depth, const nos_lm_options* options, nos_lm_report* reports) {
  return nosd::solve_batch({2, ds, n_problems, R, 9, t, 3, intr, min_depth, loss, options, reports});
}

}  // extern "C"
