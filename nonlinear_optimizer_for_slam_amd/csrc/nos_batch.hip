// nos_batch.hip — nos_ndt6_solve_batch / nos_ndt3_solve_batch / nos_reproj_solve_batch (C ABI of include/nos.h).
//
// B independent pose problems: the small flat ones in ONE launch, one workgroup each (nos::solve_batch_kernel, the loop of
// the lone single-workgroup solve), the others one at a time through the lone solve (lm_solve) after it.  Every problem ends
// with what nos_*_solve would give it.
#include "nos_internal.hpp"

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

template <typename Problem, typename T>
int launch_batch_kernel(uint32_t n_blocks, const void* d_descs, nos::BatchResult* d_results, double* d_history,
                        int history_stride, hipStream_t stream, const void** kernel_out) {
  const auto kernel = nos::solve_batch_kernel<Problem, T, kBatchBlock>;
  *kernel_out = reinterpret_cast<const void*>(kernel);
  hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(kBatchBlock), 0, stream,
                     static_cast<const nos::BatchDesc<typename Problem::Params>*>(d_descs), d_results, d_history,
                     history_stride);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NOS_ERR_HIP, "batched solve launch failed: %s", hipGetErrorString(e));
  return NOS_OK;
}

// The batch launch over the problems listed in `members`: descriptors up through pinned memory, one launch, results and
// cost histories down in one copy, one synchronisation, then the caller's arrays.
template <template <typename, int> class ProblemT, typename T>
int run_batch(const BatchCall& c, const std::vector<Request>& rq, const std::vector<int>& members) {
  using Desc = nos::BatchDesc<typename ProblemT<T, nos::kLossNone>::Params>;
  DeviceSlot& slot = c.ds[0]->ctx->slots[0];
  hipStream_t stream = slot.stream;
  const size_t B = members.size();
  const int max_it = c.opt->max_iterations;
  const bool with_history = c.opt->cost_history != nullptr;
  auto round_up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t desc_bytes = round_up(B * sizeof(Desc));
  const size_t result_bytes = round_up(B * sizeof(nos::BatchResult));
  const size_t history_bytes = with_history ? B * size_t(max_it) * sizeof(double) : 0;
  const size_t total = desc_bytes + result_bytes + history_bytes;

  NOS_HIP_CHECK(hipSetDevice(slot.device));
  if (slot.batch_pinned_bytes < total) {  // grows only; freed with the context
    if (slot.batch_pinned != nullptr) (void)hipHostFree(slot.batch_pinned);
    slot.batch_pinned = nullptr;
    slot.batch_pinned_bytes = 0;
    NOS_HIP_CHECK(hipHostMalloc(&slot.batch_pinned, total, hipHostMallocDefault));
    slot.batch_pinned_bytes = total;
  }
  unsigned char* const pinned = static_cast<unsigned char*>(slot.batch_pinned);
  for (size_t j = 0; j < B; ++j) {
    const int i = members[j];
    const nos_dataset* ds = c.ds[i];
    Desc& d = *new (pinned + j * sizeof(Desc)) Desc{};
    d.L = ds->shards[0].layout;
    fill_params(d.P, rq[size_t(i)], ds);
    d.n_chunks = uint32_t((std::max<uint64_t>(d.L.n, 1) + kBatchBlock - 1) / kBatchBlock);
    d.init = make_lm_init(ds, rq[size_t(i)], c.opt, c.R + size_t(i) * c.nR, c.nR, c.t + size_t(i) * c.nt, c.nt);  // as lm_solve
  }

  void* dev = nullptr;
  size_t dev_capacity = 0;
  int rc = pool_alloc(slot, total, &dev, &dev_capacity);
  if (rc != NOS_OK) return rc;
  unsigned char* const dev_bytes = static_cast<unsigned char*>(dev);
  nos::BatchResult* const d_results = reinterpret_cast<nos::BatchResult*>(dev_bytes + desc_bytes);
  double* const d_history = with_history ? reinterpret_cast<double*>(dev_bytes + desc_bytes + result_bytes) : nullptr;
  const void* kernel = nullptr;
  const uint32_t n_blocks = uint32_t(B);
  hipError_t e = hipMemcpyAsync(dev, pinned, desc_bytes, hipMemcpyHostToDevice, stream);
  if (e == hipSuccess) {
    switch (rq[size_t(members[0])].loss_kind) {  // one loss for the whole call
      case NOS_LOSS_NONE:
        rc = launch_batch_kernel<ProblemT<T, nos::kLossNone>, T>(n_blocks, dev, d_results, d_history, max_it, stream, &kernel);
        break;
      case NOS_LOSS_EXPONENTIAL:
        rc = launch_batch_kernel<ProblemT<T, nos::kLossExponential>, T>(n_blocks, dev, d_results, d_history, max_it, stream,
                                                                        &kernel);
        break;
      default:
        rc = launch_batch_kernel<ProblemT<T, nos::kLossHuber>, T>(n_blocks, dev, d_results, d_history, max_it, stream, &kernel);
        break;
    }
    if (rc == NOS_OK) {
      slot.last_kernel = kernel;
      e = hipMemcpyAsync(pinned + desc_bytes, dev_bytes + desc_bytes, result_bytes + history_bytes, hipMemcpyDeviceToHost,
                         stream);
    }
  }
  const hipError_t es = hipStreamSynchronize(stream);  // before the buffer goes back to the pool, after a failure too
  pool_release(slot, dev, dev_capacity);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "batched solve: %s", hipGetErrorString(e));
  if (rc != NOS_OK) return rc;

  const nos::BatchResult* const results = reinterpret_cast<const nos::BatchResult*>(pinned + desc_bytes);
  const double* const history = reinterpret_cast<const double*>(pinned + desc_bytes + result_bytes);
  for (size_t j = 0; j < B; ++j) {
    const int i = members[j];
    const nos::BatchResult& r = results[j];
    for (int k = 0; k < c.nR; ++k) c.R[size_t(i) * c.nR + k] = r.st.R[k];
    for (int k = 0; k < c.nt; ++k) c.t[size_t(i) * c.nt + k] = r.st.t[k];
    if (with_history)
      for (int k = 0; k < r.executed && k < max_it; ++k)
        c.opt->cost_history[size_t(i) * size_t(max_it) + k] = history[j * size_t(max_it) + k];
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
