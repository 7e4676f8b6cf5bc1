// nos_register.hip — nos_ndt6_register_batch / nos_ndt3_register_batch (C ABI of include/nos.h).
//
// B scan-to-map registrations against one map in ONE launch, one workgroup each (nos::register_batch_kernel,
// assemble_register.hpp): every round's matching, tail drop, LM loop and stopping test run on the device.  Problem i ends
// with what pipeline.scan_to_map gives scans[i].
#include "register_host.hpp"

namespace nosd {
namespace {

struct SnapshotLauncher {
  const nos::MapView& map;
  static constexpr bool kTallyLaunch = false;
  hipError_t prepare(hipStream_t) const { return hipSuccess; }
  template <typename Problem, typename T>
  const void* launch(uint32_t n_blocks, const nos::RegisterDesc<typename Problem::Params>* d_descs,
                     nos::RegisterResult* d_results, nos::RegisterRound* d_log, const nos_register_options* ropt,
                     hipStream_t stream) const {
    const auto kernel = nos::register_batch_kernel<Problem, T, kRegisterBlock>;
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(kRegisterBlock), 0, stream, map, d_descs, d_results, d_log,
                       ropt->max_outer_iterations, ropt->max_neighbors, ropt->keep_multiple);
    return reinterpret_cast<const void*>(kernel);
  }
};

int register_snapshot(int dof, nos_ndt_map* map, nos_scan* const* scans, int32_t n, double* R, double* t, const nos_loss* loss,
                      const nos_register_options* ropt, const nos_lm_options* opt, nos_register_report* reports) {
  static const nos::MapView no_map{};  // never launched with: a NULL map is rejected first
  return register_batch({dof, map ? map->ctx : nullptr, scans, n, R, t, loss, ropt, opt, reports}, [] { return NOS_OK; },
                        SnapshotLauncher{map ? map->view : no_map});
}

}  // namespace
}  // namespace nosd

extern "C" {

int nos_ndt6_register_batch(nos_ndt_map* map, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                            const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                            nos_register_report* reports) {
  return nosd::register_snapshot(6, map, scans, n_problems, R, t, loss, ropt, options, reports);
}

int nos_ndt3_register_batch(nos_ndt_map* map, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                            const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                            nos_register_report* reports) {
  return nosd::register_snapshot(3, map, scans, n_problems, R, t, loss, ropt, options, reports);
}

}  // extern "C"
