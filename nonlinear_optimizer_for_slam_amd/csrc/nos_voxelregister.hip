// nos_voxelregister.hip — nos_voxel_map_register6_batch / nos_voxel_map_register3_batch (C ABI of include/nos.h; the entry
// points themselves are in nos_voxelmap.hip; the store, struct nos_voxel_map, is voxel_store_host.hpp's, which only that unit
// includes).
//
// nos_ndt*_register_batch (nos_register.hip) against the LIVE voxel store: B registrations in ONE launch, one workgroup
// each (nos::register_live_kernel, assemble_register_live.hpp), every round matched through the table the inserts
// maintain — no snapshot, nothing sorted, nothing allocated in proportion to the map.
#include "register_host.hpp"
#include "assemble_register_live.hpp"

namespace nosd {
namespace {

struct LiveLauncher {
  const LiveStore& store;
  static constexpr bool kTallyLaunch = true;
  hipError_t prepare(hipStream_t stream) const { return hipMemsetAsync(store.d_error, 0, sizeof(unsigned int), stream); }
  template <typename Problem, typename T>
  const void* launch(uint32_t n_blocks, const nos::RegisterDesc<typename Problem::Params>* d_descs,
                     nos::RegisterResult* d_results, nos::RegisterRound* d_log, const nos_register_options* ropt,
                     hipStream_t stream) const {
    const auto kernel = nos::register_live_kernel<Problem, T, kRegisterBlock>;
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(kRegisterBlock), 0, stream, store.view, store.d_error, d_descs,
                       d_results, d_log, ropt->max_outer_iterations, ropt->max_neighbors, ropt->keep_multiple);
    return reinterpret_cast<const void*>(kernel);
  }
};

}  // namespace

int register_live(int dof, const LiveStore* store, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                  const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                  nos_register_report* reports) {
  static const LiveStore no_store{};  // never launched with: a NULL map is rejected first
  const LiveStore& s = store ? *store : no_store;
  auto more_checks = [&s] { return check_live_store(s); };  // what nos_voxel_map_match rejects, in its order
  return register_batch({dof, s.ctx, scans, n_problems, R, t, loss, ropt, options, reports}, more_checks, LiveLauncher{s});
}

}  // namespace nosd
