// assemble_register_live.hpp — batched registration against the LIVE voxel store (nos_voxel_map_register6_batch /
// nos_voxel_map_register3_batch): register_problem (assemble_register.hpp) instantiated for the store's
// view, so every round's match is match_point on find_two_nearest of voxelmatch_kernels.hpp.
// Part of the hand-written gfx950 kernels of the Gauss-Newton normal-equation assembly path; see assemble_kernels.hpp.
#pragma once

#include "assemble_register.hpp"
#include "voxelmatch_kernels.hpp"

namespace nos {

// The matcher keeps voxel_match_kernel's nine probes in flight per step.  One workgroup of 512 lanes per problem is two
// waves per SIMD whatever the kernel needs, so up to 256 VGPRs per lane cost nothing — beyond that, or with scratch, the
// kernel is not acceptable.  The match phase is not where the registers peak: the loop's state lives in LDS across it,
// and the peak is single_block_loop's.  Every instantiation compiles to 170 … 206 VGPRs, no spill, no scratch
// (tests/test_voxel_register_kernel_resources.py), so the probe depth is left as it is.

// register_batch_kernel on the live store.  The store is only read; `error` (its kInfoProbeError word) is the one word of
// it this kernel may write.  (The name must not contain "register_batch_kernel<": the resource test of that kernel counts
// the kernels of nos_register.o by it.)
template <typename Problem, typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void register_live_kernel(VoxelMatchView map, unsigned int* __restrict__ error,
                                                             const RegisterDesc<typename Problem::Params>* __restrict__ descs,
                                                             RegisterResult* __restrict__ results,
                                                             RegisterRound* __restrict__ round_log, int max_outer,
                                                             int max_neighbors, int keep_multiple) {
  register_problem<Problem, T, BLOCK>(map, error, descs, results, round_log, max_outer, max_neighbors, keep_multiple);
}

}  // namespace nos
