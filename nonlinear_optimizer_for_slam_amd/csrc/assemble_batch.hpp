// assemble_batch.hpp — many small LM problems in one launch: one workgroup per problem, each running the loop of the
// single-workgroup solve on its own dataset, pose and loop state (nos_*_solve_batch).
// Part of the hand-written gfx950 kernels of the Gauss-Newton normal-equation assembly path; see assemble_kernels.hpp
// (the umbrella header every translation unit includes) for the overview and the reference citations.
#pragma once

#include "assemble_misc.hpp"

namespace nos {

// ---------------------------------------------------------------- batched solve: one problem per workgroup
//
// The single-workgroup solve (solve_single_block_kernel) keeps one CU busy, and every further pose pays a launch and a host
// wait of its own.  The batched form runs B independent problems in ONE launch, workgroup b on problem b.  Its descriptor
// names the dataset's layout, the item parameters (loss; intrinsics and depth rules for reprojection), the chunk count and
// the start of the loop (pose, settings).  Lane 0 makes the initial state with the same nos_host::LmInit6 / LmInit3 call as
// lm_init_kernel, then the workgroup runs single_block_loop — the loop of solve_single_block_kernel — so that every problem
// ends with the bits of its lone solve.  No workgroup waits for another: any B is safe, the ones that are not resident
// queue in the dispatcher.
template <typename Params>
struct BatchDesc {
  TiledLayout L;
  Params P;
  uint32_t n_chunks;  // chunks of 512 correspondences: (max(n, 1) + 511) / 512, as the lone solve launches it
  LmInitArgs init;    // start pose, settings, dof — what lm_init_kernel gets
};

// What workgroup b leaves behind (plain stores; the host copies the whole array back once).
struct BatchResult {
  nos_host::LmState st;  // final loop state
  double sums[32];       // the 28 / 10 sums of the last executed iteration (0 when none ran)
  int executed;          // iterations executed inside the launch
  int pad;
};

template <typename Problem, typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void solve_batch_kernel(const BatchDesc<typename Problem::Params>* __restrict__ descs,
                                                           BatchResult* __restrict__ results,
                                                           double* __restrict__ cost_history, int history_stride) {
  constexpr int kOut = Problem::kOut;
  const BatchDesc<typename Problem::Params>& d = descs[blockIdx.x];
  __shared__ double s_lm_raw[(sizeof(LmDevice) + 7) / 8];  // raw storage: the struct has default member initialisers
  LmDevice& s_lm = *reinterpret_cast<LmDevice*>(s_lm_raw);
  __shared__ double s_sum[kLmTotDoubles(kOut)];
  if (threadIdx.x == 0) {  // lm_init_kernel's body, into LDS
    nos_host::LmState st;
    if (d.init.dof == 6)
      nos_host::LmInit6(&st, d.init.R, d.init.t, d.init.settings.max_iterations, d.init.settings.float_schedule);
    else
      nos_host::LmInit3(&st, d.init.R, d.init.t, d.init.settings.max_iterations, d.init.settings.float_schedule);
    s_lm.st = st;
    s_lm.settings = d.init.settings;
  }
  __syncthreads();
  const TiledLayout L = d.L;
  typename Problem::Params P = d.P;
  // row b of the history: history_stride (= max_iterations) entries, of which the executed ones are written
  double* const history = cost_history != nullptr ? cost_history + size_t(blockIdx.x) * size_t(history_stride) : nullptr;
  const int executed = single_block_loop<Problem, T, BLOCK, false>(L, P, d.n_chunks, s_lm, s_sum, history, history_stride);
  BatchResult& r = results[blockIdx.x];
  if (threadIdx.x < kOut) r.sums[threadIdx.x] = executed > 0 ? s_sum[threadIdx.x] : 0.0;
  if (threadIdx.x == 0) {
    r.st = s_lm.st;
    r.executed = executed;
  }
}

}  // namespace nos
