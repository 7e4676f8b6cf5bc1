// assemble_register.hpp — many scan-to-map registrations in one launch: one workgroup per problem, each running the
// reference's outer loop (match at the current pose, tail drop, LM solve, stopping test) on the device
// (nos_ndt6_register_batch / nos_ndt3_register_batch).
// Part of the hand-written gfx950 kernels of the Gauss-Newton normal-equation assembly path; see assemble_kernels.hpp
// (the umbrella header every translation unit includes) for the overview and the reference citations.
#pragma once

#include "match_kernels.hpp"

namespace nos {

// ---------------------------------------------------------------- batched registration: one problem per workgroup
//
// pipeline.scan_to_map runs OptimizePoseAnalytic's outer loop (MDM/tests/simple_optimization_test.cc:474-503) from the
// host: per round a match launch, an optional tail-drop launch, a solve launch and a host synchronisation.  Here workgroup b
// runs all rounds of problem b inside one launch.  Per round:
//   1. match: the lanes stride over scan b's points, each through match_point (match_kernels.hpp: the body of
//      match_kernel and, instantiated for the live voxel store's view, of voxel_match_kernel) into the problem's
//      scratch dataset — the layout nos_ndt_match gives a dataset of 2n slots of that element type;
//   2. count the matches (integer workgroup sum) and, with keep_multiple = k > 0, clear the last matches % k non-empty
//      records (drop_last_records, drop_last_matches_kernel's body);
//   3. make the loop state with the LmInit6 / LmInit3 call of the lone solve and run single_block_loop, the loop of
//      solve_single_block_kernel, over the (2n + 511) / 512 chunks;
//   4. lane 0 writes the pose back as the drop-in classes do and runs scan_to_map's stopping test.
// A scan of ≤ 512 points is exactly what the lone solve runs in one workgroup, so such a row ends with the bits of
// scan_to_map.  No workgroup waits for another: any B is safe, the ones that are not resident queue in the dispatcher.
template <typename Params>
struct RegisterDesc {
  TiledLayout L;          // the problem's scratch dataset (L.base = its storage): 2 slots per scan point, kNdtStored planes
  Params P;               // item parameters: the loss (the pose is set by the loop)
  const double* points;   // the scan: 3 planes of n_points doubles (nos_scan::d_planes)
  uint64_t n_points;
  uint32_t n_chunks;      // (max(2 n, 1) + 511) / 512, as the lone solve launches it
  int dof;                // 6 or 3
  double R[9], t[3];      // start pose (full 3-D pose for both dof)
  nos_host::LmSettings settings;
};

// What workgroup b leaves behind (plain stores; the host copies the whole array back once).
struct RegisterResult {
  double R[9], t[3];  // final pose (a failed round leaves the pose from before it)
  int outer_iter;     // scan_to_map's `outer`: the round that met the stopping test, max_outer if none did, the failed round
  int rounds;         // rounds run (log entries written), a failed one included
  int ok;             // 0: a round's solve failed (scan_to_map raises there)
  int probe_error;    // live store only: non-zero when a table probe ran through the whole table (the call then fails)
};

// One round of one problem: the layout of nos_register_round (include/nos.h).
struct RegisterRound {
  uint64_t matches, used;
  int32_t iterations, ok;
  double printed_cost, last_cost;
};

// LmInit6 as the host computes it: lm_solve makes the state on the host when no iteration runs (max_iterations = 0), and
// QuatToMatrix's `1 - (a b + c d)` and `a b ± c d` would be fused on the device.  QuatFromMatrix has no product that a
// sum follows, so it is called as it is.
__device__ __forceinline__ void lm_init6_host_order(nos_host::LmState* st, const double R[9], int float_schedule) {
#pragma clang fp contract(off)
  *st = nos_host::LmState();
  nos_host::LmInitSchedule(st, float_schedule);
  st->q = nos_host::QuatFromMatrix(R);
  const nos_host::Quat& q = st->q;
  const double tx = 2.0 * q.x, ty = 2.0 * q.y, tz = 2.0 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  st->R[0] = 1.0 - (tyy + tzz);
  st->R[1] = txy - twz;
  st->R[2] = txz + twy;
  st->R[3] = txy + twz;
  st->R[4] = 1.0 - (txx + tzz);
  st->R[5] = tyz - twx;
  st->R[6] = txz - twy;
  st->R[7] = tyz + twx;
  st->R[8] = 1.0 - (txx + tyy);
  st->done = 1;
}

// pipeline.scan_to_map's stopping test in its operation order: dR = Rᵀ R_last, dt = Rᵀ (t_last − t),
// |dt| < 1e-5 and _quat_vec_norm(dR) = sqrt(max(0, (1 − c) / 2)), c = clamp((trace dR − 1) / 2, −1, 1), < 1e-5.
__device__ __forceinline__ bool pose_converged(const double R[9], const double t[3], const double Rl[9], const double tl[3]) {
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) tr += R[i] * Rl[i] + R[3 + i] * Rl[3 + i] + R[6 + i] * Rl[6 + i];  // dR_ii
  const double d0 = tl[0] - t[0], d1 = tl[1] - t[1], d2 = tl[2] - t[2];
  double nn = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double dti = R[i] * d0 + R[3 + i] * d1 + R[6 + i] * d2;
    nn += dti * dti;
  }
  double c = (tr - 1.0) / 2.0;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  const double h = (1.0 - c) / 2.0;
  return sqrt(nn) < 1e-5 && sqrt(h > 0.0 ? h : 0.0) < 1e-5;
}

// Problem blockIdx.x of a batched registration, all rounds: the body of register_batch_kernel (below) and of
// register_live_kernel (assemble_register_live.hpp).  View: MapView or VoxelMatchView — match_point, a template over it,
// is the only line of a registration that depends on the kind of map; error: what it reports a failed table probe
// through (the live store's kInfoProbeError word; null for a snapshot).
template <typename Problem, typename T, int BLOCK, typename View>
__device__ __forceinline__ void register_problem(const View& map, unsigned int* __restrict__ error,
                                                 const RegisterDesc<typename Problem::Params>* __restrict__ descs,
                                                 RegisterResult* __restrict__ results, RegisterRound* __restrict__ round_log,
                                                 int max_outer, int max_neighbors, int keep_multiple) {
  constexpr int kOut = Problem::kOut;
  constexpr int kWaves = BLOCK / kWave;
  const RegisterDesc<typename Problem::Params>& d = descs[blockIdx.x];
  __shared__ double s_lm_raw[(sizeof(LmDevice) + 7) / 8];  // raw storage: the struct has default member initialisers
  LmDevice& s_lm = *reinterpret_cast<LmDevice*>(s_lm_raw);
  __shared__ double s_sum[kLmTotDoubles(kOut)];
  __shared__ double s_pose[12];                  // current pose: R (9, row-major) | t (3)
  __shared__ unsigned long long s_count[kWaves];  // matches per wave
  __shared__ int s_stop;
  const TiledLayout L = d.L;
  typename Problem::Params P = d.P;
  T* const data = static_cast<T*>(const_cast<void*>(L.base));  // the problem's own scratch: written here, read by the loop
  const double* const px = d.points;
  const double* const py = d.points + d.n_points;
  const double* const pz = d.points + 2 * d.n_points;
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (threadIdx.x < 12) s_pose[threadIdx.x] = threadIdx.x < 9 ? d.R[threadIdx.x] : d.t[threadIdx.x - 9];
  // the slots the loop reads beyond 2n (its last chunk) start cleared, as zero_pad leaves a matcher-written dataset
  const uint64_t read_end = uint64_t(d.n_chunks) * BLOCK;
  for (uint64_t i = L.n + threadIdx.x; i < read_end; i += BLOCK)
    for (int f = 0; f < kNdtStored; ++f) data[plane_offset(L, i, f)] = T(0);
  RegisterRound* const log = round_log + size_t(blockIdx.x) * size_t(max_outer);
  int outer = max_outer, rounds = 0, ok = 1;
  for (int round = 0; round < max_outer; ++round) {
    __syncthreads();  // s_pose of the previous round
    PosePod pose;
#pragma unroll
    for (int k = 0; k < 9; ++k) pose.R[k] = s_pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) pose.t[k] = s_pose[9 + k];
    // 1. match
    int found = 0;
    for (uint64_t i = threadIdx.x; i < d.n_points; i += BLOCK)
      found += match_point<T>(map, px, py, pz, i, pose, max_neighbors, L, data, error);
    // 2. count: wave sums, then every lane adds the kWaves partials in one order
    unsigned long long s = (unsigned long long)found;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, kWave);
    if (lane == 0) s_count[wave] = s;
    // Records written by other waves are read below (tail drop, then the loop).  All waves of this workgroup run on one CU
    // and share its vector L1, which the CU's own stores write through, and no other workgroup touches this problem's
    // scratch: each storing wave waits for its stores to complete (vmcnt(0)) and the barrier orders them before every
    // later load of the workgroup.  That is a workgroup-scope release / acquire; the agent-scope fences
    // (buffer_wbl2 / buffer_inv, ≈ 1.7 µs each) only matter for data that crosses CUs.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned long long matches = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) matches += s_count[w];
    const unsigned long long n_drop = keep_multiple > 0 ? matches % (unsigned long long)keep_multiple : 0ull;
    // 3. tail drop (one wave, as drop_last_matches_kernel), loop state, solve
    if (n_drop > 0) {
      if (wave == 0) drop_last_records<T>(data, L, n_drop, lane);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the cleared records, before the loop reads them (as above)
    }
    if (threadIdx.x == 0) {
      nos_host::LmState st;
      if (d.dof == 6) {
        // from LDS, not from `pose`: QuatFromMatrix indexes R at run time, which would put a register copy in scratch
        if (d.settings.max_iterations > 0) {
          nos_host::LmInit6(&st, s_pose, s_pose + 9, d.settings.max_iterations, d.settings.float_schedule);
        } else {
          lm_init6_host_order(&st, s_pose, d.settings.float_schedule);
          for (int k = 0; k < 3; ++k) st.t[k] = pose.t[k];
        }
      } else {  // MahalanobisDistanceMinimizerHip3DOF::RunLoop: the top-left 2x2 and (x, y)
        const double R2[4] = {pose.R[0], pose.R[1], pose.R[3], pose.R[4]};
        const double t2[2] = {pose.t[0], pose.t[1]};
        nos_host::LmInit3(&st, R2, t2, d.settings.max_iterations, d.settings.float_schedule);
      }
      s_lm.st = st;
      s_lm.settings = d.settings;
    }
    __syncthreads();
    single_block_loop<Problem, T, BLOCK, false>(L, P, d.n_chunks, s_lm, s_sum, nullptr, 0);
    // 4. write back, log, stopping test (the loop ends behind a barrier: s_lm is final)
    if (threadIdx.x == 0) {
      const nos_host::LmState st = s_lm.st;
      RegisterRound e;
      e.matches = matches;
      e.used = matches - n_drop;
      e.iterations = st.iteration;
      e.ok = st.ok;
      e.printed_cost = st.previous_cost;
      e.last_cost = st.cost;
      log[round] = e;
      int stop = 0;
      if (st.ok == 0) {  // SolveDataset returns false: scan_to_map raises, the pose stays
        ok = 0;
        stop = 1;
      } else {
        double Rn[9], tn[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) Rn[k] = pose.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tn[k] = pose.t[k];
        if (d.dof == 6) {  // WritePose
#pragma unroll
          for (int k = 0; k < 9; ++k) Rn[k] = st.R[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) tn[k] = st.t[k];
        } else {  // z, roll and pitch pass through
          Rn[0] = st.R[0];
          Rn[1] = st.R[1];
          Rn[3] = st.R[2];
          Rn[4] = st.R[3];
          tn[0] = st.t[0];
          tn[1] = st.t[1];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) s_pose[k] = Rn[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) s_pose[9 + k] = tn[k];
        stop = pose_converged(Rn, tn, pose.R, pose.t) ? 1 : 0;
      }
      s_stop = stop;
    }
    __syncthreads();
    rounds = round + 1;
    if (s_stop != 0) {  // block-uniform
      outer = round;
      break;
    }
  }
  if (threadIdx.x == 0) {
    RegisterResult& r = results[blockIdx.x];
#pragma unroll
    for (int k = 0; k < 9; ++k) r.R[k] = s_pose[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) r.t[k] = s_pose[9 + k];
    r.outer_iter = outer;
    r.rounds = rounds;
    r.ok = ok;
    // the probe-error word as this workgroup sees it after its last round: a probe of one of ITS lanes that failed is in
    // it (every round ends behind a barrier), so the host learns of every failure from the copy that brings the results
    r.probe_error = error != nullptr ? int(__hip_atomic_load(error, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : 0;
  }
}

template <typename Problem, typename T, int BLOCK>
__global__ __launch_bounds__(BLOCK) void register_batch_kernel(MapView map,
                                                              const RegisterDesc<typename Problem::Params>* __restrict__ descs,
                                                              RegisterResult* __restrict__ results,
                                                              RegisterRound* __restrict__ round_log, int max_outer,
                                                              int max_neighbors, int keep_multiple) {
  register_problem<Problem, T, BLOCK>(map, nullptr, descs, results, round_log, max_outer, max_neighbors, keep_multiple);
}

}  // namespace nos
