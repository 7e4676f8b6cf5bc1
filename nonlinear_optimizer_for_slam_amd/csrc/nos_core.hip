// nos_core.hip — launch selection, the accumulate entry points and the device-resident LM loop (C ABI of include/nos.h).
//
// The launch logic around the kernels in assemble_kernels.hpp.  There is no CPU fallback: without a usable HIP device
// every entry point fails with NOS_ERR_NO_DEVICE / NOS_ERR_HIP.
#include "nos_internal.hpp"

namespace nosd {

// ------------------------------------------------------------------ launch variants

// Host function of the hot-path kernel the current thread launched last (launch_variant / launch_single); copied into
// the device slot by launch_assemble_raw so that nos_ctx_last_kernel can name the instantiation that actually ran.
thread_local const void* t_last_kernel = nullptr;

template <typename Problem, typename T, int ITEMS, int BLOCK, int MINW, int PREFETCH = 0>
int launch_variant(const nos::TiledLayout& L, const typename Problem::Params& P, int grid_cap, int num_cus_hint,
                   bool nt, double* partials, const nos::FusedFinal& fin_in, hipStream_t stream, int* rows_out) {
  constexpr uint32_t kChunk = BLOCK * ITEMS;
  if (L.n_padded % kChunk != 0) return fail(NOS_ERR_INVALID_ARGUMENT, "n_padded %% chunk != 0");
  if (L.tile_stride != 0 && ((size_t(L.tile_mask) + 1) % kChunk) != 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "tile not a multiple of the kernel chunk");
  const uint64_t n_chunks64 = L.n_padded / kChunk;
  if (n_chunks64 > 0xFFFFFFFFull) return fail(NOS_ERR_UNSUPPORTED, "dataset too large for one shard");
  const uint32_t n_chunks = uint32_t(n_chunks64);
  int grid = int(std::min<uint64_t>(n_chunks, uint64_t(grid_cap)));
  if (grid < 1) grid = 1;
  if (grid > kMaxPartialRows) grid = kMaxPartialRows;
  nos::FusedFinal fin = fin_in;
  // write-through hand-off only in the geometry it is documented valid for: at most one workgroup per CU
  fin.write_through = (fin.counter != nullptr && grid <= num_cus_hint && fin_in.write_through != 0) ? 1 : 0;  // in: allowed (settings.sc1)
  const auto kernel = nt ? nos::assemble_kernel<Problem, T, ITEMS, BLOCK, MINW, true, PREFETCH>
                         : nos::assemble_kernel<Problem, T, ITEMS, BLOCK, MINW, false, PREFETCH>;
  t_last_kernel = reinterpret_cast<const void*>(kernel);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, stream, L, P, n_chunks, partials, fin);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NOS_ERR_HIP, "assemble launch failed: %s", hipGetErrorString(e));
  *rows_out = grid;
  return NOS_OK;
}

template <typename Problem, typename T>
int launch_by_variant(int variant, int blocks_per_cu, int num_cus, const nos::TiledLayout& L,
                      const typename Problem::Params& P, bool nt, double* partials, const nos::FusedFinal& fin,
                      hipStream_t stream, int* rows_out) {
  if (variant < 0 || variant >= kNumVariants) variant = 0;
#define NOS_CASE(idx, ITEMS_, BLOCK_, MINW_, BPC_)                                                  \
  case idx: {                                                                                       \
    const int bpc = blocks_per_cu > 0 ? blocks_per_cu : BPC_;                                       \
    return launch_variant<Problem, T, ITEMS_, BLOCK_, MINW_>(L, P, bpc * num_cus, num_cus, nt, partials, fin, stream, \
                                                             rows_out);                             \
  }
#define NOS_CASE_PP(idx, ITEMS_, BLOCK_, MINW_, BPC_)                                               \
  case idx: {                                                                                       \
    const int bpc = blocks_per_cu > 0 ? blocks_per_cu : BPC_;                                       \
    return launch_variant<Problem, T, ITEMS_, BLOCK_, MINW_, 3>(L, P, bpc * num_cus, num_cus, nt, partials, fin, \
                                                                stream, rows_out);                  \
  }
  // variant 0 = the library's choice for this problem / element type / layout (round 3, tools/exp/tune_stream.hip on
  // MI355X, profiles/r03_tune_*.txt):
  //   reprojection (5 planes: a chunk is only 40 B / 20 B per lane, so what a wave keeps in flight decides) — the ping-pong
  //     form, two named buffers and counted waits: fp64 21.3 -> 17.5 us per launch at 2 M, fp32 16.7 -> 14.5 us;
  //   NDT fp32 — 8-byte loads of two items, two waves per SIMD, no software prefetch: 89.0 us per launch at 10 M against
  //     100.5 us of round 2's prefetched form (its register copies forced full waits) and a loads-only floor of 89.8 us;
  //   NDT fp64 — one item per lane, 512-thread blocks (unchanged).
  // The default build carries the geometries something selects by default or a test drives; `make ALL_VARIANTS=1`
  // (-DNOS_ALL_VARIANTS) compiles every geometry ever tried for tools/tune_*.py and the geometry sweep test.
  constexpr bool kReproj = Problem::kFields == 5;
  if constexpr (sizeof(T) == 8) {
    if (variant == 0 && kReproj) variant = 7;
    switch (variant) {
      NOS_CASE(0, 1, 512, 3, 1)
      NOS_CASE(1, 1, 256, 3, 2)
      NOS_CASE(3, 2, 256, 2, 2)
      NOS_CASE_PP(7, 1, 512, kReproj ? 3 : 2, 1)   // ping-pong, one item per lane (two 15-plane buffers need the 256-register budget)
#ifdef NOS_ALL_VARIANTS
      NOS_CASE(2, 1, 256, 2, 2)
      NOS_CASE(4, 2, 512, 2, 1)
      NOS_CASE_PP(8, 2, 512, 2, 1)
#endif
    }
  } else {
    if (variant == 0) variant = kReproj ? 11 : 1;
    switch (variant) {
      NOS_CASE(1, 2, 512, 2, 1)      // 8-byte loads of two items, two waves per SIMD
      NOS_CASE_PP(11, 2, 512, 2, 1)  // ping-pong
#ifdef NOS_ALL_VARIANTS
      NOS_CASE(2, 1, 256, 4, 2)
      NOS_CASE(3, 2, 256, 5, 2)
      NOS_CASE(4, 2, 256, 4, 2)
      NOS_CASE(5, 1, 1024, 4, 1)  // four waves per SIMD, 4-byte loads
      NOS_CASE(6, 2, 1024, 4, 1)  // four waves per SIMD, 8-byte loads
      NOS_CASE(9, 2, 256, 3, 3)      // three waves per SIMD from three small workgroups per CU
      NOS_CASE_PP(12, 4, 512, 2, 1)
      NOS_CASE(13, 4, 256, 2, 1)     // round 1's default on planar planes: 16-byte loads, one wave per SIMD
#endif
    }
  }
#undef NOS_CASE
#undef NOS_CASE_PP
  return fail(NOS_ERR_UNSUPPORTED, "launch geometry %d is not compiled into this build for this element type "
              "(default build: fp64 0, 1, 3, 7; fp32 1, 11; `make ALL_VARIANTS=1` builds the rest)", variant);
}

// Correspondences a lane of the resident one-launch solve can hold (registers + LDS), by plane count and element type.
size_t resident_items_per_lane(int n_fields, int dtype) {
  if (n_fields == 15)
    return dtype == NOS_F64 ? size_t(nos::ResidentShape<15, 8>::RI + nos::ResidentShape<15, 8>::LI)
                            : size_t(nos::ResidentShape<15, 4>::RI + nos::ResidentShape<15, 4>::LI);
  if (n_fields == 5)
    return dtype == NOS_F64 ? size_t(nos::ResidentShape<5, 8>::RI + nos::ResidentShape<5, 8>::LI)
                            : size_t(nos::ResidentShape<5, 4>::RI + nos::ResidentShape<5, 4>::LI);
  return 1;
}

// Arguments of the single-workgroup whole-solve kernel (small problems, see nos::solve_single_block_kernel).
struct SingleBlockArgs {
  // cluster form (one chunk per workgroup, whole loop in one launch) when cluster_blocks > 0
  int cluster_blocks = 0;
  int items_per_lane = 1;  // correspondences every lane keeps resident (registers + LDS, nos::ResidentShape)
  int stream_chunks = 0;   // > 0: the streaming form (nothing resident; this many chunks of 512 x SI per iteration)
  bool nt = false;         // streaming form: non-temporal loads
  int stream_lds_chunks = 0;      // streaming form: chunks per workgroup kept in LDS after iteration 0
  int stream_reg_rounds = 0;      // streaming form: rounds per workgroup kept in vector registers after iteration 0
  bool stage1_sc1 = false; // keep stage 1 of the tagged all-reduce on sc1 stores even where a group sits on one XCD (lm_cluster 5)
  const nos::Mailbox* mail = nullptr;  // device-memory mailbox communicator: the cross-rank exchange runs inside the launch
  double* partials = nullptr;
  nos::ClusterCtl* ctl = nullptr;
  nos::LmDevice* lm;
  double* history;  // device address of the pinned cost history (may be null)
  int history_capacity;
  double* entry;    // device address of the pinned log entry
  unsigned long long* seq_host;
  unsigned long long seq;
};

template <typename Problem, typename T>
int launch_single(const nos::TiledLayout& L, const typename Problem::Params& P, const SingleBlockArgs& a, hipStream_t stream) {
  constexpr int kBlock = 512;
  if (L.n_padded % kBlock != 0) return fail(NOS_ERR_INVALID_ARGUMENT, "n_padded %% 512 != 0");
  if (a.cluster_blocks > 0 && a.stream_chunks > 0) {
    // the whole loop in one launch, the data streamed from HBM every iteration (solve_cluster_kernel, SI > 0)
    constexpr int kSI = sizeof(T) == 8 ? 1 : 2;        // fp64: 8-byte loads of one item; fp32: 8-byte loads of two
    // fp32 prefetched the next chunk through register copies in round 2 (the geometry of launch variant 8); the copies
    // force full waits, and with the LM step out of the kernel the plain form is the faster one (tools/exp/tune_stream.hip:
    // 89.0 against 100.5 us per pass at 10 M; loads-only floor 89.8)
    constexpr bool kSPF = false;
    constexpr size_t kChunk = size_t(kBlock) * kSI;
    if (L.n_padded % kChunk != 0 || (L.tile_stride != 0 && ((size_t(L.tile_mask) + 1) % kChunk) != 0))
      return fail(NOS_ERR_INVALID_ARGUMENT, "streaming solve: layout not a multiple of the %zu-item chunk", kChunk);
    if (size_t(a.stream_chunks) * kChunk != L.n_padded) return fail(NOS_ERR_INVALID_ARGUMENT, "streaming solve: chunk count does not match the layout");
    const auto kernel = a.nt ? nos::solve_cluster_kernel<Problem, T, kBlock, 0, 0, kSI, kSPF, true>
                             : nos::solve_cluster_kernel<Problem, T, kBlock, 0, 0, kSI, kSPF, false>;
    // chunks every workgroup keeps in LDS from iteration 1 on (the kernel clamps to its own chunk count)
    uint32_t lds = uint32_t(std::min(std::max(a.stream_lds_chunks, 0), 3));
    size_t dyn_bytes = lds * size_t(Problem::kFields) * kChunk * sizeof(T);
    if (dyn_bytes > size_t(48) * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            int(dyn_bytes)) != hipSuccess) {
      (void)hipGetLastError();  // LDS refused: stream everything, as without the option
      lds = 0;
      dyn_bytes = 0;
    }
    // rounds every workgroup keeps in registers from iteration 1 on (the kernel clamps to its own slot and round counts)
    const uint32_t reg = uint32_t(std::min(std::max(a.stream_reg_rounds, 0), nos::kStreamRegRoundsMax));
    t_last_kernel = reinterpret_cast<const void*>(kernel);
    hipLaunchKernelGGL(kernel, dim3(a.cluster_blocks), dim3(kBlock), dyn_bytes, stream, L, P, a.partials, a.lm, a.ctl, a.history,
                       a.history_capacity, a.entry, a.seq_host, a.seq, uint32_t(a.stream_chunks) | (a.stage1_sc1 ? 0x80000000u : 0u),
                       a.mail, lds, reg);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(NOS_ERR_HIP, "streaming solve launch failed: %s", hipGetErrorString(e));
    return NOS_OK;
  }
  if (a.cluster_blocks > 0) {
    using Shape = nos::ResidentShape<Problem::kPlanes, int(sizeof(T))>;
    if (a.items_per_lane < 1 || a.items_per_lane > Shape::RI + Shape::LI)
      return fail(NOS_ERR_INVALID_ARGUMENT, "resident solve: %d items per lane do not fit (%d + %d)", a.items_per_lane,
                  Shape::RI, Shape::LI);
    const auto kernel = nos::solve_cluster_kernel<Problem, T, kBlock, Shape::RI, Shape::LI>;
    const size_t lds_items = a.items_per_lane > Shape::RI ? size_t(a.items_per_lane - Shape::RI) : 0;
    const size_t dyn_bytes = lds_items * size_t(Problem::kFields) * kBlock * sizeof(T);
    // Dynamic LDS beyond the default limit has to be granted per kernel AND per device (the attribute belongs to the
    // function on the current device): asked for on every launch that needs it — a host-side call of about a microsecond,
    // once per solve — instead of remembered in a process-wide static that a second device or thread would trip over.
    if (dyn_bytes > size_t(48) * 1024) {
      const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, int(dyn_bytes));
      // NOS_ERR_UNSUPPORTED: the one status for which lm_solve falls back to the launch-per-iteration loop
      if (ea != hipSuccess) return fail(NOS_ERR_UNSUPPORTED, "resident solve: %zu bytes of LDS refused: %s", dyn_bytes, hipGetErrorString(ea));
    }
    t_last_kernel = reinterpret_cast<const void*>(kernel);
    hipLaunchKernelGGL(kernel, dim3(a.cluster_blocks), dim3(kBlock), dyn_bytes, stream, L, P, a.partials, a.lm, a.ctl,
                       a.history, a.history_capacity, a.entry, a.seq_host, a.seq,
                       uint32_t(a.items_per_lane) | (a.stage1_sc1 ? 0x80000000u : 0u), a.mail, 0u, 0u);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(NOS_ERR_HIP, "cluster solve launch failed: %s", hipGetErrorString(e));
    return NOS_OK;
  }
  const uint32_t n_chunks = uint32_t((std::max<uint64_t>(L.n, 1) + kBlock - 1) / kBlock);  // pads beyond are never read
  t_last_kernel = reinterpret_cast<const void*>(&nos::solve_single_block_kernel<Problem, T, kBlock>);
  hipLaunchKernelGGL((nos::solve_single_block_kernel<Problem, T, kBlock>), dim3(1), dim3(kBlock), 0, stream, L, P, n_chunks, a.lm,
                     a.history, a.history_capacity, a.entry, a.seq_host, a.seq);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NOS_ERR_HIP, "single-workgroup solve launch failed: %s", hipGetErrorString(e));
  return NOS_OK;
}

template <template <typename, int> class ProblemT, typename T, typename ParamsT>
int launch_by_loss(int loss_kind, int variant, int blocks_per_cu, int num_cus,
                   const nos::TiledLayout& L, const ParamsT& P, bool nt, double* partials,
                   const nos::FusedFinal& fin, hipStream_t stream, int* rows_out, const SingleBlockArgs* single = nullptr) {
  return with_loss(loss_kind, [&](auto loss) {
    using Problem = ProblemT<T, decltype(loss)::value>;
    if (single) return launch_single<Problem, T>(L, P, *single, stream);
    return launch_by_variant<Problem, T>(variant, blocks_per_cu, num_cus, L, P, nt, partials, fin, stream, rows_out);
  });
}

int check_loss(const nos_loss* loss, int* kind_out) {
  int kind = loss ? loss->kind : NOS_LOSS_NONE;
  if (kind < NOS_LOSS_NONE || kind > NOS_LOSS_HUBER) return fail(NOS_ERR_INVALID_ARGUMENT, "unknown loss kind %d", kind);
  // same argument checks as the reference constructors (loss_function.h:24-25, 53-54)
  if (kind == NOS_LOSS_EXPONENTIAL && (loss->a < 0.0 || loss->b < 0.0))
    return fail(NOS_ERR_INVALID_ARGUMENT, "exponential loss needs c1 >= 0 and c2 >= 0");
  if (kind == NOS_LOSS_HUBER && !(loss->a > 0.0)) return fail(NOS_ERR_INVALID_ARGUMENT, "huber loss needs threshold > 0");
  *kind_out = kind;
  return NOS_OK;
}

// Streaming (non-temporal) loads when the shard cannot stay resident in the 256 MiB
// Infinity Cache between iterations; default-policy loads when it can.
bool use_nontemporal(const nos_dataset* ds, const Shard& sh) {
  const int force = ds->ctx->settings.nt;
  if (force >= 0) return force != 0;
  return sh.bytes > (size_t(192) << 20);
}

// One flat problem in one element type: its item parameters from the request, then the launch by loss.
template <template <typename, int> class ProblemT, typename T>
int launch_flat(const nos_dataset* ds, const Shard& sh, const Request& rq, double* partials, const nos::FusedFinal& fin,
                hipStream_t stream, int* rows_out, const SingleBlockArgs* single) {
  const nos_ctx* ctx = ds->ctx;
  typename ProblemT<T, nos::kLossNone>::Params P{};
  fill_params(P, rq, ds);
  return launch_by_loss<ProblemT, T>(rq.loss_kind, ctx->variant, ctx->blocks_per_cu, ctx->slots[sh.slot].num_cus, sh.layout, P,
                                     use_nontemporal(ds, sh), partials, fin, stream, rows_out, single);
}

int launch_assemble_inner(const nos_dataset* ds, const Shard& sh, const Request& rq, double* partials,
                          const nos::FusedFinal& fin_in, hipStream_t stream, int* rows_out, const SingleBlockArgs* single) {
  nos::FusedFinal fin = fin_in;
  fin.write_through = ds->ctx->settings.sc1;  // "allowed"; the launcher keeps it only for the geometry it is valid for
  if (ds->kind == kKindNdtIndexed) return launch_indexed(ds, sh, rq, partials, fin, stream, rows_out);
  const bool f64 = ds->dtype == NOS_F64;
  if (rq.problem == 6)
    return f64 ? launch_flat<nos::Ndt6Problem, double>(ds, sh, rq, partials, fin, stream, rows_out, single)
               : launch_flat<nos::Ndt6Problem, float>(ds, sh, rq, partials, fin, stream, rows_out, single);
  if (rq.problem == 3)
    return f64 ? launch_flat<nos::Ndt3Problem, double>(ds, sh, rq, partials, fin, stream, rows_out, single)
               : launch_flat<nos::Ndt3Problem, float>(ds, sh, rq, partials, fin, stream, rows_out, single);
  return f64 ? launch_flat<nos::ReprojProblem, double>(ds, sh, rq, partials, fin, stream, rows_out, single)
             : launch_flat<nos::ReprojProblem, float>(ds, sh, rq, partials, fin, stream, rows_out, single);
}

int launch_assemble_raw(const nos_dataset* ds, const Shard& sh, const Request& rq, double* partials,
                        const nos::FusedFinal& fin_in, hipStream_t stream, int* rows_out,
                        const SingleBlockArgs* single = nullptr) {
  t_last_kernel = nullptr;
  const int rc = launch_assemble_inner(ds, sh, rq, partials, fin_in, stream, rows_out, single);
  if (rc == NOS_OK && t_last_kernel != nullptr) ds->ctx->slots[sh.slot].last_kernel = t_last_kernel;
  return rc;
}

// Launches the assemble kernel; with profiling on, brackets it with an event pair on the
// same stream so its device duration can be read back later without perturbing the loop.
int launch_assemble(const nos_dataset* ds, const Shard& sh, const Request& rq, double* partials,
                    const nos::FusedFinal& fin, hipStream_t stream, int* rows_out) {
  DeviceSlot& slot = ds->ctx->slots[sh.slot];
  if (slot.prof_on && slot.prof_every == 0) ++slot.prof_launches;  // bracket form: count only
  const bool prof = slot.prof_on && slot.prof_every > 0 && (slot.prof_launches++ % slot.prof_every) == 0 &&
                    slot.prof_used + 2 <= slot.prof_events.size();
  if (prof) NOS_HIP_CHECK(hipEventRecord(slot.prof_events[slot.prof_used], stream));
  const int rc = launch_assemble_raw(ds, sh, rq, partials, fin, stream, rows_out);
  if (rc != NOS_OK) return rc;
  if (prof) {
    NOS_HIP_CHECK(hipEventRecord(slot.prof_events[slot.prof_used + 1], stream));
    slot.prof_used += 2;
  }
  return NOS_OK;
}

int launch_final(int n_out, const double* partials, int rows, double* out, hipStream_t stream) {
  if (n_out == 28)
    hipLaunchKernelGGL((nos::final_reduce_kernel<28>), dim3(1), dim3(1024), 0, stream, partials, uint32_t(rows), out);
  else
    hipLaunchKernelGGL((nos::final_reduce_kernel<10>), dim3(1), dim3(1024), 0, stream, partials, uint32_t(rows), out);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(NOS_ERR_HIP, "final reduce launch failed: %s", hipGetErrorString(e));
  return NOS_OK;
}

int build_request(int problem, const nos_dataset* ds, const double* R, int nR, const double* t, int nt,
                  const double* intr, double min_depth, const nos_loss* loss, Request* rq) {
  if (!ds) return fail(NOS_ERR_INVALID_ARGUMENT, "dataset is NULL");
  if (!R || !t) return fail(NOS_ERR_INVALID_ARGUMENT, "pose pointer is NULL");
  const int want_kind = (problem == 2) ? kKindReproj : kKindNdt;
  if (ds->kind != want_kind && !(want_kind == kKindNdt && ds->kind == kKindNdtIndexed))
    return fail(NOS_ERR_WRONG_KIND, "dataset kind does not match the entry point");
  memset(rq, 0, sizeof *rq);
  rq->problem = problem;
  for (int k = 0; k < nR; ++k) rq->R[k] = R[k];
  for (int k = 0; k < nt; ++k) rq->t[k] = t[k];
  if (problem == 2) {
    if (!intr) return fail(NOS_ERR_INVALID_ARGUMENT, "intrinsics pointer is NULL");
    for (int k = 0; k < 4; ++k) rq->intr[k] = intr[k];
    rq->min_depth = min_depth;
  }
  int kind = 0;
  int rc = check_loss(loss, &kind);
  if (rc != NOS_OK) return rc;
  rq->loss_kind = kind;
  if (loss) rq->loss = *loss;
  rq->n_out = (problem == 3) ? 10 : 28;
  return NOS_OK;
}


// Device result → pinned host block + sequence word (used after an RCCL all-reduce, where the
// in-launch final reduce cannot write to the host itself).
__global__ void publish_kernel(const double* __restrict__ src, int n, double* dst_host,
                               unsigned long long* seq_host, unsigned long long seq) {
  if (int(threadIdx.x) < n)
    __hip_atomic_store(dst_host + threadIdx.x, src[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(seq_host, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Mailbox descriptor for the in-launch cross-rank exchange (base == null when the context has no shm communicator).
nos::Mailbox mailbox_of(const nos_ctx* ctx, const DeviceSlot& slot) {
  nos::Mailbox mb{};
  if (ctx->shm_dev == nullptr) return mb;
  mb.base = ctx->shm_dev;
  mb.peers = ctx->d_peers;  // null: the slots are the host-memory ones behind `base`
  mb.round = ctx->d_round;
  mb.error_host = reinterpret_cast<unsigned int*>(slot.h_out_dev + kCommErrorSlot);
  mb.n_ranks = ctx->comm_ranks;
  mb.rank = ctx->comm_rank;
  return mb;
}

int check_mailbox_error(const nos_ctx* ctx, DeviceSlot& slot) {
  if (ctx->shm_dev == nullptr) return NOS_OK;
  volatile unsigned int* err = reinterpret_cast<volatile unsigned int*>(slot.h_out + kCommErrorSlot);
  if (*err != 0u) {
    *err = 0u;
    return fail(NOS_ERR_HIP, "mailbox all-reduce timed out: a peer rank did not arrive (ranks must run the same sequence of calls)");
  }
  return NOS_OK;
}

// Spins on the host-mapped sequence word the last block stores after the result, for at most max_spins looks at it; true
// once the word has reached `want` (with the acquire fence that makes what the launch wrote before it visible).
bool spin_for_sequence(DeviceSlot& slot, unsigned long long want, long max_spins) {
  volatile unsigned long long* seq = reinterpret_cast<volatile unsigned long long*>(slot.h_out + kSeqSlot);
  for (long spins = 0; spins < max_spins; ++spins) {
    if (*seq >= want) {
      __atomic_thread_fence(__ATOMIC_ACQUIRE);
      return true;
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  return false;
}

// Falls back to a stream synchronise if the word has not arrived after a generous bound, so a protocol
// error can never hang the caller.
int wait_for_sequence(DeviceSlot& slot, unsigned long long want) {
  if (spin_for_sequence(slot, want, 2000000)) return NOS_OK;
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  if (!spin_for_sequence(slot, want, 1)) return fail(NOS_ERR_HIP, "fused final reduce did not publish its sequence word");
  return NOS_OK;
}
int wait_for_sequence(DeviceSlot& slot) { return wait_for_sequence(slot, slot.seq); }

// Blocking accumulate over every shard; shard sums are added on the host in shard order
// (the reference sums its per-thread partials the same way).
int accumulate_sync(nos_dataset* ds, const Request& rq, double* out) {
  nos_ctx* ctx = ds->ctx;
  const bool fused = ctx->settings.fused != 0 || ctx->shm_dev != nullptr;  // the mailbox exchange lives in the fused tail
  if (ctx->comm != nullptr) {
    // one process per GPU: local sums → RCCL all-reduce of the n_out doubles (in place, on the
    // same stream) → publish to pinned host memory.  Every rank receives identical bits.
    const Shard& sh = ds->shards[0];
    DeviceSlot& slot = ctx->slots[sh.slot];
    NOS_HIP_CHECK(hipSetDevice(slot.device));
    int rows = 0;
    nos::FusedFinal fin{slot.counter, slot.d_out, nullptr, nullptr, 0};
    int rc = launch_assemble(ds, sh, rq, slot.partials, fin, slot.stream, &rows);
    if (rc != NOS_OK) return rc;
    NOS_RCCL_CHECK(Rccl()->AllReduce(slot.d_out, slot.d_out, size_t(rq.n_out), ncclDouble, ncclSum, ctx->comm,
                                     slot.stream));
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(64), 0, slot.stream, slot.d_out, rq.n_out, slot.h_out_dev,
                       reinterpret_cast<unsigned long long*>(slot.h_out_dev + kSeqSlot), ++slot.seq);
    NOS_HIP_CHECK(hipGetLastError());
    rc = wait_for_sequence(slot);
    if (rc != NOS_OK) return rc;
    for (int k = 0; k < rq.n_out; ++k) out[k] = slot.h_out[k];
    return NOS_OK;
  }
  for (const Shard& sh : ds->shards) {
    DeviceSlot& slot = ctx->slots[sh.slot];
    NOS_HIP_CHECK(hipSetDevice(slot.device));
    int rows = 0;
    if (fused) {
      // one launch: the last block to finish reduces all rows and writes the result plus a
      // sequence word straight into pinned host memory (no second kernel, no memcpy)
      nos::FusedFinal fin{slot.counter, nullptr, slot.h_out_dev,
                          reinterpret_cast<unsigned long long*>(slot.h_out_dev + kSeqSlot), ++slot.seq};
      fin.mail = ctx->d_mail;
      int rc = launch_assemble(ds, sh, rq, slot.partials, fin, slot.stream, &rows);
      if (rc != NOS_OK) return rc;
    } else {
      int rc = launch_assemble(ds, sh, rq, slot.partials, nos::FusedFinal{}, slot.stream, &rows);
      if (rc != NOS_OK) return rc;
      rc = launch_final(rq.n_out, slot.partials, rows, slot.d_out, slot.stream);
      if (rc != NOS_OK) return rc;
      NOS_HIP_CHECK(hipMemcpyAsync(slot.h_out, slot.d_out, sizeof(double) * rq.n_out, hipMemcpyDeviceToHost, slot.stream));
    }
  }
  for (int k = 0; k < rq.n_out; ++k) out[k] = 0.0;
  for (const Shard& sh : ds->shards) {
    DeviceSlot& slot = ctx->slots[sh.slot];
    if (fused) {
      int rc = wait_for_sequence(slot);
      if (rc == NOS_OK) rc = check_mailbox_error(ctx, slot);
      if (rc != NOS_OK) return rc;
    } else {
      NOS_HIP_CHECK(hipSetDevice(slot.device));
      NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
    }
    for (int k = 0; k < rq.n_out; ++k) out[k] += slot.h_out[k];
  }
  return NOS_OK;
}

int accumulate_async(nos_dataset* ds, const Request& rq, double* d_out) {
  if (!d_out) return fail(NOS_ERR_INVALID_ARGUMENT, "d_out is NULL");
  if (ds->shards.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "async accumulate needs a single-device context");
  nos_ctx* ctx = ds->ctx;
  const Shard& sh = ds->shards[0];
  DeviceSlot& slot = ctx->slots[sh.slot];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  int rows = 0;
  if (ctx->comm != nullptr) {
    nos::FusedFinal fin{slot.counter, d_out, nullptr, nullptr, 0};
    int rc = launch_assemble(ds, sh, rq, slot.partials, fin, slot.stream, &rows);
    if (rc != NOS_OK) return rc;
    NOS_RCCL_CHECK(Rccl()->AllReduce(d_out, d_out, size_t(rq.n_out), ncclDouble, ncclSum, ctx->comm, slot.stream));
    return NOS_OK;
  }
  if (ctx->settings.fused != 0 || ctx->shm_dev != nullptr) {
    nos::FusedFinal fin{slot.counter, d_out, nullptr, nullptr, 0};
    fin.mail = ctx->d_mail;
    return launch_assemble(ds, sh, rq, slot.partials, fin, slot.stream, &rows);
  }
  int rc = launch_assemble(ds, sh, rq, slot.partials, nos::FusedFinal{}, slot.stream, &rows);
  if (rc != NOS_OK) return rc;
  return launch_final(rq.n_out, slot.partials, rows, d_out, slot.stream);
}

int time_kernel(nos_dataset* ds, const Request& rq, int repeats, double* kernel_ms, double* total_ms) {
  if (repeats < 1) repeats = 1;
  nos_ctx* ctx = ds->ctx;
  const Shard& sh = ds->shards[0];
  DeviceSlot& slot = ctx->slots[sh.slot];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  int rows = 0;
  // warm-up
  const bool fused = ctx->settings.fused != 0;
  for (int i = 0; i < 2; ++i) {
    int rc = launch_assemble(ds, sh, rq, slot.partials, nos::FusedFinal{}, slot.stream, &rows);
    if (rc != NOS_OK) return rc;
  }
  NOS_HIP_CHECK(hipEventRecord(slot.ev0, slot.stream));
  for (int i = 0; i < repeats; ++i) {
    int rc = launch_assemble(ds, sh, rq, slot.partials, nos::FusedFinal{}, slot.stream, &rows);
    if (rc != NOS_OK) return rc;
  }
  NOS_HIP_CHECK(hipEventRecord(slot.ev1, slot.stream));
  for (int i = 0; i < repeats; ++i) {
    if (fused) {
      nos::FusedFinal fin{slot.counter, slot.d_out, nullptr, nullptr, 0};
      int rc = launch_assemble(ds, sh, rq, slot.partials, fin, slot.stream, &rows);
      if (rc != NOS_OK) return rc;
    } else {
      int rc = launch_assemble(ds, sh, rq, slot.partials, nos::FusedFinal{}, slot.stream, &rows);
      if (rc != NOS_OK) return rc;
      rc = launch_final(rq.n_out, slot.partials, rows, slot.d_out, slot.stream);
      if (rc != NOS_OK) return rc;
    }
  }
  NOS_HIP_CHECK(hipEventRecord(slot.ev2, slot.stream));
  NOS_HIP_CHECK(hipEventSynchronize(slot.ev2));
  float ms01 = 0.f, ms12 = 0.f;
  NOS_HIP_CHECK(hipEventElapsedTime(&ms01, slot.ev0, slot.ev1));
  NOS_HIP_CHECK(hipEventElapsedTime(&ms12, slot.ev1, slot.ev2));
  if (kernel_ms) *kernel_ms = double(ms01) / repeats;
  if (total_ms) *total_ms = double(ms12) / repeats;
  return NOS_OK;
}

// ------------------------------------------------------------------ device-resident LM loop (nos_*_solve)

// Host mirror of the loop state and the device's copy of it (lm_init_kernel), both from the same arguments.
int lm_init(DeviceSlot& slot, const nos::LmInitArgs& init, nos_host::LmState* st) {
  if (init.dof == 6)
    nos_host::LmInit6(st, init.R, init.t, init.settings.max_iterations, init.settings.float_schedule);
  else
    nos_host::LmInit3(st, init.R, init.t, init.settings.max_iterations, init.settings.float_schedule);
  hipLaunchKernelGGL(nos::lm_init_kernel, dim3(1), dim3(1), 0, slot.stream, slot.d_lm, init);
  NOS_HIP_CHECK(hipGetLastError());
  return NOS_OK;
}

// The loop state a pinned log entry carries (layout: assemble_loop.hpp).
void read_log_entry(const double* e, nos_host::LmState* st) {
  for (int k = 0; k < 9; ++k) st->R[k] = e[nos::kLogR + k];
  for (int k = 0; k < 3; ++k) st->t[k] = e[nos::kLogT + k];
  st->lambda = e[nos::kLogLambda];
  st->previous_cost = e[nos::kLogPrevCost];
  st->cost = e[nos::kLogCost];
  st->iteration = int(e[nos::kLogIteration]);
  st->done = int(e[nos::kLogDone]);
  st->ok = int(e[nos::kLogOk]);
}

// Cost history of a one-launch form: the kernel wrote one cost per executed iteration into the pinned history block.
void copy_history(const nos_lm_options* opt, const DeviceSlot& slot, int executed) {
  if (opt->cost_history != nullptr)
    for (int k = 0; k < executed && k < opt->max_iterations; ++k) opt->cost_history[k] = slot.h_hist[k];
}

void write_report(nos_lm_report* report, const nos_host::LmState& st, int launches, int fallback) {
  if (!report) return;
  report->iterations = st.iteration;
  report->ok = st.ok;
  report->launches = launches;
  report->fallback = fallback;
  report->printed_cost = st.previous_cost;
  report->last_cost = st.cost;
  report->final_lambda = st.lambda;
}

// Small problems: the whole loop in one workgroup and one launch (see nos::solve_single_block_kernel)
bool single_block_eligible(const nos_dataset* ds, const nos_lm_options* opt) {
  const nos_ctx* ctx = ds->ctx;
  const Shard& sh = ds->shards[0];
  const bool with_comm = ctx->comm != nullptr;
  return ds->kind != kKindNdtIndexed && !with_comm && ctx->shm_dev == nullptr && opt->max_iterations > 0 &&
         sh.layout.n * size_t(ds->n_fields) <= nos::kSingleBlockMaxElements && ctx->settings.lm_single != 0 &&
         (opt->cost_history == nullptr || opt->max_iterations <= kHistCapacity);
}

int solve_single_block(nos_dataset* ds, const Request& rq, const nos_lm_options* opt, nos_host::LmState* st) {
  const Shard& sh = ds->shards[0];
  DeviceSlot& slot = ds->ctx->slots[sh.slot];
  SingleBlockArgs single{};
  single.lm = slot.d_lm;
  single.history = opt->cost_history ? slot.h_hist_dev : nullptr;
  single.history_capacity = kHistCapacity;
  single.entry = slot.h_log_dev;
  single.seq_host = reinterpret_cast<unsigned long long*>(slot.h_out_dev + kSeqSlot);
  single.seq = ++slot.seq;
  int rows = 0;
  int rc = launch_assemble_raw(ds, sh, rq, slot.partials, nos::FusedFinal{}, slot.stream, &rows, &single);
  if (rc != NOS_OK) return rc;
  rc = wait_for_sequence(slot, single.seq);
  if (rc != NOS_OK) return rc;
  const double* e = slot.h_log;
  read_log_entry(e, st);
  const int executed = int(e[nos::kLogExecuted]);
  if (slot.prof_on && slot.prof_every == 0) slot.prof_launches += executed;  // bracket profiling counts passes over the data
  copy_history(opt, slot, executed);
  return NOS_OK;
}

// Whether this solve may try the one-launch cluster form, given its geometry (solve_cluster).
bool cluster_eligible(const nos_dataset* ds, const nos_lm_options* opt, bool mailbox_in_launch, size_t cluster_blocks,
                      bool resident_fits, bool stream_form, bool paused) {
  const nos_ctx* ctx = ds->ctx;
  const bool with_comm = ctx->comm != nullptr;
  return ds->kind != kKindNdtIndexed && !with_comm && (ctx->shm_dev == nullptr || mailbox_in_launch) && opt->max_iterations > 0 &&
         cluster_blocks >= 1 && (resident_fits || stream_form) && !paused &&
         ctx->settings.lm_cluster != 0 && (opt->cost_history == nullptr || opt->max_iterations <= kHistCapacity);
}

// Mid-size problems: one chunk per workgroup, every workgroup resident, the whole loop in one launch
// (nos::solve_cluster_kernel).  If a wait inside times out (grid not fully resident, e.g. the GPU is shared) the
// launch gives up and lm_solve runs the loop with one launch per iteration instead.
// *finished: the launch ran the loop to its end and *st is its result; otherwise the form was not eligible, or it gave up
// (*fell_back = 1) and left the device state re-initialised for the launch-per-iteration loop.
int solve_cluster(nos_dataset* ds, const Request& rq, const nos_lm_options* opt, const nos::LmInitArgs& init,
                  nos_host::LmState* st, bool* finished, int* fell_back) {
  nos_ctx* ctx = ds->ctx;
  const Shard& sh = ds->shards[0];
  DeviceSlot& slot = ctx->slots[sh.slot];
  *finished = false;
  // One 512-thread workgroup per CU at most (all of them must be resident at once); every lane keeps items_per_lane
  // correspondences in registers + LDS.  lm_cluster: 0 off, 1 on, 2 = only the one-item-per-lane form of round 1.
  // lm_cluster_max_blocks: rehearsals of several ranks on ONE GPU give every rank its share of the CUs (all workgroups of
  // all ranks have to be resident together)
  const size_t max_blocks = std::min<size_t>(std::min<size_t>(nos::kClusterMaxBlocks, size_t(slot.num_cus)),
                                             size_t(std::max(1, ctx->settings.lm_cluster_max_blocks)));
  // A device-memory mailbox communicator keeps the one-launch loop: its exchange is a third stage inside the launch
  // (solve_cluster_kernel).  RCCL and the host-memory mailbox run one launch per iteration, as before.
  const bool mailbox_in_launch = ctx->shm_dev != nullptr && ctx->d_peers != nullptr && ctx->d_mail != nullptr &&
                                 ds->kind != kKindNdtIndexed;
  const size_t cluster_blocks = std::min<size_t>(max_blocks, (sh.layout.n + 511) / 512);
  const size_t items_per_lane = cluster_blocks > 0 ? (sh.layout.n + cluster_blocks * 512 - 1) / (cluster_blocks * 512) : 0;
  const size_t resident_capacity = ctx->settings.lm_cluster == 2 ? 1 : resident_items_per_lane(ds->n_fields, ds->dtype);
  // Beyond what the chip can keep resident the same one-launch loop STREAMS the data every iteration (lm_cluster 1 only;
  // 4 = resident form only, as before).  The chunk count must fit the kernel's 32-bit counter.
  const size_t stream_chunk = size_t(512) * (ds->dtype == NOS_F64 ? 1 : 2);
  const bool resident_fits = items_per_lane >= 1 && items_per_lane <= resident_capacity;
  const bool stream_form = !resident_fits && (ctx->settings.lm_cluster == 1 || ctx->settings.lm_cluster == 5) && items_per_lane >= 1 &&
                           sh.layout.n_padded % stream_chunk == 0 && sh.layout.n_padded / stream_chunk < (size_t(1) << 31) &&
                           (sh.layout.tile_stride == 0 || (size_t(sh.layout.tile_mask) + 1) % stream_chunk == 0);
  bool paused = false;
  if (mailbox_in_launch) {
    paused = slot.cluster_paused_solves > 0;  // the same count on every rank (see DeviceSlot)
    if (paused) --slot.cluster_paused_solves;
  } else {
    if (slot.cluster_gave_up &&
        std::chrono::steady_clock::now() - slot.cluster_gave_up_at > std::chrono::milliseconds(ctx->settings.lm_cluster_retry_ms))
      slot.cluster_gave_up = false;  // try the one-launch form again
    paused = slot.cluster_gave_up;
  }
  if (!cluster_eligible(ds, opt, mailbox_in_launch, cluster_blocks, resident_fits, stream_form, paused)) return NOS_OK;
  SingleBlockArgs cl{};
  cl.cluster_blocks = int(cluster_blocks);
  cl.items_per_lane = int(items_per_lane);
  if (stream_form) {
    cl.items_per_lane = 0;
    cl.stream_chunks = int(sh.layout.n_padded / stream_chunk);
    cl.nt = use_nontemporal(ds, sh);
    cl.stream_lds_chunks = ctx->settings.stream_lds_chunks;
    cl.stream_reg_rounds = ctx->settings.stream_reg_rounds;
  }
  cl.stage1_sc1 = ctx->settings.lm_cluster == 5;
  cl.mail = mailbox_in_launch ? ctx->d_mail : nullptr;
  cl.partials = slot.partials;
  cl.ctl = slot.d_cluster;
  cl.lm = slot.d_lm;
  cl.history = opt->cost_history ? slot.h_hist_dev : nullptr;
  cl.history_capacity = kHistCapacity;
  cl.entry = slot.h_log_dev;
  cl.seq_host = reinterpret_cast<unsigned long long*>(slot.h_out_dev + kSeqSlot);
  cl.seq = ++slot.seq;
  // arrival counters and the abort word start every launch at zero
  NOS_HIP_CHECK(hipMemsetAsync(slot.d_cluster, 0, sizeof(nos::ClusterCtl), slot.stream));
  if (ctx->settings.debug_cluster_abort != 0) {  // test hook (nos_ctx_set_option): the launch finds `abort` already raised and gives up
    const unsigned int raised = 1u;
    NOS_HIP_CHECK(hipMemcpyAsync(&slot.d_cluster->abort, &raised, sizeof raised, hipMemcpyHostToDevice, slot.stream));
    NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  }
  int rows = 0;
  // A launch the device cannot take (the LDS grant refused: NOS_ERR_UNSUPPORTED) is replaced by the launch-per-iteration
  // loop; any other failure — a layout / argument error, a sticky HIP error — is the caller's to see, not a reason to run slower.
  const int rc_launch = launch_assemble_raw(ds, sh, rq, slot.partials, nos::FusedFinal{}, slot.stream, &rows, &cl);
  if (rc_launch != NOS_OK && rc_launch != NOS_ERR_UNSUPPORTED) return rc_launch;
  const bool launched_ok = rc_launch == NOS_OK;
  // spin on the sequence word; a launch that gave up never writes it
  *finished = launched_ok && spin_for_sequence(slot, cl.seq, 4000000);
  if (!*finished) {
    NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
    *finished = spin_for_sequence(slot, cl.seq, 1);
  }
  if (*finished) {
    slot.cluster_next_pause = 64;
    const double* e = slot.h_log;
    read_log_entry(e, st);
    const int executed = int(e[nos::kLogExecuted]);
#ifdef NOS_LM_TIMING
    fprintf(stderr, "[resident-timing] %d blocks x %d items/lane (0 = streamed), %d iterations; workgroup 0, us per iteration: item math %.2f, "
            "block reduce %.2f, drain+arrive+wait %.2f, rows->sums %.2f, LM step+barrier %.2f\n", cl.cluster_blocks,
            cl.items_per_lane, executed, e[50] * 0.01, e[51] * 0.01, e[52] * 0.01, e[53] * 0.01, e[54] * 0.01);
    fprintf(stderr, "[resident-timing]    inside the step, shader-clock cycles per iteration: elimination %.0f, back substitution %.0f, "
            "lane 0 (pose update, tests, schedule) %.0f\n", e[56], e[57], e[58]);
#endif
    if (slot.prof_on && slot.prof_every == 0) slot.prof_launches += executed;  // bracket profiling counts passes over the data
    copy_history(opt, slot, executed);
    return NOS_OK;
  }
  // gave up: put the shared words back in order and leave the solve to the launch-per-iteration loop from the start
  // (reported as nos_lm_report::fallback).  A launch that ran and timed out means the GPU is shared: remember it for a
  // while, so the next solves on this device do not each pay the bounded wait before falling back ("lm_cluster_retry_ms";
  // debug_cluster_abort = 2 is the test hook that leaves this latch active).  A launch the device refused sets no latch,
  // and the text of its refusal is dropped: the call goes on to succeed.
  *fell_back = 1;
  if (launched_ok && ctx->settings.debug_cluster_abort != 1) {
    if (mailbox_in_launch) {
      slot.cluster_paused_solves = slot.cluster_next_pause;
      slot.cluster_next_pause = std::min(slot.cluster_next_pause * 2, 65536);
    } else {
      slot.cluster_gave_up = true;
      slot.cluster_gave_up_at = std::chrono::steady_clock::now();
    }
  }
  if (!launched_ok) clear_last_error();
  if (mailbox_in_launch) {
    // every rank gives up together (a rank that cannot go on tells its peers); the exchange rounds the abandoned launch
    // may have used are skipped on every rank, so that no later round finds their granules
    hipLaunchKernelGGL(nos::mailbox_skip_rounds_kernel, dim3(1), dim3(1), 0, slot.stream, ctx->d_round,
                       (unsigned long long)opt->max_iterations + 1ull);
    NOS_HIP_CHECK(hipGetLastError());
  }
  NOS_HIP_CHECK(hipMemsetAsync(slot.d_cluster, 0, sizeof(nos::ClusterCtl), slot.stream));
  return lm_init(slot, init, st);
}

// Any size, any communicator: one launch per iteration.  The host keeps `window` launches in flight and reads one pinned
// log entry per finished iteration; nothing on the host sits between two consecutive kernels.  With an RCCL communicator
// every launch is followed by the all-reduce of its sums and a one-wave step kernel, so all ranks advance identical states
// in lock-step without host synchronisation either.
int solve_per_iteration(nos_dataset* ds, const Request& rq, const nos_lm_options* opt, nos_host::LmState* st, int* launches) {
  nos_ctx* ctx = ds->ctx;
  const Shard& sh = ds->shards[0];
  DeviceSlot& slot = ctx->slots[sh.slot];
  const bool with_comm = ctx->comm != nullptr;
  const bool step_in_launch = !with_comm && ctx->settings.lm_fused != 0;
  int window = opt->launches_in_flight > 0 ? opt->launches_in_flight : ctx->settings.lm_window;
  window = std::max(1, std::min(window, kLogSlots - 2));
  unsigned long long* seq_dev = reinterpret_cast<unsigned long long*>(slot.h_out_dev + kSeqSlot);
  const unsigned long long base_seq2 = slot.seq;
  int launched = 0, completed = 0;
  auto launch_one = [&]() -> int {
    double* entry = slot.h_log_dev + size_t(launched % kLogSlots) * nos::kLogEntryDoubles;
    int rows = 0;
    nos::FusedFinal fin{};
    fin.counter = slot.counter;
    fin.lm = slot.d_lm;
    fin.seq = ++slot.seq;
    fin.mail = ctx->d_mail;
    if (step_in_launch) {
      fin.out_host = entry;
      fin.seq_host = seq_dev;
      fin.lm_step = 1;
      int rc = launch_assemble(ds, sh, rq, slot.partials, fin, slot.stream, &rows);
      if (rc != NOS_OK) return rc;
    } else {
      fin.out_dev = slot.d_out;
      int rc = launch_assemble(ds, sh, rq, slot.partials, fin, slot.stream, &rows);
      if (rc != NOS_OK) return rc;
      if (with_comm)
        NOS_RCCL_CHECK(Rccl()->AllReduce(slot.d_out, slot.d_out, size_t(rq.n_out), ncclDouble, ncclSum, ctx->comm,
                                         slot.stream));
      if (rq.n_out == 28)
        hipLaunchKernelGGL((nos::lm_step_kernel<28>), dim3(1), dim3(64), 0, slot.stream, slot.d_out, slot.d_lm, entry,
                           seq_dev, fin.seq);
      else
        hipLaunchKernelGGL((nos::lm_step_kernel<10>), dim3(1), dim3(64), 0, slot.stream, slot.d_out, slot.d_lm, entry,
                           seq_dev, fin.seq);
      NOS_HIP_CHECK(hipGetLastError());
    }
    ++launched;
    return NOS_OK;
  };
  int rc = NOS_OK;
  while (rc == NOS_OK && launched < std::min(window, opt->max_iterations)) rc = launch_one();
  while (rc == NOS_OK && completed < launched) {
    rc = wait_for_sequence(slot, base_seq2 + completed + 1);
    if (rc == NOS_OK) rc = check_mailbox_error(ctx, slot);
    if (rc != NOS_OK) break;
    if (!st->done) {
      const double* e = slot.h_log + size_t(completed % kLogSlots) * nos::kLogEntryDoubles;
      if (opt->cost_history != nullptr && completed < opt->max_iterations) opt->cost_history[completed] = e[rq.n_out - 1];
      read_log_entry(e, st);
#ifdef NOS_LM_TIMING
      // wall_clock64 ticks (10 ns): start of the finishing workgroup, its ticket, step begin, step done, log written
      fprintf(stderr, "[lm-timing] it %d: loop+ticket %.2f us, rows->sums %.2f us, step %.2f us, log %.2f us\n", completed,
              (e[51] - e[50]) * 0.01, (e[52] - e[51]) * 0.01, (e[53] - e[52]) * 0.01, (e[54] - e[53]) * 0.01);
      if (ctx->shm_host != nullptr) {
        const double* mbx = static_cast<const double*>(ctx->shm_host) + size_t(ctx->comm_rank) * 2 * nos::kMailSlotDoubles;
        fprintf(stderr, "[lm-timing]        mailbox: store+flag %.2f us, poll %.2f us, gather %.2f us\n", mbx[40] * 0.01,
                mbx[41] * 0.01, mbx[42] * 0.01);
      }
      fprintf(stderr, "[lm-timing]        a block: prologue %.2f us, loads+math %.2f us, block reduce+store %.2f us\n",
              e[56] * 0.01, e[57] * 0.01, e[58] * 0.01);
#endif
    }
    ++completed;
    if (!st->done && launched < opt->max_iterations) rc = launch_one();
  }
  if (rc != NOS_OK) (void)hipStreamSynchronize(slot.stream);  // leave nothing in flight behind an error
  *launches = launched;
  return rc;
}

// Device-resident Levenberg-Marquardt loop (see nos::LmDevice) in the first form the solve is eligible for: the single
// workgroup, the one-launch cluster (resident or streamed), one launch per iteration.
int lm_solve(nos_dataset* ds, const Request& rq, const nos_lm_options* opt, double* R, int nR, double* t, int nt,
             nos_lm_report* report) {
  if (!opt) return fail(NOS_ERR_INVALID_ARGUMENT, "options pointer is NULL");
  if (ds->shards.size() != 1)
    return fail(NOS_ERR_UNSUPPORTED, "the device-resident loop needs a single-device context (use the host loop)");
  if (opt->max_iterations < 0) return fail(NOS_ERR_INVALID_ARGUMENT, "max_iterations < 0");
  DeviceSlot& slot = ds->ctx->slots[ds->shards[0].slot];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  const nos::LmInitArgs init = make_lm_init(ds, rq, opt, R, nR, t, nt);
  nos_host::LmState st;  // host mirror: what the log says after the last finished iteration
  int rc = lm_init(slot, init, &st);
  if (rc != NOS_OK) return rc;
  int launches = 1, fell_back = 0;
  if (single_block_eligible(ds, opt)) {
    rc = solve_single_block(ds, rq, opt, &st);
  } else {
    bool finished = false;
    rc = solve_cluster(ds, rq, opt, init, &st, &finished, &fell_back);
    if (rc == NOS_OK && !finished) rc = solve_per_iteration(ds, rq, opt, &st, &launches);
  }
  if (rc != NOS_OK) return rc;
  for (int k = 0; k < nR; ++k) R[k] = st.R[k];
  for (int k = 0; k < nt; ++k) t[k] = st.t[k];
  write_report(report, st, launches, fell_back);
  return NOS_OK;
}

// What the accumulate / solve / time entry points share: one call at a time per context, the request built and checked
// (its failure is reported before anything `run` checks), then the call itself.
template <typename Run>
int with_request(int problem, nos_dataset* ds, const double* R, int nR, const double* t, int nt, const double* intr,
                 double min_depth, const nos_loss* loss, Run run) {
  CtxGuard guard_(ds ? ds->ctx : nullptr);  // one solve / accumulate / create at a time per context
  Request rq;
  const int rc = build_request(problem, ds, R, nR, t, nt, intr, min_depth, loss, &rq);
  if (rc != NOS_OK) return rc;
  return run(rq);
}

}  // namespace nosd

using namespace nosd;

// ====================================================================== C ABI

extern "C" {

int nos_ndt6_accumulate(nos_dataset* ds, const double R[9], const double t[3], const nos_loss* loss,
                        double out28[NOS_NDT6_OUT]) {
  return with_request(6, ds, R, 9, t, 3, nullptr, 0.0, loss, [&](const Request& rq) {
    if (!out28) return fail(NOS_ERR_INVALID_ARGUMENT, "out28 is NULL");
    return accumulate_sync(ds, rq, out28);
  });
}

int nos_ndt3_accumulate(nos_dataset* ds, const double R2[4], const double t2[2], const nos_loss* loss,
                        double out10[NOS_NDT3_OUT]) {
  return with_request(3, ds, R2, 4, t2, 2, nullptr, 0.0, loss, [&](const Request& rq) {
    if (!out10) return fail(NOS_ERR_INVALID_ARGUMENT, "out10 is NULL");
    return accumulate_sync(ds, rq, out10);
  });
}

int nos_reproj_accumulate(nos_dataset* ds, const double R[9], const double t[3], const double intr[4],
                          const nos_loss* loss, double min_depth, double out28[NOS_REPROJ_OUT]) {
  return with_request(2, ds, R, 9, t, 3, intr, min_depth, loss, [&](const Request& rq) {
    if (!out28) return fail(NOS_ERR_INVALID_ARGUMENT, "out28 is NULL");
    return accumulate_sync(ds, rq, out28);
  });
}

int nos_ndt6_accumulate_async(nos_dataset* ds, const double R[9], const double t[3], const nos_loss* loss,
                              double* d_out28) {
  return with_request(6, ds, R, 9, t, 3, nullptr, 0.0, loss,
                      [&](const Request& rq) { return accumulate_async(ds, rq, d_out28); });
}

int nos_ndt3_accumulate_async(nos_dataset* ds, const double R2[4], const double t2[2], const nos_loss* loss,
                              double* d_out10) {
  return with_request(3, ds, R2, 4, t2, 2, nullptr, 0.0, loss,
                      [&](const Request& rq) { return accumulate_async(ds, rq, d_out10); });
}

int nos_reproj_accumulate_async(nos_dataset* ds, const double R[9], const double t[3], const double intr[4],
                                const nos_loss* loss, double min_depth, double* d_out28) {
  return with_request(2, ds, R, 9, t, 3, intr, min_depth, loss,
                      [&](const Request& rq) { return accumulate_async(ds, rq, d_out28); });
}

int nos_ndt6_solve(nos_dataset* ds, double R[9], double t[3], const nos_loss* loss, const nos_lm_options* options,
                   nos_lm_report* report) {
  return with_request(6, ds, R, 9, t, 3, nullptr, 0.0, loss,
                      [&](const Request& rq) { return lm_solve(ds, rq, options, R, 9, t, 3, report); });
}

int nos_ndt3_solve(nos_dataset* ds, double R2[4], double t2[2], const nos_loss* loss, const nos_lm_options* options,
                   nos_lm_report* report) {
  return with_request(3, ds, R2, 4, t2, 2, nullptr, 0.0, loss,
                      [&](const Request& rq) { return lm_solve(ds, rq, options, R2, 4, t2, 2, report); });
}

int nos_reproj_solve(nos_dataset* ds, double R[9], double t[3], const double intr[4], const nos_loss* loss,
                     double min_depth, const nos_lm_options* options, nos_lm_report* report) {
  return with_request(2, ds, R, 9, t, 3, intr, min_depth, loss,
                      [&](const Request& rq) { return lm_solve(ds, rq, options, R, 9, t, 3, report); });
}

int nos_ndt6_time_kernel(nos_dataset* ds, const double R[9], const double t[3], const nos_loss* loss, int repeats,
                         double* kernel_ms, double* total_ms) {
  return with_request(6, ds, R, 9, t, 3, nullptr, 0.0, loss,
                      [&](const Request& rq) { return time_kernel(ds, rq, repeats, kernel_ms, total_ms); });
}

int nos_ndt3_time_kernel(nos_dataset* ds, const double R2[4], const double t2[2], const nos_loss* loss, int repeats,
                         double* kernel_ms, double* total_ms) {
  return with_request(3, ds, R2, 4, t2, 2, nullptr, 0.0, loss,
                      [&](const Request& rq) { return time_kernel(ds, rq, repeats, kernel_ms, total_ms); });
}

int nos_reproj_time_kernel(nos_dataset* ds, const double R[9], const double t[3], const double intr[4],
                           const nos_loss* loss, double min_depth, int repeats, double* kernel_ms,
                           double* total_ms) {
  return with_request(2, ds, R, 9, t, 3, intr, min_depth, loss,
                      [&](const Request& rq) { return time_kernel(ds, rq, repeats, kernel_ms, total_ms); });
}

int nos_debug_lm_step(nos_ctx* ctx, int dof, const double* sums, const double settings[4], double state[22]) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || !sums || !settings || !state || (dof != 6 && dof != 3)) return fail(NOS_ERR_INVALID_ARGUMENT, "bad argument");
  DeviceSlot& slot = ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  nos::LmDevice lmd{};
  for (int k = 0; k < 9; ++k) lmd.st.R[k] = state[k];
  for (int k = 0; k < 3; ++k) lmd.st.t[k] = state[9 + k];
  lmd.st.q.w = state[12], lmd.st.q.x = state[13], lmd.st.q.y = state[14], lmd.st.q.z = state[15];
  lmd.st.lambda = state[16], lmd.st.previous_cost = state[17], lmd.st.cost = state[18];
  lmd.st.iteration = int(state[19]), lmd.st.done = int(state[20]), lmd.st.ok = int(state[21]);
  lmd.settings.max_iterations = int(settings[0]);
  lmd.settings.gradient_tolerance = settings[1];
  lmd.settings.parameter_tolerance = settings[2];
  lmd.settings.float_schedule = int(settings[3]);
  const int n_out = dof == 6 ? 28 : 10;
  NOS_HIP_CHECK(hipMemcpyAsync(slot.d_lm, &lmd, sizeof lmd, hipMemcpyHostToDevice, slot.stream));
  NOS_HIP_CHECK(hipMemcpyAsync(slot.d_out, sums, sizeof(double) * n_out, hipMemcpyHostToDevice, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));  // lmd is a stack object
  if (dof == 6)
    hipLaunchKernelGGL((nos::lm_step_kernel<28>), dim3(1), dim3(64), 0, slot.stream, slot.d_out, slot.d_lm,
                       static_cast<double*>(nullptr), static_cast<unsigned long long*>(nullptr), 0ull);
  else
    hipLaunchKernelGGL((nos::lm_step_kernel<10>), dim3(1), dim3(64), 0, slot.stream, slot.d_out, slot.d_lm,
                       static_cast<double*>(nullptr), static_cast<unsigned long long*>(nullptr), 0ull);
  NOS_HIP_CHECK(hipGetLastError());
  NOS_HIP_CHECK(hipMemcpyAsync(&lmd, slot.d_lm, sizeof lmd, hipMemcpyDeviceToHost, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  for (int k = 0; k < 9; ++k) state[k] = lmd.st.R[k];
  for (int k = 0; k < 3; ++k) state[9 + k] = lmd.st.t[k];
  state[12] = lmd.st.q.w, state[13] = lmd.st.q.x, state[14] = lmd.st.q.y, state[15] = lmd.st.q.z;
  state[16] = lmd.st.lambda, state[17] = lmd.st.previous_cost, state[18] = lmd.st.cost;
  state[19] = lmd.st.iteration, state[20] = lmd.st.done, state[21] = lmd.st.ok;
  return NOS_OK;
}

}  // extern "C"
