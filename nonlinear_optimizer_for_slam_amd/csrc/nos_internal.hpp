// nos_internal.hpp — declarations shared by the translation units of libnos_hip.so (not part of the ABI).
#pragma once

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <random>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/nos.h"
#include "assemble_kernels.hpp"
#include "match_kernels.hpp"
#include "voxelmatch_kernels.hpp"

namespace nosd {

struct DeviceSlot;
struct Settings;

// nos_ctx.hip
// thread-local text of the last failure + status pass-through
int fail(int status, const char* fmt, ...);
void clear_last_error();  // a failure that was handled (a fallback that went on to succeed) leaves no text behind
// Directory of the shared object that provides `symbol` in this process ("" if unknown); file_out: its path.
std::string dir_of_symbol(const void* symbol, std::string* file_out = nullptr);
int env_int(const char* name, int dflt);
// the slot's device-buffer pool; pool_drain frees what is parked there
int pool_alloc(DeviceSlot& slot, size_t bytes, void** ptr, size_t* capacity);
void pool_release(DeviceSlot& slot, void* ptr, size_t capacity);
void pool_drain(DeviceSlot& slot);
// The ONE hipMalloc of whatever an object or a call allocates on the slot's device after the context was created (the
// caller has selected the device).  While Settings::debug_alloc_fill is on, the block is filled before this returns.
hipError_t device_alloc(DeviceSlot& slot, void** ptr, size_t bytes);
template <typename T>
inline hipError_t device_alloc(DeviceSlot& slot, T** ptr, size_t bytes) {
  void* p = nullptr;
  const hipError_t e = device_alloc(slot, &p, bytes);
  *ptr = static_cast<T*>(p);
  return e;
}
// Settings::debug_alloc_fill for a block of `bytes` at `ptr`: device memory through the slot's stream, complete on return
// (the ingestion copy streams do not wait for that stream); pinned host memory (`host`) by memset.  Off: nothing.
hipError_t debug_fill(DeviceSlot& slot, void* ptr, size_t bytes, bool host = false);

#define NOS_HIP_CHECK(expr)                                                               \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::nosd::fail(e_ == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP,        \
                  "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// A failed HIP call outside a macro's reach → its status and "<what> failed: <HIP's text>".
inline int hip_fail(hipError_t e, const char* what) {
  return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
}

// RCCL is bound at run time (dlopen) so that single-GPU use never needs it and so that a process
// that already carries torch's copy of librccl shares that copy instead of loading a second one.
struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*GetVersion)(int*) = nullptr;
  std::string path;  // file the library was loaded from
  bool ok = false;
};

// nos_comm.hip
RcclApi* Rccl();
void comm_release(nos_ctx* ctx);  // frees whatever communicator the context has (nos_ctx_destroy calls it)

#define NOS_RCCL_CHECK(expr)                                                                     \
  do {                                                                                           \
    ncclResult_t r_ = (expr);                                                                    \
    if (r_ != ncclSuccess) return ::nosd::fail(NOS_ERR_HIP, "%s failed: %s", #expr, Rccl()->GetErrorString(r_)); \
  } while (0)

enum DatasetKind { kKindNdt = 1, kKindReproj = 2, kKindNdtIndexed = 3 };

constexpr int kMaxPartialRows = 8192;  // upper bound on grid size of the assemble kernel
constexpr int kMaxOut = 28;
constexpr int kHistCapacity = 4096;     // iterations whose cost the single-workgroup solve can report
constexpr int kLogSlots = 64;          // ring of loop log entries; bounds the number of launches in flight
constexpr int kNumVariants = 14;       // compiled geometry variants per dtype (the NOS_CASE tables of nos_core.hip; 0 = default)

struct DeviceSlot {
  int device = 0;
  int num_cus = 256;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;    // own_stream or an external one
  double* partials = nullptr;      // [kMaxPartialRows][kMaxOut] device
  double* d_out = nullptr;         // [kMaxOut] device
  double* h_out = nullptr;         // pinned, device-mapped host block: [0..27] result, [32] sequence word
  double* h_out_dev = nullptr;     // device-side address of h_out
  unsigned int* counter = nullptr; // device ticket word of the in-launch final reduce (kept at 0 between launches)
  unsigned long long seq = 0;      // last sequence value handed to a fused launch
  nos::LmDevice* d_lm = nullptr;   // device-resident loop state (nos_*_solve)
  double* h_log = nullptr;         // pinned, device-mapped ring of per-iteration log entries [kLogSlots][kLogEntryDoubles]
  double* h_log_dev = nullptr;
  nos::ClusterCtl* d_cluster = nullptr;  // abort word + arrival counters of the resident one-launch solve
  double* h_hist = nullptr;        // pinned, device-mapped cost history of the single-workgroup solve [kHistCapacity]
  double* h_hist_dev = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  // Ingestion resources, created on first use and kept (a cold Solve() used to spend ≈ 3 ms creating and freeing
  // them): copy stream, events, two staging buffers that only grow.
  hipStream_t copy_stream = nullptr;
  hipEvent_t ing_done[2] = {nullptr, nullptr};
  hipEvent_t ing_copied = nullptr;
  void* stage[2] = {nullptr, nullptr};
  size_t stage_bytes = 0;
  void* pack_pinned[2] = {nullptr, nullptr};  // pinned host staging of the host-pack ingestion: [n_fields][chunk] elements
  size_t pack_bytes = 0;
  // pinned host staging of a batched call (BatchTrip, batch_host.hpp: the batched solve, the batched registrations, the
  // score batch): what goes up, then what comes down; grows only
  void* batch_pinned = nullptr;
  size_t batch_pinned_bytes = 0;
  hipEvent_t pack_done[2] = {nullptr, nullptr};
  // Device-buffer pool for dataset storage: nos_dataset_destroy parks the buffer here, the next dataset of a similar
  // size takes it over (the reference's outer loop re-Solves up to 10 times with correspondences of similar count).
  struct PoolEntry {
    void* ptr;
    size_t bytes;
  };
  std::vector<PoolEntry> pool;
  size_t pool_bytes = 0;
  bool pool_enabled = true;  // Settings::pool
  Settings* settings = nullptr;  // the context's (nos_ctx_create): debug_alloc_fill, read by pool_alloc and device_alloc
  const void* last_kernel = nullptr;  // host function of the hot-path kernel launched last on this device (nos_ctx_last_kernel)
  bool cluster_gave_up = false;  // the last one-launch solve on this device timed out waiting for its grid (shared GPU)
  std::chrono::steady_clock::time_point cluster_gave_up_at{};
  // Ranks of a device-memory mailbox communicator must agree on the loop form of every solve (the one-launch loop and the
  // launch-per-iteration loop exchange through different protocols), so there the pause after a give-up is counted in
  // SOLVES — every rank gives up in the same solve and counts the same calls — not in wall time.
  int cluster_paused_solves = 0;
  int cluster_next_pause = 64;  // doubles with every give-up in a row (up to 65 536 solves), back to 64 after a one-launch solve that finished
  // per-launch kernel timing (nos_ctx_profile_begin/_end): event pairs recorded on the
  // launch stream around every assemble kernel while profiling is on
  std::vector<hipEvent_t> prof_events;
  size_t prof_used = 0;
  bool prof_on = false;
  int prof_every = 1;       // time every prof_every-th launch (event records cost ≈ 1 µs of host time each)
  long prof_launches = 0;
};

constexpr int kMapReferenceFmaMask = (4 | 8 | 16 | 32) | ((1 | 4 | 8 | 32 | 256) << 8) | (0x1ff << 17);
// Experiment / test knobs.  Read from the environment ONCE, when the context is created (nos_ctx_create), and
// changed afterwards only through nos_ctx_set_option: nothing on the solve / accumulate path calls getenv().
struct Settings {
  int plane_skew = 1088;     // NOS_PLANE_SKEW      elements between consecutive planes beyond n_padded
  int sc1 = 1;               // NOS_SC1             write-through rows instead of release / acquire fences
  int nt = -1;               // NOS_NT              -1 auto, 0 / 1 force non-temporal loads off / on
  int fused = 1;             // NOS_FUSED           in-launch final reduce
  int lm_fused = 1;          // NOS_LM_FUSED        LM step in the finishing workgroup
  int lm_window = 3;         // NOS_LM_WINDOW       launches kept in flight by the device loop
  int lm_single = 1;         // NOS_LM_SINGLE       whole solve in one workgroup for tiny problems
  int lm_cluster_retry_ms = 5000;  // after a one-launch solve gave up (GPU shared): how long the context goes straight to the launch-per-iteration loop
  int lm_cluster = 1;        // NOS_LM_CLUSTER      whole solve in one launch (resident on chip, or streamed per iteration beyond that); 5 = all-reduce stage 1 always through sc1 stores, 4 = resident form only, 3 = (round 2's counter all-reduce: removed in round 4, behaves like 1), 2 = one item per lane, 0 = off
  int pool = 1;              // NOS_POOL            device-buffer pool
  int tile_log2 = -1;        // NOS_TILE_LOG2       -1 = by element type (fp64 planar, fp32 1024-item tiles), 0 = planar
  int ingest = 0;            // NOS_INGEST          0 auto, 1 pack (host gather), 2 unpack (device)
  int ingest_threads = 0;    // NOS_INGEST_THREADS  0 = min(16, hw / 2)
  int indexed_bpc = 1;       // NOS_INDEXED_BPC
  int match_dense = 1;       // NOS_MATCH_DENSE
  int map_compact_keys = 1;  // NOS_MAP_COMPACT_KEYS  sort voxels / scan cells by their index inside the bounding box (0: 63-bit packed keys)
  int pgo_host_scalars = 0;  // NOS_PGO_HOST_SCALARS
  int pgo_precond = 1;       // NOS_PGO_PRECOND     0 block-Jacobi only, 1 two-level (rigid-motion coarse space)
  int pgo_agg = 48;          // NOS_PGO_AGG         poses per aggregate of the coarse level
  int pgo_coarse_probe = 0;  // NOS_PGO_COARSE_PROBE 1 = coarse operator probed with 18 masked products (round 2) instead of assembled
  int pgo_block = 1;         // NOS_PGO_BLOCK       block-local product (entry lists built by nos_pgo_create); 0 = owner-computes sweeps
  // NOS_MAP_REFERENCE_EXACT builds (mapexact_kernels.hpp): which multiply-adds are fused and which Eigen release's
  // deflation test / shift guard is followed.  Defaults = what reproduces the reference's captured x86-64 runs;
  // map_fma_mask = 0 follows the aarch64 captures (tests/test_reference_ndt_runs.py).
  int map_fma_mask = kMapReferenceFmaMask;
  int map_eigen_version = 34;
  int debug_cluster_abort = 0;  // test hook (no environment name): the next one-launch solve finds `abort` raised; 2 = and the
                                // give-up is remembered like a real one (the lm_cluster_retry_ms latch)
  int debug_alloc_fill = 0;     // test hook (no environment name): 0 off; -1 = every block pool_alloc returns (parked or
                                // fresh, over its whole capacity), every device_alloc block and the lazily allocated pinned
                                // staging blocks are filled with the word 0x00000000 before they are handed out; 1 …
                                // 0x7FFFFFFF = with that 32-bit word.  The context's own workspaces (nos_ctx_create) exist
                                // before the option can be set and are not filled.
  int debug_alloc_filled = 0;   // test hook: blocks filled so far (saturating); set to 0 to reset, nothing else is accepted
  int lm_cluster_max_blocks = 256;  // NOS_LM_CLUSTER_MAX_BLOCKS  workgroups of the one-launch loop (rehearsals: ranks sharing a GPU)
  int stream_lds_chunks = 3;   // NOS_STREAM_LDS_CHUNKS  streamed one-launch loop: chunks per workgroup kept in LDS after
                               //                        iteration 0 (0 … 3; 0 = everything streamed every iteration)
  int stream_reg_rounds = 3;   // NOS_STREAM_REG_ROUNDS  streamed one-launch loop: rounds per workgroup kept in vector registers
                               //                        after iteration 0 (0 … 3, clamped per kernel; 0 = none)
  int batch_max_elements = int(nos::kSingleBlockMaxElements);  // NOS_BATCH_MAX_ELEMENTS  nos_*_solve_batch: a flat problem
                               // of n x planes ≤ this runs in the batch launch (one workgroup), a larger one as a lone solve
};
}  // namespace nosd

struct nos_ctx {
  std::recursive_mutex mu;  // serialises every entry point that touches per-context state (see nosd::CtxGuard)
  nosd::Settings settings;
  std::vector<nosd::DeviceSlot> slots;
  int blocks_per_cu = 0;  // 0 = default
  int variant = 0;        // 0 = default; tuning knob (see pick_variant)
  int tile_log2 = -1;     // -1 = default; 0 = planar
  ncclComm_t comm = nullptr;  // set by nos_ctx_comm_init: accumulate results are summed over its ranks
  int comm_ranks = 1;
  int comm_rank = 0;
  // shared-memory mailbox communicator (nos_ctx_comm_init_shm): the sums are exchanged inside the launch
  void* shm_host = nullptr;            // mmap of the POSIX shm segment
  size_t shm_bytes = 0;
  double* shm_dev = nullptr;           // its device address (hipHostRegister, mapped)
  unsigned long long* d_round = nullptr;  // device word: exchange rounds completed
  nos::Mailbox* d_mail = nullptr;         // device copy of the descriptor the kernels read
  // device-memory mailbox (nos_ctx_comm_init_shm_device): every rank's slot buffer, fine-grained device memory
  double* ipc_own = nullptr;              // this rank's buffer
  std::vector<double*> ipc_peers;         // [rank] → that rank's buffer as mapped here (own buffer at comm_rank)
  double** d_peers = nullptr;             // device copy of ipc_peers
};

namespace nosd {

// One solve / accumulate / dataset create / destroy at a time per context: the per-slot state (sequence words,
// partial rows, tickets, loop state, pinned result block, staging buffers, buffer pool) is shared by every object
// created on the context — e.g. by every drop-in solver object with the same device list (AcquireRuntime).  The
// reference's solver objects are independent per instance; this lock gives the same guarantee to threads that each own
// their solver.  Recursive: entry points call each other (match → dataset create).
struct CtxGuard {
  std::unique_lock<std::recursive_mutex> lock;
  explicit CtxGuard(const nos_ctx* ctx) {
    if (ctx != nullptr) lock = std::unique_lock<std::recursive_mutex>(const_cast<nos_ctx*>(ctx)->mu);
  }
};

struct Shard {
  int slot = 0;
  nos::TiledLayout layout{};
  void* data = nullptr;
  size_t bytes = 0;
  size_t capacity = 0;        // size of the allocation behind `data` (>= bytes when it came from the pool)
  bool pooled = false;        // data goes back to the slot's pool on destroy
  // voxel-indexed datasets (kKindNdtIndexed): data = 3 point planes; plus
  int32_t* index = nullptr;   // n_slots planes of n_padded voxel ids
  void* table = nullptr;      // [n_voxels][16] voxel records
  bool one_block = false;     // index and table live inside the (pooled) allocation behind `data`: nothing else to free
  int n_slots = 0;
  size_t n_voxels = 0;
};

}  // namespace nosd

struct nos_dataset {
  nos_ctx* ctx = nullptr;
  int kind = 0;
  int dtype = NOS_F64;
  int n_fields = 0;
  size_t n = 0;
  size_t tile = 0;
  int simd_class = 0;  // nos_dataset_set_simd_class: the semantics of the reference's fp32 (SIMD) solver classes
  std::vector<nosd::Shard> shards;
};

struct nos_ndt_map {
  nos_ctx* ctx = nullptr;
  size_t n_voxels = 0;  // valid voxels only
  double* d_mean = nullptr;
  double* d_sqrt_info = nullptr;
  uint32_t* d_orig_id = nullptr;
  uint64_t* d_cell_key = nullptr;
  uint32_t* d_cell_start = nullptr;
  uint32_t* d_cell_count = nullptr;
  unsigned long long* d_n_matches = nullptr;
  uint32_t* d_dense_begin = nullptr;  // dense grid offsets (null when the bounding box is too large)
  double* d_record = nullptr;         // [V][4] candidate records of the dense path
  void* d_block = nullptr;            // the ONE allocation behind d_mean, d_sqrt_info, the hash table, d_dense_begin, d_record
  nos::MapView view{};
};

struct nos_scan {
  nos_ctx* ctx = nullptr;
  size_t n = 0;
  double* d_planes = nullptr;  // [3][n]
  uint32_t* d_order = nullptr; // after nos_scan_sort_by_cell: original index of the point stored at each position
};
// tests/test_scan_products_own_their_arrays.py reads n, d_planes and d_order out of a handle: four words in this order
static_assert(std::is_standard_layout<nos_scan>::value && sizeof(nos_scan) == 4 * sizeof(void*) && sizeof(size_t) == sizeof(void*) &&
                  offsetof(nos_scan, n) == sizeof(void*) && offsetof(nos_scan, d_planes) == 2 * sizeof(void*) &&
                  offsetof(nos_scan, d_order) == 3 * sizeof(void*),
              "nos_scan's layout is read by a test");

// per-voxel numbers of a map build (nos_mapbuild.hip) or of a voxel store (voxel_store_host.hpp; nos_voxel_map_stats in nos_voxelmap.hip), on the host
struct nos_map_stats {
  std::vector<double> means;            // [V][3] voxel order = ascending packed (ix, iy, iz); reference-exact mode: first seen
  std::vector<double> sqrt_infos;       // [V][9]
  std::vector<unsigned char> valid;     // [V]
  std::vector<uint32_t> counts;         // [V]
  std::vector<int64_t> cells;           // [V][3] integer voxel coordinates
  std::vector<double> evals;            // [V][3] un-floored eigenvalues           (reference-exact mode only)
  std::vector<double> evecs;            // [V][9] row-major eigenvector matrix V   (reference-exact mode only)
};

namespace nosd {

constexpr int kSeqSlot = 32;  // index (in doubles) of the sequence word inside the pinned block
constexpr int kCommErrorSlot = 40;  // index (in doubles) of the mailbox time-out flag (an unsigned int) in that block

// A scan under construction and its two device arrays, ONE copy of what nos_scan_create, the filter, the deskew and the
// ray cast each need: alloc sizes them (planes, then order — device_alloc, not the arena: the handle outlives the call);
// release hands the finished handle to the caller; whatever was not released is freed when this goes out of scope, and a
// failed allocation's sticky error goes with it, so that it does not surface as the next call's launch error.
struct NewScan {
  nos_scan* scan;
  explicit NewScan(nos_ctx* ctx) : scan(new (std::nothrow) nos_scan()) {
    if (scan) scan->ctx = ctx;
  }
  NewScan(const NewScan&) = delete;
  NewScan& operator=(const NewScan&) = delete;
  ~NewScan() {
    if (!scan) return;
    (void)hipGetLastError();
    if (scan->d_planes) (void)hipFree(scan->d_planes);
    if (scan->d_order) (void)hipFree(scan->d_order);
    delete scan;
  }
  explicit operator bool() const { return scan != nullptr; }
  // n points; n == 0: the empty form — a 24-byte planes block, so that d_planes is never NULL, and no order array
  hipError_t alloc(size_t n, bool with_order) {
    DeviceSlot& slot = scan->ctx->slots[0];
    hipError_t e = device_alloc(slot, &scan->d_planes, std::max<size_t>(n, 1) * 3 * sizeof(double));
    if (e == hipSuccess && with_order && n > 0) e = device_alloc(slot, &scan->d_order, n * sizeof(uint32_t));
    if (e == hipSuccess) scan->n = n;
    return e;
  }
  nos_scan* release() {
    nos_scan* s = scan;
    scan = nullptr;
    return s;
  }
};

// Scratch buffers of one call, freed when it returns: an ARENA — buffers are carved out of a few large slabs that come
// from the slot's buffer pool and go back to it, so a map build pays no hipMalloc + hipFree pair per buffer (each hipFree
// also waits for the device), and repeated builds of similar size pay none at all.  reserve() sizes the next slab when
// the caller knows what is coming.
struct DeviceBuffers {
  struct Slab {
    void* ptr;
    size_t capacity, used;
  };
  std::vector<Slab> slabs;
  DeviceSlot* slot;
  size_t next_slab = 0;
  explicit DeviceBuffers(DeviceSlot* s) : slot(s) {}
  DeviceBuffers(const DeviceBuffers&) = delete;
  DeviceBuffers& operator=(const DeviceBuffers&) = delete;
  ~DeviceBuffers() {
    if (!slabs.empty()) (void)hipStreamSynchronize(slot->stream);  // nothing in flight may still use a slab that goes back
    for (Slab& sl : slabs) pool_release(*slot, sl.ptr, sl.capacity);
  }
  void reserve(size_t bytes) { next_slab = bytes; }
  hipError_t alloc_bytes(void** out, size_t bytes) {
    bytes = (std::max<size_t>(bytes, 1) + 255) & ~size_t(255);
    *out = nullptr;
    if (slabs.empty() || slabs.back().capacity - slabs.back().used < bytes) {
      const size_t grown = slabs.empty() ? size_t(8) << 20 : std::min<size_t>(2 * slabs.back().capacity, size_t(1) << 30);
      const size_t want = std::max(std::max(bytes, next_slab), grown);
      next_slab = 0;
      void* p = nullptr;
      size_t cap = 0;
      if (pool_alloc(*slot, want, &p, &cap) != 0) return hipErrorOutOfMemory;
      slabs.push_back(Slab{p, cap, 0});
    }
    Slab& sl = slabs.back();
    *out = static_cast<char*>(sl.ptr) + sl.used;
    sl.used += bytes;
    return hipSuccess;
  }
  template <typename T>
  hipError_t alloc(T** out, size_t count) {
    void* p = nullptr;
    const hipError_t e = alloc_bytes(&p, std::max<size_t>(count, 1) * sizeof(T));
    *out = static_cast<T*>(p);
    return e;
  }
};

// A 3-D pose into whatever holds one as double R[9], t[3]: a PosePod, the descriptor of a registration or of a score.
template <typename Holder>
inline void set_pose(Holder& h, const double R[9], const double t[3]) {
  for (int k = 0; k < 9; ++k) h.R[k] = R[k];
  for (int k = 0; k < 3; ++k) h.t[k] = t[k];
}
// The pose the matcher and the store's insert warp a scan by, as their kernels take it.
inline nos::PosePod make_pose(const double R[9], const double t[3]) {
  nos::PosePod pose;
  set_pose(pose, R, t);
  return pose;
}

// What one accumulate call computes; POD so the same code path serves all three problems.
struct Request {
  int problem;  // 6, 3, 2 (reprojection)
  double R[9];
  double t[3];
  double intr[4];
  double min_depth;
  nos_loss loss;
  int loss_kind;
  int n_out;
};

template <typename T>
inline void fill_loss(const nos_loss* loss, T& la, T& lb, T& lc) {
  la = lb = lc = T(0);
  if (!loss) return;
  if (loss->kind == NOS_LOSS_EXPONENTIAL) {
    la = T(loss->a);
    lb = T(loss->b);
    lc = T(2.0 * loss->a * loss->b);
  } else if (loss->kind == NOS_LOSS_HUBER) {
    la = T(loss->a);
    lb = T(loss->a * loss->a);
    lc = T(2.0 * loss->a);
  }
}

// Item parameters of one problem from its request; ds: reprojection follows the dataset's simd_class.
template <typename T>
void fill_params(nos::Ndt6Params<T>& P, const Request& rq, const nos_dataset*) {
  for (int k = 0; k < 9; ++k) P.R[k] = T(rq.R[k]);
  for (int k = 0; k < 3; ++k) P.t[k] = T(rq.t[k]);
  fill_loss(&rq.loss, P.la, P.lb, P.lc);
}
template <typename T>
void fill_params(nos::Ndt3Params<T>& P, const Request& rq, const nos_dataset*) {
  for (int k = 0; k < 4; ++k) P.R2[k] = T(rq.R[k]);
  for (int k = 0; k < 2; ++k) P.t2[k] = T(rq.t[k]);
  fill_loss(&rq.loss, P.la, P.lb, P.lc);
}
template <typename T>
void fill_params(nos::ReprojParams<T>& P, const Request& rq, const nos_dataset* ds) {
  for (int k = 0; k < 9; ++k) P.R[k] = T(rq.R[k]);
  for (int k = 0; k < 3; ++k) P.t[k] = T(rq.t[k]);
  P.inv_fx = T(rq.intr[0]);
  P.inv_fy = T(rq.intr[1]);
  P.cx = T(rq.intr[2]);
  P.cy = T(rq.intr[3]);
  P.min_depth = T(rq.min_depth);
  nos::set_reproj_rules(P, ds->simd_class != 0);  // per dataset: each problem follows its own simd_class
  fill_loss(&rq.loss, P.la, P.lb, P.lc);
}

// Loop settings of one solve.  The one place for the float_schedule rule: the fp32 (SIMD) NDT classes of the reference keep
// lambda and previous_cost in float, its reprojection class does not.
inline nos_host::LmSettings make_lm_settings(const nos_lm_options* opt, int simd_class, int kind) {
  nos_host::LmSettings s;
  s.max_iterations = opt->max_iterations;
  s.gradient_tolerance = opt->gradient_tolerance;
  s.parameter_tolerance = opt->parameter_tolerance;
  s.float_schedule = (simd_class != 0 && kind != kKindReproj) ? 1 : 0;
  return s;
}

// What lm_init_kernel (and the host mirror of the loop state) starts a solve of `ds` from.
inline nos::LmInitArgs make_lm_init(const nos_dataset* ds, const Request& rq, const nos_lm_options* opt, const double* R, int nR,
                                    const double* t, int nt) {
  nos::LmInitArgs init{};
  for (int k = 0; k < nR; ++k) init.R[k] = R[k];
  for (int k = 0; k < nt; ++k) init.t[k] = t[k];
  init.settings = make_lm_settings(opt, ds->simd_class, ds->kind);
  init.dof = rq.n_out == 28 ? 6 : 3;
  return init;
}

// nos_dataset.hip
size_t elem_size(int dtype);
int dataset_new(nos_ctx* ctx, int kind, size_t n, int dtype, nos_dataset** out, nos_dataset** made);
// layout of a dataset's shard: tile size by element type and context settings, then the planes (flat NDT: nos::kNdtStored)
int dataset_tile_log2(const nos_ctx* ctx, int dtype);
nos::TiledLayout make_layout(size_t n, int n_fields, int tile_log2, int plane_skew);
size_t layout_elems(const nos::TiledLayout& L, int n_fields);
int zero_pad(int dtype, int n_fields, const nos::TiledLayout& L, void* dst, hipStream_t stream);
int unpack_records(int dtype, const unsigned char* d_rec, size_t stride, const nos::FieldOffsets& fo, int n_fields,
                   size_t first, size_t count, const nos::TiledLayout& L, void* dst, hipStream_t stream);
// nos_core.hip
int check_loss(const nos_loss* loss, int* kind_out);
// The one switch from a loss kind to its instantiation: f(std::integral_constant<int, LOSS>) → what f returns.
// Precondition: check_loss accepted the kind (directly or through build_request), so what is neither is Huber.
template <typename F>
inline auto with_loss(int loss_kind, F&& f) {
  switch (loss_kind) {
    case NOS_LOSS_NONE: return f(std::integral_constant<int, nos::kLossNone>{});
    case NOS_LOSS_EXPONENTIAL: return f(std::integral_constant<int, nos::kLossExponential>{});
    default: return f(std::integral_constant<int, nos::kLossHuber>{});
  }
}
int build_request(int problem, const nos_dataset* ds, const double* R, int nR, const double* t, int nt,
                  const double* intr, double min_depth, const nos_loss* loss, Request* rq);
// mailbox descriptor for the in-launch cross-rank exchange, and the time-out flag the kernels raise in the pinned block
nos::Mailbox mailbox_of(const nos_ctx* ctx, const DeviceSlot& slot);
int check_mailbox_error(const nos_ctx* ctx, DeviceSlot& slot);
// the device-resident loop of one dataset (nos_*_solve)
int lm_solve(nos_dataset* ds, const Request& rq, const nos_lm_options* opt, double* R, int nR, double* t, int nt,
             nos_lm_report* report);
// nos_match.hip: matcher tables from device-resident voxel statistics (valid may be null = all valid)
int map_create_device(nos_ctx* ctx, size_t n_voxels, const double* d_means, const double* d_S, const unsigned char* d_valid,
                      double search_radius_sq, nos_ndt_map** out_map);
// nos_mapbuild.hip: voxel_sums_kernel on device-resident 32-byte point records (the incremental store's batches run the
// build's own kernel, so a segment's nine sums — about the cell corner, voxel_finish.hpp — are the same bits from either)
hipError_t launch_voxel_sums(const double* d_records, const uint32_t* sorted_idx, const uint32_t* seg_offset,
                             const uint32_t* seg_count, uint32_t n_voxels, double inv_res, double res, double* acc_out,
                             hipStream_t stream);
// The live voxel store as whatever matches against it is handed it — the matcher of nos_voxelmap.hip (struct
// nos_voxel_map is voxel_store_host.hpp's, live_store voxel_query_host.hpp's; its match source, match_host.hpp, derives
// from this) and the batched registration of nos_voxelregister.hip.
struct LiveStore {
  nos_ctx* ctx;
  nos::VoxelMatchView view;
  unsigned long long* d_count;  // the store's kInfoMatches words: the match counter of a lone match
  unsigned int* d_error;        // the store's kInfoProbeError word
  double span;                  // cells the search ball spans per axis: 2 r / resolution + 2
  bool broken;                  // an earlier failure left the store undefined
};
// What every call that reads a store's content rejects: `broken` = a merge reported a probe error (nos_voxel_map::broken).
inline int check_usable(bool broken) {
  return broken ? fail(NOS_ERR_HIP, "the voxel store was left undefined by an earlier failure") : NOS_OK;
}
// What a lone match and a registration reject of the store itself, in this order.  The live matcher visits at most
// kVoxelMatchMaxSpan cells per axis.
inline int check_live_store(const LiveStore& s) {
  if (s.span > double(nos::kVoxelMatchMaxSpan))
    return fail(NOS_ERR_UNSUPPORTED,
                "the search ball spans more than %d voxel cells per axis (2 r / resolution + 2 = %g): match against a snapshot",
                nos::kVoxelMatchMaxSpan, s.span);
  return check_usable(s.broken);
}
// What a batched registration and a score batch reject of their scans: every scan there, and of the map's context.
inline int check_scans(const nos_ctx* ctx, nos_scan* const* scans, int n) {
  for (int i = 0; i < n; ++i) {
    if (scans[i] == nullptr) return fail(NOS_ERR_INVALID_ARGUMENT, "scan %d is NULL", i);
    if (scans[i]->ctx != ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "scan %d belongs to another context than the map", i);
  }
  return NOS_OK;
}
// nos_voxelregister.hip: a batched registration against the store.  store == NULL: the map argument was NULL.
int register_live(int dof, const LiveStore* store, nos_scan* const* scans, int32_t n_problems, double* R, double* t,
                  const nos_loss* loss, const nos_register_options* ropt, const nos_lm_options* options,
                  nos_register_report* reports);
// nos_score.hip: a batch of (scan, pose) problems scored against the store.  store == NULL: the map argument was NULL.
int score_live(const LiveStore* store, nos_scan* const* scans, int32_t n_problems, const double* R, const double* t,
               const nos_loss* loss, int max_neighbors, nos_pose_score* scores);
// nos_indexed.hip
// A voxel-indexed dataset from device-resident inputs (point planes [3][n], id planes [n_slots][n], voxel arrays), all on
// the context's stream; one host wait.  d_rows == NULL: table row r is row r of d_means / d_sqrt_infos and ids index them
// (nos_ndt_match_indexed).  Otherwise table row r is built from row d_rows[r] (n_voxels entries) and ids are ranks in
// d_rows: the compact table of nos_voxel_map_match_indexed (nos_voxelmap.hip), whose sources are the store's own arrays.
int indexed_from_device(nos_ctx* ctx, size_t n, const double* d_points, int n_slots, const int32_t* d_index, size_t n_voxels,
                        const double* d_means, const double* d_sqrt_infos, const uint32_t* d_rows, int dtype,
                        int sort_by_voxel, nos_dataset** out_ds);
int launch_indexed(const nos_dataset* ds, const Shard& sh, const Request& rq, double* partials,
                   const nos::FusedFinal& fin, hipStream_t stream, int* rows_out);

}  // namespace nosd
