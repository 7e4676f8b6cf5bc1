// nos_ctx.hip — contexts: last-error text, settings and options, the device-buffer pool, profiling (C ABI of include/nos.h).
//
// Owns contexts (per-device stream + workspaces).  There is no CPU fallback: without a usable HIP device every entry point
// fails with NOS_ERR_NO_DEVICE / NOS_ERR_HIP.
#include "nos_internal.hpp"

#include <cxxabi.h>

namespace nosd {

namespace {
thread_local std::string g_last_error;
}

int fail(int status, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return status;
}

const char* last_error_text() { return g_last_error.c_str(); }
void clear_last_error() { g_last_error.clear(); }

// Directory of the shared object that provides `symbol` in this process ("" if unknown).
std::string dir_of_symbol(const void* symbol, std::string* file_out) {
  Dl_info info{};
  if (symbol == nullptr || dladdr(symbol, &info) == 0 || info.dli_fname == nullptr) return std::string();
  char resolved[PATH_MAX];
  std::string file = realpath(info.dli_fname, resolved) ? std::string(resolved) : std::string(info.dli_fname);
  if (file_out) *file_out = file;
  const size_t slash = file.rfind('/');
  return slash == std::string::npos ? std::string() : file.substr(0, slash);
}

int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return atoi(v);
}

// ------------------------------------------------------------------ device-buffer pool

// Pool limits: at most 8 parked buffers and 16 GiB per device; a parked buffer serves a request if it is large
// enough and not more than twice (+1 MiB) the size asked for.  The caller has selected the slot's device.
constexpr size_t kPoolMaxEntries = 8;
constexpr size_t kPoolMaxBytes = size_t(16) << 30;

void pool_drain(DeviceSlot& slot) {
  for (auto& pe : slot.pool) (void)hipFree(pe.ptr);
  slot.pool.clear();
  slot.pool_bytes = 0;
}

// Settings::debug_alloc_fill.  The word goes out with hipMemsetD32Async on the slot's stream and the stream is waited for:
// the ingestion copy streams are non-blocking streams of their own, so the caller must get a finished block.  A tail of
// fewer than four bytes gets the word's low bytes.  The counter is the context's, not the slot's, and plain: every
// allocation is made by the thread that holds the context's lock (CtxGuard) — the ingestion's worker threads pack host
// memory and allocate nothing.
hipError_t debug_fill(DeviceSlot& slot, void* ptr, size_t bytes, bool host) {
  Settings& st = *slot.settings;
  if (st.debug_alloc_fill == 0) return hipSuccess;  // off: this branch and nothing else
  const uint32_t word = st.debug_alloc_fill < 0 ? 0u : uint32_t(st.debug_alloc_fill);
  char* tail = static_cast<char*>(ptr) + (bytes & ~size_t(3));
  if (host) {
    for (size_t i = 0; i < bytes / 4; ++i) memcpy(static_cast<char*>(ptr) + 4 * i, &word, 4);
    memcpy(tail, &word, bytes & 3);
  } else {
    hipError_t e = bytes >= 4 ? hipMemsetD32Async(ptr, int(word), bytes / 4, slot.stream) : hipSuccess;
    if (e == hipSuccess && (bytes & 3) != 0) e = hipMemcpyAsync(tail, &word, bytes & 3, hipMemcpyHostToDevice, slot.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(slot.stream);
    if (e != hipSuccess) return e;
  }
  if (st.debug_alloc_filled < INT_MAX) ++st.debug_alloc_filled;
  return hipSuccess;
}

hipError_t device_alloc(DeviceSlot& slot, void** ptr, size_t bytes) {
  *ptr = nullptr;
  hipError_t e = hipMalloc(ptr, bytes);
  if (e == hipSuccess && (e = debug_fill(slot, *ptr, bytes)) != hipSuccess) {
    (void)hipFree(*ptr);
    *ptr = nullptr;
  }
  return e;
}

namespace {
// what pool_alloc hands out, parked or fresh, filled over its whole capacity while Settings::debug_alloc_fill is on
int pool_filled(DeviceSlot& slot, void* ptr, size_t capacity) {
  const hipError_t e = debug_fill(slot, ptr, capacity);
  if (e == hipSuccess) return NOS_OK;
  pool_release(slot, ptr, capacity);
  return hip_fail(e, "filling a device block (debug_alloc_fill)");
}
}  // namespace

int pool_alloc(DeviceSlot& slot, size_t bytes, void** ptr, size_t* capacity) {
  if (bytes == 0) bytes = 8;
  int best = -1;
  for (int i = 0; i < int(slot.pool.size()); ++i) {
    const size_t have = slot.pool[i].bytes;
    if (have >= bytes && have <= 2 * bytes + (size_t(1) << 20) && (best < 0 || have < slot.pool[best].bytes)) best = i;
  }
  if (best >= 0) {
    *ptr = slot.pool[best].ptr;
    *capacity = slot.pool[best].bytes;
    slot.pool_bytes -= slot.pool[best].bytes;
    slot.pool.erase(slot.pool.begin() + best);
    return pool_filled(slot, *ptr, *capacity);
  }
  hipError_t e = hipMalloc(ptr, bytes);
  if (e == hipErrorOutOfMemory && !slot.pool.empty()) {  // give the parked buffers back and try once more
    pool_drain(slot);
    e = hipMalloc(ptr, bytes);
  }
  if (e != hipSuccess)
    return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", bytes,
                hipGetErrorString(e));
  *capacity = bytes;
  return pool_filled(slot, *ptr, *capacity);
}

void pool_release(DeviceSlot& slot, void* ptr, size_t capacity) {
  if (!ptr) return;
  if (!slot.pool_enabled || capacity > kPoolMaxBytes) {
    (void)hipFree(ptr);
    return;
  }
  slot.pool.push_back({ptr, capacity});
  slot.pool_bytes += capacity;
  while (slot.pool.size() > kPoolMaxEntries || slot.pool_bytes > kPoolMaxBytes) {  // oldest first
    (void)hipFree(slot.pool.front().ptr);
    slot.pool_bytes -= slot.pool.front().bytes;
    slot.pool.erase(slot.pool.begin());
  }
}

}  // namespace nosd

using namespace nosd;

namespace {
struct OptionEntry {
  const char* key;
  int nosd::Settings::*field;
  int lo, hi;
};
const OptionEntry kOptions[] = {
    // key, field, lowest and highest accepted value
    {"plane_skew", &nosd::Settings::plane_skew, 0, 1 << 20},
    {"sc1", &nosd::Settings::sc1, 0, 1},
    {"nt", &nosd::Settings::nt, -1, 1},
    {"fused", &nosd::Settings::fused, 0, 1},
    {"lm_fused", &nosd::Settings::lm_fused, 0, 1},
    {"lm_window", &nosd::Settings::lm_window, 1, nosd::kLogSlots - 2},
    {"lm_single", &nosd::Settings::lm_single, 0, 1},
    {"lm_cluster", &nosd::Settings::lm_cluster, 0, 5},
    {"lm_cluster_retry_ms", &nosd::Settings::lm_cluster_retry_ms, 0, 3600000},
    {"pool", &nosd::Settings::pool, 0, 1},
    {"tile_log2", &nosd::Settings::tile_log2, -1, 24},
    {"ingest", &nosd::Settings::ingest, 0, 2},
    {"ingest_threads", &nosd::Settings::ingest_threads, 0, 1024},
    {"indexed_bpc", &nosd::Settings::indexed_bpc, 1, 16},
    {"match_dense", &nosd::Settings::match_dense, 0, 1},
    {"map_compact_keys", &nosd::Settings::map_compact_keys, 0, 1},
    {"pgo_host_scalars", &nosd::Settings::pgo_host_scalars, 0, 1},
    {"pgo_precond", &nosd::Settings::pgo_precond, 0, 1},
    {"pgo_agg", &nosd::Settings::pgo_agg, 2, 1 << 20},
    {"pgo_block", &nosd::Settings::pgo_block, 0, 1},
    {"pgo_coarse_probe", &nosd::Settings::pgo_coarse_probe, 0, 1},
    {"map_fma_mask", &nosd::Settings::map_fma_mask, 0, (1 << 26) - 1},
    {"map_eigen_version", &nosd::Settings::map_eigen_version, 33, 34},
    {"debug_cluster_abort", &nosd::Settings::debug_cluster_abort, 0, 2},
    {"debug_alloc_fill", &nosd::Settings::debug_alloc_fill, -1, INT_MAX},
    {"debug_alloc_filled", &nosd::Settings::debug_alloc_filled, 0, 0},  // a counter: read it, or reset it to 0
    {"lm_cluster_max_blocks", &nosd::Settings::lm_cluster_max_blocks, 1, 256},
    {"stream_lds_chunks", &nosd::Settings::stream_lds_chunks, 0, 3},
    {"stream_reg_rounds", &nosd::Settings::stream_reg_rounds, 0, nos::kStreamRegRoundsMax},
    {"batch_max_elements", &nosd::Settings::batch_max_elements, 0, 1 << 30},
};
bool option_in_range(const OptionEntry& o, int value) {
  if (value < o.lo || value > o.hi) return false;
  if (!strcmp(o.key, "tile_log2")) return value <= 0 || value >= 10;  // -1 by element type, 0 planar, tiles of 2^10 … 2^24
  return true;
}
void drop_out_of_range_settings(nosd::Settings& st) {
  const nosd::Settings defaults;
  for (const OptionEntry& o : kOptions)
    if (!option_in_range(o, st.*(o.field))) {
      fprintf(stderr, "[nos-hip] NOS_%s = %d is outside [%d, %d]: ignored\n", o.key, st.*(o.field), o.lo, o.hi);
      st.*(o.field) = defaults.*(o.field);
    }
}
}  // namespace

// ====================================================================== C ABI

extern "C" {

int nos_ctx_create(const int* device_ids, int n_devices, nos_ctx** out_ctx) {
  if (!out_ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "out_ctx is NULL");
  *out_ctx = nullptr;
  if (n_devices < 1 || n_devices > 64 || !device_ids) return fail(NOS_ERR_INVALID_ARGUMENT, "bad device list");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count < 1)
    return fail(NOS_ERR_NO_DEVICE, "no usable HIP device (%s); this library has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  for (int i = 0; i < n_devices; ++i)
    if (device_ids[i] < 0 || device_ids[i] >= count)
      return fail(NOS_ERR_INVALID_ARGUMENT, "device id %d out of range [0,%d)", device_ids[i], count);
  nos_ctx* ctx = new (std::nothrow) nos_ctx();
  if (!ctx) return fail(NOS_ERR_OUT_OF_MEMORY, "host allocation failed");
  ctx->slots.resize(n_devices);
  ctx->blocks_per_cu = env_int("NOS_BLOCKS_PER_CU", 0);
  ctx->variant = env_int("NOS_VARIANT", 0);
  {  // the only place the experiment knobs are read from the environment
    Settings& st = ctx->settings;
    st.plane_skew = env_int("NOS_PLANE_SKEW", st.plane_skew);
    st.sc1 = env_int("NOS_SC1", st.sc1);
    st.nt = env_int("NOS_NT", st.nt);
    st.fused = env_int("NOS_FUSED", st.fused);
    st.lm_fused = env_int("NOS_LM_FUSED", st.lm_fused);
    st.lm_window = env_int("NOS_LM_WINDOW", st.lm_window);
    st.lm_single = env_int("NOS_LM_SINGLE", st.lm_single);
    st.lm_cluster = env_int("NOS_LM_CLUSTER", st.lm_cluster);
    st.lm_cluster_max_blocks = env_int("NOS_LM_CLUSTER_MAX_BLOCKS", st.lm_cluster_max_blocks);
    st.stream_lds_chunks = env_int("NOS_STREAM_LDS_CHUNKS", st.stream_lds_chunks);
    st.stream_reg_rounds = env_int("NOS_STREAM_REG_ROUNDS", st.stream_reg_rounds);
    st.batch_max_elements = env_int("NOS_BATCH_MAX_ELEMENTS", st.batch_max_elements);
    st.pool = env_int("NOS_POOL", st.pool);
    st.tile_log2 = env_int("NOS_TILE_LOG2", st.tile_log2);
    const char* ingest = getenv("NOS_INGEST");
    st.ingest = (ingest && !strcmp(ingest, "pack")) ? 1 : ((ingest && !strcmp(ingest, "unpack")) ? 2 : 0);
    st.ingest_threads = env_int("NOS_INGEST_THREADS", 0);
    st.indexed_bpc = env_int("NOS_INDEXED_BPC", st.indexed_bpc);
    st.match_dense = env_int("NOS_MATCH_DENSE", st.match_dense);
    st.map_compact_keys = env_int("NOS_MAP_COMPACT_KEYS", st.map_compact_keys);
    st.pgo_host_scalars = env_int("NOS_PGO_HOST_SCALARS", st.pgo_host_scalars);
    st.pgo_precond = env_int("NOS_PGO_PRECOND", st.pgo_precond);
    st.pgo_agg = env_int("NOS_PGO_AGG", st.pgo_agg);
    st.pgo_block = env_int("NOS_PGO_BLOCK", st.pgo_block);
    st.pgo_coarse_probe = env_int("NOS_PGO_COARSE_PROBE", st.pgo_coarse_probe);
    drop_out_of_range_settings(st);  // the same ranges nos_ctx_set_option enforces
  }
  for (int i = 0; i < n_devices; ++i) {
    DeviceSlot& s = ctx->slots[i];
    s.device = device_ids[i];
    s.pool_enabled = ctx->settings.pool != 0;
    s.settings = &ctx->settings;
    hipDeviceProp_t prop;
    e = hipSetDevice(s.device);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, s.device);
    if (e == hipSuccess) {
      s.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
      e = hipStreamCreateWithFlags(&s.own_stream, hipStreamNonBlocking);
    }
    if (e == hipSuccess) e = hipMalloc(&s.partials, sizeof(double) * kMaxPartialRows * kMaxOut);
    if (e == hipSuccess) e = hipMalloc(&s.d_out, sizeof(double) * kMaxOut);
    if (e == hipSuccess) e = hipHostMalloc(&s.h_out, sizeof(double) * 64, hipHostMallocMapped);
    if (e == hipSuccess) memset(s.h_out, 0, sizeof(double) * 64);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&s.h_out_dev), s.h_out, 0);
    if (e == hipSuccess) e = hipMalloc(&s.d_lm, sizeof(nos::LmDevice));
    const size_t log_bytes = sizeof(double) * kLogSlots * nos::kLogEntryDoubles;
    if (e == hipSuccess) e = hipHostMalloc(&s.h_log, log_bytes, hipHostMallocMapped);
    if (e == hipSuccess) memset(s.h_log, 0, log_bytes);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&s.h_log_dev), s.h_log, 0);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&s.d_cluster), sizeof(nos::ClusterCtl));
    if (e == hipSuccess) e = hipMemset(s.d_cluster, 0, sizeof(nos::ClusterCtl));
    if (e == hipSuccess) e = hipHostMalloc(&s.h_hist, sizeof(double) * kHistCapacity, hipHostMallocMapped);
    if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&s.h_hist_dev), s.h_hist, 0);
    if (e == hipSuccess) e = hipMalloc(&s.counter, 2048);  // top ticket + 8 group tickets, 128 bytes apart
    if (e == hipSuccess) e = hipMemset(s.counter, 0, 2048);
    if (e == hipSuccess) e = hipEventCreate(&s.ev0);
    if (e == hipSuccess) e = hipEventCreate(&s.ev1);
    if (e == hipSuccess) e = hipEventCreate(&s.ev2);
    s.stream = s.own_stream;
    if (e != hipSuccess) {
      nos_ctx_destroy(ctx);
      return fail(e == hipErrorOutOfMemory ? NOS_ERR_OUT_OF_MEMORY : NOS_ERR_HIP, "context setup failed on device %d: %s",
                  device_ids[i], hipGetErrorString(e));
    }
  }
  *out_ctx = ctx;
  return NOS_OK;
}

int nos_ctx_destroy(nos_ctx* ctx) {
  if (!ctx) return NOS_OK;
  comm_release(ctx);
  for (DeviceSlot& s : ctx->slots) {
    (void)hipSetDevice(s.device);
    if (s.own_stream) {
      (void)hipStreamSynchronize(s.own_stream);
      (void)hipStreamDestroy(s.own_stream);
    }
    if (s.partials) (void)hipFree(s.partials);
    if (s.d_out) (void)hipFree(s.d_out);
    if (s.h_out) (void)hipHostFree(s.h_out);
    if (s.counter) (void)hipFree(s.counter);
    if (s.d_lm) (void)hipFree(s.d_lm);
    if (s.copy_stream) {
      (void)hipStreamSynchronize(s.copy_stream);
      (void)hipStreamDestroy(s.copy_stream);
    }
    for (int b = 0; b < 2; ++b) {
      if (s.stage[b]) (void)hipFree(s.stage[b]);
      if (s.ing_done[b]) (void)hipEventDestroy(s.ing_done[b]);
    }
    if (s.ing_copied) (void)hipEventDestroy(s.ing_copied);
    for (int b = 0; b < 2; ++b) {
      if (s.pack_pinned[b]) (void)hipHostFree(s.pack_pinned[b]);
      if (s.pack_done[b]) (void)hipEventDestroy(s.pack_done[b]);
    }
    if (s.batch_pinned) (void)hipHostFree(s.batch_pinned);
    pool_drain(s);
    if (s.h_log) (void)hipHostFree(s.h_log);
    if (s.h_hist) (void)hipHostFree(s.h_hist);
    if (s.d_cluster) (void)hipFree(s.d_cluster);
    if (s.ev0) (void)hipEventDestroy(s.ev0);
    if (s.ev1) (void)hipEventDestroy(s.ev1);
    if (s.ev2) (void)hipEventDestroy(s.ev2);
    for (hipEvent_t e : s.prof_events) (void)hipEventDestroy(e);
  }
  delete ctx;
  return NOS_OK;
}

int nos_ctx_num_devices(const nos_ctx* ctx) { return ctx ? int(ctx->slots.size()) : 0; }

int nos_ctx_set_stream(nos_ctx* ctx, int shard, void* hip_stream) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || shard < 0 || shard >= int(ctx->slots.size())) return fail(NOS_ERR_INVALID_ARGUMENT, "bad ctx / shard");
  ctx->slots[shard].stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->slots[shard].own_stream;
  return NOS_OK;
}

int nos_ctx_synchronize(nos_ctx* ctx) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx is NULL");
  for (DeviceSlot& s : ctx->slots) {
    NOS_HIP_CHECK(hipSetDevice(s.device));
    NOS_HIP_CHECK(hipStreamSynchronize(s.stream));
  }
  return NOS_OK;
}

int nos_ctx_set_option(nos_ctx* ctx, const char* key, int value) {
  if (!ctx || !key) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx / key is NULL");
  nosd::CtxGuard guard_(ctx);
  for (const OptionEntry& o : kOptions)
    if (!strcmp(o.key, key)) {
      if (!option_in_range(o, value))
        return fail(NOS_ERR_INVALID_ARGUMENT, "option '%s' = %d is outside [%d, %d]", key, value, o.lo, o.hi);
      ctx->settings.*(o.field) = value;
      for (DeviceSlot& s : ctx->slots) s.pool_enabled = ctx->settings.pool != 0;
      return NOS_OK;
    }
  return fail(NOS_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
}

int nos_ctx_get_option(const nos_ctx* ctx, const char* key, int* value) {
  if (!ctx || !key || !value) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx / key / value is NULL");
  nosd::CtxGuard guard_(ctx);
  for (const OptionEntry& o : kOptions)
    if (!strcmp(o.key, key)) {
      *value = ctx->settings.*(o.field);
      return NOS_OK;
    }
  return fail(NOS_ERR_INVALID_ARGUMENT, "unknown option '%s'", key);
}

// Where the HIP runtime and the collectives library mapped into this process come from, and whether that is the ROCm
// the library was built with.  One line of JSON.
int nos_runtime_info(char* buf, size_t capacity) {
  if (!buf || capacity == 0) return fail(NOS_ERR_INVALID_ARGUMENT, "buf is NULL");
  int runtime = 0, driver = 0;
  (void)hipRuntimeGetVersion(&runtime);
  (void)hipDriverGetVersion(&driver);
  std::string hip_file;
  const std::string hip_dir = dir_of_symbol(reinterpret_cast<const void*>(&hipGetDeviceCount), &hip_file);
  RcclApi* api = Rccl();
  int rccl_version = 0;
  if (api->ok && api->GetVersion) (void)api->GetVersion(&rccl_version);
  const std::string rccl_file = api->ok ? api->path : std::string();
  const size_t slash = rccl_file.rfind('/');
  const std::string rccl_dir = slash == std::string::npos ? std::string() : rccl_file.substr(0, slash);
  const int build = HIP_VERSION;  // major * 10^7 + minor * 10^5 + patch, same encoding as hipRuntimeGetVersion
  const int n = snprintf(buf, capacity,
                         "{\"build_hip_version\": %d, \"runtime_hip_version\": %d, \"driver_version\": %d, "
                         "\"hip_runtime_path\": \"%s\", \"rccl_path\": \"%s\", \"rccl_version\": %d, "
                         "\"same_rocm_tree\": %s, \"runtime_matches_build\": %s}",
                         build, runtime, driver, hip_file.c_str(), rccl_file.c_str(), rccl_version,
                         (!rccl_dir.empty() && rccl_dir == hip_dir) ? "true" : "false",
                         (build / 100000 == runtime / 100000) ? "true" : "false");
  if (n < 0 || size_t(n) >= capacity) return fail(NOS_ERR_INVALID_ARGUMENT, "buffer too small");
  return NOS_OK;
}

// Symbol (demangled) of the hot-path kernel launched last on `shard` of this context — the instantiation the library
// chose (problem, element type, loss, launch geometry / loop form), as rocprofv3 will list it.
int nos_ctx_last_kernel(const nos_ctx* ctx, int shard, char* buf, size_t capacity) {
  if (!ctx || !buf || capacity == 0) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx / buf is NULL");
  nosd::CtxGuard guard_(ctx);
  if (shard < 0 || size_t(shard) >= ctx->slots.size()) return fail(NOS_ERR_INVALID_ARGUMENT, "bad shard index");
  buf[0] = 0;
  const DeviceSlot& slot = ctx->slots[shard];
  if (slot.last_kernel == nullptr) return NOS_OK;
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  const char* mangled = hipKernelNameRefByPtr(slot.last_kernel, slot.stream);
  if (mangled == nullptr) return fail(NOS_ERR_HIP, "hipKernelNameRefByPtr returned NULL");
  int status = 0;
  char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  snprintf(buf, capacity, "%s", (status == 0 && dem) ? dem : mangled);
  free(dem);
  return NOS_OK;
}

int nos_ctx_set_launch(nos_ctx* ctx, int blocks_per_cu, int variant) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx is NULL");
  if (blocks_per_cu < 0 || blocks_per_cu > 32 || variant < 0 || variant >= kNumVariants)
    return fail(NOS_ERR_INVALID_ARGUMENT, "launch override out of range");
  ctx->blocks_per_cu = blocks_per_cu;
  ctx->variant = variant;
  return NOS_OK;
}

int nos_ctx_profile_begin(nos_ctx* ctx, int max_launches, int sample_every) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || max_launches < 1 || max_launches > (1 << 20) || sample_every < 0)
    return fail(NOS_ERR_INVALID_ARGUMENT, "bad profile request");
  for (DeviceSlot& s : ctx->slots) {
    NOS_HIP_CHECK(hipSetDevice(s.device));
    if (sample_every == 0) {  // bracket form
      s.prof_used = 0;
      s.prof_every = 0;
      s.prof_launches = 0;
      s.prof_on = true;
      NOS_HIP_CHECK(hipEventRecord(s.ev0, s.stream));
      continue;
    }
    while (s.prof_events.size() < size_t(max_launches) * 2) {
      hipEvent_t e = nullptr;
      NOS_HIP_CHECK(hipEventCreate(&e));
      s.prof_events.push_back(e);
    }
    s.prof_used = 0;
    s.prof_every = sample_every;
    s.prof_launches = 0;
    s.prof_on = true;
  }
  return NOS_OK;
}

int nos_ctx_profile_end(nos_ctx* ctx, int* n_launches, double* mean_ms, double* min_ms, double* max_ms) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx is NULL");
  int count = 0;
  double sum = 0.0, lo = 1e300, hi = 0.0;
  for (DeviceSlot& s : ctx->slots) {
    const bool bracket = s.prof_on && s.prof_every == 0;
    s.prof_on = false;
    NOS_HIP_CHECK(hipSetDevice(s.device));
    if (bracket) {
      NOS_HIP_CHECK(hipEventRecord(s.ev1, s.stream));
      NOS_HIP_CHECK(hipEventSynchronize(s.ev1));
      float ms = 0.f;
      NOS_HIP_CHECK(hipEventElapsedTime(&ms, s.ev0, s.ev1));
      if (s.prof_launches > 0) {
        const double per = double(ms) / double(s.prof_launches);
        sum += per * double(s.prof_launches);
        lo = std::min(lo, per);
        hi = std::max(hi, per);
        count += int(s.prof_launches);
      }
      s.prof_every = 1;
      continue;
    }
    NOS_HIP_CHECK(hipStreamSynchronize(s.stream));
    for (size_t i = 0; i + 1 < s.prof_used; i += 2) {
      float ms = 0.f;
      NOS_HIP_CHECK(hipEventElapsedTime(&ms, s.prof_events[i], s.prof_events[i + 1]));
      sum += ms;
      lo = std::min(lo, double(ms));
      hi = std::max(hi, double(ms));
      ++count;
    }
    s.prof_used = 0;
  }
  if (n_launches) *n_launches = count;
  if (mean_ms) *mean_ms = count ? sum / count : 0.0;
  if (min_ms) *min_ms = count ? lo : 0.0;
  if (max_ms) *max_ms = count ? hi : 0.0;
  return NOS_OK;
}

const char* nos_status_string(int status) {
  switch (status) {
    case NOS_OK: return "ok";
    case NOS_ERR_INVALID_ARGUMENT: return "invalid argument";
    case NOS_ERR_NO_DEVICE: return "no HIP device (no CPU fallback)";
    case NOS_ERR_HIP: return "HIP runtime error";
    case NOS_ERR_OUT_OF_MEMORY: return "out of memory";
    case NOS_ERR_WRONG_KIND: return "dataset kind mismatch";
    case NOS_ERR_UNSUPPORTED: return "unsupported";
  }
  return "unknown status";
}

const char* nos_last_error(void) { return nosd::last_error_text(); }
#ifdef NOS_ALL_VARIANTS
const char* nos_version(void) { return "nos-hip 0.3 (gfx950, all launch geometries)"; }
#else
const char* nos_version(void) { return "nos-hip 0.3 (gfx950)"; }
#endif

}  // extern "C"
