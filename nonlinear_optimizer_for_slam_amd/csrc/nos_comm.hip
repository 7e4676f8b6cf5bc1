// nos_comm.hip — the three communicators: RCCL (bound with dlopen), the host-memory mailbox and the device-memory mailbox
// (C ABI of include/nos.h).
#include "nos_internal.hpp"

namespace nosd {

// librccl is bound with dlopen on first use.  Search order: $NOS_RCCL_PATH, then the librccl that sits NEXT TO the HIP
// runtime already mapped into the process (so runtime and collectives always come from one ROCm tree — a process that
// imported torch first runs on torch's bundled runtime and gets torch's bundled librccl; one that did not gets the
// system pair), then the loader's default search.
namespace {
void LoadRccl(RcclApi& api) {
  std::vector<std::string> names;
  if (const char* forced = getenv("NOS_RCCL_PATH")) names.push_back(forced);
  const std::string hip_dir = dir_of_symbol(reinterpret_cast<const void*>(&hipGetDeviceCount));
  if (!hip_dir.empty()) {
    names.push_back(hip_dir + "/librccl.so.1");
    names.push_back(hip_dir + "/librccl.so");
  }
  names.push_back("librccl.so.1");
  names.push_back("librccl.so");
  names.push_back("/opt/rocm/lib/librccl.so.1");
  for (const std::string& n : names) {
    api.handle = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (api.handle) break;
  }
  if (!api.handle) return;
  api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.handle, "ncclGetUniqueId"));
  api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.handle, "ncclCommInitRank"));
  api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.handle, "ncclCommDestroy"));
  api.AllReduce = reinterpret_cast<decltype(api.AllReduce)>(dlsym(api.handle, "ncclAllReduce"));
  api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.handle, "ncclGetErrorString"));
  api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(api.handle, "ncclCommCount"));
  api.GetVersion = reinterpret_cast<decltype(api.GetVersion)>(dlsym(api.handle, "ncclGetVersion"));
  api.ok = api.GetUniqueId && api.CommInitRank && api.CommDestroy && api.AllReduce && api.GetErrorString;
  if (api.ok) dir_of_symbol(reinterpret_cast<const void*>(api.AllReduce), &api.path);
}
}  // namespace

// Process-wide, bound once: two threads that each own a context may get here at the same time (std::call_once).
RcclApi* Rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] { LoadRccl(api); });
  return &api;
}

// Frees whatever communicator the context has (nos_ctx_comm_destroy, and nos_ctx_destroy on its way out).
void comm_release(nos_ctx* ctx) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (ctx)
    for (DeviceSlot& sl : ctx->slots) sl.cluster_paused_solves = 0, sl.cluster_next_pause = 64;  // a new communicator starts with every rank unpaused
  if (!ctx) return;
  if (ctx->comm != nullptr) {
    if (!ctx->slots.empty()) {
      (void)hipSetDevice(ctx->slots[0].device);
      (void)hipStreamSynchronize(ctx->slots[0].stream);
    }
    (void)Rccl()->CommDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  if (ctx->shm_host != nullptr) {
    if (!ctx->slots.empty()) {
      (void)hipSetDevice(ctx->slots[0].device);
      (void)hipStreamSynchronize(ctx->slots[0].stream);
    }
    for (size_t k = 0; k < ctx->ipc_peers.size(); ++k)
      if (ctx->ipc_peers[k] != nullptr && int(k) != ctx->comm_rank) (void)hipIpcCloseMemHandle(ctx->ipc_peers[k]);
    ctx->ipc_peers.clear();
    if (ctx->ipc_own) (void)hipFree(ctx->ipc_own);
    if (ctx->d_peers) (void)hipFree(ctx->d_peers);
    ctx->ipc_own = nullptr;
    ctx->d_peers = nullptr;
    (void)hipHostUnregister(ctx->shm_host);
    munmap(ctx->shm_host, ctx->shm_bytes);
    if (ctx->d_round) (void)hipFree(ctx->d_round);
    if (ctx->d_mail) (void)hipFree(ctx->d_mail);
    ctx->shm_host = nullptr;
    ctx->shm_dev = nullptr;
    ctx->d_round = nullptr;
    ctx->d_mail = nullptr;
  }
  ctx->comm_ranks = 1;
  ctx->comm_rank = 0;
}

}  // namespace nosd

using namespace nosd;

extern "C" {

int nos_comm_get_unique_id(unsigned char id[NOS_COMM_ID_BYTES]) {
  if (!id) return fail(NOS_ERR_INVALID_ARGUMENT, "id is NULL");
  RcclApi* api = Rccl();
  if (!api->ok) return fail(NOS_ERR_UNSUPPORTED, "librccl could not be loaded: %s", dlerror() ? dlerror() : "missing symbols");
  static_assert(NOS_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  ncclUniqueId uid;
  NOS_RCCL_CHECK(api->GetUniqueId(&uid));
  memcpy(id, uid.internal, NOS_COMM_ID_BYTES);
  return NOS_OK;
}

int nos_ctx_comm_init(nos_ctx* ctx, int n_ranks, int rank, const unsigned char id[NOS_COMM_ID_BYTES]) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(NOS_ERR_INVALID_ARGUMENT, "bad comm arguments");
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "a communicator needs a single-device context");
  if (ctx->comm != nullptr) return fail(NOS_ERR_INVALID_ARGUMENT, "communicator already initialised");
  RcclApi* api = Rccl();
  if (!api->ok) return fail(NOS_ERR_UNSUPPORTED, "librccl could not be loaded");
  NOS_HIP_CHECK(hipSetDevice(ctx->slots[0].device));
  ncclUniqueId uid;
  memcpy(uid.internal, id, NOS_COMM_ID_BYTES);
  ncclComm_t comm = nullptr;
  NOS_RCCL_CHECK(api->CommInitRank(&comm, n_ranks, uid, rank));
  ctx->comm = comm;
  ctx->comm_ranks = n_ranks;
  return NOS_OK;
}

int nos_ctx_comm_size(const nos_ctx* ctx) { return (ctx && (ctx->comm || ctx->shm_dev)) ? ctx->comm_ranks : 0; }

int nos_ctx_comm_destroy(nos_ctx* ctx) {
  comm_release(ctx);
  return NOS_OK;
}

// Number of ranks RCCL itself reports for the context's communicator (ncclCommCount); 0 without an RCCL communicator.
int nos_ctx_comm_rccl_count(const nos_ctx* ctx, int* count) {
  if (!ctx || !count) return fail(NOS_ERR_INVALID_ARGUMENT, "ctx / count is NULL");
  nosd::CtxGuard guard_(ctx);
  *count = 0;
  if (ctx->comm == nullptr) return NOS_OK;
  RcclApi* api = Rccl();
  if (!api->ok || !api->CommCount) return fail(NOS_ERR_UNSUPPORTED, "ncclCommCount unavailable");
  NOS_RCCL_CHECK(api->CommCount(ctx->comm, count));
  return NOS_OK;
}

}  // extern "C"

namespace {
// Both mailbox communicators: the handshake and control words always live in the POSIX shm segment; the SLOTS the kernels
// exchange through live there too (device_slots = false: bytes travel over PCIe to host memory) or in fine-grained device
// memory of every rank, exported with hipIpcGetMemHandle and opened by the peers (device_slots = true: a rank writes its
// sums straight into every peer's buffer — over xGMI between GPUs — and polls only its own memory).
int comm_init_mailbox(nos_ctx* ctx, int n_ranks, int rank, const char* shm_name, bool device_slots) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || !shm_name || shm_name[0] != '/' || n_ranks < 1 || n_ranks > 64 || rank < 0 || rank >= n_ranks)
    return fail(NOS_ERR_INVALID_ARGUMENT, "bad comm arguments (name must start with '/', at most 64 ranks)");
  if (ctx->slots.size() != 1) return fail(NOS_ERR_UNSUPPORTED, "a communicator needs a single-device context");
  if (ctx->comm != nullptr || ctx->shm_dev != nullptr) return fail(NOS_ERR_INVALID_ARGUMENT, "communicator already initialised");
  DeviceSlot& slot = ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  size_t bytes = 0;
  // Attach with a handshake that cannot be fooled by a segment of that name left behind by a crashed run (whose flag
  // words would otherwise match the first round numbers and feed stale sums into the exchange):
  //   rank 0 unlinks the name, creates the segment EXCLUSIVELY (a fresh, zero-filled inode), publishes a random nonce and
  //   acknowledges every rank's own fresh random hello word with hello ^ nonce;
  //   rank k opens the name (retrying), writes its hello and accepts the mapping only when its acknowledgement shows up —
  //   a stale inode never acknowledges a fresh 64-bit random, so rank k drops it and opens the name again.
  // Bounded: NOS_SHM_ATTACH_TIMEOUT_MS (default 30 s) in total.  Header (after the slots): [0] nonce, [1..64] hello, [65..128] ack.
  const int kAttachTimeoutMs = std::max(100, env_int("NOS_SHM_ATTACH_TIMEOUT_MS", 30000));  // set-up path, not the solve path
  const size_t slots_bytes = size_t(n_ranks) * 2 * nos::kMailSlotDoubles * sizeof(double);
  // header (after the slots), in 8-byte words: [0] nonce, [1..64] hello, [65..128] ack, [129..192] ipc-ready, [193..704] 64 IPC handles of 64 bytes
  const size_t header_words = 1 + 64 + 64 + 64 + 64 * 8;
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
  bytes = (slots_bytes + header_words * sizeof(unsigned long long) + 4095) & ~size_t(4095);
  auto now_ms = [] {
    return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
  };
  auto fresh_random = [&]() -> unsigned long long {
    unsigned long long v = 0;
    std::random_device rd;
    while (v == 0) v = (static_cast<unsigned long long>(rd()) << 32) ^ rd() ^ (static_cast<unsigned long long>(getpid()) << 17);
    return v;
  };
  const long long deadline = now_ms() + kAttachTimeoutMs;
  void* host = MAP_FAILED;
  if (rank == 0) {
    (void)shm_unlink(shm_name);
    int fd = shm_open(shm_name, O_CREAT | O_EXCL | O_RDWR, 0600);
    if (fd < 0 && errno == EEXIST) {  // somebody re-created it in between: once more
      (void)shm_unlink(shm_name);
      fd = shm_open(shm_name, O_CREAT | O_EXCL | O_RDWR, 0600);
    }
    if (fd < 0) return fail(NOS_ERR_HIP, "shm_open(%s) failed: %s", shm_name, strerror(errno));
    if (ftruncate(fd, off_t(bytes)) != 0) {  // fresh pages read as zero = round 0 everywhere
      const int e = errno;
      close(fd);
      (void)shm_unlink(shm_name);
      return fail(NOS_ERR_HIP, "ftruncate(%s) failed: %s", shm_name, strerror(e));
    }
    host = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (host == MAP_FAILED) return fail(NOS_ERR_HIP, "mmap(%s) failed: %s", shm_name, strerror(errno));
    auto* hdr = reinterpret_cast<std::atomic<unsigned long long>*>(static_cast<char*>(host) + slots_bytes);
    const unsigned long long nonce = fresh_random();
    hdr[0].store(nonce, std::memory_order_release);
    for (int k = 1; k < n_ranks; ++k) {
      unsigned long long hello = 0;
      while ((hello = hdr[1 + k].load(std::memory_order_acquire)) == 0) {
        if (now_ms() > deadline) {
          munmap(host, bytes);
          return fail(NOS_ERR_HIP, "rank %d did not attach to the mailbox %s within %d ms", k, shm_name, kAttachTimeoutMs);
        }
        usleep(200);
      }
      hdr[65 + k].store(hello ^ nonce, std::memory_order_release);
    }
  } else {
    const unsigned long long hello = fresh_random();
    for (;;) {
      if (now_ms() > deadline)
        return fail(NOS_ERR_HIP, "mailbox %s: no acknowledgement from rank 0 within %d ms", shm_name, kAttachTimeoutMs);
      const int fd = shm_open(shm_name, O_RDWR, 0600);
      if (fd < 0) {
        usleep(500);
        continue;
      }
      struct stat st {};
      if (fstat(fd, &st) != 0 || size_t(st.st_size) < bytes) {  // not sized yet (or somebody else's segment)
        close(fd);
        usleep(500);
        continue;
      }
      void* m = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
      close(fd);
      if (m == MAP_FAILED) return fail(NOS_ERR_HIP, "mmap(%s) failed: %s", shm_name, strerror(errno));
      auto* hdr = reinterpret_cast<std::atomic<unsigned long long>*>(static_cast<char*>(m) + slots_bytes);
      hdr[1 + rank].store(hello, std::memory_order_release);
      bool acked = false;
      const long long until = std::min<long long>(deadline, now_ms() + 250);  // then look at the name again
      while (now_ms() <= until) {
        const unsigned long long nonce = hdr[0].load(std::memory_order_acquire);
        if (nonce != 0 && hdr[65 + rank].load(std::memory_order_acquire) == (hello ^ nonce)) {
          acked = true;
          break;
        }
        usleep(200);
      }
      if (acked) {
        host = m;
        break;
      }
      munmap(m, bytes);  // stale inode (or rank 0 not there yet): drop it and open the name again
    }
  }
  hipError_t e = hipHostRegister(host, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
  void* dev = nullptr;
  if (e == hipSuccess) {
    e = hipHostGetDevicePointer(&dev, host, 0);
    if (e != hipSuccess) (void)hipHostUnregister(host);
  }
  unsigned long long* d_round = nullptr;
  if (e == hipSuccess) {
    e = hipMalloc(reinterpret_cast<void**>(&d_round), 2 * sizeof(unsigned long long));  // [0] round, [1] patient-until round
    if (e == hipSuccess) e = hipMemset(d_round, 0, 2 * sizeof(unsigned long long));
    if (e != hipSuccess) (void)hipHostUnregister(host);
  }
  if (e != hipSuccess) {
    if (d_round) (void)hipFree(d_round);
    munmap(host, bytes);
    return fail(NOS_ERR_HIP, "mapping the mailbox into the GPU failed: %s", hipGetErrorString(e));
  }
  *reinterpret_cast<volatile unsigned int*>(slot.h_out + kCommErrorSlot) = 0u;
  ctx->shm_host = host;
  ctx->shm_bytes = bytes;
  ctx->shm_dev = static_cast<double*>(dev);
  ctx->d_round = d_round;
  ctx->comm_ranks = n_ranks;
  ctx->comm_rank = rank;
  if (device_slots) {
    // every rank: its own [n_ranks][2][kMailSlotDoubles] buffer in fine-grained device memory (peers write into it across the
    // fabric while this GPU polls it: no cache may keep a stale copy), exported through the shm header and opened by the others
    auto* hdr = reinterpret_cast<std::atomic<unsigned long long>*>(static_cast<char*>(host) + slots_bytes);
    hipIpcMemHandle_t* handles = reinterpret_cast<hipIpcMemHandle_t*>(hdr + 193);
    double* own = nullptr;
    // second half: the granule slots of the one-launch loop's in-launch exchange (solve_cluster_kernel, stage 3)
    e = hipExtMallocWithFlags(reinterpret_cast<void**>(&own), 2 * slots_bytes, hipDeviceMallocFinegrained);
    if (e == hipSuccess) e = hipMemset(own, 0, 2 * slots_bytes);
    hipIpcMemHandle_t mine{};
    if (e == hipSuccess) e = hipIpcGetMemHandle(&mine, own);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
      if (own) (void)hipFree(own);
      (void)nos_ctx_comm_destroy(ctx);
      return fail(NOS_ERR_UNSUPPORTED, "device-memory mailbox: fine-grained allocation / IPC export failed: %s", hipGetErrorString(e));
    }
    ctx->ipc_own = own;
    memcpy(&handles[rank], &mine, sizeof mine);
    hdr[129 + rank].store(1ull, std::memory_order_release);
    ctx->ipc_peers.assign(size_t(n_ranks), nullptr);
    ctx->ipc_peers[size_t(rank)] = own;
    for (int k = 0; k < n_ranks; ++k) {
      if (k == rank) continue;
      while (hdr[129 + k].load(std::memory_order_acquire) == 0ull) {
        if (now_ms() > deadline) {
          (void)nos_ctx_comm_destroy(ctx);
          return fail(NOS_ERR_HIP, "device-memory mailbox %s: rank %d did not publish its IPC handle within %d ms", shm_name, k, kAttachTimeoutMs);
        }
        usleep(200);
      }
      hipIpcMemHandle_t theirs;
      memcpy(&theirs, &handles[k], sizeof theirs);
      void* p = nullptr;
      e = hipIpcOpenMemHandle(&p, theirs, hipIpcMemLazyEnablePeerAccess);
      if (e != hipSuccess) {
        (void)nos_ctx_comm_destroy(ctx);
        return fail(NOS_ERR_UNSUPPORTED, "device-memory mailbox: hipIpcOpenMemHandle(rank %d) failed: %s", k, hipGetErrorString(e));
      }
      ctx->ipc_peers[size_t(k)] = static_cast<double*>(p);
    }
    e = hipMalloc(reinterpret_cast<void**>(&ctx->d_peers), sizeof(double*) * size_t(n_ranks));
    if (e == hipSuccess) e = hipMemcpy(ctx->d_peers, ctx->ipc_peers.data(), sizeof(double*) * size_t(n_ranks), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)nos_ctx_comm_destroy(ctx);
      return fail(NOS_ERR_HIP, "device-memory mailbox: uploading the peer table failed: %s", hipGetErrorString(e));
    }
    // nobody may start exchanging (or leave and free its buffer) before every rank has opened every buffer
    hdr[129 + rank].store(2ull, std::memory_order_release);
    for (int k = 0; k < n_ranks; ++k)
      while (hdr[129 + k].load(std::memory_order_acquire) < 2ull) {
        if (now_ms() > deadline) {
          (void)nos_ctx_comm_destroy(ctx);
          return fail(NOS_ERR_HIP, "device-memory mailbox %s: rank %d did not finish attaching within %d ms", shm_name, k, kAttachTimeoutMs);
        }
        usleep(200);
      }
  }
  const nos::Mailbox mb = mailbox_of(ctx, slot);
  e = hipMalloc(reinterpret_cast<void**>(&ctx->d_mail), sizeof(nos::Mailbox));
  if (e == hipSuccess) e = hipMemcpy(ctx->d_mail, &mb, sizeof mb, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)nos_ctx_comm_destroy(ctx);
    return fail(NOS_ERR_HIP, "uploading the mailbox descriptor failed: %s", hipGetErrorString(e));
  }
  return NOS_OK;
}

}  // namespace

extern "C" {

int nos_ctx_comm_init_shm(nos_ctx* ctx, int n_ranks, int rank, const char* shm_name) {
  return comm_init_mailbox(ctx, n_ranks, rank, shm_name, false);
}

int nos_ctx_comm_init_shm_device(nos_ctx* ctx, int n_ranks, int rank, const char* shm_name) {
  return comm_init_mailbox(ctx, n_ranks, rank, shm_name, true);
}

int nos_comm_shm_unlink(const char* shm_name) {
  if (!shm_name) return fail(NOS_ERR_INVALID_ARGUMENT, "name is NULL");
  if (shm_unlink(shm_name) != 0 && errno != ENOENT) return fail(NOS_ERR_HIP, "shm_unlink(%s) failed: %s", shm_name, strerror(errno));
  return NOS_OK;
}

int nos_ctx_comm_allreduce(nos_ctx* ctx, double* values, int count) {
  nosd::CtxGuard guard_(ctx);  // one solve / accumulate / create at a time per context
  if (!ctx || !values || count < 1 || count > kMaxOut) return fail(NOS_ERR_INVALID_ARGUMENT, "bad allreduce arguments");
  if (ctx->comm == nullptr && ctx->shm_dev == nullptr) return fail(NOS_ERR_INVALID_ARGUMENT, "no communicator");
  DeviceSlot& slot = ctx->slots[0];
  NOS_HIP_CHECK(hipSetDevice(slot.device));
  NOS_HIP_CHECK(hipMemcpyAsync(slot.d_out, values, sizeof(double) * count, hipMemcpyHostToDevice, slot.stream));
  if (ctx->shm_dev != nullptr) {
    hipLaunchKernelGGL(nos::mailbox_allreduce_kernel, dim3(1), dim3(64), 0, slot.stream, mailbox_of(ctx, slot), slot.d_out, count);
    NOS_HIP_CHECK(hipGetLastError());
  } else {
    NOS_RCCL_CHECK(Rccl()->AllReduce(slot.d_out, slot.d_out, size_t(count), ncclDouble, ncclSum, ctx->comm, slot.stream));
  }
  NOS_HIP_CHECK(hipMemcpyAsync(values, slot.d_out, sizeof(double) * count, hipMemcpyDeviceToHost, slot.stream));
  NOS_HIP_CHECK(hipStreamSynchronize(slot.stream));
  return check_mailbox_error(ctx, slot);
}

}  // extern "C"
